"""The serial definition of psamd_update (include/psamd.h, "changing particles in place") in numpy: over a record array of
particles (P_DTYPE, one record per slot of the container) the entries are taken one after the other, in entry order.

By id an entry updates its slot when the id is valid, the slot is owned and live, and no earlier entry of the call has
updated it: the first occurrence wins.  By export order entry k belongs to the k-th live owned slot in ascending slot id.
SET writes the given bits; ADD is one np.float32 addition per component."""
import numpy as np

VEL, AGE, MASS, FERT, ADD, EXPORT_ORDER = 0x1, 0x2, 0x4, 0x8, 0x100, 0x200
UPDATED, NOT_LIVE, FOREIGN, INVALID, DUPLICATE = 0, 1, 2, 3, 4
RESULT_KEYS = ("done", "updated", "not_live", "foreign", "invalid", "duplicate")


def raw_copy(a):
    """(.copy() of a record array leaves its pad bytes undefined)"""
    return np.frombuffer(bytearray(a.tobytes()), a.dtype)


def result_of(outcome, n):
    return {"done": int(n), "updated": int((outcome == UPDATED).sum()), "not_live": int((outcome == NOT_LIVE).sum()),
            "foreign": int((outcome == FOREIGN).sum()), "invalid": int((outcome == INVALID).sum()),
            "duplicate": int((outcome == DUPLICATE).sum())}


def as_bits(p, name):
    """a float field seen as its words: assignments through it carry NaN payloads unchanged"""
    return p[name].view(np.uint32)


def apply(particles, num_cells, fields, ids=None, vel4=None, w=None, fert_age=None, n=None, owned=None):
    """(edited copy of the particles, outcome[n], result).  ids None: export order.  owned: bool per slot (None: all)."""
    bits = raw_copy(particles)
    cont = len(bits)
    owned = np.ones(cont, bool) if owned is None else owned
    live = owned & (bits["cell"] >= 0) & (bits["cell"] < num_cells)
    m = len(ids) if ids is not None else len(next(a for a in (vel4, w, fert_age) if a is not None))
    n = m if n is None else max(0, min(int(n), m))
    outcome = np.full(n, -1, np.int32)
    vel4 = None if vel4 is None else np.asarray(vel4, np.float32).reshape(-1, 4)
    # SET moves words, not values: uint32 views, so that no NaN is quietened on the way
    vb = None if vel4 is None else vel4.view(np.uint32)
    wb = None if w is None else np.asarray(w, np.float32).view(np.uint32)
    fb = None if fert_age is None else np.asarray(fert_age, np.float32).view(np.uint32)

    def write(slot, k):
        if fields & VEL:
            for c, name in enumerate(("vx", "vy", "vz")):
                if fields & ADD:
                    with np.errstate(all="ignore"):
                        bits[name][slot] = np.float32(bits[name][slot]) + np.float32(vel4[k, c])
                else:
                    as_bits(bits, name)[slot] = vb[k, c]
        if fields & AGE:
            as_bits(bits, "age")[slot] = vb[k, 3]
        if fields & MASS:
            as_bits(bits, "w")[slot] = wb[k]
        if fields & FERT:
            as_bits(bits, "fertility_age")[slot] = fb[k]
    if ids is None:
        slots = np.nonzero(live)[0]
        for k in range(n):
            if k < len(slots):
                write(int(slots[k]), k)
                outcome[k] = UPDATED
            else:
                outcome[k] = NOT_LIVE
    else:
        done = set()
        for k in range(n):
            sid = int(ids[k])
            if sid < 0 or sid >= cont:
                outcome[k] = INVALID
            elif not owned[sid]:
                outcome[k] = FOREIGN
            elif not live[sid]:
                outcome[k] = NOT_LIVE
            elif sid in done:
                outcome[k] = DUPLICATE
            else:
                write(sid, k)
                done.add(sid)
                outcome[k] = UPDATED
    return bits, outcome, result_of(outcome, n)
