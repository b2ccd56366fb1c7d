"""The closed form psamd_remove's kernels use (particlesystem_amd/csrc/remove.hip), restated in numpy, and the serial
definition it must equal: pso_get_id_info, pso_reset_particle and pso_q_insert of the oracle, entry by entry.

Closed form: an entry removes its slot when the id is valid, the slot is owned and live before the call, and no earlier
entry names the slot (first occurrence: the minimum entry index per slot).  The k-th such entry of a queue record, in
entry order, is the record's k-th q_insert; with (front, rear, count) as they were before the call the queue takes the
first room = seg_size - count of them, at rloc + (first + k) % seg_size, first = 0 for an empty record and
rear - rloc + 1 otherwise, and drops the rest."""
import ctypes as C

import numpy as np

REMOVED, NOT_LIVE, FOREIGN, INVALID, DROPPED = 0, 1, 2, 3, 4
RESULT_KEYS = ("done", "removed", "not_live", "foreign", "invalid", "dropped")
ZERO_FIELDS = ("w", "age", "fertility_age", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az")


def record_of_slot(d, ids):
    """get_id_info + get_info_rloc of valid ids (d: the oracle's Derived or psamd's Sizes): the QUEUE_INFO record"""
    seg_size, seg_size_t, seg_count = np.array(d.seg_size[:]), np.array(d.seg_size_t[:]), np.array(d.seg_count[:])
    slot_base = np.concatenate([[0], np.cumsum(seg_size)])
    info_base = np.concatenate([[0], np.cumsum(seg_count)])
    k = np.searchsorted(slot_base[1:], ids, side="right")
    return info_base[k] + (ids - slot_base[k]) // seg_size_t[k]


def result_of(outcome, n):
    return {"done": int(n), "removed": int(((outcome == REMOVED) | (outcome == DROPPED)).sum()),
            "not_live": int((outcome == NOT_LIVE).sum()), "foreign": int((outcome == FOREIGN).sum()),
            "invalid": int((outcome == INVALID).sum()), "dropped": int((outcome == DROPPED).sum())}


def closed_form(d, num_cells, particles, qinfo, queue, ids, owned=None):
    """The kernels' algorithm on copies of the three buffers: (particles, qinfo, queue, outcome, result).  owned: bool per
    slot (None: every slot)."""
    # (raw copies: .copy() of a record array leaves its pad bytes undefined)
    p, qi, q = (np.frombuffer(bytearray(a.tobytes()), a.dtype) for a in (particles, qinfo, queue))
    ids = np.asarray(ids, np.int64)
    n, cont = len(ids), len(p)
    idx = np.arange(n)
    outcome = np.full(n, -1, np.int32)
    valid = (ids >= 0) & (ids < cont)
    outcome[~valid] = INVALID
    safe = np.where(valid, ids, 0)
    mine = valid & (np.ones(cont, bool) if owned is None else owned)[safe]
    outcome[valid & ~mine] = FOREIGN
    live = mine & (p["cell"][safe] >= 0) & (p["cell"][safe] < num_cells)
    # k_remove_claim: the lowest entry index per slot
    claim = np.full(cont, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(claim, ids[live], idx[live])
    win = live & (claim[safe] == idx)
    outcome[mine & ~win] = NOT_LIVE
    # k_remove_rank + the prefix of k_remove_commit: the stable rank of a winner among the winners of its record
    w = idx[win]
    rec = record_of_slot(d, ids[w])
    order = np.argsort(rec, kind="stable")
    srec = rec[order]
    start = np.searchsorted(srec, srec, side="left")
    k = np.empty(len(w), np.int64)
    k[order] = np.arange(len(w)) - start
    # the insert rule of every record, from the record before the call
    count, rear, rloc, seg = (qi[f].astype(np.int64) for f in ("count", "rear", "rloc", "seg_size"))
    room = seg - count
    first = np.where(count == 0, 0, (rear - rloc + 1) % seg)
    taken = k < room[rec]
    q[rloc[rec[taken]] + (first[rec[taken]] + k[taken]) % seg[rec[taken]]] = ids[w][taken]
    outcome[w] = np.where(taken, REMOVED, DROPPED)
    # the commit
    R = np.bincount(rec, minlength=len(qi))
    A = np.minimum(R, room)
    ch = A > 0
    qi["front"][ch & (count == 0)] = rloc[ch & (count == 0)]
    qi["rear"][ch] = (rloc + (first + A - 1) % seg)[ch]
    qi["count"][ch] = (count + A)[ch]
    # the reset slots
    s = ids[w]
    for f in ("cell", "chunk", "seg_type", "seg_tid"):
        p[f][s] = -1
    p["seg_fault"][s] = 0
    p["is_parent"][s] = 0
    for f in ZERO_FIELDS:
        p[f][s] = 0.0
    return p, qi, q, outcome, result_of(outcome, n)


def serial(o, ids, owned=None):
    """The definition, on the oracle system `o` in place: entry by entry get_id_info, reset_particle, q_insert.  Returns
    (outcome, result).  owned: bool per slot (None: every slot)."""
    L, d = o.L, o.d
    p, qi, q = o.particles, o.queue_info, o.queue
    seg = (C.c_int * 2)()
    outcome = np.full(len(ids), -1, np.int32)
    for i, sid in enumerate(int(x) for x in ids):
        if sid < 0 or sid >= d.container_size:
            outcome[i] = INVALID
        elif owned is not None and not owned[sid]:
            outcome[i] = FOREIGN
        elif not 0 <= p["cell"][sid] < d.num_cells:
            outcome[i] = NOT_LIVE
        else:
            L.pso_get_id_info(C.byref(d), sid, seg)
            rec = L.pso_get_info_rloc(C.byref(d), seg[0], seg[1])
            before = int(qi["count"][rec])
            L.pso_reset_particle(p.ctypes.data + 72 * sid)
            L.pso_q_insert(qi.ctypes.data, q.ctypes.data, C.byref(d), seg[0], seg[1], sid)
            outcome[i] = REMOVED if int(qi["count"][rec]) == before + 1 else DROPPED
    return outcome, result_of(outcome, len(ids))
