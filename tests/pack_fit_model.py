"""The packing rule of the force pass's leftovers restated in Python, independently of csrc/pack_fit.hpp: the reference of
tests/test_pack_fit_cpu.py (pack for pack against the serial C++) and of tests/test_gpu_pack_fit.py (against the device)."""
WINDOW, LANES, GROUPS = 64, 64, 4


def best_fit_packs(r):
    """r: leftovers by computed cell.  Returns the packs in order, each a list of indices into r in placement order."""
    packs = []
    for w0 in range(0, len(r), WINDOW):
        items = sorted((i for i in range(w0, min(len(r), w0 + WINDOW)) if r[i] > 0), key=lambda i: (-int(r[i]), i))
        mine = []                                   # [used, cells] of this window's packs
        for i in items:
            fits = [b for b in mine if len(b[1]) < GROUPS and b[0] + int(r[i]) <= LANES]
            if fits:
                most = max(b[0] for b in fits)
                b = next(b for b in fits if b[0] == most)      # least room left, the lowest pack number first
            else:
                b = [0, []]
                mine.append(b)
            b[0] += int(r[i])
            b[1].append(i)
        packs += [b[1] for b in mine]
    return packs


def as_rows(packs):
    return [tuple(p) + (-1,) * (GROUPS - len(p)) for p in packs]
