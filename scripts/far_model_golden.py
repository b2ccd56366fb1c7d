"""What the far-field model computed when it was four files, on fixed small frames: tests/golden/far_model.json; and what the
quadrupole field computed when it had a file of its own: tests/golden/far_field_quadrupole.json.

    python scripts/far_model_golden.py --commit <a commit that has tests/far_{monopole,pyramid,quadrupole,potential}_model.py>
    python scripts/far_model_golden.py --quadrupole-field --commit <a commit that has tests/far_quad_field_model.py>

tests/far_model.py is the oracle of every GPU far-field test, so a silent change to it would weaken them all.  This script reads
the four model files it replaced out of git history (git show <commit>:tests/far_..._model.py, into a temporary directory),
evaluates quantities() with them and writes the result, naming the commit.  tests/test_far_model_cpu.py evaluates quantities()
with tests/far_model.py and compares: it reads the JSON only, never git.  The second mode does the same for field_quantities() --
phi64, phi32, accel64 and quad_sum64 of the quadrupole method -- with tests/far_quad_field_model.py and the tests/far_model.py it
stood on, as they were at the commit.  This script needs neither a GPU nor the library.

The frames: 4^3, 6^3 and 10^3 cells (one level; levels 6, 3; levels 10, 5, 3 with ragged parents), 8 bodies a cell in the mean,
unequal masses, every 13th body a kid, force_sign +1, -1, +1, one cell with 70 bodies more (phi32 takes a second chain there); 64
targets (eight of them in that cell) and 64 probe points.  Byte quantities are kept as SHA-256, the fp64 fields in full (base64
of little-endian float64), so that one that could not be kept bit for bit can still be held to a bound."""
import argparse
import base64
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = ("far_monopole_model", "far_pyramid_model", "far_quadrupole_model", "far_potential_model")
FRAMES = ((4, 1.0), (6, -1.0), (10, 1.0))
EPS2 = 0.2
# quad_pull takes u ** 5 and u ** 7, and a float64 power is not correctly rounded: its last bit may differ between hosts and
# numpy versions.  The two fields that hold it are compared at NEAR of the vector's norm -- five orders under the 1e-5 bar these
# values serve, far above the fp64 noise of sums of a few thousand terms; every other field and digest is compared bit for bit.
# So are the three fp64 fields of field_quantities(): quad_terms64 takes u ** 5 and u ** 3, quad_pull is in accel64.  (phi32 has no
# power and only correctly rounded operations: its digest is compared bit for bit.)
APPROXIMATE, NEAR = ("accel/quadrupole", "quad_accel"), 1e-10
FIELD_APPROXIMATE = ("phi64/quadrupole", "quad_sum64", "accel64/quadrupole")


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pack(a):
    return base64.b64encode(np.ascontiguousarray(a, "<f8").tobytes()).decode()


def unpack(s):
    return np.frombuffer(base64.b64decode(s), "<f8")


def frame_of(G, sign):
    rng = np.random.default_rng(500 + G)
    half = G * 2.5 * 0.9995
    inner = G // 2
    lo = np.array([(inner - G // 2) * 5.0, -(inner - G // 2) * 5.0 - 5.0, -(inner - G // 2) * 5.0 - 5.0])      # low corner of (inner, inner, inner)
    xyz = np.concatenate([rng.uniform(-half, half, (8 * G ** 3, 3)), lo + rng.uniform(0.05, 4.95, (70, 3))]).astype(np.float32)
    n = len(xyz)
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    kid = np.arange(n) % 13 == 0
    w_eff = np.where(kid, np.float32(0.0), np.float32(sign) * w).astype(np.float32)
    adults = np.nonzero(~kid)[0]
    targets = np.concatenate([adults[adults >= n - 70][:8], rng.choice(adults[adults < n - 70], 56, replace=False)])
    probes = rng.uniform(-half, half, (64, 3)).astype(np.float32)
    cells = {"corner": 0, "edge": inner * G * G, "face": (inner * G) * G + inner, "inner": (inner * G + inner) * G + inner}
    return dict(G=G, xyz=xyz, w_eff=w_eff, targets=targets, probes=probes, cells=cells)


def quantities(F):
    """{frame: {"sha256": {name: digest}, "f64": {name: packed array}}} of a model with far_model.py's interface"""
    out = {}
    for G, sign in FRAMES:
        fr = frame_of(G, sign)
        xyz, w, t, G = fr["xyz"], fr["w_eff"], fr["targets"], fr["G"]
        lists = F.lists_of(xyz, G)
        assert max(len(l) for l in lists) > 64
        cell = F.cells_of(xyz, G)
        pcell = F.cells_of(fr["probes"], G)
        digest, field = {}, {}
        for method in ("flat", "pyramid", "quadrupole"):
            moments = F.level_moments(lists, xyz, w, G, method)
            if method != "flat":
                digest["sums/" + method] = sha(F.level_sums(lists, xyz, w, G, method))
            digest["mom/" + method] = sha(moments[0])
            if moments[1] is not None:
                digest["cen/" + method] = sha(moments[1])
            digest["far_set/" + method] = sha([np.array(F.far_set(c, G, method), np.int64).reshape(-1, 2) for c in fr["cells"].values()])
            digest["coverage/" + method] = sha([F.coverage(c, G, method) for c in fr["cells"].values()])
            # (the moments are handed in or left to the default in turn, so that both ways are pinned)
            field["accel/" + method] = pack(F.accel(lists, xyz, w, G, EPS2, t, method, None if method == "flat" else moments))
            if method != "quadrupole":                               # (the quadrupole field: field_quantities())
                digest["phi32/" + method] = sha([F.phi32(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, method),
                                                 F.phi32(lists, xyz, w, G, EPS2, fr["probes"], pcell, np.full(64, -1), method, moments)])
                field["phi64/" + method] = pack(F.phi64(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, method, None if method == "pyramid" else moments))
                field["accel64/" + method] = pack(F.accel64(lists, xyz, w, G, EPS2, fr["probes"], pcell, method, moments))
        field["accel/stencil"] = pack(F.accel(lists, xyz, w, G, EPS2, t, "flat", far=False))
        field["phi64/stencil"] = pack(F.phi64(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, "flat", far=False))
        digest["phi32/stencil"] = sha([F.phi32(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, "flat", far=False)])
        field["quad_accel"] = pack(F.quad_accel(lists, xyz, w, G, EPS2, t))
        field["direct"] = pack(F.direct(xyz, w, EPS2, t))
        field["direct_phi"] = pack(F.direct_phi(xyz, w, EPS2, t))
        out["%d^3, sign %+d" % (G, sign)] = {"sha256": digest, "f64": field}
    return out


def field_quantities(F):
    """the same of the quadrupole method's field: phi64 at the 64 targets (own entry left out), quad_sum64 there, accel64 at the
    64 probes, and phi32 at both as one digest.  The moments are handed in or left to the default in turn over the frames"""
    out = {}
    for k, (G, sign) in enumerate(FRAMES):
        fr = frame_of(G, sign)
        xyz, w, t, G = fr["xyz"], fr["w_eff"], fr["targets"], fr["G"]
        lists = F.lists_of(xyz, G)
        cell = F.cells_of(xyz, G)
        pcell = F.cells_of(fr["probes"], G)
        moments = F.level_moments(lists, xyz, w, G, "quadrupole")
        given, other = (moments, None) if k % 2 == 0 else (None, moments)
        digest = {"phi32/quadrupole": sha([F.phi32(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, "quadrupole", given),
                                           F.phi32(lists, xyz, w, G, EPS2, fr["probes"], pcell, np.full(64, -1), "quadrupole", other)])}
        field = {"phi64/quadrupole": pack(F.phi64(lists, xyz, w, G, EPS2, xyz[t], cell[t], t, "quadrupole", given)),
                 "quad_sum64": pack(F.quad_sum64(lists, xyz, w, G, EPS2, xyz[t], cell[t], other)),
                 "accel64/quadrupole": pack(F.accel64(lists, xyz, w, G, EPS2, fr["probes"], pcell, "quadrupole", given))}
        out["%d^3, sign %+d" % (G, sign)] = {"sha256": digest, "f64": field}
    return out


def modules_at(commit, names):
    """tests/<name>.py as they were at `commit`, imported from a temporary directory"""
    tmp = tempfile.mkdtemp(prefix="far_models_")
    for name in names:
        text = subprocess.run(["git", "show", "%s:tests/%s.py" % (commit, name)], cwd=ROOT, check=True, capture_output=True, text=True).stdout
        with open(os.path.join(tmp, name + ".py"), "w") as fo:
            fo.write(text)
    sys.path.insert(0, tmp)
    return [importlib.import_module(name) for name in names]


def field_parents(commit):
    """far_model.py's interface for the quadrupole field on top of far_quad_field_model.py and far_model.py as they were at `commit`"""
    F, Q = modules_at(commit, ("far_model", "far_quad_field_model"))
    return types.SimpleNamespace(
        lists_of=F.lists_of, cells_of=F.cells_of, level_moments=F.level_moments, quad_sum64=Q.quad_sum64,
        phi32=lambda l, x, w, G, e, at, cell, own, method, moments=None: Q.phi32(l, x, w, G, e, at, cell, own, moments),
        phi64=lambda l, x, w, G, e, at, cell, own, method, moments=None: Q.phi64(l, x, w, G, e, at, cell, own, moments),
        accel64=lambda l, x, w, G, e, at, cell, method, moments=None: Q.accel64(l, x, w, G, e, at, cell, moments))


def parents(commit):
    """far_model.py's interface on top of the four files as they were at `commit`"""
    M, Y, Q, P = modules_at(commit, OLD)
    pyr = lambda method: method != "flat"

    def level_moments(lists, xyz, w, G, method):
        if method == "quadrupole":
            return Q.level_moments(lists, xyz, w, G)
        return P.level_moments(lists, xyz, w, G, pyr(method)), None

    def accel(lists, xyz, w, G, eps2, targets, method, moments=None, far=True):
        if not far or method == "flat":
            return M.accel(lists, xyz, w, G, eps2, targets, mom=None if moments is None else moments[0][0], far=far)
        if method == "pyramid":
            return Y.accel(lists, xyz, w, G, eps2, targets, levmom=None if moments is None else moments[0])
        return Q.accel(lists, xyz, w, G, eps2, targets, moments)

    return types.SimpleNamespace(
        lists_of=M.lists_of, cells_of=M.cells_of, level_moments=level_moments, accel=accel, quad_accel=Q.quad_accel,
        level_sums=lambda lists, xyz, w, G, method: (Q if method == "quadrupole" else Y).level_sums(lists, xyz, w, G),
        far_set=lambda c, G, method: P.far_set(c, G, pyr(method)),
        coverage=lambda c, G, method: Y.coverage(c, G, P.far_set(c, G, pyr(method))),
        phi32=lambda l, x, w, G, e, at, cell, own, method, moments=None, far=True:
            P.phi32(l, x, w, G, e, at, cell, own, moments and moments[0], pyr(method), far),
        phi64=lambda l, x, w, G, e, at, cell, own, method, moments=None, far=True:
            P.phi64(l, x, w, G, e, at, cell, own, moments and moments[0], pyr(method), far),
        accel64=lambda l, x, w, G, e, at, cell, method, moments: P.accel64(l, x, w, G, e, at, cell, moments[0], pyr(method)),
        direct=M.direct, direct_phi=P.direct_phi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose model files are evaluated")
    ap.add_argument("--quadrupole-field", action="store_true", help="the quadrupole field of far_quad_field_model.py, not the four model files")
    ap.add_argument("--out")
    a = ap.parse_args()
    commit = subprocess.run(["git", "rev-parse", a.commit], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    mode = "--quadrupole-field " if a.quadrupole_field else ""
    frames = field_quantities(field_parents(commit)) if a.quadrupole_field else quantities(parents(commit))
    res = {"commit": commit, "command": "python scripts/far_model_golden.py %s--commit %s" % (mode, commit), "numpy": np.__version__,
           "f64": "base64 of little-endian float64", "frames": frames}
    a.out = a.out or os.path.join(ROOT, "tests", "golden", "far_field_quadrupole.json" if a.quadrupole_field else "far_model.json")
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print("wrote %s: %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
