"""particlesystem_amd -- MI355X-native step of abraj/particleSystem behind a C ABI.

This package is a thin ctypes mirror of ``include/psamd.h`` (the drop-in boundary):
the product is ``libpsamd.so`` (hand-written HIP kernels for gfx950 + a C++ host
context).  The Python layer exists for tests, the benchmark and torch.distributed
plumbing; it never computes anything itself and there is no CPU fallback: if the
library is not built, or no HIP device is visible, calls fail loudly.

Stage names follow the reference's task list (particleSystem.cpp:2269-2282):
``init_iframe`` (task 3), ``build_grid`` (task 8), ``calc_forces`` (task 6),
``fill_particles`` (task 5).
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import build as _build
# psamd_slab_msg_download / _upload `which`: slab.py's message slots, under the names of the C header
from .slab import (HALO_OUT as MSG_HALO_OUT, HALO_IN as MSG_HALO_IN, FORCE_OUT as MSG_FORCE_OUT, FORCE_IN as MSG_FORCE_IN,
                   XFER_OUT as MSG_XFER_OUT, XFER_IN as MSG_XFER_IN, STATUS_OUT as MSG_STATUS_OUT, STATUS_IN as MSG_STATUS_IN,
                   ALLG_OUT as MSG_ALLG_OUT, ALLG_IN as MSG_ALLG_IN, XFER2_OUT as MSG_XFER2_OUT, XFER2_IN as MSG_XFER2_IN,
                   FAR_OUT as MSG_FAR_OUT, FAR_IN as MSG_FAR_IN)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSAMD_LIB") or os.path.join(HERE, "libpsamd.so")   # PSAMD_LIB: another build, for A/B measurements

ABI_VERSION = 8         # the struct layouts below are include/psamd.h's at this PSAMD_ABI_VERSION
MAX_RANKS = 64
FLAG_EXPLOSIONS = 0x1
FLAG_FAST_MATH = 0x2
FLAG_ALL_PAIRS = 0x4
FLAG_EULER = 0x8
FLAG_FAR_MONOPOLE = 0x10
FLAG_FAR_PYRAMID = 0x20
FLAG_FAR_QUADRUPOLE = 0x40
FLAG_FAR_SLAB = 0x80
NUM_TIMERS = 9
TIMER_NAMES = ("hist", "scan", "scatter", "sort_cells", "pairs", "apply", "lifecycle", "init_iframe", "collide")

# numpy images of the reference's records (common.h:94-145)
P_DTYPE = np.dtype({
    "names": ["id", "cell", "chunk", "seg_type", "seg_tid", "seg_fault", "is_parent",
              "w", "age", "fertility_age", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az"],
    "formats": ["<i4"] * 5 + ["u1", "u1"] + ["<f4"] * 12,
    "offsets": [0, 4, 8, 12, 16, 20, 21] + list(range(24, 72, 4)),
    "itemsize": 72,
})
T_DTYPE = np.dtype([("id", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4"), ("age", "<f4")])
Q_DTYPE = np.dtype([("front", "<i4"), ("rear", "<i4"), ("count", "<i4"), ("lock", "<i4"),
                    ("rloc", "<i4"), ("seg_size", "<i4")])


class Config(C.Structure):
    _fields_ = [("max_particles_num", C.c_int32), ("x_factor", C.c_int32),
                ("chunk_factor", C.c_int32), ("chunk_dim", C.c_int32),
                ("cell_size", C.c_double), ("eps2", C.c_double), ("collision_radius", C.c_double),
                ("particle_weight", C.c_double), ("dt", C.c_double), ("max_v", C.c_double),
                ("explosion_speed", C.c_double), ("life_steps", C.c_double),
                ("device", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("rank", C.c_int32), ("world", C.c_int32),
                ("halo_cap_cell", C.c_int32), ("xfer_cap", C.c_int32),
                ("cuts", C.c_int32 * (MAX_RANKS + 1)),
                ("drag", C.c_double), ("force_sign", C.c_double),
                ("xfer_cap_max", C.c_int32), ("reserved0", C.c_int32)]


class Sizes(C.Structure):
    _fields_ = [("grid_dim", C.c_int32), ("num_cells", C.c_int32), ("num_chunks", C.c_int32),
                ("cells_per_chunk", C.c_int32), ("max_per_cell", C.c_int32), ("max_per_chunk", C.c_int32),
                ("container_size", C.c_int32), ("queue_info_size", C.c_int32),
                ("n_chunkgrid", C.c_int64), ("n_cellgrid", C.c_int64), ("n_pkgdistrib", C.c_int32),
                ("seg_count", C.c_int32 * 4), ("seg_size_t", C.c_int32 * 4), ("seg_size", C.c_int32 * 4)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in
                ("deaths_age", "deaths_collision", "survives", "integrated", "relocations",
                 "relocations_lost", "births", "births_failed", "cell_overflow_kills", "steps",
                 "particles_processed", "max_ops_one_queue")]


class DeviceView(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("pos4", "vel4", "acc4", "cell", "pflags", "sorted_id", "snap_soa", "force4", "cell_start")] + \
               [("container_size", C.c_int64), ("num_cells", C.c_int32), ("live", C.c_int32),
                ("sorted_cap", C.c_int64), ("stream", C.c_void_p)]


class SlabPlan(C.Structure):
    """psamd_slab_plan: which cell layers, slots and queue records one rank holds."""
    _fields_ = [(n, C.c_int32) for n in
                ("world", "rank", "grid_dim", "cut_lo", "cut_hi", "state_lo", "state_hi", "below_lo", "below_hi",
                 "above_lo", "above_hi", "lentin_lo", "lentin_hi", "lentout_lo", "lentout_hi",
                 "send_up_lo", "send_up_hi", "send_down_lo", "send_down_hi")] + \
               [("slot_lo", C.c_int32 * 4), ("slot_hi", C.c_int32 * 4), ("rec_lo", C.c_int32 * 4), ("rec_hi", C.c_int32 * 4),
                ("up_rank", C.c_int32), ("down_rank", C.c_int32)]


class SlabBuffers(C.Structure):
    _fields_ = [("halo_out", C.c_void_p * 2), ("halo_in", C.c_void_p * 2),
                ("halo_out_bytes", C.c_int64 * 2), ("halo_in_bytes", C.c_int64 * 2),
                ("force_out", C.c_void_p), ("force_in", C.c_void_p),
                ("force_out_bytes", C.c_int64), ("force_in_bytes", C.c_int64),
                ("xfer_out", C.c_void_p * 2), ("xfer_in", C.c_void_p * 2), ("xfer_bytes", C.c_int64),
                ("status_out", C.c_void_p), ("status_in", C.c_void_p), ("status_bytes", C.c_int64),
                ("allg_out", C.c_void_p), ("allg_in", C.c_void_p), ("allg_bytes", C.c_int64),
                ("xfer2_out", C.c_void_p * 2), ("xfer2_in", C.c_void_p * 2), ("xfer2_bytes", C.c_int64),
                ("far_out", C.c_void_p), ("far_in", C.c_void_p), ("far_bytes", C.c_int64), ("xfer_bytes_max", C.c_int64)]


# psamd_export_live / psamd_download_live: the fields (bits of `fields`)
EXPORT_POS, EXPORT_VEL, EXPORT_ACC, EXPORT_ID, EXPORT_CELL = 0x1, 0x2, 0x4, 0x8, 0x10
EXPORT_ALL = 0x1F
_EXPORT_FIELDS = (("pos4", EXPORT_POS, 4, np.float32), ("vel4", EXPORT_VEL, 4, np.float32), ("acc4", EXPORT_ACC, 4, np.float32),
                  ("id", EXPORT_ID, 1, np.int32), ("cell", EXPORT_CELL, 1, np.int32))


class _Record(C.Structure):
    """A result record of the C header.  to_dict: every field but the reserved ones, an integer field as int, a double as
    float, an array of doubles as a float64 array."""

    def to_dict(self):
        out = {}
        for n, t in self._fields_:
            if not n.startswith("reserved"):
                v = getattr(self, n)
                out[n] = np.array(v[:], np.float64) if hasattr(t, "_length_") else float(v) if t is C.c_double else int(v)
        return out

    @classmethod
    def from_device(cls, t):
        """the record a service left in a uint8 torch device tensor of sizeof(cls) bytes"""
        return cls.from_buffer_copy(t.cpu().numpy().tobytes())


class LiveStats(_Record):
    """psamd_live_stats: count and fp64 statistics of the live particles."""
    _fields_ = [("live", C.c_int64), ("nonfinite", C.c_int64), ("mass", C.c_double), ("momentum", C.c_double * 3),
                ("kinetic", C.c_double), ("mass_moment", C.c_double * 3), ("lo", C.c_double * 3), ("hi", C.c_double * 3),
                ("age_min", C.c_double), ("age_max", C.c_double), ("age_sum", C.c_double)]


class Export(C.Structure):
    """psamd_export: what psamd_export_live writes and where (device pointers)."""
    _fields_ = [("fields", C.c_uint32), ("reserved", C.c_int32),
                ("pos4", C.c_void_p), ("vel4", C.c_void_p), ("acc4", C.c_void_p), ("id", C.c_void_p), ("cell", C.c_void_p),
                ("capacity", C.c_int64), ("count_dev", C.c_void_p), ("stats_dev", C.c_void_p)]


class InjectResult(_Record):
    """psamd_inject_result: what psamd_inject did (done, placed, status)."""
    _fields_ = [("done", C.c_int64), ("placed", C.c_int64), ("status", C.c_int32), ("reserved", C.c_int32)]


class Inject(C.Structure):
    """psamd_inject_spec: what psamd_inject reads and where it writes (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_int32), ("pos4", C.c_void_p), ("vel4", C.c_void_p),
                ("fert_age", C.c_void_p), ("max_count", C.c_int64), ("count_dev", C.c_void_p), ("ids_dev", C.c_void_p),
                ("result_dev", C.c_void_p)]


def _merge_counts(results, cls):
    """every field of the ranks' records (dicts) added up"""
    results = list(results)
    return {n: sum(int(r[n]) for r in results) for n, _ in cls._fields_}


# psamd_remove: the flags, and the outcome codes of the entries of a removal by id
REMOVE_BOX, REMOVE_OUTSIDE = 0x1, 0x2
REMOVED, REMOVE_NOT_LIVE, REMOVE_FOREIGN, REMOVE_INVALID, REMOVE_DROPPED = 0, 1, 2, 3, 4


class RemoveResult(_Record):
    """psamd_remove_result: what psamd_remove did."""
    _fields_ = [(n, C.c_int64) for n in ("done", "removed", "not_live", "foreign", "invalid", "dropped")]


class Remove(C.Structure):
    """psamd_remove_spec: what psamd_remove reads and where it writes (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_int32), ("ids", C.c_void_p), ("max_count", C.c_int64),
                ("count_dev", C.c_void_p), ("outcome_dev", C.c_void_p), ("lo", C.c_float * 3), ("hi", C.c_float * 3),
                ("result_dev", C.c_void_p)]


def merge_remove(results):
    """The result of a removal on a system from its ranks' (dicts of remove() / remove_result()): every count adds (by id
    each rank is given all entries, so `done` adds up to world * n)."""
    return _merge_counts(results, RemoveResult)


# psamd_update: the words an entry carries, the two modifiers, and the outcome codes of the entries
UPDATE_VEL, UPDATE_AGE, UPDATE_MASS, UPDATE_FERT = 0x1, 0x2, 0x4, 0x8
UPDATE_ADD, UPDATE_EXPORT_ORDER = 0x100, 0x200
UPDATED, UPDATE_NOT_LIVE, UPDATE_FOREIGN, UPDATE_INVALID, UPDATE_DUPLICATE = 0, 1, 2, 3, 4


class UpdateResult(_Record):
    """psamd_update_result: what psamd_update did."""
    _fields_ = [(n, C.c_int64) for n in ("done", "updated", "not_live", "foreign", "invalid", "duplicate")]


class Update(C.Structure):
    """psamd_update_spec: what psamd_update reads and where it writes (device pointers)."""
    _fields_ = [("fields", C.c_uint32), ("reserved", C.c_int32), ("ids", C.c_void_p), ("vel4", C.c_void_p), ("w", C.c_void_p),
                ("fert_age", C.c_void_p), ("max_count", C.c_int64), ("count_dev", C.c_void_p), ("outcome_dev", C.c_void_p),
                ("result_dev", C.c_void_p)]


def merge_update(results):
    """The result of an update by id on a system from its ranks' (dicts of update() / update_result()): every count adds
    (each rank is given all entries, so `done` adds up to world * n)."""
    return _merge_counts(results, UpdateResult)


class PotentialResult(_Record):
    """psamd_potential_result: counts, the potential energy U and the extrema of phi."""
    _fields_ = [("listed", C.c_int64), ("nonfinite", C.c_int64), ("potential", C.c_double),
                ("phi_min", C.c_double), ("phi_max", C.c_double)]


POTENTIAL_FAR = 0x1     # psamd_potential_spec.flags: the stencil and the far bodies of a far-monopole context's force model
POTENTIAL_QUADRUPOLE = 0x2      # a modifier of POTENTIAL_FAR on a quadrupole context: the far bodies' quadrupole terms too


class Potential(C.Structure):
    """psamd_potential_spec: what psamd_potential writes and where (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_int32), ("phi", C.c_void_p), ("capacity", C.c_int64),
                ("result_dev", C.c_void_p)]


def merge_potential(results):
    """The potential of a system from its ranks' (dicts of potential() / download_potential()): counts and U add, in
    rank order; the extrema take the minimum and the maximum.  (No "phi": the ranks' arrays pair with their own exports.)"""
    results = list(results)
    return {"listed": sum(int(r["listed"]) for r in results), "nonfinite": sum(int(r["nonfinite"]) for r in results),
            "potential": float(sum(float(r["potential"]) for r in results)),
            "phi_min": float(min(float(r["phi_min"]) for r in results)), "phi_max": float(max(float(r["phi_max"]) for r in results))}


# psamd_probe: the field bits, and the outcome codes of the entries
PROBE_ACC, PROBE_PHI = 0x1, 0x2
PROBE_FAR = 0x4         # a modifier beside ACC / PHI on a far-monopole context: the far bodies of its force model too
PROBE_QUADRUPOLE = 0x8  # a modifier of PROBE_FAR on a quadrupole context: the far bodies' quadrupole terms too
PROBE_SERVED, PROBE_OUTSIDE, PROBE_FOREIGN = 0, 1, 2


class ProbeResult(_Record):
    """psamd_probe_result: what psamd_probe did."""
    _fields_ = [(n, C.c_int64) for n in ("done", "served", "outside", "foreign", "nonfinite")]


class ProbeSpec(C.Structure):
    """psamd_probe_spec: what psamd_probe reads and where it writes (device pointers)."""
    _fields_ = [("fields", C.c_uint32), ("reserved", C.c_int32), ("pos4", C.c_void_p), ("max_count", C.c_int64),
                ("count_dev", C.c_void_p), ("out4", C.c_void_p), ("outcome_dev", C.c_void_p), ("result_dev", C.c_void_p)]


def merge_probe(results):
    """The probes of a slab world from its ranks' (dicts of probe(outcome=True), every rank given all entries): each
    entry's out4 from the rank whose outcome is 0 (the quiet NaN where no rank serves it), `served` and `nonfinite`
    add, `outside` and `done` are any one rank's (every rank sees the same entries), `foreign` is what no rank served
    inside the box: 0.  out4 / outcome may be torch tensors or numpy arrays; the merged ones are numpy arrays."""
    results = list(results)

    def host(a):
        return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    outs = [host(r["out4"]).astype(np.float32, copy=False) for r in results]
    codes = [host(r["outcome"]).astype(np.int32, copy=False) for r in results]
    out4 = np.full(outs[0].shape, np.float32(np.nan), np.float32).view(np.uint32)
    out4[...] = 0x7fc00000
    outcome = np.where(codes[0] == PROBE_OUTSIDE, PROBE_OUTSIDE, PROBE_FOREIGN).astype(np.int32)
    for o, c in zip(outs, codes):
        sel = c == PROBE_SERVED
        out4[sel] = o.view(np.uint32)[sel]
        outcome[sel] = PROBE_SERVED
    served = sum(int(r["served"]) for r in results)
    return {"out4": out4.view(np.float32), "outcome": outcome, "done": int(results[0]["done"]), "served": served,
            "outside": int(results[0]["outside"]), "foreign": int(results[0]["done"]) - int(results[0]["outside"]) - served,
            "nonfinite": sum(int(r["nonfinite"]) for r in results)}


class DepositResult(_Record):
    """psamd_deposit_result: what psamd_deposit wrote and of which bodies."""
    _fields_ = [("voxels", C.c_int64), ("bodies", C.c_int64), ("skipped", C.c_int64), ("mass", C.c_double), ("vmax", C.c_double)]


class DepositSpec(C.Structure):
    """psamd_deposit_spec: what psamd_deposit writes and where (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("refine", C.c_int32), ("out", C.c_void_p), ("capacity", C.c_int64), ("result_dev", C.c_void_p)]


def merge_deposit(results):
    """The deposit of a system from its ranks' (dicts of deposit(result=True)[1] / download_deposit()[1]): voxels, bodies,
    skipped and mass add, in rank order; vmax takes the maximum.  (The arrays: every voxel is written by one rank, into the
    full lattice; the host forms are +0 elsewhere and add.)"""
    results = list(results)
    out = {n: sum(int(r[n]) for r in results) for n in ("voxels", "bodies", "skipped")}
    out["mass"] = float(sum(float(r["mass"]) for r in results))
    out["vmax"] = float(max(float(r["vmax"]) for r in results))
    return out


# psamd_sample: the flags, and the outcome codes of the entries
SAMPLE_VEC4, SAMPLE_EXPORT_ORDER = 0x1, 0x2
SAMPLE_SERVED, SAMPLE_OUTSIDE = 0, 1


class SampleResult(_Record):
    """psamd_sample_result: what psamd_sample did."""
    _fields_ = [(n, C.c_int64) for n in ("done", "served", "outside", "nonfinite")]


class SampleSpec(C.Structure):
    """psamd_sample_spec: what psamd_sample reads and where it writes (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("refine", C.c_int32), ("field", C.c_void_p), ("capacity", C.c_int64), ("pos4", C.c_void_p),
                ("max_count", C.c_int64), ("count_dev", C.c_void_p), ("out", C.c_void_p), ("scale", C.c_float), ("reserved", C.c_int32),
                ("outcome_dev", C.c_void_p), ("result_dev", C.c_void_p)]


def merge_sample(results):
    """The sample of a slab world from its ranks' records (dicts of sample(result=True) / sample_result()): every count adds
    (by export order each rank serves its own particles; given the same points, `done` adds up to world * n)."""
    return _merge_counts(results, SampleResult)


NEIGHBOURS_INDEX = 0x1  # psamd_neighbours_spec.flags: a neighbour is named by its export index, not by its global slot id


class NeighboursResult(_Record):
    """psamd_neighbours_result: the queries, the directed pairs, the list entries wanted, the largest count, the smallest d2."""
    _fields_ = [("listed", C.c_int64), ("pairs", C.c_int64), ("wanted", C.c_int64), ("max_count", C.c_int32),
                ("reserved", C.c_int32), ("d2_min", C.c_double)]


class NeighboursSpec(C.Structure):
    """psamd_neighbours_spec: what psamd_neighbours writes and where (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("radius", C.c_float), ("count", C.c_void_p), ("nearest", C.c_void_p),
                ("nearest_d2", C.c_void_p), ("offsets", C.c_void_p), ("capacity", C.c_int64), ("list", C.c_void_p),
                ("list_capacity", C.c_int64), ("result_dev", C.c_void_p)]


def merge_neighbours(results):
    """The record of a slab world from its ranks' (dicts of neighbours() / neighbours_result()): the counts add, max_count
    and d2_min take the maximum and the minimum.  (The arrays pair with the ranks' own exports.)"""
    results = list(results)
    out = {n: sum(int(r[n]) for r in results) for n in ("listed", "pairs", "wanted")}
    out["max_count"] = max(int(r["max_count"]) for r in results)
    out["d2_min"] = float(min(float(r["d2_min"]) for r in results))
    return out


GROUPS_INDEX = 0x1  # psamd_groups_spec.flags: group_first names a particle by its export index, not by its global slot id


class GroupsResult(_Record):
    """psamd_groups_result: the members, the groups, the undirected links, the groups of one, the largest group, the unions
    that hit the step cap (0 on correct code)."""
    _fields_ = [("members", C.c_int64), ("groups", C.c_int64), ("links", C.c_int64), ("singles", C.c_int64),
                ("largest", C.c_int32), ("unfinished", C.c_int32)]


class GroupsSpec(C.Structure):
    """psamd_groups_spec: what psamd_groups writes and where (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("radius", C.c_float), ("group", C.c_void_p), ("capacity", C.c_int64),
                ("group_first", C.c_void_p), ("group_size", C.c_void_p), ("group_capacity", C.c_int64), ("result_dev", C.c_void_p)]


KNN_INDEX = 0x1  # psamd_knn_spec.flags: a neighbour is named by its export index, not by its global slot id
KNN_MAX_K = 32   # the largest k psamd_knn serves


class KnnResult(_Record):
    """psamd_knn_result: the queries, the sum of min(count, k), the queries with count >= k, k, the smallest and the largest
    d2 of a k-th neighbour over the full queries (+inf / -inf: none)."""
    _fields_ = [("listed", C.c_int64), ("found", C.c_int64), ("full", C.c_int64), ("k", C.c_int32), ("reserved", C.c_int32),
                ("dk2_min", C.c_double), ("dk2_max", C.c_double)]


class KnnSpec(C.Structure):
    """psamd_knn_spec: what psamd_knn writes and where (device pointers)."""
    _fields_ = [("flags", C.c_uint32), ("radius", C.c_float), ("k", C.c_int32), ("reserved", C.c_int32), ("found", C.c_void_p),
                ("who", C.c_void_p), ("d2", C.c_void_p), ("capacity", C.c_int64), ("result_dev", C.c_void_p)]


def merge_knn(results):
    """The record of a slab world from its ranks' (dicts of knn() / knn_result()): the counts add, dk2_min and dk2_max take
    the minimum and the maximum.  (The rows pair with the ranks' own exports.)"""
    results = list(results)
    out = {n: sum(int(r[n]) for r in results) for n in ("listed", "found", "full")}
    out["k"] = int(results[0]["k"])
    out["dk2_min"] = float(min(float(r["dk2_min"]) for r in results))
    out["dk2_max"] = float(max(float(r["dk2_max"]) for r in results))
    return out


def merge_live_stats(stats):
    """The statistics of a system from its ranks' (dicts of live_stats() / export_live()["stats"]): counts and sums
    add, in rank order; the box and the ages take the minima and maxima."""
    stats = list(stats)
    out = {}
    for n, _ in LiveStats._fields_:
        vals = [np.asarray(s[n], np.float64) for s in stats]
        if n in ("lo", "age_min"):
            v = np.minimum.reduce(vals)
        elif n in ("hi", "age_max"):
            v = np.maximum.reduce(vals)
        else:
            v = vals[0]
            for x in vals[1:]:
                v = v + x
        out[n] = int(v) if n in ("live", "nonfinite") else (v if v.ndim else float(v))
    return out


class PsamdError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("psamd status %d: %s" % (status, message))
        self.status = status


# every entry point include/psamd.h declares: (name, restype, argtypes)
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
ABI = [
    ("psamd_abi_version", C.c_int, []),
    ("psamd_status_string", C.c_char_p, [C.c_int]),
    ("psamd_default_config", C.c_int, [C.POINTER(Config)]),
    ("psamd_create", C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    ("psamd_destroy", C.c_int, [_vp]),
    ("psamd_last_error", C.c_char_p, [_vp]),
    ("psamd_get_sizes", C.c_int, [_vp, C.POINTER(Sizes)]),
    ("psamd_describe", C.c_int, [C.POINTER(Config), C.POINTER(Sizes), _vp, _vp, _vp, _vp]),
    ("psamd_get_config", C.c_int, [_vp, C.POINTER(Config)]),
    ("psamd_fill_particles", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("psamd_uniform_cloud", C.c_int, [_vp, _i64, C.c_uint32, _vp]),
    ("psamd_upload_particles", C.c_int, [_vp, _vp, _i64, _i64]),
    ("psamd_download_particles", C.c_int, [_vp, _vp, _i64, _i64]),
    ("psamd_download_tdata", C.c_int, [_vp, _vp, _i64, _i64]),
    ("psamd_upload_queues", C.c_int, [_vp, _vp, _vp]),
    ("psamd_download_queues", C.c_int, [_vp, _vp, _vp]),
    ("psamd_download_cellgrid", C.c_int, [_vp, _vp]),
    ("psamd_download_chunkgrid", C.c_int, [_vp, _vp]),
    ("psamd_download_force_counts", C.c_int, [_vp, _vp]),
    ("psamd_download_cell_moments", C.c_int, [_vp, _vp]),
    ("psamd_download_level_moments", C.c_int, [_vp, C.c_int32, _vp]),
    ("psamd_download_level_quadrupoles", C.c_int, [_vp, C.c_int32, _vp]),
    ("psamd_far_levels", C.c_int, [C.POINTER(Config), _ip, _ip]),
    ("psamd_get_pkgdistrib", C.c_int, [_vp, _vp]),
    ("psamd_get_cell_table", C.c_int, [_vp, _vp]),
    ("psamd_get_gridmax", C.c_int, [_vp, _ip]),
    ("psamd_init_iframe", C.c_int, [_vp]),
    ("psamd_build_grid", C.c_int, [_vp]),
    ("psamd_calc_forces", C.c_int, [_vp]),
    ("psamd_calc_forces_pairs", C.c_int, [_vp]),
    ("psamd_calc_forces_apply", C.c_int, [_vp]),
    ("psamd_step", C.c_int, [_vp, _i32]),
    ("psamd_synchronize", C.c_int, [_vp]),
    ("psamd_download_force4", C.c_int, [_vp, _vp, _i64, _i64]),
    ("psamd_snapshot_save", C.c_int, [_vp]),
    ("psamd_snapshot_restore", C.c_int, [_vp]),
    ("psamd_set_stream", C.c_int, [_vp, _vp]),
    ("psamd_get_stream", C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    ("psamd_slab_plan_describe", C.c_int, [C.POINTER(Config), C.POINTER(SlabPlan)]),
    ("psamd_get_slab_plan", C.c_int, [_vp, C.POINTER(SlabPlan)]),
    ("psamd_slab_buffers_get", C.c_int, [_vp, C.POINTER(SlabBuffers)]),
    ("psamd_slab_build", C.c_int, [_vp]),
    ("psamd_slab_pairs_interior", C.c_int, [_vp]),
    ("psamd_slab_pairs", C.c_int, [_vp]),
    ("psamd_slab_apply", C.c_int, [_vp]),
    ("psamd_slab_finish", C.c_int, [_vp]),
    ("psamd_slab_msg_download", C.c_int, [_vp, C.c_int, _vp, _i64]),
    ("psamd_slab_msg_upload", C.c_int, [_vp, C.c_int, _vp, _i64]),
    ("psamd_get_counters", C.c_int, [_vp, C.POINTER(Counters)]),
    ("psamd_live_count", C.c_int, [_vp, C.POINTER(_i64)]),
    ("psamd_device_view_get", C.c_int, [_vp, C.POINTER(DeviceView)]),
    ("psamd_debug_wave_trace", C.c_int, [_vp, _vp, _i64]),
    ("psamd_debug_packs", C.c_int, [_vp, _vp, _i64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]),
    ("psamd_selftest_math", C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("psamd_set_graphs", C.c_int, [_vp, C.c_int]),
    ("psamd_get_graph_stats", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    ("psamd_set_wait_policy", C.c_int, [_vp, C.c_int]),
    ("psamd_set_timing", C.c_int, [_vp, C.c_int]),
    ("psamd_set_timing_period", C.c_int, [_vp, C.c_int]),
    ("psamd_get_timing", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(_i64)]),
    ("psamd_get_timing_stats", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i64)]),
    ("psamd_set_run_ahead", C.c_int, [_vp, C.c_int]),
    ("psamd_set_tdata_mirror", C.c_int, [_vp, C.c_int]),
    ("psamd_export_live", C.c_int, [_vp, C.POINTER(Export)]),
    ("psamd_download_live", C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    ("psamd_live_stats_get", C.c_int, [_vp, C.POINTER(LiveStats)]),
    ("psamd_inject", C.c_int, [_vp, C.POINTER(Inject)]),
    ("psamd_inject_result_get", C.c_int, [_vp, C.POINTER(InjectResult)]),
    ("psamd_remove", C.c_int, [_vp, C.POINTER(Remove)]),
    ("psamd_remove_result_get", C.c_int, [_vp, C.POINTER(RemoveResult)]),
    ("psamd_update", C.c_int, [_vp, C.POINTER(Update)]),
    ("psamd_update_result_get", C.c_int, [_vp, C.POINTER(UpdateResult)]),
    ("psamd_potential", C.c_int, [_vp, C.POINTER(Potential)]),
    ("psamd_potential_result_get", C.c_int, [_vp, C.POINTER(PotentialResult)]),
    ("psamd_download_potential", C.c_int, [_vp, _vp, _i64, C.POINTER(PotentialResult)]),
    ("psamd_download_potential_far", C.c_int, [_vp, _vp, _i64, C.POINTER(PotentialResult)]),
    ("psamd_download_potential_flags", C.c_int, [_vp, C.c_uint32, _vp, _i64, C.POINTER(PotentialResult)]),
    ("psamd_probe", C.c_int, [_vp, C.POINTER(ProbeSpec)]),
    ("psamd_probe_result_get", C.c_int, [_vp, C.POINTER(ProbeResult)]),
    ("psamd_deposit", C.c_int, [_vp, C.POINTER(DepositSpec)]),
    ("psamd_deposit_result_get", C.c_int, [_vp, C.POINTER(DepositResult)]),
    ("psamd_download_deposit", C.c_int, [_vp, C.c_int32, _vp, _i64, C.POINTER(DepositResult)]),
    ("psamd_sample", C.c_int, [_vp, C.POINTER(SampleSpec)]),
    ("psamd_sample_result_get", C.c_int, [_vp, C.POINTER(SampleResult)]),
    ("psamd_neighbours", C.c_int, [_vp, C.POINTER(NeighboursSpec)]),
    ("psamd_neighbours_result_get", C.c_int, [_vp, C.POINTER(NeighboursResult)]),
    ("psamd_download_neighbours", C.c_int, [_vp, C.c_uint32, C.c_float, _vp, _vp, _vp, _vp, _i64, _vp, _i64, C.POINTER(NeighboursResult)]),
    ("psamd_groups", C.c_int, [_vp, C.POINTER(GroupsSpec)]),
    ("psamd_groups_result_get", C.c_int, [_vp, C.POINTER(GroupsResult)]),
    ("psamd_download_groups", C.c_int, [_vp, C.c_uint32, C.c_float, _vp, _i64, _vp, _vp, _i64, C.POINTER(GroupsResult)]),
    ("psamd_knn", C.c_int, [_vp, C.POINTER(KnnSpec)]),
    ("psamd_knn_result_get", C.c_int, [_vp, C.POINTER(KnnResult)]),
    ("psamd_download_knn", C.c_int, [_vp, C.c_uint32, C.c_float, C.c_int32, _vp, _vp, _vp, _i64, C.POINTER(KnnResult)]),
]

def _knn_dict(rec, out, m, k):
    """knn()'s and download_knn()'s result: the record (its `found`, a sum, under "found_sum": the array has the name), the
    arrays cut to m entries, the rows as [m, k]"""
    res = dict(rec)
    res["found_sum"] = res.pop("found")
    for name, a in out.items():
        res[name] = a[:m] if name == "found" else a[:m * k].reshape(m, k)
    return res


_lib = None


def build(force=False):
    """Compile libpsamd.so for gfx950 (hipcc cross-compiles without a GPU)."""
    return _build.build(force=force)


def load():
    """Load libpsamd.so and bind every ABI symbol. Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libpsamd.so is not built (run particlesystem_amd.build()); "
                               "the HIP library is the only implementation, there is no fallback")
        lib = C.CDLL(LIB_PATH)
        for name, res, args in ABI:
            fn = getattr(lib, name)  # AttributeError here = a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        have = lib.psamd_abi_version()
        if have != ABI_VERSION:
            # (PSAMD_LIB may point at another build: a library with other struct layouts would misread the
            # configuration and hand out garbage message pointers)
            raise RuntimeError("%s has ABI version %d, this module is written for %d: rebuild it (particlesystem_amd.build(force=True))"
                               % (LIB_PATH, have, ABI_VERSION))
        _lib = lib
    return _lib


def default_config(**over):
    cfg = Config()
    load().psamd_default_config(C.byref(cfg))
    for k, v in over.items():
        if k == "cuts":
            for i, c in enumerate(v):
                cfg.cuts[i] = c
        else:
            setattr(cfg, k, v)
    return cfg


def slab_plan(cfg):
    """Host-only: the slab plan of cfg.rank in a world of cfg.world ranks (no GPU needed)."""
    lib = load()
    plan = SlabPlan()
    st = lib.psamd_slab_plan_describe(C.byref(cfg), C.byref(plan))
    if st != 0:
        raise PsamdError(st, lib.psamd_status_string(st).decode())
    return plan


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def far_levels(cfg):
    """Host-only: the cells per axis of every level of the pyramid of monopoles, [G_0 .. G_L] (no GPU needed)."""
    lib = load()
    n = C.c_int32()
    dims = (C.c_int32 * 16)()
    st = lib.psamd_far_levels(C.byref(cfg), C.byref(n), dims)
    if st != 0:
        raise PsamdError(st, lib.psamd_status_string(st).decode())
    return [int(dims[k]) for k in range(n.value)]


def describe(cfg):
    """Host-only geometry of a configuration: sizes, cell table [num_cells, 3], package
    table [num_chunks, 54], initial QUEUE_INFO records and queue array.  Needs no GPU."""
    lib = load()
    sizes = Sizes()
    st = lib.psamd_describe(C.byref(cfg), C.byref(sizes), None, None, None, None)
    if st != 0:
        raise PsamdError(st, lib.psamd_status_string(st).decode())
    table = np.zeros((sizes.num_cells, 3), np.int32)
    pkg = np.zeros((sizes.num_chunks, 54), np.int32)
    qi = np.zeros(sizes.queue_info_size, Q_DTYPE)
    q = np.zeros(sizes.container_size, np.int32)
    st = lib.psamd_describe(C.byref(cfg), None, _ptr(table), _ptr(pkg), _ptr(qi), _ptr(q))
    if st != 0:
        raise PsamdError(st, lib.psamd_status_string(st).decode())
    return sizes, table, pkg, qi, q


# ---- the services' Python front: a torch device tensor checked, as the pointer the C spec takes -------------------------------------
def _tensor_ptr(who, t, dtype, shape, dev=None, what="tensor"):
    """None for None; dev: the device the tensor must be on as well (where the service compares devices)"""
    if t is None:
        return None
    assert t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() and (dev is None or t.device == dev), \
        "%s: bad %s" % (who, what)
    return t.data_ptr()


def _count_ptr(who, count, dev=None):
    """the one-element int64 device count"""
    import torch
    return _tensor_ptr(who, count, torch.int64, (1,), dev, "count tensor")


def _outcome(m, dev):
    """the int32 codes of m entries, -1 until the service writes them"""
    import torch
    return torch.full((max(m, 1),), -1, dtype=torch.int32, device=dev)


class ParticleSystem:
    """One psamd context: the reference's nine buffers, resident on one MI355X."""

    def __init__(self, cfg=None, **over):
        self.lib = load()
        self.cfg = cfg if cfg is not None else default_config(**over)
        h = C.c_void_p()
        st = self.lib.psamd_create(C.byref(self.cfg), C.byref(h))
        self.h = h
        if st != 0:
            msg = self.lib.psamd_last_error(h).decode() if h else self.lib.psamd_status_string(st).decode()
            if h:
                self.lib.psamd_destroy(h)
            self.h = None
            raise PsamdError(st, msg)
        self.sizes = Sizes()
        self._ck(self.lib.psamd_get_sizes(self.h, C.byref(self.sizes)))

    def _own_record(self, cls, fn):
        """the record the context keeps of a service's last call, as a dict"""
        r = cls()
        self._ck(fn(self.h, C.byref(r)))
        return r.to_dict()

    def _ck(self, st):
        if st != 0:
            raise PsamdError(st, self.lib.psamd_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.psamd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup ------------------------------------------------------------
    def uniform_cloud(self, n, seed):
        xyz = np.empty((n, 3), np.float32)
        self._ck(self.lib.psamd_uniform_cloud(self.h, n, seed, _ptr(xyz)))
        return xyz

    def fill_particles(self, xyz, age=None, fert_age=None, w=None, vxyz=None):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)

        def arr(v):
            if v is None:
                return None
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (n,)))
        age, fert_age, w = arr(age), arr(fert_age), arr(w)
        vxyz = None if vxyz is None else np.ascontiguousarray(vxyz, np.float32).reshape(-1, 3)
        ids = np.empty(n, np.int32)
        done = C.c_int64()
        self._ck(self.lib.psamd_fill_particles(self.h, n, _ptr(xyz), _ptr(vxyz), _ptr(w), _ptr(age),
                                               _ptr(fert_age), _ptr(ids), C.byref(done)))
        return ids

    # ---- reference-layout buffers ------------------------------------------
    def upload_particles(self, p, first=0):
        p = np.ascontiguousarray(p)
        assert p.dtype == P_DTYPE
        self._ck(self.lib.psamd_upload_particles(self.h, _ptr(p), first, len(p)))

    def download_particles(self, first=0, count=None):
        count = self.sizes.container_size - first if count is None else count
        p = np.zeros(count, P_DTYPE)
        self._ck(self.lib.psamd_download_particles(self.h, _ptr(p), first, count))
        return p

    def download_tdata(self, first=0, count=None):
        count = self.sizes.container_size - first if count is None else count
        t = np.zeros(count, T_DTYPE)
        self._ck(self.lib.psamd_download_tdata(self.h, _ptr(t), first, count))
        return t

    def upload_queues(self, queue_info, queue):
        qi = np.ascontiguousarray(queue_info)
        q = np.ascontiguousarray(queue, np.int32)
        assert qi.dtype == Q_DTYPE and len(qi) == self.sizes.queue_info_size and len(q) == self.sizes.container_size
        self._ck(self.lib.psamd_upload_queues(self.h, _ptr(qi), _ptr(q)))

    def download_queues(self):
        qi = np.zeros(self.sizes.queue_info_size, Q_DTYPE)
        q = np.zeros(self.sizes.container_size, np.int32)
        self._ck(self.lib.psamd_download_queues(self.h, _ptr(qi), _ptr(q)))
        return qi, q

    def download_cellgrid(self):
        out = np.zeros(self.sizes.n_cellgrid, np.int32)
        self._ck(self.lib.psamd_download_cellgrid(self.h, _ptr(out)))
        return out.reshape(self.sizes.num_cells, -1)

    def download_chunkgrid(self):
        out = np.zeros(self.sizes.n_chunkgrid, np.int32)
        self._ck(self.lib.psamd_download_chunkgrid(self.h, _ptr(out)))
        return out.reshape(self.sizes.num_chunks, -1)

    def download_force_counts(self):
        """Per cell: particles the last pair pass computed a force for."""
        out = np.zeros(self.sizes.num_cells, np.int32)
        self._ck(self.lib.psamd_download_force_counts(self.h, _ptr(out)))
        return out

    def download_cell_moments(self):
        """Per cell of the frame (far monopoles): (X, Y, Z, M), the centre of mass and the total w_eff, float32 [num_cells, 4]."""
        out = np.zeros((self.sizes.num_cells, 4), np.float32)
        self._ck(self.lib.psamd_download_cell_moments(self.h, _ptr(out)))
        return out

    def download_level_moments(self, level):
        """Per cell of a level of the pyramid (PSAMD_FLAG_FAR_PYRAMID; level 0: the cells): (X, Y, Z, M), float32 [G_level^3, 4]."""
        dims = far_levels(self.cfg)
        if not 0 <= level < len(dims):
            raise PsamdError(1, "no such level")
        out = np.zeros((dims[level] ** 3, 4), np.float32)
        self._ck(self.lib.psamd_download_level_moments(self.h, level, _ptr(out)))
        return out

    def download_level_quadrupoles(self, level):
        """Per cell of a level of a quadrupole context (PSAMD_FLAG_FAR_QUADRUPOLE): the central second moments
        (Cxx, Cyy, Czz, Cxy, Cxz, Cyz), float32 [G_level^3, 6]."""
        dims = far_levels(self.cfg)
        if not 0 <= level < len(dims):
            raise PsamdError(1, "no such level")
        out = np.zeros((dims[level] ** 3, 6), np.float32)
        self._ck(self.lib.psamd_download_level_quadrupoles(self.h, level, _ptr(out)))
        return out

    def pkgdistrib(self):
        out = np.zeros(self.sizes.n_pkgdistrib * 2, np.int32)
        self._ck(self.lib.psamd_get_pkgdistrib(self.h, _ptr(out)))
        return out.reshape(self.sizes.num_chunks, 54)

    def cell_table(self):
        out = np.zeros(self.sizes.num_cells * 3, np.int32)
        self._ck(self.lib.psamd_get_cell_table(self.h, _ptr(out)))
        return out.reshape(-1, 3)

    def gridmax(self):
        out = np.zeros(2, np.int32)
        self._ck(self.lib.psamd_get_gridmax(self.h, out.ctypes.data_as(_ip)))
        return out

    # ---- stages -------------------------------------------------------------
    def init_iframe(self):
        self._ck(self.lib.psamd_init_iframe(self.h))

    def build_grid(self):
        self._ck(self.lib.psamd_build_grid(self.h))

    def calc_forces(self):
        self._ck(self.lib.psamd_calc_forces(self.h))

    def calc_forces_pairs(self):
        self._ck(self.lib.psamd_calc_forces_pairs(self.h))

    def calc_forces_apply(self):
        self._ck(self.lib.psamd_calc_forces_apply(self.h))

    # ---- slab stages (multi-GPU; see include/psamd.h "slab partition") ------
    def slab_plan(self):
        plan = SlabPlan()
        self._ck(self.lib.psamd_get_slab_plan(self.h, C.byref(plan)))
        return plan

    def slab_buffers(self):
        b = SlabBuffers()
        self._ck(self.lib.psamd_slab_buffers_get(self.h, C.byref(b)))
        return b

    def slab_build(self):
        self._ck(self.lib.psamd_slab_build(self.h))

    def slab_pairs_interior(self):
        self._ck(self.lib.psamd_slab_pairs_interior(self.h))

    def slab_pairs(self):
        self._ck(self.lib.psamd_slab_pairs(self.h))

    def slab_apply(self):
        self._ck(self.lib.psamd_slab_apply(self.h))

    def slab_finish(self):
        self._ck(self.lib.psamd_slab_finish(self.h))

    def msg_table(self):
        """For every `which` of psamd_slab_msg_download: (device pointer, bytes that travel, bytes of room), read once.  Only
        the transfer messages (6-9) travel with less than their room, and that may grow: msg_bytes() asks for it afresh."""
        if getattr(self, "_msg_table", None) is None:
            b, w = self.slab_buffers(), max(1, self.cfg.world)
            t = [(b.halo_out[k], b.halo_out_bytes[k]) for k in (0, 1)] + [(b.halo_in[k], b.halo_in_bytes[k]) for k in (0, 1)]
            t += [(b.force_out, b.force_out_bytes), (b.force_in, b.force_in_bytes)]
            t += [(p, b.xfer_bytes, b.xfer_bytes_max) for p in (*b.xfer_out, *b.xfer_in)]
            t += [(b.status_out, b.status_bytes), (b.status_in, b.status_bytes * w), (b.allg_out, b.allg_bytes), (b.allg_in, b.allg_bytes * w)]
            t += [(p, b.xfer2_bytes) for p in (*b.xfer2_out, *b.xfer2_in)]
            t += [(b.far_out, b.far_bytes), (b.far_in, b.far_bytes * w)]
            self._msg_table = [(e[0] or 0, e[1], e[-1]) for e in t]
        return self._msg_table

    def msg_bytes(self, which):
        """Size of message buffer `which` (psamd_slab_msg_download numbering); 0: no such message.  The transfer messages
        (6-9) may grow from step to step (config.xfer_cap_max): their size is asked for afresh."""
        if 6 <= which <= 9:
            return self.slab_buffers().xfer_bytes
        return self.msg_table()[which][1]

    def msg_download(self, which, nbytes=None):
        nbytes = self.msg_bytes(which) if nbytes is None else nbytes
        out = np.zeros(nbytes // 4, np.int32)
        self._ck(self.lib.psamd_slab_msg_download(self.h, which, _ptr(out), nbytes))
        return out

    def msg_upload(self, which, words):
        words = np.ascontiguousarray(words, np.int32)
        self._ck(self.lib.psamd_slab_msg_upload(self.h, which, _ptr(words), words.nbytes))

    def step(self, n=1):
        self._ck(self.lib.psamd_step(self.h, n))

    def synchronize(self):
        self._ck(self.lib.psamd_synchronize(self.h))

    def download_force4(self, first, count):
        out = np.zeros((count, 4), np.float32)
        self._ck(self.lib.psamd_download_force4(self.h, _ptr(out), first, count))
        return out

    def snapshot_save(self):
        self._ck(self.lib.psamd_snapshot_save(self.h))

    def snapshot_restore(self):
        self._ck(self.lib.psamd_snapshot_restore(self.h))

    def set_stream(self, hip_stream):
        self._ck(self.lib.psamd_set_stream(self.h, hip_stream))

    # ---- introspection ------------------------------------------------------
    @property
    def counters(self):
        c = Counters()
        self._ck(self.lib.psamd_get_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def live_count(self):
        n = C.c_int64()
        self._ck(self.lib.psamd_live_count(self.h, C.byref(n)))
        return n.value

    # ---- getting frames out (include/psamd.h) --------------------------------
    def stream(self):
        """the hipStream_t the context enqueues on, as an integer"""
        p = C.c_void_p()
        self._ck(self.lib.psamd_get_stream(self.h, C.byref(p)))
        return p.value or 0

    @contextlib.contextmanager
    def _on_stream(self, dev):
        """Calls enqueued inside follow what torch's current stream holds so far (the tensors they use are torch's: allocated,
        maybe written, there); leaving waits for the context's stream."""
        import torch
        st = torch.cuda.ExternalStream(self.stream(), device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        yield
        st.synchronize()

    def owned_slots(self):
        """slots this context holds (the whole container on one context): the most live particles it can have"""
        return int(self.device_view().container_size)

    def export_live(self, fields, capacity=None):
        """psamd_export_live into fresh torch device tensors: {"count": n, "stats": dict, field: tensor sliced to
        min(n, capacity)} for the fields asked for ("pos4", "vel4", "acc4": float32 [k, 4]; "id", "cell": int32 [k]).
        Waits for the context's stream before it returns.  torch must have been imported before the library was loaded
        (tests/conftest.py does) so that both use one HIP runtime."""
        import torch
        capacity = self.owned_slots() if capacity is None else int(capacity)
        dev = torch.device("cuda", int(self.cfg.device))
        spec = Export(fields=int(fields), capacity=capacity)
        out = {}
        for name, bit, width, dt in _EXPORT_FIELDS:
            if fields & bit:
                t = torch.empty((max(capacity, 1), width) if width > 1 else (max(capacity, 1),),
                                dtype=torch.float32 if dt is np.float32 else torch.int32, device=dev)
                out[name] = t
                setattr(spec, name, t.data_ptr())
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        stats = torch.zeros(C.sizeof(LiveStats), dtype=torch.uint8, device=dev)
        spec.count_dev, spec.stats_dev = count.data_ptr(), stats.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_export_live(self.h, C.byref(spec)))
        n = int(count.item())
        res = {name: t[:min(n, capacity)] for name, t in out.items()}
        res["count"] = n
        res["stats"] = LiveStats.from_device(stats).to_dict()
        return res

    def download_live(self, fields, capacity=None):
        """psamd_download_live: {"count": n, field: numpy array of min(n, capacity) entries} (fields as export_live)"""
        capacity = self.owned_slots() if capacity is None else int(capacity)
        arrs = {}
        ptrs = []
        for name, bit, width, dt in _EXPORT_FIELDS:
            if fields & bit:
                arrs[name] = np.zeros((capacity, width) if width > 1 else capacity, dt)
            ptrs.append(_ptr(arrs.get(name)))
        n = C.c_int64()
        self._ck(self.lib.psamd_download_live(self.h, int(fields), *ptrs, capacity, C.byref(n)))
        res = {name: a[:min(n.value, capacity)] for name, a in arrs.items()}
        res["count"] = n.value
        return res

    def live_stats(self):
        """psamd_live_stats_get as a dict (momentum, mass_moment, lo, hi: float64 arrays of 3)"""
        return self._own_record(LiveStats, self.lib.psamd_live_stats_get)

    # ---- putting particles in (include/psamd.h) --------------------------------
    def inject(self, pos4, vel4=None, fert_age=None, count=None, ids=False):
        """psamd_inject from torch device tensors: pos4 float32 [m, 4] (x, y, z, w), vel4 float32 [m, 4] (vx, vy, vz, age)
        or None, fert_age float32 [m] or None; count: None (all m entries) or a 1-element int64 device tensor that work
        on torch's current stream may write just before.  Returns {"done", "placed", "status"} and, with ids=True,
        "ids": an int32 device tensor of m entries (-1 where nothing was placed here).  Waits for the context's stream."""
        import torch
        dev = pos4.device
        m = int(pos4.shape[0])
        spec = Inject(max_count=m)
        spec.pos4 = _tensor_ptr("inject", pos4, torch.float32, (m, 4), dev)
        spec.vel4 = _tensor_ptr("inject", vel4, torch.float32, (m, 4), dev)
        spec.fert_age = _tensor_ptr("inject", fert_age, torch.float32, (m,), dev)
        spec.count_dev = _tensor_ptr("inject", count, torch.int64, (1,), dev)
        out_ids = _outcome(m, dev) if ids else None
        spec.ids_dev = None if out_ids is None else out_ids.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_inject(self.h, C.byref(spec)))
        res = self.inject_result()
        if ids:
            res["ids"] = out_ids[:m]
        return res

    def inject_result(self):
        """psamd_inject_result_get: the last inject's {"done", "placed", "status"}"""
        return self._own_record(InjectResult, self.lib.psamd_inject_result_get)

    # ---- taking particles out (include/psamd.h) ---------------------------------
    def remove(self, ids=None, count=None, box=None, outside=False, outcome=False):
        """psamd_remove.  By id: ids is an int32 [m] torch device tensor of slot ids, count None (all m entries) or a
        1-element int64 device tensor that work on torch's current stream may write just before; with outcome=True the
        result has "outcome": an int32 device tensor of m entries (the codes REMOVED .. REMOVE_DROPPED).  By box:
        box=(lo, hi), two triples; outside=True removes the live particles that are NOT inside.  Returns the result
        record as a dict (done, removed, not_live, foreign, invalid, dropped).  Waits for the context's stream.  torch must
        have been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        spec = Remove()
        out = None
        if box is not None:
            assert ids is None and count is None and not outcome, "remove: by box takes no ids, count or outcome"
            spec.flags = REMOVE_BOX | (REMOVE_OUTSIDE if outside else 0)
            for k in range(3):
                spec.lo[k], spec.hi[k] = float(box[0][k]), float(box[1][k])
        else:
            assert ids is not None and not outside, "remove: ids or box"
            m = int(ids.shape[0])
            p = _tensor_ptr("remove", ids, torch.int32, (m,), what="ids tensor")
            spec.max_count = m
            spec.ids = p if m > 0 else None
            spec.count_dev = _count_ptr("remove", count)
            if outcome:
                out = _outcome(m, dev)
                spec.outcome_dev = out.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_remove(self.h, C.byref(spec)))
        res = self.remove_result()
        if out is not None:
            res["outcome"] = out[:int(ids.shape[0])]
        return res

    def remove_result(self):
        """psamd_remove_result_get: the last remove's record as a dict"""
        return self._own_record(RemoveResult, self.lib.psamd_remove_result_get)

    # ---- changing particles in place (include/psamd.h) --------------------------
    def update(self, ids=None, vel4=None, w=None, fert_age=None, age=False, add=False, count=None, outcome=False, *, fields=None):
        """psamd_update from torch device tensors.  ids: an int32 [m] tensor of slot ids, or None: export order -- entry k
        belongs to the k-th live particle of export_live().  The words come from the arrays that are given: vel4 float32
        [m, 4] sets vx, vy, vz (add=True: adds to them, a kick) and, with age=True, the age from its fourth column; w float32
        [m] the mass; fert_age float32 [m] the fertility age.  fields: the PSAMD_UPDATE_* bits themselves, instead of what the
        arrays imply (UPDATE_AGE alone reads vel4's fourth column only; the order bit still follows ids).  count: None (all m
        entries) or a 1-element int64 device tensor that work on torch's current stream may write just before.  Returns the
        result record as a dict (done, updated, not_live, foreign, invalid, duplicate) and, with outcome=True, "outcome": an
        int32 device tensor of m entries (UPDATED .. UPDATE_DUPLICATE; -1 at and past the count).  Waits for the context's
        stream.  torch must have been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        given = [t for t in (ids, vel4, w, fert_age) if t is not None]
        assert given, "update: no array"
        m = int(given[0].shape[0])

        def ptr(t, dtype, shape):
            p = _tensor_ptr("update", t, dtype, shape)
            return p if m > 0 else None
        if fields is None:
            fields = ((UPDATE_VEL if vel4 is not None else 0) | (UPDATE_AGE if age else 0) | (UPDATE_ADD if add else 0) |
                      (UPDATE_MASS if w is not None else 0) | (UPDATE_FERT if fert_age is not None else 0))
        spec = Update(fields=int(fields) & ~UPDATE_EXPORT_ORDER | (UPDATE_EXPORT_ORDER if ids is None else 0), max_count=m)
        spec.ids = ptr(ids, torch.int32, (m,))
        spec.vel4 = ptr(vel4, torch.float32, (m, 4))
        spec.w = ptr(w, torch.float32, (m,))
        spec.fert_age = ptr(fert_age, torch.float32, (m,))
        spec.count_dev = _count_ptr("update", count)
        out = _outcome(m, dev) if outcome else None
        spec.outcome_dev = None if out is None else out.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_update(self.h, C.byref(spec)))
        res = self.update_result()
        if out is not None:
            res["outcome"] = out[:m]
        return res

    def update_result(self):
        """psamd_update_result_get: the last update's record as a dict"""
        return self._own_record(UpdateResult, self.lib.psamd_update_result_get)

    # ---- energy (include/psamd.h) -----------------------------------------------
    def potential(self, phi=False, capacity=None, far=False, *, quadrupole=False):
        """psamd_potential: {"listed", "nonfinite", "potential", "phi_min", "phi_max"} of the frame that is built (after
        build_grid; a slab: between slab_pairs and slab_apply) and, with phi=True, "phi": a float32 torch device tensor of
        min(live count, capacity) entries that pairs, entry for entry, with export_live() at the same point of the stream.
        far=True: PSAMD_POTENTIAL_FAR -- on a far-monopole context, the far bodies of its force model behind the stencil;
        quadrupole=True beside it: PSAMD_POTENTIAL_QUADRUPOLE -- on a quadrupole context, their quadrupole terms too.
        Waits for the context's stream.  torch must have been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        spec = Potential(flags=(POTENTIAL_FAR if far else 0) | (POTENTIAL_QUADRUPOLE if quadrupole else 0))
        result = torch.zeros(C.sizeof(PotentialResult), dtype=torch.uint8, device=dev)
        spec.result_dev = result.data_ptr()
        out = count = None
        if phi:
            capacity = self.owned_slots() if capacity is None else int(capacity)
            out = torch.empty(max(capacity, 1), dtype=torch.float32, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            spec.phi, spec.capacity = out.data_ptr(), capacity
        with self._on_stream(dev):
            self._ck(self.lib.psamd_potential(self.h, C.byref(spec)))
            if phi:      # how many entries were written: the live count at this point of the stream
                self._ck(self.lib.psamd_export_live(self.h, C.byref(Export(fields=0, capacity=0, count_dev=count.data_ptr()))))
        res = PotentialResult.from_device(result).to_dict()
        if phi:
            res["phi"] = out[:min(int(count.item()), capacity)]
        return res

    def potential_result(self):
        """psamd_potential_result_get: the last potential call's record"""
        return self._own_record(PotentialResult, self.lib.psamd_potential_result_get)

    def download_potential(self, phi=True, capacity=None, far=False, *, quadrupole=False):
        """psamd_download_potential (far=True: psamd_download_potential_far; quadrupole=True: psamd_download_potential_flags
        with PSAMD_POTENTIAL_QUADRUPOLE beside what `far` gives), the numpy form of potential(): "phi" is a float32 array of
        min(live count, capacity)"""
        r = PotentialResult()
        call = self.lib.psamd_download_potential_far if far else self.lib.psamd_download_potential
        if quadrupole:
            flags = (POTENTIAL_FAR if far else 0) | POTENTIAL_QUADRUPOLE
            call = lambda h, out, cap, res: self.lib.psamd_download_potential_flags(h, flags, out, cap, res)
        if not phi:
            self._ck(call(self.h, None, 0, C.byref(r)))
            return r.to_dict()
        capacity = self.owned_slots() if capacity is None else int(capacity)
        out = np.full(max(capacity, 1), np.nan, np.float32)
        self._ck(call(self.h, _ptr(out), capacity, C.byref(r)))
        res = r.to_dict()
        n = C.c_int64()        # how many entries were written: the export's count at this point (no fields, nothing copied)
        self._ck(self.lib.psamd_download_live(self.h, 0, None, None, None, None, None, 0, C.byref(n)))
        res["phi"] = out[:min(n.value, capacity)]
        return res

    def energy(self, far=False, *, quadrupole=False):
        """{"kinetic", "potential", "total"} of the frame that is built: one potential() and one live_stats() at the same
        point of the stream (kinetic: psamd_live_stats.kinetic, sum 0.5 w |v|^2 over the live particles); far=True: the
        potential of a far-monopole context's own field (PSAMD_POTENTIAL_FAR), with quadrupole=True beside it of a
        quadrupole context's (PSAMD_POTENTIAL_QUADRUPOLE)"""
        u = self.potential(far=far, quadrupole=quadrupole)["potential"]
        k = float(self.live_stats()["kinetic"])
        return {"kinetic": k, "potential": u, "total": k + u}

    # ---- the field at chosen points (include/psamd.h) ---------------------------
    def probe(self, pos4, count=None, acc=True, phi=True, outcome=False, far=False, *, quadrupole=False):
        """psamd_probe from a torch device tensor: pos4 float32 [m, 4] (x, y, z; w ignored -- an export's "pos4" as it is);
        count: None (all m entries) or a 1-element int64 device tensor that work on torch's current stream may write just
        before.  Returns {"out4": float32 [m, 4] device tensor (acceleration in xyz, potential in w; quiet NaNs where the
        entry was not served), "done", "served", "outside", "foreign", "nonfinite"} and, with outcome=True, "outcome": an
        int32 device tensor of m entries (PROBE_SERVED, PROBE_OUTSIDE, PROBE_FOREIGN).  Entries at or past the count keep
        the zeros (out4) and -1 (outcome) they were allocated with.  far=True: PSAMD_PROBE_FAR beside the components -- on a
        far-monopole context, the far bodies of its force model too; quadrupole=True beside it: PSAMD_PROBE_QUADRUPOLE -- on a
        quadrupole context, their quadrupole terms too.  Waits for the context's stream."""
        import torch
        dev = pos4.device
        m = int(pos4.shape[0])
        p = _tensor_ptr("probe", pos4, torch.float32, (m, 4), what="pos4 tensor")
        spec = ProbeSpec(fields=(PROBE_ACC if acc else 0) | (PROBE_PHI if phi else 0) | (PROBE_FAR if far else 0) |
                         (PROBE_QUADRUPOLE if quadrupole else 0), max_count=m)
        out4 = torch.zeros((max(m, 1), 4), dtype=torch.float32, device=dev)
        spec.pos4, spec.out4 = (p, out4.data_ptr()) if m > 0 else (None, None)
        spec.count_dev = _count_ptr("probe", count, dev)
        codes = _outcome(m, dev) if outcome else None
        spec.outcome_dev = None if codes is None else codes.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_probe(self.h, C.byref(spec)))
        res = self.probe_result()
        res["out4"] = out4[:m]
        if outcome:
            res["outcome"] = codes[:m]
        return res

    def probe_result(self):
        """psamd_probe_result_get: the last probe's record as a dict"""
        return self._own_record(ProbeResult, self.lib.psamd_probe_result_get)

    # ---- mass on a lattice (include/psamd.h) ------------------------------------
    def deposit(self, refine=1, out=None, result=False):
        """psamd_deposit: the mass density of the frame that is built (after build_grid; a slab: between slab_pairs and
        slab_apply) on the lattice of `refine` voxels per cell edge, cloud-in-cell: a float32 torch device tensor of shape
        (M, M, M), M = grid_dim * refine, indexed [n3, n1, n2] (the cell axes: -z, -y, x).  out: such a tensor to write
        into (a slab rank writes the voxels of its compute cells and leaves the others as they are); None: a fresh one of
        zeros.  result=True: (tensor, the record as a dict).  Waits for the context's stream.  torch must have been
        imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        m = int(self.sizes.grid_dim) * int(refine)
        if out is None:
            out = torch.zeros((m, m, m), dtype=torch.float32, device=dev)
        p = _tensor_ptr("deposit", out, torch.float32, (m, m, m), what="out tensor")
        rec = torch.zeros(C.sizeof(DepositResult), dtype=torch.uint8, device=dev)
        spec = DepositSpec(flags=0, refine=int(refine), out=p, capacity=out.numel(), result_dev=rec.data_ptr())
        with self._on_stream(dev):
            self._ck(self.lib.psamd_deposit(self.h, C.byref(spec)))
        return (out, DepositResult.from_device(rec).to_dict()) if result else out

    def deposit_result(self):
        """psamd_deposit_result_get: the last deposit's record as a dict"""
        return self._own_record(DepositResult, self.lib.psamd_deposit_result_get)

    def download_deposit(self, refine=1):
        """psamd_download_deposit, the numpy form of deposit(): (float32 array [M, M, M] of the whole lattice -- on a slab +0
        where another rank serves the voxel -- and the record as a dict)"""
        m = int(self.sizes.grid_dim) * int(refine)
        out = np.full((max(m, 1),) * 3, np.nan, np.float32)
        r = DepositResult()
        self._ck(self.lib.psamd_download_deposit(self.h, int(refine), _ptr(out), out.size, C.byref(r)))
        return out, r.to_dict()

    # ---- a lattice field at the particles (include/psamd.h) ---------------------
    def sample(self, field, pos4=None, count=None, scale=1.0, out=None, outcome=False, result=False):
        """psamd_sample: a lattice field of the caller's read at points, cloud-in-cell with deposit()'s weights.  field: a
        float32 torch device tensor [M, M, M] or [M, M, M, 4] on deposit()'s lattice (indexed [n3, n1, n2]; refine is
        M / grid_dim).  pos4: float32 [m, 4] (x, y, z; w ignored), or None: export order -- entry k is the k-th live particle
        of export_live(), as many entries as `out` has, or as the context owns slots.  count: None (all entries) or a
        1-element int64 device tensor that work on torch's current stream may write just before.  out: a float32 tensor [m]
        or [m, 4] to write into (entries that are not served stay as they are); None: a fresh one of zeros.  Every word is
        scale times the interpolated value; a point outside the box gets quiet NaNs.  Returns out, or with outcome=True
        and / or result=True the tuple (out, [outcome: int32 [m], SAMPLE_SERVED / SAMPLE_OUTSIDE, -1 where no entry was
        examined], [the record as a dict]).  Waits for the context's stream.  torch must have been imported before the
        library was loaded."""
        import torch
        dev = field.device
        vec4 = field.dim() == 4
        M = int(field.shape[0])
        G = int(self.sizes.grid_dim)
        assert M % G == 0, "sample: the field's edge is no multiple of grid_dim"
        fp = _tensor_ptr("sample", field, torch.float32, (M, M, M, 4) if vec4 else (M, M, M), what="field tensor")
        if pos4 is not None:
            m = int(pos4.shape[0])
        else:
            m = int(out.shape[0]) if out is not None else self.owned_slots()
        shape = (max(m, 1), 4) if vec4 else (max(m, 1),)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float32, device=dev)
            op = out.data_ptr()
        else:
            op = _tensor_ptr("sample", out, torch.float32, (m, 4) if vec4 else (m,), dev, "out tensor")
        spec = SampleSpec(flags=(SAMPLE_VEC4 if vec4 else 0) | (SAMPLE_EXPORT_ORDER if pos4 is None else 0), refine=M // G, field=fp,
                          capacity=M ** 3, max_count=m, scale=float(scale))
        spec.pos4 = _tensor_ptr("sample", pos4, torch.float32, (m, 4), dev, "pos4 tensor") if m > 0 else None
        spec.out = op if m > 0 else None
        spec.count_dev = _count_ptr("sample", count, dev)
        codes = _outcome(m, dev) if outcome else None
        spec.outcome_dev = None if codes is None else codes.data_ptr()
        rec = torch.zeros(C.sizeof(SampleResult), dtype=torch.uint8, device=dev) if result else None
        spec.result_dev = None if rec is None else rec.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_sample(self.h, C.byref(spec)))
        ret = (out[:m],) + ((codes[:m],) if outcome else ()) + ((SampleResult.from_device(rec).to_dict(),) if result else ())
        return ret if len(ret) > 1 else ret[0]

    def sample_result(self):
        """psamd_sample_result_get: the last sample's record as a dict"""
        return self._own_record(SampleResult, self.lib.psamd_sample_result_get)

    # ---- neighbours within a radius (include/psamd.h) -----------------------------
    def neighbours(self, radius, lists=True, nearest=False, index=False, capacity=None, list_capacity=None):
        """psamd_neighbours on the frame that is built (psamd_potential's window): every pair within `radius` (<= cell_size)
        over the 27-cell stencil, in export order -- entry k belongs to the k-th live particle of export_live() at the same
        point of the stream.  Returns the record (listed, pairs, wanted, max_count, d2_min) as a dict with torch tensors on
        the context's device beside it: "count" int32 [m] (-1: in no list of the frame), m = min(live count, capacity); with
        lists=True "offsets" int64 [m + 1] and "list" int32 [min(wanted, list_capacity)] -- the neighbours of entry k are
        list[offsets[k]:offsets[k + 1]], in walk order, named by global slot id or, with index=True, by export index
        (pos[list] is then a plain gather; world == 1 only); with nearest=True "nearest" int32 [m] and "nearest_d2" float32 [m].
        With lists=True and no list_capacity this is the two-call pattern: a count call first, whose `wanted` is read back
        and sizes the list -- it waits for the context's stream once more than the one call a given list_capacity takes.
        Waits for the context's stream.  torch must have been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        capacity = self.owned_slots() if capacity is None else int(capacity)
        flags = NEIGHBOURS_INDEX if index else 0

        def call(want_list, room):
            spec = NeighboursSpec(flags=flags, radius=float(radius), capacity=capacity)
            out = {"count": torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)}
            spec.count = out["count"].data_ptr()
            if lists:
                out["offsets"] = torch.zeros(capacity + 1, dtype=torch.int64, device=dev)
                spec.offsets = out["offsets"].data_ptr()
            if nearest:
                out["nearest"] = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
                out["nearest_d2"] = torch.empty(max(capacity, 1), dtype=torch.float32, device=dev)
                spec.nearest, spec.nearest_d2 = out["nearest"].data_ptr(), out["nearest_d2"].data_ptr()
            if want_list:
                out["list"] = torch.empty(max(room, 1), dtype=torch.int32, device=dev)
                spec.list, spec.list_capacity = out["list"].data_ptr(), room
            result = torch.zeros(C.sizeof(NeighboursResult), dtype=torch.uint8, device=dev)
            live = torch.zeros(1, dtype=torch.int64, device=dev)
            spec.result_dev = result.data_ptr()
            with self._on_stream(dev):
                self._ck(self.lib.psamd_neighbours(self.h, C.byref(spec)))
                # how many entries were written: the live count at this point of the stream
                self._ck(self.lib.psamd_export_live(self.h, C.byref(Export(fields=0, capacity=0, count_dev=live.data_ptr()))))
            return out, NeighboursResult.from_device(result).to_dict(), min(int(live.item()), capacity)
        if lists and list_capacity is None:
            _, rec, _ = call(False, 0)
            list_capacity = rec["wanted"]
        out, rec, m = call(lists, int(list_capacity or 0))
        res = dict(rec)
        for k, t in out.items():
            res[k] = t[:m + 1] if k == "offsets" else t[:min(rec["wanted"], int(list_capacity))] if k == "list" else t[:m]
        return res

    def neighbours_result(self):
        """psamd_neighbours_result_get: the last neighbours call's record"""
        return self._own_record(NeighboursResult, self.lib.psamd_neighbours_result_get)

    def download_neighbours(self, radius, lists=True, nearest=False, index=False, capacity=None, list_capacity=None):
        """psamd_download_neighbours, the numpy form of neighbours(): the same keys, numpy arrays"""
        capacity = self.owned_slots() if capacity is None else int(capacity)
        flags = NEIGHBOURS_INDEX if index else 0
        r = NeighboursResult()
        if lists and list_capacity is None:
            offs = np.zeros(capacity + 1, np.int64)       # the count call: `wanted` is offsets[m]
            self._ck(self.lib.psamd_download_neighbours(self.h, flags, float(radius), None, None, None, _ptr(offs), capacity, None, 0, C.byref(r)))
            list_capacity = int(r.wanted)
        list_capacity = int(list_capacity or 0)
        out = {"count": np.full(max(capacity, 1), -7, np.int32)}
        if lists:
            out["offsets"] = np.zeros(capacity + 1, np.int64)
            out["list"] = np.full(max(list_capacity, 1), -7, np.int32)
        if nearest:
            out["nearest"] = np.full(max(capacity, 1), -7, np.int32)
            out["nearest_d2"] = np.zeros(max(capacity, 1), np.float32)
        self._ck(self.lib.psamd_download_neighbours(self.h, flags, float(radius), _ptr(out["count"]), _ptr(out.get("nearest")),
                                                    _ptr(out.get("nearest_d2")), _ptr(out.get("offsets")), capacity,
                                                    _ptr(out.get("list")), list_capacity if lists else 0, C.byref(r)))
        n = C.c_int64()        # how many entries were written: the export's count at this point (no fields, nothing copied)
        self._ck(self.lib.psamd_download_live(self.h, 0, None, None, None, None, None, 0, C.byref(n)))
        m = min(n.value, capacity)
        res = r.to_dict()
        for k, a in out.items():
            res[k] = a[:m + 1] if k == "offsets" else a[:min(res["wanted"], list_capacity)] if k == "list" else a[:m]
        return res

    # ---- groups within a radius (include/psamd.h) -----------------------------------
    def groups(self, radius, index=False, capacity=None, group_capacity=None):
        """psamd_groups on the frame that is built (psamd_potential's window, world == 1): the friends-of-friends groups --
        the connected components of neighbours()' relation at `radius` (<= cell_size) over the members, the listed particles
        that are no kids.  Returns the record (members, groups, links, singles, largest, unfinished) as a dict with torch
        tensors on the context's device beside it: "group" int32 [m], m = min(live count, capacity), in export order -- the
        dense group number of the k-th live particle of export_live() at the same point of the stream, -1: no member;
        "group_first" and "group_size" int32 [min(groups, group_capacity)] -- group g's smallest member (by global slot id
        or, with index=True, by export index) and its member count.  Groups are numbered in ascending order of their smallest
        member.  With no group_capacity this is the two-call pattern: a record-only call first, whose `groups` is read back
        and sizes the tables -- it waits for the context's stream once more than the one call a given group_capacity takes.
        Waits for the context's stream.  torch must have been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        capacity = self.owned_slots() if capacity is None else int(capacity)
        flags = GROUPS_INDEX if index else 0

        def call(arrays, room):
            spec = GroupsSpec(flags=flags, radius=float(radius))
            out = {}
            if arrays:
                out = {"group": torch.empty(max(capacity, 1), dtype=torch.int32, device=dev),
                       "group_first": torch.empty(max(room, 1), dtype=torch.int32, device=dev),
                       "group_size": torch.empty(max(room, 1), dtype=torch.int32, device=dev)}
                spec.group, spec.capacity = out["group"].data_ptr(), capacity
                spec.group_first, spec.group_size, spec.group_capacity = out["group_first"].data_ptr(), out["group_size"].data_ptr(), room
            result = torch.zeros(C.sizeof(GroupsResult), dtype=torch.uint8, device=dev)
            live = torch.zeros(1, dtype=torch.int64, device=dev)
            spec.result_dev = result.data_ptr()
            with self._on_stream(dev):
                self._ck(self.lib.psamd_groups(self.h, C.byref(spec)))
                # how many entries were written: the live count at this point of the stream
                self._ck(self.lib.psamd_export_live(self.h, C.byref(Export(fields=0, capacity=0, count_dev=live.data_ptr()))))
            return out, GroupsResult.from_device(result).to_dict(), min(int(live.item()), capacity)
        if group_capacity is None:
            _, rec, _ = call(False, 0)
            group_capacity = rec["groups"]
        group_capacity = int(group_capacity)
        out, rec, m = call(True, group_capacity)
        res = dict(rec)
        for k, t in out.items():
            res[k] = t[:m] if k == "group" else t[:min(rec["groups"], group_capacity)]
        return res

    def groups_result(self):
        """psamd_groups_result_get: the last groups call's record"""
        return self._own_record(GroupsResult, self.lib.psamd_groups_result_get)

    def download_groups(self, radius, index=False, capacity=None, group_capacity=None):
        """psamd_download_groups, the numpy form of groups(): the same keys, numpy arrays"""
        capacity = self.owned_slots() if capacity is None else int(capacity)
        flags = GROUPS_INDEX if index else 0
        r = GroupsResult()
        if group_capacity is None:
            self._ck(self.lib.psamd_download_groups(self.h, flags, float(radius), None, 0, None, None, 0, C.byref(r)))
            group_capacity = int(r.groups)
        group_capacity = int(group_capacity)
        out = {"group": np.full(max(capacity, 1), -7, np.int32), "group_first": np.full(max(group_capacity, 1), -7, np.int32),
               "group_size": np.full(max(group_capacity, 1), -7, np.int32)}
        self._ck(self.lib.psamd_download_groups(self.h, flags, float(radius), _ptr(out["group"]), capacity, _ptr(out["group_first"]),
                                                _ptr(out["group_size"]), group_capacity, C.byref(r)))
        n = C.c_int64()        # how many entries were written: the export's count at this point (no fields, nothing copied)
        self._ck(self.lib.psamd_download_live(self.h, 0, None, None, None, None, None, 0, C.byref(n)))
        m = min(n.value, capacity)
        res = r.to_dict()
        for k, a in out.items():
            res[k] = a[:m] if k == "group" else a[:min(res["groups"], group_capacity)]
        return res

    # ---- the k nearest within a radius (include/psamd.h) ------------------------------
    def knn(self, radius, k, index=False, capacity=None, found=True):
        """psamd_knn on the frame that is built (psamd_neighbours' window): every listed particle's k nearest neighbours within
        `radius` (<= cell_size) over the 27-cell stencil, ordered by (d2, global slot id), in export order -- entry o belongs
        to the o-th live particle of export_live() at the same point of the stream.  Returns the record (listed, found, full,
        k, dk2_min, dk2_max) as a dict with torch tensors on the context's device beside it: "who" int32 [m, k] and "d2"
        float32 [m, k], m = min(live count, capacity) -- the words past a row's min(count, k) are -1 and +inf -- and, with
        found=True, "found" int32 [m]: min(count, k), -1: in no list of the frame.  The record's own `found`, the sum, stands
        under "found_sum" (knn_result() has it under the record's name).  A neighbour is named by its global slot id or, with index=True, by its export index (world == 1 only).
        With no capacity the live count is read first and sizes the rows.  Waits for the context's stream.  torch must have
        been imported before the library was loaded."""
        import torch
        dev = torch.device("cuda", int(self.cfg.device))
        k = int(k)
        capacity = self.live_count() if capacity is None else int(capacity)
        spec = KnnSpec(flags=KNN_INDEX if index else 0, radius=float(radius), k=k, capacity=capacity)
        rows = max(capacity, 1) * max(min(k, KNN_MAX_K), 1)
        out = {"who": torch.empty(rows, dtype=torch.int32, device=dev), "d2": torch.empty(rows, dtype=torch.float32, device=dev)}
        spec.who, spec.d2 = out["who"].data_ptr(), out["d2"].data_ptr()
        if found:
            out["found"] = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
            spec.found = out["found"].data_ptr()
        result = torch.zeros(C.sizeof(KnnResult), dtype=torch.uint8, device=dev)
        live = torch.zeros(1, dtype=torch.int64, device=dev)
        spec.result_dev = result.data_ptr()
        with self._on_stream(dev):
            self._ck(self.lib.psamd_knn(self.h, C.byref(spec)))
            # how many entries were written: the live count at this point of the stream
            self._ck(self.lib.psamd_export_live(self.h, C.byref(Export(fields=0, capacity=0, count_dev=live.data_ptr()))))
        m = min(int(live.item()), capacity)
        return _knn_dict(KnnResult.from_device(result).to_dict(), out, m, k)

    def knn_result(self):
        """psamd_knn_result_get: the last knn call's record"""
        return self._own_record(KnnResult, self.lib.psamd_knn_result_get)

    def download_knn(self, radius, k, index=False, capacity=None, found=True):
        """psamd_download_knn, the numpy form of knn(): the same keys, numpy arrays"""
        k = int(k)
        capacity = self.live_count() if capacity is None else int(capacity)
        rows = max(capacity, 1) * max(min(k, KNN_MAX_K), 1)
        out = {"who": np.full(rows, -7, np.int32), "d2": np.zeros(rows, np.float32)}
        if found:
            out["found"] = np.full(max(capacity, 1), -7, np.int32)
        r = KnnResult()
        self._ck(self.lib.psamd_download_knn(self.h, KNN_INDEX if index else 0, float(radius), k, _ptr(out.get("found")), _ptr(out["who"]),
                                             _ptr(out["d2"]), capacity, C.byref(r)))
        n = C.c_int64()        # how many entries were written: the export's count at this point (no fields, nothing copied)
        self._ck(self.lib.psamd_download_live(self.h, 0, None, None, None, None, None, 0, C.byref(n)))
        return _knn_dict(r.to_dict(), out, min(n.value, capacity), k)

    def device_view(self):
        v = DeviceView()
        self._ck(self.lib.psamd_device_view_get(self.h, C.byref(v)))
        return v

    def wave_trace(self):
        n = 3 * (self.sizes.num_cells * ((self.sizes.max_per_cell + 63) // 64) + 4)
        out = np.zeros(n, np.uint64)
        self._ck(self.lib.psamd_debug_wave_trace(self.h, _ptr(out), n))
        return out.reshape(-1, 3)

    def download_packs(self):
        """psamd_debug_packs: (the last pair stage's packs as an (n, 4) array of cell numbers, -1 unused; its launch shape as a
        dict: wave slots, tile walk, two-pass stage, pack workgroups)"""
        n, shape = C.c_int64(), C.c_uint64()
        out = np.full((self.sizes.num_cells, 4), -1, np.int32)
        self._ck(self.lib.psamd_debug_packs(self.h, _ptr(out), len(out), C.byref(n), C.byref(shape)))
        s = shape.value
        return out[:n.value], dict(waves=32 * (s & 1023), tile=bool(s >> 10 & 1), two_pass=bool(s >> 11 & 1), pack_workgroups=8 * (s >> 12 & 0xfff))

    def selftest_math(self, lo_bits, hi_bits):
        out = (C.c_uint64 * 24)()
        self._ck(self.lib.psamd_selftest_math(self.h, lo_bits, hi_bits, out))
        return list(out)

    def set_graphs(self, on=True):
        """stage sequences as hipGraphs: one submission per stage instead of one per kernel"""
        self._ck(self.lib.psamd_set_graphs(self.h, 1 if on else 0))

    def graph_stats(self):
        """(replays, captures); raises if the runtime refused to capture and the context fell back"""
        a, b = C.c_int64(), C.c_int64()
        self._ck(self.lib.psamd_get_graph_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_wait_policy(self, policy):
        self._ck(self.lib.psamd_set_wait_policy(self.h, int(policy)))

    def set_tdata_mirror(self, on):
        """build_grid also writes the reference's T_DATA rows (needed by download_tdata only); default on"""
        self._ck(self.lib.psamd_set_tdata_mirror(self.h, 1 if on else 0))

    def set_run_ahead(self, steps):
        """1 (default): a call that ends a step returns once the step BEFORE has reported; 0: waits for its own step"""
        self._ck(self.lib.psamd_set_run_ahead(self.h, int(steps)))

    def set_timing(self, on=True, every_stage=False, period=1):
        """HIP-event timing of the step's kernels: pair pass, apply and life cycle, or every
        stage (an event between two kernels costs ~6 us of idle GPU each); period n: on every
        n-th step only."""
        self._ck(self.lib.psamd_set_timing_period(self.h, int(period)))
        self._ck(self.lib.psamd_set_timing(self.h, (2 if every_stage else 1) if on else 0))

    def timing(self):
        us = (C.c_double * NUM_TIMERS)()
        n = C.c_int64()
        self._ck(self.lib.psamd_get_timing(self.h, us, C.byref(n)))
        return dict(zip(TIMER_NAMES, list(us))), n.value

    def timing_stats(self):
        """({timer: median us}, {timer: max us}, samples) over the timed steps"""
        med, mx = (C.c_double * NUM_TIMERS)(), (C.c_double * NUM_TIMERS)()
        n = C.c_int64()
        self._ck(self.lib.psamd_get_timing_stats(self.h, med, mx, C.byref(n)))
        return dict(zip(TIMER_NAMES, list(med))), dict(zip(TIMER_NAMES, list(mx))), n.value
