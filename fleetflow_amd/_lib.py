"""ctypes binding of libfleetplace.so (include/fleetplace.h).

The product path has NO CPU fallback: if the HIP library is missing or no gfx950
device is present, calls raise.  The binding is the same one a Rust crate would
declare with ``extern "C"``.
"""
from __future__ import annotations

import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLEETPLACE_LIB selects another build of the same ABI (e.g. the diagnostics build
# libfleetplace_stats.so used by tools/pipe_stats.py); default is the release build.
LIB_PATH = os.environ.get("FLEETPLACE_LIB") or os.path.join(_HERE, "libfleetplace.so")

FP_OK, FP_EINVAL, FP_ENOMEM, FP_EDEVICE, FP_EOVERFLOW, FP_ECORRUPT = 0, -1, -2, -3, -4, -5
FP_NONE = 0xFFFFFFFF
REASON_OK, REASON_NOFIT, REASON_CYCLE, REASON_SKEW, REASON_QUOTA = 0, 1, 2, 3, 4
FP_K_PLACE, FP_K_SORT, FP_K_FEAS, FP_K_LEVEL, FP_K_GEN = 0, 1, 2, 3, 4
# scored placement (fleetplace.h enum fp_strategy, SPEC.md 2.6); the strings are the control plane's
# PlacementPolicy.strategy constants (crates/fleetflow-controlplane/src/model.rs:56-95)
STRATEGY_FIRST_FIT, STRATEGY_SPREAD, STRATEGY_PACK, STRATEGY_FILL_LOWEST = 0, 1, 2, 3
POLICY_STRATEGIES = {"spread_across_pool": STRATEGY_SPREAD, "pack_into_dedicated": STRATEGY_PACK,
                     "fill_lowest": STRATEGY_FILL_LOWEST}
FP_POLICY_MAX_NODES = 8192
# hard topology spread (SPEC.md 2.7): the domain ids of fp_place_policy_spread are below this
FP_SPREAD_MAX_DOMAINS = 64
# fallback chain (SPEC.md 2.8): at most this many hops, relax_mask rows hold this many words
FP_FALLBACK_MAX_HOPS = 4
# resource quota (SPEC.md 2.10): the dimension indices of a quota row (also the bits of quota_why), their
# names in that order, and the cap that is none
QUOTA_CPU, QUOTA_MEM, QUOTA_SERVICES, QUOTA_DIMS = 0, 1, 2, 3
QUOTA_NAMES = ("cpu", "memory", "services")
QUOTA_UNLIMITED = 0xFFFFFFFF
# rejection diagnosis (SPEC.md 2.9): fp_why bits, the word indices of an fp_explain row and of a histogram
WHY_CORDON, WHY_CPU, WHY_MEM, WHY_LABEL, WHY_CONFLICT = 1, 2, 4, 8, 16
EXPLAIN_FAIL, EXPLAIN_ONLY, EXPLAIN_FEASIBLE, EXPLAIN_ALL, EXPLAIN_MISSING, EXPLAIN_NEAR = 0, 5, 10, 11, 12, 13
EXPLAIN_WORDS = 16
EXPLAIN_HIST_MIXED, EXPLAIN_HIST_FITS, EXPLAIN_HIST_SELECTED, EXPLAIN_HIST_WORDS = 5, 6, 7, 8
# drain what-if sweep (SPEC.md 2.11): the word indices of a candidate's summary row, and their names in order
DRAIN_EVICTED, DRAIN_STRANDED, DRAIN_STRANDED_CPU, DRAIN_STRANDED_MEM = 0, 1, 2, 3
DRAIN_TARGETS, DRAIN_FIRST_STRANDED, DRAIN_NODES, DRAIN_WORDS = 4, 5, 6, 8
DRAIN_FIELDS = ("evicted", "stranded", "stranded_cpu", "stranded_mem", "targets", "first_stranded", "nodes")
# the drain sweep under the policy (SPEC.md 2.15): the word indices of a candidate's policy row, and their names
DRAIN_STRANDED_SKEW, DRAIN_RELAXED, DRAIN_SKEW_BEFORE, DRAIN_SKEW_AFTER, DRAIN_POLICY_WORDS = 0, 1, 2, 3, 4
DRAIN_POLICY_FIELDS = ("stranded_skew", "relaxed", "skew_before", "skew_after")
# scale-in sweep (SPEC.md 2.16): the word indices of a variant's summary row, their names in order, and the values
# of a node's state byte
SHRINK_RELEASED, SHRINK_TRIED, SHRINK_FAILED, SHRINK_MOVES, SHRINK_MOVED = 0, 1, 2, 3, 4
SHRINK_MOVED_CPU, SHRINK_MOVED_MEM, SHRINK_FIRST_FAILED, SHRINK_WORDS = 5, 6, 7, 8
SHRINK_FIELDS = ("released", "tried", "failed", "moves", "moved", "moved_cpu", "moved_mem", "first_failed")
SHRINK_STATE_NEVER, SHRINK_STATE_RELEASED, SHRINK_STATE_FAILED = 0, 1, 2
# the scale-in sweep under the policy (SPEC.md 2.17): the word indices of a variant's policy row, and their names
SHRINK_FAILED_SKEW, SHRINK_RELAXED, SHRINK_SKEW_BEFORE, SHRINK_SKEW_AFTER, SHRINK_POLICY_WORDS = 0, 1, 2, 3, 4
SHRINK_POLICY_FIELDS = ("failed_skew", "relaxed", "skew_before", "skew_after")
# rebalance sweep (SPEC.md 2.19): the word indices of a variant's summary row, and their names in order
REBAL_MOVES, REBAL_STUCK, REBAL_STUCK_SKEW, REBAL_RELAXED, REBAL_MOVED_CPU = 0, 1, 2, 3, 4
REBAL_MOVED_MEM, REBAL_SKEW_BEFORE, REBAL_SKEW_AFTER, REBAL_WORDS = 5, 6, 7, 8
REBAL_FIELDS = ("moves", "stuck", "stuck_skew", "relaxed", "moved_cpu", "moved_mem", "skew_before", "skew_after")
# scale-out sweep (SPEC.md 2.12): the word indices of a candidate's summary row, their names in order, and the
# most new servers a candidate may open
GROW_PENDING, GROW_PLACED, GROW_OPENED, GROW_UNPLACEABLE, GROW_CAPPED = 0, 1, 2, 3, 4
GROW_LEFT_CPU, GROW_LEFT_MEM, GROW_FIRST_UNPLACED, GROW_WORDS = 5, 6, 7, 8
GROW_FIELDS = ("pending", "placed", "opened", "unplaceable", "capped", "left_cpu", "left_mem", "first_unplaced")
GROW_MAX_NEW = 8192
# the scale-out sweep under the policy (SPEC.md 2.18): the word indices of a candidate's policy row, and their names
GROW_ON_LIVE, GROW_RELAXED, GROW_STUCK_SKEW, GROW_STUCK_QUOTA, GROW_SKEW_BEFORE, GROW_SKEW_AFTER = 0, 1, 2, 3, 4, 5
GROW_POLICY_WORDS = 8
GROW_POLICY_FIELDS = ("on_live", "relaxed", "stuck_skew", "stuck_quota", "skew_before", "skew_after")
# re-planning a running stage (SPEC.md 2.13): enum fp_change with its names in value order, and the word indices
# of a scenario's summary row (words 0..4 count the change values)
CHANGE_KEPT, CHANGE_NEW, CHANGE_MOVED, CHANGE_LOST, CHANGE_ABSENT = 0, 1, 2, 3, 4
CHANGE_NAMES = ("kept", "new", "moved", "lost", "absent")
REPLAN_KEPT, REPLAN_NEW, REPLAN_MOVED, REPLAN_LOST, REPLAN_ABSENT = 0, 1, 2, 3, 4
REPLAN_MOVED_CPU, REPLAN_MOVED_MEM, REPLAN_WORDS = 5, 6, 8
# context options (fleetplace.h enum fp_option); FP_OPT_AUTO = the production default
# ("segsort" is ignored by the library and kept for ABI stability)
FP_OPT_AUTO = -1
OPTIONS = {"pipe_w": 0, "pipe_seg": 1, "pipe_r": 2, "pipe_lag": 3, "link_slots": 4, "link_bounded": 5,
           "pipe_flush": 6, "spin_ticks": 7, "kpack": 8, "scen_sort": 9, "segsort": 10, "systolic": 11,
           "levelize_sync": 12, "systolic_extra": 13, "screen": 14, "payload_lds": 15, "systolic_valu": 16, "link_publish": 17,
           "level_sort": 18, "level_small": 19, "pipe_prio": 20,
           "indeg_bin": 21, "packed": 22, "sort_fused": 23, "prepack": 24}
# fp_place_geometry out[] (fleetplace.h FP_GEOM_*)
GEOM_FIELDS = ("groups", "stages", "segments", "ring", "lag", "link_slots", "bounded", "resident", "systolic")

u8p = ct.POINTER(ct.c_uint8)
u32p = ct.POINTER(ct.c_uint32)
u64p = ct.POINTER(ct.c_uint64)
vp = ct.c_void_p


class FpGraph(ct.Structure):
    _fields_ = [("n_vertices", ct.c_uint32), ("n_edges", ct.c_uint32), ("row_ptr", vp), ("col", vp),
                ("has_deps", vp)]


class FpContainers(ct.Structure):
    _fields_ = [("n", ct.c_uint32), ("cpu_m", vp), ("mem_mib", vp), ("req_labels", vp), ("conflict", vp)]


class FpNodes(ct.Structure):
    _fields_ = [("n", ct.c_uint32), ("cpu_free", vp), ("mem_free", vp), ("labels", vp),
                ("conflict_used", vp), ("schedulable", vp)]


class FpBatch(ct.Structure):
    _fields_ = [("n_scen", ct.c_uint32), ("scen_base", ct.c_uint32), ("n_containers", ct.c_uint32),
                ("n_nodes", ct.c_uint32),
                ("cpu_m", vp), ("mem_mib", vp), ("req_labels", vp), ("conflict", vp), ("level", vp),
                ("cpu_free", vp), ("mem_free", vp), ("labels", vp), ("conflict_used", vp),
                ("schedulable", vp), ("assign", vp), ("reason", vp), ("cost", vp)]


class FleetplaceError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = _lib_strerror(code) if _LIB is not None else str(code)
        super().__init__(f"{where}: {msg} ({code})")


_LIB = None

# name -> (restype, argtypes); the full export list of include/fleetplace.h
SIGNATURES = {
    "fp_ctx_create": (ct.c_int, [ct.POINTER(vp), ct.c_int]),
    "fp_ctx_destroy": (None, [vp]),
    "fp_ctx_set_stream": (ct.c_int, [vp, vp]),
    "fp_ctx_reset_stream": (ct.c_int, [vp]),
    "fp_ctx_sync": (ct.c_int, [vp]),
    "fp_strerror": (ct.c_char_p, [ct.c_int]),
    "fp_abi_version": (ct.c_int, []),
    "fp_ctx_profile": (ct.c_int, [vp, ct.c_int]),
    "fp_ctx_kernel_stats": (ct.c_int, [vp, ct.c_int, ct.POINTER(ct.c_double), ct.POINTER(ct.c_uint64)]),
    "fp_ctx_place_path": (ct.c_int, [vp, u32p]),
    "fp_ctx_set_option": (ct.c_int, [vp, ct.c_int, ct.c_int64]),
    "fp_ctx_get_option": (ct.c_int, [vp, ct.c_int, ct.POINTER(ct.c_int64)]),
    "fp_legacy_order": (ct.c_int, [vp, ct.POINTER(FpGraph), u32p]),
    "fp_levelize": (ct.c_int, [vp, ct.POINTER(FpGraph), u32p, u32p, u32p]),
    "fp_place": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, u8p]),
    "fp_place_batch": (ct.c_int, [vp, ct.POINTER(FpBatch)]),
    "fp_feasibility": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, u64p]),
    # output arrays as plain addresses (vp): a 3-service stage's call is on the config-1 clock
    "fp_plan_stage": (ct.c_int, [vp, ct.POINTER(FpGraph), ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp,
                                 vp, u32p, vp, vp, vp, vp]),
    "fp_dev_legacy_order": (ct.c_int, [vp, ct.POINTER(FpGraph), vp]),
    "fp_dev_levelize": (ct.c_int, [vp, ct.POINTER(FpGraph), vp, vp, vp]),
    "fp_dev_place_batch": (ct.c_int, [vp, ct.POINTER(FpBatch)]),
    "fp_place_ws_bytes": (ct.c_int, [vp, ct.c_uint32, ct.c_uint32, ct.c_uint32, u64p]),
    "fp_place_geometry": (ct.c_int, [vp, ct.c_uint32, ct.c_uint32, ct.c_uint32, u32p]),
    "fp_dev_feasibility": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, vp]),
    "fp_dev_feasibility_batch": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp]),
    "fp_place_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, ct.c_uint32, ct.c_uint32,
                                   u32p, u32p, u8p]),
    "fp_place_batch_policy": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p]),
    "fp_dev_place_batch_policy": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp]),
    "fp_place_policy_spread": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, ct.c_uint32,
                                          ct.c_uint32, u32p, u32p, ct.c_uint32, u32p, u8p]),
    "fp_place_batch_policy_spread": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p, u32p, u32p]),
    "fp_dev_place_batch_policy_spread": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp, vp, vp]),
    "fp_place_policy_fallback": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, ct.c_uint32,
                                            ct.c_uint32, u32p, u32p, ct.c_uint32, u32p, ct.c_uint32, u32p, u8p, u8p]),
    "fp_place_batch_policy_fallback": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p, u32p, u32p, u32p, u32p,
                                                  u8p]),
    "fp_dev_place_batch_policy_fallback": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp, vp, vp, vp, vp, vp]),
    "fp_place_policy_quota": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, ct.c_uint32,
                                         ct.c_uint32, u32p, u32p, ct.c_uint32, u32p, ct.c_uint32, u32p, u8p, u8p,
                                         u32p, u32p, u8p]),
    "fp_place_batch_policy_quota": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p, u32p, u32p, u32p, u32p,
                                               u8p, u32p, u32p, u8p]),
    "fp_dev_place_batch_policy_quota": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                   vp]),
    "fp_explain": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, ct.c_uint32, ct.c_uint32, u32p]),
    "fp_explain_batch": (ct.c_int, [vp, ct.POINTER(FpBatch), ct.c_uint32, u32p, u32p]),
    "fp_dev_explain": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, ct.c_uint32, ct.c_uint32, vp]),
    "fp_dev_explain_batch": (ct.c_int, [vp, ct.POINTER(FpBatch), ct.c_uint32, vp, vp]),
    "fp_drain_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                  ct.c_uint32, ct.c_uint32, u32p, u32p, u8p, u32p]),
    "fp_dev_drain_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, ct.c_uint32,
                                      ct.c_uint32, ct.c_uint32, vp, vp, vp, vp]),
    "fp_drain_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                         ct.c_uint32, ct.c_uint32, u32p, u32p, ct.c_uint32, u32p, ct.c_uint32, u32p,
                                         u8p, u8p, u32p, u32p]),
    # relax_mask (u32p) is a host array in the device entry too
    "fp_dev_drain_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, ct.c_uint32,
                                             ct.c_uint32, ct.c_uint32, vp, vp, ct.c_uint32, u32p, ct.c_uint32, vp,
                                             vp, vp, vp, vp]),
    "fp_shrink_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                   ct.c_uint32, ct.c_uint32, ct.c_uint32, u32p, u32p, u8p, u32p, u32p]),
    "fp_dev_shrink_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, ct.c_uint32,
                                       ct.c_uint32, ct.c_uint32, ct.c_uint32, vp, vp, vp, vp, vp]),
    "fp_shrink_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                          ct.c_uint32, ct.c_uint32, ct.c_uint32, u32p, u32p, ct.c_uint32, u32p,
                                          ct.c_uint32, u32p, u8p, u32p, u32p, u8p, u8p, u32p]),
    "fp_dev_shrink_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, ct.c_uint32,
                                              ct.c_uint32, ct.c_uint32, ct.c_uint32, vp, vp, ct.c_uint32, u32p,
                                              ct.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
    "fp_rebalance_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                      ct.c_uint32, u32p, ct.c_uint32, ct.c_uint32, u32p, u32p, ct.c_uint32, u32p,
                                      ct.c_uint32, u32p, u8p, u8p, u32p]),
    # relax_mask (u32p) is a host array in the device entry too
    "fp_dev_rebalance_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), vp, vp, ct.c_uint32,
                                          ct.c_uint32, vp, ct.c_uint32, ct.c_uint32, vp, vp, ct.c_uint32, u32p,
                                          ct.c_uint32, vp, vp, vp, vp]),
    "fp_grow_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), u8p, ct.c_uint32, ct.c_uint32, u32p, u32p, u32p, u32p,
                                 ct.c_uint32, u32p, u32p]),
    "fp_dev_grow_sweep": (ct.c_int, [vp, ct.POINTER(FpContainers), vp, ct.c_uint32, ct.c_uint32, vp, vp, vp, vp,
                                     ct.c_uint32, vp, vp]),
    "fp_grow_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), u8p, ct.c_uint32, ct.POINTER(FpNodes), u32p,
                                        ct.c_uint32, u32p, u32p, u32p, u32p, ct.c_uint32, ct.c_uint32, ct.c_uint32,
                                        u32p, u32p, ct.c_uint32, u32p, ct.c_uint32, u32p, u32p, u32p, u32p, u32p,
                                        u8p, u8p]),
    # relax_mask, quota and quota_used (u32p) are host arrays in the device entry too
    "fp_dev_grow_sweep_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), vp, ct.c_uint32, ct.POINTER(FpNodes), vp,
                                            ct.c_uint32, vp, vp, vp, vp, ct.c_uint32, ct.c_uint32, ct.c_uint32,
                                            vp, vp, ct.c_uint32, u32p, ct.c_uint32, u32p, u32p, vp, vp, vp, vp, vp]),
    "fp_replan": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32, ct.c_uint32,
                             u32p, u32p, u8p, u8p, u32p]),
    "fp_replan_batch": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p, u32p, u8p, u32p]),
    "fp_dev_replan_batch": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp, vp, vp, vp]),
    "fp_replan_policy": (ct.c_int, [vp, ct.POINTER(FpContainers), ct.POINTER(FpNodes), u32p, u32p, ct.c_uint32,
                                    ct.c_uint32, u32p, u32p, ct.c_uint32, u32p, ct.c_uint32, u32p, u8p, u8p, u32p, u32p,
                                    u8p, u8p, u32p]),
    "fp_replan_batch_policy": (ct.c_int, [vp, ct.POINTER(FpBatch), u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u8p,
                                          u32p, u32p, u8p, u8p, u32p]),
    "fp_dev_replan_batch_policy": (ct.c_int, [vp, ct.POINTER(FpBatch), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, vp]),
    "fp_dev_argmin_cost": (ct.c_int, [vp, vp, ct.c_uint32, vp]),
    "fp_dev_gen_batch": (ct.c_int, [vp, ct.c_uint64, ct.POINTER(FpBatch), ct.c_uint32]),
}


def load():
    """Load libfleetplace.so; raise loudly if it has not been built."""
    global _LIB
    if _LIB is None:
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.
        # Loading torch first makes our DT_NEEDED libamdhip64.so.7 bind to that same
        # runtime (same SONAME), so device pointers from torch tensors and from this
        # library live in one HIP context.  Loading ours first would leave torch with
        # a second runtime that finds no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        L = ct.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def raw_function(name):
    """A second handle to an export with no argtypes (no per-argument conversion on the call): the
    caller passes ctypes objects only.  For the per-plan fast path (Planner.plan_stage_lists)."""
    load()
    f = getattr(ct.CDLL(LIB_PATH), name)
    f.restype = ct.c_int
    f.argtypes = None
    return f


def _lib_strerror(code):
    return load().fp_strerror(code).decode()


def check(rc, where):
    if rc != FP_OK:
        raise FleetplaceError(rc, where)
