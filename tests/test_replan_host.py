"""Re-planning a running stage (SPEC.md 2.13) without a GPU: the theorems on the numpy reference
(tests/replan_ref.py), the reference anchored on the C oracle, hand-made cases (shared with the GPU tests), the
Planner wrappers' length checks and what they send to which export, ``replan_stage`` through a reference-backed
planner, the report's text and JSON forms, and the ABI's declarations."""
import ctypes as ct
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import replan_ref as RP  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402
from fleetflow_amd.planner import Planner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
KEPT, NEW, MOVED, LOST, ABSENT = RP.KEPT, RP.NEW, RP.MOVED, RP.LOST, RP.ABSENT
PREF2 = (1 << 4) | (1 << 8)


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def _nodes(cf, mf=None, lab=None, cu=None, sched=None):
    n = len(cf)
    return _u(cf, mf or [10 ** 6] * n, lab or [0] * n, cu or [0] * n) + (np.array(sched or [1] * n, np.uint8),)


def _cont(cpu, mem=None, req=None, conf=None):
    n = len(cpu)
    return _u(cpu, mem or [1] * n, req or [0] * n, conf or [0] * n)


def same(got, exp):
    """(assign, reason, change, summary, nodes_after, node_count_after), bit for bit."""
    for i in range(4):
        assert np.array_equal(got[i], exp[i]), i
    for i in range(5):
        assert np.array_equal(got[4][i], exp[4][i]), ("node table", i)
    assert np.array_equal(got[5], exp[5])


# ---- the theorems, on generated fleets ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fleet(seed, C, N):
    from oracle import pyoracle as P
    cont = tuple(np.array(x, np.uint32) for x in P.gen_containers(P.scenario_seed(seed, 0), C, 7))
    nodes = P.gen_nodes(P.scenario_seed(seed, 0), N)
    nodes = tuple(np.array(x, np.uint32) for x in nodes[:4]) + (np.array(nodes[4], np.uint8),)
    for a in cont + nodes:
        a.setflags(write=False)
    return cont, nodes


def grown(cont, seed=3):
    """The issue's perturbation: 15 % of the services ask for half as much CPU again, and 100 more."""
    g = np.random.default_rng(seed).random(cont[0].size) < 0.15
    cpu = cont[0].copy()
    cpu[g] = cpu[g] * 3 // 2 + 100
    return (cpu,) + tuple(cont[1:])


FLEETS = [(3, 600, 40), (9, 800, 100), (5, 384, 64)]


@pytest.mark.parametrize("seed,C,N", FLEETS)
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_1_no_prev_is_the_scored_placement(seed, C, N, strategy):
    cont, nodes = fleet(seed, C, N)
    cnt0 = (np.arange(N, dtype=np.uint32) * 7) % 5
    level = np.where(np.random.default_rng(1).random(C) < 0.05, NONE, 3).astype(np.uint32)
    a, r, after, cnt = R.place(cont, nodes, strategy, PREF2, level, cnt0)
    got = RP.replan(cont, nodes, np.full(C, NONE), strategy, PREF2, level, cnt0)
    same(got, (a, r, np.where(a != NONE, NEW, ABSENT), got[3], after, cnt))
    assert got[3].tolist() == [0, int((a != NONE).sum()), 0, 0, int((a == NONE).sum()), 0, 0, 0]
    assert RP.cost(got[0], got[1], 5) == R.cost(a, r, 5)


@pytest.mark.parametrize("seed,C,N", FLEETS)
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_2_a_plan_is_a_fixed_point(seed, C, N, strategy):
    cont, nodes = fleet(seed, C, N)
    cnt0 = (np.arange(N, dtype=np.uint32) * 7) % 5
    a, r, after, cnt = R.place(cont, nodes, strategy, PREF2, node_count=cnt0)
    got = RP.replan(cont, nodes, a, strategy, PREF2, node_count=cnt0)
    same(got, (a, r, np.where(a != NONE, KEPT, ABSENT), got[3], after, cnt))
    assert got[3][KEPT] == (a != NONE).sum() > 0 and got[3][NEW] == got[3][MOVED] == got[3][LOST] == 0


@pytest.mark.parametrize("seed,C,N", FLEETS)
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_3_a_lost_seat_is_never_taken_again(seed, C, N, strategy):
    cont, nodes = fleet(seed, C, N)
    a = R.place(cont, nodes, strategy)[0]
    got = RP.replan(grown(cont), nodes, a, strategy)
    moved = got[2] == MOVED
    assert moved.any() and (got[0][moved] != a[moved]).all()
    assert np.array_equal(got[0][got[2] == KEPT], a[got[2] == KEPT])


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_4_grow_then_replan_keeps_every_running_service(strategy):
    cont, nodes = fleet(3, 600, 40)
    a, r, _, _ = R.place(cont, nodes, strategy)
    more = tuple(np.append(x, v).astype(x.dtype) for x, v in zip(nodes, (64000, 1 << 20, 0, 0, 1)))
    got = RP.replan(cont, more, a, strategy)
    assert np.array_equal(got[0][a != NONE], a[a != NONE]) and (got[2][a != NONE] == KEPT).all()
    assert got[3][NEW] > 0 and (got[0][got[2] == NEW] != NONE).all()  # the unplaced find room on the new server


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_the_perturbed_fleet_has_every_kind_of_change(strategy):
    """The generated case of the GPU tests, on the reference: kept >= 364, moved >= 5, lost >= 30, new >= 11."""
    cont, nodes = fleet(3, 600, 40)
    a = R.place(cont, nodes, strategy)[0]
    s = RP.replan(grown(cont), nodes, a, strategy)[3]
    assert s[KEPT] >= 364 and s[MOVED] >= 5 and s[LOST] >= 30 and s[NEW] >= 11
    assert int(s[:5].sum()) == 600


@pytest.mark.parametrize("C,N,flags", [(600, 70, 7), (1, 1, 7), (300, 64, 0), (2000, 1025, 7)])
def test_theorem_1_first_fit_is_the_c_oracle(C, N, flags, O):
    cont, nodes = O.gen_scenario(0x5EED0013, 3, C, N, flags)
    level = np.where(np.random.default_rng(1).random(C) < 0.05, NONE, 3).astype(np.uint32)
    exp = O.place(cont, nodes, level=level)
    got = RP.replan(cont, nodes, np.full(C, NONE), R.FIRST_FIT, 0, level)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    for i in (0, 1, 3):
        assert np.array_equal(got[4][i], exp[2][i])


# ---- hand-made cases: (name, cont, nodes, prev, keywords, assign, reason, change) -----------------------------
HAND_CASES = [
    # node 0 has room for one of its two residents: the bigger one is visited first and keeps
    ("bigger keeps", _cont([30, 50]), _nodes([60, 100]), [0, 0], {}, [1, 0], [0, 0], [MOVED, KEPT]),
    ("index tie", _cont([40, 40]), _nodes([60, 100]), [0, 0], {}, [0, 1], [0, 0], [KEPT, MOVED]),
    # a cordoned node keeps what runs on it and receives nothing: first fit would give container 1 node 0
    ("cordoned seat", _cont([10, 10, 200]), _nodes([100, 100], sched=[0, 1]), [0, NONE, NONE], {},
     [0, 1, NONE], [0, 0, 1], [KEPT, NEW, ABSENT]),
    ("cordoned everywhere", _cont([10, 10]), _nodes([100], sched=[0]), [0, NONE], {}, [0, NONE], [0, 1], [KEPT, ABSENT]),
    ("new required label", _cont([10], req=[2]), _nodes([100, 100], lab=[1, 3]), [0], {}, [1], [0], [MOVED]),
    ("label nowhere", _cont([10], req=[4]), _nodes([100, 100], lab=[1, 3]), [0], {}, [NONE], [1], [LOST]),
    ("residents now anti-affine", _cont([20, 10], conf=[1 << 16, 1 << 16]), _nodes([100, 100]), [0, 0], {},
     [0, 1], [0, 0], [KEPT, MOVED]),
    ("seat against the base conflicts", _cont([10], conf=[1]), _nodes([100, 100], cu=[1, 0]), [0], {}, [1], [0], [MOVED]),
    # a CYCLE container takes no seat, so container 1 keeps the node they shared
    ("cycle", _cont([50, 50, 5]), _nodes([50]), [0, 0, NONE], {"level": [NONE, 0, NONE]}, [NONE, 0, NONE], [2, 0, 2],
     [LOST, KEPT, ABSENT]),
    ("spread sees the seats", _cont([10, 10, 10]), _nodes([100, 100, 100]), [0, 0, NONE], {"strategy": R.SPREAD},
     [0, 0, 1], [0, 0, 0], [KEPT, KEPT, NEW]),
    ("spread, counts given", _cont([10, 10, 10]), _nodes([100, 100, 100]), [0, 0, NONE],
     {"strategy": R.SPREAD, "node_count": [0, 1, 0]}, [0, 0, 2], [0, 0, 0], [KEPT, KEPT, NEW]),
    ("memory decides", _cont([10, 10], mem=[60, 50]), _nodes([100, 100], mf=[100, 100]), [0, 0], {"strategy": R.PACK},
     [0, 1], [0, 0], [KEPT, MOVED]),
    ("sums wrap", _cont([0xFFFFFFF0, 0x20], mem=[0x80000000, 0x80000001]),
     _nodes([0, 0, 0xFFFFFFFF, 0x20], mf=[0, 0, 0xFFFFFFFF, 0x80000001]), [0, 1], {}, [2, 3], [0, 0], [MOVED, MOVED]),
]


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_made_cases_on_the_reference(case):
    _, cont, nodes, prev, kw, assign, reason, change = case
    got = RP.replan(cont, nodes, prev, **kw)
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == (assign, reason, change)
    assert got[3][:5].tolist() == [change.count(v) for v in range(5)] and got[3][7] == 0
    moved = [i for i, c in enumerate(change) if c == MOVED]
    assert got[3][RP.MOVED_CPU] == sum(int(cont[0][i]) for i in moved) & NONE
    assert got[3][RP.MOVED_MEM] == sum(int(cont[1][i]) for i in moved) & NONE
    # the node table: the base table minus every assigned container's request
    cf, mf, cu = (x.astype(np.uint32).copy() for x in (nodes[0], nodes[1], nodes[3]))
    cnt = np.array(kw.get("node_count", [0] * cf.size), np.uint32)
    for i, n in enumerate(assign):
        if n != NONE:
            cf[n:n + 1] -= cont[0][i]
            mf[n:n + 1] -= cont[1][i]
            cu[n] |= cont[3][i]
            cnt[n] += 1
    assert np.array_equal(got[4][0], cf) and np.array_equal(got[4][1], mf) and np.array_equal(got[4][3], cu)
    assert np.array_equal(got[5], cnt)


def test_the_wrapping_case_counts_its_migration_volume():
    got = RP.replan(*HAND_CASES[-1][1:4])
    assert got[3].tolist() == [0, 0, 2, 0, 0, 0x10, 0x1, 0]


# ---- the wrappers: length checks first, then what reaches the export ---------------------------------------
class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def _addr(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "_obj"):
        return ct.addressof(x._obj)
    return ct.cast(x, ct.c_void_p).value or 0


class _Rec:
    """Stands in for the library: records (name, args, the u32 words of the peeked arguments)."""

    def __init__(self, peek=None):
        self.calls, self.peek = [], peek or {}

    def __getattr__(self, name):
        def export(*args):
            seen = {i: list(ct.cast(ct.c_void_p(_addr(args[i])), ct.POINTER(ct.c_uint32))[:n])
                    for i, n in self.peek.items()}
            self.calls.append((name, args, seen))
            return 0
        return export


def _planner(lib):
    q = object.__new__(Planner)
    q._L, q._ctx, q._tstream, q.device = lib, ct.c_void_p(0x5EED), None, 0
    q._dev = lambda fn, *a: fn(*a)
    return q


def _refused(msg, fn, *a, **kw):
    with pytest.raises(ValueError, match=re.escape(msg)):
        fn(*a, **kw)


def test_replan_length_checks():
    p = _planner(_NoLib())
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    for i in range(4):
        short = cont[:i] + (cont[i][:-1],) + cont[i + 1:]
        _refused("every container array must hold C entries", p.replan, short, nodes, [0, 0])
    for i in range(5):
        short = nodes[:i] + (nodes[i][:-1],) + nodes[i + 1:]
        _refused("every node array must hold N entries", p.replan, cont, short, [0, 0])
    _refused("prev must hold C entries", p.replan, cont, nodes, [0])
    _refused("prev must hold C entries", p.replan, cont, nodes, [0, 0, 0])
    _refused("level must hold C entries", p.replan, cont, nodes, [0, 0], level=[0])
    _refused("node_count must hold N entries", p.replan, cont, nodes, [0, 0], node_count=[0] * 4)
    with pytest.raises(ValueError, match="unknown placement strategy"):
        p.replan(cont, nodes, [0, 0], strategy="round_robin")
    b = (2, 2, 3, tuple(np.tile(x, 2) for x in cont), tuple(np.tile(x, 2) for x in nodes))
    _refused("prev must hold S * C entries", p.replan_batch, *b, [0, 0], [0, 0])
    _refused("strategy and preferred must hold S entries", p.replan_batch, *b, [0] * 4, [0])
    _refused("strategy and preferred must hold S entries", p.replan_batch, *b, [0] * 4, [0, 0], preferred=[0])
    _refused("node_count must hold S * N entries", p.replan_batch, *b, [0] * 4, [0, 0], node_count=[0] * 3)
    _refused("level must hold S * C entries", p.replan_batch, *b, [0] * 4, [0, 0], level=[0] * 3)
    _refused("every container array must hold S * C entries", p.replan_batch, 3, 2, 3, b[3], b[4], [0] * 6, [0] * 3)


def test_replan_call():
    lib = _Rec(peek={4: 2, 7: 3})
    p = _planner(lib)
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    assign, reason, change, summary, after, nc = p.replan(cont, nodes, [2, NONE], "fill_lowest", -1, [0, NONE], [4, 5, 6])
    (name, args, seen), = lib.calls
    assert name == "fp_replan" and len(args) == 12 == len(_lib.SIGNATURES[name][1]) and _addr(args[0]) == 0x5EED
    assert seen == {4: [2, NONE], 7: [4, 5, 6]} and args[5:7] == (_lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, ns.n) == (2, 3) and cs.cpu_m == cont[0].ctypes.data and ns.labels == nodes[2].ctypes.data
    assert ns.cpu_free == after[0].ctypes.data != nodes[0].ctypes.data  # the mutable node fields are copies
    assert [_addr(args[i]) for i in (7, 8, 9, 10, 11)] == [x.ctypes.data for x in (nc, assign, reason, change, summary)]
    assert (assign.dtype, reason.dtype, change.dtype, change.shape, summary.dtype, summary.shape) == (
        np.uint32, np.uint8, np.uint8, (2,), np.uint32, (_lib.REPLAN_WORDS,))
    lib = _Rec()
    p = _planner(lib)
    out = p.replan(cont, nodes, [0, 1], want_change=False, want_summary=False)
    args = lib.calls[0][1]
    assert args[5:7] == (0, 0) and [_addr(args[i]) for i in (3, 7, 10, 11)] == [0] * 4  # level, counts, change, summary
    assert out[2] is None and out[3] is None and out[5] is None


def test_replan_batch_call():
    lib = _Rec(peek={2: 4, 3: 2, 4: 2})
    p = _planner(lib)
    cont, nodes = tuple(np.tile(x, 2) for x in _cont([1, 1])), tuple(np.tile(x, 2) for x in _nodes([9, 9, 9]))
    out = p.replan_batch(2, 2, 3, cont, nodes, [0, NONE, 2, 1], ["pack_into_dedicated", 1], [7, 8], scen_base=5)
    (name, args, seen), = lib.calls
    assert name == "fp_replan_batch" and len(args) == 8 == len(_lib.SIGNATURES[name][1])
    assert seen == {2: [0, NONE, 2, 1], 3: [_lib.STRATEGY_PACK, 1], 4: [7, 8]} and _addr(args[5]) == 0
    b = args[1]._obj
    assert (b.n_scen, b.scen_base, b.n_containers, b.n_nodes) == (2, 5, 2, 3)
    assign, reason, cost, change, summary, after, nc = out
    assert (b.assign, b.reason, b.cost) == (assign.ctypes.data, reason.ctypes.data, cost.ctypes.data)
    assert [_addr(args[6]), _addr(args[7])] == [change.ctypes.data, summary.ctypes.data]
    assert change.shape == (4,) and summary.shape == (2, _lib.REPLAN_WORDS) and cost.shape == (2,) and nc is None
    lib = _Rec()
    p = _planner(lib)
    out = p.replan_batch(2, 2, 3, cont, nodes, [0] * 4, [0, 0], want_change=False, want_summary=False)
    assert [_addr(lib.calls[0][1][i]) for i in (4, 5, 6, 7)] == [0] * 4 and out[3] is None and out[4] is None


def test_dev_replan_batch_call_and_checks():
    torch = pytest.importorskip("torch")
    from fleetflow_amd.planner import DevBatch
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    S, C, N = 2, 3, 4
    db = DevBatch.allocate(S, C, N, "cpu", scen_base=3)
    prev, st, pf, cnt, chg, sm = i32(S * C), i32(S), i32(S), i32(S * N), u8(S * C), i32(S * 8)
    lib = _Rec()
    q = _planner(lib)  # kept: a planner that goes away closes its context through the library
    q.dev_replan_batch(db, prev, st, pf, cnt, chg, sm)
    (name, args, _), = lib.calls
    assert name == "fp_dev_replan_batch" and len(args) == 8 == len(_lib.SIGNATURES[name][1])
    b = args[1]._obj
    assert (b.n_scen, b.scen_base, b.n_containers, b.n_nodes, b.cpu_m, b.assign) == (
        S, 3, C, N, db.cpu.data_ptr(), db.assign.data_ptr())
    assert [_addr(a) for a in args[2:]] == [t.data_ptr() for t in (prev, st, pf, cnt, chg, sm)]
    q.dev_replan_batch(db, prev, st)
    assert [_addr(a) for a in lib.calls[1][1][4:]] == [0] * 4
    fn = _planner(_NoLib()).dev_replan_batch
    _refused("prev_t must hold S * C 32-bit entries", fn, db, i32(S * C - 1), st)
    _refused("prev_t must hold S * C 32-bit entries", fn, db, u8(S * C), st)
    _refused("strategy_t must hold S entries", fn, db, prev, i32(S + 1))
    _refused("preferred_t must hold S entries", fn, db, prev, st, i32(1))
    _refused("count_t must hold S * N entries", fn, db, prev, st, None, i32(N))
    _refused("change_t must hold S * C bytes", fn, db, prev, st, change_t=i32(S * C))
    _refused("summary_t must hold S * 8 32-bit entries", fn, db, prev, st, summary_t=i32(S * 8 - 1))


def test_abi_declares_the_replan_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    assert "int fp_replan(fp_ctx *ctx, const fp_containers *c, fp_nodes *nodes, const uint32_t *level, const uint32_t *prev" in hdr
    for name in ("fp_replan_batch", "fp_dev_replan_batch"):
        assert f"int {name}(fp_ctx *ctx, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy" in hdr
    for name in ("fp_replan", "fp_replan_batch", "fp_dev_replan_batch"):
        assert name in _lib.SIGNATURES and f"pub fn {name}(" in ffi
    assert "model.rs:435-442" in hdr and "model.rs:421-427" in hdr and "ffi::fp_replan(" in lib
    assert "#define FP_ABI_VERSION 1" in hdr
    words = dict(re.findall(r"(FP_REPLAN_\w+) = (\d+)", hdr))
    assert words == {"FP_REPLAN_KEPT": "0", "FP_REPLAN_NEW": "1", "FP_REPLAN_MOVED": "2", "FP_REPLAN_LOST": "3",
                     "FP_REPLAN_ABSENT": "4", "FP_REPLAN_MOVED_CPU": "5", "FP_REPLAN_MOVED_MEM": "6", "FP_REPLAN_WORDS": "8"}
    for name, val in words.items():
        assert getattr(_lib, name[3:]) == int(val)
        assert re.search(rf"pub const {name}: usize = {val};", ffi), name
    assert (RP.MOVED_CPU, RP.MOVED_MEM, RP.WORDS) == (_lib.REPLAN_MOVED_CPU, _lib.REPLAN_MOVED_MEM, _lib.REPLAN_WORDS)
    changes = dict(re.findall(r"(FP_CHANGE_\w+) = (\d+)", hdr))
    assert changes == {"FP_CHANGE_KEPT": "0", "FP_CHANGE_NEW": "1", "FP_CHANGE_MOVED": "2", "FP_CHANGE_LOST": "3",
                       "FP_CHANGE_ABSENT": "4"}
    for name, val in changes.items():
        assert getattr(_lib, name[3:]) == int(val) == getattr(RP, name[10:])
        assert re.search(rf"pub const {name}: u8 = {val};", ffi), name
    assert _lib.CHANGE_NAMES == ("kept", "new", "moved", "lost", "absent")
    mk = open(os.path.join(ROOT, "fleetflow_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS := .*\bfp_replan\.hip\b", mk, re.M)


# ---- the flow level ------------------------------------------------------------------------------------
class _RefPlanner:
    """replan answered by the numpy reference and the graph by the Python oracle; remembers what it was asked."""

    def plan_stage(self, row_ptr, col, has_deps, cont=None, nodes=None):
        from oracle import pyoracle as P
        assert cont is None and nodes is None
        level, order = P.levelize(len(has_deps), list(row_ptr), list(col), list(has_deps))
        return np.array(P.legacy_order(has_deps)), np.array(level, np.uint32), np.array(order), 0, None

    def replan(self, cont, nodes, prev, strategy=0, preferred=0, level=None, node_count=None):
        self.asked = (cont, nodes, prev, strategy, preferred, level, node_count)
        return RP.replan(cont, nodes, prev, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred, level, node_count)


def _flow():
    f = F.Flow("shop")
    spec = {"db": (3000, 4096, ["class=ssd"], None), "api": (1000, 1024, [], "web"), "web": (1000, 512, [], "web"),
            "cache": (500, 2048, [], None), "cron": (250, 128, [], None), "batch": (2500, 1024, [], None)}
    for name, (cpu, mem, labels, group) in spec.items():
        f.services[name] = F.Service(cpu_m=cpu, mem_mib=mem, labels=labels, anti_affinity=group)
    servers = [("a1", 4000, 8192, ["region=east", "class=ssd"]), ("a2", 4000, 8192, ["region=east"]),
               ("b1", 4000, 8192, ["region=west"]), ("b2", 2000, 4096, ["region=west"])]
    for slug, cpu, mem, labels in servers:
        f.servers[slug] = F.Server(slug, cpu, mem, labels)
    f.stages["live"] = F.Stage(services=list(spec), servers=[s[0] for s in servers])
    return f


def _first_plan(f, policy=None):
    """The stage's plan by policy_ref.place, as a flow.Plan."""
    policy = policy or F.PlacementPolicy()
    stage = f.stages["live"]
    nodes = [f.servers[s] for s in stage.servers]
    cont, ntab = F._stage_tables(stage.services, f, nodes, policy.preferred)
    pmask = F._stage_labels(stage.services, f, nodes, policy.preferred).mask(policy.preferred)
    a, _, _, _ = R.place(cont, ntab, _lib.POLICY_STRATEGIES.get(policy.strategy, 0), pmask)
    plan = F.Plan("live", [], {}, [], {n: stage.servers[a[v]] for v, n in enumerate(stage.services) if a[v] != NONE},
                  {n: "NOFIT" for v, n in enumerate(stage.services) if a[v] == NONE})
    plan.strategy, plan.preferred = policy.strategy, policy.preferred
    return plan


def test_replan_stage_keeps_moves_and_reports():
    f = _flow()
    plan = _first_plan(f)
    assert len(plan.assignment) == 6  # every service is placed
    p = _RefPlanner()
    rep = F.replan_stage(f, "live", plan, planner=p)
    assert rep.kept == list(f.stages["live"].services) and not (rep.new or rep.moved or rep.lost)  # theorem 2
    assert rep.plan.assignment == plan.assignment and rep.plan.rejected == {} and rep.plan.stage == "live"
    assert rep.plan.order == list(f.stages["live"].services) and set(rep.plan.levels.values()) == {0}
    assert (rep.moved_cpu_m, rep.moved_mem_mib) == (0, 0)
    slugs = f.stages["live"].servers
    assert p.asked[2] == [slugs.index(plan.assignment[n]) for n in f.stages["live"].services]
    assert [int(x) for x in p.asked[1][0]] == [4000, 4000, 4000, 2000]  # the base table, nothing deducted
    # one service asks for more than its server has left: it alone moves
    home = plan.assignment["cache"]
    f.services["cache"].cpu_m = 2100
    rep2 = F.replan_stage(f, "live", plan, planner=p)
    assert [m[:2] for m in rep2.moved] == [("cache", home)] and rep2.moved[0][2] != home
    assert sorted(rep2.kept) == sorted(n for n in plan.assignment if n != "cache") and not rep2.lost and not rep2.new
    assert (rep2.moved_cpu_m, rep2.moved_mem_mib) == (2100, 2048)
    assert rep2.plan.assignment["cache"] == rep2.moved[0][2]
    # the new plan goes straight into the next re-plan, and into a drain sweep's live tables
    rep3 = F.replan_stage(f, "live", rep2.plan, planner=p)
    assert sorted(rep3.kept) == sorted(plan.assignment) and rep3.plan.assignment == rep2.plan.assignment
    assert F.live_tables(f, "live", rep2.plan)[4] == [slugs.index(rep2.plan.assignment[n]) for n in f.stages["live"].services]
    # a service that did not run is new; one that no server takes any more is lost
    f.services["extra"] = F.Service(cpu_m=100, mem_mib=64)
    f.stages["live"].services.append("extra")
    f.services["db"].cpu_m = 5000
    rep4 = F.replan_stage(f, "live", rep2.plan, planner=p)
    assert rep4.new == ["extra"] and rep4.lost == [("db", plan.assignment["db"], "NOFIT")]
    assert rep4.plan.rejected == {"db": "NOFIT"} and "db" not in rep4.plan.assignment


def test_replan_stage_cordoned_draining_and_vanished_servers():
    f = _flow()
    plan = _first_plan(f, F.PlacementPolicy("spread_across_pool"))
    assert set(plan.assignment.values()) == {"a1", "a2", "b1", "b2"}
    on = {s: [n for n in f.stages["live"].services if plan.assignment[n] == s] for s in f.stages["live"].servers}
    p = _RefPlanner()
    # cordon: existing placements continue
    f.servers["a2"].schedulable = False
    rep = F.replan_stage(f, "live", plan, planner=p)
    assert rep.kept == list(f.stages["live"].services) and p.asked[3] == "spread_across_pool"
    # drain: they leave -- no seat at the ABI, moved (from the old slug) or lost on the host
    f.servers["a2"].draining = True
    rep = F.replan_stage(f, "live", plan, planner=p)
    idx = {n: v for v, n in enumerate(f.stages["live"].services)}
    assert all(p.asked[2][idx[n]] == NONE for n in on["a2"]) and on["a2"]
    assert sorted(m[0] for m in rep.moved) + sorted(x[0] for x in rep.lost) == sorted(on["a2"])
    assert all(m[1] == "a2" and m[2] != "a2" for m in rep.moved) and all(x[1] == "a2" for x in rep.lost)
    assert not rep.new and sorted(rep.kept) == sorted(n for n in idx if n not in on["a2"])
    cpu = sum(f.services[m[0]].cpu_m for m in rep.moved)
    assert rep.moved and rep.moved_cpu_m == cpu and rep.moved_mem_mib == sum(f.services[m[0]].mem_mib for m in rep.moved)
    # a server that is no longer in the stage: the same
    f.servers["a2"].draining = False
    f.stages["live"].servers.remove("b1")
    rep = F.replan_stage(f, "live", plan, planner=p)
    assert all(p.asked[2][idx[n]] == NONE for n in on["b1"]) and len(p.asked[1][0]) == 3
    assert sorted([m[0] for m in rep.moved] + [x[0] for x in rep.lost]) == sorted(on["b1"])
    assert all(m[1] == "b1" for m in rep.moved) and all(x[1:] == ("b1", "NOFIT") for x in rep.lost)
    assert "b1" not in rep.plan.assignment.values()
    # no servers at all: everything that ran is lost, nothing is asked of the planner
    f.stages["live"].servers.clear()
    del p.asked
    rep = F.replan_stage(f, "live", plan, planner=p)
    assert sorted(x[0] for x in rep.lost) == sorted(plan.assignment) and not rep.plan.assignment and not hasattr(p, "asked")


def test_replan_stage_cycle_members_are_lost():
    f = _flow()
    plan = _first_plan(f)
    f.services["api"].depends_on = ["web"]
    f.services["web"].depends_on = ["api"]
    rep = F.replan_stage(f, "live", plan, planner=_RefPlanner())
    assert sorted(rep.lost) == sorted([("api", plan.assignment["api"], "CYCLE"), ("web", plan.assignment["web"], "CYCLE")])
    assert rep.plan.rejected == {"api": "CYCLE", "web": "CYCLE"} and rep.plan.levels["api"] == NONE
    assert sorted(rep.kept) == ["batch", "cache", "cron", "db"]


def test_replan_stage_refuses_to_drop_a_hard_guarantee():
    f = _flow()
    plan = _first_plan(f)
    p = _RefPlanner()
    for policy, what in ((F.PlacementPolicy(spread_topology_key="region", spread_max_skew=1), "spread constraint"),
                         (F.PlacementPolicy(fallback_relax_order=("class",)), "fallback chain"),
                         (F.PlacementPolicy(quota_services=3), "resource quota")):
        with pytest.raises(ValueError, match=what):
            F.replan_stage(f, "live", plan, planner=p, policy=policy)
    both = F.PlacementPolicy("fill_lowest", spread_topology_key="region", spread_max_skew=2, quota_cpu_m=9000)
    with pytest.raises(ValueError, match="spread constraint and the resource quota of the policy"):
        F.replan_stage(f, "live", plan, planner=p, policy=both)
    assert not hasattr(p, "asked")  # refused before anything is planned
    # a plan made under one, when no policy is given
    for field, value, what in (("spread_topology_key", "region", "spread constraint"),
                               ("fallback_relax_order", ["class"], "fallback chain"), ("quota", (None, None, 3), "resource quota")):
        made = _first_plan(f)
        setattr(made, field, value)
        if field == "spread_topology_key":
            made.spread_max_skew = 1
        with pytest.raises(ValueError, match=what + " of the plan"):
            F.replan_stage(f, "live", made, planner=p)
        # an explicit policy without it re-plans
        assert F.replan_stage(f, "live", made, planner=p, policy=F.PlacementPolicy("fill_lowest")).plan.strategy == "fill_lowest"
    # a spread of max_skew 0 and a chain of max_hops 0 constrain nothing
    idle = F.PlacementPolicy("pack_into_dedicated", spread_topology_key="region", spread_max_skew=0,
                             fallback_relax_order=("class",), fallback_max_hops=0)
    assert F.replan_stage(f, "live", plan, planner=p, policy=idle).kept


def test_replan_stage_policy_and_preferred_labels():
    f = _flow()
    policy = F.PlacementPolicy("fill_lowest", {"region": "west"})
    plan = _first_plan(f, policy)
    p = _RefPlanner()
    rep = F.replan_stage(f, "live", plan, planner=p)
    nodes = [f.servers[s] for s in f.stages["live"].servers]
    pmask = F._stage_labels(f.stages["live"].services, f, nodes, policy.preferred).mask(policy.preferred)
    assert p.asked[3:5] == ("fill_lowest", pmask) and pmask != 0
    assert (rep.plan.strategy, rep.plan.preferred) == ("fill_lowest", ["region=west"])
    F.replan_stage(f, "live", plan, planner=p, policy=F.PlacementPolicy())
    assert p.asked[3:5] == (0, 0)
    assert F.replan_stage(F.Flow("x", stages={"s": F.Stage()}), "s", plan, planner=p).plan.order == []


def test_report_text_and_json_round_trip():
    plan = F.Plan("live", ["db", "api", "web", "new1"], {"db": 0, "api": 1, "web": NONE, "new1": 0}, ["db", "new1", "api"],
                  {"db": "a1", "api": "b1", "new1": "a2"}, {"web": "CYCLE", "old": "NOFIT"}, strategy="fill_lowest",
                  preferred=["class=ssd"])
    rep = F.Replan(plan, ["db"], ["new1"], [("api", "a2", "b1")], [("web", "a1", "CYCLE"), ("old", "b2", "NOFIT")], 1000, 1024)
    assert PO.format_replan_report(rep) == (
        "replan live: 1 kept, 1 new, 1 moved (1000m cpu, 1024 MiB), 2 lost\n"
        "  api: a2 -> b1\n"
        "  new1: -> a2\n"
        "  web: a1 -> lost (CYCLE)\n"
        "  old: b2 -> lost (NOFIT)")
    text = PO.replan_report_to_json(rep)
    back = PO.replan_report_from_json(text)
    assert back == rep and isinstance(back.moved[0], tuple) and isinstance(back.lost[0], tuple)
    assert PO.replan_report_to_json(back) == text and PO.replan_report_to_json(rep, indent=2) != text
    empty = F.Replan(F.Plan("s", [], {}, [], {}, {}))
    assert PO.replan_report_from_json(PO.replan_report_to_json(empty)) == empty
    assert PO.format_replan_report(empty) == "replan s: 0 kept, 0 new, 0 moved (0m cpu, 0 MiB), 0 lost"
