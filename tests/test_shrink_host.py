"""CPU tests of the scale-in sweep (SPEC.md 2.16): the numpy reference (tests/shrink_ref.py) against the
section's theorems and hand-made traps, the Planner wrappers' checks and calls, and flow.shrink_stage with its
report.  No GPU and no library: the wrappers talk to a recording stand-in."""
import ctypes as ct
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import policy_ref as R  # noqa: E402
import shrink_ref as S  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402
from fleetflow_amd.planner import Planner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def _nodes(cf, mf=None, lab=None, cu=None, sched=None):
    n = len(cf)
    return _u(cf, mf or [1 << 20] * n, lab or [0] * n, cu or [0] * n) + (np.array(sched or [1] * n, np.uint8),)


def _cont(cpu, mem=None, req=None, conf=None):
    n = len(cpu)
    return _u(cpu, mem or [1] * n, req or [0] * n, conf or [0] * n)


# ---- the random cases, and the conditions that keep them from being vacuous --------------------------------
@functools.lru_cache(maxsize=None)
def _case(seed, strategy):
    cont, live, assign, cnt, order = S.random_case(seed, strategy)
    return cont, live, assign, cnt, order, S.variant(cont, live, assign, order, strategy, 0, cnt)


CASES = [(seed, st) for seed in range(6) for st in R.STRATEGIES]


def _moves_twice(cont, live, assign, cnt, order, strategy):
    """Containers that change node in two committed attempts of the variant."""
    times = np.zeros(assign.size, np.int64)
    for i in range(1, len(order) + 1):
        prev = S.variant(cont, live, assign, order[:i - 1], strategy, 0, cnt)[0]
        times += S.variant(cont, live, assign, order[:i], strategy, 0, cnt)[0] != prev
    return int((times >= 2).sum())


@pytest.mark.parametrize("seed,strategy", CASES)
def test_random_cases_are_not_vacuous(seed, strategy):
    cont, live, assign, cnt, order, (out, state, blocker, row, trace, _) = _case(seed, strategy)
    done = [t[1] for t in trace]
    assert any(done), "no committed attempt"
    assert any(not d for d in done[done.index(True):]), "no failed attempt after a commit"
    assert any(not d and made > 0 for _, d, made in trace), "no failed attempt that moved something first"
    assert row[S.MOVES] > row[S.MOVED] or _moves_twice(cont, live, assign, cnt, order, strategy) > 0, "no double move"
    assert row[S.RELEASED] + row[S.FAILED] == row[S.TRIED] == len(trace)


# ---- theorem D: the plan a variant ends with is one the base allows --------------------------------------------
def check_valid(cont, live, assign, out, state):
    cpu, mem, req, conf = cont
    cf, mf, lab, cu, sched = live
    N = cf.size
    assert np.array_equal(out == NONE, assign == NONE)  # nothing is lost, nothing starts
    for n in range(N):
        here, was = np.flatnonzero(out == n), np.flatnonzero(assign == n)
        assert int(cpu[here].astype(np.int64).sum()) <= int(cf[n]) + int(cpu[was].astype(np.int64).sum())
        assert int(mem[here].astype(np.int64).sum()) <= int(mf[n]) + int(mem[was].astype(np.int64).sum())
        new = np.setdiff1d(here, was)
        assert ((lab[n] & req[new]) == req[new]).all()
        assert int(conf[here].astype(np.int64).sum()) == int(np.bitwise_or.reduce(conf[here], initial=0))  # disjoint
        # what came must not collide with what the base holds there from containers outside the table either
        mine = int(np.bitwise_or.reduce(conf[was], initial=0))
        assert (conf[new] & (int(cu[n]) & ~mine)).sum() == 0
        if state[n] == S.ST_RELEASED:
            assert here.size == 0
        if new.size:
            assert sched[n] != 0
    assert ((state == S.ST_RELEASED) | (state == S.ST_FAILED) | (state == S.ST_NEVER)).all()


@pytest.mark.parametrize("seed,strategy", CASES)
def test_theorem_d_validity(seed, strategy):
    cont, live, assign, cnt, order, (out, state, blocker, row, trace, _) = _case(seed, strategy)
    check_valid(cont, live, assign, out, state)
    moved = np.flatnonzero(out != assign)
    assert row[S.MOVED] == moved.size and row[S.MOVED_CPU] == int(cont[0][moved].sum()) & NONE
    assert ((blocker != NONE) == (state == S.ST_FAILED)).all()
    assert (assign[blocker[state == S.ST_FAILED]] != NONE).all()


# ---- theorem A: one attempt is one drain candidate ----------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_a_drain_anchor(strategy):
    cont, live, assign, cnt, order = S.random_case(1, strategy, 300, 22)  # tight: some servers cannot leave alone
    N = live[0].size
    seen = set()
    for n in range(N):
        out, state, blocker, row, _, _ = S.variant(cont, live, assign, [n], strategy, 5, cnt)
        group = np.where(np.arange(N) == n, 0, NONE).astype(np.uint32)
        d_out, _, d_rows = D.sweep(cont, live, assign, group, 1, strategy, 5, cnt)
        if d_rows[0, D.STRANDED] == 0:
            assert np.array_equal(out, d_out) and row[:3].tolist() == [1, 1, 0] and state[n] == S.ST_RELEASED
            assert row[S.MOVES] == row[S.MOVED] == d_rows[0, D.EVICTED] and row[S.FIRST_FAILED] == NONE
        else:
            assert np.array_equal(out, assign) and row[:5].tolist() == [0, 1, 1, 0, 0] and state[n] == S.ST_FAILED
            assert blocker[n] == d_rows[0, D.FIRST_STRANDED] and row[S.FIRST_FAILED] == n
        seen.add(int(state[n]))
        assert (np.delete(state, n) == S.ST_NEVER).all() and (np.delete(blocker, n) == NONE).all()
    assert seen == {S.ST_RELEASED, S.ST_FAILED}


# ---- theorem B: a failed attempt leaves nothing behind -----------------------------------------------------------
def check_undo(run, order, at, N):
    """run(order) -> (out, state, blocker, row); ``order`` names every node once and its attempt number ``at``
    fails.  The variant with that entry taken out ends the same."""
    tried = [int(n) for n in order]
    assert len(set(tried)) == len(tried) and NONE not in tried
    x = tried[at]
    with_x, without = run(tried), run(tried[:at] + tried[at + 1:])
    assert np.array_equal(with_x[0], without[0])
    rest = np.arange(N) != x
    assert np.array_equal(with_x[1][rest], without[1][rest]) and np.array_equal(with_x[2][rest], without[2][rest])
    assert with_x[1][x] == S.ST_FAILED and without[1][x] == S.ST_NEVER
    a, b = with_x[3].astype(np.int64), without[3].astype(np.int64)
    assert (a - b)[[S.RELEASED, S.MOVES, S.MOVED, S.MOVED_CPU, S.MOVED_MEM]].tolist() == [0] * 5
    assert (a - b)[[S.TRIED, S.FAILED]].tolist() == [1, 1]
    assert with_x[3][S.FIRST_FAILED] == x or with_x[3][S.FIRST_FAILED] == without[3][S.FIRST_FAILED]


@pytest.mark.parametrize("seed,strategy", CASES)
def test_theorem_b_undo_is_exact(seed, strategy):
    cont, live, assign, cnt, order, ref = _case(seed, strategy)
    run = lambda o: S.variant(cont, live, assign, o, strategy, 0, cnt)[:4]  # noqa: E731
    first = next(i for i, t in enumerate(ref[4]) if not t[1])
    partial = next(i for i, t in enumerate(ref[4]) if not t[1] and t[2] > 0)  # it had moved something before its blocker
    for at in {first, partial}:
        check_undo(run, order, at, live[0].size)


# ---- theorem C: a committed attempt is a drain, step by step ------------------------------------------------------
def stepwise(cont, live, assign, order, strategy, preferred, cnt):
    """The variant as the host loop it replaces: one single-candidate drain per attempt (drain_ref), its moves
    applied to the tables as Planner.drain applies them, the released node made unschedulable."""
    cf, mf, lab, cu, sched = (np.array(x) for x in live)
    cur, cnt = np.array(assign), np.array(cnt)
    state = np.zeros(cf.size, np.uint8)
    for n in (int(x) for x in order):
        if n == NONE or state[n] == S.ST_RELEASED:
            continue
        group = np.where(np.arange(cf.size) == n, 0, NONE).astype(np.uint32)
        out, _, rows = D.sweep(cont, (cf, mf, lab, cu, sched), cur, group, 1, strategy, preferred, cnt)
        if rows[0, D.STRANDED]:
            state[n] = S.ST_FAILED
            continue
        for c in np.flatnonzero(out != cur):
            t = int(out[c])
            cf[t] -= cont[0][c]
            mf[t] -= cont[1][c]
            cu[t] |= cont[3][c]
            cnt[t] += 1
        cur, state[n], sched[n] = out, S.ST_RELEASED, 0
    return cur, state, (cf, mf, cu, cnt)


@pytest.mark.parametrize("seed,strategy", [(0, s) for s in R.STRATEGIES] + [(3, R.SPREAD), (4, R.PACK)])
def test_theorem_c_composition(seed, strategy):
    cont, live, assign, cnt, order, ref = _case(seed, strategy)
    cur, state, (cf, mf, cu, c2) = stepwise(cont, live, assign, order, strategy, 0, cnt)
    assert np.array_equal(cur, ref[0]) and np.array_equal(state, ref[1])
    (fcf, fmf, _, fcu, fsched), fcnt = ref[5]
    assert np.array_equal(cf, fcf) and np.array_equal(mf, fmf) and np.array_equal(cu, fcu) and np.array_equal(c2, fcnt)
    # and the statement itself: after a committed x, the rest of the order is a variant of its own on what x left
    x = next(t[0] for t in ref[4] if t[1])
    head = [int(n) for n in order[:list(order).index(x) + 1]]
    tail = [int(n) for n in order[list(order).index(x) + 1:]]
    mid = S.variant(cont, live, assign, head, strategy, 0, cnt)
    rest = S.variant(cont, mid[5][0], mid[0], tail, strategy, 0, mid[5][1])
    assert np.array_equal(rest[0], ref[0])
    keep = np.array([n not in head for n in range(live[0].size)])
    assert np.array_equal(rest[1][keep], ref[1][keep])


# ---- theorem E: FP_NONE entries change nothing ------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_e_none_entries(strategy):
    cont, live, assign, cnt, order, ref = _case(2, strategy)
    holes = np.full(order.size * 2 + 3, NONE, np.uint32)
    holes[1:1 + 2 * order.size:2] = order
    got = S.variant(cont, live, assign, holes, strategy, 0, cnt)
    for a, b in zip(got[:4], ref[:4]):
        assert np.array_equal(a, b)
    both = S.sweep(cont, live, assign, S.pad([list(order), list(order[:5])]), strategy, 0, cnt)
    assert np.array_equal(both[0][0], ref[0]) and np.array_equal(both[3][0], ref[3])
    assert np.array_equal(both[3][1], S.variant(cont, live, assign, order[:5], strategy, 0, cnt)[3])


# ---- hand-made traps ---------------------------------------------------------------------------------------------
def test_trap_blocker_after_moves_gives_the_conflict_bits_back():
    """Node 0 holds a (bit 1), b (bit 2) and c, which fits nowhere.  a and b move to node 1 first; the undo must
    clear exactly their bits there, or d (bit 1) could not follow when node 2 is tried."""
    cont = _cont([50, 40, 30, 20], conf=[1, 2, 0, 1], req=[0, 0, 4, 0])
    nodes = _nodes([0, 200, 0], cu=[3, 8, 1])
    out, state, blocker, row, trace, (after, _) = S.variant(cont, nodes, [0, 0, 0, 2], [0, 2])
    assert trace == [(0, False, 2), (2, True, 1)] and blocker[0] == 2
    assert out.tolist() == [0, 0, 0, 1] and state.tolist() == [2, 0, 1]
    assert after[0].tolist() == [0, 180, 0] and after[3].tolist() == [3, 9, 1]
    assert row.tolist() == [1, 2, 1, 1, 1, 20, 1, 0]


def test_trap_a_service_moves_twice():
    cont = _cont([100, 10])
    nodes = _nodes([0, 100, 100])
    out, state, _, row, _, _ = S.variant(cont, nodes, [0, 2], [0, 1])  # first fit: 0 -> 1, then 1 -> 2
    assert out.tolist() == [2, 2] and state.tolist() == [1, 1, 0]
    assert row[[S.RELEASED, S.MOVES, S.MOVED, S.MOVED_CPU]].tolist() == [2, 2, 1, 100]


def test_trap_a_node_listed_twice():
    """Node 0 holds A (60 cpu, 1 mem) and B (50 cpu, 100 mem).  First fit puts A on node 1 and B then fits
    nowhere (node 2 has 1 MiB).  Once node 3's D (45 cpu) has moved to node 1, A no longer fits there, goes to
    node 2, and B takes node 1: the same node fails, then succeeds."""
    cont = _cont([60, 50, 45], mem=[1, 100, 1])
    nodes = _nodes([0, 100, 60, 0], mf=[0, 101, 1, 0])
    assign = [0, 0, 3]
    out, state, blocker, row, trace, _ = S.variant(cont, nodes, assign, [0, 3, 0])
    assert trace == [(0, False, 1), (3, True, 1), (0, True, 2)]
    assert out.tolist() == [2, 1, 1] and state.tolist() == [1, 0, 0, 1] and (blocker == NONE).all()
    assert row.tolist() == [2, 3, 1, 3, 3, 155, 102, 0]
    # listed twice with nothing in between, it fails again; a third entry after its release is skipped
    out, state, blocker, row, trace, _ = S.variant(cont, nodes, assign, [0, 0, 3, 0, 0])
    assert [t[:2] for t in trace] == [(0, False), (0, False), (3, True), (0, True)] and row[:3].tolist() == [2, 4, 2]
    out, state, blocker, row, trace, _ = S.variant(cont, nodes, assign, [0, 0])
    assert state.tolist() == [2, 0, 0, 0] and blocker[0] == 1 and row.tolist() == [0, 2, 2, 0, 0, 0, 0, 0]
    assert np.array_equal(out, assign)


def test_trap_empty_cordoned_and_no_target():
    cont = _cont([10, 10])
    nodes = _nodes([100, 100, 100, 100], sched=[1, 0, 1, 0])
    # node 3 is empty and cordoned: released with zero moves.  node 1 is cordoned and holds a container: it is
    # attempted like any other and its container goes to a schedulable node
    out, state, _, row, trace, _ = S.variant(cont, nodes, [1, 0], [3, 1])
    assert trace == [(3, True, 0), (1, True, 1)] and out.tolist() == [0, 0] and row[:5].tolist() == [2, 2, 0, 1, 1]
    # every target cordoned or released: the attempt on 0 fails with its first container as the blocker
    out, state, blocker, row, _, _ = S.variant(cont, nodes, [0, 0], [2, 0])
    assert state.tolist() == [2, 0, 1, 0] and blocker[0] == 0 and np.array_equal(out, [0, 0]) and row[S.FIRST_FAILED] == 0
    # no containers at all: every tried node is released
    none = tuple(np.zeros(0, np.uint32) for _ in range(4))
    out, state, _, row, _, _ = S.variant(none, nodes, np.zeros(0, np.uint32), [1, NONE, 1, 2])
    assert state.tolist() == [0, 1, 1, 0] and row.tolist() == [2, 2, 0, 0, 0, 0, 0, NONE]


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


def test_shrink_sweep_length_checks():
    p = _planner(_NoLib())
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    for i in range(4):
        short = cont[:i] + (cont[i][:-1],) + cont[i + 1:]
        _refused("every container array must hold C entries", p.shrink_sweep, short, nodes, [0, 0], [[0, 1]])
    for i in range(5):
        short = nodes[:i] + (nodes[i][:-1],) + nodes[i + 1:]
        _refused("every node array must hold N entries", p.shrink_sweep, cont, short, [0, 0], [[0, 1]])
    _refused("assign must hold C entries", p.shrink_sweep, cont, nodes, [0], [[0, 1]])
    _refused("try_order must be [n_var, n_try]", p.shrink_sweep, cont, nodes, [0, 0], [0, 1])
    _refused("node_count must hold N entries", p.shrink_sweep, cont, nodes, [0, 0], [[0, 1]], node_count=[0] * 4)
    with pytest.raises(ValueError, match="unknown placement strategy"):
        p.shrink_sweep(cont, nodes, [0, 0], [[0]], strategy="round_robin")


def test_shrink_sweep_call():
    lib = _Rec(peek={3: 2, 4: 6, 9: 3})
    p = _planner(lib)
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    out, state, blocker, summary = p.shrink_sweep(cont, nodes, [0, NONE], [[0, 1, NONE], [2, NONE, NONE]], "fill_lowest", -1,
                                                  [4, 5, 6])
    (name, args, seen), = lib.calls
    assert name == "fp_shrink_sweep" and len(args) == 14 == len(_lib.SIGNATURES[name][1]) and _addr(args[0]) == 0x5EED
    assert seen == {3: [0, NONE], 4: [0, 1, NONE, 2, NONE, NONE], 9: [4, 5, 6]}
    assert args[5:9] == (2, 3, _lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, ns.n) == (2, 3) and cs.cpu_m == cont[0].ctypes.data and ns.cpu_free == nodes[0].ctypes.data  # no copy
    assert [_addr(args[i]) for i in (10, 11, 12, 13)] == [x.ctypes.data for x in (out, state, blocker, summary)]
    assert (out.shape, state.shape, blocker.shape, summary.shape) == ((2, 2), (2, 3), (2, 3), (2, _lib.SHRINK_WORDS))
    assert (out.dtype, state.dtype, blocker.dtype) == (np.uint32, np.uint8, np.uint32)
    lib = _Rec()
    p = _planner(lib)
    p.shrink_sweep(cont, nodes, [0, 1], np.zeros((0, 4), np.uint32))
    args = lib.calls[0][1]
    assert args[5:9] == (0, 4, 0, 0) and _addr(args[9]) == 0  # no node_count: NULL


def test_dev_shrink_sweep_call_and_checks():
    torch = pytest.importorskip("torch")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    C, N, V, T = 3, 2, 2, 5
    cont_t, nodes_t = tuple(i32(C) for _ in range(4)), tuple(i32(N) for _ in range(4)) + (u8(N),)
    asg, tro, cnt, out, st, bl, sm = i32(C), i32(V * T), i32(N), i32(V * C), u8(V * N), i32(V * N), i32(V * 8)
    lib = _Rec()
    q = _planner(lib)  # kept: a planner that goes away closes its context through the library
    q.dev_shrink_sweep(cont_t, nodes_t, asg, tro, V, out, st, sm, "pack_into_dedicated", 6, cnt, bl)
    (name, args, _), = lib.calls
    assert name == "fp_dev_shrink_sweep" and len(args) == 14 == len(_lib.SIGNATURES[name][1])
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, cs.cpu_m, cs.conflict) == (C, cont_t[0].data_ptr(), cont_t[3].data_ptr())
    assert (ns.n, ns.cpu_free, ns.schedulable) == (N, nodes_t[0].data_ptr(), nodes_t[4].data_ptr())
    assert args[5:9] == (V, T, _lib.STRATEGY_PACK, 6)
    assert [_addr(args[i]) for i in (3, 4, 9, 10, 11, 12, 13)] == [t.data_ptr() for t in (asg, tro, cnt, out, st, bl, sm)]
    q.dev_shrink_sweep(cont_t, nodes_t, asg, tro, V, out, st, sm)
    assert _addr(lib.calls[1][1][12]) == 0 and _addr(lib.calls[1][1][9]) == 0
    fn = _planner(_NoLib()).dev_shrink_sweep
    _refused("every container tensor must hold C 32-bit entries", fn, cont_t[:3] + (i32(C + 1),), nodes_t, asg, tro, V,
             out, st, sm)
    _refused("every node tensor must hold N entries", fn, cont_t, nodes_t[:4] + (i32(N),), asg, tro, V, out, st, sm)
    _refused("assign_t must hold C 32-bit entries", fn, cont_t, nodes_t, i32(C - 1), tro, V, out, st, sm)
    _refused("try_order_t must hold n_var rows of 32-bit entries", fn, cont_t, nodes_t, asg, i32(V * T + 1), V, out, st, sm)
    _refused("count_t must hold N 32-bit entries", fn, cont_t, nodes_t, asg, tro, V, out, st, sm, count_t=i32(N + 1))
    _refused("assign_out_t must hold n_var * C 32-bit entries", fn, cont_t, nodes_t, asg, tro, V, i32(C), st, sm)
    _refused("state_t must hold n_var * N bytes", fn, cont_t, nodes_t, asg, tro, V, out, i32(V * N), sm)
    _refused("blocker_t must hold n_var * N 32-bit entries", fn, cont_t, nodes_t, asg, tro, V, out, st, sm, blocker_t=i32(N))
    _refused("summary_t must hold n_var * 8 32-bit entries", fn, cont_t, nodes_t, asg, tro, V, out, st, i32(V * 8 - 1))


def test_abi_declares_the_shrink_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    mk = open(os.path.join(ROOT, "fleetflow_amd", "csrc", "Makefile")).read()
    for name in ("fp_shrink_sweep", "fp_dev_shrink_sweep"):
        assert f"int {name}(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes" in hdr
        assert name in _lib.SIGNATURES and f"pub fn {name}(" in ffi
    assert "ffi::fp_shrink_sweep(" in lib and "fp_shrink.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()
    words = dict(re.findall(r"(FP_SHRINK_\w+) = (\d+)", hdr))
    assert words == {"FP_SHRINK_RELEASED": "0", "FP_SHRINK_TRIED": "1", "FP_SHRINK_FAILED": "2", "FP_SHRINK_MOVES": "3",
                     "FP_SHRINK_MOVED": "4", "FP_SHRINK_MOVED_CPU": "5", "FP_SHRINK_MOVED_MEM": "6",
                     "FP_SHRINK_FIRST_FAILED": "7", "FP_SHRINK_WORDS": "8", "FP_SHRINK_STATE_NEVER": "0",
                     "FP_SHRINK_STATE_RELEASED": "1", "FP_SHRINK_STATE_FAILED": "2"}
    for name, val in words.items():
        assert getattr(_lib, name[3:]) == int(val)
        assert re.search(rf"pub const {name}: (usize|u8) = {val};", ffi), name
    assert (S.WORDS, S.FIRST_FAILED, S.ST_FAILED) == (_lib.SHRINK_WORDS, _lib.SHRINK_FIRST_FAILED, _lib.SHRINK_STATE_FAILED)
    assert len(_lib.SHRINK_FIELDS) == _lib.SHRINK_WORDS


# ---- the flow level ------------------------------------------------------------------------------------
class _RefPlanner:
    """shrink_sweep answered by the numpy reference; remembers what it was asked."""

    def shrink_sweep(self, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None):
        self.asked = (cont, nodes, assign, np.array(try_order), strategy, preferred, node_count)
        return S.sweep(cont, nodes, assign, try_order, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred,
                       node_count)


def _flow():
    f = F.Flow("shop")
    spec = {"db": (3000, 4096, ["class=ssd"], None), "api": (1000, 1024, [], "web"), "web": (1000, 512, [], "web"),
            "cache": (500, 2048, [], None), "cron": (250, 128, [], None), "batch": (2500, 1024, [], None)}
    for name, (cpu, mem, labels, group) in spec.items():
        f.services[name] = F.Service(cpu_m=cpu, mem_mib=mem, labels=labels, anti_affinity=group)
    servers = [("a1", 4000, 8192, ["region=east", "class=ssd"]), ("a2", 4000, 8192, ["region=east"]),
               ("b1", 4000, 8192, ["region=west"]), ("b2", 2000, 4096, ["region=west"]),
               ("c1", 4000, 8192, [])]
    for slug, cpu, mem, labels in servers:
        f.servers[slug] = F.Server(slug, cpu, mem, labels)
    f.stages["live"] = F.Stage(services=list(spec), servers=[s[0] for s in servers])
    return f


def _plan_by_reference(f, policy):
    stage = f.stages["live"]
    nodes = [f.servers[s] for s in stage.servers]
    cont, ntab = F._stage_tables(stage.services, f, nodes, policy.preferred)
    pmask = F._stage_labels(stage.services, f, nodes, policy.preferred).mask(policy.preferred)
    st = _lib.POLICY_STRATEGIES.get(policy.strategy, 0)
    a, r, after, cnt = R.place(cont, ntab, st, pmask)
    plan = F.Plan("live", [], {}, [], {n: stage.servers[a[v]] for v, n in enumerate(stage.services) if a[v] != NONE},
                  {n: "NOFIT" for v, n in enumerate(stage.services) if a[v] == NONE})
    plan.strategy, plan.preferred = policy.strategy, policy.preferred
    return plan, (cont, a, after, cnt, st, pmask)


def test_shrink_stage_rules_keep_and_report():
    f = _flow()
    policy = F.PlacementPolicy("spread_across_pool")
    plan, (cont, a, after, cnt, st, pmask) = _plan_by_reference(f, policy)
    slugs = f.stages["live"].servers
    assert sorted(set(plan.assignment.values())) == sorted(slugs)  # SPREAD used every server
    p = _RefPlanner()
    rep = F.shrink_stage(f, "live", plan, planner=p)
    count = np.bincount(a, minlength=5)
    load = np.bincount(a, weights=np.array(cont[0], np.float64), minlength=5)
    rules = {"fewest": sorted(range(5), key=lambda n: (count[n], n)), "lightest": sorted(range(5), key=lambda n: (load[n], n)),
             "last": [4, 3, 2, 1, 0]}
    assert [v.name for v in rep.variants] == ["fewest", "lightest", "last"] and rep.strategy == "spread_across_pool"
    assert p.asked[3].tolist() == [rules[v.name] for v in rep.variants] and p.asked[4:6] == ("spread_across_pool", pmask)
    assert [int(x) for x in p.asked[6]] == [int(x) for x in cnt]
    out, state, blocker, rows = S.sweep(cont, after, a, p.asked[3], st, pmask, cnt)
    names = f.stages["live"].services
    for i, v in enumerate(rep.variants):
        assert v.order == [slugs[n] for n in rules[v.name]]
        assert v.released == [slugs[n] for n in rules[v.name] if state[i][n] == S.ST_RELEASED] and v.released
        assert sorted(v.moves) == sorted((names[c], slugs[a[c]], slugs[out[i][c]]) for c in range(6) if out[i][c] != a[c])
        assert v.stayed == [(slugs[n], names[blocker[i][n]]) for n in rules[v.name] if state[i][n] == S.ST_FAILED]
        assert (v.tried, v.failed, v.n_moves, v.moved_cpu_m) == tuple(int(rows[i][w]) for w in (1, 2, 3, 5))
        assert not set(v.released) & {dst for _, _, dst in v.moves}
    best = min(range(3), key=lambda i: (-int(rows[i][0]), int(rows[i][4]), i))
    assert rep.best == best and rep.plan is not plan and rep.plan.strategy == plan.strategy
    assert rep.plan.assignment == {names[c]: slugs[out[best][c]] for c in range(6)}
    assert not set(rep.plan.assignment.values()) & set(rep.variants[best].released)
    # the plan is ready for the next question: its live table has the released servers empty
    assert all(F.live_tables(f, "live", rep.plan)[5][slugs.index(s)] == 0 for s in rep.variants[best].released)
    # keep, explicit lists, draining first
    rep = F.shrink_stage(f, "live", plan, orders=["last", ["b2", "a1", "c1"]], keep=["c1"], planner=p)
    assert p.asked[3].tolist() == [[3, 2, 1, 0], [3, 0, NONE, NONE]] and rep.keep == ["c1"]
    assert [v.name for v in rep.variants] == ["last", "order1"] and rep.variants[1].order == ["b2", "a1"]
    assert all("c1" not in v.released for v in rep.variants)
    f.servers["b1"].draining = True
    f.servers["b1"].schedulable = False
    rep = F.shrink_stage(f, "live", plan, orders=["fewest", "lightest", "last"], planner=p)
    assert [r[0] for r in p.asked[3].tolist()] == [2, 2, 2] and p.asked[3][2].tolist() == [2, 4, 3, 1, 0]
    with pytest.raises(ValueError, match="no servers of stage"):
        F.shrink_stage(f, "live", plan, keep=["z9"], planner=p)
    with pytest.raises(ValueError, match="no servers of stage"):
        F.shrink_stage(f, "live", plan, orders=[["a1", "z9"]], planner=p)
    with pytest.raises(ValueError, match="unknown order rule"):
        F.shrink_stage(f, "live", plan, orders=["random"], planner=p)
    assert F.shrink_stage(f, "live", plan, orders=[], planner=p).variants == []


def test_report_text_and_json_round_trip():
    f = _flow()
    plan, _ = _plan_by_reference(f, F.PlacementPolicy("pack_into_dedicated", {"region": "west"}))
    rep = F.shrink_stage(f, "live", plan, keep=["a1"], planner=_RefPlanner())
    text = PO.format_shrink_report(rep)
    lines = text.split("\n")
    heads = [ln for ln in lines if ln.startswith("shrink ")]
    assert len(heads) == 3 and sum(ln.endswith("(best)") for ln in heads) == 1
    v = rep.variants[rep.best]
    assert f"shrink {v.name}: {len(v.released)} of {v.tried} servers released, {len(v.moves)} services move " in text
    for svc, src, dst in v.moves:
        assert f"  {svc}: {src} -> {dst}" in lines
    for srv, svc in v.stayed:
        assert f"  {srv}: stays (blocked by {svc})" in lines
    assert any(x.stayed for x in rep.variants) and any(x.moves for x in rep.variants)
    js = PO.shrink_report_to_json(rep)
    back = PO.shrink_report_from_json(js)
    assert back == rep and PO.shrink_report_to_json(back) == js
    empty = F.ShrinkReport("live")
    assert PO.shrink_report_from_json(PO.shrink_report_to_json(empty)) == empty and PO.format_shrink_report(empty) == ""
    import fleetflow_amd
    assert fleetflow_amd.shrink_stage is F.shrink_stage and fleetflow_amd.format_shrink_report is PO.format_shrink_report
