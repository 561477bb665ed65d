"""CPU tests of the rebalance sweep (SPEC.md 2.19): the theorems on the numpy reference (tests/rebalance_ref.py) over
random cases, the hand-made traps, the Planner wrappers' checks and what they send to which export, the flow-level
``rebalance_stage`` from KDL, and the report's text and JSON round trip.  No GPU."""
import ctypes as ct
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_ref as FR  # noqa: E402
import rebalance_cases as T  # noqa: E402
import rebalance_ref as RR  # noqa: E402
import replan_policy_ref as RPP  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd.planner import Planner  # noqa: E402
from fleetflow_amd.plan_output import (format_rebalance_report, rebalance_report_from_dict,  # noqa: E402
                                       rebalance_report_to_dict)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
MAX_SKEW = 2
RELAX = (1, 2)
SEEDS = tuple(range(12))
ALL = [(seed, rule, strategy) for seed in SEEDS for rule in RR.ORDERS for strategy in range(4)]
SOME = ALL[::5]  # a spread of seeds, rules and strategies for the dearer theorems


@functools.lru_cache(maxsize=None)
def _case(seed):
    return RR.random_case(seed, max_skew=MAX_SKEW, relax_mask=RELAX)


class _Steps:
    """Theorems A, B and C, asserted on the state every move leaves."""

    def __init__(self, cnt, dom, sched):
        self.dom, self.sched = dom, sched
        self.excess = RR.excess(cnt, dom, sched, MAX_SKEW)
        dc, elig = RR.dom_counts(cnt, dom, sched)
        self.mx, self.mn = int(dc[elig].max()), int(dc[elig].min())
        self.n = 0

    def __call__(self, cnt, s, t):
        dom, sched = self.dom, self.sched
        assert dom[t] != dom[s], "A: never its own domain"
        ex = RR.excess(cnt, dom, sched, MAX_SKEW)
        assert ex <= self.excess - 1, "B: the excess falls with every move"
        dc, elig = RR.dom_counts(cnt, dom, sched)
        mx, mn = int(dc[elig].max()), int(dc[elig].min())
        assert mx <= self.mx and mn >= self.mn, "B: max never rises, min never falls"
        assert not RR.heavy(cnt, dom, sched, MAX_SKEW)[dom[t]], "C: a target's domain is never heavy afterwards"
        self.excess, self.mx, self.mn = ex, mx, mn
        self.n += 1


@functools.lru_cache(maxsize=None)
def _run(seed, rule, strategy):
    """The unlimited variant of a case under a rule (visited twice) and a strategy, with the step assertions."""
    cont, live, assign, cnt, dom, _ = _case(seed)
    order = np.concatenate([RR.order_of(rule, cont)] * 2)
    steps = _Steps(cnt, dom, live[4])
    base_excess = steps.excess
    out = RR.variant(cont, live, assign, order, NONE, strategy, 0, cnt, dom, MAX_SKEW, RELAX, step=steps)
    return order, out, base_excess, steps


# ---- the cases are what the issue asks for -----------------------------------------------------------------------
def test_random_cases_show_every_condition_in_a_tenth_of_them():
    shares = dict.fromkeys(RR.CONDITIONS, 0)
    for seed in SEEDS:
        seen = set()
        for rule in RR.ORDERS:
            for strategy in range(4):
                _, out, _, _ = _run(seed, rule, strategy)
                seen |= RR.conditions(out[4], out[3], MAX_SKEW)
        for what in seen:
            shares[what] += 1
    print(shares)
    for what, n in shares.items():
        assert n * 10 >= len(SEEDS), (what, shares)


# ---- theorems A, B, C ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_theorems_a_b_c_at_every_step(seed):
    cont, live, assign, cnt, dom, _ = _case(seed)
    for rule in RR.ORDERS:
        for strategy in range(4):
            order, out, base_excess, steps = _run(seed, rule, strategy)
            row = out[3]
            assert steps.n == row[RR.MOVES] == int((out[0] != assign).sum()), "C: one move per container"
            assert row[RR.MOVES] <= base_excess and row[RR.SKEW_AFTER] <= row[RR.SKEW_BEFORE], "B"
            assert (row[RR.SKEW_AFTER] <= MAX_SKEW) == (steps.excess == 0), "B: in bound iff the excess is 0"
            assert row[RR.SKEW_BEFORE] == RR.skew(cnt, dom, live[4]) and row[RR.SKEW_AFTER] == RR.skew(out[5][1], dom, live[4])
            assert row[RR.STUCK] == sum(1 for t in out[4] if t[3] != "MOVE") >= row[RR.STUCK_SKEW]
            assert row[RR.RELAXED] == int((out[1] != 0).sum()) and not out[1][out[0] == assign].any()
            moved = out[0] != assign
            assert row[RR.MOVED_CPU] == int(cont[0][moved].sum()) and row[RR.MOVED_MEM] == int(cont[1][moved].sum())


# ---- theorem D: an attempt is the per-node statement of 2.8 on the lifted table, too -------------------------------
@pytest.mark.parametrize("seed,rule,strategy", SOME)
def test_theorem_d_anchor(seed, rule, strategy):
    cont, live, assign, cnt, dom, _ = _case(seed)
    _, out, _, _ = _run(seed, rule, strategy)
    assert out[4], "no attempt"
    i, c, s, what, t, hop = out[4][0]  # the first attempt runs on the base state
    cf, mf, lab, cu, sched = (np.array(x) for x in live)
    cf[s] += cont[0][c]
    mf[s] += cont[1][c]
    cu[s] &= ~cont[3][c]
    lifted = np.array(cnt)
    lifted[s] -= 1
    a, r, h, _, _ = FR.place_per_node(tuple(x[c:c + 1] for x in cont), (cf, mf, lab, cu, sched), strategy, node_count=lifted,
                                      domain=dom, max_skew=MAX_SKEW, relax_mask=list(RELAX))
    assert (a[0], int(h[0])) == (t, hop) and {0: "MOVE", 1: "NOFIT", 3: "SKEW"}[int(r[0])] == what


# ---- theorem E: independence, and FP_NONE entries --------------------------------------------------------------------
@pytest.mark.parametrize("seed,rule,strategy", SOME)
def test_theorem_e_independence_and_holes(seed, rule, strategy):
    cont, live, assign, cnt, dom, _ = _case(seed)
    order, out, _, _ = _run(seed, rule, strategy)
    holes = np.insert(order, [0, 5, 5, 63, 64, 200], NONE)
    other = np.concatenate([RR.order_of(RR.ORDERS[(RR.ORDERS.index(rule) + 1) % 3], cont)] * 2)
    vo = RR.pad([other, order, holes])
    got = RR.sweep(cont, live, assign, vo, strategy, 0, cnt, dom, MAX_SKEW, RELAX, max_moves=[3, NONE, NONE])
    for v in (1, 2):
        for g, e in zip(got, out[:4]):
            assert np.array_equal(g[v], e)
    assert got[3][0, RR.MOVES] <= 3


# ---- theorem F: the budget prefix --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,rule,strategy", SOME)
def test_theorem_f_budget_prefix(seed, rule, strategy):
    cont, live, assign, cnt, dom, _ = _case(seed)
    order, out, _, _ = _run(seed, rule, strategy)
    moves = [t for t in out[4] if t[3] == "MOVE"]
    for b in sorted({0, 1, 2, len(moves) // 2, len(moves), len(moves) + 1}):
        cut = RR.variant(cont, live, assign, order, b, strategy, 0, cnt, dom, MAX_SKEW, RELAX)
        end = 0 if b == 0 else moves[b - 1][0] + 1 if b <= len(moves) else len(order)
        assert cut[4] == [t for t in out[4] if t[0] < end], b  # the same moves, hops and rejections so far
        assert cut[3][RR.MOVES] == min(b, len(moves)) and cut[3][RR.STUCK] == sum(1 for t in cut[4] if t[3] != "MOVE")


# ---- theorem G: validity, and the next re-plan keeps every seat ----------------------------------------------------
@pytest.mark.parametrize("seed,rule,strategy", SOME)
def test_theorem_g_validity_and_replan_keeps_it(seed, rule, strategy):
    cont, live, assign, cnt, dom, pre = _case(seed)
    _, (out, hops, reason, row, trace, ((cf, mf, lab, cu, sched), cnt_end)), _, _ = _run(seed, rule, strategy)
    assert np.array_equal(out == NONE, assign == NONE)
    moved = np.flatnonzero(out != assign)
    cum = FR.cumulative(RELAX, len(RELAX))
    for c in moved:
        need = int(cont[2][c]) & ~cum[int(hops[c])]
        assert need & ~int(lab[out[c]]) == 0 and sched[out[c]]
        if hops[c]:
            assert (int(cont[2][c]) & ~cum[int(hops[c]) - 1]) & ~int(lab[out[c]]) != 0  # no smaller hop would do
    # capacity: what finally runs on a node is within cpu_free + the requests based there
    run = out != NONE
    for col, free in ((0, live[0]), (1, live[1])):
        based, final = np.zeros(free.size, np.int64), np.zeros(free.size, np.int64)
        np.add.at(based, assign[run].astype(np.int64), cont[col][run].astype(np.int64))
        np.add.at(final, out[run].astype(np.int64), cont[col][run].astype(np.int64))
        assert (final <= free.astype(np.int64) + based).all()
        end = free.astype(np.int64) + based - final
        assert np.array_equal(end, (cf if col == 0 else mf).astype(np.int64))
    for n in np.unique(out[moved]):  # conflict masks on one node are pairwise disjoint
        masks = cont[3][out == n]
        assert int(np.bitwise_or.reduce(masks)).bit_count() == sum(int(m).bit_count() for m in masks)
    # on the pre-plan table the next re-plan under the policy keeps every placed container (2.14 theorem C)
    two = RPP.replan(cont, pre, out, strategy, domain=dom, max_skew=MAX_SKEW, relax_mask=list(RELAX))
    assert (two[3][run] == RPP.KEPT).all() and np.array_equal(two[0][run], out[run])
    if run.all():
        assert RR.skew(two[6], dom, pre[4]) == row[RR.SKEW_AFTER]
    assert RR.skew(RR.derived_count(out, 40), dom, live[4]) == row[RR.SKEW_AFTER]


def test_the_degenerate_form():
    cont, live, assign, cnt, dom, _ = _case(0)
    order = RR.order_of("smallest", cont)
    for kw in (dict(domain=None, max_skew=2), dict(domain=np.full(40, 99, np.uint32), max_skew=0)):
        out = RR.variant(cont, live, assign, order, NONE, 0, 0, cnt, relax_mask=RELAX, **kw)
        assert np.array_equal(out[0], assign) and not out[1].any() and not out[2].any() and not out[3].any()


# ---- the traps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(T.traps())))
def test_traps_on_the_reference(i):
    name, kw, exp = T.traps()[i]
    got = RR.sweep(**kw)
    assert got[0][0].tolist() == exp["out"] and got[1][0].tolist() == exp["hops"], name
    assert got[2][0].tolist() == exp["reason"] and got[3][0].tolist() == exp["summary"], name


def test_trap_contrasts():
    traps = {name: kw for name, kw, _ in T.traps()}
    # second pass: without the repeated entry the big service stays, rejected SKEW
    kw = dict(traps["second pass"], victim_order=[[0, 1]])
    got = RR.sweep(**kw)
    assert got[0][0].tolist() == [0, 2, 0, 0, 0] and got[2][0].tolist() == [RR.SKEW, 0, 0, 0, 0]
    # NOFIT: with room on node 2 the chain gives the label up and the service moves at hop 1
    kw = traps["NOFIT even at the last hop"]
    nodes = T._nodes([0, 0, 50], lab=[1, 1, 0], sched=[0, 1, 1])
    got = RR.sweep(**dict(kw, nodes=nodes))
    assert got[0][0].tolist() == [2, 0, 0] and got[1][0].tolist() == [1, 0, 0]
    # reversal: a conflict word that holds the victim's bit makes the second service's rejection NOFIT
    kw = traps["a reversal restores the conflict word"]
    nodes = T._nodes([10, 0, 0], sched=[1, 0, 1], cu=[5, 0, 0])
    assert RR.sweep(**dict(kw, nodes=nodes, victim_order=[[1]]))[2][0].tolist() == [0, RR.NOFIT]
    # cordoned zone: schedulable again, A is the heaviest and gives its services up first
    kw = traps["a cordoned heavy zone gives no victims"]
    got = RR.sweep(**dict(kw, nodes=T._nodes([100, 100, 100])))
    assert got[0][0][0] == 2 and got[3][0][RR.SKEW_BEFORE] == 5


# ---- the wrappers -----------------------------------------------------------------------------------------------------
class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the check did not refuse first")


def _addr(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "_obj"):
        return ct.addressof(x._obj)
    return ct.cast(x, ct.c_void_p).value or 0


def _words(ptr, n):
    return [] if not _addr(ptr) else list(ct.cast(ct.c_void_p(_addr(ptr)), ct.POINTER(ct.c_uint32))[:n])


class _Rec:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def export(*args):
            self.calls.append((name, args, dict(max_moves=_words(args[7], args[5]), node_count=_addr(args[10]),
                                                domain=_addr(args[11]), max_skew=args[12], relax=_words(args[13], args[14]),
                                                n_hops=args[14])))
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


def test_rebalance_sweep_length_checks_and_call():
    cont, nodes = T._cont([1, 1]), T._nodes([9, 9, 9])
    fn = _planner(_NoLib()).rebalance_sweep
    _refused("every container array must hold C entries", fn, (cont[0][:1],) + cont[1:], nodes, [0, 0], [[0, 1]])
    _refused("every node array must hold N entries", fn, cont, (nodes[0][:2],) + nodes[1:], [0, 0], [[0, 1]])
    _refused("assign must hold C entries", fn, cont, nodes, [0], [[0, 1]])
    _refused("victim_order must be [n_var, n_try]", fn, cont, nodes, [0, 0], [0, 1])
    _refused("max_moves must hold n_var entries", fn, cont, nodes, [0, 0], [[0, 1]], max_moves=[1, 2])
    _refused("node_count must hold N entries", fn, cont, nodes, [0, 0], [[0, 1]], node_count=[0] * 4)
    _refused("domain must hold N entries", fn, cont, nodes, [0, 0], [[0, 1]], domain=[0, 1], max_skew=1)
    _refused("max_skew must be a u32", fn, cont, nodes, [0, 0], [[0, 1]], max_skew=1 << 32)
    _refused("relax_mask holds at most 4 hops", fn, cont, nodes, [0, 0], [[0, 1]], relax_mask=[1] * 5)
    lib = _Rec()
    p = _planner(lib)
    dom, cnt = np.array([0, 1, 1], np.uint32), np.array([4, 5, 6], np.uint32)
    got = p.rebalance_sweep(cont, nodes, [0, NONE], [[0, 1, NONE], [1, NONE, NONE]], "fill_lowest", -1, cnt, domain=dom,
                            max_skew=2, relax_mask=[1, 6], max_moves=[NONE, 3])
    (name, args, seen), = lib.calls
    assert name == "fp_rebalance_sweep" and len(args) == 19 == len(_lib.SIGNATURES[name][1])
    assert args[5:7] == (2, 3) and args[8:10] == (_lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    assert seen == dict(max_moves=[NONE, 3], node_count=cnt.ctypes.data, domain=dom.ctypes.data, max_skew=2, relax=[1, 6],
                        n_hops=2)
    assert [_addr(args[i]) for i in (15, 16, 17, 18)] == [x.ctypes.data for x in got]
    assert [x.shape for x in got] == [(2, 2), (2, 2), (2, 2), (2, 8)]
    assert [x.dtype for x in got] == [np.uint32, np.uint8, np.uint8, np.uint32]
    got = p.rebalance_sweep(cont, nodes, [0, 1], [[0]], want_hops=False, want_reason=False)
    assert lib.calls[1][2] == dict(max_moves=[], node_count=0, domain=0, max_skew=0, relax=[], n_hops=0)
    assert got[1] is None and got[2] is None and [_addr(lib.calls[1][1][i]) for i in (16, 17)] == [0, 0]


def test_dev_rebalance_sweep_call_and_checks():
    torch = pytest.importorskip("torch")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    C, N, V, T_ = 3, 2, 2, 5
    cont_t, nodes_t = tuple(i32(C) for _ in range(4)), tuple(i32(N) for _ in range(4)) + (u8(N),)
    asg, vo, cnt, out, sm, dom, hp, rs, mm = i32(C), i32(V * T_), i32(N), i32(V * C), i32(V * 8), i32(N), u8(V * C), u8(V * C), i32(V)
    lib = _Rec()
    q = _planner(lib)
    q.dev_rebalance_sweep(cont_t, nodes_t, asg, vo, V, out, sm, "pack_into_dedicated", 6, cnt, domain_t=dom, max_skew=3,
                          relax_mask=[4], max_moves_t=mm, hops_t=hp, reason_t=rs)
    (name, args, seen), = lib.calls
    assert name == "fp_dev_rebalance_sweep" and len(args) == 19 == len(_lib.SIGNATURES[name][1])
    assert args[5:7] == (V, T_) and args[8:10] == (_lib.STRATEGY_PACK, 6)
    assert (seen["node_count"], seen["domain"], seen["max_skew"], seen["relax"]) == (cnt.data_ptr(), dom.data_ptr(), 3, [4])
    assert [_addr(args[i]) for i in (3, 4, 7, 15, 16, 17, 18)] == [t.data_ptr() for t in (asg, vo, mm, out, hp, rs, sm)]
    q.dev_rebalance_sweep(cont_t, nodes_t, asg, vo, V, out, sm)
    assert [_addr(lib.calls[1][1][i]) for i in (7, 10, 11, 13, 16, 17)] == [0] * 6 and lib.calls[1][1][12] == 0
    fn = _planner(_NoLib()).dev_rebalance_sweep
    base = (cont_t, nodes_t, asg, vo, V, out, sm)
    _refused("assign_t must hold C 32-bit entries", fn, cont_t, nodes_t, i32(C - 1), vo, V, out, sm)
    _refused("victim_order_t must hold n_var rows of 32-bit entries", fn, cont_t, nodes_t, asg, i32(V * T_ + 1), V, out, sm)
    _refused("max_moves_t must hold n_var 32-bit entries", fn, *base, max_moves_t=i32(V + 1))
    _refused("count_t must hold N 32-bit entries", fn, *base, count_t=i32(N + 1))
    _refused("domain_t must hold N 32-bit entries", fn, *base, domain_t=i32(N + 1))
    _refused("relax_mask holds at most 4 hops", fn, *base, relax_mask=[1] * 5)
    _refused("hops_t must hold n_var * C bytes", fn, *base, hops_t=u8(C))
    _refused("reason_t must hold n_var * C bytes", fn, *base, reason_t=i32(V * C))
    _refused("summary_t must hold n_var * 8 32-bit entries", fn, cont_t, nodes_t, asg, vo, V, out, i32(V * 8 + 1))
    _refused("max_skew must be a u32", fn, *base, max_skew=-1)


def test_abi_declares_the_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    mk = open(os.path.join(ROOT, "fleetflow_amd", "csrc", "Makefile")).read()
    for name in ("fp_rebalance_sweep", "fp_dev_rebalance_sweep"):
        assert re.search(rf"\bint {name}\(", hdr) and f"pub fn {name}(" in ffi and name in _lib.SIGNATURES
    assert "ffi::fp_rebalance_sweep(" in lib and "pub fn rebalance_sweep(" in lib and "fp_rebalance.hip" in mk
    words = re.search(r"enum \{ (FP_REBAL_MOVES.*?FP_REBAL_WORDS = 8) \};", hdr, flags=re.S).group(1)
    for k, (cname, val) in enumerate(re.findall(r"(FP_REBAL_\w+) = (\d+)", words)):
        assert int(val) == k and getattr(_lib, cname[3:]) == k
        assert f"pub const {cname}: usize = {k};" in ffi
    assert len(_lib.REBAL_FIELDS) == _lib.REBAL_WORDS == RR.WORDS == 8
    assert "#define FP_ABI_VERSION 1" in hdr  # no version bump, no new reason
    assert "model.rs:56-63" in hdr[hdr.index("/* Rebalance sweep"):hdr.index("int fp_rebalance_sweep(")]
    assert ":435-442" in hdr[hdr.index("/* As fp_rebalance_sweep on device pointers"):hdr.index("int fp_dev_rebalance_sweep(")]


# ---- the flow-level path -------------------------------------------------------------------------------------------------
KDL = '''project "demo"
%s
%s
stage "live" {
%s
    placement strategy="spread_across_pool" {
        spread "region" max-skew=1
        fallback "class"
    }
}
'''
REGIONS = ("tokyo", "osaka", "nagoya")


def kdl_flow(nagoya_cpu=3000):
    """Nine servers in three regions (n2, n5, n8 in nagoya; n1 and n6 carry class=gpu), fourteen services of which
    every fourth requires class=gpu."""
    from fleetflow_amd.parser import parse_kdl_string
    servers = "\n".join(
        f'server "n{i}" {{ capacity cpu={nagoya_cpu if i % 3 == 2 else 3000} memory=8192; label "region={REGIONS[i % 3]}"; '
        + f'label "class={"gpu" if i in (1, 6) else "cpu"}" }}' for i in range(9))
    services = "\n".join(
        f'service "s{i}" {{ resources cpu={500 + 100 * (i % 3)} memory={512 * (1 + i % 2)}'
        + ('; require "class=gpu"' if i % 4 == 0 else "") + " }" for i in range(14))
    members = "\n".join(f'    service "s{i}"' for i in range(14)) + "\n" + "\n".join(f'    server "n{i}"' for i in range(9))
    return parse_kdl_string(KDL % (servers, services, members))


def _cordon(flow, region, on):
    for i in range(9):
        if REGIONS[i % 3] == region:
            flow.servers[f"n{i}"].schedulable = not on


def _reference_plan(flow):
    """plan_stage's assignment, made by the numpy reference on the flow as it stands."""
    stage = flow.stages["live"]
    pol = stage.placement
    names = list(dict.fromkeys(stage.services))
    nodes = F._server_nodes(flow, stage.servers)
    cont, ntab = F._stage_tables(names, flow, nodes, pol.preferred)
    ld = F._stage_labels(names, flow, nodes, pol.preferred)
    domain, has_key = F.spread_domains(nodes, pol.spread[0])
    relax = [ld.key_mask(k) for k in pol.fallback]
    a, r, h, _, _ = FR.place(cont, ntab, _lib.POLICY_STRATEGIES[pol.strategy], 0, domain=domain, max_skew=pol.spread[1],
                             relax_mask=relax)
    plan = F.Plan("live", [], {}, [], {n: nodes[a[v]].slug for v, n in enumerate(names) if a[v] != NONE},
                  {n: "NOFIT" for v, n in enumerate(names) if a[v] == NONE})
    plan.strategy, plan.preferred = pol.strategy, pol.preferred
    plan.spread_topology_key, plan.spread_max_skew = pol.spread
    plan.fallback_relax_order, plan.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    plan.relaxed = {names[v]: ["class"] for v in range(len(names)) if a[v] != NONE and h[v]}
    return plan


class _RefPlanner:
    """The sweep answered by the numpy reference; remembers what it was asked."""

    def rebalance_sweep(self, cont, nodes, assign, victim_order, strategy=0, preferred=0, node_count=None, *, domain=None,
                        max_skew=0, relax_mask=(), max_moves=None, want_hops=True, want_reason=True):
        self.asked = dict(nodes=nodes, domain=domain, max_skew=max_skew, relax=list(relax_mask), vo=np.array(victim_order),
                          max_moves=max_moves, count=node_count)
        return RR.sweep(cont, nodes, assign, victim_order, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred,
                        node_count, domain, max_skew, relax_mask, max_moves)


def _per_region(flow, plan):
    per = dict.fromkeys(REGIONS, 0)
    for slug in plan.assignment.values():
        per[REGIONS[int(slug[1:]) % 3]] += 1
    return per


def _check_report(flow, plan, rep, asked):
    """A report against the reference sweep over the live tables."""
    names, nodes, cont, live, assign, count, st, pmask = F.live_tables(flow, "live", plan)
    domain, _ = F.replan_domains(nodes, "region")
    relax = [F._stage_labels(names, flow, nodes, list(plan.preferred)).key_mask("class")]
    assert asked["domain"] == domain and asked["max_skew"] == 1 and asked["relax"] == relax and relax[0] != 0
    assert list(asked["count"]) == count
    ref = RR.sweep(cont, live, assign, asked["vo"], _lib.POLICY_STRATEGIES[st], pmask, count, domain, 1, relax,
                   asked["max_moves"])
    slugs = [nd.slug for nd in nodes]
    for i, v in enumerate(rep.variants):
        out, hops, why, row = (x[i] for x in ref)
        seen = list(dict.fromkeys(int(c) for c in asked["vo"][i] if c != NONE))
        assert v.order == [names[int(c)] for c in asked["vo"][i] if c != NONE]
        assert v.moves == [(names[c], slugs[assign[c]], slugs[out[c]]) for c in seen if out[c] != assign[c]]
        assert v.stuck == {names[c]: "SKEW" if why[c] == 3 else "NOFIT" for c in seen if why[c]}
        assert v.relaxed == {names[c]: ["class"] for c in seen if out[c] != assign[c] and hops[c]}
        assert (v.n_stuck, v.moved_cpu_m, v.moved_mem_mib, v.skew_before, v.skew_after) == tuple(
            int(row[k]) for k in (RR.STUCK, RR.MOVED_CPU, RR.MOVED_MEM, RR.SKEW_BEFORE, RR.SKEW_AFTER))
    vs = rep.variants
    assert rep.best == min(range(len(vs)), key=lambda i: (vs[i].skew_after > 1, vs[i].skew_after, len(vs[i].moves),
                                                          vs[i].moved_cpu_m, i))
    best = vs[rep.best]
    moved = {m[0] for m in best.moves}
    assert rep.plan.assignment == {**plan.assignment, **{svc: dst for svc, _, dst in best.moves}}
    assert rep.plan.relaxed == {**{s: k for s, k in plan.relaxed.items() if s not in moved}, **best.relaxed}
    return best


def test_rebalance_order_rules_and_names():
    flow = kdl_flow()
    _cordon(flow, "nagoya", True)
    plan = _reference_plan(flow)
    names, nodes, cont, live, assign, count, st, pmask = F.live_tables(flow, "live", plan)
    idx = list(range(14))
    assert F.rebalance_order("smallest", names, cont, assign) == sorted(idx, key=lambda v: (cont[0][v], cont[1][v], v))
    assert F.rebalance_order("largest", names, cont, assign) == sorted(idx, key=lambda v: (-cont[0][v], -cont[1][v], v))
    assert F.rebalance_order("newest", names, cont, assign, pin=["s13"]) == idx[-2::-1]
    for rule in RR.ORDERS:  # the reference's rules are the flow's
        assert F.rebalance_order(rule, names, cont, assign) == RR.order_of(rule, cont).tolist()
    with pytest.raises(ValueError, match="unknown order rule"):
        F.rebalance_order("oldest", names, cont, assign)
    p = _RefPlanner()
    with pytest.raises(ValueError, match=re.escape("['nope'] are no services")):
        F.rebalance_stage(flow, "live", plan, pin=["nope"], planner=p)
    with pytest.raises(ValueError, match=re.escape("['s99'] are no services")):
        F.rebalance_stage(flow, "live", plan, orders=[["s1", "s99"]], planner=p)
    with pytest.raises(ValueError, match="one budget per order"):
        F.rebalance_stage(flow, "live", plan, max_moves=[1, 2], planner=p)


def test_rebalance_stage_from_kdl():
    flow = kdl_flow()
    assert flow.stages["live"].placement.spread == ("region", 1) and flow.stages["live"].placement.fallback == ("class",)
    _cordon(flow, "nagoya", True)   # the zone is drained while the plan is made ...
    plan = _reference_plan(flow)
    _cordon(flow, "nagoya", False)  # ... and comes back
    assert len(plan.assignment) == 14 and _per_region(flow, plan) == {"tokyo": 7, "osaka": 7, "nagoya": 0}
    p = _RefPlanner()
    rep = F.rebalance_stage(flow, "live", plan, planner=p)
    assert [v.name for v in rep.variants] == ["smallest", "largest", "newest"]
    assert (rep.spread_topology_key, rep.spread_max_skew, rep.fallback_relax_order, rep.note) == ("region", 1, ["class"], None)
    best = _check_report(flow, plan, rep, p.asked)
    assert all(v.skew_before == 7 and v.skew_after <= 1 and v.lightest is None for v in rep.variants)
    assert len(best.moves) == 4 and all(REGIONS[int(dst[1:]) % 3] == "nagoya" for _, _, dst in best.moves)
    assert max(_per_region(flow, rep.plan).values()) - min(_per_region(flow, rep.plan).values()) <= 1
    assert any(v.relaxed for v in rep.variants)  # a service that requires class=gpu went to nagoya, which has none
    # pins, explicit lists and budgets
    victims = [m[0] for m in best.moves]
    rep2 = F.rebalance_stage(flow, "live", plan, orders=["smallest", victims + ["s0"]], pin=victims[:1], max_moves=[2, None],
                             planner=p)
    _check_report(flow, plan, rep2, p.asked)
    assert p.asked["max_moves"] == [2, NONE] and rep2.pin == victims[:1]
    assert [v.name for v in rep2.variants] == ["smallest", "order1"] and rep2.variants[0].max_moves == 2
    assert len(rep2.variants[0].moves) == 2 and rep2.variants[0].skew_after > 1 and rep2.variants[0].lightest == "region=nagoya"
    assert all(victims[0] not in v.order for v in rep2.variants)
    # the light zone has room for three services only (6, 5 and 3): every variant ends out of bound and says where
    tight = kdl_flow(nagoya_cpu=700)
    rep3 = F.rebalance_stage(tight, "live", plan, planner=p)
    best3 = _check_report(tight, plan, rep3, p.asked)
    assert len(best3.moves) == 3 and best3.skew_after == 3 and best3.lightest == "region=nagoya" and best3.stuck
    text = format_rebalance_report(rep3)
    assert "still out of bound: region=nagoya is the lightest eligible domain" in text and "grow_stage(under_policy=True)" in text
    # a stage without a spread constraint has nothing to restore
    none = F.rebalance_stage(flow, "live", plan, policy=F.PlacementPolicy("spread_across_pool"), planner=_NoLib())
    assert none.variants == [] and none.best is None and none.plan is None and "no spread constraint" in none.note
    assert format_rebalance_report(none) == "rebalance live: no spread constraint: nothing to restore"


def test_report_text_and_json_round_trip():
    flow = kdl_flow()
    _cordon(flow, "nagoya", True)
    plan = _reference_plan(flow)
    _cordon(flow, "nagoya", False)
    rep = F.rebalance_stage(flow, "live", plan, max_moves=[None, 3, None], planner=_RefPlanner())
    text = format_rebalance_report(rep).splitlines()
    heads = [ln for ln in text if ln.startswith("rebalance ")]
    assert len(heads) == 3 and sum(ln.endswith("(best)") for ln in heads) == 1
    v = rep.variants[0]
    assert heads[0].startswith(f"rebalance smallest: {len(v.moves)} services move ({v.moved_cpu_m}m cpu, {v.moved_mem_mib} MiB), "
                               f"skew over region 7 -> {v.skew_after} (max_skew 1), {v.n_stuck} attempts refused")
    assert ", budget 3" in heads[1] and "budget" not in heads[0]
    svc, src, dst = v.moves[0]
    assert any(ln.startswith(f"  {svc}: {src} -> {dst}") for ln in text)
    assert any("(relaxed: class)" in ln for ln in text)
    d = rebalance_report_to_dict(rep)
    again = rebalance_report_from_dict(json.loads(json.dumps(d)))
    assert again == rep and rebalance_report_to_dict(again) == d
    assert d["placement"]["spread"] == {"topology_key": "region", "max_skew": 1} and d["best"] == rep.best
    empty = F.RebalanceReport("live", note="no spread constraint: nothing to restore")
    assert rebalance_report_from_dict(json.loads(json.dumps(rebalance_report_to_dict(empty)))) == empty
    import fleetflow_amd
    for name in ("RebalanceReport", "RebalanceVariant", "rebalance_stage", "format_rebalance_report",
                 "rebalance_report_to_dict", "rebalance_report_from_dict"):
        assert name in fleetflow_amd.__all__ and hasattr(fleetflow_amd, name)


# ---- shared with the GPU test: the whole way on a real planner ---------------------------------------------------------
def check_rebalance_stage(planner):
    """plan under a drained zone, the zone returns, the re-plan reports the excess, the rebalance restores the bound
    and the next re-plan keeps its plan whole; where the light zone has no room the excess is the report's."""
    for nagoya_cpu, in_bound in ((3000, True), (700, False)):
        flow = kdl_flow(nagoya_cpu)
        _cordon(flow, "nagoya", True)
        plan = F.plan_stage(flow, "live", planner)
        _cordon(flow, "nagoya", False)
        assert len(plan.assignment) == 14 and _per_region(flow, plan)["nagoya"] == 0
        before = F.replan_stage(flow, "live", plan, planner, under_policy=True)
        assert before.skew_excess == 7 and not before.moved and "skew 7 over region" in F_text(before)
        rep = F.rebalance_stage(flow, "live", plan, planner=planner)
        ref = _RefPlanner()
        assert rebalance_report_to_dict(F.rebalance_stage(flow, "live", plan, planner=ref)) == rebalance_report_to_dict(rep)
        best = _check_report(flow, plan, rep, ref.asked)
        after = F.replan_stage(flow, "live", rep.plan, planner, under_policy=True)
        assert sorted(after.kept) == sorted(rep.plan.assignment) and not after.moved and not after.lost and not after.new
        assert after.plan.assignment == rep.plan.assignment
        if in_bound:
            assert best.skew_after <= 1 and after.skew_excess is None
        else:
            assert best.skew_after > 1 and after.skew_excess == best.skew_after


def F_text(report):
    from fleetflow_amd.plan_output import format_replan_report
    return format_replan_report(report)
