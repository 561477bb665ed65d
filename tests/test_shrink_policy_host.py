"""CPU tests of the scale-in sweep under the policy (SPEC.md 2.17): the numpy reference
(tests/shrink_policy_ref.py) against the section's theorems A to F and the hand-made traps
(tests/shrink_policy_cases.py), the Planner wrappers' checks and calls, flow.shrink_stage(under_policy=True) and
the report.  No GPU and no library: the wrappers talk to a recording stand-in."""
import ctypes as ct
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_policy_ref as DP  # noqa: E402
import drain_ref as D  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_ref as R  # noqa: E402
import shrink_policy_cases as T  # noqa: E402
import shrink_policy_ref as SP  # noqa: E402
import shrink_ref as S  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402
from fleetflow_amd.planner import Planner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
RELAX = (1, 2)
MAX_SKEW = 2
# per strategy: (n_dom, seed).  Chosen on the reference so that the cases of each strategy show all seven
# conditions of shrink_policy_ref.CONDITIONS between them; test_random_cases_show_every_condition asserts it
CASES = {R.FIRST_FIT: [(4, 2), (4, 3), (33, 2)], R.SPREAD: [(4, 3), (33, 2), (33, 1)],
         R.PACK: [(4, 4), (33, 2), (33, 0)], R.FILL_LOWEST: [(4, 3), (33, 3), (33, 0)]}
ALL = [(st, n_dom, seed) for st in R.STRATEGIES for n_dom, seed in CASES[st]]


@functools.lru_cache(maxsize=None)
def _case(strategy, n_dom, seed):
    cont, live, assign, cnt, dom, order = SP.random_case(seed, n_dom=n_dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    return cont, live, assign, cnt, dom, order, SP.variant(cont, live, assign, order, strategy, 0, cnt, dom, MAX_SKEW, RELAX)


def _run(case, order, strategy, **kw):
    cont, live, assign, cnt, dom = case[:5]
    kw = dict(dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX), **kw)
    return SP.variant(cont, live, assign, order, strategy, 0, cnt, **kw)


# ---- the random cases are not vacuous --------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_random_cases_show_every_condition(strategy):
    seen = set()
    for n_dom, seed in CASES[strategy]:
        trace = _case(strategy, n_dom, seed)[6][7]
        here = SP.conditions(trace)
        assert "commit with moves" in here and any(t[1] != "OK" for t in trace), (n_dom, seed)
        assert any(t[1] != "OK" and t[2] > 0 for t in trace), "a failed attempt that moved something first"
        seen |= here
    assert seen == set(SP.CONDITIONS), sorted(set(SP.CONDITIONS) - seen)


# ---- theorem A: without guarantees the call is 2.16 ------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("form", ["neither", "max_skew 0", "no hops"])
def test_theorem_a_without_guarantees_it_is_2_16(strategy, form):
    cont, live, assign, cnt, order = S.random_case(strategy + 1, strategy)
    tro = np.stack([order, order[::-1]])
    kw = {"neither": {}, "max_skew 0": dict(domain=np.arange(40) % 3, max_skew=0),
          "no hops": dict(domain=None, max_skew=5, relax_mask=())}[form]
    got = SP.sweep(cont, live, assign, tro, strategy, 5, cnt, **kw)
    exp = S.sweep(cont, live, assign, tro, strategy, 5, cnt)
    for g, e in zip(got[:4], exp):
        assert g.dtype == e.dtype and np.array_equal(g, e)
    assert not got[4].any() and not got[6].any()
    assert np.array_equal(got[5], np.where(exp[1] == S.ST_FAILED, SP.REASON_NOFIT, 0))
    assert (exp[1] == S.ST_FAILED).any()


# ---- theorem B: the drain anchor -------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_b_drain_anchor(strategy):
    kinds = set()
    for n_dom, seed in CASES[strategy]:
        case = _case(strategy, n_dom, seed)
        cont, live, assign, cnt, dom = case[:5]
        N = live[0].size
        for n in range(N):
            group = np.where(np.arange(N) == n, 0, NONE).astype(np.uint32)
            d_out, d_reason, d_rows, d_hops, d_pol = DP.sweep(cont, live, assign, group, 1, strategy, 0, cnt, dom, MAX_SKEW,
                                                              RELAX)
            out, state, blocker, summary, hops, why, row, trace, _ = _run(case, [n], strategy)
            if d_rows[0, D.STRANDED] > 0:
                first = int(d_rows[0, D.FIRST_STRANDED])
                assert state[n] == SP.ST_FAILED and blocker[n] == first and why[n] == d_reason[first]
                assert np.array_equal(out, assign) and not hops.any()
                kinds.add("stranded")
                continue
            gone = np.arange(N) == n
            sched = np.asarray(live[4])
            before = SP.skew(cnt, dom, np.zeros(N, bool), sched)
            left = cnt.astype(np.int64) + np.bincount(d_out[(assign == n)], minlength=N)
            after = SP.skew(left, dom, gone, sched * ~gone)
            if (assign == n).any():  # the drain's own word (zeros without evictees): the same state, n left out
                assert after == d_pol[0, DP.SKEW_AFTER]
            if after <= MAX_SKEW or after <= before:
                assert np.array_equal(out, d_out) and np.array_equal(hops, d_hops) and summary[SP.RELEASED] == 1
                kinds.add("commit")
            else:
                assert np.array_equal(out, assign) and state[n] == SP.ST_FAILED and blocker[n] == NONE
                assert why[n] == SP.REASON_SKEW and row[SP.FAILED_SKEW] == 1
                kinds.add("bound")
    assert {"stranded", "commit"} <= kinds


def test_theorem_b_sees_a_bound_refusal_somewhere():
    """The third branch of theorem B, on the trap built for it."""
    name, kw, _ = T.traps()[0]
    group = np.array([0, NONE, NONE, NONE], np.uint32)
    d = DP.sweep(kw["cont"], kw["nodes"], kw["assign"], group, 1, kw["strategy"], 0, kw["node_count"], kw["domain"],
                 kw["max_skew"], kw["relax_mask"])
    assert d[2][0, D.STRANDED] == 0 and d[4][0, DP.SKEW_AFTER] == 3  # the drain moves them all and reports skew 3
    got = SP.sweep(**kw)
    assert np.array_equal(got[0][0], kw["assign"]) and got[2][0][0] == NONE and got[5][0][0] == SP.REASON_SKEW


# ---- theorem C: undo is exact, for each of the three causes -----------------------------------------------------
@pytest.mark.parametrize("strategy,n_dom,seed", ALL)
def test_theorem_c_undo_is_exact(strategy, n_dom, seed):
    case = _case(strategy, n_dom, seed)
    order, full = case[5], case[6]
    failing = [i for i, t in enumerate(full[7]) if t[1] != "OK"]
    tried = [int(n) for n in order]
    # the trace has one entry per attempt; map attempts back to positions of the order
    pos, gone = [], set()
    for i, n in enumerate(tried):
        if n not in gone:
            pos.append(i)
            if full[1][n] == SP.ST_RELEASED and full[7][len(pos) - 1][1] == "OK":
                gone.add(n)
    causes = set()
    for k in failing[:8]:
        i = pos[k]
        x = tried[i]
        causes.add(full[7][k][1])
        rest = _run(case, tried[:i] + tried[i + 1:], strategy)
        assert np.array_equal(rest[0], full[0]) and np.array_equal(rest[4], full[4])
        later = x in tried[i + 1:] or x in tried[:i]
        if not later:
            keep = np.arange(full[1].size) != x
            for w in (1, 2, 5):
                assert np.array_equal(rest[w][keep], full[w][keep])
            assert rest[1][x] == SP.ST_NEVER
        d = full[3].astype(np.int64) - rest[3].astype(np.int64)
        assert d[[SP.RELEASED, SP.MOVES, SP.MOVED, SP.MOVED_CPU, SP.MOVED_MEM]].tolist() == [0] * 5
        assert d[[SP.TRIED, SP.FAILED]].tolist() == [1, 1]
        dr = full[6].astype(np.int64) - rest[6].astype(np.int64)
        assert dr.tolist() == [int(full[7][k][1] != "NOFIT"), 0, 0, 0]
        for a, b in zip(full[8][0][:4], rest[8][0][:4]):  # the table the variant ends with
            assert np.array_equal(a, b)
        assert np.array_equal(full[8][1], rest[8][1])
    assert causes


# ---- theorem D: composition, step by step -----------------------------------------------------------------------
@pytest.mark.parametrize("strategy,n_dom,seed", ALL)
def test_theorem_d_composition_step_by_step(strategy, n_dom, seed):
    """Every attempt alone, on the state the committed ones before it left (the released server unschedulable,
    its node_count 0): the steps end where the whole order ends."""
    cont, live, assign, cnt, dom, order, full = _case(strategy, n_dom, seed)
    base, cur, c, released, steps = live, assign, cnt, [], []
    for x in (int(n) for n in order):
        if x in released:
            continue
        r = SP.variant(cont, base, cur, [x], strategy, 0, c, dom, MAX_SKEW, RELAX)
        steps.append(r[7][0][1:4])
        if r[1][x] == SP.ST_RELEASED:
            base, c, _ = r[8]
            c = c.copy()
            c[x] = 0
            cur = r[0]
            released.append(x)
    assert [t[1:4] for t in full[7]] == steps
    assert np.array_equal(cur, full[0]) and sorted(released) == np.flatnonzero(full[1] == SP.ST_RELEASED).tolist()
    for a, b in zip(base, full[8][0]):
        assert np.array_equal(a, b)
    live_left = np.where(full[8][2], 0, full[8][1])
    assert np.array_equal(c, live_left)
    assert SP.skew(c, dom, np.zeros(c.size, bool), base[4]) == full[6][SP.SKEW_AFTER]


# ---- theorem E: the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,n_dom,seed", ALL)
def test_theorem_e_bound(strategy, n_dom, seed):
    case = _case(strategy, n_dom, seed)
    order = case[5]
    for o in (order, order[::-1], np.roll(order, 11)):
        row = _run(case, o, strategy)[6]
        assert row[SP.SKEW_AFTER] <= max(MAX_SKEW, row[SP.SKEW_BEFORE])
    # and from a base state outside the bound: counts that put one domain far ahead
    cont, live, assign, cnt, dom = case[:5]
    heavy = cnt + np.where(dom == 0, 9, 0).astype(np.uint32)
    row = _run(case, order, strategy, domain=dom)[6]
    out = SP.variant(cont, live, assign, order, strategy, 0, heavy, dom, MAX_SKEW, RELAX)
    assert out[6][SP.SKEW_BEFORE] > MAX_SKEW and out[6][SP.SKEW_AFTER] <= out[6][SP.SKEW_BEFORE]
    assert row[SP.SKEW_BEFORE] <= MAX_SKEW


# ---- theorem F: validity under req_hop, and NONE entries ---------------------------------------------------------
@pytest.mark.parametrize("strategy,n_dom,seed", ALL)
def test_theorem_f_validity_and_none_entries(strategy, n_dom, seed):
    cont, live, assign, cnt, dom, order, full = _case(strategy, n_dom, seed)
    out, state, hops = full[0], full[1], full[4]
    (cf, mf, lab, cu, sched), cnt_end, gone = full[8]
    assert not np.isin(out[out != NONE], np.flatnonzero(state == SP.ST_RELEASED)).any()
    assert np.array_equal(out == NONE, assign == NONE)
    moved = np.flatnonzero(out != assign)
    cum = FR.cumulative(RELAX, len(RELAX))
    for c in moved:
        need = int(cont[2][c]) & ~cum[int(hops[c])]
        assert need & ~int(lab[out[c]]) == 0 and sched[out[c]]
        if hops[c]:
            assert (int(cont[2][c]) & ~cum[int(hops[c]) - 1]) & ~int(lab[out[c]]) != 0  # no smaller hop would do
    assert not hops[out == assign].any() or (hops[out == assign] == 0).all()
    # on the servers that are left, the table the variant ends with is the base table with the moved requests
    # taken from their new nodes (a released server keeps what it held when it was released)
    exp_cf = live[0].astype(np.int64)
    np.subtract.at(exp_cf, out[moved].astype(np.int64), cont[0][moved].astype(np.int64))
    assert np.array_equal(exp_cf[~gone], cf.astype(np.int64)[~gone]) and (exp_cf >= 0).all()
    holes = np.insert(np.asarray(order, np.uint32), [0, 5, 5, 17], NONE)
    again = SP.variant(cont, live, assign, holes, strategy, 0, cnt, dom, MAX_SKEW, RELAX)
    for a, b in zip(again[:7], full[:7]):
        assert np.array_equal(a, b)


# ---- the traps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(T.traps())))
def test_traps_on_the_reference(i):
    name, kw, expected = T.traps()[i]
    T.check(SP.sweep(**kw), expected, name)
    T.check(SP.sweep(**T.padded(kw, 70)), expected, name + ", padded")


def test_trap_contrasts():
    """What each trap would give without the rule it is about."""
    traps = {name: kw for name, kw, _ in T.traps()}
    # without the bound rule (no constraint at all) the example and the empty server are released
    for name in ("the A=5/B=5/C=7 example", "an empty server refused by the bound"):
        kw = dict(traps[name], max_skew=0)
        assert SP.sweep(**kw)[1][0][0] == SP.ST_RELEASED
    # the stale count: the service of node 3 alone, on the base state, goes where it goes after the undone attempt
    kw = traps["a stale domain count after an undone SKEW attempt"]
    assert SP.sweep(**dict(kw, try_order=[[3]]))[0][0].tolist() == [0, 0, 1]


# ---- the wrappers ---------------------------------------------------------------------------------------------------
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


class _Rec:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def export(*args):
            relax = [] if not _addr(args[12]) else list(ct.cast(ct.c_void_p(_addr(args[12])), ct.POINTER(ct.c_uint32))[:args[13]])
            self.calls.append((name, args, (_addr(args[10]), args[11], relax, args[13], _addr(args[18]), _addr(args[19]),
                                            _addr(args[20]))))
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


def test_shrink_sweep_policy_length_checks_and_call():
    p = _planner(_NoLib())
    cont, nodes = T._cont([1, 1]), T._nodes([9, 9, 9])
    fn = p.shrink_sweep_policy
    _refused("every container array must hold C entries", fn, (cont[0][:1],) + cont[1:], nodes, [0, 0], [[0, 1]])
    _refused("every node array must hold N entries", fn, cont, (nodes[0][:2],) + nodes[1:], [0, 0], [[0, 1]])
    _refused("assign must hold C entries", fn, cont, nodes, [0], [[0, 1]])
    _refused("try_order must be [n_var, n_try]", fn, cont, nodes, [0, 0], [0, 1])
    _refused("node_count must hold N entries", fn, cont, nodes, [0, 0], [[0, 1]], node_count=[0] * 4)
    _refused("domain must hold N entries", fn, cont, nodes, [0, 0], [[0, 1]], domain=[0, 1], max_skew=1)
    _refused("max_skew must be a u32", fn, cont, nodes, [0, 0], [[0, 1]], max_skew=1 << 32)
    _refused("relax_mask holds at most 4 hops", fn, cont, nodes, [0, 0], [[0, 1]], relax_mask=[1] * 5)
    lib = _Rec()
    p = _planner(lib)
    dom = np.array([0, 1, 1], np.uint32)
    got = p.shrink_sweep_policy(cont, nodes, [0, NONE], [[0, 1, NONE], [2, NONE, NONE]], "fill_lowest", -1, [4, 5, 6],
                                domain=dom, max_skew=2, relax_mask=[1, 6])
    (name, args, pol), = lib.calls
    assert name == "fp_shrink_sweep_policy" and len(args) == 21 == len(_lib.SIGNATURES[name][1])
    assert args[5:9] == (2, 3, _lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    out, state, blocker, summary, hops, why, rows = got
    assert pol == (dom.ctypes.data, 2, [1, 6], 2, hops.ctypes.data, why.ctypes.data, rows.ctypes.data)
    assert [_addr(args[i]) for i in (14, 15, 16, 17)] == [x.ctypes.data for x in (out, state, blocker, summary)]
    assert [x.shape for x in got] == [(2, 2), (2, 3), (2, 3), (2, 8), (2, 2), (2, 3), (2, 4)]
    assert [x.dtype for x in got] == [np.uint32, np.uint8, np.uint32, np.uint32, np.uint8, np.uint8, np.uint32]
    p.shrink_sweep_policy(cont, nodes, [0, 1], [[0]])
    assert lib.calls[1][2][:4] == (0, 0, [], 0)


def test_dev_shrink_sweep_policy_call_and_checks():
    torch = pytest.importorskip("torch")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    C, N, V, T_ = 3, 2, 2, 5
    cont_t, nodes_t = tuple(i32(C) for _ in range(4)), tuple(i32(N) for _ in range(4)) + (u8(N),)
    asg, tro, cnt, out, st, bl, sm = i32(C), i32(V * T_), i32(N), i32(V * C), u8(V * N), i32(V * N), i32(V * 8)
    dom, hp, br, pr = i32(N), u8(V * C), u8(V * N), i32(V * 4)
    lib = _Rec()
    q = _planner(lib)
    q.dev_shrink_sweep_policy(cont_t, nodes_t, asg, tro, V, out, st, sm, "pack_into_dedicated", 6, cnt, bl, domain_t=dom,
                              max_skew=3, relax_mask=[4], hops_t=hp, blocker_reason_t=br, policy_t=pr)
    (name, args, pol), = lib.calls
    assert name == "fp_dev_shrink_sweep_policy" and len(args) == 21 == len(_lib.SIGNATURES[name][1])
    assert args[5:9] == (V, T_, _lib.STRATEGY_PACK, 6)
    assert pol == (dom.data_ptr(), 3, [4], 1, hp.data_ptr(), br.data_ptr(), pr.data_ptr())
    assert [_addr(args[i]) for i in (3, 4, 9, 14, 15, 16, 17)] == [t.data_ptr() for t in (asg, tro, cnt, out, st, bl, sm)]
    q.dev_shrink_sweep_policy(cont_t, nodes_t, asg, tro, V, out, st, sm)
    assert lib.calls[1][2] == (0, 0, [], 0, 0, 0, 0)
    fn = _planner(_NoLib()).dev_shrink_sweep_policy
    base = (cont_t, nodes_t, asg, tro, V, out, st, sm)
    _refused("assign_t must hold C 32-bit entries", fn, cont_t, nodes_t, i32(C - 1), tro, V, out, st, sm)
    _refused("domain_t must hold N 32-bit entries", fn, *base, domain_t=i32(N + 1))
    _refused("relax_mask holds at most 4 hops", fn, *base, relax_mask=[1] * 5)
    _refused("hops_t must hold n_var * C bytes", fn, *base, hops_t=u8(C))
    _refused("blocker_reason_t must hold n_var * N bytes", fn, *base, blocker_reason_t=i32(V * N))
    _refused("policy_t must hold n_var * 4 32-bit entries", fn, *base, policy_t=i32(V * 4 + 1))
    _refused("max_skew must be a u32", fn, *base, max_skew=-1)


def test_abi_declares_the_policy_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    for name in ("fp_shrink_sweep_policy", "fp_dev_shrink_sweep_policy"):
        assert f"int {name}(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes" in hdr
        assert name in _lib.SIGNATURES and f"pub fn {name}(" in ffi
    assert "ffi::fp_shrink_sweep_policy(" in lib
    # the arguments behind fp_shrink_sweep's inputs, in the header's order, in ffi.rs and in the signature table
    tail = ["domain", "max_skew", "relax_mask", "n_hops", "assign_out", "state_out", "blocker_out", "summary_out", "hops_out",
            "blocker_reason_out", "policy_out"]
    for name in ("fp_shrink_sweep_policy", "fp_dev_shrink_sweep_policy"):
        params = re.search(rf"int {name}\((.*?)\);", hdr, re.S).group(1)
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in params.split(",")][10:] == tail
        rust = re.search(rf"pub fn {name}\((.*?)\)", ffi, re.S).group(1)
        assert re.findall(r"(\w+):", rust)[10:] == tail
        assert len(_lib.SIGNATURES[name][1]) == 10 + len(tail)
    words = re.search(r"enum \{ (FP_SHRINK_FAILED_SKEW.*?)\};", hdr, re.S).group(1)
    order = re.findall(r"FP_SHRINK_\w+", words)
    assert order == ["FP_SHRINK_FAILED_SKEW", "FP_SHRINK_RELAXED", "FP_SHRINK_SKEW_BEFORE", "FP_SHRINK_SKEW_AFTER",
                     "FP_SHRINK_POLICY_WORDS"]
    for val, name in enumerate(order):
        assert getattr(_lib, name[3:]) == val and re.search(rf"pub const {name}: usize = {val};", ffi), name
    assert (SP.FAILED_SKEW, SP.RELAXED, SP.SKEW_BEFORE, SP.SKEW_AFTER, SP.POLICY_WORDS) == (0, 1, 2, 3, 4)
    assert len(_lib.SHRINK_POLICY_FIELDS) == _lib.SHRINK_POLICY_WORDS


# ---- the flow level ------------------------------------------------------------------------------------------------
class _RefPlanner:
    """Both sweeps answered by the numpy references; remembers what it was asked."""

    def shrink_sweep(self, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None):
        self.asked = ("plain",)
        return S.sweep(cont, nodes, assign, try_order, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred, node_count)

    def shrink_sweep_policy(self, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None, *,
                            domain=None, max_skew=0, relax_mask=()):
        self.asked = ("policy", nodes, domain, max_skew, list(relax_mask), np.array(try_order))
        return SP.sweep(cont, nodes, assign, try_order, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred,
                        node_count, domain, max_skew, relax_mask)


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


def _kdl_flow():
    from fleetflow_amd.parser import parse_kdl_string
    servers = "\n".join(
        f'server "n{i}" {{ capacity cpu=3000 memory=8192; '
        + (f'label "region={"tokyo" if i % 2 == 0 else "osaka"}"; ' if i != 7 else "")
        + f'label "class={"gpu" if i in (1, 6) else "cpu"}" }}' for i in range(8))
    services = "\n".join(
        f'service "s{i}" {{ resources cpu={500 + 100 * (i % 3)} memory={512 * (1 + i % 2)}'
        + ('; require "class=gpu"' if i % 4 == 0 else "") + " }" for i in range(14))
    members = "\n".join(f'    service "s{i}"' for i in range(14)) + "\n" + "\n".join(f'    server "n{i}"' for i in range(8))
    return parse_kdl_string(KDL % (servers, services, members))


def _reference_plan(flow):
    """plan_stage's assignment, made by the numpy reference."""
    stage = flow.stages["live"]
    pol = stage.placement
    names = list(dict.fromkeys(stage.services))
    nodes = F._server_nodes(flow, stage.servers)
    cont, ntab = F._stage_tables(names, flow, nodes, pol.preferred)
    ld = F._stage_labels(names, flow, nodes, pol.preferred)
    domain, has_key = F.spread_domains(nodes, pol.spread[0])
    ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
    relax = [ld.key_mask(k) for k in pol.fallback]
    a, r, h, _, _ = FR.place(cont, ntab, _lib.POLICY_STRATEGIES[pol.strategy], 0, domain=domain, max_skew=pol.spread[1],
                             relax_mask=relax)
    plan = F.Plan("live", [], {}, [], {n: nodes[a[v]].slug for v, n in enumerate(names) if a[v] != NONE},
                  {n: "NOFIT" for v, n in enumerate(names) if a[v] == NONE})
    plan.strategy, plan.preferred = pol.strategy, pol.preferred
    plan.spread_topology_key, plan.spread_max_skew = pol.spread
    plan.fallback_relax_order, plan.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    plan.relaxed = {names[v]: ["class"] for v in range(len(names)) if a[v] != NONE and h[v]}
    return plan, names, nodes, relax


def test_shrink_stage_under_policy_from_kdl():
    flow = _kdl_flow()
    assert flow.stages["live"].placement.spread == ("region", 1) and flow.stages["live"].placement.fallback == ("class",)
    plan, names, nodes, relax = _reference_plan(flow)
    assert len(plan.assignment) == 14
    p = _RefPlanner()
    plain = F.shrink_stage(flow, "live", plan, planner=p)
    assert p.asked == ("plain",) and plain.spread_topology_key is None
    assert all(v.skew_before is None and not v.relaxed and not v.stayed_reason for v in plain.variants)
    rep = F.shrink_stage(flow, "live", plan, planner=p, under_policy=True)
    kind, live, domain, max_skew, masks, tro = p.asked
    assert kind == "policy" and max_skew == 1 and masks == relax and relax[0] != 0
    assert domain == F.replan_domains(nodes, "region")[0] and live[4][7] == 0  # n7 has no region: it takes no move
    assert (rep.spread_topology_key, rep.spread_max_skew, rep.fallback_relax_order) == ("region", 1, ["class"])
    names_, nodes_, cont, live0, assign, count, st, pmask = F.live_tables(flow, "live", plan)
    ref = SP.sweep(cont, live, assign, tro, _lib.POLICY_STRATEGIES[st], pmask, count, domain, 1, relax)
    slugs = [nd.slug for nd in nodes]
    for i, v in enumerate(rep.variants):
        out, state, blocker, row, hops, why, prow = (x[i] for x in ref)
        assert v.released == [slugs[n] for n in tro[i] if state[n] == SP.ST_RELEASED]
        assert sorted(v.moves) == sorted((names[c], slugs[assign[c]], slugs[out[c]]) for c in range(14) if out[c] != assign[c])
        held = [int(n) for n in tro[i] if state[n] == SP.ST_FAILED]
        assert v.stayed == [(slugs[n], names[blocker[n]] if blocker[n] != NONE else None) for n in held]
        assert v.stayed_reason == {slugs[n]: "BOUND" if blocker[n] == NONE else "SKEW" if why[n] == 3 else "NOFIT" for n in held}
        assert v.relaxed == {names[c]: ["class"] for c in range(14) if out[c] != assign[c] and hops[c]}
        assert (v.skew_before, v.skew_after) == (int(prow[SP.SKEW_BEFORE]), int(prow[SP.SKEW_AFTER]))
        assert v.skew_after <= max(1, v.skew_before)
    assert any(v.released for v in rep.variants) and any(v.stayed for v in rep.variants)
    # the two forms disagree on this stage: that is what the feature is for
    assert [v.released for v in rep.variants] != [v.released for v in plain.variants]
    best = rep.variants[rep.best]
    moved = {m[0] for m in best.moves}
    assert rep.plan.relaxed == {**{s: k for s, k in plan.relaxed.items() if s not in moved}, **best.relaxed}
    assert not set(rep.plan.assignment.values()) & set(best.released)
    # an explicit policy replaces the plan's own
    only_chain = F.PlacementPolicy("spread_across_pool", fallback_relax_order=("class",))
    rep2 = F.shrink_stage(flow, "live", plan, planner=p, policy=only_chain, under_policy=True)
    assert p.asked[2] is None and p.asked[3] == 0 and rep2.spread_topology_key is None and rep2.fallback_relax_order == ["class"]
    assert all(v.skew_before is None for v in rep2.variants)


def test_report_text_and_json_with_and_without_the_new_fields():
    flow = _kdl_flow()
    plan, *_ = _reference_plan(flow)
    p = _RefPlanner()
    plain = F.shrink_stage(flow, "live", plan, planner=p)
    js = PO.shrink_report_to_json(plain)
    for key in ("relaxed", "stayed_reason", "skew_before", "skew_after", '"spread"', '"fallback"'):
        assert key not in js.replace(PO.plan_to_json(plain.plan), "")  # the plan inside carries its own policy
    variants = __import__("json").loads(js)["variants"]
    assert all(set(v) == {"name", "order", "released", "moves", "stayed", "tried", "failed", "n_moves", "moved_cpu_m",
                          "moved_mem_mib"} for v in variants)
    text = PO.format_shrink_report(plain)
    assert "spread:" not in text and "relaxed" not in text and "bound rule" not in text
    assert PO.shrink_report_from_json(js) == plain
    rep = F.shrink_stage(flow, "live", plan, planner=p, under_policy=True)
    js = PO.shrink_report_to_json(rep)
    back = PO.shrink_report_from_json(js)
    assert back == rep and PO.shrink_report_to_json(back) == js
    d = __import__("json").loads(js)
    assert d["placement"]["spread"] == {"topology_key": "region", "max_skew": 1}
    assert d["placement"]["fallback"] == {"relax_order": ["class"], "max_hops": None}
    text = PO.format_shrink_report(rep)
    lines = text.split("\n")
    for v in rep.variants:
        assert f"  spread: skew over region {v.skew_before} -> {v.skew_after} (max_skew 1)" in lines
        for svc, src, dst in v.moves:
            tail = f" (relaxed: {', '.join(v.relaxed[svc])})" if svc in v.relaxed else ""
            assert f"  {svc}: {src} -> {dst}{tail}" in lines
        for srv, svc in v.stayed:
            if svc is None:
                assert any(ln.startswith(f"  {srv}: stays (bound rule: ") for ln in lines)
            else:
                assert f"  {srv}: stays (blocked by {svc}, {v.stayed_reason[srv]})" in lines
    # a hand-made variant with every new field, so that the text of each is pinned
    v = F.ShrinkVariant("fewest", ["a", "b", "c"], ["a"], [("s1", "a", "b")], [("b", "s2"), ("c", None)], 3, 2, 1, 100, 64,
                        {"s1": ["class"]}, {"b": "SKEW", "c": "BOUND"}, 1, 2)
    r = F.ShrinkReport("live", "spread_across_pool", [], [], [v], 0, None, "region", 2, ["class"], 1)
    assert PO.format_shrink_report(r).split("\n") == [
        "shrink fewest: 1 of 3 servers released, 1 services move (100m cpu, 64 MiB), 2 attempts undone (best)",
        "  released: a",
        "  s1: a -> b (relaxed: class)",
        "  b: stays (blocked by s2, SKEW)",
        "  c: stays (bound rule: its release would leave the skew over region above max_skew 2 and above what it is)",
        "  spread: skew over region 1 -> 2 (max_skew 2)"]
    assert PO.shrink_report_from_json(PO.shrink_report_to_json(r)) == r
