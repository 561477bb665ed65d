"""CPU tests of the scale-out sweep under the policy (SPEC.md 2.18): the theorems of the SPEC on the numpy
reference (tests/grow_policy_ref.py), the cases the section argues from, ``grow_stage(under_policy=True)`` on a
stub planner that answers with the reference, and the report's text and JSON forms.  No GPU."""
import ctypes as ct
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_policy_ref as GP  # noqa: E402
import grow_ref as G  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402
from fleetflow_amd.registry import plan_template  # noqa: E402

NONE = 0xFFFFFFFF
NOFIT, SKEW = 1 << 1, 1 << 3
RELAX = (0x780, 0x78)  # the generator's class bits, then its region bits
SEEDS = (0x5EED0021, 0x5EED0022, 0x5EED0023)
SHAPES = ((300, 24, 3, 1), (300, 24, 4, 2), (200, 12, 3, 1))  # C, N, domains, max_skew


def _u32(*xs):
    return tuple(np.ascontiguousarray(x, dtype=np.uint32) for x in xs)


@functools.lru_cache(maxsize=None)
def _base(seed, strategy, shape):
    """A live plan under the policy, made by the 2.8 reference on the generator's fleet."""
    from oracle import pyoracle as P
    C, N, n_dom, max_skew = shape
    cont = _u32(*P.gen_containers(P.scenario_seed(seed, 0), C, 7))
    nodes = P.gen_nodes(P.scenario_seed(seed, 0), N)
    nodes = _u32(*nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8),)
    domain = (np.arange(N) % n_dom).astype(np.uint32)
    _, reason, _, live, cnt = FR.place(cont, nodes, strategy, 0, domain=domain, max_skew=max_skew, relax_mask=list(RELAX))
    return cont, live, cnt, domain, reason


def _templates(n_dom):
    """Four templates: in the populated domain 0, in a new domain, a small one in domain 1, a large one in the last."""
    return (_u32([16000, 16000, 8000, 64000], [32768, 32768, 16384, 262144], [0x1FFF, 0x1FFF, 0x0489, 0x1FFF]),
            _u32([0, n_dom, 1, n_dom - 1])[0])


def _sweep(seed, strategy, shape, t_max=None, max_new=12, **kw):
    cont, live, cnt, domain, reason = _base(seed, strategy, shape)
    tpl, td = _templates(shape[2])
    args = dict(strategy=strategy, node_count=cnt, domain=domain, t_domain=td, max_skew=shape[3], relax_mask=RELAX)
    args.update(kw)
    return GP.sweep(cont, reason, live, tpl, max_new, NOFIT | SKEW, t_max, **args)


GRID = [(seed, strategy, shape) for seed in SEEDS for strategy in range(4) for shape in SHAPES]


@pytest.mark.parametrize("seed,strategy,shape", GRID)
def test_prefix_cap_irrelevance_partition_and_independence(seed, strategy, shape):
    """144 candidates: 3 seeds x 4 strategies x 3 shapes x 4 templates."""
    N = shape[1]
    rows, pol, assign, hops, why = _sweep(seed, strategy, shape)
    for k in range(4):
        new = np.unique(assign[k][(assign[k] != NONE) & (assign[k] >= N)])
        opened = int(rows[k, G.OPENED])
        assert new.tolist() == list(range(N, N + opened))  # PREFIX
        assert rows[k, G.PENDING] == (rows[k, G.PLACED] + rows[k, G.UNPLACEABLE] + rows[k, G.CAPPED]
                                      + pol[k, GP.STUCK_SKEW] + pol[k, GP.STUCK_QUOTA])  # PARTITION
        assert pol[k, GP.ON_LIVE] + int(((assign[k] != NONE) & (assign[k] >= N)).sum()) == rows[k, G.PLACED]
    # CAP IRRELEVANCE: one server more than the sweep opened gives the same rows and per-container results
    caps = np.minimum(rows[:, G.OPENED] + 1, 12)
    again = _sweep(seed, strategy, shape, t_max=caps)
    for k in np.flatnonzero(rows[:, G.OPENED] < 12):
        for a, b in zip((rows, pol, assign, hops, why), again):
            assert np.array_equal(a[k], b[k])
    # INDEPENDENCE: a sweep equals single-candidate sweeps (one is enough per grid point: the third)
    cont, live, cnt, domain, reason = _base(seed, strategy, shape)
    tpl, td = _templates(shape[2])
    one = GP.sweep(cont, reason, live, tuple(x[2:3] for x in tpl), 12, NOFIT | SKEW, None, strategy, 0, cnt, domain,
                   td[2:3], shape[3], RELAX)
    for a, b in zip((rows, pol, assign, hops, why), one):
        assert np.array_equal(a[2], b[0])


def test_a_cap_of_exactly_opened_keeps_the_assignments_and_may_turn_skew_into_nofit():
    """What the cap-irrelevance theorem does NOT claim: with t_max = OPENED the last empty server is gone, and a
    pending service it would have fitted (rejected on the skew) now fits nowhere."""
    turned = 0
    for seed, strategy, shape in GRID[:12]:
        rows, pol, assign, hops, why = _sweep(seed, strategy, shape)
        exact = _sweep(seed, strategy, shape, t_max=rows[:, G.OPENED])
        assert np.array_equal(exact[2], assign) and np.array_equal(exact[3], hops)
        assert ((why != exact[4]) <= ((why == 3) & (exact[4] == 1))).all()
        turned += int((why != exact[4]).sum())
    assert turned > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_anchor_without_a_live_table_or_a_guarantee_it_is_the_plain_sweep(seed):
    cont, _, _, _, reason = _base(seed, 0, SHAPES[0])
    tpl, _ = _templates(3)
    none = _u32([], [], [], []) + (np.zeros(0, np.uint8),)
    caps = [12, 3, 0, 7]
    rows, pol, assign, hops, why = GP.sweep(cont, reason, none, tpl, 12, NOFIT | SKEW, caps)
    exp = G.sweep(cont, reason, tpl, 12, NOFIT | SKEW, caps)
    assert np.array_equal(rows, exp[0]) and np.array_equal(assign, exp[1]) and not pol.any() and not hops.any()
    pend = (reason == 1) | (reason == 3)
    assert np.array_equal(why, np.where(pend[None, :] & (assign == NONE), 1, 0))


@pytest.mark.parametrize("seed", SEEDS)
def test_append_theorem_against_the_c_oracle(seed, O):
    """First fit, no guarantee, the pending the NOFIT of a first-fit plan: nothing lands on a live server and the
    new servers are 2.12's, N further on."""
    C, N = 400, 24
    cont, nodes = O.gen_scenario(seed, 3, C, N, 7)
    _, reason, after, _ = O.place(cont, nodes)
    assert 10 < int((reason == 1).sum())
    tpl, _ = _templates(3)
    rows, pol, assign, _, why = GP.sweep(cont, reason, after, tpl, 16, NOFIT)
    exp_rows, exp = G.sweep(cont, reason, tpl, 16, NOFIT)
    assert np.array_equal(rows, exp_rows) and not pol[:, GP.ON_LIVE].any()
    assert np.array_equal(assign, np.where(exp == NONE, NONE, exp.astype(np.int64) + N).astype(np.uint32))


def test_where_the_new_servers_stand_decides():
    """The issue's figures: seed 0x5EED0023, 200 containers on 12 nodes in three domains, max_skew 1, spread, twelve
    8000 m / 16 GiB servers for the 114 pending (7 NOFIT, 107 SKEW)."""
    cont, live, cnt, domain, reason = _base(0x5EED0023, 1, SHAPES[2])
    assert (int((reason == 1).sum()), int((reason == 3).sum())) == (7, 107)
    tpl = _u32([8000] * 3, [16384] * 3, [0x0489] * 3)
    rows, pol, assign, hops, why = GP.sweep(cont, reason, live, tpl, 12, NOFIT | SKEW, None, 1, 0, cnt, domain, [0, 1, 3], 1,
                                            RELAX)
    assert rows[:, G.PENDING].tolist() == [114] * 3
    assert rows[0, G.PLACED] == 0 and pol[0, GP.STUCK_SKEW] == 107  # in the populated domain 0: nothing
    assert (rows[1, G.PLACED], pol[1, GP.ON_LIVE], pol[1, GP.RELAXED]) == (72, 48, 4)  # in the starved domain 1
    assert rows[2, G.PLACED] > 0 and pol[2, GP.ON_LIVE] == 0 and pol[2, GP.SKEW_BEFORE] > 1  # in a new domain
    # the plain sweep sees the 7 NOFIT only, and no live server
    plain, _ = G.sweep(cont, reason, tpl, 12)
    assert plain[:, G.PENDING].tolist() == [7] * 3
    # a quota on the services: admission comes first, the refused are neither SKEW nor NOFIT
    rows, pol, _, _, why = GP.sweep(cont, reason, live, tpl, 12, NOFIT | SKEW, None, 1, 0, cnt, domain, [0, 1, 3], 1, RELAX,
                                    (None, None, 100), (0, 0, 86))
    assert pol[1, GP.STUCK_QUOTA] > 0 and rows[1, G.PLACED] == 14 and (why[1] == 4).sum() == pol[1, GP.STUCK_QUOTA]
    # a template that lacks a relaxable label is not UNPLACEABLE for the services the chain lets through
    bare = _u32([8000], [16384], [0x0001])
    with_chain = GP.sweep(cont, reason, live, bare, 12, NOFIT | SKEW, None, 1, 0, cnt, domain, [1], 1, RELAX)
    no_chain = GP.sweep(cont, reason, live, bare, 12, NOFIT | SKEW, None, 1, 0, cnt, domain, [1], 1)
    assert with_chain[0][0, G.UNPLACEABLE] < no_chain[0][0, G.UNPLACEABLE]


def test_abi_declares_the_policy_grow_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    for name in ("fp_grow_sweep_policy", "fp_dev_grow_sweep_policy"):
        assert f"int {name}(fp_ctx *ctx, const fp_containers *c, const uint8_t *reason, uint32_t reason_mask" in hdr
        assert name in _lib.SIGNATURES and f"pub fn {name}(" in ffi and len(_lib.SIGNATURES[name][1]) == 26
    assert "ffi::fp_grow_sweep_policy(" in lib and "pub fn grow_sweep_policy(" in lib
    m = re.search(r"enum \{ (FP_GROW_ON_LIVE[^}]*)\}", hdr)
    names = re.findall(r"FP_GROW_\w+", m.group(1))
    assert names == ["FP_GROW_ON_LIVE", "FP_GROW_RELAXED", "FP_GROW_STUCK_SKEW", "FP_GROW_STUCK_QUOTA",
                     "FP_GROW_SKEW_BEFORE", "FP_GROW_SKEW_AFTER", "FP_GROW_POLICY_WORD6", "FP_GROW_POLICY_WORD7",
                     "FP_GROW_POLICY_WORDS"]
    for val, name in enumerate(names):  # an enum without initialisers: the position is the value
        if "WORD6" in name or "WORD7" in name:
            continue
        assert getattr(_lib, name[3:]) == val
        assert re.search(rf"pub const {name}: usize = {val};", ffi), name
    assert (GP.ON_LIVE, GP.RELAXED, GP.STUCK_SKEW, GP.STUCK_QUOTA, GP.SKEW_BEFORE, GP.SKEW_AFTER, GP.POLICY_WORDS) == (
        0, 1, 2, 3, 4, 5, 8)
    assert len(_lib.GROW_POLICY_FIELDS) == 6


# ---- the wrappers: length checks first, then what reaches the export -------------------------------------

def _addr(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "_obj"):
        return ct.addressof(x._obj)
    return ct.cast(x, ct.c_void_p).value or 0


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


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
    from fleetflow_amd import Planner
    q = object.__new__(Planner)
    q._L, q._ctx, q._tstream, q.device = lib, ct.c_void_p(0x5EED), None, 0
    q._dev = lambda fn, *a: fn(*a)
    return q


def _refused(msg, fn, *a, **kw):
    with pytest.raises(ValueError, match=re.escape(msg)):
        fn(*a, **kw)


def test_grow_sweep_policy_length_checks_and_call():
    cont, tpl = _u32([1, 1], [1, 1], [0, 0], [0, 0]), _u32([9] * 3, [9] * 3, [0] * 3)
    live = _u32([5, 5], [5, 5], [0, 0], [0, 0]) + (np.ones(2, np.uint8),)
    fn = _planner(_NoLib()).grow_sweep_policy
    _refused("every container array must hold C entries", fn, (cont[0][:1], *cont[1:]), [1, 1], live, tpl, 4)
    _refused("every node array must hold N entries", fn, cont, [1, 1], (*live[:4], live[4][:1]), tpl, 4)
    _refused("every template array must hold n_cand entries", fn, cont, [1, 1], live, (tpl[0][:2], *tpl[1:]), 4)
    _refused("reason must hold C entries", fn, cont, [1], live, tpl, 4)
    _refused("t_max must hold n_cand entries", fn, cont, [1, 1], live, tpl, 4, t_max=[1])
    _refused("node_count must hold N entries", fn, cont, [1, 1], live, tpl, 4, node_count=[1])
    _refused("domain must hold N entries", fn, cont, [1, 1], live, tpl, 4, domain=[0], t_domain=[0, 0, 0], max_skew=1)
    _refused("t_domain must hold n_cand entries", fn, cont, [1, 1], live, tpl, 4, domain=[0, 0], t_domain=[0], max_skew=1)
    _refused("max_skew must be a u32", fn, cont, [1, 1], live, tpl, 4, max_skew=-1)
    _refused("relax_mask holds at most 4 hops", fn, cont, [1, 1], live, tpl, 4, relax_mask=[1] * 5)
    _refused("quota_used must hold 3 entries", fn, cont, [1, 1], live, tpl, 4, quota=(1, 2, 3), quota_used=(1, 2))
    lib = _Rec(peek={5: 2, 14: 2, 15: 3, 17: 2, 19: 3, 20: 3})
    p = _planner(lib)
    out = p.grow_sweep_policy(cont, [1, 3], live, tpl, 16, NOFIT | SKEW, [16, 0, 3], "fill_lowest", 6, [2, 1],
                              domain=[0, 1], t_domain=[1, 2, 63], max_skew=2, relax_mask=(8, 16), quota=(None, 7, 9),
                              quota_used=(1, 2, 3), want_assign=True)
    (name, args, seen), = lib.calls
    assert name == "fp_grow_sweep_policy" and len(args) == 26 == len(_lib.SIGNATURES[name][1]) and _addr(args[0]) == 0x5EED
    assert seen == {5: [2, 1], 14: [0, 1], 15: [1, 2, 63], 17: [8, 16], 19: [NONE, 7, 9], 20: [1, 2, 3]}
    assert (args[3], args[6], args[11], args[12], args[13], args[16], args[18]) == (NOFIT | SKEW, 3, 16, 3, 6, 2, 2)
    assert args[4]._obj.n == 2 and args[4]._obj.cpu_free == live[0].ctypes.data  # the live table is not copied
    assert [_addr(args[i]) for i in range(21, 26)] == [x.ctypes.data for x in out]
    assert [x.shape for x in out] == [(3, 8), (3, 8), (3, 2), (3, 2), (3, 2)]
    lib = _Rec()
    bare = _planner(lib)  # p is kept: a planner that goes away closes its context through the library
    rows, pol, a, h, r = bare.grow_sweep_policy(cont, None, live, tpl, 4, 0)  # nothing optional: NULLs
    args = lib.calls[0][1]
    assert (a, h, r) == (None, None, None)
    assert [_addr(args[i]) for i in (2, 5, 10, 14, 15, 17, 19, 20, 23, 24, 25)] == [0] * 11 and args[18] == 0


def test_dev_grow_sweep_policy_call_and_checks():
    torch = pytest.importorskip("torch")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    C, N, K = 3, 2, 2
    cont_t, tpl_t = tuple(i32(C) for _ in range(4)), tuple(i32(K) for _ in range(3))
    nodes_t = tuple(i32(N) for _ in range(4)) + (u8(N),)
    rs, sm, pol, out, hp, why = u8(C), i32(K * 8), i32(K * 8), i32(K * C), u8(K * C), u8(K * C)
    dom, td, cnt = i32(N), i32(K), i32(N)
    lib = _Rec(peek={17: 1, 19: 3, 20: 3})
    q = _planner(lib)
    q.dev_grow_sweep_policy(cont_t, rs, nodes_t, tpl_t, 100, sm, 10, None, 1, 0, cnt, domain_t=dom, t_domain_t=td,
                            max_skew=1, relax_mask=(0x18,), quota=(None, None, 5), quota_used=(0, 0, 1), policy_t=pol,
                            assign_out_t=out, hops_t=hp, reason_out_t=why)
    (name, args, seen), = lib.calls
    assert name == "fp_dev_grow_sweep_policy" and len(args) == 26 == len(_lib.SIGNATURES[name][1])
    assert seen == {17: [0x18], 19: [NONE, NONE, 5], 20: [0, 0, 1]}  # the three host arrays
    assert (args[4]._obj.n, args[4]._obj.schedulable) == (N, nodes_t[4].data_ptr())
    assert [_addr(args[i]) for i in (2, 5, 14, 15, 21, 22, 23, 24, 25)] == [
        t.data_ptr() for t in (rs, cnt, dom, td, sm, pol, out, hp, why)]
    fn = _planner(_NoLib()).dev_grow_sweep_policy
    _refused("every node tensor must hold N entries", fn, cont_t, rs, nodes_t[:4] + (i32(N),), tpl_t, 100, sm)
    _refused("count_t must hold N 32-bit entries", fn, cont_t, rs, nodes_t, tpl_t, 100, sm, count_t=i32(N + 1))
    _refused("t_domain_t must hold n_cand 32-bit entries", fn, cont_t, rs, nodes_t, tpl_t, 100, sm, t_domain_t=i32(K + 1))
    _refused("policy_t must hold n_cand * 8 32-bit entries", fn, cont_t, rs, nodes_t, tpl_t, 100, sm, policy_t=i32(K * 4))
    _refused("hops_t must hold n_cand * C bytes", fn, cont_t, rs, nodes_t, tpl_t, 100, sm, hops_t=i32(K * C))
    _refused("reason_out_t must hold n_cand * C bytes", fn, cont_t, rs, nodes_t, tpl_t, 100, sm, reason_out_t=u8(C))


# ---- the flow level ------------------------------------------------------------------------------------

class _RefPlanner:
    """The two sweeps answered by the numpy references; remembers what it was asked."""

    def grow_sweep(self, cont, reason, templates, max_new, reason_mask=1 << 1, t_max=None, want_assign=False):
        self.asked = ("plain", cont, reason, templates, max_new, reason_mask)
        rows, assign = G.sweep(cont, reason, templates, max_new, reason_mask, t_max)
        return rows, (assign if want_assign else None)

    def grow_sweep_policy(self, cont, reason, nodes, templates, max_new, reason_mask=1 << 1, t_max=None, strategy=0,
                          preferred=0, node_count=None, *, domain=None, t_domain=None, max_skew=0, relax_mask=(),
                          quota=None, quota_used=None, want_assign=False):
        self.asked = ("policy", cont, reason, nodes, templates, max_new, reason_mask, strategy, preferred, node_count,
                      domain, t_domain, max_skew, list(relax_mask), quota, quota_used)
        out = GP.sweep(cont, reason, nodes, templates, max_new, reason_mask, t_max,
                       _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred, node_count, domain, t_domain, max_skew,
                       relax_mask, quota, quota_used)
        return out if want_assign else (out[0], out[1], None, None, None)


KDL = '''project "demo"
%s
%s
stage "live" {
%s
    placement strategy="spread_across_pool" { spread "region" max-skew=1; fallback "class" }
}
'''


def _kdl_flow():
    """Two large servers in tokyo and in nagoya, one small one in osaka that takes a single service, one without a
    region: under max-skew=1 osaka holds the minimum down and most of the stage is SKEW."""
    from fleetflow_amd.parser import parse_kdl_string
    spec = [("t0", 8000, "tokyo"), ("t1", 8000, "tokyo"), ("o0", 500, "osaka"), ("n0", 8000, "nagoya"),
            ("n1", 8000, "nagoya"), ("x0", 8000, None)]
    servers = "\n".join(f'server "{s}" {{ capacity cpu={cpu} memory=32768; '
                        + (f'label "region={r}"; ' if r else "") + 'label "class=cpu" }' for s, cpu, r in spec)
    services = "\n".join(f'service "s{i}" {{ resources cpu={300 + 10 * (i % 3)} memory=256'
                         + ('; require "class=gpu"' if i == 7 else "") + " }" for i in range(20))
    members = "\n".join(f'    service "s{i}"' for i in range(20)) + "\n" + "\n".join(f'    server "{s}"' for s, _, _ in spec)
    return parse_kdl_string(KDL % (servers, services, members))


def _plan_under_the_policy(flow):
    stage = flow.stages["live"]
    pol = stage.placement
    nodes = [flow.servers[s] for s in stage.servers]
    names = list(stage.services)
    cont, ntab = F._stage_tables(names, flow, nodes, pol.preferred)
    ld = F._stage_labels(names, flow, nodes, pol.preferred)
    domain, has_key = F.replan_domains(nodes, "region")
    ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
    relax = [ld.key_mask(k) for k in pol.fallback]
    a, r, h, after, cnt = FR.place(cont, ntab, _lib.STRATEGY_SPREAD, 0, domain=domain, max_skew=1, relax_mask=relax)
    plan = F.Plan("live", [], {}, [], {n: stage.servers[a[v]] for v, n in enumerate(names) if a[v] != NONE},
                  {n: {1: "NOFIT", 3: "SKEW"}[int(r[v])] for v, n in enumerate(names) if a[v] == NONE})
    plan.strategy, plan.spread_topology_key, plan.spread_max_skew = pol.strategy, "region", 1
    plan.fallback_relax_order, plan.fallback_max_hops = ["class"], pol.fallback_max_hops
    return plan, names, relax


CATALOGUE = [plan_template("8core-16gb", {"region": "tokyo", "class": "cpu"}, name="big-tokyo"),
             plan_template("8core-16gb", {"region": "osaka", "class": "cpu"}, name="big-osaka"),
             plan_template("8core-16gb", {"region": "kyoto", "class": "cpu"}, name="big-kyoto"),
             plan_template("8core-16gb", {"class": "cpu"}, name="big-nowhere")]


def test_grow_stage_under_the_policy_on_a_kdl_stage():
    flow = _kdl_flow()
    plan, names, relax = _plan_under_the_policy(flow)
    skew = [n for n in names if plan.rejected.get(n) == "SKEW"]
    assert len(skew) >= 10 and len(plan.assignment) <= 8
    p = _RefPlanner()
    # today's call: the SKEW services are not pending at all
    rep = F.grow_stage(flow, "live", plan, CATALOGUE, max_new=4, planner=p)
    assert p.asked[0] == "plain" and not set(rep.pending) & set(skew) and not rep.under_policy
    assert all(c.on_live is None and not c.moved_in for c in rep.candidates)
    rep = F.grow_stage(flow, "live", plan, CATALOGUE, max_new=4, planner=p, under_policy=True)
    kind, _, reason, live, tpl, max_new, mask, strategy, pmask, count, dom, td, max_skew, rm, quota, used = p.asked
    assert kind == "policy" and mask == NOFIT | SKEW and strategy == "spread_across_pool" and (max_skew, rm) == (1, relax)
    assert rep.under_policy and rep.pending == [n for n in names if n in plan.rejected] and set(skew) <= set(rep.pending)
    # the stage's numbering: tokyo 0, osaka 1, nagoya 2, the keyless server the spare 3; kyoto is new: 4
    assert dom == [0, 0, 1, 2, 2, 3] and td == [0, 1, 4] and list(live[4]) == [1, 1, 1, 1, 1, 0]
    assert len(tpl[0]) == 3 and quota is None and sum(count) == len(plan.assignment)
    by = {c.name: c for c in rep.candidates}
    assert by["big-nowhere"].no_topology_key and by["big-nowhere"].placed == 0 and by["big-nowhere"].servers is None
    assert by["big-nowhere"].pending == len(rep.pending)
    # the zone of the template changes the answer: tokyo is populated, osaka is the starved zone, kyoto is new
    assert by["big-tokyo"].placed == 0 and by["big-tokyo"].stuck_skew == len(skew)
    assert by["big-osaka"].placed > by["big-kyoto"].placed > 0
    assert by["big-osaka"].on_live == len(by["big-osaka"].moved_in) > 0 and by["big-kyoto"].on_live == 0
    assert by["big-osaka"].domain == "region=osaka" and by["big-osaka"].skew_before >= 1
    assert {dst for _, dst in by["big-osaka"].moved_in} <= {"t0", "t1", "n0", "n1"}
    placed = [s for srv in by["big-osaka"].servers for s in srv] + [s for s, _ in by["big-osaka"].moved_in]
    assert len(placed) == by["big-osaka"].placed == len(set(placed))
    assert by["big-osaka"].relaxed.get("s7") == ["class"] or "s7" not in placed
    text = PO.format_grow_report(rep)
    assert "grow big-nowhere: no candidate: no region label" in text and "on existing servers" in text
    assert f"  {by['big-osaka'].moved_in[0][0]}: -> {by['big-osaka'].moved_in[0][1]}" in text
    assert PO.grow_report_from_json(PO.grow_report_to_json(rep)) == rep
    # an explicit policy overrides the plan's: a quota, and the usage the plan left
    plan.quota_used = (1500, 1280, 5)
    capped = F.PlacementPolicy("spread_across_pool", {}, "region", 1, ("class",), None, None, None, 8)
    rep = F.grow_stage(flow, "live", plan, CATALOGUE[1:2], max_new=4, planner=p, policy=capped, under_policy=True)
    assert p.asked[14:] == ((None, None, 8), (1500, 1280, 5)) and rep.quota == (None, None, 8)
    assert rep.candidates[0].placed == 3 and rep.candidates[0].stuck_quota > 0
    # a 65th domain is refused
    many = [plan_template("2core-4gb", {"region": f"r{i}"}, name=f"r{i}") for i in range(61)]
    with pytest.raises(ValueError, match="distinct domains"):
        F.grow_stage(flow, "live", plan, many, planner=p, under_policy=True)
    F.grow_stage(flow, "live", plan, many[:60], max_new=1, planner=p, under_policy=True)  # 4 + 60 = 64 fit


def test_report_with_the_new_fields_and_without():
    rep = F.GrowReport("live", 4, ["db", "web", "batch"], [
        F.GrowCandidate("big-east", 8000, 16384, ["region=east"], 4, 3, 3, 1, 0, 0, 4000, 9000, None, [["batch"]],
                        2, {"db": ["class"]}, 0, 0, 3, 1, "region=east", [("db", "a1"), ("web", "b1")]),
        F.GrowCandidate("bare", 1000, 1024, [], 4, 3, no_topology_key=True)],
        True, "spread_across_pool", [], "region", 1, ["class"], None, (None, None, 9), (100, 200, 3))
    assert PO.format_grow_report(rep) == (
        "grow big-east: 1 new servers take 3 of 3 services, 0 fit no such server, 0 over the cap of 4; 2 on existing "
        "servers, 1 relaxed, 0 held by the skew, 0 by the quota [region=east: skew 3 -> 1]\n"
        "  +0: batch\n"
        "  db: -> a1\n"
        "  web: -> b1\n"
        "grow bare: no candidate: no region label")
    text = PO.grow_report_to_json(rep)
    back = PO.grow_report_from_json(text)
    assert back == rep and PO.grow_report_to_json(back) == text
    plain = F.GrowReport("live", 8, ["db"], [F.GrowCandidate("small", 1000, 1024, [], 8, 1, 1, 1, 0, 0, 0, 512, None)])
    text = PO.grow_report_to_json(plain)
    assert not any(key in text for key in ("on_live", "moved_in", "stuck_skew", "placement", "no_topology_key"))
    assert PO.grow_report_from_json(text) == plain
