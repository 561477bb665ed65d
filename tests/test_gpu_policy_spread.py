"""GPU tests of the hard topology spread (SPEC.md 2.7; k_policy<.., true> in fleetflow_amd/csrc/fp_policy.hip):
every entry point against the numpy reference (tests/policy_spread_ref.py).  Every comparison is exact:
assign, reason, the three mutated node arrays, node_count and the packed cost."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import policy_spread_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 0x5EED0004
PREF2 = (1 << 4) | (1 << 8)


@functools.lru_cache(maxsize=None)
def _scenario(C, N, flags, scen=3):
    from oracle import oracle as O
    cont, nodes = O.gen_scenario(SEED, scen, C, N, flags)
    for a in (*cont, *nodes):
        a.setflags(write=False)
    return cont, nodes


@functools.lru_cache(maxsize=None)
def _domains(kind, N, D):
    """'mod': n % D.  'lop': lopsided, min(floor(u^3 * D), D - 1): the low domains hold most nodes."""
    if kind == "mod":
        d = (np.arange(N) % D).astype(np.uint32)
    else:
        u = np.random.default_rng(N).random(N)
        d = np.minimum(np.floor(u ** 3 * D), D - 1).astype(np.uint32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _unconstrained(C, N, flags, strategy):
    return R.place(*_scenario(C, N, flags), strategy)


def _check(got, exp, sid=None):
    """got: (assign, reason, cost or None, nodes_after, count or None); exp: the reference's tuple."""
    assign, reason, cost, after, cnt = got
    assert np.array_equal(assign, exp[0])
    assert np.array_equal(reason, exp[1])
    for i in (0, 1, 3):
        assert np.array_equal(after[i], exp[2][i]), i
    if cnt is not None:
        assert np.array_equal(cnt, exp[3])
    if cost is not None:
        assert int(cost) == SR.cost(exp[0], exp[1], sid)


def _run1(planner, cont, nodes, strategy, domain, max_skew, preferred=0, level=None, node_count=None, sid=0):
    """One scenario through the batch entry (it returns the cost too)."""
    C, N = cont[0].size, nodes[0].size
    a, r, cost, after, cnt = planner.place_batch_policy(1, C, N, cont, nodes, [strategy], [preferred], level=level,
                                                        node_count=node_count, scen_base=sid, domain=domain,
                                                        max_skew=[max_skew])
    return a, r, cost[0], after, cnt


# every instantiation (64 x 1, 1024 x {1, 2, 4, 8}) at an edge: (C, N, generator flags, domains)
SHAPES = [(300, 1, 7, 1), (300, 64, 7, 3), (300, 65, 0, 64), (2000, 1024, 7, 5), (300, 2049, 0, 7), (2000, 4096, 7, 64),
          (2000, 8192, 7, 4)]


@pytest.mark.parametrize("kind", ["mod", "lop"])
@pytest.mark.parametrize("max_skew", [1, 2])
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("C,N,flags,D", SHAPES)
def test_every_strategy_vs_reference(C, N, flags, D, strategy, max_skew, kind, planner):
    cont, nodes = _scenario(C, N, flags)
    dom = _domains(kind, N, D)
    exp = SR.place(cont, nodes, strategy, domain=dom, max_skew=max_skew)
    # the inputs discriminate (asserted on the reference): the constraint changes the plan, the small
    # shapes with many or lopsided domains reject on skew, the large ones place nearly everything
    base = _unconstrained(C, N, flags, strategy)
    n_skew = int((exp[1] == SR.REASON_SKEW).sum())
    if N > 1:
        assert (exp[0] != base[0]).sum() >= 150
    if (N, kind) == (64, "lop") or N == 65:
        assert n_skew >= 120
    if N > 65 or N == 1:
        assert n_skew <= 2
    _check(_run1(planner, cont, nodes, strategy, dom, max_skew, node_count=np.zeros(N, np.uint32), sid=7), exp, 7)


@pytest.mark.parametrize("max_skew", [1, 2])
@pytest.mark.parametrize("N", [64, 2048, 8192])
def test_crafted_skew_not_nofit(N, max_skew, planner):
    """Four domains, domain 0 a single schedulable node without room: it is eligible and stays at zero, so
    each of the other three takes max_skew containers and every later one is SKEW -- none NOFIT, though
    thousands of nodes fit.  With that node cordoned domain 0 is not eligible and everything is placed."""
    C = 300
    cf = np.full(N, 1000, np.uint32)
    cf[0] = 0
    sched = np.ones(N, np.uint8)
    dom = (1 + np.arange(N) % 3).astype(np.uint32)
    dom[0] = 0
    nodes = (cf, np.full(N, 1000, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32), sched)
    cont = (np.full(C, 10, np.uint32), np.ones(C, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32))
    for strategy in R.STRATEGIES:
        got = _run1(planner, cont, nodes, strategy, dom, max_skew, node_count=np.zeros(N, np.uint32))
        assert (got[1] == 0).sum() == 3 * max_skew and (got[1] == SR.REASON_SKEW).sum() == C - 3 * max_skew
        assert (got[0][:3 * max_skew] != NONE).all() and (got[0][3 * max_skew:] == NONE).all()
        assert np.array_equal(np.bincount(dom[got[0][:3 * max_skew]], minlength=4), [0] + [max_skew] * 3)
        _check(got, SR.place(cont, nodes, strategy, domain=dom, max_skew=max_skew), 0)
    off = sched.copy()
    off[0] = 0
    nodes = (*nodes[:4], off)
    got = _run1(planner, cont, nodes, R.SPREAD, dom, max_skew, node_count=np.zeros(N, np.uint32))
    assert (got[1] == 0).all() and (got[0] != 0).all()
    _check(got, SR.place(cont, nodes, R.SPREAD, domain=dom, max_skew=max_skew), 0)


def test_ties_alternate_between_the_halves(planner):
    """2048 identical nodes (1024 threads x 2), domain = n // 1024, max_skew = 1, first fit: the lowest
    free index of each half in turn, three containers to a node."""
    N, C = 2048, 300
    nodes = (np.full(N, 100, np.uint32), np.full(N, 1000, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32),
             np.ones(N, np.uint8))
    cont = (np.full(C, 30, np.uint32), np.full(C, 1, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32))
    dom = (np.arange(N) // 1024).astype(np.uint32)
    i = np.arange(C, dtype=np.uint32)
    a, r, after, cnt = planner.place_policy(cont, nodes, R.FIRST_FIT, domain=dom, max_skew=1)
    assert np.array_equal(a, (i % 2) * 1024 + (i // 2) // 3) and (r == 0).all()
    for st in R.STRATEGIES:
        _check(_run1(planner, cont, nodes, st, dom, 1, node_count=np.zeros(N, np.uint32)),
               SR.place(cont, nodes, st, domain=dom, max_skew=1), 0)


@pytest.mark.parametrize("S", [1, 3, 300])
def test_batch_host_and_device(S, planner):
    """Scenarios with their own max_skew (0 included), strategy and preferred mask, node counts on entry
    (one of them 0xFFFFFFFF), CYCLE levels, a non-zero scen_base: the host and the device entry agree
    with each other and with the reference."""
    import torch
    from fleetflow_amd import DevBatch
    C, N, D, base = 50, 70, 24, 1000  # about three nodes a domain: the constraint rejects
    rng = np.random.default_rng(100 + S)
    scen = [_scenario(C, N, 7, scen=base + s) for s in range(S)]
    strat = [int(x) for x in rng.integers(0, 4, S)]
    pref = [int(x) for x in rng.choice([0, PREF2, 1 << 11, 0xFFFFFFFF], S)]
    skew = [int(x) for x in rng.choice([0, 1, 2, 3, 0xFFFFFFFF], S)]
    skew[0] = 1
    if S > 1:
        skew[1] = 0
    cnt0 = rng.integers(0, 4, S * N).astype(np.uint32)
    cnt0[5] = 0xFFFFFFFF
    dom = rng.integers(0, D, S * N).astype(np.uint32)
    level = np.where(rng.random(S * C) < 0.05, NONE, 0).astype(np.uint32)
    cat = lambda k, i: np.concatenate([sc[k][i] for sc in scen])  # noqa: E731
    cont, nodes = [cat(0, i) for i in range(4)], [cat(1, i) for i in range(5)]
    exp = [SR.place(scen[s][0], scen[s][1], strat[s], preferred=pref[s], level=level[s * C:(s + 1) * C],
                    node_count=cnt0[s * N:(s + 1) * N], domain=dom[s * N:(s + 1) * N], max_skew=skew[s]) for s in range(S)]
    a, r, cost, after, cnt = planner.place_batch_policy(S, C, N, cont, nodes, strat, pref, level=level, node_count=cnt0,
                                                        scen_base=base, domain=dom, max_skew=skew)
    for s in range(S):
        c, n = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N)
        _check((a[c], r[c], cost[s], tuple(x[n] for x in after), cnt[n]), exp[s], base + s)
    assert (exp[0][1] == SR.REASON_SKEW).sum() >= 5  # on the reference: scenario 0 (max_skew 1) rejects on skew
    # the device entry on the same batch
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(S, C, N, dev, scen_base=base, with_level=True)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.level, db.cf, db.mf, db.lab, db.cu),
                        (*cont, level, *nodes[:4])):
        dst.copy_(t32(src))
    db.sched.copy_(torch.from_numpy(nodes[4]).to(dev))
    st_t, pf_t, cnt_t, dom_t, sk_t = t32(strat), t32(pref), t32(cnt0), t32(dom), t32(skew)
    planner.dev_place_batch_policy(db, st_t, pf_t, cnt_t, domain_t=dom_t, max_skew_t=sk_t)
    planner.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert np.array_equal(u32(db.assign), a) and np.array_equal(db.reason.cpu().numpy(), r)
    assert np.array_equal(db.cost.cpu().numpy().view(np.uint64), cost)
    for t, h in zip((db.cf, db.mf, db.cu, cnt_t), (after[0], after[1], after[3], cnt)):
        assert np.array_equal(u32(t), h)


def test_errors_write_nothing(planner):
    import torch
    from fleetflow_amd import DevBatch
    from fleetflow_amd._lib import FP_EINVAL, FleetplaceError
    C, N = 300, 65
    cont, nodes = _scenario(C, N, 7)
    dom = (np.arange(N) % 5).astype(np.uint32)
    bad = dom.copy()
    bad[N - 1] = 64
    # host entries: refused before anything is staged
    with pytest.raises(FleetplaceError) as e:
        planner.place_policy(cont, nodes, R.SPREAD, domain=bad, max_skew=1)
    assert e.value.code == FP_EINVAL
    tile = lambda x: [np.tile(a, 2) for a in x]  # noqa: E731
    with pytest.raises(FleetplaceError) as e:
        planner.place_batch_policy(2, C, N, tile(cont), tile(nodes), [1, 1], domain=np.concatenate([dom, bad]), max_skew=[1, 2])
    assert e.value.code == FP_EINVAL
    # ignored where that scenario's max_skew is 0: scenario 1 is SPEC.md 2.6, scenario 0 constrained
    a, r, cost, after, cnt = planner.place_batch_policy(2, C, N, tile(cont), tile(nodes), [1, 1],
                                                        domain=np.concatenate([dom, bad]), max_skew=[1, 0])
    assert np.array_equal(a[:C], SR.place(cont, nodes, R.SPREAD, domain=dom, max_skew=1)[0])
    assert np.array_equal(a[C:], R.place(cont, nodes, R.SPREAD)[0])
    a1 = planner.place_policy(cont, nodes, R.PACK, domain=np.full(N, 0xFFFFFFFF, np.uint32), max_skew=0)
    assert np.array_equal(a1[0], R.place(cont, nodes, R.PACK)[0])
    # the device entry: found by the kernels, reported by sync(), nothing written
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(2, C, N, dev)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu), (*cont, *nodes[:4])):
        dst.copy_(t32(np.tile(src, 2)))
    db.sched.copy_(torch.from_numpy(np.tile(nodes[4], 2)).to(dev))
    db.assign.fill_(-7)
    db.reason.fill_(9)
    db.cost.fill_(-1)
    snap = db.node_snapshot()
    cnt_t = torch.full((2 * N,), 5, dtype=torch.int32, device=dev)
    st_t = torch.tensor([1, 3], dtype=torch.int32, device=dev)
    planner.dev_place_batch_policy(db, st_t, None, cnt_t, domain_t=t32(np.concatenate([dom, bad])), max_skew_t=t32([1, 2]))
    with pytest.raises(FleetplaceError) as e:
        planner.sync()
    assert e.value.code == FP_EINVAL
    assert bool((db.assign == -7).all()) and bool((db.reason == 9).all()) and bool((db.cost == -1).all())
    assert all(torch.equal(x, y) for x, y in zip(snap, (db.cf, db.mf, db.cu))) and bool((cnt_t == 5).all())
    planner.sync()  # reported once
    # the context still plans, and the same domains pass where that scenario is unconstrained
    planner.dev_place_batch_policy(db, st_t, None, None, domain_t=t32(np.concatenate([dom, bad])), max_skew_t=t32([1, 0]))
    planner.sync()
    got = db.assign.cpu().numpy().view(np.uint32)
    e0, e1 = SR.place(cont, nodes, R.SPREAD, domain=dom, max_skew=1), R.place(cont, nodes, R.FILL_LOWEST)
    assert np.array_equal(got[:C], e0[0]) and np.array_equal(got[C:], e1[0])
    assert int(db.cost[0].item()) == SR.cost(e0[0], e0[1], 0) and int(db.cost[1].item()) == R.cost(e1[0], e1[1], 1)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_null_pointers_are_the_unconstrained_placer(strategy, planner):
    """domain = None is exactly place_policy; so is a batch given only one of the two arrays."""
    C, N = 300, 200
    cont, nodes = _scenario(C, N, 7)
    cnt0 = np.random.default_rng(9).integers(0, 6, N).astype(np.uint32)
    exp = R.place(cont, nodes, strategy, preferred=PREF2, node_count=cnt0)
    a, r, after, cnt = planner.place_policy(cont, nodes, strategy, preferred=PREF2, node_count=cnt0, domain=None, max_skew=1)
    _check((a, r, None, after, cnt), exp)
    dom = (np.arange(N) % 3).astype(np.uint32)
    for kw in (dict(domain=dom), dict(max_skew=[1]), {}):
        a, r, cost, after, cnt = planner.place_batch_policy(1, C, N, cont, nodes, [strategy], [PREF2], node_count=cnt0, **kw)
        _check((a, r, cost[0], after, cnt), exp, 0)
    # and the constraint is live on the same call once both are given
    a, r, cost, after, cnt = planner.place_batch_policy(1, C, N, cont, nodes, [strategy], [PREF2], node_count=cnt0,
                                                        domain=dom, max_skew=[1])
    exp1 = SR.place(cont, nodes, strategy, preferred=PREF2, node_count=cnt0, domain=dom, max_skew=1)
    _check((a, r, cost[0], after, cnt), exp1, 0)
    assert (exp1[0] != exp[0]).sum() > 50


STAGE_KDL = """
project "demo"
server "t0" { capacity cpu=4000 memory=8192; label "region=tokyo" }
server "bare" { capacity cpu=64000 memory=65536 }
server "o0" { capacity cpu=1000 memory=8192; label "region=osaka" }
server "t1" { capacity cpu=4000 memory=8192; label "region=tokyo" }
%(services)s
stage "live" {
%(members)s
    server "t0"
    server "bare"
    server "o0"
    server "t1"
    %(placement)s
}
"""


def test_plan_stage_from_kdl_with_a_spread_node(planner):
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run
    cpus = [2000, 2000, 2000, 900, 50, 50]
    text = lambda placement: STAGE_KDL % {  # noqa: E731
        "services": "\n".join(f'service "s{i}" {{ resources cpu={c} memory=64 }}' for i, c in enumerate(cpus)),
        "members": "\n".join(f'    service "s{i}"' for i in range(len(cpus))), "placement": placement}
    flow = parse_kdl_string(text('placement { spread "region" max-skew=1 }'))
    plain = parse_kdl_string(text(""))
    plan, base = plan_stage(flow, "live", planner), plan_stage(plain, "live", planner)
    # two regions; the server without the key receives nothing; s1 and s2 only fit tokyo, which is one ahead
    ea, er, _, _ = SR.place((cpus, [64] * 6, [0] * 6, [0] * 6),
                            ([4000, 64000, 1000, 4000], [8192, 65536, 8192, 8192], [0] * 4, [0] * 4, [1, 0, 1, 1]), R.FIRST_FIT,
                            domain=[0, 0, 1, 0], max_skew=1)
    slugs = ["t0", "bare", "o0", "t1"]
    assert plan.assignment == {f"s{i}": slugs[n] for i, n in enumerate(ea) if n != NONE}
    assert plan.assignment == {"s0": "t0", "s3": "o0", "s4": "t0", "s5": "o0"}
    assert plan.rejected == {"s1": "SKEW", "s2": "SKEW"} and "bare" not in plan.assignment.values()
    assert (plan.spread_topology_key, plan.spread_max_skew) == ("region", 1)
    out = format_up_dry_run(flow, "live", plan)
    assert "    配置先: (配置不可: SKEW)" in out and "  配置分散保証: region (max_skew=1)" in out
    # levels, orders and candidates are the plain stage's, whose first fit fills the first server
    assert (plan.order, plan.levels, plan.level_order, plan.candidates) == (base.order, base.levels, base.level_order, base.candidates)
    assert base.rejected == {} and base.spread_topology_key is None and "配置分散保証" not in format_up_dry_run(plain, "live", base)
