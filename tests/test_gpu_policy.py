"""GPU tests of the scored placement (SPEC.md 2.6; fleetflow_amd/csrc/fp_policy.hip): every entry point
against the numpy reference (tests/policy_ref.py), and strategy 0 against the C oracle.  Every
comparison is exact: assign, reason, the three mutated node arrays, node_count and the packed cost."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402

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


def _check(got, exp, sid=None):
    """got: (assign, reason, cost or None, nodes_after, count or None); exp: policy_ref.place's tuple."""
    assign, reason, cost, after, cnt = got
    assert np.array_equal(assign, exp[0])
    assert np.array_equal(reason, exp[1])
    for i in (0, 1, 3):
        assert np.array_equal(after[i], exp[2][i]), i
    if cnt is not None:
        assert np.array_equal(cnt, exp[3])
    if cost is not None:
        assert int(cost) == R.cost(exp[0], exp[1], sid)


def _run1(planner, cont, nodes, strategy, preferred=0, level=None, node_count=None, sid=0):
    """One scenario through the batch entry (it returns the cost too)."""
    C, N = cont[0].size, nodes[0].size
    a, r, cost, after, cnt = planner.place_batch_policy(1, C, N, cont, nodes, [strategy], [preferred], level=level,
                                                        node_count=node_count, scen_base=sid)
    return a, r, cost[0], after, cnt


# every instantiation (64 x 1, 1024 x {1, 2, 4, 8}) at its lowest and highest N, odd sizes between
SHAPES = [(300, 1, 7), (1, 63, 7), (300, 64, 7), (300, 65, 0), (2000, 1024, 7), (1, 1025, 7), (300, 2048, 7),
          (300, 2049, 0), (2000, 4096, 7), (300, 4097, 7), (2000, 8192, 7), (1, 8192, 0)]


@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("C,N,flags", SHAPES)
def test_every_strategy_vs_reference(C, N, flags, strategy, planner):
    cont, nodes = _scenario(C, N, flags)
    cnt0 = np.zeros(N, np.uint32)
    exp = R.place(cont, nodes, strategy)
    _check(_run1(planner, cont, nodes, strategy, node_count=cnt0, sid=7), exp, 7)


@pytest.mark.parametrize("C,N", [(600, 70), (2000, 1025)])
def test_first_fit_vs_oracle(C, N, planner, O):
    """Strategy 0 without a preferred mask is SPEC.md 2.3: what ties the kernel to the C oracle."""
    cont, nodes = _scenario(C, N, 7)
    assign, reason, after, cnt = planner.place_policy(cont, nodes, R.FIRST_FIT)
    ea, er, eafter, _ = O.place(cont, nodes)
    assert cnt is None
    assert np.array_equal(assign, ea) and np.array_equal(reason, er)
    for i in (0, 1, 3):
        assert np.array_equal(after[i], eafter[i])
    # and the same container set under the other rules does not (the inputs discriminate)
    assert (planner.place_policy(cont, nodes, "spread_across_pool")[0] != ea).sum() > 100


def test_tie_breaking_across_lanes_waves_and_k(planner):
    """2048 identical nodes (1024 threads x 2), 300 identical containers, three to a node."""
    N, C = 2048, 300
    nodes = (np.full(N, 100, np.uint32), np.full(N, 1000, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32),
             np.ones(N, np.uint8))
    cont = (np.full(C, 30, np.uint32), np.full(C, 1, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32))
    i = np.arange(C, dtype=np.uint32)
    assert np.array_equal(planner.place_policy(cont, nodes, R.SPREAD)[0], i)
    assert np.array_equal(planner.place_policy(cont, nodes, R.PACK)[0], i // 3)
    assert np.array_equal(planner.place_policy(cont, nodes, R.FIRST_FIT)[0], i // 3)
    for st in R.STRATEGIES:
        _check(_run1(planner, cont, nodes, st, node_count=np.zeros(N, np.uint32)), R.place(cont, nodes, st), 0)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_scalar_extremes_and_gating(strategy, planner):
    """Preferred masks of 0, two bits and all 32 bits; unconstrained nodes; node counts on entry and
    none at all; CYCLE containers; cordoned nodes are never chosen and come back unchanged."""
    cont, nodes = _scenario(300, 200, 7)
    rng = np.random.default_rng(5)
    cf, mf, lab, cu, sched = (np.array(a) for a in nodes)
    cf[:20] = mf[:20] = 0xFFFFFFFF
    sched[rng.random(200) < 0.2] = 0
    sched[3] = 0
    nodes = (cf, mf, lab, cu, sched)
    level = np.where(rng.random(300) < 0.1, NONE, 1).astype(np.uint32)
    cnt0 = rng.integers(0, 6, 200).astype(np.uint32)
    cnt0[7] = 0xFFFFFFFF
    for pref in (0, PREF2, 0xFFFFFFFF):
        exp = R.place(cont, nodes, strategy, preferred=pref, level=level, node_count=cnt0)
        got = _run1(planner, cont, nodes, strategy, pref, level=level, node_count=cnt0, sid=65535)
        _check(got, exp, 65535)
        assert (got[1] == 2).sum() == (level == NONE).sum() and (got[0][level == NONE] == NONE).all()
        off = sched == 0
        assert not np.isin(got[0], np.flatnonzero(off)).any()
        assert np.array_equal(got[3][0][off], cf[off]) and np.array_equal(got[4][off], cnt0[off])
        # no node_count: counts start at zero and nothing comes back
        a, r, after, cnt = planner.place_policy(cont, nodes, strategy, preferred=pref, level=level)
        assert cnt is None
        _check((a, r, None, after, None), R.place(cont, nodes, strategy, preferred=pref, level=level))


@pytest.mark.parametrize("S", [1, 3, 300])
def test_batch_host_and_device(S, planner):
    """Scenarios with their own strategy and preferred mask, a non-zero scen_base, S above the CU
    count: the host and the device entry agree with each other and with the reference, and the
    argmin over the costs is the reference's best scenario."""
    import torch
    from fleetflow_amd import DevBatch
    C, N, base = 50, 70, 1000
    rng = np.random.default_rng(S)
    scen = [_scenario(C, N, 7, scen=base + s) for s in range(S)]
    strat = [int(x) for x in rng.integers(0, 4, S)]
    pref = [int(x) for x in rng.choice([0, PREF2, 1 << 11, 0xFFFFFFFF], S)]
    cnt0 = rng.integers(0, 4, S * N).astype(np.uint32)
    level = np.where(rng.random(S * C) < 0.05, NONE, 0).astype(np.uint32)
    cat = lambda k, i: np.concatenate([sc[k][i] for sc in scen])  # noqa: E731
    cont, nodes = [cat(0, i) for i in range(4)], [cat(1, i) for i in range(5)]
    exp = [R.place(scen[s][0], scen[s][1], strat[s], preferred=pref[s], level=level[s * C:(s + 1) * C],
                   node_count=cnt0[s * N:(s + 1) * N]) for s in range(S)]
    ecost = [R.cost(e[0], e[1], base + s) for s, e in enumerate(exp)]
    a, r, cost, after, cnt = planner.place_batch_policy(S, C, N, cont, nodes, strat, pref, level=level, node_count=cnt0,
                                                        scen_base=base)
    for s in range(S):
        c, n = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N)
        _check((a[c], r[c], cost[s], tuple(x[n] for x in after), cnt[n]), exp[s], base + s)
    # the device entry on the same batch
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(S, C, N, dev, scen_base=base, with_level=True)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.level, db.cf, db.mf, db.lab, db.cu),
                        (*cont, level, *nodes[:4])):
        dst.copy_(t32(src))
    db.sched.copy_(torch.from_numpy(nodes[4]).to(dev))
    st_t, pf_t, cnt_t = t32(strat), t32(pref), t32(cnt0)
    planner.dev_place_batch_policy(db, st_t, pf_t, cnt_t)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    planner.dev_argmin_cost(db.cost, best)
    planner.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert np.array_equal(u32(db.assign), a) and np.array_equal(db.reason.cpu().numpy(), r)
    assert np.array_equal(db.cost.cpu().numpy().view(np.uint64), cost)
    for t, h in zip((db.cf, db.mf, db.cu, cnt_t), (after[0], after[1], after[3], cnt)):
        assert np.array_equal(u32(t), h)
    assert int(best.item()) == int(np.argmin(ecost))


def test_errors_write_nothing(planner, O):
    import torch
    from fleetflow_amd import DevBatch
    from fleetflow_amd._lib import FP_EINVAL, FP_EOVERFLOW, FleetplaceError
    cont, nodes = _scenario(300, 65, 7)
    # N = 8193: refused by the host entry and by the device entry, before anything runs
    big = tuple(np.resize(a, 8193) for a in nodes)
    with pytest.raises(FleetplaceError) as e:
        planner.place_policy(cont, big, R.SPREAD)
    assert e.value.code == FP_EOVERFLOW
    with pytest.raises(FleetplaceError) as e:
        planner.place_policy(cont, nodes, 4)
    assert e.value.code == FP_EINVAL
    with pytest.raises(FleetplaceError) as e:
        planner.place_batch_policy(2, 1, 1, [np.ones(2, np.uint32)] * 4, [np.ones(2, np.uint32)] * 4 + [np.ones(2, np.uint8)],
                                   [1, 1], scen_base=65535)
    assert e.value.code == FP_EOVERFLOW
    dev = "cuda:0"
    db = DevBatch.allocate(2, 300, 8193, dev)
    db.assign.fill_(-7)
    st = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    with pytest.raises(FleetplaceError) as e:
        planner.dev_place_batch_policy(db, st)
    assert e.value.code == FP_EOVERFLOW
    planner.sync()
    assert bool((db.assign == -7).all())
    # strategy 4 on the device: found by the kernels, reported by sync(), nothing written
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(2, 300, 65, dev)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu),
                        (*cont, *nodes[:4])):
        dst.copy_(t32(np.tile(src, 2)))
    db.sched.copy_(torch.from_numpy(np.tile(nodes[4], 2)).to(dev))
    db.assign.fill_(-7)
    db.reason.fill_(9)
    db.cost.fill_(-1)
    snap = db.node_snapshot()
    cnt_t = torch.full((2 * 65,), 5, dtype=torch.int32, device=dev)
    planner.dev_place_batch_policy(db, torch.tensor([1, 4], dtype=torch.int32, device=dev), None, cnt_t)
    with pytest.raises(FleetplaceError) as e:
        planner.sync()
    assert e.value.code == FP_EINVAL
    assert bool((db.assign == -7).all()) and bool((db.reason == 9).all()) and bool((db.cost == -1).all())
    assert all(torch.equal(x, y) for x, y in zip(snap, (db.cf, db.mf, db.cu))) and bool((cnt_t == 5).all())
    planner.sync()  # reported once
    # the context still plans: the same batch with valid strategies
    planner.dev_place_batch_policy(db, torch.tensor([1, 3], dtype=torch.int32, device=dev), None, None)
    planner.sync()
    for s, stg in enumerate((R.SPREAD, R.FILL_LOWEST)):
        exp = R.place(cont, nodes, stg)
        assert np.array_equal(db.assign[s * 300:(s + 1) * 300].cpu().numpy().view(np.uint32), exp[0])
        assert int(db.cost[s].item()) == R.cost(exp[0], exp[1], s)


def test_no_containers_and_no_scenarios(planner):
    N = 5
    nodes = [np.full(3 * N, 100, np.uint32), np.full(3 * N, 100, np.uint32), np.zeros(3 * N, np.uint32),
             np.zeros(3 * N, np.uint32), np.ones(3 * N, np.uint8)]
    empty = np.zeros(0, np.uint32)
    a, r, cost, after, cnt = planner.place_batch_policy(3, 0, N, [empty] * 4, nodes, [1, 2, 3], scen_base=9,
                                                        node_count=np.full(3 * N, 2, np.uint32))
    assert a.size == 0 and r.size == 0 and [int(c) for c in cost] == [9, 10, 11]
    assert np.array_equal(after[0], nodes[0]) and (cnt == 2).all()
    a, r, cost, after, cnt = planner.place_batch_policy(0, 4, N, [empty] * 4, [empty] * 4 + [np.zeros(0, np.uint8)], [])
    assert a.size == 0 and cost.size == 0 and cnt is None
    a, r, after, cnt = planner.place_policy([empty] * 4, [x[:N] for x in nodes], "fill_lowest")
    assert a.size == 0 and np.array_equal(after[0], nodes[0][:N])
    # no nodes: every container NOFIT
    a, r, _, _ = planner.place_policy(([5, 6], [1, 1], [0, 0], [0, 0]), ([], [], [], [], []), R.PACK)
    assert a.tolist() == [NONE, NONE] and r.tolist() == [1, 1]


def test_place_path_after_a_policy_call(planner, O):
    """A policy call resets the workspace the last first-fit call's range words live in:
    place_path() must report that nothing ran, not read recycled memory; a following ordinary
    place on the same context is still the oracle's."""
    cont, nodes = _scenario(600, 70, 7)
    planner.place(cont, nodes)
    assert planner.place_path()["ran"]
    planner.place_policy(cont, nodes, R.PACK)
    assert not planner.place_path()["ran"]
    assign, reason, after = planner.place(cont, nodes)
    ea, er, eafter, _ = O.place(cont, nodes)
    assert np.array_equal(assign, ea) and np.array_equal(reason, er) and np.array_equal(after[0], eafter[0])
    assert planner.place_path()["ran"]


def test_place_path_after_the_workspace_is_reused(planner, O):
    """The last placement's range words live in the workspace arena, and the arena's reset forgets them:
    after a levelize or a plan_stage that reuses the arena, place_path() reports that nothing ran instead of
    reading recycled memory, and the next placement is unchanged.  FP_OPT_LEVEL_SMALL = 0 keeps both on the
    general path: the one-launch kernels of a 20-vertex graph take no workspace."""
    S, C, N = 1, 130, 65
    cont, nodes = _scenario(C, N, 7)
    rp, col, hd = O.gen_dag(SEED, 20, 10, 5, 40, 3)
    first = planner.place_batch(S, C, N, cont, nodes)
    assert planner.place_path()["ran"]
    planner.set_option("level_small", 0)
    try:
        for reuse, level_at in ((planner.levelize, 0), (planner.plan_stage, 1)):
            assert np.array_equal(reuse(rp, col, hd)[level_at], O.levelize(rp, col, hd)[0])
            assert not planner.place_path()["ran"]
            again = planner.place_batch(S, C, N, cont, nodes)
            assert planner.place_path()["ran"]
            for x, y in zip(first[:3] + first[3], again[:3] + again[3]):
                assert np.array_equal(x, y)
    finally:
        planner.set_option("level_small")


STAGE_KDL = """
project "demo"
%(servers)s
%(services)s
stage "live" {
%(members)s
    %(placement)s
}
"""


def _stage_text(placement):
    servers = "\n".join(
        f'server "n{i}" {{ capacity cpu={2000 + 1000 * (i % 3)} memory={4096 + 2048 * (i % 2)}; '
        f'label "region={"tokyo" if i % 3 == 0 else "osaka"}"; label "class={"gpu" if i % 4 == 1 else "cpu"}"'
        + ('; scheduling "cordon"' if i == 2 else "") + " }" for i in range(8))
    services = "\n".join(
        f'service "s{i}" {{ resources cpu={300 + 100 * (i % 4)} memory={512 * (1 + i % 3)}'
        + ('; require "class=gpu"' if i % 7 == 0 else "") + (f'; depends_on "s{i - 1}"' if i % 5 == 1 else "") + " }"
        for i in range(24))
    members = "\n".join(f'    service "s{i}"' for i in range(24)) + "\n" + "\n".join(f'    server "n{i}"' for i in range(8))
    return STAGE_KDL % {"servers": servers, "services": services, "members": members, "placement": placement}


@pytest.mark.parametrize("strategy", ["spread_across_pool", "pack_into_dedicated", "fill_lowest"])
def test_plan_stage_from_kdl_with_a_placement_node(strategy, planner):
    from fleetflow_amd.flow import LabelDict, PlacementPolicy, plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run
    flow = parse_kdl_string(_stage_text(f'placement strategy="{strategy}" {{ prefer "region=tokyo" }}'))
    plain = parse_kdl_string(_stage_text(""))
    plan, base = plan_stage(flow, "live", planner), plan_stage(plain, "live", planner)
    stage = flow.stages["live"]
    svcs, nodes = [flow.services[n] for n in stage.services], [flow.servers[n] for n in stage.servers]
    ld = LabelDict([x for s in svcs for x in s.labels] + [x for n in nodes for x in n.labels] + ["region=tokyo"])
    cont = ([s.cpu_m for s in svcs], [s.mem_mib for s in svcs], [ld.mask(s.labels) for s in svcs], [0] * len(svcs))
    nd = ([n.cpu_m for n in nodes], [n.mem_mib for n in nodes], [ld.mask(n.labels) for n in nodes], [0] * len(nodes),
          [int(n.schedulable) for n in nodes])
    level = [plan.levels[s] for s in stage.services]
    ea, er, _, _ = R.place(cont, nd, R.STRATEGIES[1 + ["spread_across_pool", "pack_into_dedicated", "fill_lowest"].index(strategy)],
                           preferred=ld.mask(["region=tokyo"]), level=level)
    for i, s in enumerate(stage.services):
        if ea[i] != NONE:
            assert plan.assignment[s] == nodes[ea[i]].slug
        else:
            assert plan.rejected[s] == "NOFIT"
    assert plan.strategy == strategy and plan.preferred == ["region=tokyo"]
    assert f"配置戦略: {strategy}" in format_up_dry_run(flow, "live", plan)
    # levels, orders and candidates are the plain stage's; without the node the plan is today's
    assert (plan.order, plan.levels, plan.level_order, plan.candidates) == (base.order, base.levels, base.level_order, base.candidates)
    fa, fr, _, _ = R.place(cont, nd, R.FIRST_FIT, level=level)
    assert base.assignment == {s: nodes[fa[i]].slug for i, s in enumerate(stage.services) if fa[i] != NONE}
    assert base.strategy is None and "配置戦略" not in format_up_dry_run(plain, "live", base)
    # a policy passed in wins over the parsed node, and one that sets nothing is today's path
    assert plan_stage(plain, "live", planner, policy=PlacementPolicy(strategy, {"region": "tokyo"})) == plan
    assert plan_stage(plain, "live", planner, policy=PlacementPolicy()) == base
