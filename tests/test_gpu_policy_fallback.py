"""GPU tests of the fallback chain (SPEC.md 2.8; k_policy<.., .., true> in fleetflow_amd/csrc/fp_policy.hip):
every entry point against the numpy reference (tests/policy_fallback_ref.py).  Every comparison is exact:
assign, reason, hops, the three mutated node arrays, node_count and the packed cost."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_cases as K  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_ref as R  # noqa: E402
import policy_spread_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _check(got, exp, sid=None):
    """got: (assign, reason, hops, cost or None, nodes_after, count or None); exp: the reference's
    (assign, reason, hops, nodes_after, count)."""
    assign, reason, hops, cost, after, cnt = got
    assert np.array_equal(assign, exp[0])
    assert np.array_equal(reason, exp[1])
    assert np.array_equal(hops, exp[2])
    for i in (0, 1, 3):
        assert np.array_equal(after[i], exp[3][i]), i
    if cnt is not None:
        assert np.array_equal(cnt, exp[4])
    if cost is not None:
        assert int(cost) == FR.cost(exp[0], exp[1], sid)


def _run1(planner, cont, nodes, strategy, relax, n_hops=None, domain=None, max_skew=None, preferred=0, level=None,
          node_count=None, sid=0):
    """One scenario through the batch entry (it returns the cost too)."""
    C, N = cont[0].size, nodes[0].size
    a, r, h, cost, after, cnt = planner.place_batch_policy_fallback(
        1, C, N, cont, nodes, [strategy], [preferred], level=level, node_count=node_count, scen_base=sid, domain=domain,
        max_skew=None if max_skew is None else [max_skew], relax_mask=K.relax_rows([relax]),
        n_hops=[len(relax) if n_hops is None else n_hops])
    return a, r, h, cost[0], after, cnt


# every instantiation (64 x 1, 1024 x {1, 2, 4, 8}) at an edge
SHAPES = [(300, 1), (300, 64), (300, 65), (2000, 1024), (300, 2049), (2000, 4096), (2000, 8192)]


@pytest.mark.parametrize("n_hops", [1, 2, 4])
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("C,N", SHAPES)
def test_every_strategy_vs_reference(C, N, strategy, n_hops, planner):
    cont, nodes = K.crafted(C, N)
    exp = K.expected(C, N, strategy, n_hops)
    # the inputs discriminate (asserted on the reference): pools run dry, so containers relax
    if N > 1:
        placed = exp[0] != NONE
        at = np.bincount(exp[2][placed], minlength=5)
        if n_hops == 2:
            assert at[1] >= 20 and at[2] >= 15
            assert (exp[0] != K.expected(C, N, strategy, 0)[0]).sum() >= 80
        if n_hops == 4:
            assert at[3] + at[4] >= 3
    _check(_run1(planner, cont, nodes, strategy, K.RELAX[n_hops], node_count=np.zeros(N, np.uint32), sid=7), exp, 7)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("C,N", [(300, 64), (300, 65), (2000, 1024), (2000, 8192)])
def test_every_strategy_with_a_spread(C, N, strategy, planner):
    """SKEW and relaxed placements in one call: domain = n % 5, max_skew = 2, relax = [class, region]."""
    cont, nodes = K.crafted(C, N)
    exp = K.expected(C, N, strategy, 2, True)
    assert (exp[1] == SR.REASON_SKEW).sum() >= 140 and (exp[2] >= 1).sum() >= 25
    _check(_run1(planner, cont, nodes, strategy, K.RELAX[2], domain=K.spread_domain(N), max_skew=2,
                 node_count=np.zeros(N, np.uint32), sid=7), exp, 7)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("C,N", [(300, 64), (2000, 1024)])
def test_no_hops_is_the_spread_entry(C, N, strategy, planner):
    """n_hops = 0 through the FB kernels, with a relax_mask that is not read: exactly SPEC.md 2.7."""
    cont, nodes = K.crafted(C, N)
    dom = K.spread_domain(N)
    a, r, after, cnt = SR.place(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), domain=dom, max_skew=2)
    assert (r == SR.REASON_SKEW).sum() >= 100
    got = _run1(planner, cont, nodes, strategy, [0xFFFFFFFF] * 4, n_hops=0, domain=dom, max_skew=2,
                node_count=np.zeros(N, np.uint32), sid=7)
    _check(got, (a, r, np.zeros(C, np.uint8), after, cnt), 7)


@pytest.mark.parametrize("N", [64, 2048, 8192])
def test_crafted_closed_form(N, planner):
    """Every node holds one container; labels by n % 4 are A|Y, B|Y, A|X, B|X; every container requires
    A|Y; first fit."""
    cont, nodes = K.closed_form(N)
    q, i = N // 4, np.arange(N)
    k = 4 * np.arange(q)
    run = lambda relax, **kw: planner.place_policy_fallback(cont, nodes, R.FIRST_FIT, relax, **kw)  # noqa: E731
    # class, then region: the matching nodes, then the other class, then the other region in index order
    a, r, h, _, _ = run([K.CLASS, K.REGION])
    assert np.array_equal(a, np.concatenate([k, k + 1, np.sort(np.concatenate([k + 2, k + 3]))]))
    assert (r == 0).all() and np.array_equal(h, np.repeat([0, 1, 2], [q, q, 2 * q]))
    a, r, h, _, _ = run([K.CLASS])
    assert np.array_equal(a[:2 * q], np.concatenate([k, k + 1])) and np.array_equal(h[:2 * q], np.repeat([0, 1], q))
    assert (a[2 * q:] == NONE).all() and (r[2 * q:] == 1).all() and (h[2 * q:] == 0).all()
    a, r, h, _, _ = run([K.REGION])
    assert np.array_equal(a[:2 * q], np.concatenate([k, k + 2])) and np.array_equal(h[:2 * q], np.repeat([0, 1], q))
    assert (a[2 * q:] == NONE).all() and (r[2 * q:] == 1).all() and (h[2 * q:] == 0).all()
    # one domain per label pair, max_skew 1: the skew test forces the relaxation
    dom = (i % 4).astype(np.uint32)
    a, r, h, _, _ = run([K.CLASS, K.REGION], domain=dom, max_skew=1)
    assert np.array_equal(a, i) and np.array_equal(h, np.array([0, 1, 2, 2])[i % 4]) and (r == 0).all()
    a, r, h, _, _ = run([K.CLASS], domain=dom, max_skew=1)
    assert (a != NONE).sum() == 2 and (r == SR.REASON_SKEW).sum() == N - 2 and (r == 1).sum() == 0
    if N <= 2048:  # and the reference says the same
        for relax, kw in (([K.CLASS, K.REGION], {}), ([K.CLASS], dict(domain=dom, max_skew=1))):
            e = FR.place(cont, nodes, R.FIRST_FIT, relax_mask=relax, **kw)
            g = run(relax, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(g[:3], e[:3]))


def _batch_case(S, seed=0):
    """S scenarios at (300, 65): per-scenario n_hops in {0, 1, 2, 4}, strategy, preferred mask and max_skew
    (0 included), node counts on entry, CYCLE levels."""
    C, N, base = 300, 65, 1000
    rng = np.random.default_rng(200 + S + seed)
    scen = [K.crafted(C, N, scen=s % 3) for s in range(S)]
    strat = [int(x) for x in rng.integers(0, 4, S)]
    pref = [int(x) for x in rng.choice([0, (1 << 4) | (1 << 8), 1 << 11], S)]
    skew = [int(x) for x in rng.choice([0, 2, 3], S)]
    nh = [int(x) for x in rng.choice([0, 1, 2, 4], S)]
    nh[0], skew[0] = 2, 2
    if S > 1:
        nh[1], skew[1] = 0, 2
    if S > 2:
        nh[2], skew[2] = 4, 0
    relax = [K.RELAX[4] for _ in range(S)]  # entries past n_hops are not read
    cnt0 = rng.integers(0, 3, S * N).astype(np.uint32)
    dom = rng.integers(0, 6, S * N).astype(np.uint32)
    level = np.where(rng.random(S * C) < 0.05, NONE, 0).astype(np.uint32)
    cat = lambda k, i: np.concatenate([sc[k][i] for sc in scen])  # noqa: E731
    cont, nodes = [cat(0, i) for i in range(4)], [cat(1, i) for i in range(5)]

    def one(s):
        return FR.place(scen[s][0], scen[s][1], strat[s], preferred=pref[s], level=level[s * C:(s + 1) * C],
                        node_count=cnt0[s * N:(s + 1) * N], domain=dom[s * N:(s + 1) * N], max_skew=skew[s],
                        relax_mask=relax[s], n_hops=nh[s])
    return dict(C=C, N=N, base=base, cont=cont, nodes=nodes, strat=strat, pref=pref, skew=skew, nh=nh,
                relax=K.relax_rows(relax), cnt0=cnt0, dom=dom, level=level, scen=scen, one=one)


@pytest.mark.parametrize("S", [1, 3, 300])
def test_batch_host_and_device(S, planner):
    """The host and the device entry agree with each other and with the reference, every scenario of the
    batch (S = 300: more blocks than compute units, each with its own n_hops, masks and hops rows)."""
    import torch
    from fleetflow_amd import DevBatch
    b = _batch_case(S)
    C, N, base = b["C"], b["N"], b["base"]
    a, r, h, cost, after, cnt = planner.place_batch_policy_fallback(
        S, C, N, b["cont"], b["nodes"], b["strat"], b["pref"], level=b["level"], node_count=b["cnt0"], scen_base=base,
        domain=b["dom"], max_skew=b["skew"], relax_mask=b["relax"], n_hops=b["nh"])
    seen = 0
    for s in range(S):
        c, n = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N)
        exp = b["one"](s)
        _check((a[c], r[c], h[c], cost[s], tuple(x[n] for x in after), cnt[n]), exp, base + s)
        seen += int((exp[2] >= 1).sum())
        if b["nh"][s] == 0:  # a scenario without hops equals the spread entry's result
            e = SR.place(b["scen"][s][0], b["scen"][s][1], b["strat"][s], preferred=b["pref"][s], level=b["level"][c],
                         node_count=b["cnt0"][n], domain=b["dom"][n], max_skew=b["skew"][s])
            assert np.array_equal(a[c], e[0]) and np.array_equal(r[c], e[1]) and (h[c] == 0).all()
    assert seen >= 20  # on the reference: the batch relaxes
    # the device entry on the same batch
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(S, C, N, dev, scen_base=base, with_level=True)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.level, db.cf, db.mf, db.lab, db.cu),
                        (*b["cont"], b["level"], *b["nodes"][:4])):
        dst.copy_(t32(src))
    db.sched.copy_(torch.from_numpy(b["nodes"][4]).to(dev))
    cnt_t = t32(b["cnt0"])
    hops_t = torch.full((S * C,), 77, dtype=torch.uint8, device=dev)
    planner.dev_place_batch_policy_fallback(db, t32(b["strat"]), t32(b["pref"]), cnt_t, domain_t=t32(b["dom"]),
                                            max_skew_t=t32(b["skew"]), relax_mask_t=t32(b["relax"]), n_hops_t=t32(b["nh"]),
                                            hops_t=hops_t)
    planner.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert np.array_equal(u32(db.assign), a) and np.array_equal(db.reason.cpu().numpy(), r)
    assert np.array_equal(hops_t.cpu().numpy(), h)
    assert np.array_equal(db.cost.cpu().numpy().view(np.uint64), cost)
    for t, x in zip((db.cf, db.mf, db.cu, cnt_t), (after[0], after[1], after[3], cnt)):
        assert np.array_equal(u32(t), x)


def _host_entries_write_nothing(planner, b, bad_hops):
    """The two host entries through ctypes, on caller-owned buffers with a fill pattern: FP_EINVAL, and
    neither an output nor an in/out node array changes."""
    import ctypes as ct
    from fleetflow_amd import _lib
    from fleetflow_amd._lib import FpBatch, FpContainers, FpNodes
    L = _lib.load()
    S, C, N = len(bad_hops), b["C"], b["N"]
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).copy()  # noqa: E731
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    p8 = lambda x: x.ctypes.data_as(_lib.u8p)  # noqa: E731
    cont = [u32(x) for x in b["cont"]]
    cf, mf, lab, cu = (u32(x) for x in b["nodes"][:4])
    sched = np.ascontiguousarray(b["nodes"][4], np.uint8).copy()
    cnt = np.full(S * N, 5, np.uint32)
    assign, reason, hops = np.full(S * C, 0xABCDEF01, np.uint32), np.full(S * C, 9, np.uint8), np.full(S * C, 77, np.uint8)
    cost = np.full(S, 0x1234567890ABCDEF, np.uint64)
    strat, relax, nh = u32(b["strat"]), u32(b["relax"]), u32(bad_hops)
    before = [x.copy() for x in (cf, mf, cu, cnt, assign, reason, hops, cost)]

    def untouched():
        return all(np.array_equal(x, y) for x, y in zip(before, (cf, mf, cu, cnt, assign, reason, hops, cost)))
    bt = FpBatch(S, 0, C, N, *(x.ctypes.data for x in cont), None, cf.ctypes.data, mf.ctypes.data, lab.ctypes.data,
                 cu.ctypes.data, sched.ctypes.data, assign.ctypes.data, reason.ctypes.data, cost.ctypes.data)
    rc = L.fp_place_batch_policy_fallback(planner._ctx, ct.byref(bt), p32(strat), None, p32(cnt), None, None, p32(relax),
                                          p32(nh), p8(hops))
    assert rc == _lib.FP_EINVAL and untouched()
    # the single-scenario entry on scenario 0's slices of the same buffers
    cs = FpContainers(C, *(x.ctypes.data for x in cont))
    ns = FpNodes(N, cf.ctypes.data, mf.ctypes.data, lab.ctypes.data, cu.ctypes.data, sched.ctypes.data)
    rc = L.fp_place_policy_fallback(planner._ctx, ct.byref(cs), ct.byref(ns), None, 1, 0, p32(cnt), None, 0, p32(relax), 5,
                                    p32(assign), p8(reason), p8(hops))
    assert rc == _lib.FP_EINVAL and untouched()
    # the same call with a legal n_hops does write: the check above can fail
    rc = L.fp_place_policy_fallback(planner._ctx, ct.byref(cs), ct.byref(ns), None, 1, 0, p32(cnt), None, 0, p32(relax), 4,
                                    p32(assign), p8(reason), p8(hops))
    assert rc == 0 and not untouched() and (hops[:C] <= 4).all() and (hops[C:] == 77).all()


def test_errors_write_nothing(planner):
    import torch
    from fleetflow_amd import DevBatch
    from fleetflow_amd._lib import FP_EINVAL, FleetplaceError
    b = _batch_case(3)
    S, C, N = 3, b["C"], b["N"]
    bad = list(b["nh"])
    bad[2] = 5
    # host entries: refused before anything is staged
    with pytest.raises(FleetplaceError) as e:
        planner.place_policy_fallback(b["scen"][0][0], b["scen"][0][1], R.SPREAD, K.RELAX[4], n_hops=5)
    assert e.value.code == FP_EINVAL
    _host_entries_write_nothing(planner, b, bad)
    with pytest.raises(FleetplaceError) as e:
        planner.place_batch_policy_fallback(S, C, N, b["cont"], b["nodes"], b["strat"], b["pref"], relax_mask=b["relax"],
                                            n_hops=bad)
    assert e.value.code == FP_EINVAL
    # the device entry: found by the kernels, reported by sync(), nothing written
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(S, C, N, dev)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu), (*b["cont"], *b["nodes"][:4])):
        dst.copy_(t32(src))
    db.sched.copy_(torch.from_numpy(b["nodes"][4]).to(dev))
    db.assign.fill_(-7)
    db.reason.fill_(9)
    db.cost.fill_(-1)
    snap = db.node_snapshot()
    cnt_t = torch.full((S * N,), 5, dtype=torch.int32, device=dev)
    hops_t = torch.full((S * C,), 77, dtype=torch.uint8, device=dev)
    st_t, rm_t = t32(b["strat"]), t32(b["relax"])
    planner.dev_place_batch_policy_fallback(db, st_t, None, cnt_t, relax_mask_t=rm_t, n_hops_t=t32(bad), hops_t=hops_t)
    with pytest.raises(FleetplaceError) as e:
        planner.sync()
    assert e.value.code == FP_EINVAL
    assert bool((db.assign == -7).all()) and bool((db.reason == 9).all()) and bool((db.cost == -1).all())
    assert bool((hops_t == 77).all()) and bool((cnt_t == 5).all())
    assert all(torch.equal(x, y) for x, y in zip(snap, (db.cf, db.mf, db.cu)))
    planner.sync()  # reported once
    # the context still plans; hops_out = NULL works on the device and on the host
    planner.dev_place_batch_policy_fallback(db, st_t, None, None, relax_mask_t=rm_t, n_hops_t=t32(b["nh"]))
    planner.sync()
    exp = [FR.place(b["scen"][s][0], b["scen"][s][1], b["strat"][s], relax_mask=K.RELAX[4], n_hops=b["nh"][s]) for s in range(S)]
    got = db.assign.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(got[s * C:(s + 1) * C], exp[s][0]) for s in range(S))
    assert all(int(db.cost[s].item()) == FR.cost(exp[s][0], exp[s][1], s) for s in range(S))
    a, r, h, cost, _, _ = planner.place_batch_policy_fallback(S, C, N, b["cont"], b["nodes"], b["strat"], relax_mask=b["relax"],
                                                              n_hops=b["nh"], want_hops=False)
    assert h is None and np.array_equal(a, got)
    a1, r1, h1, _, _ = planner.place_policy_fallback(b["scen"][0][0], b["scen"][0][1], b["strat"][0], K.RELAX[2], want_hops=False)
    assert h1 is None and np.array_equal(a1, exp[0][0]) and np.array_equal(r1, exp[0][1])


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_inherited_behaviour(strategy, planner):
    """CYCLE gating with level, node_count in and out, an overlapping and a zero relax_mask, and
    relax_mask / n_hops NULL = the spread entry."""
    C, N = 300, 200
    cont, nodes = K.crafted(C, N)
    rng = np.random.default_rng(9)
    cnt0 = rng.integers(0, 6, N).astype(np.uint32)
    level = np.where(rng.random(C) < 0.1, NONE, 0).astype(np.uint32)
    dom = (np.arange(N) % 3).astype(np.uint32)
    pref = (1 << 4) | (1 << 8)
    # overlapping masks, a zero mask in the middle: hop 2 is skipped by construction, hops 1, 3, 4 are used
    relax = [K.MASK["class"] | 0x8, 0, K.MASK["class"] | K.MASK["region"], K.MASK["arch"] | K.MASK["tier"]]
    exp = FR.place(cont, nodes, strategy, preferred=pref, level=level, node_count=cnt0, domain=dom, max_skew=3,
                   relax_mask=relax)
    placed = exp[0] != NONE
    at = np.bincount(exp[2][placed], minlength=5)
    assert at[2] == 0 and at[1] >= 5 and at[3] >= 5 and at[4] >= 1 and (exp[1] == 2).sum() >= 15
    assert (exp[2][~placed] == 0).all()
    got = _run1(planner, cont, nodes, strategy, relax, domain=dom, max_skew=3, preferred=pref, level=level, node_count=cnt0,
                sid=3)
    _check(got, exp, 3)
    a, r, h, after, cnt = planner.place_policy_fallback(cont, nodes, strategy, relax, preferred=pref, level=level,
                                                        node_count=cnt0, domain=dom, max_skew=3)
    _check((a, r, h, None, after, cnt), exp)
    # node_count = NULL starts at zero and returns nothing
    a, r, h, after, cnt = planner.place_policy_fallback(cont, nodes, strategy, relax, level=level)
    assert cnt is None
    _check((a, r, h, None, after, None), FR.place(cont, nodes, strategy, level=level, relax_mask=relax))
    # either pointer NULL: the spread entry, hops all zero
    e = SR.place(cont, nodes, strategy, preferred=pref, level=level, node_count=cnt0, domain=dom, max_skew=3)
    for kw in (dict(relax_mask=K.relax_rows([relax])), dict(n_hops=[4]), {}):
        a, r, h, cost, after, cnt = planner.place_batch_policy_fallback(1, C, N, cont, nodes, [strategy], [pref], level=level,
                                                                        node_count=cnt0, domain=dom, max_skew=[3], **kw)
        _check((a, r, h, cost[0], after, cnt), (e[0], e[1], np.zeros(C, np.uint8), e[2], e[3]), 0)
    assert (exp[0] != e[0]).sum() > 20  # and the chain changes the plan on these inputs


STAGE_KDL = """
project "demo"
server "g0" { capacity cpu=1000 memory=8192; label "class=gpu"; label "region=tokyo" }
server "c0" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=tokyo" }
server "c1" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=osaka" }
service "train" { resources cpu=900 memory=64; require "class=gpu" "region=tokyo" }
service "infer" { resources cpu=800 memory=64; require "class=gpu" "region=tokyo" }
service "web" { resources cpu=100 memory=64; require "region=osaka" }
stage "live" {
    service "train"
    service "infer"
    service "web"
    server "g0"
    server "c0"
    server "c1"
    %s
}
"""


def test_plan_stage_from_kdl_with_a_fallback_node(planner):
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run
    flow = parse_kdl_string(STAGE_KDL % 'placement { fallback "class" "region" }')
    plain = parse_kdl_string(STAGE_KDL % "")
    plan, base = plan_stage(flow, "live", planner), plan_stage(plain, "live", planner)
    # the one gpu server holds train; infer's class is unavailable, so it gives class up and stays in tokyo
    assert base.assignment == {"train": "g0", "web": "c1"} and base.rejected == {"infer": "NOFIT"}
    assert plan.assignment == {"train": "g0", "infer": "c0", "web": "c1"} and plan.rejected == {}
    assert plan.relaxed == {"infer": ["class"]}
    assert (plan.fallback_relax_order, plan.fallback_max_hops) == (["class", "region"], None)
    out = format_up_dry_run(flow, "live", plan)
    assert "    配置先: c0 (緩和: class)" in out and "  配置フォールバック: class → region" in out
    assert "    配置先: g0\n" in out
    assert (plan.order, plan.levels, plan.level_order, plan.candidates) == (base.order, base.levels, base.level_order, base.candidates)
    assert base.relaxed == {} and "緩和" not in format_up_dry_run(plain, "live", base)
