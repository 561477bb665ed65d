"""GPU tests of the drain what-if sweep (SPEC.md 2.11; fleetflow_amd/csrc/fp_drain.hip): both entry points
against the numpy reference (tests/drain_ref.py), which makes one policy_ref.place call per candidate.  Every
comparison is exact: assign_out, reason and every word of every summary row."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import policy_ref as R  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 0x5EED0011
PREF2 = (1 << 4) | (1 << 8)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _live(C, N, strategy, flags=7, scen=2, counts=False):
    """Generated containers placed on generated nodes by the reference under ``strategy``: (cont, live node
    table, assign, counts after).  ``counts`` starts the placement from non-zero node counts."""
    from oracle import oracle as O
    cont, nodes = O.gen_scenario(SEED, scen, C, N, flags)
    cnt0 = (np.arange(N, dtype=np.uint32) * 7) % 5 if counts else None
    a, _, after, cnt = R.place(cont, nodes, strategy, node_count=cnt0)
    _ro(*cont, *after, a, cnt)
    return cont, after, a, cnt


def _check(got, exp):
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(got[1], exp[1])
    assert got[2].shape == exp[2].shape and np.array_equal(got[2], exp[2])


def _both(planner, cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None):
    got = planner.drain_sweep(cont, nodes, assign, group, n_cand, strategy, preferred, node_count)
    _check(got, D.sweep(cont, nodes, assign, group, n_cand, strategy, preferred, node_count))
    return got


# ---- geometry: 64 x 1 and 1024 x {1, 2, 4, 8}, on both sides of every switch ---------------------------------
GEOMETRY = [(40, 1), (40, 2), (200, 63), (200, 64), (200, 65), (2000, 1024), (2000, 1025), (2000, 2048), (2000, 2049),
            (3000, 4096), (3000, 4097), (4000, 8192)]


@pytest.mark.parametrize("i", range(len(GEOMETRY)))
def test_every_block_geometry(i, planner):
    """Single-server candidates up to 65 nodes, 64 zone candidates above; the strategy rotates with the shape."""
    C, N = GEOMETRY[i]
    strategy = i % 4
    cont, nodes, assign, cnt = _live(C, N, strategy)
    if N <= 65:
        group, n_cand = np.arange(N, dtype=np.uint32), N
    else:
        group, n_cand = (np.arange(N, dtype=np.uint32) * 37) % 64, 64
    got = _both(planner, cont, nodes, assign, group, n_cand, strategy, PREF2 if i % 2 else 0, cnt)
    running = int((assign != NONE).sum())
    assert int(got[2][:, D.EVICTED].sum()) == running and running > 0
    assert int(got[2][:, D.NODES].sum()) <= N


# ---- evictee counts round the 64-record chunk ------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 128, 129)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_evictee_counts_at_the_chunk_boundaries(strategy, planner):
    """Candidate k holds COUNTS[k] containers on one node; 20 more nodes take what fits."""
    rng = np.random.default_rng(11)
    C, N = sum(COUNTS), len(COUNTS) + 20
    cont = (rng.integers(1, 40, C).astype(np.uint32) * 10, rng.integers(1, 9, C).astype(np.uint32) * 64,
            np.zeros(C, np.uint32), np.where(rng.random(C) < 0.2, 1 << 16, 0).astype(np.uint32))
    assign = rng.permutation(np.repeat(np.arange(len(COUNTS)), COUNTS)).astype(np.uint32)
    nodes = (rng.integers(300, 1500, N).astype(np.uint32), np.full(N, 4096, np.uint32), np.zeros(N, np.uint32),
             np.zeros(N, np.uint32), np.ones(N, np.uint8))
    group = np.where(np.arange(N) < len(COUNTS), np.arange(N), NONE).astype(np.uint32)
    got = _both(planner, cont, nodes, assign, group, len(COUNTS), strategy)
    assert got[2][:, D.EVICTED].tolist() == list(COUNTS)
    assert got[2][1, D.STRANDED] == 0 and (got[2][5:, D.STRANDED] > 0).all()  # 128 and more do not fit the 20 nodes


def test_all_containers_on_one_node(planner):
    cont, nodes, _, _ = _live(300, 70, 0)
    assign = np.full(300, 5, np.uint32)
    for st in (R.FIRST_FIT, R.SPREAD):
        got = _both(planner, cont, nodes, assign, np.arange(70, dtype=np.uint32), 70, st)
        assert got[2][5, D.EVICTED] == 300 and got[2][:, D.EVICTED].sum() == 300


# ---- strategies x preferred labels x node counts ------------------------------------------------------------------
@pytest.mark.parametrize("pref", [0, PREF2, 0xFFFFFFFF])
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_strategies_preferred_and_counts(strategy, pref, planner):
    cont, nodes, assign, cnt = _live(500, 130, strategy, counts=True)
    assert cnt.max() > 4
    got = _both(planner, cont, nodes, assign, np.arange(130, dtype=np.uint32), 130, strategy, pref, cnt)
    # no node_count is zeros
    none = planner.drain_sweep(cont, nodes, assign, np.arange(130), 130, strategy, pref)
    _check(none, D.sweep(cont, nodes, assign, np.arange(130), 130, strategy, pref, np.zeros(130, np.uint32)))
    if strategy == R.SPREAD:
        assert not np.array_equal(none[0], got[0])  # the counts matter


# ---- the generator's inputs: candidates that strand and candidates that do not --------------------------------
@functools.lru_cache(maxsize=None)
def _generated(seed, C, N, strategy):
    from oracle import pyoracle as P
    cont = tuple(np.array(x, np.uint32) for x in P.gen_containers(P.scenario_seed(seed, 0), C, 7))
    nodes = P.gen_nodes(P.scenario_seed(seed, 0), N)
    nodes = tuple(np.array(x, np.uint32) for x in nodes[:4]) + (np.array(nodes[4], np.uint8),)
    assign, live, cnt = D.live(cont, nodes, strategy)
    exp = D.sweep(cont, live, assign, np.arange(N), N, strategy, 0, cnt)
    return cont, live, assign, cnt, exp


@pytest.mark.parametrize("seed,C,N,strategy", [(5, 384, 64, s) for s in R.STRATEGIES]
                         + [(9, 800, 100, s) for s in (R.FIRST_FIT, R.PACK, R.FILL_LOWEST)])
def test_generated_fleet_every_single_server(seed, C, N, strategy, planner):
    cont, live, assign, cnt, exp = _generated(seed, C, N, strategy)
    rows = exp[2]
    assert int((rows[:, D.STRANDED] > 0).sum()) >= 10  # the condition, on the reference
    assert int(((rows[:, D.EVICTED] > 0) & (rows[:, D.STRANDED] == 0)).sum()) >= 10
    _check(planner.drain_sweep(cont, live, assign, np.arange(N), N, strategy, 0, cnt), exp)


# ---- crafted cases --------------------------------------------------------------------------------------------
def _plain_nodes(cf, sched=None):
    n = len(cf)
    return (np.array(cf, np.uint32), np.full(n, 1 << 20, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
            np.array(sched if sched is not None else [1] * n, np.uint8))


def test_zone_evictees_sharing_an_anti_affinity_bit_land_on_distinct_targets(planner):
    """Zone 0 = nodes 0..2, one container of the group on each; the targets could each take all three."""
    cont = (np.array([100, 100, 100, 50], np.uint32), np.ones(4, np.uint32), np.zeros(4, np.uint32),
            np.array([1 << 20, 1 << 20, 1 << 20, 0], np.uint32))
    nodes = _plain_nodes([0, 0, 0, 1000, 1000, 1000, 1000])
    group = np.array([0, 0, 0, 1, 1, NONE, NONE], np.uint32)
    for st in R.STRATEGIES:
        got = _both(planner, cont, nodes, [0, 1, 2, 0], group, 2, st)
        assert len(set(got[0][:3].tolist())) == 3 and got[2][0, D.TARGETS] >= 3
    # with two targets left the third is stranded
    got = _both(planner, cont, nodes, [0, 1, 2, 0], [0, 0, 0, 1, 1, 0, 0], 2)
    assert got[0].tolist() == [3, 4, NONE, 3] and got[2][0, :7].tolist() == [4, 1, 100, 1, 2, 2, 5]


def test_equal_evictees_go_by_index(planner):
    C = 150  # more than two record chunks
    cont = (np.full(C, 30, np.uint32), np.full(C, 2, np.uint32), np.zeros(C, np.uint32), np.zeros(C, np.uint32))
    nodes = _plain_nodes([0] + [30] * 100)
    got = _both(planner, cont, nodes, np.zeros(C, np.uint32), [0] + [NONE] * 100, 1)
    assert got[0].tolist() == list(range(1, 101)) + [NONE] * 50 and got[2][0, D.FIRST_STRANDED] == 100


def test_unschedulable_nodes_inside_and_outside_a_candidate(planner):
    cont = (np.array([10, 20, 30], np.uint32), np.ones(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint32))
    nodes = _plain_nodes([100, 100, 100, 100], sched=[0, 1, 0, 1])
    got = _both(planner, cont, nodes, [0, 0, 1], [0, 1, 2, 3], 4)
    assert got[0].tolist() == [1, 1, 3]  # node 0's containers leave it; node 2 is never a target
    assert got[2][:, D.EVICTED].tolist() == [2, 1, 0, 0]


def test_containers_that_do_not_run_and_groups_of_none(planner):
    cont, nodes, assign, cnt = _live(300, 70, 2)
    assign = assign.copy()
    assign[::3] = NONE
    got = _both(planner, cont, nodes, assign, np.arange(70, dtype=np.uint32), 70, 2, 0, cnt)
    assert (got[0][::3] == NONE).all() and not got[1][::3].any()
    got = _both(planner, cont, nodes, assign, np.full(70, NONE, np.uint32), 3)
    assert np.array_equal(got[0], assign) and not got[1].any()
    assert got[2][:, :7].tolist() == [[0, 0, 0, 0, 0, NONE, 0]] * 3
    got = _both(planner, cont, nodes, assign, np.full(70, NONE, np.uint32), 0)
    assert np.array_equal(got[0], assign) and got[2].shape == (0, 8)
    # no container at all: rows of zeros
    none = tuple(np.zeros(0, np.uint32) for _ in range(4))
    got = _both(planner, none, nodes, np.zeros(0, np.uint32), np.arange(70, dtype=np.uint32), 70)
    assert got[2][:, :7].tolist() == [[0, 0, 0, 0, 0, NONE, 0]] * 70


def test_one_candidate_holding_every_node(planner):
    cont, nodes, assign, cnt = _live(300, 70, 1)
    got = _both(planner, cont, nodes, assign, np.zeros(70, np.uint32), 1, 1, 0, cnt)
    run = assign != NONE
    assert (got[0] == NONE).all() and np.array_equal(got[1], run.astype(np.uint8))
    assert got[2][0, D.TARGETS] == 0 and got[2][0, D.STRANDED] == got[2][0, D.EVICTED] == run.sum()
    assert got[2][0, D.NODES] == 70


# ---- independence, and the differential against the scored placer ------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_candidates_are_independent_and_equal_one_place_policy_call(strategy, planner):
    """Candidate k's moves and row do not change when every other node belongs to no candidate, and they are
    what Planner.place_policy (fp_policy.hip) makes of k's evictees on the masked table."""
    N = 64
    cont, live, assign, cnt, exp = _generated(5, 384, N, strategy)
    full = planner.drain_sweep(cont, live, assign, np.arange(N), N, strategy, PREF2, cnt)
    for k in (0, 7, 31, 63):
        alone = np.where(np.arange(N) == k, k, NONE).astype(np.uint32)
        one = planner.drain_sweep(cont, live, assign, alone, N, strategy, PREF2, cnt)
        ev = np.flatnonzero(assign == k)
        assert np.array_equal(one[0][ev], full[0][ev]) and np.array_equal(one[1][ev], full[1][ev])
        assert np.array_equal(one[2][k], full[2][k])
        rest = np.setdiff1d(np.arange(assign.size), ev)
        assert np.array_equal(one[0][rest], assign[rest]) and not one[1][rest].any()
        sched = live[4] * (np.arange(N) != k)
        a, r, _, _ = planner.place_policy(tuple(x[ev] for x in cont), (*live[:4], sched), strategy, PREF2,
                                          node_count=cnt)
        assert np.array_equal(a, full[0][ev]) and np.array_equal(r, full[1][ev])


def test_inputs_are_inputs(planner):
    cont, nodes, assign, cnt = (tuple(x.copy() for x in t) if isinstance(t, tuple) else t.copy()
                                for t in _live(500, 130, 3, counts=True))
    group = (np.arange(130, dtype=np.uint32) * 3) % 20
    before = [x.tobytes() for x in (*cont, *nodes, assign, cnt, group)]
    planner.drain_sweep(cont, nodes, assign, group, 20, 3, PREF2, cnt)
    assert [x.tobytes() for x in (*cont, *nodes, assign, cnt, group)] == before


# ---- the device entry -------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
    return t.to("cuda:0")


def _dev_call(planner, cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None, fill=0x5A):
    """dev_drain_sweep on copies of the inputs; returns (the call's tensors, the outputs as numpy).  The outputs
    start filled with ``fill`` bytes."""
    import torch
    C = len(assign)
    ins = ([_dev(np.asarray(x, np.uint32)) for x in cont],
           [_dev(np.asarray(x, np.uint32)) for x in nodes[:4]] + [_dev(np.asarray(nodes[4], np.uint8))],
           _dev(np.asarray(assign, np.uint32)), _dev(np.asarray(group, np.uint32)),
           None if node_count is None else _dev(np.asarray(node_count, np.uint32)))
    out = torch.full((C,), fill * 0x01010101 - (1 << 32) * (fill >= 0x80), dtype=torch.int32, device="cuda:0")
    reason = torch.full((C,), fill, dtype=torch.uint8, device="cuda:0")
    rows = torch.full((n_cand * 8,), fill * 0x01010101 - (1 << 32) * (fill >= 0x80), dtype=torch.int32, device="cuda:0")
    planner.dev_drain_sweep(tuple(ins[0]), tuple(ins[1]), ins[2], ins[3], n_cand, out, reason, rows, strategy, preferred,
                            ins[4])
    return ins, (out, reason, rows)


def _np_out(outs, n_cand):
    out, reason, rows = outs
    return (out.cpu().numpy().view(np.uint32), reason.cpu().numpy(), rows.cpu().numpy().view(np.uint32).reshape(n_cand, 8))


def test_device_entry_equals_the_host_entry_and_keeps_its_inputs(planner):
    cont, nodes, assign, cnt = _live(500, 130, 1, counts=True)
    group = np.arange(130, dtype=np.uint32)
    ins, outs = _dev_call(planner, cont, nodes, assign, group, 130, 1, PREF2, cnt)
    planner.sync()
    _check(_np_out(outs, 130), planner.drain_sweep(cont, nodes, assign, group, 130, 1, PREF2, cnt))
    flat = [*ins[0], *ins[1], ins[2], ins[3], ins[4]]
    for t, a in zip(flat, (*cont, *nodes, assign, group, cnt)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_two_device_calls_of_different_shapes_with_a_placement_between(planner):
    """The calls share the context's workspace: a larger call, a place_batch, then a smaller call."""
    big = _live(2000, 1025, 2)
    small = _live(200, 63, 3)
    gb, gs = (np.arange(1025, dtype=np.uint32) * 37) % 64, np.arange(63, dtype=np.uint32)
    _, o1 = _dev_call(planner, big[0], big[1], big[2], gb, 64, 2, 0, big[3])
    from oracle import oracle as O
    cont, nodes = O.gen_scenario(SEED, 9, 300, 40, 7)
    a, r, _, _ = planner.place_batch(1, 300, 40, cont, nodes)
    _, o2 = _dev_call(planner, small[0], small[1], small[2], gs, 63, 3, PREF2, small[3])
    planner.sync()
    _check(_np_out(o1, 64), D.sweep(big[0], big[1], big[2], gb, 64, 2, 0, big[3]))
    _check(_np_out(o2, 63), D.sweep(small[0], small[1], small[2], gs, 63, 3, PREF2, small[3]))
    ea, er, _, _ = O.place(cont, nodes)
    assert np.array_equal(a, ea) and np.array_equal(r, er)


# ---- errors: nothing is written -----------------------------------------------------------------------------------
def _raw_host(planner, cont, nodes, assign, group, n_cand, strategy=0, alias=False):
    """fp_drain_sweep itself, on outputs pre-filled with 0xA5: (rc, outputs untouched?)."""
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)  # noqa: E731
    cont, assign, group = tuple(u32(x) for x in cont), u32(assign).copy(), u32(group)
    nodes = tuple(u32(x) for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8),)
    C, N = assign.size, group.size
    out = assign if alias else np.full(C, 0xA5A5A5A5, np.uint32)
    reason, rows = np.full(C, 0xA5, np.uint8), np.full(n_cand * 8, 0xA5A5A5A5, np.uint32)
    keep = out.copy()
    cs = _lib.FpContainers(C, *(x.ctypes.data for x in cont))
    ns = _lib.FpNodes(N, *(x.ctypes.data for x in nodes))
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    rc = planner._L.fp_drain_sweep(planner._ctx, ct.byref(cs), ct.byref(ns), p(assign, _lib.u32p), p(group, _lib.u32p),
                                   n_cand, strategy, 0, None, p(out, _lib.u32p), p(reason, _lib.u8p), p(rows, _lib.u32p))
    untouched = np.array_equal(out, keep) and (reason == 0xA5).all() and (rows == 0xA5A5A5A5).all()
    return rc, bool(untouched)


def _bad_cases():
    cont, nodes, assign, _ = _live(200, 65, 0)
    group = np.arange(65, dtype=np.uint32)
    bad_group, bad_assign, last_assign = group.copy(), assign.copy(), assign.copy()
    bad_group[64] = 65
    bad_assign[0] = 65
    last_assign[199] = 0xFFFFFFFE
    big = tuple(np.resize(x, 8193) for x in nodes)
    return cont, nodes, assign, group, [
        ("strategy", _lib.FP_EINVAL, dict(nodes=nodes, assign=assign, group=group, n_cand=65, strategy=4)),
        ("nodes", _lib.FP_EOVERFLOW, dict(nodes=big, assign=assign, group=np.zeros(8193, np.uint32), n_cand=1)),
        ("n_cand", _lib.FP_EOVERFLOW, dict(nodes=nodes, assign=assign, group=group, n_cand=8193)),
        ("group", _lib.FP_EINVAL, dict(nodes=nodes, assign=assign, group=bad_group, n_cand=65)),
        ("group == n_cand", _lib.FP_EINVAL, dict(nodes=nodes, assign=assign, group=group, n_cand=64)),
        ("assign", _lib.FP_EINVAL, dict(nodes=nodes, assign=bad_assign, group=group, n_cand=65)),
        ("assign, last", _lib.FP_EINVAL, dict(nodes=nodes, assign=last_assign, group=group, n_cand=65)),
    ]


def test_host_entry_errors_write_nothing(planner):
    cont, nodes, assign, group, cases = _bad_cases()
    for name, code, kw in cases:
        assert _raw_host(planner, cont, **kw) == (code, True), name
    assert _raw_host(planner, cont, nodes, assign, group, 65, alias=True) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, cont, nodes, assign, group, 65) == (_lib.FP_OK, False)  # and the same call is fine
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.drain_sweep(cont, nodes, assign, group, 65, strategy=7)
    assert e.value.code == _lib.FP_EINVAL


def test_device_entry_errors_write_nothing_and_the_context_goes_on(planner):
    import torch
    cont, nodes, assign, group, cases = _bad_cases()
    for name, code, kw in cases:
        on_device = name.startswith(("group", "assign"))
        if on_device:  # found on the device: the call returns, sync() reports
            _, outs = _dev_call(planner, cont, kw["nodes"], kw["assign"], kw["group"], kw["n_cand"], fill=0xA5)
            with pytest.raises(_lib.FleetplaceError) as e:
                planner.sync()
        else:
            with pytest.raises(_lib.FleetplaceError) as e:
                _dev_call(planner, cont, kw["nodes"], kw["assign"], kw["group"], kw["n_cand"], kw.get("strategy", 0))
        assert e.value.code == code, name
        if on_device:
            out, reason, rows = _np_out(outs, kw["n_cand"])
            assert (out == 0xA5A5A5A5).all() and (reason == 0xA5).all() and (rows == 0xA5A5A5A5).all(), name
        planner.sync()  # reported once, then clear
    # assign_out == assign
    ins, _ = _dev_call(planner, cont, nodes, assign, group, 65)
    rows, reason = torch.zeros(65 * 8, dtype=torch.int32, device="cuda:0"), torch.zeros(200, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.dev_drain_sweep(tuple(ins[0]), tuple(ins[1]), ins[2], ins[3], 65, ins[2], reason, rows)
    assert e.value.code == _lib.FP_EINVAL
    planner.sync()
    _, outs = _dev_call(planner, cont, nodes, assign, group, 65, 3)
    planner.sync()
    _check(_np_out(outs, 65), D.sweep(cont, nodes, assign, group, 65, 3))


# ---- the flow-level path ----------------------------------------------------------------------------------------
def _stage_text(placement):
    servers = "\n".join(
        f'server "n{i}" {{ capacity cpu={2000 + 1000 * (i % 3)} memory={4096 + 2048 * (i % 2)}; '
        f'label "region={"tokyo" if i % 3 == 0 else "osaka"}"; label "class={"gpu" if i % 4 == 1 else "cpu"}"'
        + ('; scheduling "cordon"' if i == 2 else "") + " }" for i in range(8))
    services = "\n".join(
        f'service "s{i}" {{ resources cpu={300 + 100 * (i % 4)} memory={512 * (1 + i % 3)}'
        + ('; require "class=gpu"' if i % 7 == 0 else "") + " }" for i in range(24))
    members = "\n".join(f'    service "s{i}"' for i in range(24)) + "\n" + "\n".join(f'    server "n{i}"' for i in range(8))
    return f'project "demo"\n{servers}\n{services}\nstage "live" {{\n{members}\n    {placement}\n}}\n'


@pytest.mark.parametrize("strategy", ["spread_across_pool", "pack_into_dedicated", "fill_lowest"])
def test_drain_stage_from_kdl_with_a_placement_node(strategy, planner):
    from fleetflow_amd.flow import drain_stage, live_tables, plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import drain_report_from_json, drain_report_to_json, format_drain_report
    flow = parse_kdl_string(_stage_text(f'placement strategy="{strategy}" {{ prefer "region=tokyo" }}'))
    plan = plan_stage(flow, "live", planner)
    names, nodes, cont, live, assign, count, st, pmask = live_tables(flow, "live", plan)
    assert st == strategy and pmask != 0 and len(plan.assignment) >= 20
    sid = _lib.POLICY_STRATEGIES[strategy]
    slugs = [n.slug for n in nodes]
    for by, group, cand in ((None, list(range(8)), slugs),
                            ("region", [0 if i % 3 == 0 else 1 for i in range(8)], ["region=tokyo", "region=osaka"])):
        rep = drain_stage(flow, "live", plan, by=by, planner=planner)
        out, _, rows = D.sweep(cont, live, assign, group, len(cand), sid, pmask, count)
        assert [c.name for c in rep.candidates] == cand and rep.strategy == strategy
        for k, c in enumerate(rep.candidates):
            ev = [v for v in R.ffd_order(cont[0], cont[1]) if assign[v] != NONE and group[assign[v]] == k]
            assert c.moves == [(names[v], slugs[assign[v]], slugs[out[v]]) for v in ev if out[v] != NONE]
            assert c.stranded == [names[v] for v in ev if out[v] == NONE]
            assert (c.evicted, c.targets) == (int(rows[k, D.EVICTED]), int(rows[k, D.TARGETS]))
        assert drain_report_from_json(drain_report_to_json(rep)) == rep
        assert format_drain_report(rep).count("\ndrain ") == len(cand) - 1
    assert any(c.stranded for c in rep.candidates)  # the gpu-class services have nowhere to go without a region
