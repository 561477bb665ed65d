"""Rejection diagnosis on the GPU (SPEC.md 2.9): fp_explain / fp_explain_batch and their device entries
against the numpy reference, word for word.  The kernels' paths: a row leaves as one 64-byte store when the
node range is not split (N <= 64, or 2048 blocks and more) and through atomics otherwise; the rows kernel
carries 512 containers per block, the batch kernel 1024."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explain_cases as K  # noqa: E402
import explain_ref as ER  # noqa: E402
from test_gpu_policy_fallback import STAGE_KDL  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NOFIT, CYCLE, SKEW = 1, 2, 3
IGNORE = 0x2078  # bit 13 (the label no node has) and the region dimension


def _t32(x, dev="cuda:0"):
    import torch
    return torch.from_numpy(np.array(x, np.uint32).view(np.int32)).to(dev)  # a copy: the inputs are read-only


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 300, 1100])
def test_rows_vs_reference(C, N, planner):
    cont, nodes = K.crafted(C, N)
    snap = [np.array(a) for a in (*cont, *nodes)]
    exp = K.expected(C, N)
    if (C, N) in K.SHAPES:
        K.assert_floors(exp)
    got = planner.explain(cont, nodes)
    assert got.shape == (C, 16) and got.dtype == np.uint32
    assert np.array_equal(got, exp)
    assert np.array_equal(planner.explain(cont, nodes, ignore_labels=IGNORE), K.expected(C, N, IGNORE))
    assert all(np.array_equal(a, b) for a, b in zip(snap, (*cont, *nodes)))  # no input is modified


@pytest.mark.parametrize("N", [0, 64, 65, 1025])
@pytest.mark.parametrize("C", [1, 65, 1100])
def test_selection(C, N, planner):
    """sel: a permuted subset, repeats, n_sel = 0, 1, 64, 65 -- rows in sel's order."""
    cont, nodes = K.crafted(C, N)
    rng = np.random.default_rng(C + N)
    for ign in (0, IGNORE):
        exp = K.expected(C, N, ign)
        sels = [rng.permutation(C)[:max(1, C // 3)], rng.integers(0, C, 2 * C + 3)]
        sels += [rng.integers(0, C, m) for m in (0, 1, 64, 65)]
        for sel in sels:
            got = planner.explain(cont, nodes, sel=sel, ignore_labels=ign)
            assert got.shape == (len(sel), 16) and np.array_equal(got, exp[sel])


def test_all_cordoned_and_the_unsplit_large_call(planner):
    """ALL bit 0 on a table with every node cordoned; and 2048 blocks of selected containers (repeats of 64),
    where the node range is no longer split: rows stored whole, over two LDS tiles."""
    cont, nodes = K.all_cordoned(300, 65)
    got = planner.explain(cont, nodes)
    assert np.array_equal(got, ER.rows(cont, nodes)) and (got[:, ER.ALL] & ER.CORDON).all()
    C, N = 64, 1030
    cont, nodes = K.crafted(C, N)
    exp = K.expected(C, N)
    for m in (2047 * 512, 2048 * 512):  # split, not split
        sel = (np.arange(m) * 7 % C).astype(np.uint32)
        got = planner.explain(cont, nodes, sel=sel)
        assert np.array_equal(got, exp[sel])


def _dev_batch(b, nodes, reason=None):
    import torch
    from fleetflow_amd import DevBatch
    db = DevBatch.allocate(b["S"], b["C"], b["N"], "cuda:0")
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu), (*b["cont"], *nodes[:4])):
        dst.copy_(_t32(src))
    db.sched.copy_(torch.from_numpy(np.array(nodes[4], np.uint8)).to("cuda:0"))
    db.reason.fill_(9)
    if reason is not None:
        db.reason.copy_(torch.from_numpy(reason).to("cuda:0"))
    return db


def test_device_entry_matches_the_host_entry(planner):
    """One scenario of a DevBatch through offset pointers: sel = NULL and a sel with repeats."""
    import torch
    b = K.batch_case(3)
    C, N = b["C"], b["N"]
    db = _dev_batch(b, b["nodes"])
    snap = [t.clone() for t in (db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu, db.sched, db.reason)]
    for s in (0, 2):
        cont, nodes = b["scen"][s]
        host = planner.explain(cont, nodes, ignore_labels=IGNORE)
        assert np.array_equal(host, ER.rows(cont, nodes, ignore=IGNORE))
        rows_t = torch.full((C * 16,), -3, dtype=torch.int32, device="cuda:0")
        planner.dev_explain(db, rows_t, ignore_labels=IGNORE, scenario=s)
        planner.sync()
        assert np.array_equal(_u32(rows_t).reshape(C, 16), host)
        sel = np.random.default_rng(s).integers(0, C, 700).astype(np.uint32)
        rows_t = torch.full((700 * 16 + 16,), -3, dtype=torch.int32, device="cuda:0")
        planner.dev_explain(db, rows_t, sel_t=_t32(sel), scenario=s)
        planner.sync()
        got = _u32(rows_t)
        assert np.array_equal(got[:700 * 16].reshape(700, 16), planner.explain(cont, nodes, sel=sel))
        assert (got[700 * 16:] == 0xFFFFFFFD).all()  # nothing past the last row
    assert all(torch.equal(x, y) for x, y in zip(snap, (db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu,
                                                        db.sched, db.reason)))


def _expected_hist(b, nodes, reason, mask, ignore):
    S, C, N = b["S"], b["C"], b["N"]
    out = np.zeros((S, 8), np.uint32)
    for s in range(S):
        r = ER.rows_matrix(b["scen"][s][0], tuple(x[s * N:(s + 1) * N] for x in nodes), 0 if ignore is None else int(ignore[s]))
        pick = np.ones(C, bool) if mask == 0 else ((mask >> reason[s * C:(s + 1) * C].astype(np.uint32)) & 1).astype(bool)
        out[s] = ER.hist(r[pick])
    return out


@pytest.mark.parametrize("S", [1, 3, 300])
def test_batch_histograms(S, planner):
    """reason and the node state from a real place_batch_policy_fallback call (CYCLE levels, SKEW present);
    per-scenario ignore_labels = the chain's cum[n_hops]; the host and the device entry."""
    import torch
    b = K.batch_case(S)
    C, N = b["C"], b["N"]
    _, reason, _, _, after, _ = planner.place_batch_policy_fallback(
        S, C, N, b["cont"], b["nodes"], b["strat"], level=b["level"], domain=b["dom"], max_skew=b["skew"],
        relax_mask=b["relax"], n_hops=b["nh"], want_hops=False)
    assert (reason == CYCLE).sum() >= 5 and (reason == SKEW).sum() >= 1 and (reason == NOFIT).sum() >= 50
    db = _dev_batch(b, after, reason)
    ign_t = _t32(b["ignore"])
    for mask in (0, 1 << NOFIT, (1 << NOFIT) | (1 << SKEW)):
        exp = _expected_hist(b, after, reason, mask, b["ignore"])
        n_match = [int(np.isin(reason[s * C:(s + 1) * C], [r for r in range(8) if mask >> r & 1]).sum()) if mask else C
                   for s in range(S)]
        assert exp[:, 7].tolist() == n_match
        got = planner.explain_batch(S, C, N, b["cont"], after, reason, mask, b["ignore"])
        assert got.shape == (S, 8) and np.array_equal(got, exp)
        hist_t = torch.full((S * 8,), -3, dtype=torch.int32, device="cuda:0")
        planner.dev_explain_batch(db, mask, ign_t, hist_t)
        planner.sync()
        assert np.array_equal(_u32(hist_t).reshape(S, 8), exp)
    # ignore_labels = NULL is 0; reason is not read with reason_mask = 0
    exp = _expected_hist(b, after, reason, 0, None)
    assert np.array_equal(planner.explain_batch(S, C, N, b["cont"], after, None, 0), exp)
    assert np.array_equal(db.reason.cpu().numpy(), reason)  # the entry writes only hist_out


@pytest.mark.parametrize("S,C,N", [(3, 300, 64), (3, 1100, 64), (2048, 8, 1030), (2, 1100, 0), (5, 1100, 1025)])
def test_batch_paths(S, C, N, planner):
    """The batch kernel's other paths: an unsplit node range (N <= 64, with one and with two blocks of 1024
    containers; 2048 blocks over two LDS tiles), N = 0, and a split range with two blocks per scenario over
    two LDS tiles.  reason: a synthetic pattern."""
    scen = [K.crafted(C, N, seed=s % 3) for s in range(S)]
    b = dict(S=S, C=C, N=N, scen=scen, cont=[np.concatenate([sc[0][i] for sc in scen]) for i in range(4)])
    nodes = [np.concatenate([sc[1][i] for sc in scen]) for i in range(5)]
    rng = np.random.default_rng(S + C + N)
    reason = rng.choice(np.array([0, 1, 1, 2, 3], np.uint8), S * C)
    ignore = rng.choice(np.array([0, IGNORE, 0x7], np.uint32), S)
    for mask in (0, 1 << NOFIT, (1 << NOFIT) | (1 << SKEW)):
        got = planner.explain_batch(S, C, N, b["cont"], nodes, reason, mask, ignore)
        assert np.array_equal(got, _expected_hist(b, nodes, reason, mask, ignore))


def test_monotonicity(planner):
    """SPEC.md 2.9's corollary: on the table a placement call left, every NOFIT container has FEASIBLE == 0
    (word 6 of its histogram is 0) -- after place, after place_policy for each strategy, and after the
    fallback entry with ignore = cum[n_hops]."""
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    cum = int(np.bitwise_or.reduce(np.array(K.RELAX[:2], np.uint32)))
    runs = [(planner.place(cont, nodes)[1:], 0)]
    for strategy in range(4):
        a, r, after, _ = planner.place_policy(cont, nodes, strategy)
        runs.append(((r, after), 0))
        a, r, _, after, _ = planner.place_policy_fallback(cont, nodes, strategy, K.RELAX[:2], want_hops=False)
        runs.append(((r, after), cum))
    for (reason, after), ign in runs:
        nofit = np.flatnonzero(reason == NOFIT)
        assert nofit.size >= 50
        rows = planner.explain(cont, after, sel=nofit, ignore_labels=ign)
        assert (rows[:, ER.FEASIBLE] == 0).all()
        h = planner.explain_batch(1, C, N, cont, after, reason, 1 << NOFIT, [ign])
        assert h[0, ER.HIST_FITS] == 0 and h[0, 7] == nofit.size
        assert np.array_equal(h[0], ER.hist(ER.rows(cont, after, sel=nofit, ignore=ign)))


def test_skew_rejections_under_a_spread(planner):
    """With a spread constraint a SKEW container had a node that fits when its turn came, so it has one on
    the pristine table.  On the table the call left it still has one (FEASIBLE > 0) unless later containers
    took the capacity: then every node that fitted it has a changed cpu_free, mem_free or conflict_used."""
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    dom = (np.arange(N) % 3).astype(np.uint32)
    seen = 0
    for strategy in range(4):
        a, r, after, _ = planner.place_policy(cont, nodes, strategy, domain=dom, max_skew=1)
        skew = np.flatnonzero(r == SKEW)
        seen += skew.size
        before, rows = planner.explain(cont, nodes, sel=skew), planner.explain(cont, after, sel=skew)
        assert (before[:, ER.FEASIBLE] > 0).all()
        changed = (after[0] != nodes[0]) | (after[1] != nodes[1]) | (after[3] != nodes[3])
        for i, c in enumerate(skew):
            assert rows[i, ER.FEASIBLE] > 0 or changed[ER.why(c, cont, nodes) == 0].all()
        h = planner.explain_batch(1, C, N, cont, after, r, 1 << SKEW)
        assert h[0, ER.HIST_FITS] == (rows[:, ER.FEASIBLE] > 0).sum() and h[0, 7] == skew.size
    assert seen >= 4


def test_errors_write_nothing(planner):
    import torch
    from fleetflow_amd import _lib
    from fleetflow_amd._lib import FP_ECORRUPT, FP_EINVAL, FleetplaceError, FpContainers, FpNodes
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    snap = [np.array(a) for a in (*cont, *nodes)]
    sel = np.arange(70, dtype=np.uint32)
    sel[69] = C
    with pytest.raises(FleetplaceError) as e:
        planner.explain(cont, nodes, sel=sel)
    assert e.value.code == FP_EINVAL
    # the host entry through ctypes on a buffer with a fill pattern
    L = _lib.load()
    rows = np.full((70, 16), 0xABCDEF01, np.uint32)
    arrs = [np.ascontiguousarray(a) for a in (*cont, *nodes)]
    cs = FpContainers(C, *(x.ctypes.data for x in arrs[:4]))
    ns = FpNodes(N, *(x.ctypes.data for x in arrs[4:]))
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    assert L.fp_explain(planner._ctx, ct.byref(cs), ct.byref(ns), p32(sel), 70, 0, p32(rows)) == FP_EINVAL
    assert (rows == 0xABCDEF01).all()
    sel[69] = C - 1
    assert L.fp_explain(planner._ctx, ct.byref(cs), ct.byref(ns), p32(sel), 70, 0, p32(rows)) == 0
    assert np.array_equal(rows, K.expected(C, N)[sel])  # the same call with a legal index does write
    # the device entry: found on the device, reported by sync() once, no row written
    b = dict(S=1, C=C, N=N, cont=cont)
    db = _dev_batch(b, nodes)
    sel[69] = C
    rows_t = torch.full((70 * 16,), -3, dtype=torch.int32, device="cuda:0")
    planner.dev_explain(db, rows_t, sel_t=_t32(sel))
    with pytest.raises(FleetplaceError) as e:
        planner.sync()
    assert e.value.code == FP_ECORRUPT
    assert bool((rows_t == -3).all())
    planner.sync()  # reported once
    # the context still works
    sel[69] = 5
    rows_t = torch.full((70 * 16,), -3, dtype=torch.int32, device="cuda:0")
    planner.dev_explain(db, rows_t, sel_t=_t32(sel))
    planner.sync()
    assert np.array_equal(_u32(rows_t).reshape(70, 16), K.expected(C, N)[sel])
    assert np.array_equal(planner.explain(cont, nodes), K.expected(C, N))
    assert all(np.array_equal(a, b_) for a, b_ in zip(snap, (*cont, *nodes)))
    # an S above the grid limit, and a sel beyond C on a split call (N = 1025): nothing written either
    with pytest.raises(FleetplaceError) as e:
        planner.explain_batch(65536, 0, 0, [np.zeros(0, np.uint32)] * 4, [np.zeros(0, np.uint32)] * 4 + [np.zeros(0, np.uint8)],
                              None, 0)
    assert e.value.code == _lib.FP_EOVERFLOW
    cont2, nodes2 = K.crafted(65, 1025)
    db2 = _dev_batch(dict(S=1, C=65, N=1025, cont=cont2), nodes2)
    rows_t = torch.full((70 * 16,), -3, dtype=torch.int32, device="cuda:0")
    bad = np.full(70, 3, np.uint32)
    bad[0] = 65
    planner.dev_explain(db2, rows_t, sel_t=_t32(bad))
    with pytest.raises(FleetplaceError) as e:
        planner.sync()
    assert e.value.code == FP_ECORRUPT and bool((rows_t == -3).all())


def test_between_other_calls(planner, O):
    """The context's workspace is shared: a levelize and a place_batch before and after explain calls give
    the same results, and so do the explain calls."""
    C, N = 300, 65
    b = K.batch_case(3)
    row_ptr, col, has_deps = O.gen_dag(5, 20, 10, 4, 30, 2)
    lv0 = planner.levelize(row_ptr, col, has_deps)
    pb0 = planner.place_batch(3, C, N, b["cont"], b["nodes"], level=b["level"])
    path0 = planner.place_path()
    rows = planner.explain(b["scen"][1][0], b["scen"][1][1], sel=np.arange(C - 1, -1, -1))
    hist = planner.explain_batch(3, C, N, b["cont"], pb0[3], pb0[1], 1 << NOFIT)
    assert np.array_equal(rows, K.expected(C, N, seed=1)[::-1])
    assert (hist[:, ER.HIST_FITS] == 0).all() and np.array_equal(hist[:, 7], (pb0[1].reshape(3, C) == NOFIT).sum(axis=1))
    assert path0["ran"] and not planner.place_path()["ran"]  # the arena was reset: nothing stale is reported
    lv1 = planner.levelize(row_ptr, col, has_deps)
    pb1 = planner.place_batch(3, C, N, b["cont"], b["nodes"], level=b["level"])
    assert all(np.array_equal(x, y) for x, y in zip(lv0[:2], lv1[:2])) and lv0[2] == lv1[2]
    assert all(np.array_equal(x, y) for x, y in zip(pb0[:3], pb1[:3]))
    assert all(np.array_equal(x, y) for x, y in zip(pb0[3], pb1[3]))
    assert planner.place_path() == path0
    assert np.array_equal(planner.explain_batch(3, C, N, b["cont"], pb1[3], pb1[1], 1 << NOFIT), hist)


def test_plan_stage_from_kdl_explains_the_rejection(planner):
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    flow = parse_kdl_string(STAGE_KDL % "")
    base = plan_stage(flow, "live", planner)
    plan = plan_stage(flow, "live", planner, explain=True)
    assert plan.rejected == {"infer": "NOFIT"} and set(plan.why) == {"infer"}
    w = plan.why["infer"]
    # train took g0's cpu: g0 is one cause (CPU) away; c0 and c1 lack class=gpu (c1 region=tokyo too: still LABEL alone)
    assert w.fail == {"CORDON": 0, "CPU": 1, "MEM": 0, "LABEL": 2, "CONFLICT": 0}
    assert w.only["CPU"] == 1 and w.only["LABEL"] == 2
    assert (w.universal, w.missing_labels, w.nearest, w.feasible, w.servers) == ([], [], "g0", 0, 3)
    out = format_up_dry_run(flow, "live", plan)
    assert "    配置先: (配置不可: NOFIT)\n    配置不可の理由: CPU 1/3 台, LABEL 2/3 台 (最も近い: g0)\n" in out
    assert plan_from_json(plan_to_json(plan)) == plan
    # explain=False: the plan and the text of today
    assert base.why == {} and "配置不可の理由" not in format_up_dry_run(flow, "live", base)
    plan.why = {}
    assert plan == base and format_up_dry_run(flow, "live", plan) == format_up_dry_run(flow, "live", base)
    assert "why" not in plan_to_json(base)
    # under a policy with a chain that gives class up, infer is placed: nothing to explain
    relaxed = plan_stage(parse_kdl_string(STAGE_KDL % 'placement { fallback "class" }'), "live", planner, explain=True)
    assert relaxed.rejected == {} and relaxed.why == {}
    # a chain that does not help (region): the diagnosis ignores the region bits, so only class=gpu blocks on c0, c1
    flow2 = parse_kdl_string(STAGE_KDL % 'placement { fallback "region" }')
    p2 = plan_stage(flow2, "live", planner, explain=True)
    assert p2.rejected == {"infer": "NOFIT"} and p2.why["infer"].fail == w.fail and p2.why["infer"].only == w.only
