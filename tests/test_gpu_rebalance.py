"""GPU tests of the rebalance sweep (SPEC.md 2.19; k_rebal_sweep<BLK, K, FB> in fleetflow_amd/csrc/fp_rebalance.hip):
both entry points against the numpy reference (tests/rebalance_ref.py), which makes one policy_fallback_ref.place
call per attempt.  Every comparison is exact: assign_out, hops, reasons and every word of every summary row."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import rebalance_cases as T  # noqa: E402
import rebalance_ref as RR  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
PREF2 = (1 << 0) | (1 << 2)
RELAX = (1, 2)
MAX_SKEW = 2
NAMES = ("assign_out", "hops", "reason", "summary")


def _check(got, exp):
    for g, e, what in zip(got, exp, NAMES):
        assert g.shape == e.shape and g.dtype == e.dtype, what
        assert np.array_equal(g, e), what


def _both(planner, cont, nodes, assign, victim_order, strategy=0, preferred=0, node_count=None, **kw):
    got = planner.rebalance_sweep(cont, nodes, assign, victim_order, strategy, preferred, node_count, **kw)
    _check(got, RR.sweep(cont, nodes, assign, victim_order, strategy, preferred, node_count, **kw))
    return got


@functools.lru_cache(maxsize=None)
def _case(seed, n_dom=4, C=300, N=40):
    return RR.random_case(seed, C=C, N=N, n_dom=n_dom, max_skew=MAX_SKEW, relax_mask=RELAX)[:5]


@functools.lru_cache(maxsize=None)
def _orders(seed, n_dom=4, C=300, N=40):
    """The three rules of the flow layer on a case, each twice over, so that a rejected victim is tried again."""
    cont = _case(seed, n_dom, C, N)[0]
    res = tuple(np.concatenate([RR.order_of(rule, cont)] * 2) for rule in RR.ORDERS)
    for o in res:
        o.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _embedded(seed, N, n_dom=4):
    """A live fleet of ``_case`` (40 servers, 128 for more than four domains) spread over N node indices (0 and
    N - 1 among them); every other server is cordoned, full and empty, in domain 63.  A fleet of at most N servers
    is the case itself."""
    n0 = 40 if n_dom <= 4 else 128
    if N <= n0:
        return _case(seed, n_dom, N=N)
    cont, live, assign, cnt, dom = _case(seed, n_dom, N=n0)
    pos = np.unique(np.linspace(0, N - 1, n0).astype(np.int64))
    assert pos.size == n0 and pos[0] == 0 and pos[-1] == N - 1

    def wide(x, fill=0):
        out = np.full(N, fill, x.dtype)
        out[pos] = x
        return out
    nodes = tuple(wide(x) for x in live)
    assign_w = np.where(assign == NONE, NONE, pos[np.where(assign == NONE, 0, assign)]).astype(np.uint32)
    res = (cont, nodes, assign_w, wide(cnt), wide(dom, 63))
    for a in (*nodes, *res[2:]):
        a.setflags(write=False)
    return res


# ---- geometry: 64 x 1 and 1024 x {1, 2, 4, 8}, on both sides of every switch, with and without the chain --------
@pytest.mark.parametrize("n_dom", [1, 2, 63, 64])
@pytest.mark.parametrize("N", [1, 64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 8192])
def test_every_block_geometry(N, n_dom, planner):
    cont, nodes, assign, cnt, dom = _embedded(4, N, n_dom)
    assert n_dom < 64 or N < 64 or 63 in dom
    strategy = (N + n_dom) % 4
    order = np.concatenate([RR.order_of("smallest", cont)] * 2)
    vo = np.stack([order, order[::-1]])
    for relax in ((), RELAX):
        got = _both(planner, cont, nodes, assign, vo, strategy, 0, cnt, domain=dom, max_skew=MAX_SKEW, relax_mask=relax)
        if n_dom > 1 and N >= 64:
            assert got[3][:, RR.MOVES].min() > 0, "not vacuous"
            assert N < 1024 or (got[0] == N - 1).any() or (assign == N - 1).any()  # the last slot row is in play


# ---- with and without the chain, all four strategies, preferred labels -------------------------------------------
@pytest.mark.parametrize("relax", [(), RELAX, (4, 1, 2, 0)])
@pytest.mark.parametrize("pref", [0, PREF2])
@pytest.mark.parametrize("strategy", list(R.STRATEGIES))
def test_chain_strategies_and_preferred(strategy, pref, relax, planner):
    cont, live, assign, cnt, dom = _case(1 + strategy)
    got = _both(planner, cont, live, assign, np.stack(_orders(1 + strategy)), strategy, pref, cnt, domain=dom,
                max_skew=MAX_SKEW, relax_mask=relax)
    assert got[3][:, RR.MOVES].min() > 0
    if relax == RELAX:
        assert got[3][:, RR.RELAXED].max() > 0 and got[1].max() > 0


# ---- order lengths round the 64-entry chunk ----------------------------------------------------------------------
@pytest.mark.parametrize("n_try", [1, 63, 64, 65, 129])
def test_order_lengths_at_the_chunk_boundaries(n_try, planner):
    cont, live, assign, cnt, dom = _case(5)
    # the victims of a full pass, so that a short order is all attempts
    full = RR.variant(cont, live, assign, _orders(5)[0], NONE, R.SPREAD, 0, cnt, dom, MAX_SKEW, RELAX)
    hot = np.array([t[1] for t in full[4]], np.uint32)
    assert hot.size >= 129
    vo = np.stack([hot[:n_try], hot[::-1][:n_try], _orders(5)[2][:n_try]])
    got = _both(planner, cont, live, assign, vo, R.SPREAD, 0, cnt, domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    assert got[3][0, RR.MOVES] + got[3][0, RR.STUCK] == n_try


# ---- ragged rows, 1 and 33 variants, budgets of 0, 1 and NONE and a mixed array of them --------------------------
@pytest.mark.parametrize("n_var", [1, 33])
def test_ragged_rows_variants_and_budgets(n_var, planner):
    cont, live, assign, cnt, dom = _case(6)
    rng = np.random.default_rng(n_var)
    rows = []
    for v in range(n_var):
        o = _orders(6)[v % 3][:int(rng.integers(40, 400))].copy()
        o[rng.random(o.size) < 0.2] = NONE  # holes
        rows.append(np.roll(o, v))
    vo = RR.pad(rows)
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    for budgets in ([0] * n_var, [1] * n_var, [NONE] * n_var, [(0, 1, NONE, 5, 17)[v % 5] for v in range(n_var)], None):
        got = _both(planner, cont, live, assign, vo, R.PACK, 0, cnt, max_moves=budgets, **kw)
        if budgets is not None:
            assert (got[3][:, RR.MOVES] <= np.array(budgets, np.uint32)).all()
    assert (got[3][:, RR.MOVES] > 5).any()


# ---- node_count given and absent ---------------------------------------------------------------------------------
def test_node_count_given_absent_and_charged(planner):
    cont, live, assign, cnt, dom = _case(7)
    vo = np.stack(_orders(7))
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    given = _both(planner, cont, live, assign, vo, R.SPREAD, 0, cnt, **kw)
    absent = _both(planner, cont, live, assign, vo, R.SPREAD, 0, None, **kw)  # derived, not zero
    assert np.array_equal(cnt, RR.derived_count(assign, 40))
    _check(given, absent)
    assert absent[3][:, RR.SKEW_BEFORE].min() > MAX_SKEW
    charged = cnt + (np.arange(40) % 5 == 1).astype(np.uint32) * 9  # other tables' services in domain 1
    other = _both(planner, cont, live, assign, vo, R.SPREAD, 0, charged, **kw)
    assert not np.array_equal(other[0], given[0])


# ---- the degenerate form ------------------------------------------------------------------------------------------
def test_without_a_constraint_nothing_moves(planner):
    cont, live, assign, cnt, dom = _case(7)
    vo = np.stack(_orders(7))
    for kw in (dict(domain=None, max_skew=2), dict(domain=np.full(40, 99, np.uint32), max_skew=0)):  # domain is not read
        got = _both(planner, cont, live, assign, vo, R.SPREAD, 0, cnt, relax_mask=RELAX, **kw)
        assert (got[0] == assign).all() and not got[1].any() and not got[2].any() and not got[3].any()


# ---- theorems E and F on the device ------------------------------------------------------------------------------
def test_theorem_e_independence_and_holes(planner):
    cont, live, assign, cnt, dom = _case(8)
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    rows = list(_orders(8))
    holes = np.insert(rows[0], [0, 5, 5, 63, 64, 200], NONE)
    vo = RR.pad(rows + [holes])
    budgets = [NONE, 3, NONE, NONE]
    got = planner.rebalance_sweep(cont, live, assign, vo, R.FILL_LOWEST, 0, cnt, max_moves=budgets, **kw)
    for v in range(4):
        one = planner.rebalance_sweep(cont, live, assign, vo[v:v + 1], R.FILL_LOWEST, 0, cnt, max_moves=budgets[v:v + 1], **kw)
        for g, o in zip(got, one):
            assert np.array_equal(g[v], o[0])
    for g in got:
        assert np.array_equal(g[3], g[0])  # FP_NONE entries change nothing


def test_theorem_f_budget_prefix(planner):
    cont, live, assign, cnt, dom = _case(10)
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    order = _orders(10)[1]
    full = RR.variant(cont, live, assign, order, NONE, R.SPREAD, 0, cnt, dom, MAX_SKEW, RELAX)
    moves = [t for t in full[4] if t[3] == "MOVE"]
    assert len(moves) >= 8 and any(t[3] != "MOVE" for t in full[4])
    budgets = [0, 1, 2, 3, len(moves) // 2, len(moves) - 1, len(moves), len(moves) + 1]
    got = _both(planner, cont, live, assign, np.stack([order] * len(budgets)), R.SPREAD, 0, cnt, max_moves=budgets, **kw)
    for k, b in enumerate(budgets):
        cut = moves[:b]
        exp = np.array(assign)
        for _, c, _, _, t, _ in cut:
            exp[c] = t
        assert np.array_equal(got[0][k], exp)
        assert got[3][k, RR.MOVES] == len(cut)
        # cut right after its b-th move: the rejections counted are those in front of it (all, if it never gets there)
        end = 0 if b == 0 else cut[-1][0] if b <= len(moves) else len(order)
        assert got[3][k, RR.STUCK] == sum(1 for t in full[4] if t[3] != "MOVE" and t[0] < end)


# ---- the traps ------------------------------------------------------------------------------------------------------
def _padded(kw, N):
    """A trap with cordoned, full, empty servers of domain 63 appended up to N nodes: they change nothing."""
    n0 = len(kw["domain"])
    if N <= n0:
        return kw
    cf, mf, lab, cu, sched = kw["nodes"]
    z32, z8 = np.zeros(N - n0, np.uint32), np.zeros(N - n0, np.uint8)
    nodes = tuple(np.concatenate([x, z32]) for x in (cf, mf, lab, cu)) + (np.concatenate([sched, z8]),)
    out = dict(kw, nodes=nodes, domain=list(kw["domain"]) + [63] * (N - n0))
    if kw["node_count"] is not None:
        out["node_count"] = list(kw["node_count"]) + [0] * (N - n0)
    return out


@pytest.mark.parametrize("N", [0, 70, 1030])
@pytest.mark.parametrize("i", range(len(T.traps())))
def test_traps(i, N, planner):
    name, kw, exp = T.traps()[i]
    kw = _padded(kw, N)
    got = planner.rebalance_sweep(**kw)
    assert got[0][0].tolist() == exp["out"] and got[1][0].tolist() == exp["hops"], name
    assert got[2][0].tolist() == exp["reason"] and got[3][0].tolist() == exp["summary"], name
    _check(got, RR.sweep(**kw))


# ---- theorem D: one attempt is one fp_place_policy_fallback call with C = 1 on the lifted table ------------------
@pytest.mark.parametrize("strategy", list(R.STRATEGIES))
def test_one_attempt_against_place_policy_fallback(strategy, planner):
    cont, live, assign, cnt, dom = _case(10)
    hot = np.flatnonzero(RR.heavy(cnt, dom, live[4], MAX_SKEW)[dom[np.where(assign == NONE, 0, assign)]] & (assign != NONE))
    victims = hot[:: max(1, hot.size // 24)][:24].astype(np.uint32)
    got = planner.rebalance_sweep(cont, live, assign, victims[:, None], strategy, PREF2, cnt, domain=dom, max_skew=MAX_SKEW,
                                  relax_mask=RELAX)
    seen = set()
    for v, c in enumerate(victims.tolist()):
        s = int(assign[c])
        cf, mf, lab, cu, sched = (np.array(x) for x in live)
        cf[s] += cont[0][c]
        mf[s] += cont[1][c]
        cu[s] &= ~cont[3][c]
        lifted = np.array(cnt)
        lifted[s] -= 1
        a, r, h, _, _ = planner.place_policy_fallback(tuple(x[c:c + 1] for x in cont), (cf, mf, lab, cu, sched), strategy,
                                                      RELAX, PREF2, None, lifted, domain=dom, max_skew=MAX_SKEW)
        exp = np.array(assign)
        if a[0] != NONE:
            exp[c] = a[0]
        assert np.array_equal(got[0][v], exp) and got[1][v][c] == h[0] and got[2][v][c] == r[0]
        assert got[3][v, RR.MOVES] == int(a[0] != NONE) and got[3][v, RR.STUCK] == int(a[0] == NONE)
        seen.add(int(r[0]))
    assert 0 in seen


# ---- the device entry ------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
    return t.to("cuda:0")


FILL32 = 0xA5A5A5A5 - (1 << 32)
ALL_OUT = ("hops", "reason")


def _dev_call(planner, cont, nodes, assign, victim_order, strategy=0, preferred=0, node_count=None, domain=None,
              max_skew=0, relax_mask=(), max_moves=None, want=ALL_OUT):
    """dev_rebalance_sweep on copies of the inputs; returns (the call's tensors, the outputs in the order of
    Planner.rebalance_sweep's result).  The outputs start filled with 0xA5 bytes; those not in ``want`` are NULL."""
    import torch
    vo = np.asarray(victim_order, np.uint32)
    C, V = len(assign), vo.shape[0]
    ins = ([_dev(np.asarray(x, np.uint32)) for x in cont],
           [_dev(np.asarray(x, np.uint32)) for x in nodes[:4]] + [_dev(np.asarray(nodes[4], np.uint8))],
           _dev(np.asarray(assign, np.uint32)), _dev(vo.reshape(-1)),
           None if node_count is None else _dev(np.asarray(node_count, np.uint32)),
           None if domain is None else _dev(np.asarray(domain, np.uint32)),
           None if max_moves is None else _dev(np.asarray(max_moves, np.uint32)))
    w32 = lambda n: torch.full((n,), FILL32, dtype=torch.int32, device="cuda:0")  # noqa: E731
    w8 = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    out, rows = w32(V * C), w32(V * 8)
    hops = w8(V * C) if "hops" in want else None
    why = w8(V * C) if "reason" in want else None
    planner.dev_rebalance_sweep(tuple(ins[0]), tuple(ins[1]), ins[2], ins[3], V, out, rows, strategy, preferred, ins[4],
                                domain_t=ins[5], max_skew=max_skew, relax_mask=relax_mask, max_moves_t=ins[6], hops_t=hops,
                                reason_t=why)
    return ins, (out, hops, why, rows)


def _np_out(outs, V, C):
    res = []
    for t, shape in zip(outs, ((V, C), (V, C), (V, C), (V, 8))):
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        res.append((a.view(np.uint32) if a.dtype == np.int32 else a).reshape(shape))
    return tuple(res)


def _untouched(outs):
    return all((t is None) or bool((t.cpu().numpy().view(np.uint8) == 0xA5).all()) for t in outs)


def test_device_entry_a_levelize_between_two_sweeps_and_a_placement_after(planner):
    from oracle import oracle as O
    cont, nodes, assign, cnt, dom = _embedded(3, 1025)
    order = np.concatenate([RR.order_of("largest", cont)] * 2)
    vo = np.stack([order, order[::-1], np.roll(order, 7)])
    budgets = [NONE, 4, NONE]
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX, max_moves=budgets)
    ins, outs = _dev_call(planner, cont, nodes, assign, vo, R.SPREAD, PREF2, cnt, **kw)
    rp, col, hd = O.gen_dag(0x5EED0005, 20, 10, 5, 40, 3)
    level, lorder, ncyc = planner.levelize(rp, col, hd)  # the sweep's workspace is recycled under it
    el, eo, en = O.levelize(rp, col, hd)
    assert np.array_equal(level, el) and np.array_equal(lorder, eo) and ncyc == en
    _, outs2 = _dev_call(planner, cont, nodes, assign, vo, R.SPREAD, PREF2, None, **kw)
    pc, pn = O.gen_scenario(0x5EED0011, 9, 300, 40, 7)
    ea, er, _, _ = O.place(pc, pn)
    a, r, _, _ = planner.place_batch(1, 300, 40, pc, pn)
    assert np.array_equal(a, ea) and np.array_equal(r, er)
    planner.sync()
    exp = RR.sweep(cont, nodes, assign, vo, R.SPREAD, PREF2, cnt, **kw)
    assert exp[3][:, RR.MOVES].tolist()[1] == 4 and exp[3][0, RR.MOVES] > 4
    _check(_np_out(outs, 3, 300), exp)
    _check(_np_out(outs2, 3, 300), exp)  # the counts derived on the device are the counts given
    for t, a in zip([*ins[0], *ins[1], ins[2], ins[3], ins[4], ins[5]], (*cont, *nodes, assign, vo, cnt, dom)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    _check(planner.rebalance_sweep(cont, nodes, assign, vo, R.SPREAD, PREF2, cnt, **kw), exp)


@pytest.mark.parametrize("relax", [(), RELAX])
def test_each_nullable_output_as_null(relax, planner):
    cont, live, assign, cnt, dom = _case(3)
    vo = np.stack(_orders(3)[:2])
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=relax)
    exp = RR.sweep(cont, live, assign, vo, R.PACK, 0, cnt, **kw)
    for want in (ALL_OUT, ("hops",), ("reason",), ()):
        _, outs = _dev_call(planner, cont, live, assign, vo, R.PACK, 0, cnt, want=want, **kw)
        planner.sync()
        got = _np_out(outs, 2, 300)
        assert [g is None for g in got] == [False, "hops" not in want, "reason" not in want, False]
        for g, e, what in zip(got, exp, NAMES):
            assert g is None or np.array_equal(g, e), (what, want)
        host = planner.rebalance_sweep(cont, live, assign, vo, R.PACK, 0, cnt, want_hops="hops" in want,
                                       want_reason="reason" in want, **kw)
        for g, e in zip(host, exp):
            assert g is None or np.array_equal(g, e)
        assert (host[1] is None) == ("hops" not in want) and (host[2] is None) == ("reason" not in want)
    # and without a constraint
    _, outs = _dev_call(planner, cont, live, assign, vo, R.PACK, 0, cnt, want=(), relax_mask=relax)
    planner.sync()
    got = _np_out(outs, 2, 300)
    assert (got[0] == assign).all() and not got[3].any()


# ---- errors: nothing is written -----------------------------------------------------------------------------------
def _raw_host(planner, cont, nodes, assign, victim_order, strategy=0, alias=False, n_var=None, domain=None, max_skew=0,
              n_hops=0, null=None):
    """fp_rebalance_sweep itself, on outputs pre-filled with 0xA5: (rc, outputs untouched?)."""
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)  # noqa: E731
    cont, assign, vo = tuple(u32(x) for x in cont), u32(assign).copy(), u32(victim_order)
    nodes = tuple(u32(x) for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8),)
    C, N = assign.size, nodes[0].size
    V, T_ = (vo.shape if n_var is None else (n_var, 0))
    rows_v = min(V, 4)  # an n_var the call refuses is never written for
    out = assign if alias else np.full(rows_v * C, 0xA5A5A5A5, np.uint32)
    rows = np.full(rows_v * 8, 0xA5A5A5A5, np.uint32)
    hops, why = np.full(rows_v * C, 0xA5, np.uint8), np.full(rows_v * C, 0xA5, np.uint8)
    keep = out.copy()
    dom = None if domain is None else u32(domain)
    relax = u32([1, 2, 4, 8, 16])
    cs = _lib.FpContainers(C, *(x.ctypes.data for x in cont))
    ns = _lib.FpNodes(N, *(x.ctypes.data for x in nodes))
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    args = dict(assign=p(assign, _lib.u32p), victim=p(vo, _lib.u32p), out=p(out, _lib.u32p), rows=p(rows, _lib.u32p))
    if null:
        args[null] = None
    rc = planner._L.fp_rebalance_sweep(planner._ctx, ct.byref(cs), ct.byref(ns), args["assign"], args["victim"], V, T_, None,
                                       strategy, 0, None, p(dom, _lib.u32p), max_skew, p(relax, _lib.u32p), n_hops,
                                       args["out"], p(hops, _lib.u8p), p(why, _lib.u8p), args["rows"])
    untouched = (np.array_equal(out, keep) and (rows == 0xA5A5A5A5).all() and (hops == 0xA5).all() and (why == 0xA5).all())
    return rc, bool(untouched)


def _bad_cases():
    cont, nodes, assign, cnt, dom = _embedded(2, 65)
    order = np.concatenate([RR.order_of("smallest", cont)] * 2)
    vo = np.stack([order, order[::-1]])
    bad_vic, last_vic, bad_assign, last_assign = vo.copy(), vo.copy(), assign.copy(), assign.copy()
    bad_vic[0, 0] = 300
    last_vic[1, -1] = 0xFFFFFFFE
    bad_assign[0] = 65
    last_assign[299] = 0xFFFFFFFE
    bad_dom, last_dom = dom.copy(), dom.copy()
    bad_dom[0] = 64
    last_dom[64] = 0xFFFFFFFF
    big = tuple(np.resize(x, 8193) for x in nodes)
    ok = dict(nodes=nodes, assign=assign, victim_order=vo, domain=dom, max_skew=2, n_hops=2)
    return cont, ok, [
        ("strategy", _lib.FP_EINVAL, dict(ok, strategy=4)),
        ("n_hops", _lib.FP_EINVAL, dict(ok, n_hops=5)),
        ("nodes", _lib.FP_EOVERFLOW, dict(ok, nodes=big, domain=np.resize(dom, 8193))),
        ("n_var", _lib.FP_EOVERFLOW, dict(ok, victim_order=vo[:, :0], n_var=65536)),
        ("victim_order", _lib.FP_EINVAL, dict(ok, victim_order=bad_vic)),
        ("victim_order, last", _lib.FP_EINVAL, dict(ok, victim_order=last_vic)),
        ("assign", _lib.FP_EINVAL, dict(ok, assign=bad_assign)),
        ("assign, last", _lib.FP_EINVAL, dict(ok, assign=last_assign)),
        ("domain", _lib.FP_EINVAL, dict(ok, domain=bad_dom)),
        ("domain, last", _lib.FP_EINVAL, dict(ok, domain=last_dom)),
    ]


def test_host_entry_errors_write_nothing(planner):
    cont, ok, cases = _bad_cases()
    for name, code, kw in cases:
        assert _raw_host(planner, cont, **kw) == (code, True), name
    for null in ("assign", "victim", "out", "rows"):  # a required pointer that is null
        assert _raw_host(planner, cont, **dict(ok, null=null)) == (_lib.FP_EINVAL, True), null
    assert _raw_host(planner, cont, **dict(ok, victim_order=ok["victim_order"][:1], alias=True)) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, cont, **dict(ok, n_var=0)) == (_lib.FP_OK, True)  # no variant: nothing to write
    # a domain id of 64 or more is nothing wrong without a constraint: domain is not read
    assert _raw_host(planner, cont, **dict(cases[8][2], max_skew=0)) == (_lib.FP_OK, False)
    assert _raw_host(planner, cont, **ok) == (_lib.FP_OK, False)  # and the same call is fine
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.rebalance_sweep(cont, ok["nodes"], ok["assign"], ok["victim_order"], domain=cases[8][2]["domain"], max_skew=1)
    assert e.value.code == _lib.FP_EINVAL


def test_device_entry_errors_write_nothing_and_the_context_goes_on(planner):
    import torch
    cont, ok, cases = _bad_cases()
    kw0 = dict(domain=ok["domain"], max_skew=2, relax_mask=RELAX)
    for name, code, kw in cases:
        if not name.startswith(("victim_order", "assign", "domain")):
            continue  # returned directly, below
        # found on the device: the call returns, sync() reports FP_EINVAL
        _, outs = _dev_call(planner, cont, kw["nodes"], kw["assign"], kw["victim_order"], 0, 0, None, kw["domain"], 2, RELAX)
        with pytest.raises(_lib.FleetplaceError) as e:
            planner.sync()
        assert e.value.code == code, name
        assert _untouched(outs), name
        planner.sync()  # reported once, then clear
    # returned directly, before anything is read or launched: every array is a few device words of 0xA5
    word = lambda: torch.full((64,), FILL32, dtype=torch.int32, device="cuda:0")  # noqa: E731
    for C, N, n_var, strategy, n_hops, null, code in (
            (8, 8, 1, 0, 5, None, _lib.FP_EINVAL), (8, 8, 1, 4, 0, None, _lib.FP_EINVAL),
            (8, 8193, 1, 0, 0, None, _lib.FP_EOVERFLOW), (8, 8, 65536, 0, 0, None, _lib.FP_EOVERFLOW),
            (8, 8, 1, 0, 0, 0, _lib.FP_EINVAL), (8, 8, 1, 0, 0, 3, _lib.FP_EINVAL), (8, 8, 1, 0, 0, "alias", _lib.FP_EINVAL)):
        ins, outs = [word() for _ in range(12)], [word() for _ in range(4)]
        relax = np.array([1, 2, 4, 8, 16], np.uint32)
        cs = _lib.FpContainers(C, *(t.data_ptr() for t in ins[:4]))
        ns = _lib.FpNodes(N, *(t.data_ptr() for t in ins[4:9]))
        ptrs = [t.data_ptr() for t in outs]
        if null == "alias":
            ptrs[0] = ins[9].data_ptr()
        elif null is not None:
            ptrs[null] = None
        rc = planner._L.fp_dev_rebalance_sweep(planner._ctx, ct.byref(cs), ct.byref(ns), ins[9].data_ptr(),
                                               ins[10].data_ptr(), n_var, 2, None, strategy, 0, None, ins[11].data_ptr(), 1,
                                               relax.ctypes.data_as(_lib.u32p), n_hops, *ptrs)
        torch.cuda.synchronize()
        assert rc == code and all(bool((t.cpu().numpy().view(np.uint8) == 0xA5).all()) for t in ins + outs)
    planner.sync()  # and nothing is pending
    _, outs = _dev_call(planner, cont, ok["nodes"], ok["assign"], ok["victim_order"], 3, 0, None, **kw0)
    planner.sync()
    _check(_np_out(outs, 2, 300), RR.sweep(cont, ok["nodes"], ok["assign"], ok["victim_order"], 3, **kw0))


def test_no_entries_no_containers_no_nodes(planner):
    cont, live, assign, cnt, dom = _case(2)
    kw = dict(domain=dom, max_skew=MAX_SKEW, relax_mask=RELAX)
    got = _both(planner, cont, live, assign, np.zeros((3, 0), np.uint32), R.SPREAD, 0, cnt, **kw)
    assert (got[0] == assign).all() and (got[3][:, RR.SKEW_BEFORE] == got[3][:, RR.SKEW_AFTER]).all()
    none = tuple(np.zeros(0, np.uint32) for _ in range(4))
    got = _both(planner, none, live, np.zeros(0, np.uint32), np.full((2, 3), NONE, np.uint32), R.SPREAD, 0, cnt, **kw)
    assert got[0].shape == (2, 0) and (got[3][:, RR.SKEW_BEFORE] == RR.skew(cnt, dom, live[4])).all()
    nonodes = tuple(np.zeros(0, np.uint32) for _ in range(4)) + (np.zeros(0, np.uint8),)
    got = _both(planner, cont, nonodes, np.full(300, NONE, np.uint32), np.stack(_orders(2)), R.SPREAD, 0, None,
                domain=np.zeros(0, np.uint32), max_skew=1, relax_mask=())
    assert (got[0] == NONE).all() and not got[3].any()


# ---- the flow-level path ------------------------------------------------------------------------------------------
def test_rebalance_stage_from_kdl(planner):
    from test_rebalance_host import check_rebalance_stage
    check_rebalance_stage(planner)
