"""Every host-pointer entry point through a growing staging arena and workspace: a fresh context, then three calls
in a row -- a small shape, a shape that needs more than the first one's capacity after its 25 % + 4096 bytes of
headroom (both arenas are freed and allocated again), and the small shape once more in the larger, dirty arenas.
Each call is compared for exact equality with the oracle or with the tests/*_ref.py reference the entry's own test
file uses.  The shapes are the smallest that do this with a 1024-thread placer block (N > 64) and more than one
64-record chunk: S = 2, C = 70, N = 9, then S = 3, C = 3000, N = 700 (single-scenario entries drop S; the graph
entries use V = 70 / 3000)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import explain_ref as ER  # noqa: E402
import policy_fallback_cases as K  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_quota_ref as QR  # noqa: E402
import policy_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 0x5EED0011
SHAPES = [(2, 70, 9), (3, 3000, 700), (2, 70, 9)]
BASE = 40  # scen_base of the batch calls
PREF = (1 << 4) | (1 << 8)
RELAX = K.RELAX[2]


@pytest.fixture
def fresh():
    from fleetflow_amd import Planner
    p = Planner(0)
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def _scen(s, C, N):
    from oracle import oracle as O
    return O.gen_scenario(SEED, s, C, N, 7)


def _cat(parts, n):
    return [np.concatenate([p[i] for p in parts]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _batch(S, C, N):
    conts, nodes = zip(*[_scen(BASE + s, C, N) for s in range(S)])
    return _cat(conts, 4), _cat(nodes, 5)


def _rows(a, s, n):
    return a[s * n:(s + 1) * n]


# ---- the graph entries ------------------------------------------------------------------------------------
GRAPHS = [(5, 6, 2, 20, 2), (50, 20, 4, 500, 3), (5, 6, 2, 20, 2)]  # V = 70, 3000, 70; two or three cycles each


def test_legacy_order_and_levelize(fresh, O):
    for g in GRAPHS:
        rp, col, hd = O.gen_dag(SEED, *g)
        assert hd.size in (70, 3000)
        assert np.array_equal(fresh.legacy_order(hd), O.legacy_order(hd))
        level, order, ncyc = fresh.levelize(rp, col, hd)
        el, eo, en = O.levelize(rp, col, hd)
        assert np.array_equal(level, el) and np.array_equal(order, eo) and ncyc == en and en > 0


# ---- first fit ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ffd(s, C, N):
    from oracle import oracle as O
    cont, nodes = _scen(s, C, N)
    a, r, after, _ = O.place(cont, nodes)
    return a, r, after, O.cost(a, N, s)


def test_place(fresh):
    for _, C, N in SHAPES:
        cont, nodes = _scen(BASE, C, N)
        assign, reason, after = fresh.place(cont, nodes)
        ea, er, eafter, _ = _ffd(BASE, C, N)
        assert np.array_equal(assign, ea) and np.array_equal(reason, er)
        for i in (0, 1, 3):
            assert np.array_equal(after[i], eafter[i])


def test_place_batch(fresh):
    for S, C, N in SHAPES:
        cont, nodes = _batch(S, C, N)
        assign, reason, cost, after = fresh.place_batch(S, C, N, cont, nodes, scen_base=BASE)
        for s in range(S):
            ea, er, eafter, ecost = _ffd(BASE + s, C, N)
            assert np.array_equal(_rows(assign, s, C), ea) and np.array_equal(_rows(reason, s, C), er)
            assert int(cost[s]) == ecost
            for i in (0, 1, 3):
                assert np.array_equal(_rows(after[i], s, N), eafter[i])


# ---- the eight scored entries ---------------------------------------------------------------------------------
# what each export's signature has: (spread constraint, fallback chain, quota)
ENTRIES = {"policy": (False, False, False), "spread": (True, False, False), "fallback": (True, True, False),
           "quota": (True, True, True)}


@functools.lru_cache(maxsize=None)
def _policy_args(s, C, N, sp, fb, qt):
    strategy = R.STRATEGIES[s % 4] if C < 1000 else (R.SPREAD, R.PACK, R.FILL_LOWEST)[s % 3]
    kw = dict(preferred=PREF, node_count=(np.arange(N) % 3).astype(np.uint32))
    if sp:
        kw.update(domain=((np.arange(N) + s) % 5).astype(np.uint32), max_skew=2 + s % 2)
    if fb:
        kw.update(relax_mask=tuple(RELAX))
    quota = used = None
    if qt:
        # caps that bite at every shape: shares of what the scenario uses without a quota; the tenant already
        # holds something
        cont, nodes = _scen(s, C, N)
        u = QR.usage(cont, FR.place(cont, nodes, strategy, **kw)[0])
        quota, used = (u[0] * 7 // 10 + 100, u[1] * 3 // 5 + 64, u[2] * 4 // 5 + 2), (100, 64, 2)
    return strategy, kw, quota, used


@functools.lru_cache(maxsize=None)
def _scored(s, C, N, sp, fb, qt):
    """(assign, reason, hops, nodes_after, count, why, used) of scenario id s"""
    cont, nodes = _scen(s, C, N)
    strategy, kw, quota, used = _policy_args(s, C, N, sp, fb, qt)
    if qt:
        return QR.place(cont, nodes, strategy, quota, used, **kw)
    a, r, h, after, cnt = FR.place(cont, nodes, strategy, **kw)
    return a, r, h, after, cnt, None, None


def _check_scored(exp, assign, reason, hops, after, cnt, why, used, s=0, C=None, N=None):
    assert np.array_equal(_rows(assign, s, C), exp[0]) and np.array_equal(_rows(reason, s, C), exp[1])
    if hops is not None:
        assert np.array_equal(_rows(hops, s, C), exp[2])
    for i in (0, 1, 3):
        assert np.array_equal(_rows(after[i], s, N), exp[3][i])
    assert np.array_equal(_rows(cnt, s, N), exp[4])
    if why is not None:
        assert np.array_equal(_rows(why, s, C), exp[5]) and np.array_equal(_rows(used, s, 3), exp[6])


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_place_policy_single(entry, fresh):
    sp, fb, qt = ENTRIES[entry]
    for _, C, N in SHAPES:
        cont, nodes = _scen(BASE, C, N)
        strategy, kw, quota, used = _policy_args(BASE, C, N, sp, fb, qt)
        exp = _scored(BASE, C, N, sp, fb, qt)
        hops = why = qu = None
        if qt:
            assign, reason, hops, after, cnt, why, qu = fresh.place_policy_quota(cont, nodes, strategy, quota, used, **kw)
            assert (exp[1] == QR.REASON_QUOTA).any() and (exp[0] != NONE).any()  # a condition on the inputs
        elif fb:
            assign, reason, hops, after, cnt = fresh.place_policy_fallback(cont, nodes, strategy, **kw)
        else:
            assign, reason, after, cnt = fresh.place_policy(cont, nodes, strategy, **kw)
        _check_scored(exp, assign, reason, hops, after, cnt, why, qu, 0, C, N)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_place_batch_policy(entry, fresh):
    sp, fb, qt = ENTRIES[entry]
    for S, C, N in SHAPES:
        cont, nodes = _batch(S, C, N)
        per = [_policy_args(BASE + s, C, N, sp, fb, qt) for s in range(S)]
        kw = dict(preferred=[PREF] * S, node_count=np.concatenate([p[1]["node_count"] for p in per]), scen_base=BASE)
        if sp:
            kw.update(domain=np.concatenate([p[1]["domain"] for p in per]), max_skew=[p[1]["max_skew"] for p in per])
        if fb:
            kw.update(relax_mask=K.relax_rows([RELAX] * S), n_hops=[len(RELAX)] * S)
        strategy = [p[0] for p in per]
        hops = why = qu = None
        if qt:
            quota = np.array([p[2] for p in per], np.uint32).reshape(-1)
            used = np.array([p[3] for p in per], np.uint32).reshape(-1)
            assign, reason, hops, cost, after, cnt, why, qu = fresh.place_batch_policy_quota(
                S, C, N, cont, nodes, strategy, quota, used, **kw)
        elif fb:
            assign, reason, hops, cost, after, cnt = fresh.place_batch_policy_fallback(S, C, N, cont, nodes, strategy, **kw)
        else:
            assign, reason, cost, after, cnt = fresh.place_batch_policy(S, C, N, cont, nodes, strategy, **kw)
        for s in range(S):
            exp = _scored(BASE + s, C, N, sp, fb, qt)
            _check_scored(exp, assign, reason, hops, after, cnt, why, qu, s, C, N)
            assert int(cost[s]) == R.cost(exp[0], exp[1], BASE + s)


# ---- feasibility and rejection diagnosis ------------------------------------------------------------------------
def test_feasibility_with_bitmap(fresh, O):
    for _, C, N in SHAPES:
        cont, nodes = _scen(BASE, C, N)
        first, count, bm = fresh.feasibility(cont, nodes, bitmap=True)
        ef, ec, eb = O.feasibility(cont, nodes)
        assert np.array_equal(first, ef) and np.array_equal(count, ec) and np.array_equal(bm, eb)


@functools.lru_cache(maxsize=None)
def _explained(s, C, N):
    cont, _ = _scen(s, C, N)
    return ER.rows_matrix(cont, _ffd(s, C, N)[2], ignore=1 << 4)


def test_explain(fresh):
    for _, C, N in SHAPES:
        cont, _ = _scen(BASE, C, N)
        after = _ffd(BASE, C, N)[2]
        exp = _explained(BASE, C, N)
        assert np.array_equal(fresh.explain(cont, after, ignore_labels=1 << 4), exp)
        sel = np.array([C - 1, 0, C // 2, 0], np.uint32)
        assert np.array_equal(fresh.explain(cont, after, sel=sel, ignore_labels=1 << 4), exp[sel])


def test_explain_batch_with_reason_mask(fresh):
    mask = (1 << 0) | (1 << 1)  # FP_REASON_OK and FP_REASON_NOFIT: every container here, selected by its reason
    for S, C, N in SHAPES:
        cont, _ = _batch(S, C, N)
        ffd = [_ffd(BASE + s, C, N) for s in range(S)]
        after, reason = _cat([f[2] for f in ffd], 5), np.concatenate([f[1] for f in ffd])
        got = fresh.explain_batch(S, C, N, cont, after, reason, mask, [1 << 4] * S)
        for s in range(S):
            assert np.array_equal(got[s], ER.hist(_explained(BASE + s, C, N)[ffd[s][1] <= 1]))


# ---- drain sweep ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drained(C, N):
    cont, nodes = _scen(BASE, C, N)
    assign, live, cnt = D.live(cont, nodes, R.SPREAD, PREF)
    group = np.arange(N, dtype=np.uint32)
    return cont, live, assign, cnt, group, D.sweep(cont, live, assign, group, N, R.SPREAD, PREF, cnt)


def test_drain_sweep(fresh):
    for _, C, N in SHAPES:
        cont, live, assign, cnt, group, exp = _drained(C, N)
        out, reason, summary = fresh.drain_sweep(cont, live, assign, group, N, R.SPREAD, PREF, cnt)
        assert np.array_equal(out, exp[0]) and np.array_equal(reason, exp[1])
        assert summary.shape == exp[2].shape and np.array_equal(summary, exp[2])
