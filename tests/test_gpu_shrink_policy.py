"""GPU tests of the scale-in sweep under the policy (SPEC.md 2.17; k_shrink_sweep<.., SP, FB> in
fleetflow_amd/csrc/fp_shrink.hip): both entry points against the numpy reference (tests/shrink_policy_ref.py),
which makes one policy_fallback_ref.place call per attempt.  Every comparison is exact: assign_out, state,
blocker, every summary word, hops, blocker reasons and every word of every policy row."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import policy_ref as R  # noqa: E402
import shrink_policy_cases as T  # noqa: E402
import shrink_policy_ref as SP  # noqa: E402
import shrink_ref as S  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
PREF2 = (1 << 0) | (1 << 2)
RELAX = (1, 2)
NAMES = ("assign_out", "state", "blocker", "summary", "hops", "blocker_reason", "policy rows")
# the three kernels of a geometry: under the constraint, under the chain, under both
MODES = {"SP": dict(max_skew=2, relax_mask=()), "FB": dict(max_skew=0, relax_mask=RELAX),
         "SPFB": dict(max_skew=2, relax_mask=RELAX)}


def _check(got, exp):
    for g, e, what in zip(got, exp, NAMES):
        assert g.shape == e.shape and g.dtype == e.dtype, what
        assert np.array_equal(g, e), what


def _both(planner, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None, **kw):
    got = planner.shrink_sweep_policy(cont, nodes, assign, try_order, strategy, preferred, node_count, **kw)
    _check(got, SP.sweep(cont, nodes, assign, try_order, strategy, preferred, node_count, **kw))
    return got


@functools.lru_cache(maxsize=None)
def _case(seed, n_dom=4, C=300, N=40):
    return SP.random_case(seed, C=C, N=N, n_dom=n_dom, max_skew=2, relax_mask=RELAX)


@functools.lru_cache(maxsize=None)
def _embedded(seed, N, n_dom=4):
    """The 40-server live fleet of ``_case`` spread over N node indices (0 and N - 1 among them); every other
    server is cordoned, full and empty, in domain 63."""
    cont, live, assign, cnt, dom, order = _case(seed, n_dom)
    pos = np.unique(np.linspace(0, N - 1, 40).astype(np.int64))
    assert pos.size == 40 and pos[0] == 0 and pos[-1] == N - 1

    def wide(x, fill=0):
        out = np.full(N, fill, x.dtype)
        out[pos] = x
        return out
    nodes = tuple(wide(x) for x in live)
    assign_w = np.where(assign == NONE, NONE, pos[np.where(assign == NONE, 0, assign)]).astype(np.uint32)
    res = (cont, nodes, assign_w, wide(cnt), wide(dom, 63), pos[order].astype(np.uint32))
    for a in (*nodes, *res[2:]):
        a.setflags(write=False)
    return res


def _not_vacuous(trace):
    assert any(t[1] == "OK" and t[2] > 0 for t in trace), "a commit with moves"
    assert any(t[1] != "OK" and t[2] > 0 for t in trace), "a failed attempt that moved something first"


# ---- geometry: 64 x 1 and 1024 x {1, 2, 4, 8}, on both sides of every switch, each under SP, FB and both ---------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [40, 64, 65, 1024, 1025, 2049, 4097])
def test_every_block_geometry(N, mode, planner):
    cont, nodes, assign, cnt, dom, order = _embedded(2, N) if N > 40 else _case(2)
    strategy = (N + len(mode)) % 4
    kw = dict(MODES[mode], domain=dom)
    ref = SP.variant(cont, nodes, assign, order, strategy, 0, cnt, **kw)
    _not_vacuous(ref[7])
    assert max(t[0] for t in ref[7]) == N - 1  # the last slot row is in play
    got = _both(planner, cont, nodes, assign, np.stack([order, order[::-1]]), strategy, 0, cnt, **kw)
    assert np.array_equal(got[0][0], ref[0]) and np.array_equal(got[6][0], ref[6])


# ---- evictee counts round the 64-record chunk; an undo of more than 64 moves under the constraint -----------------
COUNTS = (63, 64, 65, 129)


@pytest.mark.parametrize("mode", list(MODES))
def test_evictee_counts_at_the_chunk_boundaries_and_a_long_undo(mode, planner):
    """Node k holds COUNTS[k] services; forty more servers in four domains take them.  One variant per node.  A
    fifth node holds 129 services of which the smallest requires a label no server has: 128 moves, then the
    blocker, then the undo; and the variant goes on to release node 0 on the state that undo left."""
    rng = np.random.default_rng(11)
    k = len(COUNTS)
    C, N = sum(COUNTS) + 129, k + 1 + 40
    cont = (rng.integers(2, 40, C).astype(np.uint32) * 10, rng.integers(1, 9, C).astype(np.uint32) * 64,
            np.where(rng.random(C) < 0.3, 1, 0).astype(np.uint32), np.where(rng.random(C) < 0.2, 1 << 16, 0).astype(np.uint32))
    assign = np.concatenate((rng.permutation(np.repeat(np.arange(k), COUNTS)), np.full(129, k))).astype(np.uint32)
    last = C - 1
    cont[0][last], cont[2][last] = 10, 1 << 9  # visited last, and no server carries bit 9
    lab = np.where(np.arange(N) % 3 == 0, 1, 0).astype(np.uint32)
    nodes = (rng.integers(2000, 5000, N).astype(np.uint32), np.full(N, 1 << 16, np.uint32), lab, np.zeros(N, np.uint32),
             np.ones(N, np.uint8))
    nodes[0][:k + 1] = 0
    dom = (np.arange(N) % 4).astype(np.uint32)
    cnt = np.bincount(assign, minlength=N).astype(np.uint32)
    orders = SP.pad([[n] for n in range(k)] + [[k, 0]])
    kw = dict(MODES[mode], domain=dom)
    kw["max_skew"] = 1000 if kw["max_skew"] else 0  # wide enough that every move is made; the counters still run
    got = _both(planner, cont, nodes, assign, orders, R.SPREAD, 0, cnt, **kw)
    assert got[3][:k, SP.MOVES].tolist() == list(COUNTS)
    ref = SP.variant(cont, nodes, assign, orders[k], R.SPREAD, 0, cnt, **kw)
    assert ref[7][0][:3] == (k, "NOFIT", 128) and ref[7][1][1] == "OK" and got[2][k][k] == last


# ---- C round the scan step: BLK * 16 positions (1024 for N <= 64, 16384 above) ----------------------------------
@pytest.mark.parametrize("C,N", [(1023, 40), (1024, 40), (1025, 64), (16383, 70), (16384, 70), (16385, 70)])
def test_container_counts_at_the_scan_step(C, N, planner):
    """The last containers of the 2.3 order (the smallest) sit on the tried nodes, so the scan has to reach the
    last position to find them; the first ones too."""
    rng = np.random.default_rng(C)
    cpu = rng.integers(10, 60, C).astype(np.uint32)
    cpu[:3] = [5, 5, 61]
    cont = (cpu, rng.integers(1, 9, C).astype(np.uint32), np.where(np.arange(C) % 5 == 0, 1, 0).astype(np.uint32),
            np.zeros(C, np.uint32))
    assign = rng.integers(3, N, C).astype(np.uint32)
    assign[:3] = [0, 1, 2]
    assign[C - 1] = 0
    nodes = (rng.integers(70, 500, N).astype(np.uint32), np.full(N, 1 << 20, np.uint32),
             np.where(np.arange(N) % 7 == 0, 1, 0).astype(np.uint32), np.zeros(N, np.uint32), np.ones(N, np.uint8))
    order = np.concatenate(([0, 1, 2], rng.permutation(np.arange(3, N))[:12])).astype(np.uint32)
    dom = (np.arange(N) % 5).astype(np.uint32)
    cnt = np.bincount(assign, minlength=N).astype(np.uint32)
    got = _both(planner, cont, nodes, assign, order[None, :], R.FIRST_FIT, 0, cnt, domain=dom, max_skew=C, relax_mask=(1,))
    assert got[1][0, :3].tolist() == [1, 1, 1] and got[3][0, SP.MOVES] >= 4


# ---- strategies x preferred labels x node counts -------------------------------------------------------------------
@pytest.mark.parametrize("pref", [0, PREF2])
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_strategies_preferred_and_counts(strategy, pref, planner):
    cont, live, assign, cnt, dom, order = _case(3)
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    _not_vacuous(SP.variant(cont, live, assign, order, strategy, pref, cnt, **kw)[7])
    with_cnt = _both(planner, cont, live, assign, order[None, :], strategy, pref, cnt, **kw)
    none = _both(planner, cont, live, assign, order[None, :], strategy, pref, **kw)  # no node_count is zeros
    _check(none, SP.sweep(cont, live, assign, order[None, :], strategy, pref, np.zeros(cnt.size, np.uint32), **kw))
    assert with_cnt[3][0, SP.RELEASED] > 0 and not np.array_equal(with_cnt[0], none[0])


# ---- domain counts: one, two, 33 (both mask words) and all 64 -------------------------------------------------------
@pytest.mark.parametrize("n_dom", [1, 2, 33, 64])
def test_domain_counts(n_dom, planner):
    cont, live, assign, cnt, dom, order = _case(2, n_dom, 300, 70)
    assert int(dom.max()) == n_dom - 1
    for mode in ("SP", "SPFB"):
        got = _both(planner, cont, live, assign, order[None, :], R.SPREAD, 0, cnt, **dict(MODES[mode], domain=dom))
        assert got[3][0, SP.RELEASED] > 0
        if n_dom == 1:  # one domain: the constraint never closes anything and the bound never refuses
            assert got[6][0, SP.FAILED_SKEW] == 0 and got[6][0, SP.SKEW_BEFORE] == 0
    if n_dom > 32:
        trace = SP.variant(cont, live, assign, order, R.SPREAD, 0, cnt, dom, 2, RELAX)[7]
        assert "last target released" in SP.conditions(trace)


# ---- ragged rows, one variant and thirty-three ---------------------------------------------------------------------
@pytest.mark.parametrize("n_var", [1, 33])
def test_ragged_rows_and_variant_counts(n_var, planner):
    cont, live, assign, cnt, dom, order = _case(4)
    rng = np.random.default_rng(n_var)
    rows = []
    for v in range(n_var):
        o = rng.permutation(order[:40])[:rng.integers(0, 41)].tolist()
        for at in sorted(rng.integers(0, len(o) + 1, 3).tolist(), reverse=True):
            o.insert(at, NONE)  # holes anywhere
        rows.append(o + o[:2])  # and a few nodes named twice
    rows[0] = [int(x) for x in order]
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    got = _both(planner, cont, live, assign, SP.pad(rows), R.PACK, 0, cnt, **kw)
    alone = planner.shrink_sweep_policy(cont, live, assign, np.array([rows[0]], np.uint32), R.PACK, 0, cnt, **kw)
    for g, a in zip(got, alone):  # theorem F: the padding changes nothing
        assert np.array_equal(g[0], a[0])
    if n_var > 1:
        assert len({r.tobytes() for r in got[0]}) > 10  # the variants differ


def test_no_try_entries_no_containers_no_variants(planner):
    cont, live, assign, cnt, dom, order = _case(0)
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    got = _both(planner, cont, live, assign, np.zeros((2, 0), np.uint32), 0, 0, cnt, **kw)
    assert np.array_equal(got[0], np.stack([assign, assign])) and not got[4].any() and not got[5].any()
    assert got[6][0, SP.SKEW_BEFORE] == got[6][0, SP.SKEW_AFTER]
    none = tuple(np.zeros(0, np.uint32) for _ in range(4))
    got = _both(planner, none, live, np.zeros(0, np.uint32), np.array([[3, 3, NONE, 7]], np.uint32), 0, 0, cnt, **kw)
    assert got[3][0, SP.TRIED] in (2, 3) and got[4].shape == (1, 0)  # 3: the bound kept node 3 the first time
    got = planner.shrink_sweep_policy(cont, live, assign, np.zeros((0, 4), np.uint32), **kw)
    assert [x.shape for x in got] == [(0, 300), (0, 40), (0, 40), (0, 8), (0, 300), (0, 40), (0, 4)]


# ---- theorems A, B and C on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 1025])
@pytest.mark.parametrize("form", ["neither", "max_skew 0", "no hops"])
def test_theorem_a_without_guarantees_it_is_fp_shrink_sweep(form, N, planner):
    cont, nodes, assign, cnt, dom, order = _embedded(1, N) if N > 40 else _case(1)
    tro = np.stack([order, order[::-1]])
    kw = {"neither": {}, "max_skew 0": dict(domain=dom, max_skew=0), "no hops": dict(domain=None, max_skew=3)}[form]
    plain = planner.shrink_sweep(cont, nodes, assign, tro, R.SPREAD, PREF2, cnt)
    got = planner.shrink_sweep_policy(cont, nodes, assign, tro, R.SPREAD, PREF2, cnt, **kw)
    for g, e in zip(got[:4], plain):
        assert g.dtype == e.dtype and np.array_equal(g, e)
    assert not got[4].any() and not got[6].any() and (plain[1] == S.ST_FAILED).any()
    assert np.array_equal(got[5], np.where(plain[1] == S.ST_FAILED, SP.REASON_NOFIT, 0).astype(np.uint8))


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_b_drain_anchor(strategy, planner):
    """Variant [n] against fp_drain_sweep_policy (fp_drain.hip) with node n as the one candidate, for every node."""
    cont, live, assign, cnt, dom, _ = _case(2, 33)
    N = live[0].size
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    got = planner.shrink_sweep_policy(cont, live, assign, np.arange(N, dtype=np.uint32)[:, None], strategy, 0, cnt, **kw)
    kinds = set()
    for n in range(N):
        group = np.where(np.arange(N) == n, 0, NONE).astype(np.uint32)
        d_out, d_reason, d_rows, d_hops, d_pol = planner.drain_sweep_policy(cont, live, assign, group, 1, strategy, 0, cnt, **kw)
        if d_rows[0, D.STRANDED] > 0:
            first = int(d_rows[0, D.FIRST_STRANDED])
            assert got[1][n][n] == SP.ST_FAILED and got[2][n][n] == first and got[5][n][n] == d_reason[first]
            assert np.array_equal(got[0][n], assign)
            kinds.add("stranded")
            continue
        gone = np.arange(N) == n
        sched = np.asarray(live[4])
        left = cnt.astype(np.int64) + np.bincount(d_out[assign == n], minlength=N)
        before, after = SP.skew(cnt, dom, np.zeros(N, bool), sched), SP.skew(left, dom, gone, sched * ~gone)
        if after <= 2 or after <= before:
            assert np.array_equal(got[0][n], d_out) and np.array_equal(got[4][n], d_hops) and got[3][n][SP.RELEASED] == 1
            kinds.add("commit")
        else:
            assert np.array_equal(got[0][n], assign) and got[1][n][n] == SP.ST_FAILED and got[2][n][n] == NONE
            assert got[5][n][n] == SP.REASON_SKEW
            kinds.add("bound")
    assert "commit" in kinds and len(kinds) > 1


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_theorem_c_undo_is_exact(strategy, planner):
    """The order with and without each of its failing first-pass entries, all in one call."""
    cont, live, assign, cnt, dom, order = _case(2, 33)
    once = order[:40]
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    trace = SP.variant(cont, live, assign, once, strategy, 0, cnt, **kw)[7]
    assert len(trace) == 40
    failing = [i for i, t in enumerate(trace) if t[1] != "OK"]
    assert {trace[i][1] for i in failing} >= {"SKEW"} and any(trace[i][2] > 0 for i in failing)
    rows = [list(once)] + [list(once[:i]) + list(once[i + 1:]) for i in failing]
    got = _both(planner, cont, live, assign, SP.pad(rows), strategy, 0, cnt, **kw)
    for k, i in enumerate(failing, 1):
        x = int(once[i])
        rest = np.arange(live[0].size) != x
        assert np.array_equal(got[0][k], got[0][0]) and np.array_equal(got[4][k], got[4][0])
        for w in (1, 2, 5):
            assert np.array_equal(got[w][k][rest], got[w][0][rest])
        assert (got[1][0][x], got[1][k][x]) == (SP.ST_FAILED, SP.ST_NEVER)
        diff = got[3][0].astype(np.int64) - got[3][k].astype(np.int64)
        assert diff[:7].tolist() == [0, 1, 1, 0, 0, 0, 0]
        diff = got[6][0].astype(np.int64) - got[6][k].astype(np.int64)
        assert diff.tolist() == [int(trace[i][1] != "NOFIT"), 0, 0, 0]


# ---- the hand-made traps, on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [None, 70, 1100])
def test_traps(N, planner):
    for name, kw, expected in T.traps():
        kw = kw if N is None else T.padded(kw, N)
        args = dict(kw)
        got = planner.shrink_sweep_policy(args.pop("cont"), args.pop("nodes"), args.pop("assign"), args.pop("try_order"),
                                          args.pop("strategy"), 0, args.pop("node_count"), **args)
        T.check(got, expected, name)
        _check(got, SP.sweep(**kw))


# ---- the device entry ------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
    return t.to("cuda:0")


FILL32 = 0xA5A5A5A5 - (1 << 32)
ALL_OUT = ("blocker", "hops", "reason", "policy")


def _dev_call(planner, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
              relax_mask=(), want=ALL_OUT):
    """dev_shrink_sweep_policy on copies of the inputs; returns (the call's tensors, the outputs in the order of
    Planner.shrink_sweep_policy's result).  The outputs start filled with 0xA5 bytes; those not in ``want`` are
    NULL."""
    import torch
    try_order = np.asarray(try_order, np.uint32)
    C, N, V = len(assign), len(nodes[0]), try_order.shape[0]
    ins = ([_dev(np.asarray(x, np.uint32)) for x in cont],
           [_dev(np.asarray(x, np.uint32)) for x in nodes[:4]] + [_dev(np.asarray(nodes[4], np.uint8))],
           _dev(np.asarray(assign, np.uint32)), _dev(try_order.reshape(-1)),
           None if node_count is None else _dev(np.asarray(node_count, np.uint32)),
           None if domain is None else _dev(np.asarray(domain, np.uint32)))
    w32 = lambda n: torch.full((n,), FILL32, dtype=torch.int32, device="cuda:0")  # noqa: E731
    w8 = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    out, state, rows = w32(V * C), w8(V * N), w32(V * 8)
    blk = w32(V * N) if "blocker" in want else None
    hops = w8(V * C) if "hops" in want else None
    why = w8(V * N) if "reason" in want else None
    prow = w32(V * 4) if "policy" in want else None
    planner.dev_shrink_sweep_policy(tuple(ins[0]), tuple(ins[1]), ins[2], ins[3], V, out, state, rows, strategy, preferred,
                                    ins[4], blk, domain_t=ins[5], max_skew=max_skew, relax_mask=relax_mask, hops_t=hops,
                                    blocker_reason_t=why, policy_t=prow)
    return ins, (out, state, blk, rows, hops, why, prow)


def _np_out(outs, V, C, N):
    shapes = ((V, C), (V, N), (V, N), (V, 8), (V, C), (V, N), (V, 4))
    res = []
    for t, shape in zip(outs, shapes):
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        res.append((a.view(np.uint32) if a.dtype == np.int32 else a).reshape(shape))
    return tuple(res)


def _untouched(outs):
    return all((t is None) or bool((t.cpu().numpy().view(np.uint8) == 0xA5).all()) for t in outs)


def test_device_entry_equals_the_reference_keeps_its_inputs_and_a_placement_follows(planner):
    from oracle import oracle as O
    cont, nodes, assign, cnt, dom, order = _embedded(3, 1025)
    tro = np.stack([order, order[::-1], np.roll(order, 7)])
    kw = dict(domain=dom, max_skew=2, relax_mask=RELAX)
    ins, outs = _dev_call(planner, cont, nodes, assign, tro, R.SPREAD, PREF2, cnt, **kw)
    pc, pn = O.gen_scenario(0x5EED0011, 9, 300, 40, 7)
    ea, er, _, _ = O.place(pc, pn)
    a, r, _, _ = planner.place_batch(1, 300, 40, pc, pn)  # the sweep's workspace is recycled under it
    assert np.array_equal(a, ea) and np.array_equal(r, er)
    planner.sync()
    exp = SP.sweep(cont, nodes, assign, tro, R.SPREAD, PREF2, cnt, **kw)
    _check(_np_out(outs, 3, 300, 1025), exp)
    for t, a in zip([*ins[0], *ins[1], ins[2], ins[3], ins[4], ins[5]], (*cont, *nodes, assign, tro, cnt, dom)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    host = planner.shrink_sweep_policy(cont, nodes, assign, tro, R.SPREAD, PREF2, cnt, **kw)
    _check(host, exp)


@pytest.mark.parametrize("mode", ["none"] + list(MODES))
def test_each_nullable_output_as_null(mode, planner):
    cont, live, assign, cnt, dom, order = _case(3)
    kw = dict(domain=dom, max_skew=0, relax_mask=()) if mode == "none" else dict(MODES[mode], domain=dom)
    exp = SP.sweep(cont, live, assign, order[None, :], R.PACK, 0, cnt, **kw)
    for leave in ALL_OUT + (None,):
        want = tuple(w for w in ALL_OUT if w != leave) if leave else ()
        _, outs = _dev_call(planner, cont, live, assign, order[None, :], R.PACK, 0, cnt, want=want, **kw)
        planner.sync()
        got = _np_out(outs, 1, 300, 40)
        assert [g is None for g in got] == [False, False, "blocker" not in want, False, "hops" not in want,
                                            "reason" not in want, "policy" not in want]
        for g, e, what in zip(got, exp, NAMES):
            assert g is None or np.array_equal(g, e), (what, leave)
    # the host entry without a guarantee and without any of the three further outputs is fp_shrink_sweep
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)  # noqa: E731
    arrs = [u32(x) for x in cont] + [u32(x) for x in live[:4]] + [np.ascontiguousarray(live[4], dtype=np.uint8)]
    tro = u32(order[None, :])
    outs = [np.empty(300, np.uint32), np.empty(40, np.uint8), np.empty(40, np.uint32), np.empty(8, np.uint32)]
    cs = _lib.FpContainers(300, *(x.ctypes.data for x in arrs[:4]))
    ns = _lib.FpNodes(40, *(x.ctypes.data for x in arrs[4:]))
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    rc = planner._L.fp_shrink_sweep_policy(planner._ctx, ct.byref(cs), ct.byref(ns), p(u32(assign), _lib.u32p),
                                           p(tro, _lib.u32p), 1, tro.shape[1], R.PACK, 0, p(u32(cnt), _lib.u32p), None, 0,
                                           None, 0, p(outs[0], _lib.u32p), p(outs[1], _lib.u8p), p(outs[2], _lib.u32p),
                                           p(outs[3], _lib.u32p), None, None, None)
    assert rc == _lib.FP_OK
    for g, e in zip(outs, S.sweep(cont, live, assign, tro, R.PACK, 0, cnt)):
        assert np.array_equal(g, e[0])


# ---- errors: nothing is written -----------------------------------------------------------------------------------
def _raw_host(planner, cont, nodes, assign, try_order, strategy=0, alias=False, n_var=None, domain=None, max_skew=0,
              n_hops=0):
    """fp_shrink_sweep_policy itself, on outputs pre-filled with 0xA5: (rc, outputs untouched?)."""
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)  # noqa: E731
    cont, assign, tro = tuple(u32(x) for x in cont), u32(assign).copy(), u32(try_order)
    nodes = tuple(u32(x) for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8),)
    C, N = assign.size, nodes[0].size
    V, T_ = (tro.shape if n_var is None else (n_var, 0))
    rows_v = min(V, 4)  # an n_var the call refuses is never written for
    out = assign if alias else np.full(rows_v * C, 0xA5A5A5A5, np.uint32)
    state, blk = np.full(rows_v * N, 0xA5, np.uint8), np.full(rows_v * N, 0xA5A5A5A5, np.uint32)
    rows = np.full(rows_v * 8, 0xA5A5A5A5, np.uint32)
    hops, why, prow = np.full(rows_v * C, 0xA5, np.uint8), np.full(rows_v * N, 0xA5, np.uint8), np.full(rows_v * 4, 0xA5A5A5A5, np.uint32)
    keep = out.copy()
    dom = None if domain is None else u32(domain)
    relax = u32([1, 2, 4, 8, 16])
    cs = _lib.FpContainers(C, *(x.ctypes.data for x in cont))
    ns = _lib.FpNodes(N, *(x.ctypes.data for x in nodes))
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    rc = planner._L.fp_shrink_sweep_policy(planner._ctx, ct.byref(cs), ct.byref(ns), p(assign, _lib.u32p), p(tro, _lib.u32p),
                                           V, T_, strategy, 0, None, None if dom is None else p(dom, _lib.u32p), max_skew,
                                           p(relax, _lib.u32p), n_hops, p(out, _lib.u32p), p(state, _lib.u8p),
                                           p(blk, _lib.u32p), p(rows, _lib.u32p), p(hops, _lib.u8p), p(why, _lib.u8p),
                                           p(prow, _lib.u32p))
    untouched = (np.array_equal(out, keep) and (state == 0xA5).all() and (blk == 0xA5A5A5A5).all()
                 and (rows == 0xA5A5A5A5).all() and (hops == 0xA5).all() and (why == 0xA5).all()
                 and (prow == 0xA5A5A5A5).all())
    return rc, bool(untouched)


def _bad_cases():
    cont, nodes, assign, cnt, dom, order = _embedded(2, 65)
    tro = np.stack([order, order[::-1]])
    bad_try, last_try, bad_assign, last_assign = tro.copy(), tro.copy(), assign.copy(), assign.copy()
    bad_try[0, 0] = 65
    last_try[1, -1] = 0xFFFFFFFE
    bad_assign[0] = 65
    last_assign[299] = 0xFFFFFFFE
    bad_dom, last_dom = dom.copy(), dom.copy()
    bad_dom[0] = 64
    last_dom[64] = 0xFFFFFFFF
    big = tuple(np.resize(x, 8193) for x in nodes)
    ok = dict(nodes=nodes, assign=assign, try_order=tro, domain=dom, max_skew=2, n_hops=2)
    return cont, ok, [
        ("strategy", _lib.FP_EINVAL, dict(ok, strategy=4)),
        ("n_hops", _lib.FP_EINVAL, dict(ok, n_hops=5)),
        ("nodes", _lib.FP_EOVERFLOW, dict(ok, nodes=big, domain=np.resize(dom, 8193))),
        ("n_var", _lib.FP_EOVERFLOW, dict(ok, try_order=tro[:, :0], n_var=65536)),
        ("try_order", _lib.FP_EINVAL, dict(ok, try_order=bad_try)),
        ("try_order, last", _lib.FP_EINVAL, dict(ok, try_order=last_try)),
        ("assign", _lib.FP_EINVAL, dict(ok, assign=bad_assign)),
        ("assign, last", _lib.FP_EINVAL, dict(ok, assign=last_assign)),
        ("domain", _lib.FP_EINVAL, dict(ok, domain=bad_dom)),
        ("domain, last", _lib.FP_EINVAL, dict(ok, domain=last_dom)),
    ]


def test_host_entry_errors_write_nothing(planner):
    cont, ok, cases = _bad_cases()
    for name, code, kw in cases:
        assert _raw_host(planner, cont, **kw) == (code, True), name
    assert _raw_host(planner, cont, **dict(ok, try_order=ok["try_order"][:1], alias=True)) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, cont, **dict(ok, n_var=0)) == (_lib.FP_OK, True)  # no variant: nothing to write
    # a domain id of 64 or more is nothing wrong without a constraint: domain is not read
    assert _raw_host(planner, cont, **dict(cases[8][2], max_skew=0)) == (_lib.FP_OK, False)
    assert _raw_host(planner, cont, **ok) == (_lib.FP_OK, False)  # and the same call is fine
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.shrink_sweep_policy(cont, ok["nodes"], ok["assign"], ok["try_order"], domain=cases[8][2]["domain"], max_skew=1)
    assert e.value.code == _lib.FP_EINVAL


def test_device_entry_errors_write_nothing_and_the_context_goes_on(planner):
    import torch
    cont, ok, cases = _bad_cases()
    kw0 = dict(domain=ok["domain"], max_skew=2, relax_mask=RELAX)
    for name, code, kw in cases:
        if not name.startswith(("try_order", "assign", "domain")):
            continue  # returned directly, below
        # found on the device: the call returns, sync() reports FP_EINVAL
        _, outs = _dev_call(planner, cont, kw["nodes"], kw["assign"], kw["try_order"], 0, 0, None, kw["domain"], 2, RELAX)
        with pytest.raises(_lib.FleetplaceError) as e:
            planner.sync()
        assert e.value.code == code, name
        assert _untouched(outs), name
        planner.sync()  # reported once, then clear
    # returned directly, before anything is read or launched: every array is a few device words of 0xA5
    word = lambda: torch.full((64,), FILL32, dtype=torch.int32, device="cuda:0")  # noqa: E731
    for C, N, n_var, strategy, n_hops, code in ((8, 8, 1, 0, 5, _lib.FP_EINVAL), (8, 8, 1, 4, 0, _lib.FP_EINVAL),
                                                (8, 8193, 1, 0, 0, _lib.FP_EOVERFLOW), (8, 8, 65536, 0, 0, _lib.FP_EOVERFLOW)):
        ins, outs = [word() for _ in range(12)], [word() for _ in range(7)]
        relax = np.array([1, 2, 4, 8, 16], np.uint32)
        cs = _lib.FpContainers(C, *(t.data_ptr() for t in ins[:4]))
        ns = _lib.FpNodes(N, *(t.data_ptr() for t in ins[4:9]))
        rc = planner._L.fp_dev_shrink_sweep_policy(planner._ctx, ct.byref(cs), ct.byref(ns), ins[9].data_ptr(),
                                                   ins[10].data_ptr(), n_var, 2, strategy, 0, None, ins[11].data_ptr(), 1,
                                                   relax.ctypes.data_as(_lib.u32p), n_hops, *(t.data_ptr() for t in outs))
        torch.cuda.synchronize()
        assert rc == code and all(bool((t.cpu().numpy().view(np.uint8) == 0xA5).all()) for t in ins + outs)
    planner.sync()  # and nothing is pending
    _, outs = _dev_call(planner, cont, ok["nodes"], ok["assign"], ok["try_order"], 3, 0, None, **kw0)
    planner.sync()
    _check(_np_out(outs, 2, 300, 65), SP.sweep(cont, ok["nodes"], ok["assign"], ok["try_order"], 3, **kw0))


# ---- the flow-level path ------------------------------------------------------------------------------------------
def test_shrink_stage_under_policy_from_kdl(planner):
    from test_shrink_policy_host import _kdl_flow
    from fleetflow_amd.flow import live_tables, plan_stage, replan_domains, shrink_stage
    from fleetflow_amd.plan_output import format_shrink_report, shrink_report_from_json, shrink_report_to_json
    flow = _kdl_flow()
    plan = plan_stage(flow, "live", planner)
    assert plan.spread_topology_key == "region" and plan.spread_max_skew == 1 and plan.fallback_relax_order == ["class"]
    names, nodes, cont, live, assign, count, st, pmask = live_tables(flow, "live", plan)
    rep = shrink_stage(flow, "live", plan, planner=planner, under_policy=True)
    domain, has_key = replan_domains(nodes, "region")
    live = (*live[:4], [s if k else 0 for s, k in zip(live[4], has_key)])
    from fleetflow_amd.flow import _stage_labels, shrink_order
    relax = [_stage_labels(names, flow, nodes, list(plan.preferred)).key_mask("class")]
    orders = [shrink_order(rule, nodes, cont, assign) for rule in ("fewest", "lightest", "last")]
    ref = SP.sweep(cont, live, assign, np.array(orders, np.uint32), _lib.POLICY_STRATEGIES[st], pmask, count, domain, 1, relax)
    slugs = [n.slug for n in nodes]
    for i, v in enumerate(rep.variants):
        out, state, blocker, row, hops, why, prow = (x[i] for x in ref)
        assert v.released == [slugs[n] for n in orders[i] if state[n] == SP.ST_RELEASED]
        assert sorted(v.moves) == sorted((names[c], slugs[assign[c]], slugs[out[c]]) for c in range(len(names))
                                         if assign[c] != NONE and out[c] != assign[c])
        held = [n for n in orders[i] if state[n] == SP.ST_FAILED]
        assert v.stayed_reason == {slugs[n]: "BOUND" if blocker[n] == NONE else "SKEW" if why[n] == 3 else "NOFIT" for n in held}
        assert (v.skew_before, v.skew_after) == (int(prow[SP.SKEW_BEFORE]), int(prow[SP.SKEW_AFTER]))
        assert v.relaxed == {names[c]: ["class"] for c in range(len(names)) if out[c] != assign[c] and hops[c]}
    assert any(v.released for v in rep.variants) and any(v.stayed for v in rep.variants)
    assert shrink_report_from_json(shrink_report_to_json(rep)) == rep
    assert format_shrink_report(rep).count("\n  spread: skew over region ") == 3
