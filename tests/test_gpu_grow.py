"""GPU tests of the scale-out sweep (SPEC.md 2.12; fleetflow_amd/csrc/fp_grow.hip): both entry points against
the numpy reference (tests/grow_ref.py), which makes one policy_ref.place call per candidate.  Every comparison
is exact: all eight words of every summary row, and assign_out where it is asked for."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_ref as G  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 0x5EED0012
NOFIT, CYCLE, SKEW = 1 << 1, 1 << 2, 1 << 3


def _u32(*xs):
    return tuple(np.ascontiguousarray(x, dtype=np.uint32) for x in xs)


def _both(planner, cont, reason, templates, max_new, reason_mask=NOFIT, t_max=None):
    """grow_sweep with assign_out against the reference; the call without assign_out gives the same rows."""
    exp = G.sweep(cont, reason, templates, max_new, reason_mask, t_max)
    rows, assign = planner.grow_sweep(cont, reason, templates, max_new, reason_mask, t_max, want_assign=True)
    assert rows.shape == exp[0].shape and np.array_equal(rows, exp[0])
    assert assign.shape == exp[1].shape and np.array_equal(assign, exp[1])
    only, none = planner.grow_sweep(cont, reason, templates, max_new, reason_mask, t_max)
    assert none is None and np.array_equal(only, exp[0])
    assert np.array_equal(rows[:, G.PENDING], rows[:, G.PLACED] + rows[:, G.UNPLACEABLE] + rows[:, G.CAPPED])
    return rows, assign


# ---- geometry: one wave up to 64 servers, blocks of 256 x {4, 8, 16, 32} above, both sides of every switch -----
EDGES = (1, 63, 64, 65, 1024, 1025, 2048, 2049, 4096, 4097, 8192)


@pytest.mark.parametrize("max_new", EDGES)
def test_every_server_slot_of_every_geometry(max_new, planner):
    """max_new + 3 small containers that share one host port: each needs a server of its own."""
    C = max_new + 3
    cont = _u32(np.full(C, 10), np.full(C, 16), np.zeros(C), np.ones(C))
    rows, assign = _both(planner, cont, None, _u32([1000], [4096], [0]), max_new, 0)
    assert rows[0].tolist() == [C, max_new, max_new, 0, 3, (990 * max_new) & NONE, (4080 * max_new) & NONE, max_new]
    assert assign[0].tolist() == list(range(max_new)) + [NONE] * 3


@pytest.mark.parametrize("max_new", (64, 1025, 8192))
def test_two_per_server_but_for_a_shared_anti_affinity_bit(max_new, planner):
    """The template takes two containers; every third carries one anti-affinity bit and a little more memory,
    so those come first, open a server each, and the others fill the second places from server 0 on."""
    C = max_new + 3
    third = np.arange(C) % 3 == 0
    cont = _u32(np.full(C, 10), np.where(third, 17, 16), np.zeros(C), np.where(third, 1 << 16, 0))
    rows, assign = _both(planner, cont, None, _u32([20], [4096], [0]), max_new, 0)
    n_third = int(third.sum())  # they open servers 0 .. n_third - 1 and never share one
    opened = n_third + (C - 2 * n_third + 1) // 2
    assert rows[0, :5].tolist() == [C, C, opened, 0, 0] and rows[0, G.FIRST_UNPLACED] == NONE
    assert assign[0][third].tolist() == list(range(n_third))
    assert assign[0][~third].tolist() == list(range(n_third)) + [n_third + i // 2 for i in range(C - 2 * n_third)]


# ---- one launch of everything ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(C, seed=7):
    rng = np.random.default_rng(seed)
    cont = _u32(rng.integers(1, 60, C) * 50, rng.integers(1, 33, C) * 128,
                np.where(rng.random(C) < 0.5, 1 << rng.integers(0, 6, C), 0) | np.where(rng.random(C) < 0.1, 1 << 9, 0),
                np.where(rng.random(C) < 0.3, 1 << rng.integers(0, 4, C), 0)
                | np.where(rng.random(C) < 0.2, 1 << (16 + rng.integers(0, 3, C)), 0))
    for x in cont:
        x.setflags(write=False)
    return cont


@pytest.mark.parametrize("max_new", (40, 100))
def test_mixed_templates_and_caps_in_one_launch(max_new, planner):
    rng = np.random.default_rng(max_new)
    cont, K = _random(300), 97
    t_cpu = rng.integers(0, 9, K) * 1000
    t_mem = rng.integers(0, 9, K) * 1024
    t_cpu[:3], t_mem[3:6] = 0, 0  # too small for anything
    t_lab = np.where(rng.random(K) < 0.5, 0xFFFFFFFF, rng.integers(0, 64, K))
    t_lab[6:9] = 1 << 20  # labels no container asks for
    t_max = rng.choice([0, 1, 7, max_new], K)
    t_cpu[96], t_mem[96], t_lab[96], t_max[96] = 10 ** 6, 10 ** 6, 0xFFFFFFFF, max_new  # takes everything
    rows, _ = _both(planner, cont, None, _u32(t_cpu, t_mem, t_lab), max_new, 0, t_max)
    assert (rows[:6, G.PLACED] == 0).all() and (rows[:, G.UNPLACEABLE] > 0).any() and (rows[:, G.CAPPED] > 0).any()
    assert (rows[:, G.OPENED] <= t_max).all() and (rows[:, G.OPENED] == max_new).any()
    assert rows[96, G.PLACED] == 300 and 1 < rows[96, G.OPENED] < max_new
    _both(planner, cont, None, _u32(t_cpu, t_mem, t_lab), max_new, 0)  # t_max NULL: max_new everywhere


# ---- which containers are pending -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(C=600, N=40, cycles=True):
    """Generated containers placed first fit on N generated nodes by the C oracle, some of them CYCLE."""
    from oracle import oracle as O
    cont, nodes = O.gen_scenario(SEED, 3, C, N, 7)
    level = np.zeros(C, np.uint32)
    if cycles:
        level[5::11] = NONE
    assign, reason, after, _ = O.place(cont, nodes, level)
    assert 20 < int((reason == 1).sum()) < C // 2 and (not cycles or int((reason == 2).sum()) > 10)
    return cont, nodes, level, assign, reason


TEMPLATES = _u32([4000, 16000, 2000, 64000], [8192, 65536, 4096, 262144], [0xFFFFFFFF, 0x3F, 0xFFFFFFFF, 0x15])


def test_pending_selection_by_reason_mask(planner):
    cont, _, _, _, reason = _plan()
    n_nofit, n_cycle = int((reason == 1).sum()), int((reason == 2).sum())
    rows, assign = _both(planner, cont, reason, TEMPLATES, 64)
    assert (rows[:, G.PENDING] == n_nofit).all() and (assign[:, reason != 1] == NONE).all()
    rows, _ = _both(planner, cont, reason, TEMPLATES, 64, NOFIT | CYCLE)  # CYCLE containers like any other
    assert (rows[:, G.PENDING] == n_nofit + n_cycle).all()
    rows, _ = _both(planner, cont, None, TEMPLATES, 200, 0)  # sizing a fleet from nothing, reason NULL
    assert (rows[:, G.PENDING] == 600).all()
    rows, assign = _both(planner, cont, reason, TEMPLATES, 64, 1 << 7)  # a mask that selects nothing
    assert rows.tolist() == [[0, 0, 0, 0, 0, 0, 0, NONE]] * 4 and (assign == NONE).all()


def test_pending_nofit_and_skew_of_a_spread_plan(planner):
    cont, nodes, _, _, _ = _plan()
    domain = np.arange(40, dtype=np.uint32) % 4
    _, reason, _, _ = planner.place_policy(cont, nodes, 1, domain=domain, max_skew=1)
    assert (reason == 3).any() and (reason == 1).any()
    rows, _ = _both(planner, cont, reason, TEMPLATES, 128, NOFIT | SKEW)
    assert (rows[:, G.PENDING] == int(((reason == 1) | (reason == 3)).sum())).all()


# ---- ties and extremes ----------------------------------------------------------------------------------------
def test_identical_containers_go_by_index(planner):
    C = 200  # more than three record chunks
    cont = _u32(np.full(C, 30), np.full(C, 2), np.zeros(C), np.zeros(C))
    rows, assign = _both(planner, cont, None, _u32([100], [100], [0]), 50, 0)
    assert assign[0].tolist() == [i // 3 for i in range(150)] + [NONE] * 50
    assert rows[0].tolist() == [200, 150, 50, 0, 50, 500, 4700, 150]


def test_zero_requests_unbounded_templates_and_a_wrapping_sum(planner):
    zero = _u32(np.zeros(70), np.zeros(70), np.zeros(70), np.zeros(70))
    rows, assign = _both(planner, zero, None, _u32([0, 5], [0, 5], [0, 0]), 3, 0)
    assert rows.tolist() == [[70, 70, 1, 0, 0, 0, 0, NONE], [70, 70, 1, 0, 0, 5, 5, NONE]]
    # the largest fills server 0; three containers on one host port take a server each: 3 * 0xFFFFFFFE wraps
    cont = _u32([1, 1, 1, 0xFFFFFFFF], [2, 2, 2, 0xFFFFFFFF], [0, 0, 0, 0xFFFFFFFF], [1, 1, 1, 2])
    rows, assign = _both(planner, cont, None, _u32([0xFFFFFFFF] * 2, [0xFFFFFFFF] * 2, [0xFFFFFFFF, 0]), 8, 0)
    assert rows[0].tolist() == [4, 4, 4, 0, 0, (3 * 0xFFFFFFFE) & NONE, (3 * 0xFFFFFFFD) & NONE, NONE]
    assert assign[0].tolist() == [1, 2, 3, 0] and rows[1, G.UNPLACEABLE] == 1 and rows[1, G.FIRST_UNPLACED] == 3


# ---- the append theorem, on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2))
def test_append_theorem_against_place_on_the_extended_table(k, planner):
    cont, nodes, level, _, _ = _plan()
    N = 40
    assign, reason, _ = planner.place(cont, nodes, level)
    caps = _u32([0, 5, 64])[0]
    tpl = tuple(np.repeat(x[k:k + 1], 3) for x in TEMPLATES)
    rows, grown = planner.grow_sweep(cont, reason, tpl, 64, NOFIT, caps, want_assign=True)
    assert rows[1, G.CAPPED] > 0  # five servers are not enough
    pend = reason == 1
    for j, m in enumerate(caps.tolist()):
        more = G.template_table(tpl[0][j], tpl[1][j], tpl[2][j], m)
        ext = tuple(np.concatenate([a, b]) for a, b in zip(nodes, more))
        a2, r2, _ = planner.place(cont, ext, level)
        assert np.array_equal(a2[~pend], assign[~pend]) and np.array_equal(r2[~pend], reason[~pend])
        exp = np.where(grown[j] == NONE, NONE, N + grown[j].astype(np.int64)).astype(np.uint32)
        assert np.array_equal(a2[pend], exp[pend])


# ---- the device entry -----------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.array(a)  # a writable copy
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _dev_call(planner, cont, reason, templates, max_new, reason_mask=NOFIT, t_max=None, want_assign=True, fill=0x5A):
    """dev_grow_sweep on copies of the inputs; returns (the input tensors, (rows, assign)).  The outputs start
    filled with ``fill`` bytes."""
    import torch
    C, K = len(cont[0]), len(templates[0])
    word = fill * 0x01010101 - (1 << 32) * (fill >= 0x80)
    ins = [_dev(np.asarray(x, np.uint32)) for x in cont], None if reason is None else _dev(np.asarray(reason, np.uint8)), \
        [_dev(np.asarray(x, np.uint32)) for x in templates], None if t_max is None else _dev(np.asarray(t_max, np.uint32))
    rows = torch.full((K * 8,), word, dtype=torch.int32, device="cuda:0")
    assign = torch.full((K * C,), word, dtype=torch.int32, device="cuda:0") if want_assign else None
    planner.dev_grow_sweep(tuple(ins[0]), ins[1], tuple(ins[2]), max_new, rows, reason_mask, ins[3], assign)
    return ins, (rows, assign)


def _np_out(outs, K):
    rows, assign = outs
    return (rows.cpu().numpy().view(np.uint32).reshape(K, 8),
            None if assign is None else assign.cpu().numpy().view(np.uint32).reshape(K, -1))


def test_device_entry_on_another_stream_equals_the_host_entry_and_keeps_its_inputs(planner):
    import torch
    cont, _, _, _, reason = _plan()
    caps = _u32([64, 7, 0, 33])[0]
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        ins, outs = _dev_call(planner, cont, reason, TEMPLATES, 64, NOFIT, caps)
    planner.sync()
    st.synchronize()
    rows, assign = _np_out(outs, 4)
    exp = planner.grow_sweep(cont, reason, TEMPLATES, 64, NOFIT, caps, want_assign=True)
    assert np.array_equal(rows, exp[0]) and np.array_equal(assign, exp[1])
    assert np.array_equal(rows, G.sweep(cont, reason, TEMPLATES, 64, NOFIT, caps)[0])
    for t, a in zip([*ins[0], ins[1], *ins[2], ins[3]], (*cont, reason, *TEMPLATES, caps)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_workspace_reuse_after_other_calls_and_a_larger_sweep_after_a_smaller(planner):
    from oracle import oracle as O
    cont, _, _, _, reason = _plan()
    rp, col, hd = O.gen_dag(SEED, 4, 5, 3, 6, 1)[:3]
    planner.levelize(rp, col, hd)
    _both(planner, cont, reason, TEMPLATES, 64)  # right after a levelize
    bc, bn = O.gen_scenario(SEED, 9, 3000, 200, 7)
    planner.place_batch(1, 3000, 200, bc, bn)
    _both(planner, cont, reason, TEMPLATES, 64)  # after a place_batch of a larger shape
    _, o1 = _dev_call(planner, tuple(x[:50] for x in cont), reason[:50], TEMPLATES, 64)
    big = _random(5000, seed=3)
    _, o2 = _dev_call(planner, big, None, TEMPLATES, 1024, 0, want_assign=False)  # larger, behind the smaller
    planner.sync()
    assert np.array_equal(_np_out(o1, 4)[0], G.sweep(tuple(x[:50] for x in cont), reason[:50], TEMPLATES, 64)[0])
    assert np.array_equal(_np_out(o2, 4)[0], G.sweep(big, None, TEMPLATES, 1024, 0)[0])


# ---- errors: nothing is written -------------------------------------------------------------------------------
def _raw_host(planner, cont, reason, reason_mask, K, max_new, t_max=None, n_cand=None):
    """fp_grow_sweep itself, on outputs pre-filled with 0xA5: (rc, outputs untouched?)."""
    cont = _u32(*cont)
    C = cont[0].size
    tpl = _u32(np.full(K, 1000), np.full(K, 1000), np.zeros(K))
    rs = None if reason is None else np.ascontiguousarray(reason, dtype=np.uint8)
    tm = None if t_max is None else _u32(t_max)[0]
    rows, assign = np.full(K * 8, 0xA5A5A5A5, np.uint32), np.full(K * C, 0xA5A5A5A5, np.uint32)
    cs = _lib.FpContainers(C, *(x.ctypes.data for x in cont))
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    rc = planner._L.fp_grow_sweep(planner._ctx, ct.byref(cs), p(rs, _lib.u8p), reason_mask, K if n_cand is None else n_cand,
                                  p(tpl[0], _lib.u32p), p(tpl[1], _lib.u32p), p(tpl[2], _lib.u32p), p(tm, _lib.u32p),
                                  max_new, p(rows, _lib.u32p), p(assign, _lib.u32p))
    return rc, bool((rows == 0xA5A5A5A5).all() and (assign == 0xA5A5A5A5).all())


def test_host_entry_errors_write_nothing(planner):
    cont, _, _, _, reason = _plan()
    assert _raw_host(planner, cont, reason, NOFIT, 4, 8193) == (_lib.FP_EOVERFLOW, True)
    assert _raw_host(planner, cont, reason, NOFIT, 4, 64, n_cand=65536) == (_lib.FP_EOVERFLOW, True)
    assert _raw_host(planner, cont, None, NOFIT, 4, 64) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, cont, reason, NOFIT, 4, 64, [64, 64, 65, 0]) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, cont, reason, NOFIT, 4, 64, [64, 64, 64, 0]) == (_lib.FP_OK, False)  # the same call is fine
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.grow_sweep(cont, reason, TEMPLATES, 64, t_max=[1, 2, 3, 65])
    assert e.value.code == _lib.FP_EINVAL


def test_device_entry_errors_write_nothing_and_the_context_goes_on(planner):
    cont, _, _, _, reason = _plan()
    for code, kw in ((_lib.FP_EOVERFLOW, dict(max_new=8193)), (_lib.FP_EINVAL, dict(max_new=64, reason=None))):
        with pytest.raises(_lib.FleetplaceError) as e:
            _dev_call(planner, cont, kw.get("reason", reason), TEMPLATES, kw["max_new"])
        assert e.value.code == code
        planner.sync()
    import torch
    many = tuple(torch.zeros(65536, dtype=torch.int32, device="cuda:0") for _ in range(3))
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.dev_grow_sweep(tuple(_dev(x) for x in cont), _dev(reason), many, 64,
                               torch.zeros(65536 * 8, dtype=torch.int32, device="cuda:0"))
    assert e.value.code == _lib.FP_EOVERFLOW
    planner.sync()
    # a t_max above max_new is found on the device: the call returns, sync() reports once
    _, outs = _dev_call(planner, cont, reason, TEMPLATES, 64, NOFIT, [64, 65, 0, 1], fill=0xA5)
    with pytest.raises(_lib.FleetplaceError) as e:
        planner.sync()
    assert e.value.code == _lib.FP_EINVAL
    rows, assign = _np_out(outs, 4)
    assert (rows == 0xA5A5A5A5).all() and (assign == 0xA5A5A5A5).all()
    planner.sync()  # reported once, then clear
    _, outs = _dev_call(planner, cont, reason, TEMPLATES, 64, NOFIT, [64, 64, 0, 1])
    planner.sync()
    exp = G.sweep(cont, reason, TEMPLATES, 64, NOFIT, [64, 64, 0, 1])
    rows, assign = _np_out(outs, 4)
    assert np.array_equal(rows, exp[0]) and np.array_equal(assign, exp[1])


def test_no_containers_and_no_candidates(planner):
    none = _u32([], [], [], [])
    rows, assign = _both(planner, none, np.zeros(0, np.uint8), TEMPLATES, 64)
    assert rows.tolist() == [[0, 0, 0, 0, 0, 0, 0, NONE]] * 4 and assign.shape == (4, 0)
    rows, assign = _both(planner, none, None, TEMPLATES, 64, 0, [0, 1, 2, 64])
    assert rows.tolist() == [[0, 0, 0, 0, 0, 0, 0, NONE]] * 4
    cont, _, _, _, reason = _plan()
    rows, assign = _both(planner, cont, reason, _u32([], [], []), 64)
    assert rows.shape == (0, 8) and assign.shape == (0, 600)
    _, outs = _dev_call(planner, none, None, TEMPLATES, 64, 0)
    planner.sync()
    assert _np_out(outs, 4)[0].tolist() == [[0, 0, 0, 0, 0, 0, 0, NONE]] * 4
