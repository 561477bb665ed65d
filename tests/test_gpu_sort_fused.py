"""GPU parity of the fused per-scenario sort (fp_place.hip k_scen_sort<true>, fp_payload.h): after phase B the
workgroup that sorted a scenario gathers its payload too (phase P: req, conf, the CYCLE / screen bit of the
position word), taking the container indices from the order it still holds in LDS instead of reading the
`order` row back in a second kernel.  Three paths leave no final order in LDS and make the workgroup read its
own `order` row: a cpu bucket above 1024 containers, the generic fallback, and the fallback reached after a
sample miss.  planner.place_batch against the oracle, bit for bit in assign, reason, cost and node tables, at
the sizes where phase P changes path (below one row of positions, the edges of one row, the chunk boundary of
K = 36,864 containers, the sort's LDS limit where the chunk buffer overlays the most), for each of those
paths alone and mixed in one batch, with the screen off, without nodes, with every and with no container
rejected, and against the two-kernel form (FP_OPT_SORT_FUSED = 0) on the same inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED7171
K = 36 * 1024          # PL_FIELD_CHUNK
SS_MAX_C = 50_336      # the LDS sort's limit (fp_place.hip ss_lds_bytes)
S, BASE = 3, 5
SIZES = [37, 1023, 1024, 1025, K - 1, K, K + 1, SS_MAX_C]
NONE = 0xFFFFFFFF

_inputs, _expected = {}, {}


def _nodes_for(C):
    return 600 if C > 4096 else 900


def _levels(C, n_scen, seed):
    """3-5 % FP_NONE, at least one per scenario."""
    rng = np.random.default_rng(seed)
    level = [np.where(rng.random(C) < 0.03 + 0.02 * (s % 2), NONE, rng.integers(0, 7, C)).astype(np.uint32)
             for s in range(n_scen)]
    for lv in level:
        if not (lv == NONE).any():
            lv[C // 2] = NONE
    return level


def _case(O, C, with_level):
    """Generator scenarios with flags 7 (labels and conflicts, so the screen fires), generated once."""
    key = (C, with_level)
    if key not in _inputs:
        N = _nodes_for(C)
        conts, nodes = zip(*[O.gen_scenario(SEED + C, s, C, N, 7) for s in range(S)])
        _inputs[key] = (list(conts), list(nodes), _levels(C, S, C) if with_level else None)
    return _inputs[key]


def _oracle(O, key, conts, nodes, level):
    """The oracle's plans for a batch, computed once per key and shared."""
    if key not in _expected:
        _expected[key] = [O.place(conts[s], nodes[s], level=None if level is None else level[s])
                          for s in range(len(conts))]
    return _expected[key]


def _run(planner, conts, nodes, level, base=BASE):
    C, N = conts[0][0].size, nodes[0][0].size
    cat = lambda parts, i: np.concatenate([p[i] for p in parts])  # noqa: E731
    lv = None if level is None else np.concatenate(level).astype(np.uint32)
    return planner.place_batch(len(conts), C, N, [cat(conts, i) for i in range(4)],
                               [cat(nodes, i) for i in range(5)], level=lv, scen_base=base)


def _check(planner, O, key, conts, nodes, level, base=BASE):
    C, N = conts[0][0].size, nodes[0][0].size
    assign, reason, cost, after = _run(planner, conts, nodes, level, base)
    for s, (ea, er, eafter, _) in enumerate(_oracle(O, key, conts, nodes, level)):
        assert np.array_equal(assign[s * C:(s + 1) * C], ea), s
        assert np.array_equal(reason[s * C:(s + 1) * C], er), s
        assert int(cost[s]) == O.cost(ea, N, base + s), s
        for i in (0, 1, 3):
            assert np.array_equal(after[i][s * N:(s + 1) * N], eafter[i]), s
    return assign, reason, cost, after


@pytest.mark.parametrize("with_level", [False, True], ids=["nolevel", "level"])
@pytest.mark.parametrize("C", SIZES)
def test_sort_fused_sizes(C, with_level, planner, O):
    conts, nodes, level = _case(O, C, with_level)
    reason = _check(planner, O, (C, with_level), conts, nodes, level)[1]
    if with_level:  # FP_REASON_CYCLE exactly where level says so
        assert np.array_equal(reason == 2, np.concatenate(level) == NONE)


# ---- the paths that leave no final order in LDS ----

def _nodes(rng, N, big=40_000):
    return (rng.integers(0, big, N).astype(np.uint32), rng.integers(0, big, N).astype(np.uint32),
            rng.integers(0, 8, N).astype(np.uint32), np.zeros(N, np.uint32),
            (rng.random(N) < 0.97).astype(np.uint8))


def _cont(rng, C, cpu, mem_vals):
    """cpu as given; mem from mem_vals; a fifth of the containers with a label / a conflict bit."""
    return (np.asarray(cpu, np.uint32), rng.choice(mem_vals, C).astype(np.uint32),
            (rng.random(C) < 0.2).astype(np.uint32) * (1 << rng.integers(0, 3, C)).astype(np.uint32),
            (rng.random(C) < 0.2).astype(np.uint32) << rng.integers(0, 32, C).astype(np.uint32))


def _hbm_cont(rng, kind, C):
    mem_vals = np.arange(1, 200) * 64
    if kind == "digits":          # every bucket small: the order stays in LDS
        cpu = rng.choice(np.arange(1, 60) * 40, C)
    elif kind == "one_bucket":    # every container the same cpu: one bucket of C > 1024
        cpu = np.full(C, 1500)
    elif kind == "bucket_1025":   # buckets of exactly 1024 (registers) and 1025 (scattered) beside small ones
        cpu = rng.permutation(np.concatenate([np.full(1024, 3000), np.full(1025, 2500),
                                              rng.choice(np.arange(1, 60) * 40, C - 2049)]))
    else:                         # 257 distinct cpu values: the generic fallback
        assert kind == "generic"
        cpu = rng.permutation(np.concatenate([np.arange(1, 258) * 7, rng.choice(np.arange(1, 258) * 7, C - 257)]))
    return _cont(rng, C, cpu, mem_vals)


def _hbm_case(kinds, C, seed):
    key = ("hbm", kinds, C)
    if key not in _inputs:
        rng = np.random.default_rng(seed)
        N = _nodes_for(C)
        _inputs[key] = ([_hbm_cont(rng, k, C) for k in kinds], [_nodes(rng, N) for _ in kinds],
                        _levels(C, len(kinds), seed + 1))
    return (key,) + _inputs[key]


@pytest.mark.parametrize("C", [6_000, K + 1])
@pytest.mark.parametrize("kind", ["one_bucket", "bucket_1025", "generic"])
def test_sort_fused_order_from_hbm(kind, C, planner, O):
    key, conts, nodes, level = _hbm_case((kind,) * S, C, 11 + C)
    _check(planner, O, key, conts, nodes, level)


def test_sort_fused_mixed_batch(planner, O):
    """A digit scenario, a large-bucket scenario and a fallback scenario in one batch: each workgroup
    chooses where its indices come from."""
    key, conts, nodes, level = _hbm_case(("digits", "one_bucket", "generic"), 6_000, 23)
    _check(planner, O, key, conts, nodes, level)


def test_sort_fused_sample_miss(planner, O):
    """The sample is the first 8 scenarios; scenario 9 of 10 holds a value they lack, so its workgroup runs
    rank pass 1 on its own values and then phase P."""
    n_scen, C = 10, 6_000
    N = _nodes_for(C)
    conts, nodes = [], []
    for s in range(n_scen):
        c, n = O.gen_scenario(SEED + 91, s, C, N, 7)
        c = [np.array(a, np.uint32) for a in c]
        if s == 9:
            c[0][C // 3] = 50 * 40 + 25  # between two sample cpu values
        conts.append(tuple(c))
        nodes.append(n)
    _check(planner, O, "sample_miss", conts, nodes, _levels(C, n_scen, 9))


# ---- screen, rejection extremes ----

@pytest.mark.parametrize("C", [K + 1, SS_MAX_C])
def test_sort_fused_screen_off(C, planner, O, opts):
    """FP_OPT_SCREEN = 0: no summ rows, only the CYCLE bits are set (the nodes' OR words still are)."""
    opts(screen=0)
    conts, nodes, level = _case(O, C, True)
    _check(planner, O, (C, True), conts, nodes, level)


@pytest.mark.parametrize("screen", [None, 0])
def test_sort_fused_no_nodes(screen, planner, O, opts):
    """N = 0: no node summary runs; every container is NOFIT or CYCLE."""
    if screen is not None:
        opts(screen=screen)
    C = 1025
    conts, _, level = _case(O, C, True)
    empty = tuple(np.zeros(0, np.uint32) for _ in range(4)) + (np.zeros(0, np.uint8),)
    assign, reason, _, _ = _check(planner, O, "no_nodes", conts, [empty] * S, level)
    assert (assign == NONE).all()
    assert np.array_equal(reason, np.where(np.concatenate(level) == NONE, 2, 1))


def test_sort_fused_all_rejected(planner, O):
    """Every container is a CYCLE member or fails the screen: every node uses conflict bit 0 and every
    container conflicts with it; half the containers are CYCLE members."""
    C = K + 1
    conts, nodes, _ = _case(O, C, False)
    conts = [c[:3] + (c[3] | np.uint32(1),) for c in conts]
    nodes = [n[:3] + (n[3] | np.uint32(1),) + n[4:] for n in nodes]
    rng = np.random.default_rng(1)
    level = [np.where(rng.random(C) < 0.5, NONE, 1).astype(np.uint32) for _ in range(S)]
    reason = _check(planner, O, "all_rejected", conts, nodes, level)[1]
    assert (reason != 0).all()


def test_sort_fused_none_rejected(planner, O):
    """No container is screened: every node carries every label and uses no conflict bit; no level."""
    C = K + 1
    conts, nodes, _ = _case(O, C, False)
    nodes = [n[:2] + (np.full_like(n[2], NONE), np.zeros_like(n[3])) + n[4:] for n in nodes]
    _check(planner, O, "none_rejected", conts, nodes, None)


# ---- options ----

def _same(x, y):
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
    for i in range(5):
        assert np.array_equal(x[3][i], y[3][i]), i


def test_sort_fused_option_parity(planner, O, opts):
    """The same batch (every source of indices in it) fused and as two kernels: identical outputs."""
    key, conts, nodes, level = _hbm_case(("digits", "one_bucket", "generic"), 6_000, 23)
    fused = _check(planner, O, key, conts, nodes, level)
    opts(sort_fused=0)
    _same(fused, _check(planner, O, key, conts, nodes, level))
    conts, nodes, level = _case(O, K + 1, True)
    two = _check(planner, O, (K + 1, True), conts, nodes, level)
    opts(sort_fused=-1)
    _same(two, _check(planner, O, (K + 1, True), conts, nodes, level))


@pytest.mark.parametrize("off", ["payload_lds", "scen_sort"])
def test_sort_fused_unfused_paths(off, planner, O, opts):
    """FP_OPT_PAYLOAD_LDS = 0 (random-gather payload) and FP_OPT_SCEN_SORT = 0 (radix order) leave nothing to
    fuse: the separate launches stay, and stay correct."""
    opts(**{off: 0})
    conts, nodes, level = _case(O, K + 1, True)
    _check(planner, O, (K + 1, True), conts, nodes, level)


def test_sort_fused_twice_on_one_context(planner, O):
    """The LDS limit, then C = 37 on the same context: no LDS size or flag of the first call survives."""
    for C in (SS_MAX_C, 37):
        conts, nodes, level = _case(O, C, True)
        _check(planner, O, (C, True), conts, nodes, level)
