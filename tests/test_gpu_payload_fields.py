"""GPU parity of the by-field payload gather (fp_pipe.hip k_payload_lds, FPP_PAYLOAD_BY_FIELD): one
workgroup per scenario keeps the container indices of all its positions t + 1024 j as u16 pairs and
streams level, conf and req through LDS once each, in chunks of K = 36,864 containers (PL_CHUNK: 144 KB of
one 4-byte field).  planner.place_batch against the oracle, bit for bit in assign, reason, cost and node
tables, at the sizes where the kernel changes path: below one row of positions, the edges of one row
(1,023 / 1,024 / 1,025), a chunk boundary (K - 1, K, K + 1) and the LDS sort's limit (50,336, whose last
row of positions is partly filled); 2K + 1 = 73,729 is past that limit and takes the radix path, so it is
not a case.  Each with and without level (3-5 % FP_NONE), the screen off (summ null), batches where every
container or none is CYCLE or screened, and the other two payload paths on the same inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED7070
K = 36 * 1024          # PL_CHUNK
SS_MAX_C = 50_336      # the LDS sort's limit (fp_place.hip ss_lds_bytes)
S, BASE = 3, 5
SIZES = [37, 1023, 1024, 1025, K - 1, K, K + 1, SS_MAX_C]
assert 2 * K + 1 > SS_MAX_C

_inputs, _expected = {}, {}


def _nodes_for(C):
    return 600 if C > 4096 else 900


def _case(O, C, with_level):
    """Inputs of (C, with_level), generated once: generator scenarios with flags 7 (labels and conflicts, so
    the screen fires)."""
    key = (C, with_level)
    if key not in _inputs:
        N = _nodes_for(C)
        conts, nodes = zip(*[O.gen_scenario(SEED + C, s, C, N, 7) for s in range(S)])
        level = None
        if with_level:
            rng = np.random.default_rng(C)
            level = [np.where(rng.random(C) < 0.03 + 0.01 * s, 0xFFFFFFFF, rng.integers(0, 7, C)).astype(np.uint32)
                     for s in range(S)]
            for lv in level:  # (C = 37: at least one)
                if not (lv == 0xFFFFFFFF).any():
                    lv[C // 2] = 0xFFFFFFFF
        _inputs[key] = (list(conts), list(nodes), level)
    return _inputs[key]


def _oracle(O, key, conts, nodes, level):
    """The oracle's plans for a batch, computed once per key and shared."""
    if key not in _expected:
        _expected[key] = [O.place(conts[s], nodes[s], level=None if level is None else level[s])
                          for s in range(len(conts))]
    return _expected[key]


def _check(planner, O, key, conts, nodes, level):
    C, N = conts[0][0].size, nodes[0][0].size
    cat = lambda parts, i: np.concatenate([p[i] for p in parts])  # noqa: E731
    lv = None if level is None else np.concatenate(level).astype(np.uint32)
    assign, reason, cost, after = planner.place_batch(len(conts), C, N, [cat(conts, i) for i in range(4)],
                                                      [cat(nodes, i) for i in range(5)], level=lv, scen_base=BASE)
    for s, (ea, er, eafter, _) in enumerate(_oracle(O, key, conts, nodes, level)):
        assert np.array_equal(assign[s * C:(s + 1) * C], ea), s
        assert np.array_equal(reason[s * C:(s + 1) * C], er), s
        assert int(cost[s]) == O.cost(ea, N, BASE + s), s
        for i in (0, 1, 3):
            assert np.array_equal(after[i][s * N:(s + 1) * N], eafter[i]), s
    return reason


@pytest.mark.parametrize("with_level", [False, True], ids=["nolevel", "level"])
@pytest.mark.parametrize("C", SIZES)
def test_payload_fields_sizes(C, with_level, planner, O):
    conts, nodes, level = _case(O, C, with_level)
    reason = _check(planner, O, (C, with_level), conts, nodes, level)
    if with_level:  # FP_REASON_CYCLE exactly where level says so
        assert np.array_equal(reason == 2, np.concatenate(level) == 0xFFFFFFFF)


@pytest.mark.parametrize("C", [K + 1, SS_MAX_C])
def test_payload_fields_screen_off(C, planner, O, opts):
    """FP_OPT_SCREEN = 0: summ is null, only the CYCLE bits are set."""
    opts(screen=0)
    conts, nodes, level = _case(O, C, True)
    _check(planner, O, (C, True), conts, nodes, level)


def test_payload_fields_all_rejected(planner, O):
    """Every container is a CYCLE member or fails the screen: every node uses conflict bit 0 and every
    container conflicts with it; half the containers are CYCLE members."""
    C = K + 1
    conts, nodes, _ = _case(O, C, False)
    conts = [c[:3] + (c[3] | np.uint32(1),) for c in conts]
    nodes = [n[:3] + (n[3] | np.uint32(1),) + n[4:] for n in nodes]
    rng = np.random.default_rng(1)
    level = [np.where(rng.random(C) < 0.5, 0xFFFFFFFF, 1).astype(np.uint32) for _ in range(S)]
    reason = _check(planner, O, "all_rejected", conts, nodes, level)
    assert (reason != 0).all()


def test_payload_fields_none_rejected(planner, O):
    """No container is screened: every node carries every label and uses no conflict bit; no level."""
    C = K + 1
    conts, nodes, _ = _case(O, C, False)
    nodes = [n[:2] + (np.full_like(n[2], 0xFFFFFFFF), np.zeros_like(n[3])) + n[4:] for n in nodes]
    _check(planner, O, "none_rejected", conts, nodes, None)


@pytest.mark.parametrize("path", ["fields", "gather", "radix"])
def test_payload_fields_three_paths(path, planner, O, opts):
    """The by-field kernel, k_gather_payload (FP_OPT_PAYLOAD_LDS = 0) and the radix path on one batch."""
    opts(scen_sort=0 if path == "radix" else -1, payload_lds=0 if path == "gather" else -1)
    conts, nodes, level = _case(O, K + 1, True)
    _check(planner, O, (K + 1, True), conts, nodes, level)
