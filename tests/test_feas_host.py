"""Stage-2 feasibility (SPEC.md 2.3, 2.5) without a GPU: the numpy reference against both oracles, the
conditions that make the generated inputs worth comparing on, and the launch plan every shape of
test_gpu_feasibility.py is named for, pinned to the constants in fp_feas.hip."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feas_cases as K  # noqa: E402
import feas_ref as FR  # noqa: E402

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the shapes of test_gpu_feasibility.py and the launch each must get: (ysplit, span, tiles per blockIdx.y) ----
GRID_C = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
GRID_N = (0, 1, 63, 64, 65, 127, 128, 129, 1025)
DEVICE_SHAPES = ((1100, 1089), (300, 65))
PERIOD = 64 * 37  # the container table the two large single calls repeat
SINGLE_PLANS = {
    (1023 * 1024 + 1, 2200): (2, 1152, [[1024, 128], [1024, 24]]),  # split, several tiles, last block: 1 container
    (2047 * 1024 + 1, 1089): (1, 1152, [[1024, 65]]),               # unsplit, several tiles
    (2047 * 1024, 1089): (2, 576, [[576], [513]]),                  # one block fewer: split again
}
BATCH_PLANS = {
    (2048, 70, 2120): (1, 2176, [[1024, 1024, 72]]),
    (1024, 1030, 2120): (1, 2176, [[1024, 1024, 72]]),
    (2048, 16, 5000): (1, 5056, [[1024, 1024, 1024, 1024, 904]]),   # the benchmark's node count and tiles
    (2047, 70, 2120): (2, 1088, [[1024, 64], [1024, 8]]),
    (1, 70, 2120): (34, 64, [[64]] * 33 + [[8]]),
    (2, 1100, 64): (1, 64, [[64]]),
    (3, 1100, 64): (1, 64, [[64]]),
    (5, 1100, 0): (1, 64, []),
    (5, 0, 40): (1, 64, []),
}


def _plan(S, C, N):
    return FR.feas_plan(S, C, N)[1:]


def test_plan_of_every_named_shape():
    for (C, N), want in SINGLE_PLANS.items():
        assert _plan(None, C, N) == want, (C, N)
    assert FR.feas_plan(None, 1023 * 1024 + 1, 2200)[0] == 1024 and FR.feas_plan(None, 2047 * 1024 + 1, 1089)[0] == 2048
    for (S, C, N), want in BATCH_PLANS.items():
        assert _plan(S, C, N) == want, (S, C, N)
    assert FR.feas_plan(1024, 1030, 2120)[0] == 2 and 1030 - 1024 == 6  # the second block holds 6 containers
    # the edge grid: N <= 64 is one unsplit range, every other N runs in ranges of 64 with a ragged end
    for C in GRID_C:
        for N in GRID_N:
            ysplit, span, tiles = _plan(None, C, N)
            if N == 0:
                assert tiles == []
            elif N <= 64:
                assert (ysplit, span, tiles) == (1, 64, [[N]])
            else:
                assert span == 64 and ysplit == (N + 63) // 64 and tiles == [[64]] * (N // 64) + [[N % 64]] * (N % 64 > 0)
    assert _plan(None, 1100, 1089) == (18, 64, [[64]] * 17 + [[1]]) and _plan(None, 300, 65) == (2, 64, [[64], [1]])
    # the benchmark's stage-2 leg and the shapes test_gpu_parity.py runs
    assert _plan(512, 50_000, 5_000) == (1, 5056, [[1024, 1024, 1024, 1024, 904]])
    assert _plan(4, 50_000, 5_000)[:2] == (16, 320) and _plan(5, 3000, 5000)[:2] == (79, 64)
    assert _plan(None, 64, 70_000)[:2] == (1094, 64) and _plan(None, 1, 1) == (1, 64, [[1]])


def test_plan_constants_are_the_kernels():
    """Whoever retunes k_feas: feas_ref.feas_plan and the shapes above have to be derived again."""
    with open(os.path.join(ROOT, "fleetflow_amd", "csrc", "fp_feas.hip")) as f:
        src = f.read()
    const = {k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(kBlock|kPer|kTile)\s*=\s*(\d+)\s*;", src)}
    assert const == {"kBlock": FR.K_BLOCK, "kPer": FR.K_PER, "kTile": FR.K_TILE}
    below = re.findall(r"while\s*\(\s*\(uint64_t\)xb \* ysplit(?: \* S)? < (\d+) && ysplit < max_split\)", src)
    assert below == [str(FR.SPLIT_BELOW)] * 2  # the batch and the single launch
    assert "kBlock * kPer" in src and "(N + 63) / 64" in src and "(span + 63) & ~63u" in src


# ---- the reference against the oracles ---------------------------------------------------------------------
def _same_as_oracles(cont, nodes, O, P=None):
    first, count, bm = FR.feasibility(cont, nodes)
    ef, ec, eb = O.feasibility(cont, nodes)
    assert first.dtype == count.dtype == np.uint32 and bm.dtype == np.uint64
    assert np.array_equal(first, ef) and np.array_equal(count, ec) and np.array_equal(bm, eb)
    f2, c2, none = FR.feasibility(cont, nodes, want_bitmap=False)
    assert none is None and np.array_equal(f2, first) and np.array_equal(c2, count)
    if P is not None:
        pf, pc, pb = P.feasibility(*(np.asarray(x).tolist() for x in (*cont, *nodes)))
        assert pf == first.tolist() and pc == count.tolist() and pb == bm.tolist()
    return first, count, bm


@pytest.mark.parametrize("C,N,mask", [(1, 1, False), (65, 130, False), (65, 130, True), (200, 1030, False),
                                      (130, 70, True), (64, 64, False)])
def test_reference_vs_oracles_generated(C, N, mask, O, P):
    cont, nodes = K.case(C, N, seed=3, mask_nodes=mask)
    _same_as_oracles(cont, nodes, O, P if C * N <= 10_000 else None)
    if mask:
        assert K.has_mask_node_in_every_group(nodes)


@pytest.mark.parametrize("C,N", [(300, 65), (1030, 2120)])
def test_reference_vs_oracle_at_gpu_shapes(C, N, O):
    _same_as_oracles(*K.case(C, N), O)
    S = 3
    cont, nodes, _ = K.batch(S, C, N)
    first, count = FR.feasibility_batch(S, C, N, cont, nodes)
    ef, ec = K.batch_expected(S, C, N)
    assert np.array_equal(first, ef) and np.array_equal(count, ec)


B31 = 2**31
HAND_ROWS = [
    # cpu, mem, req, conf | cf, mf, lab, cu, sched | feasible
    ((4000, 64, 0b101, 0b10), (4000, 64, 0b101, 0b01, 1), True),                 # exact equality on every field
    ((4001, 64, 0, 0), (4000, 64, 0, 0, 1), False),                              # one short: cpu
    ((4000, 65, 0, 0), (4000, 64, 0, 0, 1), False),                              # one short: mem
    ((0, 0, 0b111, 0), (9, 9, 0b101, 0, 1), False),                              # one short: a label bit
    ((0, 0, 0, 0b100), (9, 9, 0, 0b100, 1), False),                              # one short: a port in use
    ((B31, B31 - 1, 0, 0), (B31 - 1, B31, 0, 0, 1), False),                      # 2^31 asked of 2^31 - 1
    ((B31 - 1, B31, 0, 0), (B31, B31, 0, 0, 1), True),                           # 2^31 - 1 asked of 2^31
    ((1, B31, 0, 0), (B31, B31 - 1, 0, 0, 1), False),                            # mem the same way
    ((0, 0, 1 << 31, 1 << 31), (0, 0, 1 << 31, 1 << 30, 1), True),               # the top label and port bits
    ((0, 0, 1 << 31, 0), (0, 0, (1 << 31) - 1, 0, 1), False),
    ((0, 0, 0, 1 << 31), (0, 0, 0, 1 << 31, 1), False),
    ((NONE, NONE, NONE, NONE), (NONE, NONE, NONE, 0, 1), True),                  # all ones on an accept-all node
    ((0, 0, NONE, 0), (0, 0, NONE, NONE, 1), True),
    ((0, 0, NONE, 0), (0, 0, NONE ^ (1 << 17), 0, 1), False),
    ((0, 0, 0, 0), (NONE, NONE, NONE, 0, 0), False),                             # a cordoned accept-all node
    ((0, 0, 0, 0), (0, 0, 0, 0, 2), True),                                       # schedulable is "not zero"
]


def test_reference_by_hand(O, P):
    for cont, node, want in HAND_ROWS:
        c = tuple(np.array([x], np.uint32) for x in cont)
        n = tuple(np.array([x], np.uint32) for x in node[:4]) + (np.array([node[4]], np.uint8),)
        first, count, bm = _same_as_oracles(c, n, O, P)
        assert (first.tolist(), count.tolist(), bm.tolist()) == (([0], [1], [1]) if want else ([NONE], [0], [0])), (cont, node)
    # all rows at once, every container on every node: 65 containers wide, so that the bitmap has a second word
    cont = tuple(np.array([r[0][i] for r in HAND_ROWS] * 5, np.uint32)[:65] for i in range(4))
    nodes = tuple(np.array([r[1][i] for r in HAND_ROWS], np.uint32) for i in range(4)) + \
        (np.array([r[1][4] for r in HAND_ROWS], np.uint8),)
    first, count, bm = _same_as_oracles(cont, nodes, O, P)
    assert bm.size == 2 * len(HAND_ROWS) and (bm[len(HAND_ROWS):] <= 1).all()  # word 1 holds container 64 alone
    # N = 0 and C = 0
    empty_n = tuple(np.zeros(0, np.uint32) for _ in range(4)) + (np.zeros(0, np.uint8),)
    first, count, bm = _same_as_oracles(cont, empty_n, O, P)
    assert (first == NONE).all() and (count == 0).all() and bm.size == 0
    empty_c = tuple(np.zeros(0, np.uint32) for _ in range(4))
    first, count, bm = _same_as_oracles(empty_c, nodes, O, P)
    assert first.size == count.size == bm.size == 0
    assert FR.feasibility_batch(5, 0, 2, empty_c, tuple(np.tile(x[:2], 5) for x in nodes))[0].size == 0


# ---- the conditions on the generated inputs, on the reference alone ------------------------------------------
@pytest.mark.parametrize("C,N", DEVICE_SHAPES + ((PERIOD, 2200), (PERIOD, 1089)))
def test_conditions_single(C, N):
    K.assert_conditions(K.stats(*K.case(C, N)))
    cont, nodes = K.case(C, N, mask_nodes=True)
    assert K.has_mask_node_in_every_group(nodes)
    assert all(np.array_equal(a, b) for a, b in zip(cont, K.case(C, N)[0]))  # the same containers
    first, count, _ = K.expected(C, N, mask_nodes=True, want_bitmap=False)
    assert (count >= (N + 63) // 64).all() and (first < 64).all()  # why the plain table is asserted on


@pytest.mark.parametrize("S,C,N", [k for k in BATCH_PLANS if k[1] and k[2]])
def test_conditions_batch(S, C, N):
    """Over the whole batch, that is over the pool of scenarios it repeats: a pool too small to meet the
    conditions would be repeated S / P times and still miss them."""
    P = K.pool_of(S, C, N)
    assert P == S or (P >= 5 and P * C >= 1000)
    per_tile = P * C >= 1000  # (1, 70, 2120) is one scenario of 70 containers; its path, ranges of 64, is the grid's
    assert per_tile or (S, C, N) == (1, 70, 2120)
    total = None
    for p in range(P):
        total = K.add(total, K.stats(*K.case(C, N, seed=p)))
    K.assert_conditions(total, per_tile)
    # neighbouring scenarios differ, so a z rebase that is off by one scenario shows
    assert all(not np.array_equal(K.case(C, N, seed=p)[0][0], K.case(C, N, seed=p + 1)[0][0]) for p in range(P - 1))


def test_conditions_edge_grid():
    """The grid's cells are too small one by one (C = 1, N = 1): the shares are taken over the grid, the
    per-tile floors on every cell with a thousand containers."""
    total = None
    for C in GRID_C:
        for N in GRID_N:
            if N == 0:
                continue
            st = K.stats(*K.case(C, N))
            if C >= 1023:
                assert all(x >= 4 for x in st["tile_firsts"]) and all(x >= 1 for x in st["last_firsts"]), (C, N, st)
            st["tile_firsts"], st["last_firsts"] = [], []
            total = K.add(total, st)
            if C % 64:
                assert K.has_mask_node_in_every_group(K.case(C, N, mask_nodes=True)[1])
    K.assert_conditions(total)


def test_generator_structure():
    cont, nodes = K.case(300, 2200)
    cf, mf, lab, cu, sched = nodes
    n = np.arange(2200)
    edge = (n % 1024 == 1023) | (n == 2199)
    assert ((lab >> 23) & 1).astype(bool).tolist() == edge.tolist()
    assert (cf[edge] == NONE).all() and (mf[edge] == NONE).all() and (cu[edge] == 0).all() and sched[edge].all()
    own = ((lab >> (24 + n // 1024).astype(np.uint32)) & 1).astype(bool)
    assert own.all() and ((lab >> 27) == 0).sum() > 2000  # every node its tile's bit; no tile of this N has bits 27..31
    assert (sched[128:192] == 0).all() and (sched[9 * 64:10 * 64] == 0).all()  # whole cordoned groups
    assert (sched[1000:1023] == 0).all() and (sched[1024:1051] == 0).all()   # the run across node 1024
    assert 0.10 < 1 - sched.mean() < 0.35
    assert set(np.unique(np.concatenate([cf, mf, cont[0], cont[1]])).tolist()) == set(K.POOL.tolist())
    assert (lab & 0x7FFFFF == 0x7FFFFF).sum() >= 10 and (np.bitwise_or.reduce(cu) == NONE) and (np.bitwise_or.reduce(cont[3]) == NONE)
    cpu, mem, req, conf = K.case(1100, 1089)[0]
    assert 0.4 < (req & 0x7FFFFF == 0).mean() < 0.6 and 0.4 < (req >> 24 != 0).mean() < 0.6  # ordinary bits, a tile bit
    assert 0.05 < ((req >> 23) & 1).mean() < 0.2 and (req == NONE).sum() >= 3 and (conf == NONE).sum() >= 3
