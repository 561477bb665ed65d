"""Stage-2 feasibility sweep (SPEC.md 2.3's predicate, 2.5's outputs) in plain numpy.  TEST INFRASTRUCTURE ONLY.

Independent of the C oracle: every input is widened to uint64, the predicate is written out once, and the
outputs are taken from the [C, N] matrix.  ``feas_plan`` restates the launch arithmetic of fp_feas.hip, so that
a test can say which path of k_feas a shape takes; test_feas_host.py pins its constants to the kernel's.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
CHUNK_PAIRS = 1 << 23  # pairs per [c, N] slab: its widest temporaries are two uint64 matrices, 128 MB together

# fp_feas.hip: threads per block, containers per thread, nodes per LDS tile, and the grid size below which the
# node range is split further
K_BLOCK, K_PER, K_TILE, SPLIT_BELOW = 256, 4, 1024, 2048


def _wide(cont, nodes):
    cpu, mem, req, conf = (np.asarray(x).astype(np.uint64) for x in cont)
    cf, mf, lab, cu = (np.asarray(x).astype(np.uint64) for x in nodes[:4])
    return (cpu, mem, req, conf), (cf, mf, lab, cu, np.asarray(nodes[4]).astype(np.uint64))


def predicates(cont, nodes):
    """The five conditions of SPEC 2.3 as bool [C, N] matrices: (schedulable, cpu, mem, labels, conflict)."""
    (cpu, mem, req, conf), (cf, mf, lab, cu, sched) = _wide(cont, nodes)
    C = cpu.size
    p_sched = np.broadcast_to(sched[None, :] != 0, (C, sched.size))
    p_cpu = cf[None, :] >= cpu[:, None]
    p_mem = mf[None, :] >= mem[:, None]
    p_lab = (req[:, None] & ~lab[None, :] & np.uint64(0xFFFFFFFF)) == 0
    p_conf = (cu[None, :] & conf[:, None]) == 0
    return p_sched, p_cpu, p_mem, p_lab, p_conf


def ok_matrix(cont, nodes):
    """ok[c, n], bool [C, N]."""
    p = predicates(cont, nodes)
    return p[0] & p[1] & p[2] & p[3] & p[4]


def _chunks(C, N):
    step = max(1, CHUNK_PAIRS // max(N, 1))
    return [(lo, min(C, lo + step)) for lo in range(0, C, step)]


def feasibility(cont, nodes, want_bitmap=True):
    """(first [C] u32, count [C] u32, bitmap [ceil(C/64) * N] u64 or None)."""
    C, N = len(cont[0]), len(nodes[0])
    first = np.full(C, NONE, np.uint32)
    count = np.zeros(C, np.uint32)
    WC = (C + 63) // 64
    padded = np.zeros((WC * 64, N), bool) if want_bitmap else None
    for lo, hi in _chunks(C, N):
        ok = ok_matrix(tuple(np.asarray(x)[lo:hi] for x in cont), nodes)
        count[lo:hi] = ok.sum(1)
        if N:
            first[lo:hi] = np.where(count[lo:hi] == 0, NONE, ok.argmax(1)).astype(np.uint32)
        if want_bitmap:
            padded[lo:hi] = ok
    if not want_bitmap:
        return first, count, None
    # word [(c / 64) * N + n], bit c % 64: pack the 64 containers of a word along the last axis
    lanes = padded.reshape(WC, 64, N).transpose(0, 2, 1)
    bitmap = np.ascontiguousarray(np.packbits(lanes, axis=-1, bitorder="little")).view("<u8").reshape(WC * N).astype(np.uint64)
    return first, count, bitmap


def feasibility_batch(S, C, N, cont, nodes):
    """Scenario-major inputs ([S*C] and [S*N]): (first [S*C], count [S*C])."""
    first = np.empty(S * C, np.uint32)
    count = np.empty(S * C, np.uint32)
    for s in range(S):
        c_s = tuple(np.asarray(x)[s * C:(s + 1) * C] for x in cont)
        n_s = tuple(np.asarray(x)[s * N:(s + 1) * N] for x in nodes)
        first[s * C:(s + 1) * C], count[s * C:(s + 1) * C], _ = feasibility(c_s, n_s, want_bitmap=False)
    return first, count


def feas_plan(S, C, N):
    """(blocks_x, ysplit, span, tiles) of the launch for ``C`` containers on ``N`` nodes: ``S`` = None is the
    single call (fp_feasibility, fp_dev_feasibility), a number the batch of that many scenarios.  ``tiles``
    lists, per blockIdx.y, the lengths of the LDS tiles a block walks; no launch (C = 0 or N = 0) has none."""
    per_block = K_BLOCK * K_PER
    blocks_x = (C + per_block - 1) // per_block
    if C == 0 or N == 0 or S == 0:
        return blocks_x, 1, 64, []
    grid = blocks_x * (1 if S is None else S)
    max_split = (N + 63) // 64
    ysplit = 1
    while grid * ysplit < SPLIT_BELOW and ysplit < max_split:
        ysplit *= 2
    ysplit = min(ysplit, max_split)
    span = (N + ysplit - 1) // ysplit
    span = (span + 63) & ~63
    ysplit = (N + span - 1) // span
    tiles = []
    for y in range(ysplit):
        y0, y1 = y * span, min(N, (y + 1) * span)
        tiles.append([min(K_TILE, y1 - n0) for n0 in range(y0, y1, K_TILE)])
    return blocks_x, ysplit, span, tiles
