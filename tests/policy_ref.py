"""numpy restatement of SPEC.md 2.6 (scored placement).

TEST INFRASTRUCTURE ONLY: the reference the HIP placer (fleetflow_amd/csrc/fp_policy.hip) is compared
with; never imported by the product package.  One vectorised pass over the nodes per container.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
FIRST_FIT, SPREAD, PACK, FILL_LOWEST = 0, 1, 2, 3
STRATEGIES = (FIRST_FIT, SPREAD, PACK, FILL_LOWEST)
_INFEASIBLE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def ffd_order(cpu, mem):
    """SPEC.md 2.3 step 1: (cpu_m desc, mem_mib desc, index asc)."""
    cpu, mem = _u32(cpu), _u32(mem)
    return np.lexsort((np.arange(cpu.size), -mem.astype(np.int64), -cpu.astype(np.int64)))


def popcount32(x):
    x = np.asarray(x, dtype=np.uint32).astype(np.uint64)
    n = np.zeros(x.shape, np.uint64)
    for b in range(32):
        n += (x >> np.uint64(b)) & np.uint64(1)
    return n


def place(cont, nodes, strategy, preferred=0, level=None, node_count=None):
    """cont = (cpu, mem, req, conf); nodes = (cf, mf, lab, cu, sched) -- copied, not mutated.
    Returns (assign, reason, nodes_after, node_count_after): node_count_after is the counts the call
    ends with (from zero when node_count is None)."""
    assert strategy in STRATEGIES
    cpu, mem, req, conf = (_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x).copy() for x in nodes[:4])
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    C, N = cpu.size, cf.size
    cnt = _u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    lv = _u32(level) if level is not None else None
    assign = np.full(C, NONE, np.uint32)
    reason = np.zeros(C, np.uint8)
    ok_s = sched != 0
    idx = np.arange(N, dtype=np.uint64)
    miss = popcount32(np.uint32(preferred & 0xFFFFFFFF) & ~lab) << np.uint64(58)
    for i in ffd_order(cpu, mem):
        if lv is not None and lv[i] == NONE:
            reason[i] = 2
            continue
        c, m, r, x = cpu[i], mem[i], req[i], conf[i]
        ok = ok_s & (cf >= c) & (mf >= m) & ((lab & r) == r) & ((cu & x) == 0)
        if strategy == SPREAD:
            prim = cnt
        elif strategy == PACK:
            prim = cf - c  # wraps only on infeasible nodes
        elif strategy == FILL_LOWEST:
            prim = ~cf
        else:
            prim = np.zeros(N, np.uint32)
        key = np.where(ok, miss | (prim.astype(np.uint64) << np.uint64(26)) | idx, _INFEASIBLE)
        n = int(np.argmin(key)) if N else 0
        if N == 0 or key[n] == _INFEASIBLE:
            reason[i] = 1
            continue
        assign[i] = n
        cf[n] -= c
        mf[n] -= m
        cu[n] |= x
        cnt[n:n + 1] += np.uint32(1)  # u32, wraps
    return assign, reason, (cf, mf, lab, cu, sched), cnt


def cost(assign, reason, scenario_id):
    """SPEC.md 2.4 over this call's plan: rejected = NOFIT + CYCLE, used = distinct nodes assigned."""
    assign = _u32(assign)
    rej = int((np.asarray(reason) != 0).sum())
    used = int(np.unique(assign[assign != NONE]).size)
    return (min(rej, 0xFFFFFF) << 40) | (min(used, 0xFFFFFF) << 16) | (scenario_id & 0xFFFF)
