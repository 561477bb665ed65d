"""numpy restatement of SPEC.md 2.13 (re-planning a running stage).

TEST INFRASTRUCTURE ONLY: the reference the HIP kernel (fleetflow_amd/csrc/fp_replan.hip) is compared with; never
imported by the product package.  Pass 1 (seats) is written out; pass 2 is one policy_ref.place call on the
containers that are neither CYCLE nor kept, in their original relative order -- the subset's 2.3 order is the
restriction of the full one -- on the node table and counts pass 1 left.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R

NONE = 0xFFFFFFFF
KEPT, NEW, MOVED, LOST, ABSENT = 0, 1, 2, 3, 4
MOVED_CPU, MOVED_MEM, WORDS = 5, 6, 8


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def replan(cont, nodes, prev, strategy=0, preferred=0, level=None, node_count=None):
    """cont = (cpu, mem, req, conf); nodes = (cf, mf, lab, cu, sched), the base table -- copied, not mutated;
    prev [C].  Returns (assign, reason, change, summary [8], nodes_after, node_count_after): node_count_after
    is the counts the call ends with (from zero when node_count is None)."""
    assert strategy in R.STRATEGIES
    cpu, mem, req, conf = (_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x).copy() for x in nodes[:4])
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    C, N = cpu.size, cf.size
    prev = _u32(prev).reshape(-1)
    assert prev.size == C and all(p < N or p == NONE for p in prev.tolist())
    cnt = _u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    lv = _u32(level) if level is not None else None
    cycle = (lv == NONE) if lv is not None else np.zeros(C, bool)
    assign = np.full(C, NONE, np.uint32)
    reason = np.zeros(C, np.uint8)
    change = np.zeros(C, np.uint8)
    kept = np.zeros(C, bool)
    # ---- pass 1: seats, in the 2.3 order; the 2.3 predicate without the schedulable term ----
    for i in R.ffd_order(cpu, mem):
        if cycle[i] or prev[i] == NONE:
            continue
        n = int(prev[i])
        if cf[n] >= cpu[i] and mf[n] >= mem[i] and (lab[n] & req[i]) == req[i] and (cu[n] & conf[i]) == 0:
            cf[n:n + 1] -= cpu[i]
            mf[n:n + 1] -= mem[i]
            cu[n] |= conf[i]
            cnt[n:n + 1] += np.uint32(1)
            kept[i] = True
            assign[i] = n
    # ---- pass 2: 2.6 on the rest, on the state pass 1 left ----
    rest = np.flatnonzero(~cycle & ~kept)
    a, r, after, cnt = R.place(tuple(x[rest] for x in (cpu, mem, req, conf)), (cf, mf, lab, cu, sched), strategy,
                               preferred, node_count=cnt)
    assign[rest] = a
    reason[rest] = r
    reason[cycle] = 2
    had = prev != NONE
    placed = assign != NONE
    change[placed & ~kept & ~had] = NEW
    change[placed & ~kept & had] = MOVED
    change[~placed & had] = LOST
    change[~placed & ~had] = ABSENT
    summary = np.zeros(WORDS, np.uint32)
    for v in range(5):
        summary[v] = int((change == v).sum())
    moved = change == MOVED
    summary[MOVED_CPU] = int(cpu[moved].astype(np.uint64).sum()) & 0xFFFFFFFF
    summary[MOVED_MEM] = int(mem[moved].astype(np.uint64).sum()) & 0xFFFFFFFF
    return assign, reason, change, summary, after, cnt


def cost(assign, reason, scenario_id):
    """SPEC.md 2.4 over the re-plan: rejected = NOFIT + CYCLE, used = the distinct nodes that hold a container
    (every assigned container was seated or placed by this call)."""
    return R.cost(assign, reason, scenario_id)
