"""numpy restatement of SPEC.md 2.16 (scale-in sweep).

TEST INFRASTRUCTURE ONLY: the reference the HIP sweep (fleetflow_amd/csrc/fp_shrink.hip) is compared with;
never imported by the product package.  Each attempt is ONE ``policy_ref.place`` call, with the containers now
on the tried node (in index order, so place's (cpu desc, mem desc, index asc) is the visiting order) and the
masked ``schedulable``, on the variant's current table; its result is committed or discarded.  SPEC.md 2.6 is
not restated here.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
RELEASED, TRIED, FAILED, MOVES, MOVED, MOVED_CPU, MOVED_MEM, FIRST_FAILED, WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8
ST_NEVER, ST_RELEASED, ST_FAILED = 0, 1, 2


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def variant(cont, nodes, assign, order, strategy=0, preferred=0, node_count=None):
    """One release order.  Returns (assign_out [C], state [N], blocker [N], summary [8], trace, final) where trace
    holds one (node, committed, moves made before the attempt ended) per attempt and final = (node table,
    node_count) the variant ends with.  The inputs are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x).copy() for x in nodes[:4])
    sched0 = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    assign = _u32(assign)
    N, C = cf.size, assign.size
    assert ((assign < N) | (assign == NONE)).all()
    cnt = _u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    cur = assign.copy()
    gone = np.zeros(N, bool)
    state = np.zeros(N, np.uint8)
    blocker = np.full(N, NONE, np.uint32)
    summary = np.zeros(WORDS, np.uint32)
    summary[FIRST_FAILED] = NONE
    trace = []
    for n in (int(x) for x in np.asarray(order, dtype=np.uint64).reshape(-1)):
        assert n < N or n == NONE
        if n == NONE or gone[n]:
            continue
        summary[TRIED] += 1
        ev = np.flatnonzero(cur == n)
        sched = sched0 * ~gone
        sched[n] = 0
        a, _, after, cnt_after = policy_ref.place(tuple(x[ev] for x in cont), (cf, mf, lab, cu, sched), strategy,
                                                  preferred, node_count=cnt)
        if (a != NONE).all():
            cf, mf, _, cu, _ = after
            cnt = cnt_after
            cur[ev] = a
            gone[n] = True
            state[n] = ST_RELEASED
            blocker[n] = NONE
            summary[RELEASED] += 1
            summary[MOVES] += ev.size
            trace.append((n, True, int(ev.size)))
        else:  # the call's result is discarded; the blocker is the first unplaced evictee in the visiting order
            # (place goes on after it, but up to it the call is the attempt)
            perm = policy_ref.ffd_order(cont[0][ev], cont[1][ev])
            at = int(np.flatnonzero(a[perm] == NONE)[0])
            state[n] = ST_FAILED
            blocker[n] = ev[perm[at]]
            summary[FAILED] += 1
            if summary[FIRST_FAILED] == NONE:
                summary[FIRST_FAILED] = n
            trace.append((n, False, at))
    moved = np.flatnonzero(cur != assign)
    summary[MOVED] = moved.size
    summary[MOVED_CPU] = int(cont[0][moved].astype(np.uint64).sum()) & 0xFFFFFFFF
    summary[MOVED_MEM] = int(cont[1][moved].astype(np.uint64).sum()) & 0xFFFFFFFF
    return cur, state, blocker, summary, trace, ((cf, mf, lab, cu, sched0 * ~gone), cnt)


def sweep(cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None):
    """try_order [n_var][n_try].  Returns (assign_out [n_var, C], state [n_var, N], blocker [n_var, N],
    summary [n_var, 8])."""
    tro = np.asarray(try_order, dtype=np.uint64)
    tro = tro.reshape(tro.shape[0], -1) if tro.ndim == 2 else tro.reshape(len(try_order), -1)
    C, N = _u32(assign).size, _u32(nodes[0]).size
    out = np.empty((tro.shape[0], C), np.uint32)
    state = np.empty((tro.shape[0], N), np.uint8)
    blocker = np.empty((tro.shape[0], N), np.uint32)
    summary = np.empty((tro.shape[0], WORDS), np.uint32)
    for v in range(tro.shape[0]):
        out[v], state[v], blocker[v], summary[v] = variant(cont, nodes, assign, tro[v], strategy, preferred, node_count)[:4]
    return out, state, blocker, summary


def random_case(seed, strategy, C=300, N=40):
    """300 containers placed with SPREAD on 40 nodes, 90 % schedulable; the order is `fewest`.  Returns (cont, live
    node table, assign, counts, order), read-only.  ``strategy`` is the one the caller shrinks under: it names
    the case and does not change the inputs."""
    rng = np.random.default_rng(1000 + seed)
    cont = (rng.integers(50, 901, C).astype(np.uint32), rng.integers(64, 2049, C).astype(np.uint32),
            np.where(rng.random(C) < 0.3, 1 << rng.integers(0, 3, C), 0).astype(np.uint32),
            np.where(rng.random(C) < 0.2, 1 << rng.integers(0, 8, C), 0).astype(np.uint32))
    nodes = (np.full(N, 8000, np.uint32), np.full(N, 16384, np.uint32), rng.integers(0, 8, N).astype(np.uint32),
             np.zeros(N, np.uint32), (rng.random(N) < 0.9).astype(np.uint8))
    assign, _, live, cnt = policy_ref.place(cont, nodes, policy_ref.SPREAD)
    count = np.bincount(assign[assign != NONE], minlength=N)
    order = np.lexsort((np.arange(N), count)).astype(np.uint32)
    for a in (*cont, *live, assign, cnt, order):
        a.setflags(write=False)
    return cont, live, assign, cnt, order


def pad(orders, n_try=None):
    """Ragged release orders as the [n_var, n_try] array of the ABI, NONE-padded."""
    n_try = max([len(o) for o in orders] + [n_try or 0])
    out = np.full((len(orders), n_try), NONE, np.uint32)
    for v, o in enumerate(orders):
        out[v, :len(o)] = o
    return out
