"""numpy restatement of SPEC.md 2.11 (drain what-if sweep).

TEST INFRASTRUCTURE ONLY: the reference the HIP sweep (fleetflow_amd/csrc/fp_drain.hip) is compared with;
never imported by the product package.  Each candidate is ONE ``policy_ref.place`` call, with that
candidate's evictees (in index order, so place's (cpu desc, mem desc, index asc) is the visiting order)
and the masked ``schedulable``, on the base table: SPEC.md 2.6 is not restated here.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
EVICTED, STRANDED, STRANDED_CPU, STRANDED_MEM, TARGETS, FIRST_STRANDED, NODES, WORDS = 0, 1, 2, 3, 4, 5, 6, 8


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def candidate(cont, nodes, assign, group, k, strategy=0, preferred=0, node_count=None):
    """Candidate k alone: (evictees in index order, their new nodes, their reasons)."""
    cont = tuple(_u32(x) for x in cont)
    assign, group = _u32(assign), _u32(group)
    running = assign != NONE
    ev = np.flatnonzero(running & (group[np.where(running, assign, 0)] == k)) if group.size else np.empty(0, np.int64)
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8) * (group != k)
    a, r, _, _ = policy_ref.place(tuple(x[ev] for x in cont), (*nodes[:4], sched), strategy, preferred,
                                  node_count=node_count)
    return ev, a, r


def sweep(cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None):
    """Returns (assign_out [C], reason [C], summary [n_cand, 8]).  The inputs are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    assign, group = _u32(assign), _u32(group)
    assert ((group < n_cand) | (group == NONE)).all() and ((assign < group.size) | (assign == NONE)).all()
    out = assign.copy()
    reason = np.zeros(assign.size, np.uint8)
    summary = np.zeros((n_cand, WORDS), np.uint32)
    summary[:, FIRST_STRANDED] = NONE
    for k in range(n_cand):
        ev, a, r = candidate(cont, nodes, assign, group, k, strategy, preferred, node_count)
        if ev.size == 0:
            continue  # a row of zeros
        out[ev] = a
        reason[ev] = r
        lost = ev[a == NONE]
        row = summary[k]
        row[EVICTED] = ev.size
        row[STRANDED] = lost.size
        row[STRANDED_CPU] = int(cont[0][lost].astype(np.uint64).sum()) & 0xFFFFFFFF
        row[STRANDED_MEM] = int(cont[1][lost].astype(np.uint64).sum()) & 0xFFFFFFFF
        row[TARGETS] = np.unique(a[a != NONE]).size
        if lost.size:  # the first of them in the visiting order
            sub = policy_ref.ffd_order(cont[0][lost], cont[1][lost])
            row[FIRST_STRANDED] = lost[sub[0]]
        row[NODES] = int((group == k).sum())
    return out, reason, summary


def live(cont, nodes, strategy=0, preferred=0, node_count=None):
    """A live state to drain: the containers placed by policy_ref.place.  Returns (assign, live node table,
    counts after)."""
    a, _, after, cnt = policy_ref.place(cont, nodes, strategy, preferred, node_count=node_count)
    return a, after, cnt
