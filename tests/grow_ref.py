"""numpy restatement of SPEC.md 2.12 (scale-out sweep).

TEST INFRASTRUCTURE ONLY: the reference the HIP sweep (fleetflow_amd/csrc/fp_grow.hip) is compared with;
never imported by the product package.  Each candidate is ONE ``policy_ref.place`` call (FIRST_FIT) with the
pending containers (in index order, so place's (cpu desc, mem desc, index asc) is the visiting order) on the
candidate's table of ``t_max[k]`` identical empty servers: SPEC.md 2.3 is not restated here.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
PENDING, PLACED, OPENED, UNPLACEABLE, CAPPED, LEFT_CPU, LEFT_MEM, FIRST_UNPLACED, WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8
MAX_NEW = 8192


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def pending(C, reason, reason_mask):
    """The indices of the pending containers, ascending."""
    if reason_mask == 0:
        return np.arange(C)
    r = np.ascontiguousarray(reason, dtype=np.uint8).astype(np.uint32)
    assert r.size == C
    return np.flatnonzero((r < 32) & (((np.uint32(reason_mask) >> np.minimum(r, 31)) & 1) != 0))


def template_table(t_cpu, t_mem, t_labels, m):
    """``m`` empty servers of one template as a node table."""
    return (np.full(m, t_cpu, np.uint32), np.full(m, t_mem, np.uint32), np.full(m, t_labels, np.uint32),
            np.zeros(m, np.uint32), np.ones(m, np.uint8))


def sweep(cont, reason, templates, max_new, reason_mask=1 << 1, t_max=None):
    """Returns (summary [n_cand, 8], assign [n_cand, C]).  The inputs are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    t_cpu, t_mem, t_lab = (_u32(x).reshape(-1) for x in templates)
    C, n_cand = cont[0].size, t_cpu.size
    assert max_new <= MAX_NEW
    tm = _u32(t_max).reshape(-1) if t_max is not None else np.full(n_cand, max_new, np.uint32)
    assert tm.size == n_cand and (tm <= max_new).all()
    pend = pending(C, reason, reason_mask)
    sub = tuple(x[pend] for x in cont)
    visit = pend[policy_ref.ffd_order(sub[0], sub[1])] if pend.size else pend
    summary = np.zeros((n_cand, WORDS), np.uint32)
    assign = np.full((n_cand, C), NONE, np.uint32)
    for k in range(n_cand):
        a, r, after, _ = policy_ref.place(sub, template_table(t_cpu[k], t_mem[k], t_lab[k], int(tm[k])),
                                          policy_ref.FIRST_FIT)
        assign[k, pend] = a
        placed = a != NONE
        opened = int(a[placed].max()) + 1 if placed.any() else 0
        never = (sub[0] > t_cpu[k]) | (sub[1] > t_mem[k]) | ((t_lab[k] & sub[2]) != sub[2])
        assert not (never & placed).any()
        row = summary[k]
        row[PENDING] = pend.size
        row[PLACED] = int(placed.sum())
        row[OPENED] = opened
        row[UNPLACEABLE] = int(never.sum())
        row[CAPPED] = int((~placed & ~never).sum())
        row[LEFT_CPU] = int(after[0][:opened].astype(np.uint64).sum()) & 0xFFFFFFFF
        row[LEFT_MEM] = int(after[1][:opened].astype(np.uint64).sum()) & 0xFFFFFFFF
        lost = visit[assign[k, visit] == NONE]
        row[FIRST_UNPLACED] = lost[0] if lost.size else NONE
    return summary, assign
