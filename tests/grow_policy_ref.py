"""numpy restatement of SPEC.md 2.18 (the scale-out sweep under the policy: strategy, preferred labels, spread
constraint, fallback chain and quota).

TEST INFRASTRUCTURE ONLY: the reference the HIP sweep (fleetflow_amd/csrc/fp_grow.hip, k_grow_policy<.., SP, FB>)
is compared with; never imported by the product package.  Candidate k is ONE ``policy_quota_ref.place`` call over
the pending containers (in index order, so place's (cpu desc, mem desc, index asc) is the visiting order) on the
live table followed by ``t_max[k]`` empty servers of the template, the live counts and domains in front:
SPEC.md 2.6 to 2.10 are not restated here.  The summary follows grow_ref.py, read by the reason that call gives.
The two skew words come from ``drain_policy_ref.skew``, which shares nothing with ``place``.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_policy_ref as DP  # noqa: E402
import grow_ref as G  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_quota_ref as Q  # noqa: E402
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
UNLIMITED = Q.UNLIMITED
MAX_NODES = 8192
REASON_NOFIT, REASON_SKEW, REASON_QUOTA = 1, 3, 4
ON_LIVE, RELAXED, STUCK_SKEW, STUCK_QUOTA, SKEW_BEFORE, SKEW_AFTER, POLICY_WORDS = 0, 1, 2, 3, 4, 5, 8
_M32 = 0xFFFFFFFF


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def constrained(t_domain, max_skew):
    return t_domain is not None and int(max_skew) != 0


def combined(nodes, node_count, domain, t_cpu, t_mem, t_lab, t_dom, m):
    """The live table followed by ``m`` empty servers of one template: (table, counts, domains or None)."""
    live = tuple(_u32(x) for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8).reshape(-1),)
    n = live[0].size
    more = G.template_table(t_cpu, t_mem, t_lab, m)
    tab = tuple(np.concatenate([a, b]) for a, b in zip(live, more))
    cnt = np.concatenate([_u32(node_count) if node_count is not None else np.zeros(n, np.uint32), np.zeros(m, np.uint32)])
    dom = None
    if t_dom is not None:
        dom = np.concatenate([_u32(domain) if n else np.zeros(0, np.uint32), np.full(m, t_dom, np.uint32)])
    return tab, cnt, dom


def candidate(cont, pend, nodes, template, m, strategy=0, preferred=0, node_count=None, domain=None, t_dom=None,
              max_skew=0, relax_mask=(), quota=None, quota_used=None):
    """One candidate alone, over the pending containers ``pend`` (indices, ascending) and ``m`` new servers of
    ``template`` = (cpu, mem, labels): (assign, reason, hops of the pending; table, counts, domains before;
    table and counts after)."""
    cont = tuple(_u32(x) for x in cont)
    sp = constrained(t_dom, max_skew)
    tab, cnt, dom = combined(nodes, node_count, domain, *template, t_dom if sp else None, m)
    assert tab[0].size <= MAX_NODES
    caps = tuple(UNLIMITED if q is None else int(q) for q in quota) if quota is not None else (UNLIMITED,) * 3
    a, r, h, after, cnt_after, _, _ = Q.place(
        tuple(x[pend] for x in cont), tab, strategy, caps,
        quota_used if quota is not None else None, preferred=preferred, node_count=cnt, domain=dom,
        max_skew=max_skew if sp else 0, relax_mask=list(relax_mask))
    return a, r, h, tab, cnt, dom, after, cnt_after


def sweep(cont, reason, nodes, templates, max_new, reason_mask=1 << 1, t_max=None, strategy=0, preferred=0,
          node_count=None, domain=None, t_domain=None, max_skew=0, relax_mask=(), quota=None, quota_used=None):
    """Returns (summary [n_cand, 8], policy rows [n_cand, 8], assign [n_cand, C], hops [n_cand, C], reason
    [n_cand, C]).  The inputs are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    t_cpu, t_mem, t_lab = (_u32(x) for x in templates)
    C, n_cand, N = cont[0].size, t_cpu.size, _u32(nodes[0]).size
    assert max_new <= G.MAX_NEW and N + max_new <= MAX_NODES
    tm = _u32(t_max) if t_max is not None else np.full(n_cand, max_new, np.uint32)
    assert tm.size == n_cand and (tm <= max_new).all()
    sp = constrained(t_domain, max_skew)
    td = _u32(t_domain) if sp else None
    cum = FR.cumulative(relax_mask, len(relax_mask))[-1]
    pend = G.pending(C, reason, reason_mask)
    sub = tuple(x[pend] for x in cont)
    visit = pend[policy_ref.ffd_order(sub[0], sub[1])] if pend.size else pend
    summary = np.zeros((n_cand, G.WORDS), np.uint32)
    summary[:, G.FIRST_UNPLACED] = NONE
    rows = np.zeros((n_cand, POLICY_WORDS), np.uint32)
    assign = np.full((n_cand, C), NONE, np.uint32)
    hops = np.zeros((n_cand, C), np.uint8)
    why = np.zeros((n_cand, C), np.uint8)
    if pend.size == 0:
        return summary, rows, assign, hops, why
    for k in range(n_cand):
        a, r, h, tab, cnt, dom, after, cnt_after = candidate(
            cont, pend, nodes, (t_cpu[k], t_mem[k], t_lab[k]), int(tm[k]), strategy, preferred, node_count, domain,
            td[k] if sp else None, max_skew, relax_mask, quota, quota_used)
        assign[k, pend], hops[k, pend], why[k, pend] = a, h, r
        placed = r == 0
        assert np.array_equal(placed, a != NONE)
        new = np.unique(a[placed & (a >= N)])
        req_l = sub[2] & np.uint32(~cum & _M32)
        never = (sub[0] > t_cpu[k]) | (sub[1] > t_mem[k]) | ((t_lab[k] & req_l) != req_l)
        row = summary[k]
        row[G.PENDING] = pend.size
        row[G.PLACED] = int(placed.sum())
        row[G.OPENED] = new.size
        row[G.UNPLACEABLE] = int(((r == REASON_NOFIT) & never).sum())
        row[G.CAPPED] = int(((r == REASON_NOFIT) & ~never).sum())
        row[G.LEFT_CPU] = int(after[0][new].astype(np.uint64).sum()) & _M32
        row[G.LEFT_MEM] = int(after[1][new].astype(np.uint64).sum()) & _M32
        lost = visit[why[k, visit] != 0]
        row[G.FIRST_UNPLACED] = lost[0] if lost.size else NONE
        prow = rows[k]
        prow[ON_LIVE] = int((placed & (a < N)).sum())
        prow[RELAXED] = int((placed & (h > 0)).sum())
        prow[STUCK_SKEW] = int((r == REASON_SKEW).sum())
        prow[STUCK_QUOTA] = int((r == REASON_QUOTA).sum())
        if sp:
            prow[SKEW_BEFORE] = DP.skew(cnt, dom, tab[4])
            prow[SKEW_AFTER] = DP.skew(cnt_after, dom, tab[4])
    return summary, rows, assign, hops, why
