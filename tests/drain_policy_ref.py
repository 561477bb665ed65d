"""numpy restatement of SPEC.md 2.15 (the drain what-if sweep under the policy's spread constraint and
fallback chain).

TEST INFRASTRUCTURE ONLY: the reference the SP / FB variants of the HIP sweep (fleetflow_amd/csrc/fp_drain.hip,
k_drain_sweep<.., SP, FB>) are compared with; never imported by the product package.  Candidate k is ONE
``policy_fallback_ref.place`` call over k's evictees (in index order, so place's (cpu desc, mem desc, index asc)
is the visiting order) on the base table with ``schedulable[n] &= group[n] != k`` and ``node_count[n] = 0`` where
``group[n] == k``: SPEC.md 2.6 to 2.8 are not restated here.  The summary follows drain_ref.py.  The two skew
words are computed from the counts, independently of ``place``.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
REASON_NOFIT, REASON_SKEW = 1, 3
STRANDED_SKEW, RELAXED, SKEW_BEFORE, SKEW_AFTER, POLICY_WORDS = 0, 1, 2, 3, 4
_M32 = 0xFFFFFFFF


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def constrained(domain, max_skew):
    return domain is not None and int(max_skew) != 0


def masked(nodes, group, k, node_count):
    """Candidate k's table: (nodes with the candidate's own nodes unschedulable, counts with theirs zeroed)."""
    group = _u32(group)
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8) * (group != k)
    cnt = _u32(node_count).copy() if node_count is not None else np.zeros(group.size, np.uint32)
    cnt[group == k] = 0
    return (*nodes[:4], sched), cnt


def skew(counts, domain, targets):
    """max - min of the per-domain sums (u32, wrap) of ``counts`` over the domains that hold a target; 0
    without one.  Written on its own: it shares nothing with ``place``."""
    per, eligible = {}, set()
    for n, d in enumerate(_u32(domain).tolist()):
        per[d] = (per.get(d, 0) + int(counts[n])) & _M32
        if targets[n]:
            eligible.add(d)
    if not eligible:
        return 0
    vals = [per[d] for d in eligible]
    return max(vals) - min(vals)


def candidate(cont, nodes, assign, group, k, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
              relax_mask=()):
    """Candidate k alone: (evictees in index order, their new nodes, reasons, hops, counts after)."""
    cont = tuple(_u32(x) for x in cont)
    assign, group = _u32(assign), _u32(group)
    running = assign != NONE
    ev = np.flatnonzero(running & (group[np.where(running, assign, 0)] == k)) if group.size else np.empty(0, np.int64)
    tab, cnt = masked(nodes, group, k, node_count)
    sp = constrained(domain, max_skew)
    a, r, h, _, after = FR.place(tuple(x[ev] for x in cont), tab, strategy, preferred, node_count=cnt,
                                 domain=domain if sp else None, max_skew=max_skew if sp else 0,
                                 relax_mask=list(relax_mask))
    return ev, a, r, h, after


def sweep(cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
          relax_mask=()):
    """Returns (assign_out [C], reason [C], summary [n_cand, 8], hops [C], policy rows [n_cand, 4]).  The inputs
    are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    assign, group = _u32(assign), _u32(group)
    assert ((group < n_cand) | (group == NONE)).all() and ((assign < group.size) | (assign == NONE)).all()
    assert len(relax_mask) <= FR.MAX_HOPS
    sp = constrained(domain, max_skew)
    if sp:
        assert int(_u32(domain).max(initial=0)) < 64
    out = assign.copy()
    reason = np.zeros(assign.size, np.uint8)
    hops = np.zeros(assign.size, np.uint8)
    summary = np.zeros((n_cand, D.WORDS), np.uint32)
    summary[:, D.FIRST_STRANDED] = NONE
    rows = np.zeros((n_cand, POLICY_WORDS), np.uint32)
    for k in range(n_cand):
        ev, a, r, h, after = candidate(cont, nodes, assign, group, k, strategy, preferred, node_count, domain,
                                       max_skew, relax_mask)
        if ev.size == 0:
            continue  # rows of zeros
        out[ev] = a
        reason[ev] = r
        hops[ev] = np.where(a != NONE, h, 0)
        lost = ev[a == NONE]
        row = summary[k]
        row[D.EVICTED] = ev.size
        row[D.STRANDED] = lost.size
        row[D.STRANDED_CPU] = int(cont[0][lost].astype(np.uint64).sum()) & _M32
        row[D.STRANDED_MEM] = int(cont[1][lost].astype(np.uint64).sum()) & _M32
        row[D.TARGETS] = np.unique(a[a != NONE]).size
        if lost.size:  # the first of them in the visiting order, whatever its reason
            sub = policy_ref.ffd_order(cont[0][lost], cont[1][lost])
            row[D.FIRST_STRANDED] = lost[sub[0]]
        row[D.NODES] = int((group == k).sum())
        rows[k, STRANDED_SKEW] = int((r == REASON_SKEW).sum())
        rows[k, RELAXED] = int(((a != NONE) & (h != 0)).sum())
        if sp:
            tab, base = masked(nodes, group, k, node_count)
            moved = base.astype(np.uint64)
            np.add.at(moved, a[a != NONE].astype(np.int64), 1)
            rows[k, SKEW_BEFORE] = skew(base, domain, tab[4])
            rows[k, SKEW_AFTER] = skew(moved & np.uint64(_M32), domain, tab[4])
    return out, reason, summary, hops, rows


def live(cont, nodes, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0, relax_mask=()):
    """A live state placed under the policy: (assign, live node table, counts after)."""
    a, _, _, after, cnt = FR.place(cont, nodes, strategy, preferred, node_count=node_count, domain=domain,
                                   max_skew=max_skew, relax_mask=list(relax_mask))
    return a, after, cnt


def generated(seed, C, N, strategy, n_dom, max_skew, relax_mask=()):
    """The generator's fleet (scenario 0 of ``seed``, every flag), placed under ``domain = n % n_dom``,
    ``max_skew`` and the chain: (cont, live table, assign, counts, domain)."""
    from oracle import pyoracle as P
    cont = tuple(np.array(x, np.uint32) for x in P.gen_containers(P.scenario_seed(seed, 0), C, 7))
    nodes = P.gen_nodes(P.scenario_seed(seed, 0), N)
    nodes = tuple(np.array(x, np.uint32) for x in nodes[:4]) + (np.array(nodes[4], np.uint8),)
    domain = (np.arange(N) % n_dom).astype(np.uint32)
    assign, after, cnt = live(cont, nodes, strategy, 0, None, domain, max_skew, relax_mask)
    return cont, after, assign, cnt, domain
