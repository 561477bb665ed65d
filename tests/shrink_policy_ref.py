"""numpy restatement of SPEC.md 2.17 (the scale-in sweep under the policy's spread constraint and fallback
chain).

TEST INFRASTRUCTURE ONLY: the reference the SP / FB variants of the HIP sweep (fleetflow_amd/csrc/fp_shrink.hip,
k_shrink_sweep<.., SP, FB>) are compared with; never imported by the product package.  Each attempt is ONE
``policy_fallback_ref.place`` call over the containers now on the tried node (in index order, so place's (cpu
desc, mem desc, index asc) is the visiting order) on the variant's current table with the tried node and the
released nodes unschedulable and their ``node_count`` 0; the call is cut at its first rejection and its result
committed or discarded.  SPEC.md 2.6 to 2.8 are not restated here.  The bound rule's two skews come from ``skew``,
which shares nothing with ``place``.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_ref as FR  # noqa: E402
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
RELEASED, TRIED, FAILED, MOVES, MOVED, MOVED_CPU, MOVED_MEM, FIRST_FAILED, WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8
ST_NEVER, ST_RELEASED, ST_FAILED = 0, 1, 2
REASON_NOFIT, REASON_SKEW = 1, 3
FAILED_SKEW, RELAXED, SKEW_BEFORE, SKEW_AFTER, POLICY_WORDS = 0, 1, 2, 3, 4
_M32 = 0xFFFFFFFF


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def constrained(domain, max_skew):
    return domain is not None and int(max_skew) != 0


def skew(counts, domain, gone, targets):
    """SPEC.md 2.17's skew(S): max - min of the per-domain sums (u32, wrap) of ``counts`` over the nodes that are
    not ``gone``, taken over the domains that hold a target; 0 without one."""
    per, eligible = {}, set()
    for n, d in enumerate(_u32(domain).tolist()):
        if not gone[n]:
            per[d] = (per.get(d, 0) + int(counts[n])) & _M32
        if targets[n]:
            assert not gone[n]
            eligible.add(d)
    if not eligible:
        return 0
    vals = [per[d] for d in eligible]
    return max(vals) - min(vals)


def variant(cont, nodes, assign, order, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
            relax_mask=()):
    """One release order.  Returns (assign_out [C], state [N], blocker [N], summary [8], hops [C], blocker_reason
    [N], policy row [4], trace, final): trace holds one (node, cause, moves made before the attempt ended, moves
    at a hop >= 1, the node was its domain's last target) per attempt with cause "OK", "NOFIT", "SKEW" or
    "BOUND"; final = (node table, node_count, released mask) the variant ends with.  Inputs are not mutated."""
    cont = tuple(_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x).copy() for x in nodes[:4])
    sched0 = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    assign = _u32(assign)
    N, C = cf.size, assign.size
    assert ((assign < N) | (assign == NONE)).all() and len(relax_mask) <= FR.MAX_HOPS
    sp = constrained(domain, max_skew)
    dom = _u32(domain) if sp else None
    if sp:
        assert int(dom.max(initial=0)) < 64
    cnt = _u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    cur = assign.copy()
    gone = np.zeros(N, bool)
    state = np.zeros(N, np.uint8)
    blocker = np.full(N, NONE, np.uint32)
    why = np.zeros(N, np.uint8)
    hops = np.zeros(C, np.uint8)
    summary = np.zeros(WORDS, np.uint32)
    summary[FIRST_FAILED] = NONE
    row = np.zeros(POLICY_WORDS, np.uint32)
    if sp:
        row[SKEW_BEFORE] = skew(cnt, dom, gone, sched0 * ~gone)
    trace = []
    for n in (int(x) for x in np.asarray(order, dtype=np.uint64).reshape(-1)):
        assert n < N or n == NONE
        if n == NONE or gone[n]:
            continue
        summary[TRIED] += 1
        ev = np.flatnonzero(cur == n)
        sched = sched0 * ~gone
        sched[n] = 0
        masked = cnt.copy()
        masked[gone] = 0
        masked[n] = 0
        a, r, h, after, _ = FR.place(tuple(x[ev] for x in cont), (cf, mf, lab, cu, sched), strategy, preferred,
                                     node_count=masked, domain=dom, max_skew=max_skew if sp else 0,
                                     relax_mask=list(relax_mask))
        last = bool(sp and sched0[n] and not (sched[dom == dom[n]]).any())
        cause, at, block = "OK", int(ev.size), NONE
        if (a == NONE).any():  # cut at the first rejection of the visiting order: the blocker and its reason
            perm = policy_ref.ffd_order(cont[0][ev], cont[1][ev])
            at = int(np.flatnonzero(a[perm] == NONE)[0])
            block = int(ev[perm[at]])
            cause = "SKEW" if int(r[perm[at]]) == REASON_SKEW else "NOFIT"
            assert int(r[perm[at]]) in (REASON_NOFIT, REASON_SKEW)
        elif sp:
            left = cnt.astype(np.uint64)
            np.add.at(left, a.astype(np.int64), 1)
            left = (left & np.uint64(_M32)).astype(np.uint32)
            out = gone.copy()
            out[n] = True
            before = skew(cnt, dom, gone, sched0 * ~gone)
            aft = skew(left, dom, out, sched0 * ~out)
            if not (aft <= int(max_skew) or aft <= before):
                cause = "BOUND"
        relaxed = int((h != 0).sum()) if cause == "OK" else 0
        trace.append((n, cause, at, relaxed, last))
        if cause == "OK":
            cf, mf, _, cu, _ = after
            cnt = cnt.copy()
            np.add.at(cnt, a.astype(np.int64), np.uint32(1))
            cur[ev] = a
            hops[ev] = h
            gone[n] = True
            state[n] = ST_RELEASED
            blocker[n] = NONE
            why[n] = 0
            summary[RELEASED] += 1
            summary[MOVES] += ev.size
            row[RELAXED] += relaxed
        else:
            state[n] = ST_FAILED
            blocker[n] = block
            why[n] = REASON_NOFIT if cause == "NOFIT" else REASON_SKEW
            summary[FAILED] += 1
            row[FAILED_SKEW] += cause != "NOFIT"
            if summary[FIRST_FAILED] == NONE:
                summary[FIRST_FAILED] = n
    moved = np.flatnonzero(cur != assign)
    summary[MOVED] = moved.size
    summary[MOVED_CPU] = int(cont[0][moved].astype(np.uint64).sum()) & _M32
    summary[MOVED_MEM] = int(cont[1][moved].astype(np.uint64).sum()) & _M32
    if sp:
        row[SKEW_AFTER] = skew(cnt, dom, gone, sched0 * ~gone)
    return cur, state, blocker, summary, hops, why, row, trace, ((cf, mf, lab, cu, sched0 * ~gone), cnt, gone)


def sweep(cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
          relax_mask=()):
    """try_order [n_var][n_try].  Returns (assign_out [n_var, C], state [n_var, N], blocker [n_var, N], summary
    [n_var, 8], hops [n_var, C], blocker_reason [n_var, N], policy rows [n_var, 4])."""
    tro = np.asarray(try_order, dtype=np.uint64)
    tro = tro.reshape(tro.shape[0], -1) if tro.ndim == 2 else tro.reshape(len(try_order), -1)
    C, N, V = _u32(assign).size, _u32(nodes[0]).size, tro.shape[0]
    out = np.empty((V, C), np.uint32)
    state = np.empty((V, N), np.uint8)
    blocker = np.empty((V, N), np.uint32)
    summary = np.empty((V, WORDS), np.uint32)
    hops = np.empty((V, C), np.uint8)
    why = np.empty((V, N), np.uint8)
    rows = np.empty((V, POLICY_WORDS), np.uint32)
    for v in range(V):
        out[v], state[v], blocker[v], summary[v], hops[v], why[v], rows[v] = variant(
            cont, nodes, assign, tro[v], strategy, preferred, node_count, domain, max_skew, relax_mask)[:7]
    return out, state, blocker, summary, hops, why, rows


def random_case(seed, C=300, N=40, n_dom=4, max_skew=2, relax_mask=(1, 2), cpu=8000, mem=16384):
    """C containers placed with SPREAD under the policy on N nodes, 90 % schedulable, domain = n % n_dom.  The
    order is `fewest`, twice over, so that a node that failed is tried again on the state the others left.
    Returns (cont, live node table, assign, counts, domain, order), read-only."""
    rng = np.random.default_rng(1700 + seed)
    cont = (rng.integers(50, 901, C).astype(np.uint32), rng.integers(64, 2049, C).astype(np.uint32),
            np.where(rng.random(C) < 0.4, 1 << rng.integers(0, 3, C), 0).astype(np.uint32),
            np.where(rng.random(C) < 0.2, 1 << rng.integers(0, 8, C), 0).astype(np.uint32))
    nodes = (np.full(N, cpu, np.uint32), np.full(N, mem, np.uint32), rng.integers(0, 8, N).astype(np.uint32),
             np.zeros(N, np.uint32), (rng.random(N) < 0.9).astype(np.uint8))
    domain = (np.arange(N) % n_dom).astype(np.uint32)
    assign, _, _, live, cnt = FR.place(cont, nodes, policy_ref.SPREAD, domain=domain, max_skew=max_skew,
                                       relax_mask=list(relax_mask))
    count = np.bincount(assign[assign != NONE], minlength=N)
    once = np.lexsort((np.arange(N), count)).astype(np.uint32)
    order = np.concatenate([once, once])
    for a in (*cont, *live, assign, cnt, domain, order):
        a.setflags(write=False)
    return cont, live, assign, cnt, domain, order


CONDITIONS = ("commit with moves", "NOFIT blocker", "SKEW blocker", "bound refusal", "relaxed move",
              "fails then succeeds", "last target released")


def conditions(trace):
    """Which of the seven conditions of the issue's test plan a variant's trace shows."""
    seen, failed = set(), set()
    for n, cause, at, relaxed, last in trace:
        if cause == "OK":
            if at:
                seen.add("commit with moves")
            if relaxed:
                seen.add("relaxed move")
            if n in failed:
                seen.add("fails then succeeds")
            if last:
                seen.add("last target released")
        else:
            failed.add(n)
            seen.add({"NOFIT": "NOFIT blocker", "SKEW": "SKEW blocker", "BOUND": "bound refusal"}[cause])
    return seen


def pad(orders, n_try=None):
    """Ragged release orders as the [n_var, n_try] array of the ABI, NONE-padded."""
    n_try = max([len(o) for o in orders] + [n_try or 0])
    out = np.full((len(orders), n_try), NONE, np.uint32)
    for v, o in enumerate(orders):
        out[v, :len(o)] = o
    return out
