"""numpy restatement of SPEC.md 2.19 (the rebalance sweep).

TEST INFRASTRUCTURE ONLY: the reference the HIP kernel (fleetflow_amd/csrc/fp_rebalance.hip) is compared with; never
imported by the product package.  It restates neither 2.6, 2.7 nor 2.8: an attempt is ONE ``policy_fallback_ref.place``
call with C = 1 on the lifted table (theorem D), and everything else here is the pass over the victim order, the
lift and its reversal.  ``skew`` and ``excess`` are functions of their own, so that the tests can evaluate them on
any state.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_ref as FR  # noqa: E402
import policy_ref  # noqa: E402

NONE = 0xFFFFFFFF
NOFIT, SKEW = 1, 3
MAX_DOMAINS = 64
_M32 = 0xFFFFFFFF
# the word indices of a variant's summary row (fleetplace.h FP_REBAL_*)
MOVES, STUCK, STUCK_SKEW, RELAXED, MOVED_CPU, MOVED_MEM, SKEW_BEFORE, SKEW_AFTER, WORDS = range(9)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def dom_counts(count, domain, sched):
    """(dom_count [64] as python ints mod 2^32 over ALL nodes of each domain, eligible [64] bool)."""
    dc = np.zeros(MAX_DOMAINS, np.uint64)
    np.add.at(dc, _u32(domain), _u32(count).astype(np.uint64))
    dc &= np.uint64(_M32)
    elig = np.zeros(MAX_DOMAINS, bool)
    elig[_u32(domain)[np.asarray(sched) != 0]] = True
    return dc.astype(np.int64), elig


def skew(count, domain, sched):
    """max - min of dom_count over the eligible domains, 0 without one."""
    dc, elig = dom_counts(count, domain, sched)
    return int(dc[elig].max() - dc[elig].min()) if elig.any() else 0


def heavy(count, domain, sched, max_skew):
    """[64] bool: the domain is eligible and dom_count - min > max_skew."""
    dc, elig = dom_counts(count, domain, sched)
    if not elig.any():
        return np.zeros(MAX_DOMAINS, bool)
    return elig & (dc - dc[elig].min() > max_skew)


def excess(count, domain, sched, max_skew):
    """sum over the eligible domains of max(0, dom_count - min - max_skew)."""
    dc, elig = dom_counts(count, domain, sched)
    if not elig.any():
        return 0
    return int(np.maximum(0, dc[elig] - dc[elig].min() - max_skew).sum())


def derived_count(assign, N):
    a = _u32(assign)
    return np.bincount(a[a != NONE].astype(np.int64), minlength=N).astype(np.uint32)


def variant(cont, nodes, assign, order, budget=NONE, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
            relax_mask=(), step=None):
    """One victim order.  Returns (assign_out, hops, reason, summary row, trace, final state): the trace holds one
    (position, container, source, outcome, target, hop) per attempt with outcome "MOVE", "NOFIT" or "SKEW"; the
    final state is ((cpu_free, mem_free, labels, conflict_used, schedulable), node_count).  ``step``, if given, is
    called as step(count, moved_from, moved_to) after every move with the state it left (for the theorems)."""
    cpu, mem, req, conf = (_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x).copy() for x in nodes[:4])
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    N, C = cf.size, cpu.size
    cur = _u32(assign).copy()
    cnt = _u32(node_count).copy() if node_count is not None else derived_count(cur, N)
    hops, reason = np.zeros(C, np.uint8), np.zeros(C, np.uint8)
    row = np.zeros(WORDS, np.uint32)
    trace = []
    relax = [int(m) for m in relax_mask]
    if domain is None or int(max_skew) == 0:  # the degenerate form: nothing is heavy, domain is not read
        return cur, hops, reason, row, trace, ((cf, mf, lab, cu, sched), cnt)
    dom = _u32(domain)
    max_skew, budget = int(max_skew), int(budget)
    row[SKEW_BEFORE] = skew(cnt, dom, sched)
    for i, c in enumerate(_u32(order).reshape(-1).tolist()):
        if int(row[MOVES]) == budget:
            break
        if c == NONE or cur[c] == NONE:
            continue
        s = int(cur[c])
        if not heavy(cnt, dom, sched, max_skew)[dom[s]]:
            continue
        # ---- lift ----
        saved = (cf[s], mf[s], cu[s], cnt[s])
        cf[s:s + 1] += cpu[c]
        mf[s:s + 1] += mem[c]
        cu[s] &= ~conf[c]
        cnt[s:s + 1] -= np.uint32(1)
        # ---- place: the only container of a 2.8 call on that state ----
        a1, r1, h1, after, cnt1 = FR.place(tuple(x[c:c + 1] for x in (cpu, mem, req, conf)), (cf, mf, lab, cu, sched),
                                           strategy, preferred=preferred, node_count=cnt, domain=dom, max_skew=max_skew,
                                           relax_mask=relax)
        if a1[0] == NONE:  # ---- rejection: exactly the state before the lift ----
            cf[s], mf[s], cu[s], cnt[s] = saved
            reason[c] = r1[0]
            row[STUCK] += 1
            row[STUCK_SKEW] += int(r1[0] == SKEW)
            trace.append((i, c, s, "SKEW" if r1[0] == SKEW else "NOFIT", NONE, 0))
            continue
        t = int(a1[0])
        cf, mf, cu, cnt = after[0], after[1], after[3], cnt1
        cur[c], hops[c], reason[c] = t, h1[0], 0
        row[MOVES] += 1
        row[RELAXED] += int(h1[0] != 0)
        row[MOVED_CPU:MOVED_CPU + 1] += cpu[c]  # u32, wraps
        row[MOVED_MEM:MOVED_MEM + 1] += mem[c]
        trace.append((i, c, s, "MOVE", t, int(h1[0])))
        if step is not None:
            step(cnt, s, t)
    row[SKEW_AFTER] = skew(cnt, dom, sched)
    return cur, hops, reason, row, trace, ((cf, mf, lab, cu, sched), cnt)


def sweep(cont, nodes, assign, victim_order, strategy=0, preferred=0, node_count=None, domain=None, max_skew=0,
          relax_mask=(), max_moves=None):
    """Planner.rebalance_sweep's results: (assign_out [n_var, C], hops, reason, summary [n_var, 8])."""
    vo = _u32(victim_order)
    C = _u32(cont[0]).size
    outs = [variant(cont, nodes, assign, vo[v], NONE if max_moves is None else max_moves[v], strategy, preferred,
                    node_count, domain, max_skew, relax_mask) for v in range(vo.shape[0])]
    stack = lambda k, dt, w: (np.stack([o[k] for o in outs]) if outs else np.zeros((0, w), dt))  # noqa: E731
    return stack(0, np.uint32, C), stack(1, np.uint8, C), stack(2, np.uint8, C), stack(3, np.uint32, WORDS)


def pad(orders, n_try=None):
    """Ragged victim orders as the [n_var, n_try] array of the ABI, NONE-padded."""
    n_try = max([len(o) for o in orders] + [n_try or 0])
    out = np.full((len(orders), n_try), NONE, np.uint32)
    for v, o in enumerate(orders):
        out[v, :len(o)] = o
    return out


ORDERS = ("smallest", "largest", "newest")


def order_of(rule, cont):
    """flow.rebalance_order's three rules on a container table (stage order = index order)."""
    cpu, mem = _u32(cont[0]), _u32(cont[1])
    idx = np.arange(cpu.size)
    if rule == "smallest":
        return np.lexsort((idx, mem, cpu)).astype(np.uint32)
    if rule == "largest":
        return policy_ref.ffd_order(cpu, mem).astype(np.uint32)
    assert rule == "newest"
    return idx[::-1].astype(np.uint32)


def random_case(seed, C=300, N=40, n_dom=4, max_skew=2, relax_mask=(1, 2), cpu=8000, mem=16384, taken=None, zone=0):
    """shrink_policy_ref.random_case's tables, with the nodes of domain ``zone`` unschedulable while the plan is made
    (a drained zone) and schedulable again in the live table, their capacity partly taken by other tenants'
    services (``taken``: the share of it, None = by the seed: a third of the seeds leave the zone too little room
    for what the bound asks).  Returns (cont, live node table, assign, counts, domain, pre-plan node table),
    read-only; the pre-plan table is the live one before the plan's requests were taken from it."""
    rng = np.random.default_rng(1900 + seed)
    cont = (rng.integers(50, 901, C).astype(np.uint32), rng.integers(64, 2049, C).astype(np.uint32),
            np.where(rng.random(C) < 0.4, 1 << rng.integers(0, 3, C), 0).astype(np.uint32),
            np.where(rng.random(C) < 0.2, 1 << rng.integers(0, 8, C), 0).astype(np.uint32))
    domain = (np.arange(N) % n_dom).astype(np.uint32)
    base_sched = (rng.random(N) < 0.9).astype(np.uint8)
    base_sched[zone] = 1  # the zone comes back with at least one schedulable node
    if taken is None:
        taken = (0.3, 0.6, 0.93)[seed % 3]
    cf, mf = np.full(N, cpu, np.uint32), np.full(N, mem, np.uint32)
    inz = domain == zone
    cf[inz] = (cf[inz] * (1 - taken * rng.uniform(0.8, 1.0, int(inz.sum())))).astype(np.uint32)
    mf[inz] = (mf[inz] * (1 - taken * rng.uniform(0.8, 1.0, int(inz.sum())))).astype(np.uint32)
    plan_nodes = (cf, mf, rng.integers(0, 8, N).astype(np.uint32), np.zeros(N, np.uint32),
                  np.where(inz, 0, base_sched).astype(np.uint8))
    assign, _, _, after, cnt = FR.place(cont, plan_nodes, policy_ref.SPREAD, domain=domain, max_skew=max_skew,
                                        relax_mask=list(relax_mask))
    live = (after[0], after[1], after[2], after[3], base_sched)
    pre = plan_nodes[:4] + (base_sched,)
    for a in (*cont, *live, *pre, assign, cnt, domain):
        a.setflags(write=False)
    return cont, live, assign, cnt, domain, pre


CONDITIONS = ("a move", "a relaxed move", "a SKEW rejection", "a move after a rejection", "restored into bound",
              "ends out of bound")


def conditions(trace, row, max_skew):
    """Which of the six conditions of the test plan a variant shows."""
    seen, rejected = set(), False
    for _, _, _, what, _, hop in trace:
        if what == "MOVE":
            seen.add("a move")
            if hop:
                seen.add("a relaxed move")
            if rejected:
                seen.add("a move after a rejection")
        else:
            rejected = True
            if what == "SKEW":
                seen.add("a SKEW rejection")
    if row[SKEW_BEFORE] > max_skew:
        seen.add("restored into bound" if row[SKEW_AFTER] <= max_skew else "ends out of bound")
    return seen
