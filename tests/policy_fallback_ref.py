"""numpy restatement of SPEC.md 2.8 (scored placement under a fallback chain).

TEST INFRASTRUCTURE ONLY: the reference the FB variants of the HIP placer (fleetflow_amd/csrc/fp_policy.hip,
k_policy<.., .., true>) are compared with; never imported by the product package.  Built on policy_ref.py
(SPEC.md 2.6) and policy_spread_ref.py (2.7): the same order, capacity and conflict tests, key, skew test
and reasons, with the label test relaxed hop by hop.

Two statements of the same rule: ``place`` tries hop 0, 1, ... and takes the first hop that has a feasible
node (the iterative form; the one the GPU is compared with), ``place_per_node`` gives every node its hop and
takes the (hop, key) minimum.  The CPU tests compare the two.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
import policy_spread_ref as SR

NONE = R.NONE
MAX_HOPS = 4
_M32 = 0xFFFFFFFF


def cumulative(relax_mask, n_hops):
    """cum[0 .. n_hops]: cum[0] = 0, cum[h] = cum[h-1] | relax_mask[h-1]."""
    assert 0 <= n_hops <= MAX_HOPS and len(relax_mask) >= n_hops
    cum = [0]
    for h in range(n_hops):
        cum.append(cum[-1] | (int(relax_mask[h]) & _M32))
    return cum


def _place(cont, nodes, strategy, preferred, level, node_count, domain, max_skew, relax_mask, n_hops, per_node):
    assert strategy in R.STRATEGIES
    n_hops, max_skew = int(n_hops), int(max_skew)
    if n_hops == 0:  # no fallback: SPEC.md 2.7 (or 2.6) itself, relax_mask is not read
        a, r, after, cnt = SR.place(cont, nodes, strategy, preferred=preferred, level=level, node_count=node_count,
                                    domain=domain, max_skew=max_skew)
        return a, r, np.zeros(a.size, np.uint8), after, cnt
    cum = cumulative(relax_mask, n_hops)
    cpu, mem, req, conf = (R._u32(x) for x in cont)
    cf, mf, lab, cu = (R._u32(x).copy() for x in nodes[:4])
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    C, N = cpu.size, cf.size
    spread = domain is not None and max_skew != 0
    cnt = R._u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    lv = R._u32(level) if level is not None else None
    assign = np.full(C, NONE, np.uint32)
    reason = np.zeros(C, np.uint8)
    hops = np.zeros(C, np.uint8)
    ok_s = sched != 0
    if spread:
        dom = R._u32(domain)
        assert dom.size == N and (N == 0 or int(dom.max()) < SR.MAX_DOMAINS)
        dc = np.zeros(SR.MAX_DOMAINS, np.uint64)
        np.add.at(dc, dom, cnt.astype(np.uint64))
        dc &= np.uint64(_M32)
        elig = np.zeros(SR.MAX_DOMAINS, bool)
        elig[dom[ok_s]] = True
    idx = np.arange(N, dtype=np.uint64)
    miss = R.popcount32(np.uint32(preferred & _M32) & ~lab) << np.uint64(58)
    for i in R.ffd_order(cpu, mem):
        if lv is not None and lv[i] == NONE:
            reason[i] = 2
            continue
        c, m, r, x = cpu[i], mem[i], req[i], conf[i]
        base = ok_s & (cf >= c) & (mf >= m) & ((cu & x) == 0)  # 2.3 without the label test
        passes = np.ones(N, bool)
        if spread and elig.any():
            mn = dc[elig].min()
            passes = (((dc - mn) & np.uint64(_M32)) < np.uint64(max_skew))[dom]
        if strategy == R.SPREAD:
            prim = cnt
        elif strategy == R.PACK:
            prim = cf - c
        elif strategy == R.FILL_LOWEST:
            prim = ~cf
        else:
            prim = np.zeros(N, np.uint32)
        key = miss | (prim.astype(np.uint64) << np.uint64(26)) | idx
        req_h = [np.uint32(int(r) & ~cu_h & _M32) for cu_h in cum]
        lab_ok = [(lab & q) == q for q in req_h]  # lab_ok[h]: the node matches the requirement of hop h
        n = hop = None
        if per_node:
            # hop(n) = the smallest h whose requirement the node matches; the (hop, key) minimum
            node_hop = np.full(N, n_hops + 1, np.int64)
            for h in range(n_hops, -1, -1):
                node_hop[lab_ok[h]] = h
            ok = base & passes & (node_hop <= n_hops)
            if ok.any():
                cand = np.flatnonzero(ok)
                best = cand[np.lexsort((key[cand], node_hop[cand]))[0]]
                n, hop = int(best), int(node_hop[best])
        else:
            # the first hop at which any node is feasible; there, the 2.6 key decides
            for h in range(n_hops + 1):
                ok = base & passes & lab_ok[h]
                if ok.any():
                    n, hop = int(np.argmin(np.where(ok, key, R._INFEASIBLE))), h
                    break
        if n is None:
            # NOFIT: no node fits by 2.3 even under req_{n_hops}; SKEW: some does, none passes the skew test
            reason[i] = SR.REASON_SKEW if (base & lab_ok[n_hops]).any() else 1
            continue
        assign[i] = n
        hops[i] = hop
        cf[n] -= c
        mf[n] -= m
        cu[n] |= x
        cnt[n:n + 1] += np.uint32(1)  # u32, wraps
        if spread:
            dc[dom[n]] = (dc[dom[n]] + np.uint64(1)) & np.uint64(_M32)
    return assign, reason, hops, (cf, mf, lab, cu, sched), cnt


def place(cont, nodes, strategy, preferred=0, level=None, node_count=None, domain=None, max_skew=0, relax_mask=(),
          n_hops=None):
    """As policy_spread_ref.place, with relax_mask (per hop, the label bits it gives up) and n_hops (None =
    every mask given).  Returns (assign, reason, hops, nodes_after, node_count_after).  The iterative form."""
    n_hops = len(relax_mask) if n_hops is None else n_hops
    return _place(cont, nodes, strategy, preferred, level, node_count, domain, max_skew, relax_mask, n_hops, False)


def place_per_node(cont, nodes, strategy, preferred=0, level=None, node_count=None, domain=None, max_skew=0,
                   relax_mask=(), n_hops=None):
    """The same rule stated per node: every node gets its hop, the (hop(n), key(n)) minimum wins."""
    n_hops = len(relax_mask) if n_hops is None else n_hops
    return _place(cont, nodes, strategy, preferred, level, node_count, domain, max_skew, relax_mask, n_hops, True)


cost = R.cost  # SPEC.md 2.4 is unchanged: a relaxed placement counts as placed
