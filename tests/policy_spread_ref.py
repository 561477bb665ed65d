"""numpy restatement of SPEC.md 2.7 (scored placement under a hard topology spread).

TEST INFRASTRUCTURE ONLY: the reference the constrained variant of the HIP placer
(fleetflow_amd/csrc/fp_policy.hip, k_policy<.., true>) is compared with; never imported by the product
package.  Built on policy_ref.py (SPEC.md 2.6): the same order, predicate and key, with the skew test
beside the predicate and the SKEW reason.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R

NONE = R.NONE
MAX_DOMAINS = 64
REASON_SKEW = 3
_M32 = 0xFFFFFFFF


def place(cont, nodes, strategy, preferred=0, level=None, node_count=None, domain=None, max_skew=0, trace=None):
    """As policy_ref.place, with domain [N] (ids < 64) and max_skew (u32).  max_skew = 0 or no domain is
    SPEC.md 2.6 itself.  ``trace`` (a list) receives, after every placement, the u32 dom_count array."""
    assert strategy in R.STRATEGIES
    max_skew = int(max_skew)
    assert 0 <= max_skew <= _M32
    if domain is None or max_skew == 0:
        return R.place(cont, nodes, strategy, preferred=preferred, level=level, node_count=node_count)
    cpu, mem, req, conf = (R._u32(x) for x in cont)
    cf, mf, lab, cu = (R._u32(x).copy() for x in nodes[:4])
    sched = np.ascontiguousarray(nodes[4], dtype=np.uint8)
    dom = R._u32(domain)
    C, N = cpu.size, cf.size
    assert dom.size == N and (N == 0 or int(dom.max()) < MAX_DOMAINS)
    cnt = R._u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
    lv = R._u32(level) if level is not None else None
    assign = np.full(C, NONE, np.uint32)
    reason = np.zeros(C, np.uint8)
    ok_s = sched != 0
    # dom_count: the sum of node_count per domain, u32 and wrapping; eligible: a schedulable node in it
    dc = np.zeros(MAX_DOMAINS, np.uint64)
    np.add.at(dc, dom, cnt.astype(np.uint64))
    dc &= np.uint64(_M32)
    elig = np.zeros(MAX_DOMAINS, bool)
    elig[dom[ok_s]] = True
    idx = np.arange(N, dtype=np.uint64)
    miss = R.popcount32(np.uint32(preferred & _M32) & ~lab) << np.uint64(58)
    for i in R.ffd_order(cpu, mem):
        if lv is not None and lv[i] == NONE:
            reason[i] = 2
            continue
        c, m, r, x = cpu[i], mem[i], req[i], conf[i]
        fit = ok_s & (cf >= c) & (mf >= m) & ((lab & r) == r) & ((cu & x) == 0)
        if not fit.any():
            reason[i] = 1
            continue
        mn = dc[elig].min()  # a fitting node is schedulable, so some domain is eligible
        passes = ((dc - mn) & np.uint64(_M32)) < np.uint64(max_skew)  # u32 arithmetic
        ok = fit & passes[dom]
        if not ok.any():
            reason[i] = REASON_SKEW
            continue
        if strategy == R.SPREAD:
            prim = cnt
        elif strategy == R.PACK:
            prim = cf - c
        elif strategy == R.FILL_LOWEST:
            prim = ~cf
        else:
            prim = np.zeros(N, np.uint32)
        key = np.where(ok, miss | (prim.astype(np.uint64) << np.uint64(26)) | idx, R._INFEASIBLE)
        n = int(np.argmin(key))
        assign[i] = n
        cf[n] -= c
        mf[n] -= m
        cu[n] |= x
        cnt[n:n + 1] += np.uint32(1)  # u32, wraps
        dc[dom[n]] = (dc[dom[n]] + np.uint64(1)) & np.uint64(_M32)
        if trace is not None:
            trace.append((dc.astype(np.uint32), elig.copy()))
    return assign, reason, (cf, mf, lab, cu, sched), cnt


cost = R.cost  # SPEC.md 2.4 counts reason != 0, SKEW included
