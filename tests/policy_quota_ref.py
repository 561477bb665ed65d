"""numpy restatement of SPEC.md 2.10 (scored placement under a resource quota).

TEST INFRASTRUCTURE ONLY: the reference the QT variants of the HIP placer (fleetflow_amd/csrc/fp_policy.hip,
k_policy<.., .., .., true>) are compared with; never imported by the product package.  Built on
policy_fallback_ref.py (SPEC.md 2.8, and through it 2.7 and 2.6): the containers are visited in the FFD order,
the admission test of 2.10 comes first, and a container it lets through is placed by ``policy_fallback_ref.place``
itself, called with that one container on the node state, the node counts and the CYCLE level the earlier
containers left.  So nothing of 2.6 to 2.8 is restated here.

Two statements of the admission test: ``blocks_sub`` is the u32 form of the SPEC (it cannot wrap),
``blocks_wide`` adds in 64 bits.  The CPU tests compare the two.
"""
from __future__ import annotations

import numpy as np

import policy_fallback_ref as FR
import policy_ref as R

NONE = R.NONE
UNLIMITED = 0xFFFFFFFF
CPU, MEM, SERVICES = 0, 1, 2
REASON_QUOTA = 4
_M32 = 0xFFFFFFFF


def blocks_sub(quota, used, r):
    """SPEC.md 2.10 as written: u32 operands, and no intermediate leaves 0 .. 2^32 - 1."""
    quota, used, r = int(quota), int(used), int(r)
    assert all(0 <= x <= _M32 for x in (quota, used, r))
    return quota != UNLIMITED and r != 0 and not (used <= quota and r <= quota - used)


def blocks_wide(quota, used, r):
    """The same test with the sum taken in 64 bits."""
    quota, used, r = np.uint64(quota), np.uint64(used), np.uint64(r)
    return bool(quota != np.uint64(UNLIMITED) and r != np.uint64(0) and not (used + r <= quota))


def place(cont, nodes, strategy, quota, quota_used=None, preferred=0, level=None, node_count=None, domain=None,
          max_skew=0, relax_mask=(), n_hops=None, blocks=blocks_sub):
    """As policy_fallback_ref.place under ``quota`` = (cpu millicores, memory MiB, services), UNLIMITED = no cap in
    that dimension, with ``quota_used`` (None = zeros) what the tenant holds on entry.  Returns (assign, reason, hops,
    nodes_after, node_count_after, quota_why, quota_used_after)."""
    cpu, mem, req, conf = (R._u32(x) for x in cont)
    C = cpu.size
    quota = [int(q) for q in quota]
    used = [0, 0, 0] if quota_used is None else [int(u) for u in quota_used]
    assert len(quota) == 3 and len(used) == 3
    state = tuple(R._u32(x).copy() for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8),)
    cnt = R._u32(node_count).copy() if node_count is not None else np.zeros(state[0].size, np.uint32)
    lv = R._u32(level) if level is not None else None
    assign = np.full(C, NONE, np.uint32)
    reason = np.zeros(C, np.uint8)
    hops = np.zeros(C, np.uint8)
    why = np.zeros(C, np.uint8)
    for i in R.ffd_order(cpu, mem):
        if lv is not None and lv[i] == NONE:  # CYCLE first: neither tested against the quota nor charged
            reason[i] = 2
            continue
        r = (int(cpu[i]), int(mem[i]), 1)
        mask = sum(1 << d for d in range(3) if blocks(quota[d], used[d], r[d]))
        if mask:  # admission before scheduling: no node is searched, no state changes
            reason[i], why[i] = REASON_QUOTA, mask
            continue
        one = tuple(x[i:i + 1] for x in (cpu, mem, req, conf))
        a, rs, h, state, cnt = FR.place(one, state, strategy, preferred=preferred, node_count=cnt, domain=domain,
                                        max_skew=max_skew, relax_mask=relax_mask, n_hops=n_hops)
        assign[i], reason[i], hops[i] = a[0], rs[0], h[0]
        if a[0] != NONE:  # charged in all three dimensions, capped or not; u32, wraps
            used = [(u + x) & _M32 for u, x in zip(used, r)]
    return assign, reason, hops, state, cnt, why, np.array(used, np.uint32)


cost = R.cost  # SPEC.md 2.4 is unchanged: it counts reason != 0, so QUOTA counts as rejected


def usage(cont, assign):
    """What a plan charges: (cpu, memory, services) summed over the placed containers, modulo 2^32."""
    placed = np.asarray(assign) != NONE
    return (int(R._u32(cont[0])[placed].astype(np.uint64).sum()) & _M32,
            int(R._u32(cont[1])[placed].astype(np.uint64).sum()) & _M32, int(placed.sum()))
