"""Inputs the stage-2 feasibility tests share (SPEC.md 2.3, 2.5).  TEST INFRASTRUCTURE ONLY.

A seeded generator built to tell a wrong k_feas from a right one, not SPEC 3's:

* demands and capacities come from one small pool with both sides of the sign bit, so ``cf == cpu`` is common;
* labels use all 32 bits.  Bits 0..22 are set with p = 0.8 (all of them on some nodes); bits 24..31 are tile bits -- node n carries bit
  24 + (n / 1024) % 8 -- and half the containers require one of the eight, which pins their ``first`` to one
  LDS tile or, for a bit no tile of this N carries, makes them infeasible everywhere; bit 23 is the edge bit,
  carried only by the last node of every tile and by node N - 1, which accept everything but a required bit
  they lack;
* about 15 % of the nodes are cordoned, and so are whole aligned 64-node groups at a stride and a run across
  node 1024;
* ``mask_nodes=True`` overwrites one node of every 64-node group with the only kind of node an absent lane of
  the kernel (all-ones demands) fits: labels and capacities all ones, nothing in use, schedulable.  Every
  container fits those nodes, so such a table has no ``count == 0`` and every ``first`` below 64: it is a
  second table for the calls that write a bitmap with C % 64 != 0, beside the plain one.
"""
from __future__ import annotations

import functools

import numpy as np

import feas_ref as FR

POOL = np.array([0, 1, 64, 4000, 2**31 - 1, 2**31, 2**32 - 1], np.uint64).astype(np.uint32)
ALL = np.uint32(0xFFFFFFFF)
EDGE_BIT, TILE_BIT0 = 23, 24
GROUP_STRIDE, GROUP_FIRST = 7, 2  # cordoned 64-node groups: 2, 9, 16, ...


def _bits(rng, n, p, width=32):
    out = np.zeros(n, np.uint32)
    for b in range(width):
        out |= (rng.random(n) < p).astype(np.uint32) << np.uint32(b)
    return out


def _one_bit(rng, n, lo, width):
    return np.uint32(1) << (lo + rng.integers(0, width, n)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(C, N, seed=0, mask_nodes=False):
    """(cont, nodes), read-only arrays: (cpu, mem, req, conf) and (cf, mf, lab, cu, sched)."""
    rng = np.random.default_rng(52000 + 7919 * seed)  # not of C or N: scenario p is the same draw at any size
    rc, rn = (np.random.default_rng(rng.integers(1 << 62)) for _ in range(2))
    # ---- nodes
    n = np.arange(N)
    cf = POOL[rn.integers(0, POOL.size, N)]
    mf = POOL[rn.integers(0, POOL.size, N)]
    lab = _bits(rn, N, 0.8, EDGE_BIT)
    lab |= np.uint32(1) << (TILE_BIT0 + (n // FR.K_TILE) % 8).astype(np.uint32)
    lab[rn.random(N) < 0.02] |= np.uint32((1 << EDGE_BIT) - 1)  # every ordinary bit; all 32 only on a mask node
    cu = _bits(rn, N, 0.08)
    sched = (rn.random(N) >= 0.15).astype(np.uint8)
    sched[(n // 64) % GROUP_STRIDE == GROUP_FIRST] = 0
    sched[(n >= 1000) & (n < 1051)] = 0
    edge = (n % FR.K_TILE == FR.K_TILE - 1) | (n == N - 1)
    lab[edge] |= np.uint32(1 << EDGE_BIT)
    lab[~edge] &= ~np.uint32(1 << EDGE_BIT)
    cf[edge], mf[edge], cu[edge], sched[edge] = ALL, ALL, 0, 1
    if mask_nodes:
        pick = (n % 64 == (7 * (n // 64) + 5) % 64) | ((n == N - 1) & (N % 64 != 0) & (N % 64 <= (7 * ((N - 1) // 64) + 5) % 64))
        cf[pick], mf[pick], lab[pick], cu[pick], sched[pick] = ALL, ALL, ALL, 0, 1
    # ---- containers
    cpu = POOL[rc.integers(0, POOL.size, C)]
    mem = POOL[rc.integers(0, POOL.size, C)]
    two = _one_bit(rc, C, 0, EDGE_BIT) | _one_bit(rc, C, 0, EDGE_BIT)
    req = np.where(rc.random(C) < 0.5, 0, two).astype(np.uint32)
    req |= np.where(rc.random(C) < 0.5, _one_bit(rc, C, TILE_BIT0, 8), 0).astype(np.uint32)
    req |= np.where(rc.random(C) < 0.10, 1 << EDGE_BIT, 0).astype(np.uint32)
    conf = np.where(rc.random(C) < 0.5, 0, _one_bit(rc, C, 0, 32) | _one_bit(rc, C, 0, 32)).astype(np.uint32)
    req[rc.random(C) < 0.01] = ALL
    conf[rc.random(C) < 0.01] = ALL
    cont, nodes = (cpu, mem, req, conf), (cf, mf, lab, cu, sched)
    for a in (*cont, *nodes):
        a.setflags(write=False)
    return cont, nodes


@functools.lru_cache(maxsize=None)
def expected(C, N, seed=0, mask_nodes=False, want_bitmap=True):
    """The reference outputs of case(...): computed once, shared, read-only."""
    out = FR.feasibility(*case(C, N, seed, mask_nodes), want_bitmap=want_bitmap)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def has_mask_node_in_every_group(nodes):
    cf, mf, lab, cu, sched = nodes
    hit = (cf == ALL) & (mf == ALL) & (lab == ALL) & (cu == 0) & (sched != 0)
    return all(hit[g:g + 64].any() for g in range(0, len(cf), 64))


# ---- a batch: S scenarios that walk through a pool of P generated ones ---------------------------------------
def pool_of(S, C, N):
    """Distinct scenarios of a batch of S.  The reference is O(P * C * N), so a large S repeats a pool whose
    size is coprime to everything the launch plan knows; the per-tile floors need about a thousand containers."""
    return min(S, max(5, -(-1100 // max(C, 1)) | 1))


def batch(S, C, N):
    """Scenario-major (cont, nodes) of scenario s = case(C, N, seed=s % P), and P."""
    P = pool_of(S, C, N)
    pool = [case(C, N, seed=p) for p in range(P)]
    idx = np.arange(S) % P
    cont = tuple(np.stack([pool[p][0][i] for p in range(P)])[idx].reshape(-1) for i in range(4))
    nodes = tuple(np.stack([pool[p][1][i] for p in range(P)])[idx].reshape(-1) for i in range(5))
    return cont, nodes, P


def batch_expected(S, C, N):
    """(first [S*C], count [S*C]) of batch(S, C, N) from the pool's references."""
    P = pool_of(S, C, N)
    idx = np.arange(S) % P
    first = np.stack([expected(C, N, p, want_bitmap=False)[0] for p in range(P)])[idx].reshape(-1)
    count = np.stack([expected(C, N, p, want_bitmap=False)[1] for p in range(P)])[idx].reshape(-1)
    return first, count


# ---- what the inputs must be for a comparison on them to mean something --------------------------------------
def stats(cont, nodes):
    """Counts on the reference alone; dictionaries of several cases add up with ``add``."""
    p = FR.predicates(cont, nodes)
    ok = p[0] & p[1] & p[2] & p[3] & p[4]
    C, N = ok.shape
    sole = [int((~p[k] & np.logical_and.reduce([p[j] for j in range(5) if j != k])).sum()) for k in range(5)]
    count = ok.sum(1)
    first = np.where(count == 0, -1, ok.argmax(1) if N else 0)
    n_tiles = (N + FR.K_TILE - 1) // FR.K_TILE
    lasts = [min(N, (t + 1) * FR.K_TILE) - 1 for t in range(n_tiles)]
    cpu, mem = (np.asarray(x).astype(np.uint64) for x in cont[:2])
    cf, mf = (np.asarray(x).astype(np.uint64) for x in nodes[:2])
    return dict(pairs=C * N, feasible=int(ok.sum()), sole=sole, rows=C, none=int((count == 0).sum()),
                tile_firsts=[int(((first >= 0) & (first // FR.K_TILE == t)).sum()) for t in range(n_tiles)],
                last_firsts=[int((first == n).sum()) for n in lasts],
                cpu_eq=int((ok & (cf[None, :] == cpu[:, None])).sum()), mem_eq=int((ok & (mf[None, :] == mem[:, None])).sum()))


def add(a, b):
    if a is None:
        return b
    out = {}
    for k in a:
        out[k] = [x + y for x, y in zip(a[k], b[k])] if isinstance(a[k], list) else a[k] + b[k]
    return out


def assert_conditions(st, per_tile=True):
    """``per_tile=False`` only where the case has too few containers for a floor per tile (a single scenario of
    70: six in a thousand containers ask for the edge bit and one given tile)."""
    assert 0.05 <= st["feasible"] / st["pairs"] <= 0.6, st
    for k in range(5):
        assert st["sole"][k] >= 0.003 * st["pairs"], ("sole blocker", k, st)
    assert st["none"] >= 0.05 * st["rows"] and st["rows"] - st["none"] >= 0.05 * st["rows"], st
    if per_tile:
        assert all(x >= 4 for x in st["tile_firsts"]), st
        assert all(x >= 1 for x in st["last_firsts"]), st
    assert st["cpu_eq"] >= 0.01 * st["feasible"] and st["mem_eq"] >= 0.01 * st["feasible"], st
