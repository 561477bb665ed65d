"""Inputs the rejection-diagnosis tests share (SPEC.md 2.9).  TEST INFRASTRUCTURE ONLY.

``crafted`` makes every cause a sole blocker somewhere and a universal one for some container: a quarter
of the containers ask for no cpu and no memory (so that labels, ports or a cordon block alone), bit 13 is a
label no node has, bit 15 a port every node has in use.
"""
from __future__ import annotations

import functools

import numpy as np

import explain_ref as ER

# label dimensions of SPEC.md 3.2: (first bit, bits)
DIMS = ((0, 3), (3, 4), (7, 4), (11, 2))
# the shapes the floors below were tried at
SHAPES = ((300, 63), (300, 64), (300, 65), (1100, 1023), (1100, 1025), (300, 2049))


@functools.lru_cache(maxsize=None)
def crafted(C, N, seed=0):
    """(cont, nodes), read-only arrays."""
    rng = np.random.default_rng(7000 + 31 * C + N + 1000003 * seed)
    u32 = lambda x: np.asarray(x, np.uint32)  # noqa: E731
    cf = u32(rng.integers(0, 4001, N))
    mf = u32(rng.integers(0, 8193, N))
    lab = np.zeros(N, np.uint32)
    for lo, w in DIMS:
        lab |= np.uint32(1) << u32(lo + rng.integers(0, w, N))
    cu = np.full(N, 1 << 15, np.uint32)
    cu |= np.where(rng.random(N) < 0.3, np.uint32(1) << u32(rng.integers(0, 8, N)), 0).astype(np.uint32)
    sched = (rng.random(N) < 0.85).astype(np.uint8)
    cpu = u32(rng.integers(1, 5001, C))
    mem = u32(rng.integers(1, 10001, C))
    zero = rng.random(C) < 0.25
    cpu[zero] = 0
    mem[zero] = 0
    req = np.where(rng.random(C) < 0.4, 0, np.uint32(1) << u32(rng.integers(0, 13, C))).astype(np.uint32)
    req |= np.where(rng.random(C) < 0.15, np.uint32(1) << u32(rng.integers(0, 13, C)), 0).astype(np.uint32)
    req |= np.where(rng.random(C) < 0.08, 1 << 13, 0).astype(np.uint32)
    conf = np.where(rng.random(C) < 0.3, np.uint32(1) << u32(rng.integers(0, 8, C)), 0).astype(np.uint32)
    conf |= np.where(rng.random(C) < 0.08, 1 << 15, 0).astype(np.uint32)
    cont, nodes = (cpu, mem, req, conf), (cf, mf, lab, cu, sched)
    for a in (*cont, *nodes):
        a.setflags(write=False)
    return cont, nodes


@functools.lru_cache(maxsize=None)
def expected(C, N, ignore=0, seed=0):
    """The reference rows of crafted(C, N) for every container; computed once, shared, read-only."""
    r = ER.rows(*crafted(C, N, seed), ignore=ignore)
    r.setflags(write=False)
    return r


def assert_floors(r):
    """The floors of the recipe on reference rows (ignore = 0): a change of the generator cannot hollow the
    comparisons out.  ALL bit 0 (CORDON) has a case of its own: all_cordoned."""
    for k in range(5):
        assert (r[:, ER.ONLY + k] > 0).sum() >= 20, ("ONLY", k)
    for k in range(1, 5):
        assert ((r[:, ER.ALL] >> k) & 1).sum() >= 10, ("ALL", k)
    assert ((r[:, ER.FEASIBLE] == 0) & (r[:, ER.ALL] == 0)).sum() >= 1
    assert (r[:, ER.MISSING] != 0).sum() >= 10


def all_cordoned(C, N):
    cont, nodes = crafted(C, N)
    return cont, (*nodes[:4], np.zeros(N, np.uint8))


# ---- a batch at (300, 65) for the scored placer with a fallback chain and a spread constraint ---------------
RELAX = [0x780, 0x78, 0x1800, 0x7]  # the label dimensions of DIMS, hop by hop: class, region, arch, tier


def batch_case(S):
    """Scenario-major inputs of S scenarios of crafted(300, 65, seed): per scenario a strategy, max_skew
    (0 included), n_hops in {0, 1, 2, 4}, domains n % 3, and CYCLE levels on 5 % of the containers."""
    C, N = 300, 65
    rng = np.random.default_rng(900 + S)
    scen = [crafted(C, N, seed=s % 3) for s in range(S)]
    cat = lambda k, i: np.concatenate([sc[k][i] for sc in scen])  # noqa: E731
    strat = [int(x) for x in rng.integers(0, 4, S)]
    skew = [int(x) for x in rng.choice([0, 1, 2], S)]
    nh = [int(x) for x in rng.choice([0, 1, 2, 4], S)]
    skew[0], nh[0] = 1, 2
    dom = np.tile((np.arange(N) % 3).astype(np.uint32), S)
    level = np.where(rng.random(S * C) < 0.05, 0xFFFFFFFF, 0).astype(np.uint32)
    cum = [int(np.bitwise_or.reduce(np.array(RELAX[:h] + [0], np.uint32))) for h in nh]
    return dict(S=S, C=C, N=N, scen=scen, cont=[cat(0, i) for i in range(4)], nodes=[cat(1, i) for i in range(5)],
                strat=strat, skew=skew, nh=nh, relax=np.tile(np.array(RELAX, np.uint32), S), dom=dom, level=level,
                ignore=np.array(cum, np.uint32))
