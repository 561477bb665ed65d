"""Inputs the fallback-chain tests share (SPEC.md 2.8).  TEST INFRASTRUCTURE ONLY.

The generator's own required labels (one bit of 13, SPEC.md 3.2) almost never exhaust a pool, so the
chain would relax nothing.  ``crafted`` keeps the generator's containers and nodes and makes the pools run
dry: dense requirements (per label dimension, with probability 0.6, one uniformly drawn bit of it) and a
node table thinned to about C / 10 schedulable nodes.  The winners still fall in every thread and row.
"""
from __future__ import annotations

import functools

import numpy as np

SEED = 0x5EED0004
# the four label dimensions of SPEC.md 3.2: (first bit, bits)
DIMS = {"tier": (0, 3), "region": (3, 4), "class": (7, 4), "arch": (11, 2)}
MASK = {k: ((1 << w) - 1) << lo for k, (lo, w) in DIMS.items()}
assert MASK == {"tier": 0x7, "region": 0x78, "class": 0x780, "arch": 0x1800}
RELAX = {1: [MASK["class"]], 2: [MASK["class"], MASK["region"]],
         4: [MASK["class"], MASK["region"], MASK["arch"], MASK["tier"]]}


@functools.lru_cache(maxsize=None)
def crafted(C, N, scen=3):
    """(cont, nodes) of gen_scenario(SEED, scen, C, N, 7) with dense requirements and a thinned node table;
    read-only arrays."""
    from oracle import oracle as O
    cont, nodes = O.gen_scenario(SEED, scen, C, N, 7)
    rng = np.random.default_rng(C + N)
    req = np.zeros(C, np.uint32)
    for lo, w in DIMS.values():
        use = rng.random(C) < 0.6
        bit = rng.integers(0, w, C)
        req |= np.where(use, np.uint32(1) << (lo + bit).astype(np.uint32), 0).astype(np.uint32)
    keep = np.random.default_rng(N).random(N) < min(1.0, C / (10.0 * N))
    cont = (cont[0], cont[1], req, cont[3])
    nodes = (*nodes[:4], (np.asarray(nodes[4]) & keep).astype(np.uint8))
    for a in (*cont, *nodes):
        a.setflags(write=False)
    return cont, nodes


def relax_rows(per_scenario):
    """[S][4] relax words from per-scenario mask lists (zero-padded)."""
    return np.array([list(m) + [0] * (4 - len(m)) for m in per_scenario], np.uint32).reshape(-1)


# ---- the closed form: N nodes with room for one container each, labels by n % 4 = A|Y, B|Y, A|X, B|X -------
A, B, X, Y = 1, 2, 4, 8
CLASS, REGION = A | B, X | Y


def closed_form(N):
    lab = np.array([A | Y, B | Y, A | X, B | X], np.uint32)[np.arange(N) % 4]
    nodes = (np.full(N, 100, np.uint32), np.full(N, 100, np.uint32), lab, np.zeros(N, np.uint32), np.ones(N, np.uint8))
    cont = (np.full(N, 100, np.uint32), np.full(N, 1, np.uint32), np.full(N, A | Y, np.uint32), np.zeros(N, np.uint32))
    return cont, nodes


@functools.lru_cache(maxsize=None)
def expected(C, N, strategy, n_hops, spread=False):
    """The iterative reference on crafted(C, N) under RELAX[n_hops] (n_hops = 0: no chain), from zero node
    counts; with ``spread`` under domain = n % 5, max_skew = 2.  Computed once, shared, read-only."""
    import policy_fallback_ref as FR
    cont, nodes = crafted(C, N)
    kw = dict(domain=spread_domain(N), max_skew=2) if spread else {}
    out = FR.place(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), relax_mask=RELAX.get(n_hops, []), **kw)
    for a in (out[0], out[1], out[2], *out[3], out[4]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def spread_domain(N):
    d = (np.arange(N) % 5).astype(np.uint32)
    d.setflags(write=False)
    return d
