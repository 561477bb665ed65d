"""numpy reference of the rejection diagnosis (SPEC.md 2.9).  TEST INFRASTRUCTURE ONLY.

A direct transcription: per container one vectorised pass over the nodes.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
CORDON, CPU, MEM, LABEL, CONFLICT = 1, 2, 4, 8, 16
FAIL, ONLY, FEASIBLE, ALL, MISSING, NEAR, WORDS = 0, 5, 10, 11, 12, 13, 16
HIST_MIXED, HIST_FITS, HIST_SELECTED, HIST_WORDS = 5, 6, 7, 8


def why(c, cont, nodes, ignore=0):
    """[N] the 5-bit mask of the 2.3 predicates container c fails on each node."""
    cpu, mem, req, conf = (np.asarray(x, np.uint32) for x in cont)
    cf, mf, lab, cu = (np.asarray(x, np.uint32) for x in nodes[:4])
    sched = np.asarray(nodes[4], np.uint8)
    r = np.uint32(int(req[c]) & ~int(ignore) & 0xFFFFFFFF)
    w = np.where(sched == 0, CORDON, 0).astype(np.uint32)
    w |= np.where(cf < cpu[c], CPU, 0).astype(np.uint32)
    w |= np.where(mf < mem[c], MEM, 0).astype(np.uint32)
    w |= np.where((lab & r) != r, LABEL, 0).astype(np.uint32)
    w |= np.where((cu & conf[c]) != 0, CONFLICT, 0).astype(np.uint32)
    return w


def rows(cont, nodes, sel=None, ignore=0):
    """[M, 16] u32: one row per explained container (sel = None: every container in order)."""
    C = len(cont[0])
    lab = np.asarray(nodes[2], np.uint32)
    sched = np.asarray(nodes[4], np.uint8)
    N = lab.size
    sel = np.arange(C) if sel is None else np.asarray(sel, np.int64).reshape(-1)
    have = int(np.bitwise_or.reduce(lab[sched != 0])) if (sched != 0).any() else 0
    out = np.zeros((sel.size, WORDS), np.uint32)
    for i, c in enumerate(sel):
        w = why(c, cont, nodes, ignore)
        for k in range(5):
            out[i, FAIL + k] = int(((w >> k) & 1).sum())
            out[i, ONLY + k] = int((w == (1 << k)).sum())
        out[i, FEASIBLE] = int((w == 0).sum())
        out[i, ALL] = int(np.bitwise_and.reduce(w)) if N else 0x1F
        out[i, MISSING] = int(cont[2][c]) & ~int(ignore) & ~have & 0xFFFFFFFF
        one = np.flatnonzero((w != 0) & ((w & (w - 1)) == 0))
        out[i, NEAR] = int(one[0]) if one.size else NONE
    return out


def rows_matrix(cont, nodes, ignore=0):
    """rows(cont, nodes, None, ignore) as one containers x nodes pass: the same words, for the batch tests
    (hundreds of scenarios).  test_explain_host.py holds it against ``rows``."""
    cpu, mem, req, conf = (np.asarray(x, np.uint32)[:, None] for x in cont)
    cf, mf, lab, cu = (np.asarray(x, np.uint32)[None, :] for x in nodes[:4])
    sched = np.asarray(nodes[4], np.uint8)
    C, N = cpu.shape[0], sched.size
    r = req & np.uint32(~int(ignore) & 0xFFFFFFFF)
    w = np.where(sched[None, :] == 0, CORDON, 0).astype(np.uint32) | np.where(cf < cpu, CPU, 0).astype(np.uint32)
    w = w | np.where(mf < mem, MEM, 0).astype(np.uint32) | np.where((lab & r) != r, LABEL, 0).astype(np.uint32)
    w = w | np.where((cu & conf) != 0, CONFLICT, 0).astype(np.uint32)
    w = np.broadcast_to(w, (C, N))
    have = int(np.bitwise_or.reduce(lab[0, sched != 0])) if (sched != 0).any() else 0
    out = np.zeros((C, WORDS), np.uint32)
    for k in range(5):
        out[:, FAIL + k] = ((w >> k) & 1).sum(axis=1)
        out[:, ONLY + k] = (w == (1 << k)).sum(axis=1)
    out[:, FEASIBLE] = (w == 0).sum(axis=1)
    out[:, ALL] = np.bitwise_and.reduce(w, axis=1) if N else 0x1F
    out[:, MISSING] = r[:, 0] & np.uint32(~have & 0xFFFFFFFF)
    one = (w != 0) & ((w & (w - 1)) == 0)
    out[:, NEAR] = np.where(one.any(axis=1), one.argmax(axis=1), NONE) if N else NONE
    return out


def hist(r):
    """[8] the histogram of SPEC.md 2.9 over the rows r of one scenario's selected containers."""
    h = np.zeros(HIST_WORDS, np.uint32)
    for k in range(5):
        h[k] = int(((r[:, ALL] >> k) & 1).sum())
    h[HIST_MIXED] = int(((r[:, FEASIBLE] == 0) & (r[:, ALL] == 0)).sum())
    h[HIST_FITS] = int((r[:, FEASIBLE] > 0).sum())
    h[HIST_SELECTED] = r.shape[0]
    return h
