#!/usr/bin/env python3
"""CPU replay of the walk of the no-mask packed FFD kernel (bigp / bigpw, fp_pipe.hip with FPP_BIGP_LAZY 2):
what the kernel does per (batch, group), counted -- no GPU.

    tools/bigp_replay.py [--seed 0x5EED0004] [--scenarios 0,1] [-C 50000] [-N 5000] [--flags 7]
                         [--refilter-max 16] [--capacity-only] [--segments]

The walk, as the kernel runs it:

* the containers in FFD order; CYCLE members (level = NONE) and containers the stage-2 screen rejects (a
  required label no schedulable node carries, a conflict bit every schedulable node has used) never enter
  the stream;
* 12-group segments of 64-node groups; segment 0 takes the positions 64 k .. 64 k + 63 as batch k, segment
  b + 1 the lanes segment b forwards (valid and not placed), in order, 64 to a batch;
* an unschedulable node is a record nothing fits (cpu = mem = 0, every conflict bit used, no label);
* a batch's corner is (the cpu of its last valid lane, the smallest mem of its valid lanes); all-zero
  containers count in it, are never queued, and take the segment's first schedulable node;
* group g is entered when a node of it holds the corner (once nothing of the batch is left, no group is);
  its queue is every lane of the batch not yet placed.  The STOP loop checks the queue in order up to the
  first miss, which drops that lane.  Then, while lanes are left: the corner's nodes are counted; at most
  REFILTER_MAX of them: a re-test pass keeps the lanes that fit one of them (capacity, labels, conflicts),
  and another STOP loop runs on those; when the pass drops nothing, or the corner has more nodes, the
  plain loop checks every lane left and the group is done.

The plan is asserted equal to the oracle's (oracle.oracle.place).  --capacity-only re-tests on capacity
alone (still exact: the dropped lanes are a subset); --refilter-max K moves the cap.  Counters, per
scenario and with --segments per segment: visits, batches, pass-through batches (nothing placed), active
(batch, group) pairs, checks, hits, misses, re-test passes, passes with an empty corner, corner nodes
walked (and their histogram per pass), big-corner exits, plain-loop checks, queued lanes at a re-test, and
the most passes any one (batch, group) took.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NONE = 0xFFFFFFFF
GROUPS = 12                      # groups per segment
SEG = GROUPS * 64                # nodes per segment
FULL = 0xFFFFFFFF
COUNTERS = ("visits", "batches", "pass_through", "active_pairs", "checks", "hits", "misses", "passes",
            "empty_passes", "nodes", "big_exits", "plain_checks", "retest_lanes")


def _new_stats(refilter_max):
    st = {k: 0 for k in COUNTERS}
    st["node_hist"] = np.zeros(refilter_max + 1, np.int64)
    st["max_pair_passes"] = 0   # the most re-test passes in one (batch, group)
    return st


class _Group:
    """One 64-node group's records: capacity, conflicts used, inverted labels (the kernel's rw, rcu, rlab)."""

    def __init__(self, cf, mf, lab, cu, sched, first, N):
        n = min(64, N - first)
        sl = slice(first, first + n)
        sc = np.zeros(64, bool)
        sc[:n] = sched[sl] != 0
        self.cf, self.mf = np.zeros(64, np.int64), np.zeros(64, np.int64)
        self.cu, self.nlab = np.full(64, FULL, np.int64), np.full(64, FULL, np.int64)
        self.cf[:n] = np.where(sc[:n], cf[sl], 0)
        self.mf[:n] = np.where(sc[:n], mf[sl], 0)
        self.cu[:n] = np.where(sc[:n], cu[sl], FULL)
        self.nlab[:n] = np.where(sc[:n], ~lab[sl].astype(np.int64) & FULL, FULL)
        self.first = first

    def corner(self, qc, qm):
        return np.nonzero((self.cf >= qc) & (self.mf >= qm))[0]

    def check(self, c, m, r, x):
        """The exact check of one container: the first node that takes it, or -1."""
        ok = (self.cf >= c) & (self.mf >= m) & (((self.nlab & r) | (self.cu & x)) == 0)
        l = int(np.argmax(ok))
        return l if ok[l] else -1

    def place(self, l, c, m, x):
        self.cf[l] -= c
        self.mf[l] -= m
        self.cu[l] |= x


def replay(cont, nodes, level=None, refilter_max=16, capacity_only=False, screen=True):
    """One scenario.  cont = (cpu, mem, req, conf), nodes = (cf, mf, lab, cu, sched), as oracle.place takes
    them.  Returns (assign, stats, per-segment stats): assign in container order, NONE where unplaced."""
    cpu, mem, req, conf = (np.asarray(a).astype(np.int64) for a in cont)
    cf, mf, lab, cu = (np.asarray(a).astype(np.int64) for a in nodes[:4])
    sched = np.asarray(nodes[4])
    from oracle import oracle as O
    C, N = cpu.size, cf.size
    order = O.ffd_order(cpu.astype(np.uint32), mem.astype(np.uint32)).astype(np.int64)
    skip = np.zeros(C, bool) if level is None else (np.asarray(level) == NONE)
    if screen:
        on = sched != 0
        have = int(np.bitwise_or.reduce(lab[on])) if on.any() else 0
        used = int(np.bitwise_and.reduce(cu[on])) if on.any() else FULL
        skip = skip | ((req & ~have & FULL) != 0) | ((conf & used) != 0)
    zero = (cpu | mem | req | conf) == 0
    assign = np.full(C, NONE, np.int64)
    B = (((N + 63) // 64) + GROUPS - 1) // GROUPS
    total, per_seg = _new_stats(refilter_max), []

    # segment 0's batches: the positions of each 64-block that are not skipped (holes stay holes: the
    # corner and the order only need the valid lanes, in order)
    stream = [order[k:k + 64][~skip[order[k:k + 64]]] for k in range(0, C, 64)]
    for b in range(B):
        st = _new_stats(refilter_max)
        groups = [_Group(cf, mf, lab, cu, sched, b * SEG + g * 64, N) if b * SEG + g * 64 < N else None
                  for g in range(GROUPS)]
        # the segment's first schedulable node takes the all-zero containers
        zs = next((n for n in range(b * SEG, min(N, (b + 1) * SEG)) if sched[n]), None)
        out = []
        for lanes in stream:
            st["batches"] += 1
            st["visits"] += lanes.size
            hits0 = st["hits"]
            if lanes.size:
                qc, qm = int(cpu[lanes[-1]]), int(mem[lanes].min())
                remaining = [int(i) for i in lanes if not zero[i]]
                for gr in groups:
                    if not remaining:
                        break
                    if gr is None or gr.corner(qc, qm).size == 0:
                        continue
                    st["active_pairs"] += 1
                    remaining = _group(gr, remaining, qc, qm, cpu, mem, req, conf, assign, st, refilter_max,
                                       capacity_only)
                if zs is not None:
                    assign[lanes[zero[lanes]]] = zs
            if st["hits"] == hits0:
                st["pass_through"] += 1
            out.extend(int(i) for i in lanes if assign[i] == NONE)
        # the groups' records go back to the node tables
        for gr in groups:
            if gr is not None:
                n = min(64, N - gr.first)
                on = sched[gr.first:gr.first + n] != 0
                cf[gr.first:gr.first + n][on] = gr.cf[:n][on]
                mf[gr.first:gr.first + n][on] = gr.mf[:n][on]
                cu[gr.first:gr.first + n][on] = gr.cu[:n][on]
        per_seg.append(st)
        for k in COUNTERS:
            total[k] += st[k]
        total["node_hist"] += st["node_hist"]
        total["max_pair_passes"] = max(total["max_pair_passes"], st["max_pair_passes"])
        stream = [np.array(out[k:k + 64], np.int64) for k in range(0, len(out), 64)]
    return assign.astype(np.uint32), total, per_seg


def _stop_loop(gr, q, cpu, mem, req, conf, assign, st, stop):
    """The serial loop over the queue q (container indices, in order).  stop: ends at the first miss and
    returns the lanes after it; else checks every lane and returns []."""
    for k, i in enumerate(q):
        st["checks"] += 1
        l = gr.check(cpu[i], mem[i], req[i], conf[i])
        if l >= 0:
            gr.place(l, cpu[i], mem[i], conf[i])
            assign[i] = gr.first + l
            st["hits"] += 1
        else:
            st["misses"] += 1
            if stop:
                return q[k + 1:]
    return []


def _group(gr, remaining, qc, qm, cpu, mem, req, conf, assign, st, refilter_max, capacity_only):
    q = _stop_loop(gr, remaining, cpu, mem, req, conf, assign, st, True)
    passes = 0
    while q:
        e = gr.corner(qc, qm)
        if e.size <= refilter_max:
            passes += 1
            st["max_pair_passes"] = max(st["max_pair_passes"], passes)
            st["passes"] += 1
            st["nodes"] += e.size
            st["node_hist"][e.size] += 1
            st["empty_passes"] += e.size == 0
            st["retest_lanes"] += len(q)
            qi = np.array(q, np.int64)
            ok = (gr.cf[e][None, :] >= cpu[qi][:, None]) & (gr.mf[e][None, :] >= mem[qi][:, None])
            if not capacity_only:
                ok &= ((gr.nlab[e][None, :] & req[qi][:, None]) | (gr.cu[e][None, :] & conf[qi][:, None])) == 0
            fit = [i for i, f in zip(q, ok.any(axis=1)) if f]
        else:
            st["big_exits"] += 1
            fit = q
        if len(fit) == len(q):
            c0 = st["checks"]
            _stop_loop(gr, q, cpu, mem, req, conf, assign, st, False)
            st["plain_checks"] += st["checks"] - c0
            break
        q = _stop_loop(gr, fit, cpu, mem, req, conf, assign, st, True)
    return [i for i in remaining if assign[i] == NONE]


def replay_checked(cont, nodes, level=None, **kw):
    """replay(), with the plan asserted equal to the oracle's."""
    from oracle import oracle as O
    assign, total, per_seg = replay(cont, nodes, level, **kw)
    want = O.place(cont, nodes, level=level)[0]
    bad = np.nonzero(assign != want)[0]
    assert bad.size == 0, f"the replay's plan differs from the oracle's in {bad.size} containers, first {bad[:5].tolist()}"
    return assign, total, per_seg


def _fmt(st):
    h = st["node_hist"]
    return ("  ".join(f"{k} {int(st[k])}" for k in COUNTERS + ("max_pair_passes",)) +
            "  node_hist " + ",".join(str(int(v)) for v in h[:int(np.max(np.nonzero(h)[0], initial=0)) + 1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0004)
    ap.add_argument("--scenarios", default="0,1", help="comma-separated scenario numbers, or a-b")
    ap.add_argument("-C", type=int, default=50000)
    ap.add_argument("-N", type=int, default=5000)
    ap.add_argument("--flags", type=int, default=7)
    ap.add_argument("--refilter-max", type=int, default=16)
    ap.add_argument("--capacity-only", action="store_true")
    ap.add_argument("--segments", action="store_true", help="print every segment's counters too")
    args = ap.parse_args()
    from oracle import oracle as O
    scen = []
    for part in args.scenarios.split(","):
        lo, _, hi = part.partition("-")
        scen += list(range(int(lo), int(hi or lo) + 1))
    for s in scen:
        cont, nodes = O.gen_scenario(args.seed, s, args.C, args.N, args.flags)
        _, total, per_seg = replay_checked(cont, nodes, refilter_max=args.refilter_max,
                                           capacity_only=args.capacity_only)
        print(f"scenario {s}: {_fmt(total)}")
        if args.segments:
            for b, st in enumerate(per_seg):
                print(f"  segment {b}: {_fmt(st)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
