"""Drain what-if sweep timing (SPEC.md 2.11) on one config-4 scenario, on cuda:0.

    python tools/drain_timing.py [--containers C] [--nodes N] [--steps K] [--warmup W] [--rounds R]

One scenario of C x N (default 50k x 5k, the generator's config-4 inputs) is placed by
fp_dev_place_batch_policy under each strategy; that plan and the node table it leaves are the live state.
On it the tool times

* ``sweep``: fp_dev_drain_sweep for every single-server candidate (n_cand = N) and for 8 and 64 zones
  (group = n % Z), and
* ``replicated``: the only way to the same answer without it: fp_dev_place_batch_policy with one scenario per
  candidate, each holding max_evictees containers (padded with level = FP_NONE, which the placer skips) and
  its own copy of the node table and of the counts with the candidate's nodes masked out of `schedulable`.
  Building the replicas on the device (``build``) is timed apart from the call (``call``); the call changes
  its node tables, so every timed call gets freshly built replicas.

Each figure is a host clock around calls that end in a device synchronise, after `warmup` calls; a round times
the sweep and then the replicated call, and the rounds' minimum, median and maximum are kept.  The kernels' own
time comes from the context's event brackets (FP_K_PLACE, FP_K_SORT) in a separate pass.  Before anything is
timed the two answers are compared: ``same_plan`` says that every evictee got the same node from both.  Writes
profiles/drain_timing.json and prints it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fleetflow_amd import DevBatch, Planner, _lib  # noqa: E402

SEED4 = 0x5EED0004
STRATEGIES = (("first_fit_scored", 0), ("spread_across_pool", 1), ("pack_into_dedicated", 2), ("fill_lowest", 3))
ZONES = (8, 64)


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def build_replicas(db, count, group, S, dev):
    """One scenario per candidate, on the device: (batch, counts [S*N], the evictees, their slots in the
    batch).  The evictees of a candidate keep their index order, so the batch visits them as the sweep does."""
    C, N = db.C, db.N
    assign = db.assign.long()
    cand = torch.where(assign >= 0, group.long()[assign.clamp(min=0)], torch.full_like(assign, -1))
    ev = torch.nonzero(cand >= 0).flatten()
    cs, perm = torch.sort(cand[ev], stable=True)
    ev = ev[perm]
    per = torch.bincount(cs, minlength=S)
    E = max(int(per.max().item()), 1)
    slot = cs * E + (torch.arange(ev.numel(), device=dev) - (torch.cumsum(per, 0) - per)[cs])
    b = DevBatch.allocate(S, E, N, dev, with_level=True)
    for dst, src in ((b.cpu, db.cpu), (b.mem, db.mem), (b.req, db.req), (b.conf, db.conf)):
        dst.zero_()
        dst[slot] = src[ev]
    b.level.fill_(-1)
    b.level[slot] = 0
    for dst, src in ((b.cf, db.cf), (b.mf, db.mf), (b.lab, db.lab), (b.cu, db.cu)):
        dst.view(S, N).copy_(src.view(1, N).expand(S, N))
    own = group.view(1, N) == torch.arange(S, dtype=group.dtype, device=dev).view(S, 1)
    b.sched.view(S, N).copy_(db.sched.view(1, N).expand(S, N) * (~own).to(torch.uint8))
    counts = count.repeat(S)
    return b, counts, ev, slot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drain_timing.json"))
    a = ap.parse_args()
    C, N = a.containers, a.nodes
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    out = {"shape": {"containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "device": props.name, "compute_units": props.multi_processor_count,
           "order": "each round: the sweep, then the replicated batch call", "strategies": {}}
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    groupings = [("single_server", torch.arange(N, dtype=torch.int32, device=dev), N)]
    groupings += [(f"zones_{Z}", torch.arange(N, dtype=torch.int32, device=dev) % Z, Z) for Z in ZONES]
    with Planner(0) as p:
        for name, sid in STRATEGIES:
            db = DevBatch.allocate(1, C, N, dev)
            p.dev_gen_batch(SEED4, db, 7)
            count = i32(N)
            st1 = torch.full((1,), sid, dtype=torch.int32, device=dev)
            p.dev_place_batch_policy(db, st1, None, count)
            p.sync()
            cont_t, nodes_t = (db.cpu, db.mem, db.req, db.conf), (db.cf, db.mf, db.lab, db.cu, db.sched)
            rec = {"running": int((db.assign != -1).sum().item())}
            for label, group, S in groupings:
                a_out, reason, rows = i32(C), torch.zeros(C, dtype=torch.uint8, device=dev), i32(S * _lib.DRAIN_WORDS)
                stS = torch.full((S,), sid, dtype=torch.int32, device=dev)

                def sweep():
                    p.dev_drain_sweep(cont_t, nodes_t, db.assign, group, S, a_out, reason, rows, sid, 0, count)

                def replicated():
                    b, counts, ev, slot = build_replicas(db, count, group, S, dev)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    p.dev_place_batch_policy(b, stS, None, counts)
                    p.sync()
                    return time.perf_counter() - t0, b, ev, slot

                # ---- the same answer first ----
                sweep()
                p.sync()
                _, b, ev, slot = replicated()
                same = bool(torch.equal(b.assign[slot], a_out[ev])) and bool(torch.equal(b.reason[slot], reason[ev]))
                summary = rows.view(S, _lib.DRAIN_WORDS)
                g = {"n_cand": S, "evictees": int(ev.numel()), "max_evictees": b.C,
                     "stranded": int(summary[:, _lib.DRAIN_STRANDED].sum().item()),
                     "candidates_that_strand": int((summary[:, _lib.DRAIN_STRANDED] > 0).sum().item()),
                     "same_plan": same,
                     "replica_bytes": (4 * 4 + 4) * S * b.C + (4 * 4 + 1 + 4) * S * N}
                del b
                for _ in range(a.warmup):
                    sweep()
                    replicated()
                p.sync()
                sw, build, call = [], [], []
                for _ in range(a.rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        sweep()
                    p.sync()
                    sw.append(1e3 * (time.perf_counter() - t0) / a.steps)
                    tb = tc = 0.0
                    for _ in range(a.steps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        dt, *_ = replicated()
                        tb += time.perf_counter() - t0 - dt
                        tc += dt
                    build.append(1e3 * tb / a.steps)
                    call.append(1e3 * tc / a.steps)
                # ---- the kernels' own time, in a pass of its own ----
                p.profile(True)
                for _ in range(a.steps):
                    sweep()
                p.sync()
                kp, n = p.kernel_stats(_lib.FP_K_PLACE)
                ks, _ = p.kernel_stats(_lib.FP_K_SORT)
                g["sweep"] = {"ms_per_call": _stats(sw), "sweep_kernel_ms": kp / max(n, 1), "bucketing_ms": ks / max(n, 1)}
                p.profile(True)
                for _ in range(a.steps):
                    replicated()
                p.sync()
                kp, n = p.kernel_stats(_lib.FP_K_PLACE)
                ks, _ = p.kernel_stats(_lib.FP_K_SORT)
                p.profile(False)
                g["replicated"] = {"build_ms": _stats(build), "call_ms": _stats(call),
                                   "place_kernel_ms": kp / max(n, 1), "sort_ms": ks / max(n, 1)}
                g["call_over_sweep"] = g["replicated"]["call_ms"]["median"] / g["sweep"]["ms_per_call"]["median"]
                g["build_and_call_over_sweep"] = ((g["replicated"]["call_ms"]["median"] + g["replicated"]["build_ms"]["median"])
                                                  / g["sweep"]["ms_per_call"]["median"])
                rec[label] = g
                torch.cuda.empty_cache()
            out["strategies"][name] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
