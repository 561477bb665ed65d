"""Scale-out sweep timing (SPEC.md 2.12) on one config-4 scenario, on cuda:0.

    python tools/grow_timing.py [--containers C] [--nodes N] [--steps K] [--warmup W] [--rounds R]

One scenario of C x N (default 50k x 5k, the generator's config-4 inputs) is placed first fit by
fp_dev_place_batch; its NOFIT containers are the pending.  The candidates are the five node types of SPEC.md 3.2
crossed with the 96 label combinations a generated node can carry (480 templates); 5 and 5 000 candidates (the
first five, and the catalogue repeated) are timed as well, each with max_new = 64, 1024 and 8192.  For every
point the tool times

* ``sweep``: fp_dev_grow_sweep without assign_out, and
* ``replicated``: the only way to the same answer without it: fp_dev_place_batch_policy under strategy 0 with
  one scenario per candidate, each holding a copy of the pending containers and its own table of max_new
  identical empty nodes.  Building the replicas on the device (``build``) is timed apart from the call
  (``call``); the call changes its node tables, so every timed call gets freshly built replicas.

Each figure is a host clock around calls that end in a device synchronise, after `warmup` calls; a round times
the sweep and then the replicated call, and the rounds' minimum, median and maximum are kept.  The kernels' own
time comes from the context's event brackets (FP_K_PLACE, FP_K_SORT) in a separate pass.  Before anything is
timed the two answers are compared: ``same_counts`` says that both placed the same number on the same number of
servers for every candidate, ``same_plan`` (up to 480 candidates) that every pending container got the same
server from both.  Writes profiles/grow_timing.json and prints it.
"""
import argparse
import itertools
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
NODE_TYPES = ((4000, 8192), (8000, 16384), (16000, 32768), (32000, 65536), (64000, 262144))
N_CAND = (5, 480, 5000)
MAX_NEW = (64, 1024, 8192)


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def catalogue(n, dev):
    """The node types of SPEC.md 3.2 x (tier, region, class, arch) one-hot labels, repeated up to n."""
    labels = [(1 << t) | (1 << (3 + r)) | (1 << (7 + c)) | (1 << (11 + a))
              for t, r, c, a in itertools.product(range(3), range(4), range(4), range(2))]
    rows = [(cpu, mem, lab) for (cpu, mem), lab in itertools.product(NODE_TYPES, labels)]
    rows = [rows[i % len(rows)] for i in range(n)] if n > len(NODE_TYPES) else [(c, m, labels[0]) for c, m in NODE_TYPES][:n]
    return tuple(torch.tensor([r[i] for r in rows], dtype=torch.int32, device=dev) for i in range(3))


def build_replicas(pend_t, tpl, max_new, dev):
    """One scenario per candidate, on the device: the pending containers (index order, so the batch visits them
    as the sweep does) on max_new empty nodes of the candidate's template."""
    S, P = tpl[0].numel(), pend_t[0].numel()
    b = DevBatch.allocate(S, P, max_new, dev)
    for dst, src in zip((b.cpu, b.mem, b.req, b.conf), pend_t):
        dst.view(S, P).copy_(src.view(1, P).expand(S, P))
    for dst, src in zip((b.cf, b.mf, b.lab), tpl):
        dst.view(S, max_new).copy_(src.view(S, 1).expand(S, max_new))
    b.cu.zero_()
    b.sched.fill_(1)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_timing.json"))
    a = ap.parse_args()
    C, N = a.containers, a.nodes
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    out = {"shape": {"containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "device": props.name, "compute_units": props.multi_processor_count,
           "order": "each round: the sweep, then the replicated batch call", "points": []}
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    with Planner(0) as p:
        db = DevBatch.allocate(1, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.dev_place_batch(db)
        p.sync()
        cont_t = (db.cpu, db.mem, db.req, db.conf)
        pend = torch.nonzero(db.reason == _lib.REASON_NOFIT).flatten()
        pend_t = tuple(t[pend].contiguous() for t in cont_t)
        out["pending"] = int(pend.numel())
        for n_cand, max_new in itertools.product(N_CAND, MAX_NEW):
            tpl = catalogue(n_cand, dev)
            rows = i32(n_cand * _lib.GROW_WORDS)
            st = i32(n_cand)  # strategy 0

            def sweep(assign=None):
                p.dev_grow_sweep(cont_t, db.reason, tpl, max_new, rows, 1 << _lib.REASON_NOFIT, None, assign)

            def replicated():
                b = build_replicas(pend_t, tpl, max_new, dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p.dev_place_batch_policy(b, st)
                p.sync()
                return time.perf_counter() - t0, b

            # ---- the same answer first ----
            detail = n_cand <= 480
            full = i32(n_cand * C) if detail else None
            sweep(full)
            p.sync()
            _, b = replicated()
            got = b.assign.view(n_cand, -1)
            summary = rows.view(n_cand, _lib.GROW_WORDS)
            placed = (got != -1).sum(1).to(torch.int32)
            opened = (got.max(1).values + 1).to(torch.int32) if got.numel() else i32(n_cand)
            g = {"n_cand": n_cand, "max_new": max_new,
                 "placed": int(summary[:, _lib.GROW_PLACED].sum().item()),
                 "opened": int(summary[:, _lib.GROW_OPENED].sum().item()),
                 "opened_max": int(summary[:, _lib.GROW_OPENED].max().item()),
                 "unplaceable": int(summary[:, _lib.GROW_UNPLACEABLE].sum().item()),
                 "capped": int(summary[:, _lib.GROW_CAPPED].sum().item()),
                 "same_counts": bool(torch.equal(placed, summary[:, _lib.GROW_PLACED]))
                 and bool(torch.equal(opened, summary[:, _lib.GROW_OPENED])),
                 "same_plan": bool(torch.equal(full.view(n_cand, C)[:, pend], got)) if detail else None,
                 "replica_bytes": (4 * 4 + 4 + 1) * n_cand * b.C + (4 * 4 + 1) * n_cand * max_new}
            del b, got, full
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
                    dt, _ = replicated()
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
            p.profile(False)
            g["sweep"] = {"ms_per_call": _stats(sw), "sweep_kernel_ms": kp / max(n, 1), "list_build_ms": ks / max(n, 1)}
            g["replicated"] = {"build_ms": _stats(build), "call_ms": _stats(call)}
            g["call_over_sweep"] = g["replicated"]["call_ms"]["median"] / g["sweep"]["ms_per_call"]["median"]
            g["build_and_call_over_sweep"] = ((g["replicated"]["call_ms"]["median"] + g["replicated"]["build_ms"]["median"])
                                              / g["sweep"]["ms_per_call"]["median"])
            out["points"].append(g)
            print(json.dumps(g), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
