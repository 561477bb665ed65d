"""Rejection-diagnosis timing (SPEC.md 2.9) on the config-4 batch shape, on cuda:0.

    python tools/explain_timing.py [--scenarios S] [--containers C] [--nodes N] [--steps K] [--warmup W]

One process: fp_dev_gen_batch, then fp_dev_place_batch (so that the batch holds a real reason array and the
node state the placement left), then three calls on that state, interleaved round by round so that a drift
of the machine touches all three alike:

    feasibility    fp_dev_feasibility_batch -- the stage-2 sweep, the yardstick: two accumulators per
                   container, unschedulable nodes skipped
    explain_nofit  fp_dev_explain_batch, reason_mask = 1 << FP_REASON_NOFIT (the rejected containers only)
    explain_all    fp_dev_explain_batch, reason_mask = 0 (every container)

Each figure is a host clock around one call that ends in a device synchronise, after `warmup` rounds; the
kernels' own time (the context's FP_K_FEAS event bracket) is taken in a separate pass.  node_evals_per_s
is (explained containers x N) over the median.  Writes profiles/explain_timing.json and prints it.  These
are measured values, not targets.
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


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=4096)
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_timing.json"))
    a = ap.parse_args()
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    out = {"shape": {"scenarios": S, "containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "steps": a.steps,
           "warmup": a.warmup, "device": props.name, "compute_units": props.multi_processor_count,
           "method": "host clock around one call ending in a device synchronise; the three calls interleaved per round",
           "calls": {}}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.dev_place_batch(db)
        p.sync()
        first = torch.empty(S * C, dtype=torch.int32, device=dev)
        count = torch.empty(S * C, dtype=torch.int32, device=dev)
        hist = torch.empty(S * _lib.EXPLAIN_HIST_WORDS, dtype=torch.int32, device=dev)
        nofit = 1 << _lib.REASON_NOFIT
        calls = {"feasibility": lambda: p.dev_feasibility_batch(db, first, count),
                 "explain_nofit": lambda: p.dev_explain_batch(db, nofit, None, hist),
                 "explain_all": lambda: p.dev_explain_batch(db, 0, None, hist)}
        n_nofit = int((db.reason == _lib.REASON_NOFIT).sum().item())
        explained = {"feasibility": S * C, "explain_nofit": n_nofit, "explain_all": S * C}
        wall = {k: [] for k in calls}
        for r in range(a.warmup + a.steps):
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                p.sync()
                if r >= a.warmup:
                    wall[name].append(1e3 * (time.perf_counter() - t0))
        kern = {}
        for name, call in calls.items():  # the kernels' own time, a pass of its own
            p.profile(True)
            for _ in range(a.steps):
                call()
            p.sync()
            ms, n = p.kernel_stats(_lib.FP_K_FEAS)
            p.profile(False)
            kern[name] = ms / max(n, 1)
        # what the histograms say, and that the two selections agree with the reason array
        p.dev_explain_batch(db, nofit, None, hist)
        p.sync()
        h = hist.view(S, _lib.EXPLAIN_HIST_WORDS).long().sum(dim=0).tolist()
        assert h[_lib.EXPLAIN_HIST_SELECTED] == n_nofit and h[_lib.EXPLAIN_HIST_FITS] == 0, h
        out["nofit_histogram_total"] = dict(zip(("CORDON", "CPU", "MEM", "LABEL", "CONFLICT", "MIXED", "FITS", "SELECTED"), h))
        for name in calls:
            st = _stats(wall[name])
            out["calls"][name] = {"ms_per_call": st, "ms_per_call_runs": wall[name], "kernel_ms": kern[name],
                                  "explained_containers": explained[name],
                                  "node_evals_per_s": explained[name] * N / (st["median"] * 1e-3)}
        out["explain_all_over_feasibility"] = (out["calls"]["explain_all"]["ms_per_call"]["median"]
                                               / out["calls"]["feasibility"]["ms_per_call"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
