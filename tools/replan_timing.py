"""Re-plan timing (SPEC.md 2.13) on the config-4 policy batch shape, on cuda:0.

    python tools/replan_timing.py [--scenarios S] [--containers C] [--nodes N] [--steps K] [--warmup W] [--rounds R]

S what-if scenarios of C x N (default 512 x 50k x 5k, the shape tools/policy_timing.py times: the slice one of
eight ranks plans of config 4), the generator's inputs.  Per strategy four calls on the same batch, from the same
base node tables:

* ``a_place``:  fp_dev_place_batch_policy, the same build: the baseline;
* ``b_no_prev``: fp_dev_replan_batch with prev all FP_NONE: the same placement work plus pass 1;
* ``c_fixed_point``: prev = the plan of (a): every placed container is kept and runs no reduction;
* ``d_grown``: prev = the plan of (a) after 15 % of the containers asked for half as much CPU again (and 100m).

Before anything is timed the answers are compared: (b) must equal (a) in assign, reason, cost and node tables
(``b_equals_a``), and (c) must return (a)'s assignment with every placed container KEPT (``c_is_fixed_point``).

Each figure is a host clock around one call that ends in a device synchronise, with the node tables restored
before it, after `warmup` calls of every leg; a round times `steps` calls of each leg in turn (a, b, c, d), so
the legs alternate, and the rounds' minimum, median and maximum are kept.  The kernels' own time comes from the
context's event brackets (FP_K_PLACE, FP_K_SORT) in a separate pass.  No time is a target.  Writes
profiles/replan_timing.json and prints it.
"""
import argparse
import dataclasses
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
LEGS = ("a_place", "b_no_prev", "c_fixed_point", "d_grown")


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=512)
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_timing.json"))
    a = ap.parse_args()
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    out = {"shape": {"scenarios": S, "containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "device": props.name, "compute_units": props.multi_processor_count,
           "order": "each round: steps calls of a_place, then of b_no_prev, c_fixed_point, d_grown",
           "grown": "rand(seed 3) < 0.15: cpu = cpu * 3 // 2 + 100", "strategies": {}}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        snap = db.node_snapshot()
        gen = torch.Generator(device="cpu").manual_seed(3)
        grown = (torch.rand(S * C, generator=gen) < 0.15).to(dev)
        cpu_g = torch.where(grown, db.cpu * 3 // 2 + 100, db.cpu).to(torch.int32)
        dbg = dataclasses.replace(db, cpu=cpu_g)
        no_prev = torch.full((S * C,), -1, dtype=torch.int32, device=dev)
        chg = torch.zeros(S * C, dtype=torch.uint8, device=dev)
        summ = torch.zeros(S * _lib.REPLAN_WORDS, dtype=torch.int32, device=dev)
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            # ---- the answers first ----
            db.restore_nodes(snap)
            p.dev_place_batch_policy(db, st)
            p.sync()
            plan, reason_a, cost_a = db.assign.clone(), db.reason.clone(), db.cost.clone()
            nodes_a = db.node_snapshot()
            calls = {"a_place": lambda: p.dev_place_batch_policy(db, st),
                     "b_no_prev": lambda: p.dev_replan_batch(db, no_prev, st, None, None, chg, summ),
                     "c_fixed_point": lambda: p.dev_replan_batch(db, plan, st, None, None, chg, summ),
                     "d_grown": lambda: p.dev_replan_batch(dbg, plan, st, None, None, chg, summ)}
            rec = {"placed": int((plan != -1).sum().item())}
            db.restore_nodes(snap)
            calls["b_no_prev"]()
            p.sync()
            rec["b_equals_a"] = bool(torch.equal(db.assign, plan) and torch.equal(db.reason, reason_a)
                                     and torch.equal(db.cost, cost_a)
                                     and all(torch.equal(x, y) for x, y in zip(db.node_snapshot(), nodes_a)))
            db.restore_nodes(snap)
            calls["c_fixed_point"]()
            p.sync()
            rec["c_is_fixed_point"] = bool(torch.equal(db.assign, plan) and torch.equal(db.reason, reason_a)
                                           and bool((chg[plan != -1] == _lib.CHANGE_KEPT).all().item())
                                           and all(torch.equal(x, y) for x, y in zip(db.node_snapshot(), nodes_a)))
            db.restore_nodes(snap)
            calls["d_grown"]()
            p.sync()
            words = summ.view(S, _lib.REPLAN_WORDS)[:, :5].long().sum(0).tolist()
            rec["d_changes"] = dict(zip(_lib.CHANGE_NAMES, words))
            # ---- wall time, the legs alternating ----
            for _ in range(a.warmup):
                for leg in LEGS:
                    db.restore_nodes(snap)
                    calls[leg]()
            p.sync()
            wall = {leg: [] for leg in LEGS}
            for _ in range(a.rounds):
                for leg in LEGS:
                    t = 0.0
                    for _ in range(a.steps):
                        db.restore_nodes(snap)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        calls[leg]()
                        p.sync()
                        t += time.perf_counter() - t0
                    wall[leg].append(1e3 * t / a.steps)
            # ---- the kernels' own time, in a pass of its own ----
            for leg in LEGS:
                p.profile(True)
                for _ in range(a.steps):
                    db.restore_nodes(snap)
                    calls[leg]()
                p.sync()
                kp, n = p.kernel_stats(_lib.FP_K_PLACE)
                ks, _ = p.kernel_stats(_lib.FP_K_SORT)
                p.profile(False)
                rec[leg] = {"ms_per_call": _stats(wall[leg]), "place_kernel_ms": kp / max(n, 1), "sort_ms": ks / max(n, 1)}
            base = rec["a_place"]["ms_per_call"]["median"]
            for leg in LEGS[1:]:
                rec[leg[0] + "_over_a"] = rec[leg]["ms_per_call"]["median"] / base
            out["strategies"][name] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
