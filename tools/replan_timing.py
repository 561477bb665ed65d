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

    python tools/replan_timing.py --policy [...]

The same four legs under the policy (SPEC.md 2.14), with the spread constraint (domain = n % 4, max_skew 4), the
chain [0x780, 0x78] and a quota on: per scenario, three quarters of the cpu, memory and services its plan uses
without a cap.  (a) is fp_dev_place_batch_policy_quota, (b) to (d) are fp_dev_replan_batch_policy.  (b) must
equal (a) in every output, hops, quota_why and the usage included; (c) is theorem D: every placed container KEPT
on its node with its hop, and the same assignment when (a) rejected nothing for SKEW.  If either fails the
tool stops before it times anything.  Writes profiles/replan_policy_timing.json.
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
    ap.add_argument("--policy", action="store_true", help="under spread + chain + quota (SPEC.md 2.14)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "replan_policy_timing.json" if a.policy else "replan_timing.json")
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
        if a.policy:
            out["policy"] = {"domain": "n % 4", "max_skew": 4, "relax_mask": [0x780, 0x78], "n_hops": 2,
                             "quota": "per scenario, 3/4 of the cpu, memory and services its uncapped plan uses"}
            pk = dict(domain_t=(torch.arange(S * N, device=dev) % N % 4).to(torch.int32),
                      max_skew_t=torch.full((S,), 4, dtype=torch.int32, device=dev),
                      relax_mask_t=torch.tensor([0x780, 0x78, 0, 0] * S, dtype=torch.int32, device=dev),
                      n_hops_t=torch.full((S,), 2, dtype=torch.int32, device=dev),
                      hops_t=torch.zeros(S * C, dtype=torch.uint8, device=dev),
                      quota_why_t=torch.zeros(S * C, dtype=torch.uint8, device=dev))
            used = torch.zeros(S * _lib.QUOTA_DIMS, dtype=torch.int32, device=dev)
        else:
            used = None

        def restore():  # the base state of every call: the node tables (dbg shares db's) and, under the policy, the usage
            db.restore_nodes(snap)
            if used is not None:
                used.zero_()
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            # ---- the answers first ----
            restore()
            if a.policy:
                caps = torch.full((S * _lib.QUOTA_DIMS,), -1, dtype=torch.int32, device=dev)
                p.dev_place_batch_policy_quota(db, st, caps, used, **pk)
                p.sync()
                caps = (used.long() * 3 // 4).to(torch.int32)  # below 2^31 on this shape
                restore()
                calls = {"a_place": lambda: p.dev_place_batch_policy_quota(db, st, caps, used, **pk),
                         "b_no_prev": lambda: p.dev_replan_batch_policy(db, no_prev, st, caps, used, **pk, change_t=chg,
                                                                        summary_t=summ),
                         "c_fixed_point": lambda: p.dev_replan_batch_policy(db, plan, st, caps, used, **pk, change_t=chg,
                                                                            summary_t=summ),
                         "d_grown": lambda: p.dev_replan_batch_policy(dbg, plan, st, caps, used, **pk, change_t=chg,
                                                                      summary_t=summ)}
                extra = lambda: (pk["hops_t"].clone(), pk["quota_why_t"].clone(), used.clone())  # noqa: E731
            else:
                calls = {"a_place": lambda: p.dev_place_batch_policy(db, st),
                         "b_no_prev": lambda: p.dev_replan_batch(db, no_prev, st, None, None, chg, summ),
                         "c_fixed_point": lambda: p.dev_replan_batch(db, plan, st, None, None, chg, summ),
                         "d_grown": lambda: p.dev_replan_batch(dbg, plan, st, None, None, chg, summ)}
                extra = lambda: ()  # noqa: E731
            calls["a_place"]()
            p.sync()
            plan, reason_a, cost_a = db.assign.clone(), db.reason.clone(), db.cost.clone()
            nodes_a, extra_a = db.node_snapshot(), extra()
            rec = {"placed": int((plan != -1).sum().item())}
            if a.policy:
                rec["reasons"] = dict(zip(("ok", "nofit", "cycle", "skew", "quota"),
                                          torch.bincount(reason_a.long(), minlength=5).tolist()))
            restore()
            calls["b_no_prev"]()
            p.sync()
            rec["b_equals_a"] = bool(torch.equal(db.assign, plan) and torch.equal(db.reason, reason_a)
                                     and torch.equal(db.cost, cost_a)
                                     and all(torch.equal(x, y) for x, y in zip(db.node_snapshot(), nodes_a))
                                     and all(torch.equal(x, y) for x, y in zip(extra(), extra_a)))
            restore()
            calls["c_fixed_point"]()
            p.sync()
            was = plan != -1
            if a.policy:  # theorem D, as far as it goes
                same = bool(torch.equal(db.assign[was], plan[was]) and (chg[was] == _lib.CHANGE_KEPT).all().item()
                            and torch.equal(pk["hops_t"][was], extra_a[0][was]))
                if not bool((reason_a == _lib.REASON_SKEW).any().item()):
                    same = same and bool(torch.equal(db.assign, plan) and torch.equal(used, extra_a[2])
                                         and all(torch.equal(x, y) for x, y in zip(db.node_snapshot(), nodes_a)))
                rec["c_is_theorem_d"] = same
                rec["c_skew_placed"] = int(((reason_a == _lib.REASON_SKEW) & (db.assign != -1)).sum().item())
                if not (rec["b_equals_a"] and same):  # a wrong answer is not worth timing
                    raise SystemExit(f"{name}: b_equals_a = {rec['b_equals_a']}, c_is_theorem_d = {same}: not timed")
            else:
                rec["c_is_fixed_point"] = bool(torch.equal(db.assign, plan) and torch.equal(db.reason, reason_a)
                                               and bool((chg[was] == _lib.CHANGE_KEPT).all().item())
                                               and all(torch.equal(x, y) for x, y in zip(db.node_snapshot(), nodes_a)))
            restore()
            calls["d_grown"]()
            p.sync()
            words = summ.view(S, _lib.REPLAN_WORDS)[:, :5].long().sum(0).tolist()
            rec["d_changes"] = dict(zip(_lib.CHANGE_NAMES, words))
            # ---- wall time, the legs alternating ----
            for _ in range(a.warmup):
                for leg in LEGS:
                    restore()
                    calls[leg]()
            p.sync()
            wall = {leg: [] for leg in LEGS}
            for _ in range(a.rounds):
                for leg in LEGS:
                    t = 0.0
                    for _ in range(a.steps):
                        restore()
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
                    restore()
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
