"""Scored-placement timing (SPEC.md 2.6) on the config-4 batch shape, on cuda:0.

    python tools/policy_timing.py [--scenarios S] [--containers C] [--nodes N] [--steps K] [--warmup W]

Times Planner.dev_place_batch_policy per strategy on S what-if scenarios of C x N (default: the
512-scenario slice one of eight ranks plans of config 4's 4096 x 50k x 5k; --scenarios 4096 is the
whole batch), and the first-fit dev_place_batch on the same batch beside them.  The first-fit figure
is there for scale only: the two kernels do different work (first fit prunes on monotonicity, a
scored rule takes an argmin over every node for every container).

Each figure is a host clock around `steps` calls that end in a device synchronise, after `warmup`
calls, with the node state restored before each call; the placer's and the sort's own time come from
the context's event brackets (FP_K_PLACE, FP_K_SORT) in a separate pass.  Writes
profiles/policy_timing.json and prints it.

    python tools/policy_timing.py --spread [--rounds R] [--parent-tree DIR]

The hard topology spread (SPEC.md 2.7) on and off, per strategy, on the same batch: the unconstrained
call, and fp_dev_place_batch_policy_spread with domain = n % D for D in {4, 64} and max_skew = 1.  Every
round is a fresh process; with --parent-tree (a checkout of the commit to compare with, its library
built) the rounds alternate with that tree's own tools/policy_timing.py, so the unconstrained calls of
both builds are measured side by side in one run.  Writes profiles/policy_spread_timing.json: every
round's figures, and their minimum, median and maximum.

    python tools/policy_timing.py --fallback [--rounds R] [--parent-tree DIR]

The fallback chain (SPEC.md 2.8) by the same method: per strategy the calls without a chain (the
unconstrained call and the two constrained ones of --spread) and fp_dev_place_batch_policy_fallback with
n_hops = 2 (class, region) and n_hops = 4 (class, region, arch, tier) over the generator's label
dimensions (SPEC.md 3.2).  With --parent-tree the rounds alternate with that tree's `--spread-child`
process, and every call without a chain is held against the parent build: its median may exceed the
parent's maximum by at most the parent's own min-max range over the rounds (`within_margin`).  The
calls with a chain have no target: their time, ns per placement and hop histogram are recorded.  Writes
profiles/policy_fallback_timing.json.

    python tools/policy_timing.py --quota [--rounds R] [--parent-tree DIR]

The resource quota (SPEC.md 2.10) by the same method, per strategy: (a) the unconstrained call (`off`) and the
fallback call (`fb_h2`) of this build against the same calls of the parent build's `--fallback-child` process,
held to the same margin (`within_margin`): the kernels without a quota must not have moved; (b) `quota_unlimited`,
fp_dev_place_batch_policy_quota over the fb_h2 chain with every cap FP_QUOTA_UNLIMITED, against this build's
fb_h2: the price of the quota kernel itself (`vs_fb_h2`, the ratio of the medians); (c) `quota_half`, the same call
with each scenario's caps at half of what its fb_h2 plan uses, where the refused containers skip the argmin.  (b)
and (c) have no target.  Writes profiles/policy_quota_timing.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fleetflow_amd import DevBatch, Planner, _lib  # noqa: E402

SEED4 = 0x5EED0004
STRATEGIES = (("first_fit_scored", 0), ("spread_across_pool", 1), ("pack_into_dedicated", 2), ("fill_lowest", 3))


def timed(p, db, snap, call, steps, warmup):
    """(wall ms, placer kernel ms, sort ms) per call."""
    for _ in range(warmup):
        db.restore_nodes(snap)
        call()
    p.sync()
    torch.cuda.synchronize()
    wall = 0.0
    for _ in range(steps):
        db.restore_nodes(snap)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        p.sync()
        wall += time.perf_counter() - t0
    p.profile(True)
    for _ in range(steps):
        db.restore_nodes(snap)
        call()
    p.sync()
    place_ms, n_place = p.kernel_stats(_lib.FP_K_PLACE)
    sort_ms, _ = p.kernel_stats(_lib.FP_K_SORT)
    p.profile(False)
    return 1e3 * wall / steps, place_ms / max(n_place, 1), sort_ms / max(n_place, 1)


SPREAD_DOMAINS = (4, 64)


def spread_round(a):
    """One process's figures: per strategy the unconstrained call and the constrained one per D."""
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rounds = -(-S // cus) if N > 64 else None
    out = {}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        snap = db.node_snapshot()
        skew = torch.ones(S, dtype=torch.int32, device=dev)
        doms = {D: (torch.arange(N, dtype=torch.int32, device=dev) % D).repeat(S) for D in SPREAD_DOMAINS}
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            calls = [("off", lambda: p.dev_place_batch_policy(db, st))]
            calls += [(f"on_D{D}", lambda D=D: p.dev_place_batch_policy(db, st, domain_t=doms[D], max_skew_t=skew))
                      for D in SPREAD_DOMAINS]
            out[name] = {}
            for label, call in calls:
                wall, place_ms, sort_ms = timed(p, db, snap, call, a.steps, a.warmup)
                reason = db.reason
                rec = {"ms_per_call": wall, "place_kernel_ms": place_ms, "sort_ms": sort_ms,
                       "rejected": int((reason != 0).sum().item()), "skew": int((reason == _lib.REASON_SKEW).sum().item())}
                if rounds:
                    rec["ns_per_placement"] = 1e6 * place_ms / (rounds * C)
                out[name][label] = rec
    return out


# the generator's label dimensions (SPEC.md 3.2): tier bits 0-2, region 3-6, class 7-10, arch 11-12
FALLBACK_CHAINS = {"fb_h2": [0x780, 0x78], "fb_h4": [0x780, 0x78, 0x1800, 0x7]}


def fallback_round(a):
    """One process's figures: spread_round's calls, and the calls with a chain per FALLBACK_CHAINS."""
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rounds = -(-S // cus) if N > 64 else None
    out = {}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        snap = db.node_snapshot()
        skew = torch.ones(S, dtype=torch.int32, device=dev)
        doms = {D: (torch.arange(N, dtype=torch.int32, device=dev) % D).repeat(S) for D in SPREAD_DOMAINS}
        hops = torch.zeros(S * C, dtype=torch.uint8, device=dev)
        chains = {}
        for label, masks in FALLBACK_CHAINS.items():
            row = masks + [0] * (_lib.FP_FALLBACK_MAX_HOPS - len(masks))
            chains[label] = (torch.tensor(row * S, dtype=torch.int32, device=dev),
                             torch.full((S,), len(masks), dtype=torch.int32, device=dev))
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            calls = [("off", lambda: p.dev_place_batch_policy(db, st))]
            calls += [(f"on_D{D}", lambda D=D: p.dev_place_batch_policy(db, st, domain_t=doms[D], max_skew_t=skew))
                      for D in SPREAD_DOMAINS]
            calls += [(label, lambda label=label: p.dev_place_batch_policy_fallback(
                db, st, relax_mask_t=chains[label][0], n_hops_t=chains[label][1], hops_t=hops)) for label in FALLBACK_CHAINS]
            out[name] = {}
            for label, call in calls:
                wall, place_ms, sort_ms = timed(p, db, snap, call, a.steps, a.warmup)
                reason = db.reason
                rec = {"ms_per_call": wall, "place_kernel_ms": place_ms, "sort_ms": sort_ms,
                       "rejected": int((reason != 0).sum().item()), "skew": int((reason == _lib.REASON_SKEW).sum().item())}
                if rounds:
                    rec["ns_per_placement"] = 1e6 * place_ms / (rounds * C)
                if label in FALLBACK_CHAINS:  # placed containers per hop
                    rec["hop_histogram"] = torch.bincount(hops[reason == 0].long(),
                                                          minlength=_lib.FP_FALLBACK_MAX_HOPS + 1).tolist()
                out[name][label] = rec
    return out


QUOTA_CHAIN = "fb_h2"


def quota_round(a):
    """One process's figures: per strategy the unconstrained call, the fallback call, and the quota call over the
    same chain with every cap unlimited and with caps at half of each scenario's usage under the fallback call."""
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rounds = -(-S // cus) if N > 64 else None
    out = {}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        snap = db.node_snapshot()
        hops = torch.zeros(S * C, dtype=torch.uint8, device=dev)
        why = torch.zeros(S * C, dtype=torch.uint8, device=dev)
        masks = FALLBACK_CHAINS[QUOTA_CHAIN]
        relax = torch.tensor((masks + [0] * (_lib.FP_FALLBACK_MAX_HOPS - len(masks))) * S, dtype=torch.int32, device=dev)
        nh = torch.full((S,), len(masks), dtype=torch.int32, device=dev)
        unlimited = torch.full((S * _lib.QUOTA_DIMS,), -1, dtype=torch.int32, device=dev)
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            half = unlimited.clone()  # filled in after the fallback call, from its plan

            def fallback():
                p.dev_place_batch_policy_fallback(db, st, relax_mask_t=relax, n_hops_t=nh, hops_t=hops)

            def quota(caps):
                p.dev_place_batch_policy_quota(db, st, caps, relax_mask_t=relax, n_hops_t=nh, hops_t=hops, quota_why_t=why)
            calls = [("off", lambda: p.dev_place_batch_policy(db, st)), (QUOTA_CHAIN, fallback),
                     ("quota_unlimited", lambda: quota(unlimited)), ("quota_half", lambda: quota(half))]
            out[name] = {}
            for label, call in calls:
                wall, place_ms, sort_ms = timed(p, db, snap, call, a.steps, a.warmup)
                reason = db.reason
                rec = {"ms_per_call": wall, "place_kernel_ms": place_ms, "sort_ms": sort_ms,
                       "rejected": int((reason != 0).sum().item()),
                       "quota": int((reason == _lib.REASON_QUOTA).sum().item())}
                if rounds:
                    rec["ns_per_placement"] = 1e6 * place_ms / (rounds * C)
                if label == QUOTA_CHAIN:  # each scenario's usage under this plan: cpu, memory, services
                    placed = (db.assign.view(S, C) != -1).long()
                    use = torch.stack([(db.cpu.view(S, C).long() * placed).sum(1), (db.mem.view(S, C).long() * placed).sum(1),
                                       placed.sum(1)], 1)
                    half.copy_((use // 2).to(torch.int32).reshape(-1))  # below 2^31 on this shape
                out[name][label] = rec
    return out


def quota_main(a):
    """The driver: starts every round as a child process and makes no GPU call itself."""
    shape = ["--scenarios", str(a.scenarios), "--containers", str(a.containers), "--nodes", str(a.nodes), "--steps", str(a.steps),
             "--warmup", str(a.warmup)]
    new_rounds, parent_rounds = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            if a.parent_tree:
                path = os.path.join(tmp, f"parent{r}.json")
                tool = os.path.join(os.path.abspath(a.parent_tree), "tools", "policy_timing.py")
                parent_rounds.append(_child([sys.executable, tool, *shape, "--fallback-child", "--out", path],
                                            os.path.abspath(a.parent_tree), path))
            path = os.path.join(tmp, f"new{r}.json")
            new_rounds.append(_child([sys.executable, os.path.abspath(__file__), *shape, "--quota-child", "--out", path], ROOT, path))
    held = ["off", QUOTA_CHAIN]
    out = {"shape": {"scenarios": a.scenarios, "containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4},
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "chain": {QUOTA_CHAIN: [hex(m) for m in FALLBACK_CHAINS[QUOTA_CHAIN]]},
           "caps": {"quota_unlimited": "FP_QUOTA_UNLIMITED in every dimension",
                    "quota_half": "per scenario, half of the cpu, memory and services its fb_h2 plan uses"},
           "order": "each round: the parent build's process, then this build's",
           "margin": "a call without a quota: this build's median <= the parent's max + (the parent's max - min)",
           "strategies": {}}
    for name, _ in STRATEGIES:
        rec = {}
        for label in held + ["quota_unlimited", "quota_half"]:
            runs = [r[name][label] for r in new_rounds]
            rec[label] = {"place_kernel_ms": _stats([x["place_kernel_ms"] for x in runs]),
                          "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                          "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                          "rejected": runs[0]["rejected"], "quota": runs[0]["quota"]}
            if "ns_per_placement" in runs[0]:
                rec[label]["ns_per_placement"] = _stats([x["ns_per_placement"] for x in runs])
        for label in ("quota_unlimited", "quota_half"):
            rec[label]["vs_" + QUOTA_CHAIN] = rec[label]["place_kernel_ms"]["median"] / rec[QUOTA_CHAIN]["place_kernel_ms"]["median"]
        for label in held if parent_rounds else []:
            runs = [r[name][label] for r in parent_rounds]
            st = _stats([x["place_kernel_ms"] for x in runs])
            rec["parent_" + label] = {"place_kernel_ms": st, "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                                      "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                                      "rejected": runs[0]["rejected"]}
            rec[label]["within_margin"] = rec[label]["place_kernel_ms"]["median"] <= st["max"] + (st["max"] - st["min"])
        out["strategies"][name] = rec
    return out


def fallback_main(a):
    """The driver: starts every round as a child process and makes no GPU call itself."""
    shape = ["--scenarios", str(a.scenarios), "--containers", str(a.containers), "--nodes", str(a.nodes), "--steps", str(a.steps),
             "--warmup", str(a.warmup)]
    new_rounds, parent_rounds = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            if a.parent_tree:
                path = os.path.join(tmp, f"parent{r}.json")
                tool = os.path.join(os.path.abspath(a.parent_tree), "tools", "policy_timing.py")
                parent_rounds.append(_child([sys.executable, tool, *shape, "--spread-child", "--out", path],
                                            os.path.abspath(a.parent_tree), path))
            path = os.path.join(tmp, f"new{r}.json")
            new_rounds.append(_child([sys.executable, os.path.abspath(__file__), *shape, "--fallback-child", "--out", path], ROOT, path))
    plain = ["off"] + [f"on_D{D}" for D in SPREAD_DOMAINS]
    out = {"shape": {"scenarios": a.scenarios, "containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4},
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "domain_map": "n % D", "max_skew": 1,
           "chains": {k: [hex(m) for m in v] for k, v in FALLBACK_CHAINS.items()},
           "order": "each round: the parent build's process, then this build's",
           "margin": "a call without a chain: this build's median <= the parent's max + (the parent's max - min)",
           "strategies": {}}
    for name, _ in STRATEGIES:
        rec = {}
        for label in plain + list(FALLBACK_CHAINS):
            runs = [r[name][label] for r in new_rounds]
            rec[label] = {"place_kernel_ms": _stats([x["place_kernel_ms"] for x in runs]),
                          "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                          "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                          "rejected": runs[0]["rejected"], "skew": runs[0]["skew"]}
            if "ns_per_placement" in runs[0]:
                rec[label]["ns_per_placement"] = _stats([x["ns_per_placement"] for x in runs])
            if "hop_histogram" in runs[0]:
                rec[label]["hop_histogram"] = runs[0]["hop_histogram"]
        for label in plain if parent_rounds else []:
            runs = [r[name][label] for r in parent_rounds]
            st = _stats([x["place_kernel_ms"] for x in runs])
            rec["parent_" + label] = {"place_kernel_ms": st, "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                                      "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                                      "rejected": runs[0]["rejected"]}
            rec[label]["within_margin"] = rec[label]["place_kernel_ms"]["median"] <= st["max"] + (st["max"] - st["min"])
        out["strategies"][name] = rec
    return out


def _child(cmd, cwd, out_path):
    subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL)
    with open(out_path) as f:
        return json.load(f)


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def spread_main(a):
    """The driver: starts every round as a child process and makes no GPU call itself."""
    shape = ["--scenarios", str(a.scenarios), "--containers", str(a.containers), "--nodes", str(a.nodes), "--steps", str(a.steps),
             "--warmup", str(a.warmup)]
    new_rounds, parent_rounds = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            if a.parent_tree:
                path = os.path.join(tmp, f"parent{r}.json")
                tool = os.path.join(os.path.abspath(a.parent_tree), "tools", "policy_timing.py")
                parent_rounds.append(_child([sys.executable, tool, *shape, "--out", path], os.path.abspath(a.parent_tree), path))
            path = os.path.join(tmp, f"new{r}.json")
            new_rounds.append(_child([sys.executable, os.path.abspath(__file__), *shape, "--spread-child", "--out", path], ROOT, path))
    out = {"shape": {"scenarios": a.scenarios, "containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4},
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "domain_map": "n % D", "max_skew": 1,
           "order": "each round: the parent build's process, then this build's", "strategies": {}}
    for name, _ in STRATEGIES:
        rec = {}
        for label in ["off"] + [f"on_D{D}" for D in SPREAD_DOMAINS]:
            runs = [r[name][label] for r in new_rounds]
            rec[label] = {"place_kernel_ms": _stats([x["place_kernel_ms"] for x in runs]),
                          "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                          "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                          "rejected": runs[0]["rejected"], "skew": runs[0]["skew"]}
            if "ns_per_placement" in runs[0]:
                rec[label]["ns_per_placement"] = _stats([x["ns_per_placement"] for x in runs])
        if parent_rounds:
            runs = [r["strategies"][name] for r in parent_rounds]
            rec["parent_off"] = {"place_kernel_ms": _stats([x["place_kernel_ms"] for x in runs]),
                                 "ms_per_call": _stats([x["ms_per_call"] for x in runs]),
                                 "place_kernel_ms_rounds": [x["place_kernel_ms"] for x in runs],
                                 "rejected": runs[0]["rejected"]}
        out["strategies"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=512)
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--spread", action="store_true", help="the topology spread on and off (see above)")
    ap.add_argument("--rounds", type=int, default=3, help="--spread, --fallback, --quota: processes per build")
    ap.add_argument("--parent-tree", default=None,
                    help="--spread, --fallback, --quota: a built checkout of the commit to compare with")
    ap.add_argument("--spread-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fallback", action="store_true", help="the fallback chain on and off (see above)")
    ap.add_argument("--fallback-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--quota", action="store_true", help="the resource quota on and off (see above)")
    ap.add_argument("--quota-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "policy_quota_timing.json" if a.quota else
                             "policy_fallback_timing.json" if a.fallback else
                             "policy_spread_timing.json" if a.spread else "policy_timing.json")
    if a.spread or a.spread_child or a.fallback or a.fallback_child or a.quota or a.quota_child:
        out = (spread_round(a) if a.spread_child else fallback_round(a) if a.fallback_child else
               quota_round(a) if a.quota_child else quota_main(a) if a.quota else
               fallback_main(a) if a.fallback else spread_main(a))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    S, C, N = a.scenarios, a.containers, a.nodes
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    cus = props.multi_processor_count
    out = {"shape": {"scenarios": S, "containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "steps": a.steps,
           "warmup": a.warmup, "device": props.name, "compute_units": cus, "strategies": {}}
    with Planner(0) as p:
        db = DevBatch.allocate(S, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        snap = db.node_snapshot()
        wall, place_ms, sort_ms = timed(p, db, snap, lambda: p.dev_place_batch(db), a.steps, a.warmup)
        out["first_fit_pipeline"] = {"ms_per_call": wall, "place_kernel_ms": place_ms, "sort_ms": sort_ms,
                                     "rejected": int((db.reason != 0).sum().item())}
        ff_assign = db.assign.clone()
        # one 1024-thread workgroup per scenario and compute unit (N > 64; at most 4 waves per SIMD at
        # 8 nodes a thread), so a batch takes ceil(S / CUs) rounds of C dependent placements
        rounds = -(-S // cus) if N > 64 else None
        for name, sid in STRATEGIES:
            st = torch.full((S,), sid, dtype=torch.int32, device=dev)
            wall, place_ms, sort_ms = timed(p, db, snap, lambda: p.dev_place_batch_policy(db, st), a.steps, a.warmup)
            rec = {"ms_per_call": wall, "place_kernel_ms": place_ms, "sort_ms": sort_ms,
                   "rejected": int((db.reason != 0).sum().item())}
            if rounds:
                ns = 1e6 * place_ms / (rounds * C)
                rec["ns_per_placement"] = ns  # per workgroup: the dependent chain's step time
                rec["cycles_per_placement_at_2400MHz"] = ns * 2.4
            if sid == 0:  # the scored kernel under strategy 0 is first fit: the same plan
                rec["same_plan_as_first_fit"] = bool(torch.equal(db.assign, ff_assign))
            out["strategies"][name] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
