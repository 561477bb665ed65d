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

    python tools/drain_timing.py --policy [--rounds R] [--parent-tree DIR]

The sweep under the policy (SPEC.md 2.15) on the same scenario, with the live state placed by
fp_dev_place_batch_policy_fallback under domain = n % 64, max_skew = 2 and the chain class -> region
(0x780, 0x78); candidates: every server alone, and the 64 zones (group = domain).  Every round is a fresh
process and times three legs:

1. ``plain``: fp_dev_drain_sweep, the unchanged 2.11 path, in a process that runs nothing else.  With
   --parent-tree (a checkout of the commit to compare with, its library built) the rounds alternate with a process
   that runs this same leg on that tree's package and library; ``within_parent_range`` says that this build's
   median over the rounds lies within the parent's own minimum and maximum.
2. ``policy``: fp_dev_drain_sweep_policy with both guarantees on.
3. ``replicated``: the same answer from fp_dev_place_batch_policy_fallback, one scenario per candidate with the
   candidate's nodes masked out of `schedulable` and out of the counts; ``same_plan`` (node, reason and hop of
   every evictee) is checked before anything is timed.

Writes profiles/drain_policy_timing.json and prints it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR (the --policy rounds): the checkout whose package and library this process measures
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else ROOT
sys.path.insert(0, TREE)

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


POLICY_DOMAINS, POLICY_MAX_SKEW, POLICY_CHAIN = 64, 2, (0x780, 0x78)


def build_policy_replicas(db, count, group, domain, S, dev):
    """build_replicas for SPEC.md 2.15: the counts of a candidate's own nodes are zero in its scenario, and every
    scenario carries the domains, max_skew and the chain.  Returns (batch, the call's keyword tensors, evictees,
    slots)."""
    b, counts, ev, slot = build_replicas(db, count, group, S, dev)
    N = db.N
    own = group.view(1, N) == torch.arange(S, dtype=group.dtype, device=dev).view(S, 1)
    counts = (counts.view(S, N) * (~own).to(torch.int32)).reshape(-1).contiguous()
    kw = dict(count_t=counts, domain_t=domain.repeat(S),
              max_skew_t=torch.full((S,), POLICY_MAX_SKEW, dtype=torch.int32, device=dev),
              relax_mask_t=torch.tensor(list(POLICY_CHAIN) + [0, 0], dtype=torch.int32, device=dev).repeat(S),
              n_hops_t=torch.full((S,), len(POLICY_CHAIN), dtype=torch.int32, device=dev),
              hops_t=torch.zeros(S * b.C, dtype=torch.uint8, device=dev))
    return b, kw, ev, slot


def policy_round(a):
    """One process's figures.  --plain-only (the parent build's process) times leg 1 alone."""
    C, N = a.containers, a.nodes
    dev = torch.device("cuda", 0)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    domain = torch.arange(N, dtype=torch.int32, device=dev) % POLICY_DOMAINS
    groupings = [("single_server", torch.arange(N, dtype=torch.int32, device=dev), N),
                 (f"zones_{POLICY_DOMAINS}", domain, POLICY_DOMAINS)]
    out = {}

    def per_call(p, fn):
        for _ in range(a.warmup):
            fn()
        p.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        p.sync()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    with Planner(0) as p:
        for name, sid in STRATEGIES:
            db = DevBatch.allocate(1, C, N, dev)
            p.dev_gen_batch(SEED4, db, 7)
            count = i32(N)
            st1 = torch.full((1,), sid, dtype=torch.int32, device=dev)
            p.dev_place_batch_policy_fallback(
                db, st1, None, count, domain_t=domain, max_skew_t=torch.full((1,), POLICY_MAX_SKEW, dtype=torch.int32, device=dev),
                relax_mask_t=torch.tensor(list(POLICY_CHAIN) + [0, 0], dtype=torch.int32, device=dev),
                n_hops_t=torch.full((1,), len(POLICY_CHAIN), dtype=torch.int32, device=dev))
            p.sync()
            cont_t, nodes_t = (db.cpu, db.mem, db.req, db.conf), (db.cf, db.mf, db.lab, db.cu, db.sched)
            rec = {"running": int((db.assign != -1).sum().item())}
            for label, group, S in groupings:
                a_out, reason, rows = i32(C), torch.zeros(C, dtype=torch.uint8, device=dev), i32(S * _lib.DRAIN_WORDS)
                g = {"n_cand": S}
                g["plain_ms"] = per_call(p, lambda: p.dev_drain_sweep(cont_t, nodes_t, db.assign, group, S, a_out, reason,
                                                                      rows, sid, 0, count))
                if a.plain_only:
                    rec[label] = g
                    continue
                hops, prow = torch.zeros(C, dtype=torch.uint8, device=dev), i32(S * _lib.DRAIN_POLICY_WORDS)
                stS = torch.full((S,), sid, dtype=torch.int32, device=dev)

                def sweep():
                    p.dev_drain_sweep_policy(cont_t, nodes_t, db.assign, group, S, a_out, reason, rows, sid, 0, count,
                                             domain_t=domain, max_skew=POLICY_MAX_SKEW, relax_mask=POLICY_CHAIN,
                                             hops_t=hops, policy_t=prow)

                def replicated():
                    b, kw, ev, slot = build_policy_replicas(db, count, group, domain, S, dev)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    p.dev_place_batch_policy_fallback(b, stS, None, **kw)
                    p.sync()
                    return time.perf_counter() - t0, b, kw, ev, slot

                # ---- the same answer first ----
                sweep()
                p.sync()
                _, b, kw, ev, slot = replicated()
                placed = b.assign[slot] != -1
                same = (bool(torch.equal(b.assign[slot], a_out[ev])) and bool(torch.equal(b.reason[slot], reason[ev]))
                        and bool(torch.equal(kw["hops_t"][slot] * placed.to(torch.uint8), hops[ev])))
                summary, pol = rows.view(S, _lib.DRAIN_WORDS), prow.view(S, _lib.DRAIN_POLICY_WORDS)
                g.update(evictees=int(ev.numel()), max_evictees=b.C, same_plan=same,
                         stranded=int(summary[:, _lib.DRAIN_STRANDED].sum().item()),
                         stranded_skew=int(pol[:, _lib.DRAIN_STRANDED_SKEW].sum().item()),
                         relaxed=int(pol[:, _lib.DRAIN_RELAXED].sum().item()),
                         candidates_outside_before=int((pol[:, _lib.DRAIN_SKEW_BEFORE] > POLICY_MAX_SKEW).sum().item()))
                del b, kw
                g["policy_ms"] = per_call(p, sweep)
                for _ in range(a.warmup):
                    replicated()
                tb = tc = 0.0
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    dt, *_ = replicated()
                    tb += time.perf_counter() - t0 - dt
                    tc += dt
                g["replicated_build_ms"], g["replicated_call_ms"] = 1e3 * tb / a.steps, 1e3 * tc / a.steps
                p.profile(True)
                for _ in range(a.steps):
                    sweep()
                p.sync()
                kp, n = p.kernel_stats(_lib.FP_K_PLACE)
                p.profile(False)
                g["policy_kernel_ms"] = kp / max(n, 1)
                rec[label] = g
                torch.cuda.empty_cache()
            out[name] = rec
    return out


def _child(cmd, cwd, out_path):
    import subprocess
    subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.DEVNULL)
    with open(out_path) as f:
        return json.load(f)


def policy_main(a):
    """The driver: starts every round as a child process and makes no GPU call itself."""
    import tempfile
    shape = ["--containers", str(a.containers), "--nodes", str(a.nodes), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    me = os.path.abspath(__file__)
    new_rounds, plain_rounds, parent_rounds = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            if a.parent_tree:
                path = os.path.join(tmp, f"parent{r}.json")
                parent_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--plain-only", "--out", path,
                                             "--tree", os.path.abspath(a.parent_tree)], os.path.abspath(a.parent_tree), path))
            path = os.path.join(tmp, f"plain{r}.json")
            plain_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--plain-only", "--out", path,
                                        "--tree", ROOT], ROOT, path))
            path = os.path.join(tmp, f"new{r}.json")
            new_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--out", path, "--tree", ROOT], ROOT, path))
            print(f"round {r + 1} of {a.rounds} done", file=sys.stderr, flush=True)
    out = {"shape": {"containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4}, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds,
           "policy": {"domain": f"n % {POLICY_DOMAINS}", "max_skew": POLICY_MAX_SKEW, "relax_mask": [hex(m) for m in POLICY_CHAIN]},
           "order": "each round: the parent build's process (leg 1), this build's (leg 1), this build's (legs 2 and 3)",
           "acceptance": "leg 1: this build's median over the rounds within the parent's min and max over the rounds",
           "strategies": {}}
    for name, _ in STRATEGIES:
        rec = {"running": new_rounds[0][name]["running"]}
        for label in (k for k in new_rounds[0][name] if k != "running"):
            runs = [r[name][label] for r in new_rounds]
            g = {k: runs[0][k] for k in ("n_cand", "evictees", "max_evictees", "stranded", "stranded_skew", "relaxed",
                                         "candidates_outside_before")}
            g["same_plan"] = all(x["same_plan"] for x in runs)
            mine = [r[name][label]["plain_ms"] for r in plain_rounds]
            g["plain"] = {"ms_per_call": _stats(mine), "rounds": mine}
            if parent_rounds:
                pr = [r[name][label]["plain_ms"] for r in parent_rounds]
                g["parent_plain"] = {"ms_per_call": _stats(pr), "rounds": pr}
                g["within_parent_range"] = min(pr) <= g["plain"]["ms_per_call"]["median"] <= max(pr)
            g["policy"] = {"ms_per_call": _stats([x["policy_ms"] for x in runs]),
                           "sweep_kernel_ms": _stats([x["policy_kernel_ms"] for x in runs])}
            g["replicated"] = {"build_ms": _stats([x["replicated_build_ms"] for x in runs]),
                               "call_ms": _stats([x["replicated_call_ms"] for x in runs])}
            g["policy_over_plain"] = g["policy"]["ms_per_call"]["median"] / g["plain"]["ms_per_call"]["median"]
            g["replicated_call_over_policy"] = g["replicated"]["call_ms"]["median"] / g["policy"]["ms_per_call"]["median"]
            rec[label] = g
        out["strategies"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--policy", action="store_true", help="the sweep under the policy (see above)")
    ap.add_argument("--parent-tree", default=None, help="--policy: a built checkout of the commit to compare leg 1 with")
    ap.add_argument("--policy-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.policy or a.policy_child:
        res = policy_round(a) if a.policy_child else policy_main(a)
        path = a.out or os.path.join(ROOT, "profiles", "drain_policy_timing.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "drain_timing.json")
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
