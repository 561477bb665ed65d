"""Scale-in sweep timing (SPEC.md 2.16) on one config-4 scenario, on cuda:0.

    python tools/shrink_timing.py [--containers C] [--nodes N] [--strategy S] [--steps K] [--warmup W] [--rounds R]

One scenario of C x N (default 50k x 5k, the generator's config-4 inputs) is placed by
fp_dev_place_batch_policy; that plan and the node table it leaves are the live state ``as_placed``.  The fleet
is then nearly full, so nearly every attempt ends at its first evictee; ``roomy`` is the same plan on servers
that each have room for a few more requests (twice the largest request added to cpu_free and mem_free), where
attempts commit and services move.  On each of the two the tool times

* ``sweep``: fp_dev_shrink_sweep for 1, 8 and 64 variants that each try every node.  Variant 0 tries the nodes
  by running containers ascending (the `fewest` rule), the others in seeded random orders;
* ``scan_only``: the same one-variant call on a copy of the table with every node cordoned, so that every attempt
  on an occupied node scans for its evictees and ends at its first one: what the evictee scans cost without
  the moves;
* ``host_loop``: the same answer for variant 0 the way a caller gets it without the sweep: per attempt one
  single-candidate fp_dev_drain_sweep, one word read back (STRANDED), and on success the commit on the device
  (the moved requests deducted on their targets, the counts, the node cordoned, the new plan).

Each figure is a host clock around calls that end in a device synchronise, after `warmup` calls of the sweep
legs and one untimed host loop (the comparison); a round times the legs one after the other (1, 8, 64 variants and
scan only, `steps` calls each, then the host loop once, which is 5 000 drain calls), and the rounds' minimum,
median and maximum are kept.  The sweep kernel's own time comes from the context's event brackets
(FP_K_PLACE, FP_K_SORT) in a separate pass.  Before anything is timed the host loop's final plan and released
nodes are compared with variant 0's: ``same_plan``.  Writes profiles/shrink_timing.json and prints it.

    python tools/shrink_timing.py --policy [--rounds R] [--parent-tree DIR]

The sweep under the policy (SPEC.md 2.17): the same scenario placed under spread_across_pool with a spread
constraint (domain = n % 64, max_skew 2) and a fallback chain of two hops, on the `roomy` state.  Three legs, every
round in processes of its own that the driver starts one after the other (it makes no GPU call itself):

1. ``plain``: fp_dev_shrink_sweep, one variant (`fewest`), by this build; with --parent-tree (a checkout of the
   commit to compare with, its library built) the rounds alternate with a process that runs this same leg on that
   tree's package and library, the two taking turns at going first; ``within_parent_range`` says that this
   build's median over the rounds is no higher than the parent's own maximum over the rounds.
2. ``policy``: fp_dev_shrink_sweep_policy for 1 and 8 variants.
3. ``host_loop``: what the policy sweep replaces for ONE variant: per attempt a single-candidate
   fp_dev_drain_sweep_policy, the STRANDED word read back, the bound rule's two skews from the domain counts, and
   on success the commit on the device.  Its final plan and released nodes are compared with variant 0's first.

Writes profiles/shrink_policy_timing.json and prints it.
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
STRATEGIES = {"first_fit_scored": 0, "spread_across_pool": 1, "pack_into_dedicated": 2, "fill_lowest": 3}
VARIANTS = (1, 8, 64)
POLICY_DOMAINS, POLICY_MAX_SKEW, POLICY_CHAIN, POLICY_VARIANTS = 64, 2, (0x780, 0x78), (1, 8)


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def host_loop(p, cont_t, nodes_t, assign, count, order, sid, dev):
    """Variant `order` by one drain sweep and one commit per attempt.  Returns (final assign, released mask,
    attempts, failed)."""
    C, N = assign.numel(), count.numel()
    cf, mf, lab, cu, sched = (t.clone() for t in nodes_t)
    cur, cnt = assign.clone(), count.clone()
    out = torch.zeros(C, dtype=torch.int32, device=dev)
    reason = torch.zeros(C, dtype=torch.uint8, device=dev)
    row = torch.zeros(_lib.DRAIN_WORDS, dtype=torch.int32, device=dev)
    group = torch.full((N,), -1, dtype=torch.int32, device=dev)
    released = torch.zeros(N, dtype=torch.bool, device=dev)
    failed = 0
    for n in order.tolist():
        group[n] = 0
        p.dev_drain_sweep(cont_t, (cf, mf, lab, cu, sched), cur, group, 1, out, reason, row, sid, 0, cnt)
        group[n] = -1
        if int(row[_lib.DRAIN_STRANDED].item()):  # the read-back synchronises
            failed += 1
            continue
        moved = torch.nonzero(out != cur).flatten()
        tgt = out[moved].long()
        cf.index_add_(0, tgt, -cont_t[0][moved])
        mf.index_add_(0, tgt, -cont_t[1][moved])
        cu.index_add_(0, tgt, cont_t[3][moved])  # the bits a move sets were clear on its target: add is or
        cnt.index_add_(0, tgt, torch.ones_like(tgt, dtype=torch.int32))
        sched[n] = 0
        released[n] = True
        cur.copy_(out)
    return cur, released, order.numel(), failed

def _skew(cnt, sched, domain):
    """SPEC.md 2.17's skew on device tensors: max - min of the per-domain sums of ``cnt`` over the domains that
    hold a schedulable node; 0 without one.  Released nodes carry count 0 and are not schedulable."""
    per = torch.zeros(POLICY_DOMAINS, dtype=torch.int64, device=cnt.device).index_add_(0, domain, cnt.long())
    elig = torch.zeros(POLICY_DOMAINS, dtype=torch.bool, device=cnt.device)
    elig[domain[sched != 0]] = True
    if not bool(elig.any()):
        return 0
    vals = per[elig]
    return int((vals.max() - vals.min()).item())


def host_loop_policy(p, cont_t, nodes_t, assign, count, order, sid, domain, dev):
    """Variant `order` under the policy by one single-candidate drain sweep, the bound rule and one commit per
    attempt.  Returns (final assign, released mask, attempts, failed)."""
    C, N = assign.numel(), count.numel()
    cf, mf, lab, cu, sched = (t.clone() for t in nodes_t)
    cur, cnt = assign.clone(), count.clone()
    dom = domain.long()
    out = torch.zeros(C, dtype=torch.int32, device=dev)
    reason = torch.zeros(C, dtype=torch.uint8, device=dev)
    row = torch.zeros(_lib.DRAIN_WORDS, dtype=torch.int32, device=dev)
    group = torch.full((N,), -1, dtype=torch.int32, device=dev)
    released = torch.zeros(N, dtype=torch.bool, device=dev)
    failed = 0
    for n in order.tolist():
        group[n] = 0
        p.dev_drain_sweep_policy(cont_t, (cf, mf, lab, cu, sched), cur, group, 1, out, reason, row, sid, 0, cnt,
                                 domain_t=domain, max_skew=POLICY_MAX_SKEW, relax_mask=POLICY_CHAIN)
        group[n] = -1
        if int(row[_lib.DRAIN_STRANDED].item()):  # the read-back synchronises
            failed += 1
            continue
        moved = torch.nonzero(out != cur).flatten()
        tgt = out[moved].long()
        before = _skew(cnt, sched, dom)
        was, had = int(sched[n].item()), int(cnt[n].item())
        cnt.index_add_(0, tgt, torch.ones_like(tgt, dtype=torch.int32))
        cnt[n], sched[n] = 0, 0
        after = _skew(cnt, sched, dom)
        if not (after <= POLICY_MAX_SKEW or after <= before):  # the bound rule: as if nothing had happened
            cnt.index_add_(0, tgt, -torch.ones_like(tgt, dtype=torch.int32))
            cnt[n], sched[n] = had, was
            failed += 1
            continue
        cf.index_add_(0, tgt, -cont_t[0][moved])
        mf.index_add_(0, tgt, -cont_t[1][moved])
        cu.index_add_(0, tgt, cont_t[3][moved])  # the bits a move sets were clear on its target: add is or
        released[n] = True
        cur.copy_(out)
    return cur, released, order.numel(), failed


def policy_round(a):
    """One process's figures.  --plain-only (also the parent build's process) times leg 1 alone."""
    C, N, sid = a.containers, a.nodes, STRATEGIES["spread_across_pool"]
    dev = torch.device("cuda", 0)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    domain = torch.arange(N, dtype=torch.int32, device=dev) % POLICY_DOMAINS
    rec = {}

    def per_call(p, fn, steps):
        for _ in range(a.warmup):
            fn()
        p.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        p.sync()
        return 1e3 * (time.perf_counter() - t0) / steps

    with Planner(0) as p:
        db = DevBatch.allocate(1, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        count = i32(N)
        p.dev_place_batch_policy_fallback(
            db, torch.full((1,), sid, dtype=torch.int32, device=dev), None, count, domain_t=domain,
            max_skew_t=torch.full((1,), POLICY_MAX_SKEW, dtype=torch.int32, device=dev),
            relax_mask_t=torch.tensor(list(POLICY_CHAIN) + [0, 0], dtype=torch.int32, device=dev),
            n_hops_t=torch.full((1,), len(POLICY_CHAIN), dtype=torch.int32, device=dev))
        p.sync()
        extra = (2 * int(db.cpu.max().item()), 2 * int(db.mem.max().item()))
        cont_t, live = (db.cpu, db.mem, db.req, db.conf), (db.cf + extra[0], db.mf + extra[1], db.lab, db.cu, db.sched)
        rec["running"] = int((db.assign != -1).sum().item())
        gen = torch.Generator(device="cpu").manual_seed(SEED4)
        fewest = torch.sort(count, stable=True).indices.to(torch.int32)
        V = max(POLICY_VARIANTS)
        orders = torch.stack([fewest] + [torch.randperm(N, generator=gen).to(torch.int32).to(dev) for _ in range(V - 1)])
        a_out, state, blk, rows = i32(V * C), torch.zeros(V * N, dtype=torch.uint8, device=dev), i32(V * N), i32(V * _lib.SHRINK_WORDS)
        rec["plain_ms"] = per_call(p, lambda: p.dev_shrink_sweep(cont_t, live, db.assign, orders[0], 1, a_out[:C], state[:N],
                                                                 rows[:_lib.SHRINK_WORDS], sid, 0, count, blk[:N]), a.steps)
        rec["plain_variant_0"] = dict(zip(_lib.SHRINK_FIELDS, (int(x) for x in rows[:_lib.SHRINK_WORDS].cpu().numpy().view("uint32"))))
        if a.plain_only:
            return rec
        hops, why = torch.zeros(V * C, dtype=torch.uint8, device=dev), torch.zeros(V * N, dtype=torch.uint8, device=dev)
        prow = i32(V * _lib.SHRINK_POLICY_WORDS)

        def sweep(v):
            p.dev_shrink_sweep_policy(cont_t, live, db.assign, orders[:v].reshape(-1), v, a_out[:v * C], state[:v * N],
                                      rows[:v * _lib.SHRINK_WORDS], sid, 0, count, blk[:v * N], domain_t=domain,
                                      max_skew=POLICY_MAX_SKEW, relax_mask=POLICY_CHAIN, hops_t=hops[:v * C],
                                      blocker_reason_t=why[:v * N], policy_t=prow[:v * _lib.SHRINK_POLICY_WORDS])

        # ---- the same answer first ----
        sweep(1)
        p.sync()
        row = [int(x) for x in rows[:_lib.SHRINK_WORDS].cpu().numpy().view("uint32")]
        pol = [int(x) for x in prow[:_lib.SHRINK_POLICY_WORDS].cpu().numpy().view("uint32")]
        cur, released, attempts, failed = host_loop_policy(p, cont_t, live, db.assign, count, orders[0], sid, domain, dev)
        p.sync()
        rec["same_plan"] = (bool(torch.equal(cur, a_out[:C]))
                            and bool(torch.equal(released, state[:N] == _lib.SHRINK_STATE_RELEASED))
                            and failed == row[_lib.SHRINK_FAILED])
        rec["variant_0"] = dict(zip(_lib.SHRINK_FIELDS, row))
        rec["variant_0_policy"] = dict(zip(_lib.SHRINK_POLICY_FIELDS, pol))
        for v in POLICY_VARIANTS:
            rec[f"policy_ms_{v}"] = per_call(p, lambda: sweep(v), a.steps)
        p.profile(True)
        for _ in range(a.steps):
            sweep(1)
        p.sync()
        kp, n = p.kernel_stats(_lib.FP_K_PLACE)
        p.profile(False)
        rec["policy_kernel_ms"] = kp / max(n, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_loop_policy(p, cont_t, live, db.assign, count, orders[0], sid, domain, dev)
        p.sync()
        rec["host_loop_ms"], rec["attempts"] = 1e3 * (time.perf_counter() - t0), attempts
    return rec


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
        def parent(r):
            path = os.path.join(tmp, f"parent{r}.json")
            parent_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--plain-only", "--out", path,
                                         "--tree", os.path.abspath(a.parent_tree)], os.path.abspath(a.parent_tree), path))

        def plain(r):
            path = os.path.join(tmp, f"plain{r}.json")
            plain_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--plain-only", "--out", path,
                                        "--tree", ROOT], ROOT, path))

        for r in range(a.rounds):
            # the process that runs first in a round measured up to 1 ms less than the one behind it, whichever
            # build it was: the two take turns
            for leg in ((parent, plain) if r % 2 == 0 else (plain, parent)):
                if leg is plain or a.parent_tree:
                    leg(r)
            path = os.path.join(tmp, f"new{r}.json")
            new_rounds.append(_child([sys.executable, me, *shape, "--policy-child", "--out", path, "--tree", ROOT], ROOT, path))
            print(f"round {r + 1} of {a.rounds} done", file=sys.stderr, flush=True)
    first = new_rounds[0]
    out = {"shape": {"containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4}, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "strategy": "spread_across_pool", "live_state": "roomy",
           "policy": {"domain": f"n % {POLICY_DOMAINS}", "max_skew": POLICY_MAX_SKEW, "relax_mask": [hex(m) for m in POLICY_CHAIN]},
           "order": "each round: the parent build's process and this build's (leg 1), in turns first, then this build's (legs 2 and 3)",
           "acceptance": "leg 1: this build's median over the rounds no higher than the parent's maximum over the rounds",
           "running": first["running"], "same_plan": all(r["same_plan"] for r in new_rounds),
           "plain_variant_0": plain_rounds[0]["plain_variant_0"], "variant_0": first["variant_0"],
           "variant_0_policy": first["variant_0_policy"], "attempts": first["attempts"]}
    mine = [r["plain_ms"] for r in plain_rounds]
    out["plain"] = {"ms_per_call": _stats(mine), "rounds": mine}
    if parent_rounds:
        pr = [r["plain_ms"] for r in parent_rounds]
        out["parent_plain"] = {"ms_per_call": _stats(pr), "rounds": pr, "variant_0": parent_rounds[0]["plain_variant_0"]}
        out["within_parent_range"] = out["plain"]["ms_per_call"]["median"] <= max(pr)
    out["policy"].update({f"variants_{v}": {"ms_per_call": _stats([r[f"policy_ms_{v}"] for r in new_rounds])}
                          for v in POLICY_VARIANTS})
    out["policy"]["sweep_kernel_ms"] = _stats([r["policy_kernel_ms"] for r in new_rounds])
    out["host_loop"] = {"ms_per_variant": _stats([r["host_loop_ms"] for r in new_rounds])}
    one = out["policy"]["variants_1"]["ms_per_call"]["median"]
    out["policy_over_plain"] = one / out["plain"]["ms_per_call"]["median"]
    out["host_loop_over_policy"] = out["host_loop"]["ms_per_variant"]["median"] / one
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--strategy", default="spread_across_pool", choices=sorted(STRATEGIES))
    ap.add_argument("--steps", type=int, default=20, help="timed sweep calls per leg and round (the host loop runs once)")
    ap.add_argument("--warmup", type=int, default=3)
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
        path = a.out or os.path.join(ROOT, "profiles", "shrink_policy_timing.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "shrink_timing.json")
    C, N, sid = a.containers, a.nodes, STRATEGIES[a.strategy]
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"shape": {"containers": C, "nodes": N, "flags": 7, "seed": SEED4}, "strategy": a.strategy, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "device": props.name, "compute_units": props.multi_processor_count,
           "order": "each round: the sweep with 1, 8 and 64 variants, the scan-only call, the host loop (once)"}
    with Planner(0) as p:
        db = DevBatch.allocate(1, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        count = i32(N)
        p.dev_place_batch_policy(db, torch.full((1,), sid, dtype=torch.int32, device=dev), None, count)
        p.sync()
        cont_t, nodes_t = (db.cpu, db.mem, db.req, db.conf), (db.cf, db.mf, db.lab, db.cu, db.sched)
        out["running"] = int((db.assign != -1).sum().item())
        gen = torch.Generator(device="cpu").manual_seed(SEED4)
        fewest = torch.sort(count, stable=True).indices.to(torch.int32)
        orders = torch.stack([fewest] + [torch.randperm(N, generator=gen).to(torch.int32).to(dev)
                                         for _ in range(max(VARIANTS) - 1)])
        bufs = {V: (i32(V * C), torch.zeros(V * N, dtype=torch.uint8, device=dev), i32(V * N), i32(V * _lib.SHRINK_WORDS))
                for V in VARIANTS}
        # the fleet as placed has next to no room; `roomy` is the same plan on servers with room for a few more
        # requests each (twice the largest request added to what every server has left)
        extra = (2 * int(db.cpu.max().item()), 2 * int(db.mem.max().item()))
        states = {"as_placed": nodes_t, "roomy": (db.cf + extra[0], db.mf + extra[1], db.lab, db.cu, db.sched)}
        out["roomy_extra"] = {"cpu_m": extra[0], "mem_mib": extra[1]}

        def timed(fn, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            p.sync()
            return 1e3 * (time.perf_counter() - t0) / steps

        for label, live in states.items():
            cordoned = (*live[:4], torch.zeros_like(db.sched))

            def sweep(V, nodes=live):
                a_out, state, blk, rows = bufs[V]
                p.dev_shrink_sweep(cont_t, nodes, db.assign, orders[:V].reshape(-1), V, a_out, state, rows, sid, 0, count, blk)

            rec = {}
            # ---- the same answer first ----
            sweep(1)
            p.sync()
            a_out, state, _, rows = bufs[1]
            row = [int(x) for x in rows.cpu().numpy().view("uint32")]
            cur, released, attempts, failed = host_loop(p, cont_t, live, db.assign, count, orders[0], sid, dev)
            p.sync()  # this first loop is the comparison and the loop leg's warm-up: not timed
            rec["same_plan"] = (bool(torch.equal(cur, a_out))
                                and bool(torch.equal(released, state == _lib.SHRINK_STATE_RELEASED))
                                and failed == row[_lib.SHRINK_FAILED])
            rec["variant_0"] = dict(zip(_lib.SHRINK_FIELDS, row))
            sweep(1, cordoned)
            p.sync()
            rec["scan_only_attempts_failed"] = int(bufs[1][3][_lib.SHRINK_FAILED].item())
            sweep(max(VARIANTS))
            p.sync()
            rel = bufs[max(VARIANTS)][3].view(-1, _lib.SHRINK_WORDS)[:, _lib.SHRINK_RELEASED]
            rec["released_over_variants"] = {"min": int(rel.min().item()), "max": int(rel.max().item())}

            for _ in range(a.warmup):
                for V in VARIANTS:
                    sweep(V)
            p.sync()
            sw = {V: [] for V in VARIANTS}
            scan, loop = [], []
            for _ in range(a.rounds):
                for V in VARIANTS:
                    sw[V].append(timed(lambda: sweep(V), a.steps))
                scan.append(timed(lambda: sweep(1, cordoned), a.steps))
                loop.append(timed(lambda: host_loop(p, cont_t, live, db.assign, count, orders[0], sid, dev), 1))
            # ---- the kernels' own time, in a pass of its own ----
            kern = {}
            for V in VARIANTS:
                p.profile(True)
                for _ in range(a.steps):
                    sweep(V)
                p.sync()
                kp, n = p.kernel_stats(_lib.FP_K_PLACE)
                ks, _ = p.kernel_stats(_lib.FP_K_SORT)
                p.profile(False)
                kern[V] = {"sweep_kernel_ms": kp / max(n, 1), "ffd_order_ms": ks / max(n, 1)}
            rec["sweep"] = {f"variants_{V}": {"ms_per_call": _stats(sw[V]), **kern[V]} for V in VARIANTS}
            rec["scan_only"] = {"ms_per_call": _stats(scan)}
            rec["host_loop"] = {"ms_per_variant": _stats(loop), "attempts": attempts}
            one = rec["sweep"]["variants_1"]["ms_per_call"]["median"]
            rec["scan_share_of_one_variant"] = rec["scan_only"]["ms_per_call"]["median"] / one
            rec["host_loop_over_sweep"] = rec["host_loop"]["ms_per_variant"]["median"] / one
            out[label] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
