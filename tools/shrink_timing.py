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
STRATEGIES = {"first_fit_scored": 0, "spread_across_pool": 1, "pack_into_dedicated": 2, "fill_lowest": 3}
VARIANTS = (1, 8, 64)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--strategy", default="spread_across_pool", choices=sorted(STRATEGIES))
    ap.add_argument("--steps", type=int, default=20, help="timed sweep calls per leg and round (the host loop runs once)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink_timing.json"))
    a = ap.parse_args()
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
