"""Rebalance sweep timing (SPEC.md 2.19) on one config-4 scenario, on cuda:0.

    python tools/rebalance_timing.py [--containers C] [--nodes N] [--steps K] [--warmup W] [--rounds R]

One scenario of C x N (default 50k x 5k, the generator's config-4 inputs) with domain = n % D for D = 8 and 64 is
placed by fp_dev_place_batch_policy_fallback under spread_across_pool, a spread constraint (max_skew 2) and a
fallback chain of two hops WITH ZONE 0 CORDONED; the zone is then uncordoned.  That plan and the node table it leaves
are the live state: every zone but one is full of services, one is empty and schedulable.  On it the tool times

* ``sweep``: fp_dev_rebalance_sweep for 1, 8 and 64 variants that each visit every container once.  Variant 0
  visits them by (cpu asc, mem asc, index) (the `smallest` rule), the others in seeded random orders;
* ``host_loop``: the same answer for variant 0 the way a caller gets it without the sweep: the pass over the order,
  the heavy test and the lift on the host, and per attempt one fp_place_policy_fallback call with C = 1.

Each figure is a host clock around calls that end in a device synchronise, after `warmup` calls of the sweep legs
and one untimed host loop (the comparison: its final plan must be variant 0's, ``same_plan``); a round times the
legs one after the other (1, 8, 64 variants, `steps` calls each, then the host loop once), so the legs alternate,
and the rounds' minimum, median and maximum are kept.  The sweep kernel's own time comes from the context's event
brackets (FP_K_PLACE) in a separate pass.  No target is set: both numbers and their ratio are recorded.

The driver makes no GPU call itself: each domain count is measured by a child process of its own under a time limit
(--child-timeout seconds), and the driver stops at the first child that fails.  Writes
profiles/rebalance_timing.json and prints it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED4 = 0x5EED0004
SPREAD = 1  # spread_across_pool
VARIANTS = (1, 8, 64)
DOMAINS = (8, 64)
MAX_SKEW, CHAIN = 2, (0x780, 0x78)
NONE = 0xFFFFFFFF


def _stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def host_loop(p, cont, live, assign, count, domain, order):
    """Variant `order` by a host pass and one C = 1 fp_place_policy_fallback call per attempt.  Returns (final
    assign, moves, stuck)."""
    import numpy as np
    cpu, mem, req, conf = cont
    cf, mf, lab, cu, sched = (x.copy() for x in live)
    cur, cnt = assign.copy(), count.copy()
    n_dom = int(domain.max()) + 1
    dc = np.bincount(domain, weights=cnt, minlength=n_dom).astype(np.int64)
    elig = np.zeros(n_dom, bool)
    elig[domain[sched != 0]] = True
    moves = stuck = 0
    if not elig.any():
        return cur, 0, 0
    mn = int(dc[elig].min())
    for c in order.tolist():
        s = int(cur[c])
        if s == NONE:
            continue
        d = int(domain[s])
        if not elig[d] or dc[d] - mn <= MAX_SKEW:
            continue
        saved = (cf[s], mf[s], cu[s], cnt[s])
        cf[s] += cpu[c]
        mf[s] += mem[c]
        cu[s] &= ~conf[c]
        cnt[s] -= 1
        a, _, _, after, nc = p.place_policy_fallback((cpu[c:c + 1], mem[c:c + 1], req[c:c + 1], conf[c:c + 1]),
                                                     (cf, mf, lab, cu, sched), SPREAD, CHAIN, 0, None, cnt, domain=domain,
                                                     max_skew=MAX_SKEW, want_hops=False)
        if int(a[0]) == NONE:
            cf[s], mf[s], cu[s], cnt[s] = saved
            stuck += 1
            continue
        t = int(a[0])
        cf, mf, cu, cnt = after[0], after[1], after[3], nc
        cur[c] = t
        dc[d] -= 1
        dc[int(domain[t])] += 1
        mn = int(dc[elig].min())
        moves += 1
        if not (elig & (dc - mn > MAX_SKEW)).any():
            break  # nothing is heavy: no later entry is an attempt
    return cur, moves, stuck


def child(a):
    import numpy as np
    import torch
    from fleetflow_amd import DevBatch, Planner, _lib
    C, N, D = a.containers, a.nodes, a.child
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)  # noqa: E731
    rec = {"domains": D, "device": props.name, "compute_units": props.multi_processor_count}
    with Planner(0) as p:
        db = DevBatch.allocate(1, C, N, dev)
        p.dev_gen_batch(SEED4, db, 7)
        p.sync()
        domain = (torch.arange(N, device=dev) % D).to(torch.int32)
        sched = db.sched.clone()
        db.sched[domain == 0] = 0  # the zone is drained while the plan is made ...
        count = i32(N)
        one = lambda v: torch.full((1,), v, dtype=torch.int32, device=dev)  # noqa: E731
        relax = torch.tensor(list(CHAIN) + [0, 0], dtype=torch.int32, device=dev)
        p.dev_place_batch_policy_fallback(db, one(SPREAD), None, count, domain_t=domain, max_skew_t=one(MAX_SKEW),
                                          relax_mask_t=relax, n_hops_t=one(len(CHAIN)))
        p.sync()
        db.sched.copy_(sched)  # ... and comes back
        cont_t, nodes_t = (db.cpu, db.mem, db.req, db.conf), (db.cf, db.mf, db.lab, db.cu, db.sched)
        rec["running"] = int((db.assign != -1).sum().item())
        gen = torch.Generator(device="cpu").manual_seed(SEED4)
        key = db.cpu.long() * (1 << 32) + db.mem.long()
        smallest = torch.sort(key, stable=True).indices.to(torch.int32)
        orders = torch.stack([smallest] + [torch.randperm(C, generator=gen).to(torch.int32).to(dev)
                                           for _ in range(max(VARIANTS) - 1)])
        bufs = {V: (i32(V * C), u8(V * C), u8(V * C), i32(V * _lib.REBAL_WORDS)) for V in VARIANTS}

        def sweep(V):
            out, hops, why, rows = bufs[V]
            p.dev_rebalance_sweep(cont_t, nodes_t, db.assign, orders[:V].reshape(-1), V, out, rows, SPREAD, 0, count,
                                  domain_t=domain, max_skew=MAX_SKEW, relax_mask=CHAIN, hops_t=hops, reason_t=why)

        def timed(fn, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            p.sync()
            return 1e3 * (time.perf_counter() - t0) / steps

        # ---- the same answer first ----
        sweep(1)
        p.sync()
        row = [int(x) for x in bufs[1][3].cpu().numpy().view("uint32")]
        rec["variant_0"] = dict(zip(_lib.REBAL_FIELDS, row))
        u32 = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)  # noqa: E731
        h_cont = tuple(u32(t) for t in cont_t)
        h_live = tuple(u32(t) for t in nodes_t[:4]) + (nodes_t[4].cpu().numpy(),)
        h_args = (h_cont, h_live, u32(db.assign), u32(count), u32(domain).astype(np.int64), u32(orders[0]))
        cur, moves, stuck = host_loop(p, *h_args)  # the comparison and the loop leg's warm-up: not timed
        rec["same_plan"] = (bool(np.array_equal(cur, u32(bufs[1][0]))) and moves == row[_lib.REBAL_MOVES]
                            and stuck == row[_lib.REBAL_STUCK])
        rec["host_loop_calls"] = moves + stuck
        sweep(max(VARIANTS))
        p.sync()
        mv = bufs[max(VARIANTS)][3].view(-1, _lib.REBAL_WORDS)
        rec["moves_over_variants"] = {"min": int(mv[:, _lib.REBAL_MOVES].min().item()),
                                      "max": int(mv[:, _lib.REBAL_MOVES].max().item())}
        rec["skew_after_over_variants"] = {"min": int(mv[:, _lib.REBAL_SKEW_AFTER].min().item()),
                                           "max": int(mv[:, _lib.REBAL_SKEW_AFTER].max().item())}
        for _ in range(a.warmup):
            for V in VARIANTS:
                sweep(V)
        p.sync()
        sw, loop = {V: [] for V in VARIANTS}, []
        for _ in range(a.rounds):
            for V in VARIANTS:
                sw[V].append(timed(lambda: sweep(V), a.steps))
            loop.append(timed(lambda: host_loop(p, *h_args), 1))
        kern = {}
        for V in VARIANTS:  # the kernel's own time, in a pass of its own
            p.profile(True)
            for _ in range(a.steps):
                sweep(V)
            p.sync()
            kp, n = p.kernel_stats(_lib.FP_K_PLACE)
            p.profile(False)
            kern[V] = {"sweep_kernel_ms": kp / max(n, 1)}
        rec["sweep"] = {f"variants_{V}": {"ms_per_call": _stats(sw[V]), **kern[V]} for V in VARIANTS}
        rec["host_loop"] = {"ms_per_variant": _stats(loop)}
        rec["host_loop_over_sweep"] = (rec["host_loop"]["ms_per_variant"]["median"]
                                       / rec["sweep"]["variants_1"]["ms_per_call"]["median"])
    print("RESULT " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=10, help="timed sweep calls per leg and round (the host loop runs once)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebalance_timing.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"shape": {"containers": a.containers, "nodes": a.nodes, "flags": 7, "seed": SEED4},
           "strategy": "spread_across_pool", "max_skew": MAX_SKEW, "relax_mask": list(CHAIN), "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds,
           "order": "each round: the sweep with 1, 8 and 64 variants, then the host loop (once)"}
    for D in DOMAINS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(D), "--containers", str(a.containers), "--nodes",
               str(a.nodes), "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode != 0:  # nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"rebalance_timing: the child for {D} domains ended with status {r.returncode}")
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        out[f"domains_{D}"] = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
