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

    python tools/grow_timing.py --policy [--steps K] [--warmup W] [--rounds R]

The sweep under the policy (SPEC.md 2.18), written to profiles/grow_policy_timing.json.  For a live table of 1000
and of 5000 nodes (ten containers a node, eight topology domains) the scenario is placed by
fp_dev_place_batch_policy_quota under spread, max_skew 1 and a chain over class and region; its NOFIT and SKEW
containers are the pending.  The same catalogues are timed, each with max_new = 64, 1024 and the most the
placer's table leaves beside the live nodes, the templates standing in the eight live domains and a ninth:

* ``sweep``: fp_dev_grow_sweep_policy with the policy rows and without the per-container results, and
* ``route``: the only way to the same answers without it: materialise one combined table per candidate on the
  device (``build``), call fp_dev_place_batch_policy_quota with S = n_cand (``call``), and reduce its outputs to
  the counters of the rows (``rows``; FIRST_UNPLACED and the two skew words are left out, so the pass is cheaper
  than a complete one).

``same_counts`` compares PLACED, OPENED, ON_LIVE, RELAXED, STUCK_SKEW and STUCK_QUOTA of every candidate.
``sweep_faster`` says that the sweep's median is below the route's median (build + call + rows) by more than the
two spreads (max - min) together; ``sweep_faster_than_call`` says the same against the call alone.
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


RELAX = (0x780, 0x78)  # the generator's class bits, then its region bits
N_DOM = 8


def policy_leg(a):
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    out = {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": props.name,
           "compute_units": props.multi_processor_count, "policy": {"strategy": 1, "max_skew": 1, "relax_mask": list(RELAX),
                                                                    "domains": N_DOM, "quota": [None, None, 2 ** 30]},
           "order": "each round: the sweep, then the route", "points": []}
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    tens = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731
    quota, mask = (None, None, 2 ** 30), (1 << _lib.REASON_NOFIT) | (1 << _lib.REASON_SKEW)
    with Planner(0) as p:
        for N in (1000, 5000):
            C = 10 * N
            db = DevBatch.allocate(1, C, N, dev)
            p.dev_gen_batch(SEED4, db, 7)
            count, domain = i32(N), (torch.arange(N, device=dev) % N_DOM).to(torch.int32)
            p.dev_place_batch_policy_quota(db, tens([1]), None, None, None, count, domain_t=domain, max_skew_t=tens([1]),
                                           relax_mask_t=tens(list(RELAX) + [0, 0]), n_hops_t=tens([2]))
            p.sync()
            cont_t, nodes_t = (db.cpu, db.mem, db.req, db.conf), (db.cf, db.mf, db.lab, db.cu, db.sched)
            pend = torch.nonzero((db.reason == _lib.REASON_NOFIT) | (db.reason == _lib.REASON_SKEW)).flatten()
            pend_t = tuple(t[pend].contiguous() for t in cont_t)
            P = int(pend.numel())
            for n_cand, max_new in itertools.product(N_CAND, (64, 1024, _lib.FP_POLICY_MAX_NODES - N)):
                S, T = n_cand, N + max_new
                tpl = catalogue(n_cand, dev)
                t_dom = (torch.arange(n_cand, device=dev) % (N_DOM + 1)).to(torch.int32)
                rows, prow = i32(S * _lib.GROW_WORDS), i32(S * _lib.GROW_POLICY_WORDS)
                st, ms, nh = tens([1] * S), tens([1] * S), tens([2] * S)
                rm, qt = tens((list(RELAX) + [0, 0]) * S), tens([-1, -1, 2 ** 30] * S)

                def sweep():
                    p.dev_grow_sweep_policy(cont_t, db.reason, nodes_t, tpl, max_new, rows, mask, None, 1, 0, count,
                                            domain_t=domain, t_domain_t=t_dom, max_skew=1, relax_mask=RELAX, quota=quota,
                                            quota_used=(0, 0, 0), policy_t=prow)

                def route():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    b = DevBatch.allocate(S, P, T, dev)
                    for dst, src in zip((b.cpu, b.mem, b.req, b.conf), pend_t):
                        dst.view(S, P).copy_(src.view(1, P).expand(S, P))
                    for dst, src, new in zip((b.cf, b.mf, b.lab, b.cu), nodes_t, (*tpl, None)):
                        dst.view(S, T)[:, :N] = src.view(1, N)
                        dst.view(S, T)[:, N:] = new.view(S, 1) if new is not None else 0
                    b.sched.view(S, T)[:, :N] = db.sched.view(1, N)
                    b.sched.view(S, T)[:, N:] = 1
                    cnt, dom, used, hops = i32(S * T), i32(S * T), i32(S * 3), torch.zeros(S * P, dtype=torch.uint8, device=dev)
                    cnt.view(S, T)[:, :N] = count.view(1, N)
                    dom.view(S, T)[:, :N] = domain.view(1, N)
                    dom.view(S, T)[:, N:] = t_dom.view(S, 1)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    p.dev_place_batch_policy_quota(b, st, qt, used, None, cnt, domain_t=dom, max_skew_t=ms, relax_mask_t=rm,
                                                   n_hops_t=nh, hops_t=hops)
                    p.sync()
                    t2 = time.perf_counter()
                    asg, rs, new_cnt = b.assign.view(S, P), b.reason.view(S, P), cnt.view(S, T)[:, N:]
                    got = {"placed": (asg != -1).sum(1), "opened": (new_cnt > 0).sum(1),
                           "on_live": ((asg != -1) & (asg < N)).sum(1), "relaxed": (hops.view(S, P) > 0).sum(1),
                           "stuck_skew": (rs == _lib.REASON_SKEW).sum(1), "stuck_quota": (rs == _lib.REASON_QUOTA).sum(1),
                           "left_cpu": (b.cf.view(S, T)[:, N:] * (new_cnt > 0)).sum(1),
                           "left_mem": (b.mf.view(S, T)[:, N:] * (new_cnt > 0)).sum(1)}
                    keep = pend_t[2].view(1, P) & ~(RELAX[0] | RELAX[1])
                    never = ((pend_t[0].view(1, P) > tpl[0].view(S, 1)) | (pend_t[1].view(1, P) > tpl[1].view(S, 1))
                             | ((tpl[2].view(S, 1) & keep) != keep))
                    got["unplaceable"] = ((rs == _lib.REASON_NOFIT) & never).sum(1)
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    return (t1 - t0, t2 - t1, t3 - t2), got

                # ---- the same answer first ----
                sweep()
                p.sync()
                _, got = route()
                sm, pw = rows.view(S, _lib.GROW_WORDS), prow.view(S, _lib.GROW_POLICY_WORDS)
                pairs = ((got["placed"], sm[:, _lib.GROW_PLACED]), (got["opened"], sm[:, _lib.GROW_OPENED]),
                         (got["unplaceable"], sm[:, _lib.GROW_UNPLACEABLE]), (got["on_live"], pw[:, _lib.GROW_ON_LIVE]),
                         (got["relaxed"], pw[:, _lib.GROW_RELAXED]), (got["stuck_skew"], pw[:, _lib.GROW_STUCK_SKEW]),
                         (got["stuck_quota"], pw[:, _lib.GROW_STUCK_QUOTA]))
                g = {"live_nodes": N, "containers": C, "pending": P, "n_cand": n_cand, "max_new": max_new,
                     "placed": int(sm[:, _lib.GROW_PLACED].sum().item()), "opened": int(sm[:, _lib.GROW_OPENED].sum().item()),
                     "on_live": int(pw[:, _lib.GROW_ON_LIVE].sum().item()),
                     "stuck_skew": int(pw[:, _lib.GROW_STUCK_SKEW].sum().item()),
                     "same_counts": all(bool(torch.equal(x.to(torch.int32), y)) for x, y in pairs)}
                del got
                for _ in range(a.warmup):
                    sweep()
                    route()
                p.sync()
                sw, parts = [], [[], [], []]
                for _ in range(a.rounds):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        sweep()
                    p.sync()
                    sw.append(1e3 * (time.perf_counter() - t0) / a.steps)
                    acc = [0.0, 0.0, 0.0]
                    for _ in range(a.steps):
                        dt, _ = route()
                        acc = [x + y for x, y in zip(acc, dt)]
                    for xs, x in zip(parts, acc):
                        xs.append(1e3 * x / a.steps)
                total = [x + y + z for x, y, z in zip(*parts)]
                spread = lambda xs: max(xs) - min(xs)  # noqa: E731
                g["sweep"] = {"ms_per_call": _stats(sw)}
                g["route"] = {"build_ms": _stats(parts[0]), "call_ms": _stats(parts[1]), "rows_ms": _stats(parts[2]),
                              "total_ms": _stats(total)}
                g["route_over_sweep"] = statistics.median(total) / statistics.median(sw)
                g["call_over_sweep"] = statistics.median(parts[1]) / statistics.median(sw)
                g["sweep_faster"] = statistics.median(total) - statistics.median(sw) > spread(sw) + spread(total)
                g["sweep_faster_than_call"] = (statistics.median(parts[1]) - statistics.median(sw)
                                               > spread(sw) + spread(parts[1]))
                out["points"].append(g)
                print(json.dumps(g), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", action="store_true", help="time the sweep under the policy (SPEC.md 2.18)")
    ap.add_argument("--containers", type=int, default=50_000)
    ap.add_argument("--nodes", type=int, default=5_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "grow_policy_timing.json" if a.policy else "grow_timing.json")
    if a.policy:
        return policy_leg(a)
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
