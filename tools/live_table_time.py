"""Timing of a placement on a live node table: config 4's shape (S x 50k x 5k), one batch placed on
the generated nodes, then a second generated batch of containers placed on the state the first one
left (nothing restored).  Prints the FFD kernel's and the step's time of the second placement.

    [FLEETPLACE_LIB=...] python tools/live_table_time.py [S [reps]]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fleetflow_amd import DevBatch, Planner, _lib  # noqa: E402


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    C, N = 50_000, 5_000
    p = Planner(0)
    db = DevBatch.allocate(S, C, N, "cuda:0")
    p.dev_gen_batch(0x5EED0004, db, 7)
    p.dev_place_batch(db)
    p.sync()
    live = db.node_snapshot()             # the table the first batch left
    lab, sched = db.lab.clone(), db.sched.clone()
    placed1 = int((db.assign != -1).sum())
    p.dev_gen_batch(0x5EED0014, db, 7)    # the second batch's containers; its nodes are the first batch's again
    p.sync()
    db.lab.copy_(lab)
    db.sched.copy_(sched)
    torch.cuda.synchronize()
    p.profile(True)
    steps = []
    for _ in range(reps + 1):
        db.restore_nodes(live)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.dev_place_batch(db)
        p.sync()
        steps.append((time.perf_counter() - t0) * 1e3)
    ms, n = p.kernel_stats(_lib.FP_K_PLACE)
    path = p.place_path()
    placed2 = int((db.assign != -1).sum())
    print(f"S={S} C={C} N={N} lib={os.path.basename(_lib.LIB_PATH)}: first batch placed {placed1}, second batch on the "
          f"live table placed {placed2}, packed={path['packed']}; ffd kernel avg {ms / n:.3f} ms over {n} launches, step "
          f"min {min(steps[1:]):.3f} ms")


if __name__ == "__main__":
    main()
