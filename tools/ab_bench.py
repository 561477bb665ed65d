#!/usr/bin/env python3
"""A/B of library builds on the headline benchmark, alternating, every run kept:

    tools/ab_bench.py <out.jsonl> <reps> <suffix> [<suffix> ...]     ("-" = the default build)

Each round runs `bench.py --steps 20 --warmup 5` once per build, in the order given (fresh processes,
FLEETPLACE_LIB = fleetflow_amd/libfleetplace<suffix>.so), <reps> rounds.  One line per run goes to
<out.jsonl>: {"lib", "rep", "ffd_kernel", "ms_per_step", "breakdown_ms"}; the summary at the end
gives each build's range and applies the rule of DESIGN.md 7 against the first build (a build wins
when its slowest run beats the first build's fastest, in ffd_kernel and in ms_per_step).  A run that
fails or exceeds its time limit ends the A/B at once."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out, reps, libs = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    rows = []
    with open(out, "w") as fo:
        for rep in range(reps):
            for v in libs:
                suffix = "" if v == "-" else v
                env = dict(os.environ, FLEETPLACE_LIB=os.path.join(ROOT, "fleetflow_amd", f"libfleetplace{suffix}.so"))
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
                                    "--warmup", "5"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   text=True, timeout=180)
                if r.returncode:
                    print(f"lib{suffix} rep {rep}: exit {r.returncode}\n{r.stderr[-2000:]}")
                    return 1
                d = json.loads(r.stdout.strip().splitlines()[-1])
                row = {"lib": v, "rep": rep, "ffd_kernel": d["breakdown_ms"]["ffd_kernel"],
                       "ms_per_step": d["ms_per_step"], "breakdown_ms": d["breakdown_ms"]}
                rows.append(row)
                fo.write(json.dumps(row) + "\n")
                fo.flush()
                print(f"lib{suffix} rep {rep}: ffd {row['ffd_kernel']:.3f} step {row['ms_per_step']:.3f}", flush=True)
    rng = {v: {k: (min(r[k] for r in rows if r["lib"] == v), max(r[k] for r in rows if r["lib"] == v))
               for k in ("ffd_kernel", "ms_per_step")} for v in libs}
    base = rng[libs[0]]
    for v in libs:
        wins = all(rng[v][k][1] < base[k][0] for k in base)
        print(f"{v:10s} ffd {rng[v]['ffd_kernel'][0]:.3f}-{rng[v]['ffd_kernel'][1]:.3f}  step "
              f"{rng[v]['ms_per_step'][0]:.3f}-{rng[v]['ms_per_step'][1]:.3f}"
              + ("" if v == libs[0] else "  beats the first build" if wins else "  does not beat the first build"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
