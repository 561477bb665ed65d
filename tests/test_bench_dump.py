"""bench.py --dump-outputs DIR and --full.

A plain run times the headline workload only and, with --dump-outputs, writes what its last timed
step handed back (winner, winner's plan, every packed cost, a seeded sample of the per-scenario
plans) as float32 / float64 .npy files that hold the integers exactly.  The host test drives
dump_outputs with CPU tensors; the GPU test runs the benchmark itself on 6 scenarios and checks
every file against the C oracle."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"best", "plan_assign", "plan_reason", "cost_rejected", "cost_nodes_used", "cost_scenario",
         "sample_index", "assign_sample", "reason_sample"}
FULL_KEYS = {"config1", "config2", "config3", "config5", "stage2", "cpu_baseline", "cpu_single_thread"}


def _load(path):
    files = sorted(os.listdir(path))
    assert {f[:-4] for f in files} == NAMES and all(f.endswith(".npy") for f in files)
    out = {f[:-4]: np.load(os.path.join(path, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_options_default_to_a_plain_run(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("S,C", [(3, 1000), (30, 50_000)])  # every position kept / a sample of 1.5M
def test_dump_outputs_holds_the_integers_exactly(S, C, tmp_path):
    import torch

    import bench
    from fleetflow_amd import shard
    g = torch.Generator().manual_seed(S)
    assign = torch.randint(-1, 5000, (S * C,), dtype=torch.int32, generator=g)  # -1 = FP_NONE
    reason = torch.randint(0, 3, (S * C,), dtype=torch.uint8, generator=g)
    cost = torch.randint(-2**63, 2**63 - 1, (S,), dtype=torch.int64, generator=g)
    cost[1] = shard.PAD
    plan = torch.empty(shard.plan_words(C), dtype=torch.int32)
    shard.pack_plan(assign[2 * C:3 * C], reason[2 * C:3 * C], plan)
    db = types.SimpleNamespace(assign=assign, reason=reason)
    for _ in range(2):  # a second dump into the same directory writes the same files
        bench.dump_outputs(str(tmp_path / "d"), {"best": 2, "costs": cost}, plan, db, C)
    d = _load(str(tmp_path / "d"))
    a_u32 = assign.numpy().view(np.uint32)
    idx = d["sample_index"].astype(np.int64)
    assert idx.size == min(S * C, bench.DUMP_SAMPLE) and np.all(np.diff(idx) > 0) and idx[-1] < S * C
    assert np.array_equal(d["assign_sample"], a_u32[idx]) and np.array_equal(d["reason_sample"], reason.numpy()[idx])
    assert d["best"].tolist() == [2.0]
    assert np.array_equal(d["plan_assign"], a_u32[2 * C:3 * C])
    assert np.array_equal(d["plan_reason"], reason.numpy()[2 * C:3 * C])
    for s in range(S):
        got = tuple(int(d[k][s]) for k in ("cost_rejected", "cost_nodes_used", "cost_scenario"))
        assert got == shard.unpack_cost(int(cost[s]))


@pytest.mark.gpu
def test_plain_run_dumps_the_oracles_plans(O, tmp_path):
    """The benchmark itself (a child process) on 6 config-4 scenarios: --steps sets the timed steps,
    the plain result line carries no --full leg, and every dumped array is the oracle's."""
    import bench
    S, C, N = 6, bench.C4, bench.N4
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup",
                          "1", "--scenarios", str(S), "--dump-outputs", str(tmp_path / "d")],
                         env=env, capture_output=True, text=True, timeout=120, check=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"] == "u32"
    assert rec["value"] == pytest.approx(S * C * N / (rec["ms_per_step"] / 1e3)) and rec["higher_is_better"] is True
    assert not FULL_KEYS & set(rec)
    d = _load(str(tmp_path / "d"))
    plans = []
    for s in range(S):
        cont, nodes = O.gen_scenario(bench.SEED4, s, C, N, bench.FLAGS)
        ea, er, _, _ = O.place(cont, nodes)
        plans.append((ea, er, O.cost(ea, N, s)))
    from fleetflow_amd import shard
    for s, (_, _, c) in enumerate(plans):
        got = tuple(int(d[k][s]) for k in ("cost_rejected", "cost_nodes_used", "cost_scenario"))
        assert got == shard.unpack_cost(int(c)), s
    best = int(np.argmin(np.array([p[2] for p in plans], np.uint64)))
    assert d["best"].tolist() == [float(best)] and rec["best_scenario"] == best
    assert np.array_equal(d["plan_assign"], plans[best][0]) and np.array_equal(d["plan_reason"], plans[best][1])
    idx = d["sample_index"].astype(np.int64)
    assert idx.size == S * C  # fewer than DUMP_SAMPLE entries: all of them
    assert np.array_equal(d["assign_sample"], np.concatenate([p[0] for p in plans])[idx])
    assert np.array_equal(d["reason_sample"], np.concatenate([p[1] for p in plans])[idx])
