"""tools/bigp_replay.py, the CPU replay of the no-mask packed FFD kernel's walk: on random batches of the shape
tests/test_gpu_bigp_retest.py uses (C = 320, N = 2200: three 12-group segments, 8 scenarios each) the replay's
plan is the oracle's, the per-segment counters are consistent, and the capacity-only re-test gives the same
plan with at least as many checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bigp_replay as R  # noqa: E402

NONE = 0xFFFFFFFF
S, C, N = 8, 320, 2200
ABSENT = 1 << 30


def _random(seed, big_p, zero_p=0.0, cycle_p=0.0, absent_p=0.0):
    """tests/test_gpu_bigp_lazy_walk.py's random batch, S scenarios."""
    rng = np.random.default_rng(seed)
    cpu = (2 * rng.integers(1, 40, (S, C))).astype(np.uint32)
    mem = (64 * rng.integers(1, 24, (S, C))).astype(np.uint32)
    req = np.where(rng.random((S, C)) < 0.3, 1 << rng.integers(0, 4, (S, C)), 0).astype(np.uint32)
    conf = np.where(rng.random((S, C)) < 0.1, 1 << rng.integers(0, 32, (S, C)), 0).astype(np.uint32)
    req = np.where(rng.random((S, C)) < absent_p, req | ABSENT, req).astype(np.uint32)
    zero = rng.random((S, C)) < zero_p
    for a in (cpu, mem, req, conf):
        a[zero] = 0
    level = np.where(rng.random((S, C)) < cycle_p, NONE, 0).astype(np.uint32)
    big = rng.random((S, N)) < big_p
    cf = np.where(big, 2 * rng.integers(20, 60, (S, N)), 2).astype(np.uint32)
    mf = np.where(big, 64 * rng.integers(12, 40, (S, N)), 64).astype(np.uint32)
    lab = rng.integers(0, 16, (S, N)).astype(np.uint32)
    cu = np.where(rng.random((S, N)) < 0.05, 1 << rng.integers(0, 32, (S, N)), 0).astype(np.uint32)
    sched = (rng.random((S, N)) >= 0.05).astype(np.uint8)
    return [cpu, mem, req, conf], [cf, mf, lab, cu, sched], level


@pytest.mark.parametrize("seed, kw", [(21, dict(big_p=0.05)),
                                      (22, dict(big_p=0.12, zero_p=0.05, cycle_p=0.03, absent_p=0.1))])
def test_replay_gives_the_oracles_plan_and_consistent_counters(O, seed, kw):
    cont, nodes, level = _random(seed, **kw)
    active = passes = 0
    for s in range(S):
        c, n, lv = [a[s] for a in cont], [a[s] for a in nodes], level[s]
        want, reason, _, _ = O.place(c, n, level=lv)
        assign, tot, seg = R.replay(c, n, lv)
        assert np.array_equal(assign, want), f"scenario {s}: the replay's plan differs from the oracle's"
        assert len(seg) == 3
        # what enters segment 0: every container but CYCLE members and screened ones
        entered = C - int((lv == NONE).sum()) - int(((c[2] & ABSENT) != 0)[lv != NONE].sum())
        assert seg[0]["visits"] == entered and seg[0]["batches"] == C // 64
        for b in range(3):
            st = seg[b]
            assert st["checks"] == st["hits"] + st["misses"]
            assert st["pass_through"] <= st["batches"] and st["plain_checks"] <= st["checks"]
            assert st["nodes"] == int((st["node_hist"] * np.arange(st["node_hist"].size)).sum())
            assert st["passes"] == int(st["node_hist"].sum()) and st["empty_passes"] == int(st["node_hist"][0])
            if b + 1 < 3:
                # all-zero containers are placed without a check: they leave the stream in the first segment
                # that has a schedulable node, which is segment 0 here
                zeros = int((((c[0] | c[1] | c[2] | c[3]) == 0) & (lv != NONE)).sum()) if b == 0 else 0
                assert seg[b + 1]["visits"] == st["visits"] - st["hits"] - zeros
                assert seg[b + 1]["batches"] == -(-seg[b + 1]["visits"] // 64)
        assert tot["hits"] + int((((c[0] | c[1] | c[2] | c[3]) == 0) & (lv != NONE)).sum()) == int((want != NONE).sum())
        assert seg[2]["visits"] - seg[2]["hits"] == int((reason == 1).sum()) - (C - entered - int((lv == NONE).sum()))
        # the capacity-only re-test: the same plan, and no fewer checks (it drops a subset of the lanes)
        assign_c, tot_c, _ = R.replay(c, n, lv, capacity_only=True)
        assert np.array_equal(assign_c, want)
        assert tot_c["checks"] >= tot["checks"] and tot_c["nodes"] >= 0
        # an uncapped re-test never takes the big-corner exit
        assign_u, tot_u, _ = R.replay(c, n, lv, refilter_max=64)
        assert np.array_equal(assign_u, want) and tot_u["big_exits"] == 0
        active += tot["active_pairs"]
        passes += tot["passes"]
    assert active > 0 and passes > 0, "the batches exercise the walk and the re-test"
