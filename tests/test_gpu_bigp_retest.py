"""GPU parity of the re-test after a first miss in the lazy walk of the packed 4096-scenario FFD kernel
(fp_pipe_pk.h: bigp / bigpw with FPP_BIGP_RETEST).  After a queue's first miss the nodes of the batch corner
(at most 16) are walked once: per node the test word z = ((nw - cw) & G) | (req & ~labels) | (conf & used)
goes into an unsigned minimum per lane, and the lanes whose minimum is 0 stay queued.

Shape and method are tests/test_gpu_bigp_lazy_walk.py's: 4096 scenarios so that this kernel runs (asserted
through place_path), three 12-group segments, the even scenarios designed and the odd ones random, all 4096
costs, every assign / reason entry and the node tables afterwards compared with the C oracle, and each case
asserted from the oracle's plan and from the CPU replay (tools/bigp_replay.py) before the GPU is asked.

A designed scenario (that file's): cpu demands 1000 - 2 i, so FFD position = index and segment 0's batch 0
is containers 0 .. 63 (cpu 1000 .. 874, its corner (874, 64)); every demand has mem = 64, and every node is
tiny (cpu 2) unless the case places one.  The gadgets here use "B" nodes (cpu 990, mem 64): too small for
containers 0 .. 4, so a group of B nodes starts with container 0's miss, and each takes exactly one of the
containers from 5 on and then leaves the corner.  The big nodes (cpu 1000) that take what is left sit in a
later group."""
import os
import sys

import numpy as np
import pytest

import test_gpu_bigp_lazy_walk as LW

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bigp_replay as R  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, S, SEG, CPU0, LABEL = LW.NONE, LW.S, LW.SEG, LW.CPU0, LW.LABEL
CONFBIT = 1 << 7
B_CPU = 990           # a B node: takes one of the containers 5 .. 63 of batch 0, none of 0 .. 4


def _base(seed, C, N, big_p=0.05, **kw):
    """Random odd scenarios, and the even ones designed with nothing but tiny nodes."""
    cont, nodes, level = LW._random(seed, C, N, big_p, **kw)
    rows, _ = LW._design(seed * 10 + 1, cont, nodes, C, N, {})
    return cont, nodes, level, rows


def _lanes(rng, R_, k, lo=0, hi=64):
    """Per designed scenario k distinct lanes of lo .. hi - 1, ascending: (R_, k)."""
    return np.sort(np.argsort(rng.random((R_, hi - lo)), axis=1)[:, :k], axis=1) + lo


def _put(nodes, rows, n, cf, lab=None, cu=None):
    """Sets node n[r] (per designed scenario, or one index for all) of every designed scenario: cpu cf, mem 64,
    schedulable."""
    idx = (rows, n)
    nodes[0][idx] = cf
    nodes[1][idx] = 64
    nodes[4][idx] = 1
    if lab is not None:
        nodes[2][idx] = lab
    if cu is not None:
        nodes[3][idx] = cu


def _fill(nodes, rows, first, n=64, lab=None):
    """Group at node `first`: n big nodes (cpu 1000) on its first lanes."""
    for l in range(n):
        _put(nodes, rows, first + l, CPU0, lab=lab)


def _run(planner, O, C, N, cont, nodes, level, base, what, pre=None, packed=True):
    """LW._run, and the kernel by name: the prepacked-input form of the packed kernel (place_path 3), or the
    u32 twin behind the repair pass (4) for values that do not pack."""
    out = LW._run(planner, O, C, N, cont, nodes, level, base, what, pre, packed)
    path = planner.place_path()
    assert path["prepacked" if packed else "repaired"], path
    return out


def _replay(cont, nodes, level, rows, k=3):
    """The replay's counters of the first k designed scenarios (their plans are asserted against the oracle's)."""
    out = []
    for s in rows[:k]:
        c, n = [a[s] for a in cont], [a[s] for a in nodes]
        out.append(R.replay_checked(c, n, level[s])[1:])
    return out


def test_unsigned_minimum(planner, O):
    """Group 2 of segment 0 holds two corner nodes, A (cpu 880) on a lower lane than B (cpu 990).  After
    container 0's miss the re-test walks both: for container 5 (cpu 990) A's test word has bit 31 alone (a cpu
    borrow; mem fits) and B's is 0.  The minimum must be unsigned: container 5 lands on B in this group, not
    in group 7's big nodes, and container 60 (cpu 880) on A after the second pass."""
    C, N = 320, 2200
    cont, nodes, level, rows = _base(31, C, N)
    rng = np.random.default_rng(3131)
    ab = _lanes(rng, rows.size, 2) + 2 * 64
    _put(nodes, rows, ab[:, 0], 880)
    _put(nodes, rows, ab[:, 1], B_CPU)
    _fill(nodes, rows, 7 * 64)
    _fill(nodes, rows, SEG + 3 * 64, 40)

    def pre(e_assign, _after):
        assert (ab[:, 0] < ab[:, 1]).all()
        assert (e_assign[rows, 5] == ab[:, 1]).all(), "container 5 on B"
        assert (e_assign[rows, 60] == ab[:, 0]).all(), "container 60 on A"
        others = np.delete(e_assign[rows, :64], [5, 60], axis=1)
        assert ((others >= 7 * 64) & (others < 8 * 64)).all(), "the rest of batch 0 in group 7"
        for tot, seg in _replay(cont, nodes, level, rows):
            assert tot["max_pair_passes"] >= 3 and seg[0]["node_hist"][2] >= 1

    _run(planner, O, C, N, cont, nodes, level, 2, "unsigned minimum", pre)


def test_corner_sizes_0_1_16_17(planner, O):
    """At container 0's miss group 1 holds 17 B nodes (one above the cap: the plain loop), group 3 holds 16 (the
    cap: a pass, then the group fills up exactly and the next pass finds an empty corner) and group 5 one."""
    C, N = 256, 2234
    cont, nodes, level, rows = _base(32, C, N)
    rng = np.random.default_rng(3232)
    for g, k in ((1, 17), (3, 16), (5, 1)):
        ln = _lanes(rng, rows.size, k) + g * 64
        for j in range(k):
            _put(nodes, rows, ln[:, j], B_CPU)
    _fill(nodes, rows, 9 * 64)
    _fill(nodes, rows, SEG + 64, 64)
    _fill(nodes, rows, 2 * SEG + 128, 30)

    def pre(e_assign, _after):
        a0 = e_assign[rows, :64]
        g = np.where(a0 != NONE, a0 // 64, -1)
        assert (g[:, 5:22] == 1).all() and (g[:, 22:38] == 3).all() and (g[:, 38] == 5).all()
        assert (g[:, :5] == 9).all() and (g[:, 39:] == 9).all()
        for tot, seg in _replay(cont, nodes, level, rows):
            h = seg[0]["node_hist"]
            assert seg[0]["big_exits"] >= 1 and h[16] >= 1 and h[1] >= 1 and h[0] >= 2

    _run(planner, O, C, N, cont, nodes, level, 4, "corner sizes", pre)


def test_label_only_and_conflict_only_rejections(planner, O):
    """Every container requires LABEL and carries CONFBIT.  Group 2 holds L (cpu 990, no LABEL) and
    X (cpu 990, LABEL, CONFBIT used): both fit every queued container from 5 on by capacity and reject it in the
    re-test, by the label alone and by the conflict alone.  In every other designed scenario a node F (LABEL, no
    conflict) sits on a higher lane of the group and takes container 5; in the rest the first fitting node is
    in group 8.  L and X are untouched afterwards."""
    C, N = 192, 2150
    cont, nodes, level, rows = _base(33, C, N)
    rng = np.random.default_rng(3333)
    cont[2][rows] = LABEL                                    # (every batch: L and X never take a container)
    cont[3][rows] = CONFBIT
    nodes[2][rows] &= ~np.uint32(LABEL)
    lxf = _lanes(rng, rows.size, 3) + 2 * 64
    _put(nodes, rows, lxf[:, 0], B_CPU, lab=3, cu=0)
    _put(nodes, rows, lxf[:, 1], B_CPU, lab=LABEL | 1, cu=CONFBIT)
    same = np.arange(rows.size) % 2 == 0                     # F in the same group
    _put(nodes, rows[same], lxf[same, 2], B_CPU, lab=LABEL, cu=0)
    _fill(nodes, rows, 8 * 64, lab=LABEL | 2)
    _fill(nodes, rows, SEG + 5 * 64, 64, lab=LABEL)

    def pre(e_assign, e_after):
        a0 = e_assign[rows, :64]
        assert (a0[same, 5] == lxf[same, 2]).all(), "container 5 on F"
        assert (a0[~same, 5] // 64 == 8).all(), "container 5 in group 8"
        assert ((np.delete(a0, 5, axis=1) // 64) == 8).all()
        cf_after, cu_after = e_after[0].reshape(S, N), e_after[3].reshape(S, N)
        for j, cu in ((0, 0), (1, CONFBIT)):
            assert (cf_after[rows, lxf[:, j]] == B_CPU).all() and (cu_after[rows, lxf[:, j]] == cu).all()
        for s, (tot, seg) in zip(rows, _replay(cont, nodes, level, rows, 4)):
            c, n = [a[s] for a in cont], [a[s] for a in nodes]
            cap = R.replay(c, n, level[s], capacity_only=True)[1]
            assert seg[0]["passes"] >= 1 and cap["checks"] > tot["checks"], "the labels and conflicts drop lanes"

    _run(planner, O, C, N, cont, nodes, level, 6, "label-only / conflict-only rejections", pre)


STAIRS = (990, 970, 950, 930, 910, 890)


STAIRS_1 = (868, 848, 828, 808, 788)   # below batch 0's demands: for the batch segment 1 is fed


def _stairs(nodes, rows, rng, groups, steps=STAIRS):
    """A staircase per group: one node of each cpu in `steps` on random lanes.  A queue whose first container
    is above the top step misses after every placement (the next container is too large for the next step),
    so the group takes a pass per step."""
    for first in groups:
        ln = _lanes(rng, rows.size, len(steps)) + first
        perm = np.argsort(rng.random((rows.size, len(steps))), axis=1)
        for j, cpu in enumerate(steps):
            _put(nodes, rows, np.take_along_axis(ln, perm[:, j:j + 1], axis=1)[:, 0], cpu)


def test_several_passes_in_one_group(planner, O):
    """Groups 0 and 4 of segment 0 hold a staircase of six nodes, group 2 of segment 1 one of five below the
    demands of the first batch its link brings: the re-test runs a pass per step within one (batch, group)."""
    C, N = 320, 2113
    cont, nodes, level, rows = _base(34, C, N)
    rng = np.random.default_rng(3434)
    _stairs(nodes, rows, rng, (0, 4 * 64))
    _stairs(nodes, rows, rng, (SEG + 2 * 64,), STAIRS_1)
    _fill(nodes, rows, 11 * 64, 40)
    _fill(nodes, rows, SEG + 6 * 64, 64)
    _fill(nodes, rows, 2 * SEG, 64)

    def pre(e_assign, _after):
        a0 = e_assign[rows, :64]
        # group 0's steps take the containers 5, 15, 25, 35, 45, 55 (the first that fits each step)
        assert ((a0[:, 5:64:10] // 64) == 0).all() and ((a0 // 64 == 0).sum(axis=1) == 6).all()
        assert ((a0 // 64 == 4).sum(axis=1) == 6).all()
        for tot, seg in _replay(cont, nodes, level, rows):
            assert seg[0]["max_pair_passes"] >= 6 and seg[1]["max_pair_passes"] >= 3

    _run(planner, O, C, N, cont, nodes, level, 8, "several passes in one group", pre)


def test_mix_and_second_batch_on_the_live_table(planner, O):
    """All-zero containers, CYCLE members and screened containers in the batches of the staircase case and of
    the random scenarios, then a second batch on the node state the first one left."""
    C, N = 256, 2200
    cont, nodes, level, rows = _base(35, C, N, 0.12, zero_p=0.05, cycle_p=0.03, absent_p=0.1)
    rng = np.random.default_rng(3535)
    _stairs(nodes, rows, rng, (64, 6 * 64, SEG + 64, 2 * SEG + 3 * 64))
    _fill(nodes, rows, 10 * 64, 50)
    _fill(nodes, rows, SEG + 8 * 64, 64)
    cpu, mem, req, conf = cont
    zero = np.zeros((S, C), bool)
    zero[rows] = rng.random((rows.size, C)) < 0.05           # zeros sort last in FFD order: the index order holds
    for a in (cpu, mem, req, conf):
        a[zero] = 0
    req[rows] = np.where((rng.random((rows.size, C)) < 0.1) & ~zero[rows], LW.ABSENT, req[rows]).astype(np.uint32)
    level[rows] = np.where(rng.random((rows.size, C)) < 0.03, NONE, 0).astype(np.uint32)

    def pre(e_assign, _after):
        fa = e_assign.reshape(-1)
        z = ((cpu | mem | req | conf) == 0).reshape(-1) & (level.reshape(-1) == 0)
        assert int(z.sum()) >= S * 5 and (fa[z] != NONE).all()
        assert int((level == NONE).sum()) >= S * 3
        scr = ((req & LW.ABSENT) != 0) & (level == 0)
        assert int(scr.sum()) >= S * 10 and (e_assign[scr] == NONE).all()
        for tot, seg in _replay(cont, nodes, level, rows):
            assert tot["max_pair_passes"] >= 3
        odd = [R.replay_checked([a[s] for a in cont], [a[s] for a in nodes], level[s])[1] for s in (1, 3)]
        assert all(t["passes"] >= 1 for t in odd), "the random scenarios re-test too"

    got, want = _run(planner, O, C, N, cont, nodes, level, 9, "zero / CYCLE / screened", pre)
    assert int((want[1] == 2).sum()) >= S * 3                 # CYCLE
    after = [got[3][0].reshape(S, N), got[3][1].reshape(S, N), nodes[2], got[3][3].reshape(S, N), nodes[4]]
    assert int((after[0] != nodes[0]).sum()) >= S * 32        # the table is live
    cont2, _, level2 = LW._random(355, C, N, 0.12)
    _, want2 = _run(planner, O, C, N, cont2, after, level2, 0, "second batch on the live table")
    assert int((want2[0] != NONE).sum()) >= S * C // 16 and int((want2[1] == 1).sum()) >= S


def test_values_that_do_not_pack_take_the_u32_twin(planner, O):
    """The staircase case with one odd cpu demand beside a free capacity above 2^15: no shift packs the batch,
    the u32 twin runs it and gives the oracle's plan."""
    C, N = 320, 2113
    cont, nodes, level, rows = _base(36, C, N)
    rng = np.random.default_rng(3636)
    _stairs(nodes, rows, rng, (0, 4 * 64, SEG + 2 * 64))
    _fill(nodes, rows, 11 * 64, 40)
    _fill(nodes, rows, SEG + 6 * 64, 64)
    cont[0][1, 3] = 1
    nodes[0][1, 5] = 40000

    def pre(e_assign, _after):
        a0 = e_assign[rows, :64]
        assert ((a0 // 64 == 0).sum(axis=1) == 6).all() and ((a0 // 64 == 4).sum(axis=1) == 6).all()

    _run(planner, O, C, N, cont, nodes, level, 0, "values that do not pack", pre, packed=False)
