"""GPU parity of the lazy group walk of the packed 4096-scenario FFD kernel (fp_pipe.hip, bigp with
FPP_BIGP_LAZY): no prescan, each group's corner is tested where the walk reaches the group, the group's
queue is what is left of the batch, and a batch with nothing left leaves the walk.

Every case is a batch of 4096 scenarios, so that this kernel runs (asserted through place_path), on
three 12-group segments with a padded last one (34 or 35 groups of 64 nodes: 2113 <= N <= 2234), and is checked against the C oracle: all 4096 costs,
every assign / reason entry and the node tables after.

The even scenarios of a case are designed, the odd ones random (test_gpu_bigp_seven_waves.py's
generator).  In a designed scenario the cpu demands fall strictly with the index, so FFD position =
index and segment 0's batch k is containers 64 k .. 64 k + 63; every demand has mem = 64, "big" nodes
have (cpu, mem) = (CPU0, 64) and so take exactly one container each, whatever its index, and every
other node is tiny or cordoned.  The containers therefore fill the big nodes in node order, and where
the big nodes sit decides which groups a batch's walk enters.  How many big nodes a group has and on
which lanes differs from scenario to scenario.  Each case asserts from the oracle's plan, before the
GPU is asked, that the walk's case is carried:

* carry-over: one batch lands in at least four groups of a segment, group 11 among them, and one of
  them directly after a group whose corner is empty for the batch;
* early exit: a batch placed whole in the segment's first group, the next batch in later groups;
* corner in the last group only: groups 0-10 cannot take the batch's smallest demands, group 11 can;
* label-only misses: nodes that fit by capacity sit in early groups without the required label, and
  the batch is placed further on, those nodes untouched;
* the mix as before (all-zero containers, CYCLE members, screened containers; a second batch on the
  live table) on three segments;
* a designed batch whose values do not pack: the u32 twin runs it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
S = 4096
SEG = 768             # nodes per 12-group segment
CPU0 = 1000           # the largest demand of a designed scenario, and a big node's cpu
LABEL = 1 << 5        # a label the random generator never sets
ABSENT = 1 << 30      # a label no node carries: the stage-2 screen rejects its containers


def _oracle(O, C, N, cont, nodes, level, base):
    """The oracle's (assign, reason, cost, nodes_after 0 / 1 / 3) of a scenario-major batch."""
    def one(s):
        c = tuple(a[s * C:(s + 1) * C] for a in cont)
        n = tuple(a[s * N:(s + 1) * N] for a in nodes)
        ea, er, after, _ = O.place(c, n, level=level[s * C:(s + 1) * C])
        return ea, er, O.cost(ea, N, base + s), after

    with ThreadPoolExecutor(16) as ex:
        plans = list(ex.map(one, range(S)))
    cat = lambda f: np.concatenate([f(p) for p in plans])  # noqa: E731
    return (cat(lambda p: p[0]), cat(lambda p: p[1]), np.array([p[2] for p in plans], np.uint64),
            {i: cat(lambda p, i=i: p[3][i]) for i in (0, 1, 3)})


def _check(got, want, C, N, what):
    assign, reason, cost, after = got
    e_assign, e_reason, e_cost, e_after = want
    bad = np.nonzero(cost != e_cost)[0]
    assert bad.size == 0, f"{what}: {bad.size} costs differ from the oracle, first scenarios {bad[:5].tolist()}"
    for name, g, e, per in (("assign", assign, e_assign, C), ("reason", reason, e_reason, C),
                            ("cpu_free", after[0], e_after[0], N), ("mem_free", after[1], e_after[1], N),
                            ("conflict_used", after[3], e_after[3], N)):
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (f"{what}: {name} differs from the oracle in {bad.size} entries, first "
                               f"{bad[:5].tolist()} (scenario {int(bad[0]) // per})")


def _random(seed, C, N, big_p, zero_p=0.0, cycle_p=0.0, absent_p=0.0):
    """test_gpu_bigp_seven_waves.py's batch: values that pack (cpu multiples of 2, mem multiples of 64), a
    share `big_p` of the nodes takes about two containers each and the others next to none."""
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


def _design(seed, cont, nodes, C, N, layout):
    """Overwrites the even scenarios with a designed one (module docstring).  layout: {(segment, group):
    (lo, hi)}, the group gets lo .. hi big nodes on random lanes (drawn per scenario).  Returns the
    designed scenarios' indices and, per (segment, group), the big nodes as a bool (rows, N) array."""
    rng = np.random.default_rng(seed)
    rows = np.arange(0, S, 2)
    R = rows.size
    cpu, mem, req, conf = cont
    cf, mf, lab, cu, sched = nodes
    cpu[rows] = (CPU0 - 2 * np.arange(C)).astype(np.uint32)
    mem[rows] = 64
    req[rows] = 0
    conf[rows] = 0
    cf[rows] = 2
    mf[rows] = 64
    cu[rows] = 0
    lab[rows] = rng.integers(0, 16, (R, N)).astype(np.uint32)
    sched[rows] = (rng.random((R, N)) >= 0.25).astype(np.uint8)  # a quarter of the tiny nodes cordoned
    bigs = {}
    for (b, g), (lo, hi) in layout.items():
        first = b * SEG + g * 64
        width = min(64, N - first)
        assert 0 < lo <= hi <= width, (b, g, width)
        k = rng.integers(lo, hi + 1, R)
        rank = np.argsort(np.argsort(rng.random((R, width)), axis=1), axis=1)
        m = np.zeros((R, N), bool)
        m[:, first:first + width] = rank < k[:, None]
        bigs[(b, g)] = m
        for a, v in ((cf, CPU0), (mf, 64), (sched, 1)):
            x = a[rows]
            x[m] = v
            a[rows] = x
    return rows, bigs


def _flat(cont, nodes, level):
    return [a.reshape(-1) for a in cont], [a.reshape(-1) for a in nodes], level.reshape(-1)


def _run(planner, O, C, N, cont, nodes, level, base, what, pre=None, packed=True):
    """`pre(e_assign (S, C), e_after)` asserts the case from the oracle's plan before the GPU is asked."""
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["bounded"], geo["segments"]) == (12, 1, 0, 3), geo
    assert 2 * SEG + 1 <= N <= 3 * SEG - 70 and 192 <= C <= 448
    fc, fn, fl = _flat(cont, nodes, level)
    want = _oracle(O, C, N, fc, fn, fl, base)
    if pre is not None:
        pre(want[0].reshape(S, C), want[3])
    got = planner.place_batch(S, C, N, fc, fn, level=fl, scen_base=base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == packed, path
    _check(got, want, C, N, what)
    return got, want


def _corner_holds(nodes, rows, b, g, N, qc, qm=64):
    """Per designed scenario: does group g of segment b hold a schedulable node with room for (qc, qm)
    at the start?  (Capacity only shrinks: an empty corner stays empty.)"""
    first = b * SEG + g * 64
    sl = slice(first, min(first + 64, N))
    cf, mf, _, _, sched = nodes
    return ((sched[rows, sl] != 0) & (cf[rows, sl] >= qc[:, None]) & (mf[rows, sl] >= qm)).any(axis=1)


def _groups_hit(a, b):
    """Bit set (one int per scenario) of segment b's groups that the assignments a (rows, k) name."""
    inseg = (a != NONE) & (a // SEG == b)
    g = np.where(inseg, (a % SEG) // 64, 0)
    return np.bitwise_or.reduce(np.where(inseg, 1 << g, 0), axis=1)


def _popcount(x):
    return np.array([bin(int(v)).count("1") for v in x])


CARRY = {(0, 1): (6, 12), (0, 3): (12, 20), (0, 5): (3, 6), (0, 11): (16, 24),
         (1, 0): (3, 6), (1, 4): (8, 12), (1, 10): (16, 24), (1, 11): (6, 10),
         (2, 2): (30, 50), (2, 10): (4, 9)}


def _carry_pre(cont, nodes, rows, C, N):
    def pre(e_assign, _after):
        a0 = e_assign[rows, :64]                                  # segment 0's first batch
        hit = _groups_hit(a0, 0)
        assert (_popcount(hit) >= 4).all() and ((hit >> 11) & 1).all(), "four groups, group 11 among them"
        qc = cont[0][rows, 63]
        # groups 0 and 2 hold only tiny or cordoned nodes: groups 1 and 3 come directly after an empty corner
        for g in (0, 2):
            assert not _corner_holds(nodes, rows, 0, g, N, qc).any()
            assert ((hit >> (g + 1)) & 1).all()
        assert ((a0 == NONE) | (a0 >= SEG)).any(axis=1).all(), "the batch sends containers over the link too"
        # the link-fed segments carry across groups as well: segment 1 in four groups with its group 11,
        # the padded segment 2 in its partial group 10
        assert (_popcount(_groups_hit(e_assign[rows], 1)) >= 4).all() and ((_groups_hit(e_assign[rows], 1) >> 11) & 1).all()
        assert ((_groups_hit(e_assign[rows], 2) >> 10) & 1).all()
        assert (e_assign[rows] == NONE).any(axis=1).all()
    return pre


def test_carry_over_across_groups(planner, O):
    """Batch 0 of segment 0 is placed in groups 1, 3, 5 and 11 and overflows; groups 0, 2, 4, 6-10 hold no
    node for it.  Segments 1 and 2 get the same shape through their links."""
    C, N = 256, 2200
    cont, nodes, level = _random(11, C, N, 0.05)
    rows, _ = _design(111, cont, nodes, C, N, CARRY)
    _run(planner, O, C, N, cont, nodes, level, 3, "carry-over", _carry_pre(cont, nodes, rows, C, N))


def test_early_exit_in_the_first_group(planner, O):
    """Group 0 of segment 0 is 64 big nodes: batch 0 is placed there whole and the walk has nothing left;
    batch 1 finds group 0 full and lands in groups 4 and 9.  Segment 1's first group takes a whole slot too."""
    C, N = 320, 33 * 64 + 1                                   # the last segment: nine groups and one node
    cont, nodes, level = _random(12, C, N, 0.05)
    rows, _ = _design(112, cont, nodes, C, N, {(0, 0): (64, 64), (0, 4): (24, 30), (0, 9): (40, 44),
                                              (1, 0): (64, 64), (1, 7): (10, 20), (2, 0): (5, 30)})

    def pre(e_assign, _after):
        a0, a1 = e_assign[rows, :64], e_assign[rows, 64:128]
        assert (a0 < 64).all(), "batch 0 whole in group 0"
        assert (a1 != NONE).all() and (a1 >= 64).all()
        hit = _groups_hit(a1, 0)
        assert ((hit & 1) == 0).all() and ((hit >> 4) & 1).all() and ((hit >> 9) & 1).all()
        seg1_g0 = ((e_assign[rows] >= SEG) & (e_assign[rows] < SEG + 64)).sum(axis=1)
        assert (seg1_g0 == 64).all()

    _run(planner, O, C, N, cont, nodes, level, 0, "early exit", pre)


def test_corner_in_the_last_group_only(planner, O):
    """Groups 0-10 of segment 0 hold nodes of cpu 400 only (and tiny ones): too small for batch 0's
    smallest demand (874), so its walk passes eleven empty corners and places in group 11.  From container
    300 on (cpu 400 and below) the batches find their corner in groups 0-10."""
    C, N = 448, 3 * SEG - 70
    cont, nodes, level = _random(13, C, N, 0.05)
    rows, _ = _design(113, cont, nodes, C, N, {(0, 11): (30, 50), (1, 11): (40, 64), (2, 3): (20, 44)})
    rng = np.random.default_rng(1313)
    mid = np.zeros((rows.size, N), bool)
    mid[:, :11 * 64] = rng.random((rows.size, 11 * 64)) < 0.04
    for a, v in ((nodes[0], 400), (nodes[1], 64), (nodes[4], 1)):
        x = a[rows]
        x[mid] = v
        a[rows] = x

    def pre(e_assign, _after):
        a0 = e_assign[rows, :64]
        qc = cont[0][rows, 63]
        for g in range(11):
            assert not _corner_holds(nodes, rows, 0, g, N, qc).any()
        assert _corner_holds(nodes, rows, 0, 11, N, qc).all()
        assert (_groups_hit(a0, 0) == 1 << 11).all()
        late = e_assign[rows, 300:]                               # cpu 400 and below: the cpu-400 nodes take them
        assert ((_groups_hit(late, 0) & 0x7FF) != 0).all()

    _run(planner, O, C, N, cont, nodes, level, 7, "corner in the last group only", pre)


def test_label_only_misses(planner, O):
    """Every container of batch 0 (and every second one of batch 1) requires LABEL.  Groups 1 and 2 of
    segment 0 hold big nodes without it -- between 1 and 40 of them, on either side of the re-filter's
    limit -- so their corners hold nodes, their queues find nothing, and the batch is placed in groups 6
    and 11, whose big nodes carry the label."""
    C, N = 192, 2150
    cont, nodes, level = _random(14, C, N, 0.05)
    rows, bigs = _design(114, cont, nodes, C, N, {(0, 1): (1, 40), (0, 2): (1, 6), (0, 6): (20, 30),
                                                 (0, 11): (20, 30), (1, 5): (30, 60), (2, 0): (1, 1)})
    req, lab = cont[2], nodes[2]
    req[rows, :64] = LABEL
    req[np.ix_(rows, np.arange(64, 128, 2))] = LABEL
    x = lab[rows]
    x &= ~np.uint32(LABEL)
    for key in ((0, 6), (0, 11), (1, 5), (2, 0)):
        x[bigs[key]] |= LABEL
    lab[rows] = x
    bare = bigs[(0, 1)] | bigs[(0, 2)]

    def pre(e_assign, e_after):
        a0 = e_assign[rows, :64]
        hit = _groups_hit(a0, 0)
        assert ((hit & 0b110) == 0).all() and ((hit >> 6) & 1).all() and ((hit >> 11) & 1).all()
        qc = cont[0][rows, 0]                                     # the nodes fit the batch's LARGEST demand
        assert _corner_holds(nodes, rows, 0, 1, N, qc).all() and _corner_holds(nodes, rows, 0, 2, N, qc).all()
        # batch 0 leaves the unlabelled big nodes alone; batch 1's containers without a requirement take them
        n_bare = bare.sum(axis=1)
        on_bare = np.take_along_axis(np.concatenate([bare, np.zeros((rows.size, 1), bool)], axis=1),
                                     np.minimum(e_assign[rows, 64:128], N).astype(np.int64), axis=1)
        assert (on_bare.sum(axis=1) == np.minimum(n_bare, 32)).all()
        assert (n_bare <= 5).any() and (n_bare > 10).any()

    _run(planner, O, C, N, cont, nodes, level, 1, "label-only misses", pre)


def test_mix_and_second_batch_on_the_live_table(planner, O):
    """All-zero containers, CYCLE members and screened containers in the batches of a carry-over case and
    of the random scenarios, then a second batch on the node state the first one left."""
    C, N = 256, 2200
    cont, nodes, level = _random(15, C, N, 0.12, zero_p=0.05, cycle_p=0.03, absent_p=0.1)
    rows, _ = _design(115, cont, nodes, C, N, CARRY)
    rng = np.random.default_rng(1515)
    cpu, mem, req, conf = cont
    zero = np.zeros((S, C), bool)
    zero[rows] = rng.random((rows.size, C)) < 0.05           # zeros sort last in FFD order: the index order holds
    for a in (cpu, mem, req, conf):
        a[zero] = 0
    req[rows] = np.where((rng.random((rows.size, C)) < 0.1) & ~zero[rows], ABSENT, req[rows]).astype(np.uint32)
    level[rows] = np.where(rng.random((rows.size, C)) < 0.03, NONE, 0).astype(np.uint32)

    def pre(e_assign, _after):
        fa = e_assign.reshape(-1)
        z = ((cpu | mem | req | conf) == 0).reshape(-1) & (level.reshape(-1) == 0)
        assert int(z.sum()) >= S * 5 and (fa[z] != NONE).all()
        assert int((level == NONE).sum()) >= S * 3
        scr = ((req & ABSENT) != 0) & (level == 0)
        assert int(scr.sum()) >= S * 10 and (e_assign[scr] == NONE).all()
        # the designed scenarios still carry across groups of segment 0 within one batch
        assert (_popcount(_groups_hit(e_assign[rows, :64], 0)) >= 4).all()

    got, want = _run(planner, O, C, N, cont, nodes, level, 9, "zero / CYCLE / screened", pre)
    assert int((want[1] == 2).sum()) >= S * 3                 # CYCLE
    after = [got[3][0].reshape(S, N), got[3][1].reshape(S, N), nodes[2], got[3][3].reshape(S, N), nodes[4]]
    assert int((after[0] != nodes[0]).sum()) >= S * 32        # the table is live
    cont2, _, level2 = _random(155, C, N, 0.12)
    _, want2 = _run(planner, O, C, N, cont2, after, level2, 0, "second batch on the live table")
    assert int((want2[0] != NONE).sum()) >= S * C // 16 and int((want2[1] == 1).sum()) >= S


def test_values_that_do_not_pack_take_the_u32_twin(planner, O):
    """The carry-over case with one odd cpu demand beside a free capacity above 2^15: no shift packs the
    batch, `big` runs it."""
    C, N = 256, 2200
    cont, nodes, level = _random(16, C, N, 0.05)
    rows, _ = _design(116, cont, nodes, C, N, CARRY)
    cont[0][1, 3] = 1
    nodes[0][1, 5] = 40000
    _run(planner, O, C, N, cont, nodes, level, 0, "values that do not pack", _carry_pre(cont, nodes, rows, C, N),
         packed=False)
