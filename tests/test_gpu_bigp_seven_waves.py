"""GPU parity of the packed 4096-scenario FFD kernel (fp_pipe.hip, bigp): one-wave 12-group segments
at seven waves per SIMD, candidate groups from the batch corner alone (no bucket masks, a dynamic
LDS size of its own beside its u32 twin's).

Every case is a batch of 4096 scenarios, so that this kernel runs (asserted through place_path), and
is checked against the C oracle: all 4096 costs, every plan, and scenarios 0, 2047 and 4095 by name.
The inputs are built so that what the change touches carries containers -- asserted from the oracle's
plan before the GPU is asked:

* three segments per scenario: the middle one is fed by a link and feeds one;
* a padded last segment with lanes past N, and a third of the nodes cordoned: such lanes must take
  nothing, whatever the corner says;
* label queues: scenarios without any label requirement, scenarios where every container has one,
  and scenarios where one container in 64 has one that only the last node of a later group
  carries -- all three kinds in one batch;
* a live table: a second batch placed on the node state the first one left, where start-state bucket
  masks would have pruned and the corner alone must still give the oracle's plan;
* all-zero containers, CYCLE members and containers the stage-2 screen rejects, mixed in;
* a batch whose values do not pack: the u32 twin runs it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
S = 4096
NAMED = (0, 2047, 4095)
LABEL = 1 << 5        # the label of the one-in-64 scenarios
ABSENT = 1 << 30      # a label no node carries: the stage-2 screen rejects its containers


def _oracle(O, S_, C, N, cont, nodes, level, base):
    """The oracle's (assign, reason, cost, nodes_after 0 / 1 / 3) of a scenario-major batch."""
    def one(s):
        c = tuple(a[s * C:(s + 1) * C] for a in cont)
        n = tuple(a[s * N:(s + 1) * N] for a in nodes)
        ea, er, after, _ = O.place(c, n, level=level[s * C:(s + 1) * C])
        return ea, er, O.cost(ea, N, base + s), after

    with ThreadPoolExecutor(16) as ex:
        plans = list(ex.map(one, range(S_)))
    cat = lambda f: np.concatenate([f(p) for p in plans])  # noqa: E731
    return (cat(lambda p: p[0]), cat(lambda p: p[1]), np.array([p[2] for p in plans], np.uint64),
            {i: cat(lambda p, i=i: p[3][i]) for i in (0, 1, 3)})


def _check(got, want, C, N, what):
    assign, reason, cost, after = got
    e_assign, e_reason, e_cost, e_after = want
    bad = np.nonzero(cost != e_cost)[0]
    assert bad.size == 0, f"{what}: {bad.size} costs differ from the oracle, first scenarios {bad[:5].tolist()}"
    for s in NAMED:
        assert np.array_equal(assign[s * C:(s + 1) * C], e_assign[s * C:(s + 1) * C]), f"{what}: plan of scenario {s}"
        assert np.array_equal(reason[s * C:(s + 1) * C], e_reason[s * C:(s + 1) * C]), f"{what}: reasons of scenario {s}"
    for name, g, e, per in (("assign", assign, e_assign, C), ("reason", reason, e_reason, C),
                            ("cpu_free", after[0], e_after[0], N), ("mem_free", after[1], e_after[1], N),
                            ("conflict_used", after[3], e_after[3], N)):
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (f"{what}: {name} differs from the oracle in {bad.size} entries, first "
                               f"{bad[:5].tolist()} (scenario {int(bad[0]) // per})")


def _batch(seed, C, N, big_p, cordon=0.05, req_p=0.3, zero_p=0.0, cycle_p=0.0, absent_p=0.0):
    """A scenario-major batch whose values pack (cpu multiples of 2, mem multiples of 64, 15 bits after
    the shift).  A share `big_p` of the nodes takes about two containers each and the others next to
    none, so that a segment fills up and sends the rest over its link; each of four labels is on about
    half the nodes."""
    rng = np.random.default_rng(seed)
    cpu = (2 * rng.integers(1, 40, (S, C))).astype(np.uint32)
    mem = (64 * rng.integers(1, 24, (S, C))).astype(np.uint32)
    req = np.where(rng.random((S, C)) < req_p, 1 << rng.integers(0, 4, (S, C)), 0).astype(np.uint32)
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
    sched = (rng.random((S, N)) >= cordon).astype(np.uint8)
    flat = lambda *a: [x.reshape(-1) for x in a]  # noqa: E731
    return flat(cpu, mem, req, conf), flat(cf, mf, lab, cu, sched), level.reshape(-1)


def _run(planner, O, C, N, cont, nodes, level, base, what, packed=True, segments=None):
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["bounded"]) == (12, 1, 0), geo
    if segments is not None:
        assert geo["segments"] == segments, geo
    want = _oracle(O, S, C, N, cont, nodes, level, base)
    got = planner.place_batch(S, C, N, cont, nodes, level=level, scen_base=base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == packed, path
    _check(got, want, C, N, what)
    return got, want, geo


def _per_segment(e_assign, seg_nodes, segments):
    placed = e_assign[e_assign != NONE]
    return [int(((placed // seg_nodes) == b).sum()) for b in range(segments)]


def test_three_segments(planner, O):
    """C = 200 on 2304 nodes: three segments of 12 groups; the middle one reads a link and writes one."""
    C, N = 200, 2304
    cont, nodes, level = _batch(1, C, N, 0.05)
    (_, want, geo) = _run(planner, O, C, N, cont, nodes, level, 11, "three segments", segments=3)
    per = _per_segment(want[0], 768, 3)
    assert min(per) >= S * C // 20, per                      # every segment places its share
    assert int((want[1] == 1).sum()) >= S, int((want[1] == 1).sum())  # and the last one rejects


def test_padded_segment_and_cordoned_nodes(planner, O):
    """C = 256 on 1500 nodes: the last segment's last group holds 28 nodes and 36 lanes past N, and a
    third of the nodes are cordoned."""
    C, N = 256, 1500
    cont, nodes, level = _batch(2, C, N, 0.1, cordon=1 / 3)
    (_, want, geo) = _run(planner, O, C, N, cont, nodes, level, 0, "padded segment", segments=2)
    assert 0.3 < 1 - nodes[4].mean() < 0.37
    per = _per_segment(want[0], 768, 2)
    assert min(per) >= S * C // 20, per
    last = want[0][(want[0] != NONE) & (want[0] % N >= 1472)]  # the padded group takes containers too
    assert last.size >= S // 4, last.size
    assert int((want[1] == 1).sum()) >= S


def test_label_queues_of_three_kinds(planner, O):
    """Scenario s % 3 == 0: no container has a label requirement.  1: every container has one (of four
    labels that about half the nodes carry each).  2: FFD order is index order, one container in 64 needs
    LABEL, and only the last node of groups 7 and 19 carries it -- one lane of a queue, one node of a later
    group, in either segment."""
    C, N = 256, 1536
    cont, nodes, level = _batch(3, C, N, 0.08, req_p=0.0)
    cpu, mem, req, conf = (a.reshape(S, C) for a in cont)
    cf, mf, lab = (a.reshape(S, N) for a in nodes[:3])
    rng = np.random.default_rng(33)
    kind = np.arange(S) % 3
    req[kind == 1] = (1 << rng.integers(0, 4, ((kind == 1).sum(), C))).astype(np.uint32)
    k2 = kind == 2
    sched = nodes[4].reshape(S, N)
    cpu[k2] = (600 - 2 * np.arange(C)).astype(np.uint32)    # strictly decreasing: FFD position = index
    mem[k2] = 64
    req[k2] = 0
    req[np.ix_(k2, np.arange(17, C, 64))] = LABEL
    lab[k2] &= ~np.uint32(LABEL)
    cf[k2] = 600                                            # about one container per node ...
    mf[k2] = 64 * 4
    sched[k2, :320] = 0                                     # ... and segment 0 keeps three groups: it overflows
    for node, room in ((7 * 64 + 63, 1100), (19 * 64 + 63, 2000)):
        lab[k2, node] |= LABEL
        cf[k2, node] = room
        mf[k2, node] = 64 * 100
        sched[k2, node] = 1
    (_, want, geo) = _run(planner, O, C, N, cont, nodes, level, 5, "label queues", segments=2)
    e_assign = want[0].reshape(S, C)
    assert int((req[kind == 0] != 0).sum()) == 0 and int((req[kind == 1] == 0).sum()) == 0
    got_label = e_assign[k2][:, 17::64]
    assert np.isin(got_label, (7 * 64 + 63, 19 * 64 + 63, NONE)).all(), "only the labelled nodes take them"
    assert (got_label == 7 * 64 + 63).any() and (got_label == 19 * 64 + 63).any()  # in either segment
    for k in range(3):  # every kind sends containers over its link
        assert int((e_assign[kind == k] >= 768).sum() - (e_assign[kind == k] == NONE).sum()) > 0


def test_live_table_second_batch(planner, O):
    """A second generated batch placed on the node state the first one left (nothing restored): part-filled
    nodes of every size, where only the exact corner prunes."""
    C, N = 256, 1536
    cont, nodes, level = _batch(4, C, N, 0.12)
    (got, want, geo) = _run(planner, O, C, N, cont, nodes, level, 0, "first batch", segments=2)
    after = [got[3][0], got[3][1], nodes[2], got[3][3], nodes[4]]
    assert int((after[0] != nodes[0]).sum()) >= S * 64  # the table is live: many nodes part-filled
    cont2, _, level2 = _batch(44, C, N, 0.12)
    (_, want2, _) = _run(planner, O, C, N, cont2, after, level2, 0, "second batch on the live table", segments=2)
    assert int((want2[0] != NONE).sum()) >= S * C // 8 and int((want2[1] == 1).sum()) >= S


def test_zero_cycle_and_screened_containers(planner, O):
    """All-zero containers (placed on the tile's first schedulable node without a check), CYCLE members
    and containers that need a label no node carries (the stage-2 screen), mixed into every scenario."""
    C, N = 256, 1536
    cont, nodes, level = _batch(5, C, N, 0.08, zero_p=0.05, cycle_p=0.03, absent_p=0.1)
    (_, want, geo) = _run(planner, O, C, N, cont, nodes, level, 9, "zero / CYCLE / screened", segments=2)
    zero = (cont[0] | cont[1] | cont[2] | cont[3]) == 0
    assert int(zero.sum()) >= S * 5 and int((want[0][zero & (level == 0)] != NONE).all())
    assert int((want[1] == 2).sum()) >= S * 3           # CYCLE
    assert int(((cont[2] & ABSENT) != 0).sum()) >= S * 10
    assert (want[1][((cont[2] & ABSENT) != 0) & (level == 0)] == 1).all()


def test_values_that_do_not_pack_take_the_u32_twin(planner, O):
    """One odd cpu demand beside free capacities above 2^15: no shift packs the batch, `big` runs it."""
    C, N = 256, 1536
    cont, nodes, level = _batch(6, C, N, 0.08)
    cont[0][3] = 1
    nodes[0][5] = 40000
    _run(planner, O, C, N, cont, nodes, level, 0, "values that do not pack", packed=False, segments=2)
