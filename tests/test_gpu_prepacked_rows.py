"""GPU parity of the prepacked FFD demand rows (FP_OPT_PREPACK; fp_place.hip k_scen_sort's prepack mode,
fp_pipe.hip k_unpack_rows and the prepacked-input form of the packed 4096-scenario kernel).

Where the 4096-scenario pair runs, the fused sort packs a scenario's (cpu, mem) demands into ONE row with
shifts from the scenario's own OR words (its containers' value table and its schedulable nodes), carries the
skip bit in the row's bit 31, and the packed kernel reads that row with the scenario's shifts.  A batch that
does not pack as a whole is repaired into the legacy rows and runs on the u32 twin.

Every case is a batch of 4096 scenarios on three 12-group segments (2113 <= N <= 2234), asserted through
geometry and place_path, with 192 <= C <= 448 -- except the one case that needs a sort bucket above 1024
containers, which no C <= 448 reaches: it runs C = 2048 with one cpu value -- and is checked against the C
oracle: all 4096 costs, every assign / reason entry and the node tables after."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
S = 4096
ABSENT = 1 << 30      # a label no node carries: the stage-2 screen rejects its containers
FIELD_MAX = 0x7FFF    # the largest packed field


def _oracle(O, C, N, cont, nodes, level, base):
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


def _random(seed, C, N, big_p=0.12, zero_p=0.0, cycle_p=0.0, absent_p=0.0, ucpu=2, umem=64):
    """Values that pack: cpu multiples of ucpu, mem multiples of umem ((S, 1) arrays give a unit per scenario);
    a share big_p of the nodes takes about two containers each, the others next to none."""
    rng = np.random.default_rng(seed)
    ucpu, umem = np.asarray(ucpu, np.int64), np.asarray(umem, np.int64)
    cpu = (ucpu * rng.integers(1, 40, (S, C))).astype(np.uint32)
    mem = (umem * rng.integers(1, 24, (S, C))).astype(np.uint32)
    req = np.where(rng.random((S, C)) < 0.3, 1 << rng.integers(0, 4, (S, C)), 0).astype(np.uint32)
    conf = np.where(rng.random((S, C)) < 0.1, 1 << rng.integers(0, 32, (S, C)), 0).astype(np.uint32)
    req = np.where(rng.random((S, C)) < absent_p, req | ABSENT, req).astype(np.uint32)
    zero = rng.random((S, C)) < zero_p
    for a in (cpu, mem, req, conf):
        a[zero] = 0
    level = np.where(rng.random((S, C)) < cycle_p, NONE, 0).astype(np.uint32)
    big = rng.random((S, N)) < big_p
    cf = np.where(big, ucpu * rng.integers(20, 60, (S, N)), ucpu).astype(np.uint32)
    mf = np.where(big, umem * rng.integers(12, 40, (S, N)), umem).astype(np.uint32)
    lab = rng.integers(0, 16, (S, N)).astype(np.uint32)
    cu = np.where(rng.random((S, N)) < 0.05, 1 << rng.integers(0, 32, (S, N)), 0).astype(np.uint32)
    sched = (rng.random((S, N)) >= 0.05).astype(np.uint8)
    return [cpu, mem, req, conf], [cf, mf, lab, cu, sched], level


def _flat(cont, nodes, level):
    return [a.reshape(-1) for a in cont], [a.reshape(-1) for a in nodes], level.reshape(-1)


def _run(planner, O, C, N, cont, nodes, level, base, what, packed=True, want=None, small_c=True, prepack=True):
    """place_path must name the new path: the prepacked-input kernel for a batch that packs, the u32 twin
    behind a repair pass that unpacked at least one scenario for one that does not (prepack=False: the
    option is off, the legacy rows and kernels)."""
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["bounded"], geo["segments"]) == (12, 1, 0, 3), geo
    assert 2113 <= N <= 2234 and (not small_c or 192 <= C <= 448)
    fc, fn, fl = _flat(cont, nodes, level)
    if want is None:
        want = _oracle(O, C, N, fc, fn, fl, base)
    got = planner.place_batch(S, C, N, fc, fn, level=fl, scen_base=base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == packed, path
    assert path["prepacked"] == (prepack and packed) and path["repaired"] == (prepack and not packed), path
    _check(got, want, C, N, what)
    return got, want


def test_every_kind_of_container_and_a_second_batch(planner, O):
    """All-zero containers, CYCLE members (level) and screened containers in a batch that packs: the skip bit
    lives in the packed row's bit 31 from the sort's phase P to segment 0, a skipped container keeps its
    reason and an all-zero one its node.  C is no multiple of 64.  Then a second batch on the live table: the
    workspace (rows, header) is reused."""
    C, N = 301, 2200
    cont, nodes, level = _random(21, C, N, zero_p=0.05, cycle_p=0.04, absent_p=0.1)
    got, want = _run(planner, O, C, N, cont, nodes, level, 5, "zero / CYCLE / screened")
    cpu, mem, req, conf = cont
    z = ((cpu | mem | req | conf) == 0) & (level == 0)
    e_assign, e_reason = want[0].reshape(S, C), want[1].reshape(S, C)
    assert int(z.sum()) >= S * 5 and (e_assign[z] != NONE).all()
    assert int((e_reason == 2).sum()) >= S * 5                    # CYCLE
    scr = ((req & ABSENT) != 0) & (level == 0)
    assert int(scr.sum()) >= S * 10 and (e_assign[scr] == NONE).all()
    after = [got[3][0].reshape(S, N), got[3][1].reshape(S, N), nodes[2], got[3][3].reshape(S, N), nodes[4]]
    assert int((after[0] != nodes[0]).sum()) >= S * 32            # the table is live
    cont2, _, level2 = _random(211, C, N, zero_p=0.02, cycle_p=0.02)
    _, want2 = _run(planner, O, C, N, cont2, after, level2, 0, "second batch on the live table")
    assert int((want2[0] != NONE).sum()) >= S * C // 16


def test_shifts_differ_per_scenario(planner, O):
    """Even scenarios hold multiples of 64 in cpu and of 2 in mem, odd scenarios the reverse, so no two
    neighbours pack with the same shifts (the batch's are 1 and 1).  In scenarios 0, 1 mod 4 the nodes set the
    shifts (the containers are multiples of four times the unit), in 2, 3 mod 4 the containers do.  Cordoned
    nodes carry odd values: they are outside the OR words, their records are zero and never written back."""
    C, N = 333, 2150
    even = (np.arange(S) % 2 == 0)[:, None]
    ucpu, umem = np.where(even, 64, 2), np.where(even, 2, 64)
    cont, nodes, level = _random(22, C, N, ucpu=ucpu, umem=umem)
    by_nodes = (np.arange(S) % 4 < 2)[:, None]
    cont[0][:] = np.where(by_nodes, cont[0] * 4, cont[0])         # containers coarser: the nodes set the shift
    cont[1][:] = np.where(by_nodes, cont[1] * 4, cont[1])
    nodes[0][:] = np.where(by_nodes, nodes[0], nodes[0] * 4)      # nodes coarser: the containers set it
    nodes[1][:] = np.where(by_nodes, nodes[1], nodes[1] * 4)
    off = nodes[4] == 0
    nodes[0][off] |= 1
    nodes[1][off] |= 1
    assert int(max(cont[0].max(), nodes[0][~off].max())) >> 1 <= FIELD_MAX   # the batch packs (shifts 1, 1)
    assert int(max(cont[1].max(), nodes[1][~off].max())) >> 1 <= FIELD_MAX
    got, _ = _run(planner, O, C, N, cont, nodes, level, 2, "per-scenario shifts")
    assert (got[3][0].reshape(S, N)[off] & 1).all() and (got[3][1].reshape(S, N)[off] & 1).all()


def _limit_batch(seed, C, N):
    """Every scenario's largest cpu field is exactly 0x7FFF << 1 and its largest mem field 0x7FFF << 6 (node 0,
    schedulable); all shifts are 1 and 6."""
    cont, nodes, level = _random(seed, C, N)
    nodes[0][:, 0] = FIELD_MAX << 1
    nodes[1][:, 0] = FIELD_MAX << 6
    nodes[4][:, 0] = 1
    return cont, nodes, level


def test_field_limit_still_packs(planner, O):
    C, N = 256, 2113
    cont, nodes, level = _limit_batch(23, C, N)
    _run(planner, O, C, N, cont, nodes, level, 0, "fields at 0x7FFF << sc")


def test_one_scenario_past_the_limit_takes_the_repair_pass_and_the_u32_twin(planner, O):
    """One scenario holds 0x8000 << 1 in cpu: the batch does not pack by its OR words.  Every other scenario
    packs on its own and was written as one row: k_unpack_rows turns those back into cpu / mem / position rows
    (bucket bits, skip bits) and the u32 twin runs all of them."""
    C, N = 256, 2113
    cont, nodes, level = _random(24, C, N, zero_p=0.03, cycle_p=0.03, absent_p=0.05)
    nodes[0][:, 0] = FIELD_MAX << 1
    nodes[1][:, 0] = FIELD_MAX << 6
    nodes[4][:, 0] = 1
    nodes[0][1777, 0] = 0x8000 << 1
    _run(planner, O, C, N, cont, nodes, level, 0, "one scenario past the limit", packed=False)


def test_every_sort_branch_in_prepack_mode(planner, O):
    """One batch through every branch of the sort: scenarios ranked against the sample's values (pass 0),
    scenarios >= 8 holding a value the sample lacks (pass 1: their own value set and OR words), and scenarios
    with more than 256 distinct mem values (the generic fallback, which forms its OR words in its counting
    passes).  (The fourth branch, a bucket above 1024 containers, needs C > 1024: the next test.)"""
    C, N = 448, 2234
    cont, nodes, level = _random(25, C, N, zero_p=0.02, cycle_p=0.02, absent_p=0.05)
    cpu, mem = cont[0], cont[1]
    own = np.arange(8, S, 3)                                     # pass 1: values outside the sample's set
    cpu[own, 5] = 2 * 45
    mem[own, 9] = 64 * 31
    gen = np.array([9, 1001, 4095])                              # generic: 448 distinct mem values, multiples of 64
    mem[gen] = (64 * (1 + np.arange(C)))[None, :]
    assert len(np.unique(mem[gen[0]])) > 256 and 2 * 45 not in np.unique(cpu[:8]) and 64 * 31 not in np.unique(mem[:8])
    _run(planner, O, C, N, cont, nodes, level, 1, "pass 0 / pass 1 / generic")


def test_a_bucket_above_1024_containers(planner, O):
    """All demands of a scenario share one cpu value: one bucket of 2048 containers, which the sort scatters
    straight to HBM (no C <= 448 reaches that branch).  Most nodes are big, so the plan is short to check."""
    C, N = 2048, 2113
    rng = np.random.default_rng(26)
    cont, nodes, level = _random(26, 1, N, big_p=0.9)
    cpu = np.repeat((2 * rng.integers(1, 40, (S, 1))).astype(np.uint32), C, axis=1)
    mem = (64 * rng.integers(1, 24, (S, C))).astype(np.uint32)
    req = np.where(rng.random((S, C)) < 0.05, ABSENT, 0).astype(np.uint32)
    conf = np.zeros((S, C), np.uint32)
    level = np.where(rng.random((S, C)) < 0.02, NONE, 0).astype(np.uint32)
    nodes[0][:] = 2 * 2000
    nodes[1][:] = 64 * 500
    _run(planner, O, C, N, [cpu, mem, req, conf], nodes, level, 0, "one bucket of 2048", small_c=False)


def test_option_off_gives_the_same_outputs(planner, O, opts):
    """FP_OPT_PREPACK = 0 (the three legacy rows and the packed kernel that reads them) against the default on
    one random batch: identical outputs, both equal to the oracle's."""
    C, N = 257, 2200
    cont, nodes, level = _random(27, C, N, zero_p=0.02, cycle_p=0.02, absent_p=0.05)
    on, want = _run(planner, O, C, N, cont, nodes, level, 4, "prepack on")
    opts(prepack=0)
    cont2, nodes2, level2 = _random(27, C, N, zero_p=0.02, cycle_p=0.02, absent_p=0.05)
    off, _ = _run(planner, O, C, N, cont2, nodes2, level2, 4, "prepack off", want=want, prepack=False)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    for i in (0, 1, 3):
        assert np.array_equal(on[3][i], off[3][i])
