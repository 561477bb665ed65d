"""GPU parity of the FFD pipeline's unpacked-bucket path and of its ring, flush, priority and
systolic-extra options (fp_pipe.hip, include/fleetplace.h enum fp_option).

fleetplace.h promises the same plan whatever the options: only the work schedule changes.  Three
families of that promise are checked here against the C oracle, bit for bit (assignment, reason,
node arrays 0, 1 and 3 after placement, and for batches the packed cost):

A. The switch at 2^21 containers.  Up to 2^21 containers an s_idx word carries the FFD position in
   bits 0..20 and the two bucket indices above (kpack); past it the word is all position, the buckets
   are searched per stage (bucket_of) and the kernel's position mask widens from IDX_POS_MASK to ~CYC.
   C = 2^21 (packed, largest position 0x1FFFFF), 2^21 + 1 and 2^21 + 200 pin the switch from both
   sides.  The inputs are built so that the containers at the highest positions are placed beyond
   the first segment (their position words cross a global link), rejected at the last stage, screened
   and CYCLE -- asserted from the oracle's plan before the GPU is asked.
B. FP_OPT_KPACK = 0 at small shapes through every kernel that writes s_idx words (the LDS sort's
   digit path and generic fallback, the radix paths, both payload kernels), every forced geometry,
   the six-wave many-scenario kernel and both record kinds.  Each case also runs with kpack automatic
   and the two GPU plans must be equal, so a disagreement names the option.
C. FP_OPT_PIPE_R 2..6, FP_OPT_PIPE_FLUSH 0..3, FP_OPT_PIPE_PRIO 0..2 and FP_OPT_SYSTOLIC_EXTRA
   0 / 1 / 128 / 1000 (clamped to 128), each against the oracle and against the same call with the
   option automatic.

Every forced geometry, ring depth and record kind is asserted through fp_place_geometry /
fp_ctx_place_path to be the one that ran.  Oracle plans are computed once per input and shared."""
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SEED = 0x5EED0B17
P21 = 1 << 21  # IDX_POS_MASK + 1: the largest C whose s_idx words carry the buckets

_CACHE = {}


def _cached(key, make):
    """Inputs and oracle plans are made once per module run and never changed."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Case:
    """The inputs of one placement call and the oracle's answer to them."""

    def __init__(self, O, conts, nodes, levels, base=0, batch=True):
        self.conts, self.nodes, self.levels, self.base, self.batch = conts, nodes, levels, base, batch
        self.S, self.C, self.N = len(conts), conts[0][0].size, nodes[0][0].size
        assert batch or self.S == 1

        def one(s):
            ea, er, eafter, _ = O.place(conts[s], nodes[s], level=levels[s])
            return ea, er, eafter, O.cost(ea, self.N, base + s)

        if self.S > 8:
            with ThreadPoolExecutor(16) as ex:
                plans = list(ex.map(one, range(self.S)))
        else:
            plans = [one(s) for s in range(self.S)]
        self.e_assign = np.concatenate([p[0] for p in plans])
        self.e_reason = np.concatenate([p[1] for p in plans])
        self.e_after = {i: np.concatenate([p[2][i] for p in plans]) for i in (0, 1, 3)}
        self.e_cost = np.array([p[3] for p in plans], np.uint64)

    def run(self, planner):
        """(assign, reason, cost or None, nodes_after) of the GPU under the context's current options."""
        if not self.batch:
            assign, reason, after = planner.place(self.conts[0], self.nodes[0], level=self.levels[0])
            return assign, reason, None, after
        cat = lambda parts, i: np.concatenate([p[i] for p in parts])  # noqa: E731
        return planner.place_batch(self.S, self.C, self.N, [cat(self.conts, i) for i in range(4)],
                                   [cat(self.nodes, i) for i in range(5)], level=np.concatenate(self.levels),
                                   scen_base=self.base)

    def check(self, got, what):
        """The GPU's result is the oracle's: assign, reason, node arrays 0, 1, 3 and (batches) the cost."""
        assign, reason, cost, after = got
        pairs = [("assign", assign, self.e_assign, self.C), ("reason", reason, self.e_reason, self.C)]
        pairs += [(f"nodes_after[{i}]", after[i], self.e_after[i], self.N) for i in (0, 1, 3)]
        if self.batch:
            pairs.append(("cost", cost, self.e_cost, 1))
        for name, g, e, per in pairs:
            assert g.shape == e.shape, (what, name)
            bad = np.nonzero(g != e)[0]
            assert bad.size == 0, (f"{what}: {name} differs from the oracle in {bad.size} entries, first "
                                   f"{bad[:5].tolist()} (scenario {int(bad[0]) // per})")


def _same(got, ref, what):
    """Two GPU results of the same call are equal, array for array."""
    names = ("assign", "reason", "cost", "nodes_after")
    for name, g, r in zip(names[:3], got[:3], ref[:3]):
        assert (g is None) == (r is None)
        if g is not None:
            assert np.array_equal(g, r), f"{what}: {name} differs from the run under automatic options"
    for i in (0, 1, 3):
        assert np.array_equal(got[3][i], ref[3][i]), f"{what}: nodes_after[{i}] differs from the automatic run"


def _forced_and_auto(planner, opts, case, forced, fixed=None, served=None):
    """Run `case` with the options `fixed` (a geometry, a sort path) and every other one automatic, then
    again with `forced` on top; both runs must give the oracle's result and each other's.  `served`,
    if given, is called once the forced options are set, to assert what the library will run."""
    if fixed:
        opts(**fixed)
    auto = case.run(planner)
    case.check(auto, f"automatic options over {fixed}")
    opts(**forced)
    if served:
        served()
    got = case.run(planner)
    case.check(got, f"{forced} over {fixed}")
    _same(got, auto, f"{forced} over {fixed}")
    return got


def _levels(rng, C):
    """About 1 % CYCLE members (level FP_NONE): the segment-0 store of a word with the skip bit set."""
    return np.where(rng.random(C) < 0.01, NONE, 0).astype(np.uint32)


def _cordon(rng, nodes, p=0.05):
    """The node table with about `p` of the schedulable nodes cordoned."""
    n = [np.array(a) for a in nodes]
    n[4] = (n[4].astype(bool) & (rng.random(n[4].size) >= p)).astype(np.uint8)
    return tuple(n)


def _gen_case(O, key, S, C, N, flags=7, batch=True, base=0, edit=None, edit_nodes=None):
    """Generator scenarios with CYCLE members and cordoned nodes; `edit(s, cont, rng)` may replace the
    container arrays of scenario s, `edit_nodes(s, nodes, rng)` its node arrays.

    The generator's nodes hold about 8 N / C times what its containers ask for, so at these shapes the
    first few hundred nodes would take everything: no container would cross a later link or reach the
    last stage's NOFIT store.  Without `edit_nodes` the free capacities are scaled by C / (12 N), and
    the case asserts (from the oracle's plan) that some containers are NOFIT and that the last group of
    64 nodes is used, so that every stage and link of every geometry carries containers."""
    def make():
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        num, den = min(C, 12 * N), 12 * N  # the scale C / (12 N), at most 1: 12, not 8, so that demand exceeds supply
        conts, nodes, levels = [], [], []
        for s in range(S):
            c, n = O.gen_scenario(SEED + C + N, base + s, C, N, flags)
            c = [np.array(a, np.uint32) for a in c]
            if edit:
                c = edit(s, c, rng)
            conts.append(tuple(c))
            n = [np.array(a) for a in n]
            if edit_nodes:
                n = edit_nodes(s, n, rng)
            else:  # still multiples of 2 and of 64, as the generator's values: the batch packs as it would
                n[0] = (n[0].astype(np.uint64) * num // den // 2 * 2).astype(np.uint32)
                n[1] = (n[1].astype(np.uint64) * num // den // 64 * 64).astype(np.uint32)
            nodes.append(_cordon(rng, n))
            levels.append(_levels(rng, C))
        case = Case(O, conts, nodes, levels, base=base, batch=batch)
        if not edit_nodes:
            for s in range(S):
                node, why = case.e_assign[s * C:(s + 1) * C], case.e_reason[s * C:(s + 1) * C]
                assert int((why == 1).sum()) >= 1, (key, s)
                assert int(node[node != NONE].max()) >= N - 64, (key, s)
        return case
    return _cached(key, make)


def _geo3(geo):
    return geo["groups"], geo["stages"], geo["segments"]


# ---- A. across the 2^21 boundary (no option set: the production path) --------------------------------
A_N = 1300


def _ffd_position(cpu, mem):
    """Rank of every container under (cpu desc, mem desc, index asc), the order of SPEC.md 2.3."""
    C = cpu.size
    order = np.lexsort((np.arange(C), -mem.astype(np.int64), -cpu.astype(np.int64)))
    pos = np.empty(C, np.int64)
    pos[order] = np.arange(C)
    return pos


def _boundary_case(O, C, N=A_N, cordon=0):
    """Hand-built inputs (the generator's late containers are never placed at this size): small demands
    behind 5000 large ones, 1 % requiring a label no node carries (the stage-2 screen), 10 % with a
    conflict bit, 1 % CYCLE; roomy nodes, 3 % cordoned, the first `cordon` of them all cordoned."""
    def make():
        rng = np.random.default_rng(1)
        cpu = rng.integers(1, 9, C)
        mem = rng.integers(0, 4, C)
        cpu[:5000] = rng.integers(100, 4001, 5000)
        mem[:5000] = rng.integers(64, 8001, 5000)
        req = np.where(rng.random(C) < 0.01, 1 << 7, 0)
        conf = np.where(rng.random(C) < 0.10, 1 << rng.integers(0, 32, C), 0)
        level = np.where(rng.random(C) < 0.01, NONE, 0).astype(np.uint32)
        cf = 20000 - rng.integers(0, 500, N)
        sched = (rng.random(N) < 0.97).astype(np.uint8)
        sched[:cordon] = 0
        cont = tuple(a.astype(np.uint32) for a in (cpu, mem, req, conf))
        nodes = (cf.astype(np.uint32), np.full(N, 20000, np.uint32), np.zeros(N, np.uint32),
                 np.zeros(N, np.uint32), sched)
        return Case(O, [cont], [nodes], [level], batch=False)
    return _cached(("boundary", C, N, cordon), make)


def _late_preconditions(case, geo):
    """What makes the sizes past 2^21 a test (conditions on the oracle's plan and the geometry alone): of
    the containers at FFD positions >= 2^21 - 64 -- every position that needs bit 21 among them -- at
    least 100 are placed beyond the first segment, so their position words crossed a global link, at
    least 10 are NOFIT and at least one is CYCLE."""
    cpu, mem = case.conts[0][0], case.conts[0][1]
    late = _ffd_position(cpu, mem) >= P21 - 64
    assert int(late.sum()) == case.C - (P21 - 64)
    node, why = case.e_assign[late], case.e_reason[late]
    first_segment = 64 * geo["groups"] * geo["stages"]
    assert geo["segments"] > 1 and first_segment < case.N, geo
    assert int(((node != NONE) & (node >= first_segment)).sum()) >= 100, (first_segment, geo)
    assert int((why == 1).sum()) >= 10
    assert int((why == 2).sum()) >= 1


@pytest.mark.parametrize("geometry", ["auto", "w1"])
@pytest.mark.parametrize("C", [P21, P21 + 1, P21 + 200])
def test_across_the_2p21_switch(C, geometry, planner, O, opts):
    """One scenario of 2^21, 2^21 + 1 and 2^21 + 200 containers on 1300 nodes, in the automatic geometry
    (narrow: six segments of four one-group stages) and in forced segments of one 4-group stage.  Both
    have their first segment end at node 256; the oracle places the late containers on nodes 256..511."""
    if geometry == "w1":
        opts(pipe_w=1, pipe_seg=4)
    geo = planner.geometry(1, C, A_N)
    assert _geo3(geo) == ((1, 4, 6) if geometry == "auto" else (4, 1, 6)), geo
    case = _boundary_case(O, C)
    if C == P21 + 200:
        _late_preconditions(case, geo)
    case.check(case.run(planner), f"C = 2^21 + {C - P21}, {geometry} geometry")


def test_past_2p21_without_the_screen(planner, O, opts):
    """FP_OPT_SCREEN = 0: the containers the stage-2 screen would reject in segment 0 travel the whole
    pipeline and are stored NOFIT by the last stage, under the wide position mask."""
    C = P21 + 200
    case = _boundary_case(O, C)
    _late_preconditions(case, planner.geometry(1, C, A_N))
    assert int(((case.conts[0][2] != 0) & (case.e_reason == 1)).sum()) >= 1000  # screened with the screen on
    opts(screen=0)
    case.check(case.run(planner), "C = 2^21 + 200, screen = 0")


def test_past_2p21_one_wave_look_ahead(planner, O, opts):
    """Only the 64-thread one-wave kernels (a stage of 12 or more groups) carry the next link slot's
    position words a batch ahead, and 1300 nodes cannot hold two such segments.  The same containers on
    1536 nodes in two one-wave segments of 12 groups, segment 0's 768 nodes cordoned: every container
    crosses the link, the late ones are placed in segment 1."""
    C, N, head = P21 + 200, 1536, 768
    opts(pipe_w=1, pipe_seg=12)
    geo = planner.geometry(1, C, N)
    assert _geo3(geo) == (12, 1, 2), geo
    case = _boundary_case(O, C, N=N, cordon=head)
    _late_preconditions(case, geo)
    placed = case.e_assign[case.e_assign != NONE]
    assert placed.size and int(placed.min()) >= head
    case.check(case.run(planner), "C = 2^21 + 200, one-wave segments")


# ---- B. FP_OPT_KPACK = 0 at small shapes, every producer of s_idx words --------------------------------
def _digit_case(O, values, S=5, C=3000, N=400):
    """At most 256 distinct values per dimension, all below 2^18: the LDS sort's digit path.  The value
    sets are those of test_ffd_sort_key_compression; "packs" keeps every value below 2^15 (packed records)."""
    def make():
        rng = np.random.default_rng(zlib.crc32(values.encode()))
        lim = 1 << 18
        cpu = rng.choice(np.arange(1, 201) * 20, C)
        mem = rng.choice(np.arange(1, 201) * 64, C)
        if values == "all_equal":
            cpu[:] = 700; mem[:] = 900
        elif values == "zero_mix":
            cpu[::3] = 0; mem[::5] = 0
        elif values == "rank_limit":
            cpu[:5] = lim - 1; mem[-5:] = lim - 1
        else:
            assert values == "packs"
        assert np.unique(cpu).size <= 256 and np.unique(mem).size <= 256 and max(cpu.max(), mem.max()) < lim
        conf = ((rng.random(C) < 0.2).astype(np.uint32) << rng.integers(0, 32, C).astype(np.uint32))
        big = 30_000 if values == "packs" else int(max(cpu.max(), mem.max())) * 4 + 10
        nodes = (rng.integers(0, big, N).astype(np.uint32), rng.integers(0, big, N).astype(np.uint32),
                 np.zeros(N, np.uint32), np.zeros(N, np.uint32), (rng.random(N) < 0.95).astype(np.uint8))
        conts = [(np.roll(cpu, 17 * s).astype(np.uint32), np.roll(mem, 17 * s).astype(np.uint32),
                  np.zeros(C, np.uint32), conf) for s in range(S)]
        return Case(O, conts, [nodes] * S, [_levels(rng, C) for _ in range(S)], base=2)
    return _cached(("digits", values, S, C, N), make)


@pytest.mark.parametrize("payload_lds", [None, 0])
@pytest.mark.parametrize("values", ["all_equal", "zero_mix", "rank_limit"])
def test_kpack0_lds_sort_digit_path(values, payload_lds, planner, O, opts):
    """k_scen_sort's digit path writes the position words; k_payload_lds (automatic) or
    k_gather_payload (FP_OPT_PAYLOAD_LDS = 0) adds the skip bit."""
    fixed = {} if payload_lds is None else {"payload_lds": payload_lds}
    _forced_and_auto(planner, opts, _digit_case(O, values), {"kpack": 0}, fixed=fixed)


def test_kpack0_lds_sort_generic_fallback(planner, O, opts):
    """257 distinct cpu values: k_scen_sort's generic fallback writes the position words."""
    dv, S, C, N = 257, 2, 8000, 2000

    def edit(s, c, rng):
        vals = (100 + 20 * np.arange(dv)).astype(np.uint32)
        c[0] = vals[rng.integers(0, dv, C)]
        c[0][:dv] = vals  # every value present in every scenario
        return c

    case = _gen_case(O, ("generic", S, C, N), S, C, N, base=7, edit=edit)
    assert all(np.unique(c[0]).size == dv for c in case.conts)
    _forced_and_auto(planner, opts, case, {"kpack": 0})


def test_kpack0_radix_single_scenario(planner, O, opts):
    """FP_OPT_SCEN_SORT = 0, one scenario: the device-wide radix sort and k_gather_sorted."""
    case = _gen_case(O, ("radix1", 3000, 300), 1, 3000, 300, flags=7, batch=False)
    _forced_and_auto(planner, opts, case, {"kpack": 0}, fixed={"scen_sort": 0})


def test_kpack0_radix_segmented(planner, O, opts):
    """FP_OPT_SCEN_SORT = 0, three scenarios: the segmented radix sort and k_gather_sorted."""
    case = _gen_case(O, ("radix3", 4000, 700), 3, 4000, 700, base=4)
    _forced_and_auto(planner, opts, case, {"kpack": 0}, fixed={"scen_sort": 0})


# the forced geometries of tests/test_gpu_parity.py, and what fp_pipe_plan makes of them for 2561 nodes
# (41 groups) and 641 nodes (11 groups); 64 nodes are one group, one stage, one segment in every one
GEOMETRIES = {"wide": (4, 40), "narrow": (4, 4), "one-stage": (1, 16), "one-wave": (1, 32), "one-wave-40": (1, 40)}
SERVED = {("wide", 2561): (6, 4, 2), ("narrow", 2561): (1, 4, 11), ("one-stage", 2561): (16, 1, 3),
          ("one-wave", 2561): (24, 1, 2), ("one-wave-40", 2561): (24, 1, 2),
          ("wide", 641): (3, 4, 1), ("narrow", 641): (1, 4, 3), ("one-stage", 641): (11, 1, 1),
          ("one-wave", 641): (11, 1, 1), ("one-wave-40", 641): (11, 1, 1)}


@pytest.mark.parametrize("C,N", [(4000, 641), (7000, 2561), (64, 64)])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_kpack0_geometries(geometry, C, N, planner, O, opts):
    """Multi-stage segments (LDS rings carry the s_idx word), one-wave segments (the link look-ahead)
    and segments over unbounded and bounded links, each searching the buckets per stage."""
    w, seg = GEOMETRIES[geometry]
    case = _gen_case(O, ("geom", C, N), 1, C, N, flags=7, batch=False)
    opts(pipe_w=w, pipe_seg=seg)
    assert _geo3(planner.geometry(1, C, N)) == SERVED.get((geometry, N), (1, 1, 1)), planner.geometry(1, C, N)
    _forced_and_auto(planner, opts, case, {"kpack": 0})


def test_kpack0_six_wave_kernel(planner, O, opts):
    """4096 scenarios of 256 containers on 1536 nodes: two one-wave segments of 12 groups per scenario,
    phased over unbounded links -- the six-wave kernel.  All 4096 plans and costs against the oracle.
    The generator's nodes would take every container in segment 0 (the link would carry END alone): free
    capacities are a twentieth here and 70 % of segment 0's nodes cordoned, so that every scenario sends
    more than one slot of 64 containers over its link, to be placed in segment 1 or found NOFIT there."""
    S, C, N, head = 4096, 256, 1536, 768
    geo = planner.geometry(S, C, N)
    assert _geo3(geo) == (12, 1, 2) and geo["bounded"] == 0, geo
    assert 64 * geo["groups"] * geo["stages"] == head

    def edit_nodes(s, n, rng):
        n[0] //= 20
        n[1] //= 20
        n[4][:head] &= (rng.random(head) >= 0.7).astype(np.uint8)
        return n

    case = _gen_case(O, ("six-wave", S, C, N), S, C, N, base=100, edit_nodes=edit_nodes)
    beyond = ((case.e_assign != NONE) & (case.e_assign >= head)).reshape(S, C).sum(axis=1)
    nofit = (case.e_reason == 1).reshape(S, C).sum(axis=1)
    assert int((beyond + nofit).min()) > 64, int((beyond + nofit).min())
    assert int(beyond.sum()) >= S * C // 10 and int(nofit.sum()) >= S * C // 10, (int(beyond.sum()), int(nofit.sum()))
    _forced_and_auto(planner, opts, case, {"kpack": 0})


@pytest.mark.parametrize("packed", [0, None])
def test_kpack0_record_kinds(packed, planner, O, opts):
    """k_ffd_pipe<..., PK> both ways with the buckets searched per stage: values that pack run the u32
    records under FP_OPT_PACKED = 0 (record kind 1) and the packed ones otherwise (kind 2)."""
    fixed = {} if packed is None else {"packed": packed}
    _forced_and_auto(planner, opts, _digit_case(O, "packs"), {"kpack": 0}, fixed=fixed)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == (packed is None), path


# ---- C. ring depth, flush mask, priority, systolic extra ----------------------------------------------
def _batch_1500(O):
    return _gen_case(O, ("batch", 5, 3000, 1500), 5, 3000, 1500, base=7)


@pytest.mark.parametrize("depth", [2, 3, 5, 6])
@pytest.mark.parametrize("w,seg,C,N", [(4, 4, 7000, 2561), (4, 4, 64, 64), (4, 40, 7000, 2561)])
def test_pipe_r_ring_depths(w, seg, C, N, depth, planner, O, opts):
    """LDS rings of 2, 3, 5 and 6 slots between the stages of a segment (the automatic choice is 2..4; a
    stage's control block holds six slot counts).  pipe_geom keeps the automatic depth where the rings
    would not fit LDS: such a combination is skipped, not asserted around."""
    case = _gen_case(O, ("geom", C, N), 1, C, N, flags=7, batch=False)

    def served():
        geo = planner.geometry(1, C, N)
        if geo["ring"] != depth:
            pytest.skip(f"ring depth {depth} not served for {geo}")
        if N == 2561:
            assert geo["stages"] == 4, geo  # three LDS rings per segment

    _forced_and_auto(planner, opts, case, {"pipe_r": depth}, fixed={"pipe_w": w, "pipe_seg": seg}, served=served)


def test_pipe_r_depth_6_batch(planner, O, opts):
    """Five scenarios in the automatic (narrow, four-stage) geometry over six-slot rings."""
    case = _batch_1500(O)

    def served():
        geo = planner.geometry(case.S, case.C, case.N)
        assert geo["ring"] == 6 and geo["stages"] == 4, geo

    _forced_and_auto(planner, opts, case, {"pipe_r": 6}, served=served)


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
@pytest.mark.parametrize("w,seg", [(4, 4), (1, 12)])
def test_pipe_flush_bounded_links(w, seg, mask, planner, O, opts):
    """Idle flushes off and on over 8-slot bounded links: without bit 1 a consumer publishes its tail
    every four slots and the producer never publishes a partial slot before the end of its stream."""
    S, C, N = 4, 12_000, 6_000
    case = _gen_case(O, ("small-ring", S, C, N), S, C, N, base=3)
    fixed = {"link_slots": 8, "pipe_w": w, "pipe_seg": seg}

    def served():
        geo = planner.geometry(S, C, N)
        assert geo["bounded"] == 1 and geo["link_slots"] == 8, geo

    _forced_and_auto(planner, opts, case, {"pipe_flush": mask}, fixed=fixed, served=served)


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_pipe_flush_unbounded_multi_stage(mask, planner, O, opts):
    """Two segments of four 6-group stages over an unbounded link: only bit 0 (the LDS rings) acts."""
    C, N = 7000, 2561
    case = _gen_case(O, ("geom", C, N), 1, C, N, flags=7, batch=False)

    def served():
        geo = planner.geometry(1, C, N)
        assert _geo3(geo) == (6, 4, 2) and geo["bounded"] == 0, geo

    _forced_and_auto(planner, opts, case, {"pipe_flush": mask}, fixed={"pipe_w": 4, "pipe_seg": 40}, served=served)


@pytest.mark.parametrize("prio", [0, 1, 2])
def test_pipe_prio_narrow_single_scenario(prio, planner, O, opts):
    C, N = 20_000, 6_000
    case = _gen_case(O, ("geom", C, N), 1, C, N, flags=7, batch=False)
    assert _geo3(planner.geometry(1, C, N)) == (1, 4, 24)
    _forced_and_auto(planner, opts, case, {"pipe_prio": prio})


@pytest.mark.parametrize("prio", [0, 1, 2])
def test_pipe_prio_one_wave_batch(prio, planner, O, opts):
    case = _batch_1500(O)

    def served():
        assert _geo3(planner.geometry(case.S, case.C, case.N)) == (12, 1, 2)

    _forced_and_auto(planner, opts, case, {"pipe_prio": prio}, fixed={"pipe_w": 1, "pipe_seg": 12}, served=served)


def _label_only_case(O, n_lab=64, N=5):
    """The batch of test_label_only_containers_count_their_node: n_lab label-only containers fit only
    node 3, which nothing else uses; the packed cost must count that node."""
    def make():
        S, k = 3, 20
        conts, nodes = [], []
        for s in range(S):
            cont = ([5 + s] * k + [0] * n_lab, [7] * k + [0] * n_lab, [0] * k + [1 << 4] * n_lab, [0] * (k + n_lab))
            conts.append(tuple(np.array(x, np.uint32) for x in cont))
            lab = np.zeros(N, np.uint32)
            lab[3] = 1 << 4
            nodes.append((np.full(N, 1000, np.uint32), np.full(N, 1000, np.uint32), lab, np.zeros(N, np.uint32),
                          np.ones(N, np.uint8)))
        case = Case(O, conts, nodes, [np.zeros(k + n_lab, np.uint32)] * S, base=11)
        assert all(3 in set(case.e_assign[s * case.C:(s + 1) * case.C].tolist()) for s in range(S))
        return case
    return _cached(("label-only", n_lab, N), make)


# (C, N, flags, pipe_w, pipe_seg): the two smallest shapes of test_systolic_fill_vs_oracle -- the second
# has one 11-group stage, where the systolic loop is not compiled and the option must change nothing --
# and its first one, narrow stages with long queues
SYSTOLIC_SHAPES = [(64, 64, 7, 4, 4), (4_000, 641, 7, 1, 12), (20_000, 6_000, 7, 4, 4)]


@pytest.mark.parametrize("valu", [0, 1, 2])
@pytest.mark.parametrize("thr", [1, 24])
@pytest.mark.parametrize("extra", [0, 1, 128, 1000])
def test_systolic_extra(extra, thr, valu, planner, O, opts):
    """The systolic fill's steps past the queue length: 0 hands every container the systolic loop leaves
    open to the serial finish, 128 is the clamp and 1000 is clamped to it (the value shares a 16-bit field
    with the step-loop flags).  Every step loop (FP_OPT_SYSTOLIC_VALU), every queue (threshold 1) and
    queues of at least 24."""
    forced = {"systolic_extra": extra}
    for C, N, flags, w, seg in SYSTOLIC_SHAPES:
        case = _gen_case(O, ("geom", C, N), 1, C, N, flags=flags, batch=False)
        fixed = {"systolic": thr, "systolic_valu": valu, "pipe_w": w, "pipe_seg": seg}

        def served():
            geo = planner.geometry(1, C, N)
            assert geo["systolic"] == (thr if geo["groups"] <= 4 else 0), geo
            assert (geo["groups"] <= 4) == (N != 641), geo

        _forced_and_auto(planner, opts, case, forced, fixed=fixed, served=served)
        opts(systolic_extra=-1, pipe_w=-1, pipe_seg=-1)  # FP_OPT_AUTO again for the next automatic run
    # the touched bookkeeping after the serial finish, through the packed cost's n_nodes_used
    _forced_and_auto(planner, opts, _label_only_case(O), forced, fixed={"systolic": thr, "systolic_valu": valu})
