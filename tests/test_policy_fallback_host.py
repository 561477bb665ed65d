"""CPU tests of the fallback chain (SPEC.md 2.8): the two statements of the numpy reference
(tests/policy_fallback_ref.py) against each other, against SPEC.md 2.7 and by hand, and the front ends
that carry a FallbackPolicy (KDL, registry, plan_stage's masks, dry-run output)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_cases as K  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_ref as R  # noqa: E402
import policy_spread_ref as SR  # noqa: E402

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """(assign, reason, hops, nodes_after, count) twice."""
    assert all(np.array_equal(a[i], b[i]) for i in (0, 1, 2, 4))
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


# ---- the two statements of the reference ------------------------------------------------------------------
# the GPU tests' inputs (tests/test_gpu_policy_fallback.py): every shape under four hops, the shapes with a
# spread under two
@pytest.mark.parametrize("C,N", [(300, 1), (300, 64), (300, 65), (2000, 1024), (300, 2049), (2000, 4096), (2000, 8192)])
def test_iterative_and_per_node_statements_agree(C, N):
    cont, nodes = K.crafted(C, N)
    strategy = (C + N) % 4  # each strategy on at least one shape; the small shapes below take all four
    got = FR.place_per_node(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), relax_mask=K.RELAX[4])
    _same(got, K.expected(C, N, strategy, 4))


@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("n_hops", [1, 2, 4])
def test_statements_agree_on_the_small_shapes(strategy, n_hops):
    for C, N in ((300, 64), (300, 65)):
        cont, nodes = K.crafted(C, N)
        _same(FR.place_per_node(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), relax_mask=K.RELAX[n_hops]),
              K.expected(C, N, strategy, n_hops))
    # under a spread: a pool whose fitting nodes all fail the skew test counts as dry
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    got = FR.place_per_node(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), relax_mask=K.RELAX[2],
                            domain=K.spread_domain(N), max_skew=2)
    _same(got, K.expected(C, N, strategy, 2, True))


@pytest.mark.parametrize("C,N", [(300, 64), (2000, 1024), (2000, 8192)])
def test_statements_agree_under_a_spread(C, N):
    cont, nodes = K.crafted(C, N)
    strategy = (C + N + 1) % 4
    got = FR.place_per_node(cont, nodes, strategy, node_count=np.zeros(N, np.uint32), relax_mask=K.RELAX[2],
                            domain=K.spread_domain(N), max_skew=2)
    exp = K.expected(C, N, strategy, 2, True)
    _same(got, exp)
    assert (exp[1] == SR.REASON_SKEW).sum() >= 140 and (exp[2] >= 1).sum() >= 25


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_no_hops_is_section_2_7(strategy):
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    rng = np.random.default_rng(5)
    cnt0 = rng.integers(0, 4, N).astype(np.uint32)
    level = np.where(rng.random(C) < 0.1, NONE, 0).astype(np.uint32)
    for kw in (dict(domain=K.spread_domain(N), max_skew=2), {}):
        exp = SR.place(cont, nodes, strategy, preferred=0b10010000, level=level, node_count=cnt0, **kw)
        for place in (FR.place, FR.place_per_node):
            got = place(cont, nodes, strategy, preferred=0b10010000, level=level, node_count=cnt0,
                        relax_mask=[0xFFFFFFFF] * 4, n_hops=0, **kw)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and not got[2].any()
            assert np.array_equal(got[4], exp[3]) and all(np.array_equal(x, y) for x, y in zip(got[3], exp[2]))
    # and a chain changes the plan on these inputs
    assert (K.expected(C, N, strategy, 2)[0] != K.expected(C, N, strategy, 0)[0]).sum() >= 80


# ---- by hand ----------------------------------------------------------------------------------------------
def test_closed_form_on_the_reference():
    N = 64
    cont, nodes = K.closed_form(N)
    q, i = N // 4, np.arange(N)
    k = 4 * np.arange(q)
    for place in (FR.place, FR.place_per_node):
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[K.CLASS, K.REGION])
        assert np.array_equal(a, np.concatenate([k, k + 1, np.sort(np.concatenate([k + 2, k + 3]))]))
        assert (r == 0).all() and np.array_equal(h, np.repeat([0, 1, 2], [q, q, 2 * q]))
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[K.CLASS])
        assert np.array_equal(a[:2 * q], np.concatenate([k, k + 1])) and (r[2 * q:] == 1).all() and (h[2 * q:] == 0).all()
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[K.REGION])
        assert np.array_equal(a[:2 * q], np.concatenate([k, k + 2])) and (r[2 * q:] == 1).all()
        dom = (i % 4).astype(np.uint32)
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[K.CLASS, K.REGION], domain=dom, max_skew=1)
        assert np.array_equal(a, i) and np.array_equal(h, np.array([0, 1, 2, 2])[i % 4])  # the skew test forces the hop
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[K.CLASS], domain=dom, max_skew=1)
        assert (a != NONE).sum() == 2 and (r == SR.REASON_SKEW).sum() == N - 2


def test_overlapping_and_zero_masks_and_cost():
    nodes = (np.full(3, 10, np.uint32), np.full(3, 10, np.uint32), np.array([0b0101, 0b0110, 0b1000], np.uint32),
             np.zeros(3, np.uint32), np.ones(3, np.uint8))
    cont = (np.full(4, 10, np.uint32), np.ones(4, np.uint32), np.full(4, 0b0101, np.uint32), np.zeros(4, np.uint32))
    # hop 1 gives nothing up, hop 2 bit 0 (node 1 matches), hop 3 bits 0 and 2 again plus bit 1 (node 2 matches)
    for place in (FR.place, FR.place_per_node):
        a, r, h, _, _ = place(cont, nodes, R.FIRST_FIT, relax_mask=[0, 0b0001, 0b0111])
        assert a.tolist() == [0, 1, 2, NONE] and h.tolist() == [0, 2, 3, 0] and r.tolist() == [0, 0, 0, 1]
    assert FR.cost(a, r, 9) == (1 << 40) | (3 << 16) | 9  # a relaxed placement counts as placed
    assert FR.cumulative([0, 1, 7], 3) == [0, 0, 1, 7]


# ---- the ABI's names --------------------------------------------------------------------------------------
def test_header_binding_and_reference_agree():
    from fleetflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    assert f"#define FP_FALLBACK_MAX_HOPS {_lib.FP_FALLBACK_MAX_HOPS}" in hdr
    assert _lib.FP_FALLBACK_MAX_HOPS == FR.MAX_HOPS == 4 and "#define FP_ABI_VERSION 1" in hdr
    for name in ("fp_place_policy_fallback", "fp_place_batch_policy_fallback", "fp_dev_place_batch_policy_fallback"):
        assert f"int {name}(fp_ctx *ctx" in hdr and name in _lib.SIGNATURES
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    assert "pub const FP_FALLBACK_MAX_HOPS: u32 = 4;" in ffi and "pub fn fp_place_policy_fallback(" in ffi


# ---- the policy model -------------------------------------------------------------------------------------
def test_fallback_property_and_active():
    from fleetflow_amd.flow import PlacementPolicy
    P = PlacementPolicy
    assert P().fallback == () and not P().active
    assert P(fallback_relax_order=("class", "region")).fallback == ("class", "region")
    assert P(fallback_relax_order=["class", "region"], fallback_max_hops=1).fallback == ("class",)
    assert P(fallback_relax_order=("class",), fallback_max_hops=7).fallback == ("class",)
    assert P(fallback_relax_order=("class",)).active and P(fallback_relax_order=("class",), fallback_max_hops=1).active
    assert not P(fallback_relax_order=("class",), fallback_max_hops=0).active
    assert not P(fallback_max_hops=2).active
    five = ("a", "b", "c", "d", "e")
    assert P(fallback_relax_order=five, fallback_max_hops=4).fallback == five[:4]
    for kw in (dict(fallback_relax_order=five), dict(fallback_relax_order=five, fallback_max_hops=5),
               dict(fallback_relax_order=("class",), fallback_max_hops=-1), dict(fallback_relax_order=("class",), fallback_max_hops=1.0),
               dict(fallback_relax_order=("class",), fallback_max_hops="1"), dict(fallback_relax_order=("class",), fallback_max_hops=True),
               dict(fallback_relax_order=("class=gpu",))):
        with pytest.raises(ValueError):
            P(**kw)
    # the chain takes no part in ==, like the spread constraint
    assert P("fill_lowest", fallback_relax_order=("class",)) == P("fill_lowest")


def test_label_dict_key_mask():
    from fleetflow_amd.flow import LabelDict
    ld = LabelDict(["class=gpu", "class=cpu", "region=tokyo", "classy=x", "arch=amd64"])
    # sorted: arch=amd64 0, class=cpu 1, class=gpu 2, classy=x 3, region=tokyo 4
    assert ld.key_mask("class") == 0b00110 and ld.key_mask("classy") == 0b01000 and ld.key_mask("region") == 0b10000
    assert ld.key_mask("zone") == 0 and ld.key_mask("") == 0
    assert ld.key_mask("class") == ld.mask(["class=gpu", "class=cpu"])


# ---- KDL `fallback` child of `placement` ------------------------------------------------------------------
KDL = """
project "demo"
server "n0" { capacity cpu=4000 memory=8192; label "region=osaka" }
service "a" { resources cpu=500 memory=512 }
stage "live" {
    service "a"
    server "n0"
    %s
}
"""


def test_kdl_fallback_node():
    from fleetflow_amd.parser import FlowError, parse_kdl_string
    pol = parse_kdl_string(KDL % 'placement strategy="fill_lowest" { spread "region" max-skew=1; fallback "class" "region" max-hops=2 }'
                           ).stages["live"].placement
    assert (pol.strategy, pol.spread, pol.fallback_relax_order, pol.fallback_max_hops, pol.fallback) == (
        "fill_lowest", ("region", 1), ("class", "region"), 2, ("class", "region"))
    pol = parse_kdl_string(KDL % 'placement { fallback "class" "region" "arch" max-hops=1 }').stages["live"].placement
    assert (pol.strategy, pol.fallback_max_hops, pol.fallback, pol.active) == (None, 1, ("class",), True)
    pol = parse_kdl_string(KDL % 'placement { fallback "class" }').stages["live"].placement
    assert (pol.fallback_max_hops, pol.fallback) == (None, ("class",))
    pol = parse_kdl_string(KDL % 'placement { fallback "class" max-hops=0 }').stages["live"].placement
    assert pol.fallback == () and not pol.active
    # without the child nothing changes
    pol = parse_kdl_string(KDL % 'placement strategy="fill_lowest"').stages["live"].placement
    assert pol.fallback == () and pol.fallback_relax_order == () and pol.fallback_max_hops is None
    for bad in ('fallback', 'fallback max-hops=2', 'fallback "class" max-hops=-1', 'fallback "class" max-hops="2"',
                'fallback "class" max-hops=1.5', 'fallback "class=gpu"', 'fallback 3', 'fallback "class" "class"',
                'fallback "a" "b" "c" "d" "e"', 'fallback "a" "b" "c" "d" "e" max-hops=5', 'fallback "class" hops=2',
                'fallback ""'):
        with pytest.raises(FlowError):
            parse_kdl_string(KDL % ("placement { %s }" % bad))
    # five keys are fine when max-hops keeps the chain at four
    pol = parse_kdl_string(KDL % 'placement { fallback "a" "b" "c" "d" "e" max-hops=4 }').stages["live"].placement
    assert pol.fallback == ("a", "b", "c", "d")


def test_registry_reads_the_fallback_policy():
    from fleetflow_amd.registry import placement_policy
    row = {"placement_policy": {"strategy": "pack_into_dedicated", "spread_constraint": {"topology_key": "region", "max_skew": 2},
                                "fallback_policy": {"relax_order": ["class", "region"], "max_hops": 2}}}
    pol = placement_policy(row)
    assert (pol.strategy, pol.spread, pol.fallback_relax_order, pol.fallback_max_hops, pol.fallback) == (
        "pack_into_dedicated", ("region", 2), ("class", "region"), 2, ("class", "region"))
    pol = placement_policy({"placement_policy": {"fallback_policy": {"relax_order": ["class", "region"], "max_hops": 1}}})
    assert pol.strategy is None and pol.fallback == ("class",) and pol.active
    assert placement_policy({"placement_policy": {"fallback_policy": {"relax_order": ["class"]}}}).fallback == ("class",)
    assert placement_policy({"placement_policy": {"fallback_policy": None}}).fallback == ()
    assert placement_policy({"placement_policy": {"fallback_policy": {"relax_order": [], "max_hops": 2}}}).fallback == ()
    assert placement_policy({"placement_policy": {"tier": "free"}}).fallback == ()
    five = ["a", "b", "c", "d", "e"]
    assert placement_policy({"placement_policy": {"fallback_policy": {"relax_order": five, "max_hops": 4}}}).fallback == tuple(five[:4])
    for fb in ({"relax_order": ["class"], "max_hops": -1}, {"relax_order": five, "max_hops": 5}, {"relax_order": five},
               {"relax_order": ["class"], "max_hops": "2"}, {"relax_order": ["class"], "max_hops": 1.5},
               {"relax_order": "class"}, {"relax_order": [1, 2]}, "class", ["class", "region"], 2):
        with pytest.raises(ValueError):
            placement_policy({"placement_policy": {"fallback_policy": fb}})


# ---- plan_stage's masks and the plan's record ---------------------------------------------------------------
class _StubPlanner:
    """plan_stage's planner calls, answered by the numpy references: no library, no GPU."""

    def __init__(self):
        self.calls = []

    def plan_stage(self, row_ptr, col, has_deps, cont, ntab):
        v = len(has_deps)
        a, r, _, _ = R.place(cont, ntab, R.FIRST_FIT)
        return (np.arange(v, dtype=np.uint32), np.zeros(v, np.uint32), np.arange(v, dtype=np.uint32), 0,
                (np.zeros(v, np.uint32), np.full(v, len(ntab[0]), np.uint32), a, r, None))

    def place_policy(self, cont, nodes, strategy, preferred=0, level=None, node_count=None, *, domain=None, max_skew=0):
        self.calls.append(("place_policy", None))
        return SR.place(cont, nodes, strategy, preferred=preferred, level=level, domain=domain, max_skew=max_skew)

    def place_policy_fallback(self, cont, nodes, strategy, relax_mask, preferred=0, level=None, node_count=None, *,
                              domain=None, max_skew=0):
        self.calls.append(("place_policy_fallback", dict(relax_mask=list(relax_mask), domain=domain, max_skew=max_skew)))
        return FR.place(cont, nodes, strategy, preferred=preferred, level=level, domain=domain, max_skew=max_skew,
                        relax_mask=list(relax_mask))


STAGE = """
project "demo"
server "g0" { capacity cpu=1000 memory=8192; label "class=gpu"; label "region=tokyo" }
server "c0" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=tokyo" }
server "c1" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=osaka" }
service "train" { resources cpu=900 memory=64; require "class=gpu" "region=tokyo" }
service "infer" { resources cpu=800 memory=64; require "class=gpu" "region=tokyo" }
service "batch" { resources cpu=700 memory=64; require "class=tpu" "region=nagoya" }
service "web" { resources cpu=100 memory=64; require "region=osaka" }
stage "live" {
    service "train"
    service "infer"
    service "batch"
    service "web"
    server "g0"
    server "c0"
    server "c1"
    %s
}
"""


def test_plan_stage_builds_the_masks_and_records_what_was_relaxed():
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    flow = parse_kdl_string(STAGE % 'placement { fallback "class" "region" "zone" }')
    stub = _StubPlanner()
    plan = plan_stage(flow, "live", stub)
    (name, call), = stub.calls
    # sorted dictionary: class=cpu 0, class=gpu 1, class=tpu 2, region=nagoya 3, region=osaka 4, region=tokyo 5
    assert name == "place_policy_fallback" and call["relax_mask"] == [0b000111, 0b111000, 0] and call["domain"] is None
    # train takes the gpu server; infer gives class up and stays in tokyo; batch gives both up (first fit: g0 has
    # 100 left, so c0); web matches c1 as it is
    assert plan.assignment == {"train": "g0", "infer": "c0", "batch": "c0", "web": "c1"} and plan.rejected == {}
    assert plan.relaxed == {"infer": ["class"], "batch": ["class", "region"]}
    assert (plan.fallback_relax_order, plan.fallback_max_hops) == (["class", "region", "zone"], None)
    text = format_up_dry_run(flow, "live", plan)
    assert "  配置フォールバック: class → region → zone\n" in text and "  配置戦略: first_fit\n" in text
    assert "    配置先: c0 (緩和: class)\n" in text and "    配置先: c0 (緩和: class, region)\n" in text
    assert "    配置先: g0\n" in text and "    配置先: c1\n" in text
    js = plan_to_json(plan)
    assert '"fallback": {"relax_order": ["class", "region", "zone"], "max_hops": null}' in js
    assert '"relaxed": {"infer": ["class"], "batch": ["class", "region"]}' in js
    assert plan_from_json(js) == plan
    # max-hops=1: batch may only give its class up, and no server is in nagoya
    flow1 = parse_kdl_string(STAGE % 'placement { fallback "class" "region" max-hops=1 }')
    stub = _StubPlanner()
    plan1 = plan_stage(flow1, "live", stub)
    assert stub.calls[0][1]["relax_mask"] == [0b000111]
    assert plan1.rejected == {"batch": "NOFIT"} and plan1.relaxed == {"infer": ["class"]}
    assert "  配置フォールバック: class → region (max_hops=1)\n" in format_up_dry_run(flow1, "live", plan1)
    assert '"max_hops": 1' in plan_to_json(plan1) and plan_from_json(plan_to_json(plan1)) == plan1
    # with a spread beside it the new entry still takes the call, with the domains
    flow2 = parse_kdl_string(STAGE % 'placement { spread "region" max-skew=2; fallback "class" }')
    stub = _StubPlanner()
    plan2 = plan_stage(flow2, "live", stub)
    assert stub.calls[0][0] == "place_policy_fallback" and stub.calls[0][1]["domain"] == [0, 0, 1] and stub.calls[0][1]["max_skew"] == 2
    assert plan2.spread_topology_key == "region" and plan2.fallback_relax_order == ["class"]
    # a chain of no hops, or none: the existing entry, nothing recorded
    for placement in ('placement { prefer "region=tokyo"; fallback "class" max-hops=0 }', 'placement { prefer "region=tokyo" }'):
        stub = _StubPlanner()
        plan0 = plan_stage(parse_kdl_string(STAGE % placement), "live", stub)
        assert [c[0] for c in stub.calls] == ["place_policy"]
        assert plan0.fallback_relax_order == [] and plan0.relaxed == {} and "fallback" not in plan_to_json(plan0)


def test_plan_output_without_a_fallback_is_unchanged():
    from fleetflow_amd.flow import Flow, Plan, Service, Stage
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    base = ("live", ["a"], {"a": 0}, ["a"], {"a": "n1"}, {}, {"a": (2, "n0")})
    plain, scored = Plan(*base), Plan(*base, "fill_lowest", ["region=tokyo"], "zone", 2)
    # byte for byte what the output was before the chain existed
    assert plan_to_json(plain) == ('{"stage": "live", "order": ["a"], "levels": {"a": 0}, "level_order": ["a"], '
                                   '"assign": {"a": "n1"}, "rejected": {}, "candidates": {"a": {"count": 2, "first": "n0"}}}')
    assert plan_to_json(scored) == plan_to_json(plain)[:-1] + (
        ', "placement": {"strategy": "fill_lowest", "preferred": ["region=tokyo"], '
        '"spread": {"topology_key": "zone", "max_skew": 2}}}')
    assert plan_from_json(plan_to_json(scored)) == scored and plan_from_json(plan_to_json(plain)) == plain
    flow = Flow(name="demo", services={"a": Service(image="img")}, stages={"live": Stage(services=["a"])})
    text = format_up_dry_run(flow, "live", scored)
    assert "フォールバック" not in text and "緩和" not in text and "    配置先: n1\n" in text
    assert text.count("\n") == format_up_dry_run(flow, "live", plain).count("\n") + 2  # the strategy and the spread line
    # with a chain: the line, the mark and the JSON fields, and a different plan
    chain = Plan(*base, None, [], None, None, ["class"], 3, {"a": ["class"]})
    assert chain != plain and plan_from_json(plan_to_json(chain)) == chain
    text = format_up_dry_run(flow, "live", chain)
    assert "  配置戦略: first_fit\n  配置フォールバック: class (max_hops=3)\n" in text and "    配置先: n1 (緩和: class)\n" in text
