"""CPU tests of the hard topology spread (SPEC.md 2.7): the numpy reference (tests/policy_spread_ref.py)
against SPEC.md 2.6 and by hand, and the front ends that carry a SpreadConstraint (KDL, registry,
plan_stage's domain derivation, dry-run output)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import policy_spread_ref as SR  # noqa: E402

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_scenario(seed, C, N, D):
    rng = np.random.default_rng(seed)
    cont = (rng.integers(1, 40, C).astype(np.uint32) * 50, rng.integers(1, 30, C).astype(np.uint32) * 64,
            (1 << rng.integers(0, 4, C)).astype(np.uint32) * (rng.random(C) < 0.3), np.zeros(C, np.uint32))
    nodes = (rng.integers(20, 200, N).astype(np.uint32) * 50, rng.integers(20, 200, N).astype(np.uint32) * 64,
             rng.integers(0, 16, N).astype(np.uint32), np.zeros(N, np.uint32), (rng.random(N) < 0.9).astype(np.uint8))
    return cont, nodes, rng.integers(0, D, N).astype(np.uint32)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for i in range(5):
        assert np.array_equal(a[2][i], b[2][i])


# ---- the reference against SPEC.md 2.6 --------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("max_skew", [0, 0xFFFFFFFF])
def test_no_constraint_is_section_2_6(strategy, max_skew):
    cont, nodes, dom = _random_scenario(11, 200, 37, 5)
    cnt0 = np.random.default_rng(3).integers(0, 5, 37).astype(np.uint32)
    level = np.where(np.random.default_rng(4).random(200) < 0.1, NONE, 0).astype(np.uint32)
    exp = R.place(cont, nodes, strategy, preferred=0b1010, level=level, node_count=cnt0)
    got = SR.place(cont, nodes, strategy, preferred=0b1010, level=level, node_count=cnt0, domain=dom, max_skew=max_skew)
    _same(got, exp)
    # and a constraint that binds changes the plan on these inputs
    tight = SR.place(cont, nodes, strategy, preferred=0b1010, level=level, node_count=cnt0, domain=dom, max_skew=1)
    assert (tight[0] != exp[0]).sum() > 20


# ---- by hand ------------------------------------------------------------------------------------------
def _nodes(cf, sched=None):
    n = len(cf)
    return (np.array(cf, np.uint32), np.full(n, 1000, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
            np.array(sched if sched is not None else [1] * n, np.uint8))


def _cont(cpu):
    c = len(cpu)
    return (np.array(cpu, np.uint32), np.ones(c, np.uint32), np.zeros(c, np.uint32), np.zeros(c, np.uint32))


def test_skew_against_nofit():
    """Domain 1 is one schedulable node without room: it is eligible, stays at zero and holds the
    minimum down.  The container nothing fits is NOFIT, the ones only domain 0 fits are SKEW."""
    a, r, after, cnt = SR.place(_cont([10, 10, 10, 1000]), _nodes([100, 0]), R.FIRST_FIT, domain=[0, 1], max_skew=1)
    assert a.tolist() == [0, NONE, NONE, NONE] and r.tolist() == [0, 3, 3, 1]
    assert after[0].tolist() == [90, 0] and cnt.tolist() == [1, 0]
    assert SR.cost(a, r, 5) == (3 << 40) | (1 << 16) | 5  # SKEW counts as rejected
    a, r, _, _ = SR.place(_cont([10, 10, 10, 1000]), _nodes([100, 0]), R.FIRST_FIT, domain=[0, 1], max_skew=2)
    assert a.tolist() == [0, 0, NONE, NONE] and r.tolist() == [0, 0, 3, 1]


def test_an_ineligible_domain_does_not_hold_the_minimum_down():
    cont = _cont([10, 10, 10, 10])
    # domain 2's only node is cordoned: not eligible, the other two alternate
    a, r, _, _ = SR.place(cont, _nodes([100, 100, 100], [1, 1, 0]), R.FIRST_FIT, domain=[0, 1, 2], max_skew=1)
    assert a.tolist() == [0, 1, 0, 1] and r.tolist() == [0, 0, 0, 0]
    # schedulable but full: eligible whatever the container (the stated simplification), so it binds
    a, r, _, _ = SR.place(cont, _nodes([100, 100, 0], [1, 1, 1]), R.FIRST_FIT, domain=[0, 1, 2], max_skew=1)
    assert a.tolist() == [0, 1, NONE, NONE] and r.tolist() == [0, 0, 3, 3]


def test_entry_counts_come_from_node_count():
    a, r, _, cnt = SR.place(_cont([10, 10, 10]), _nodes([100, 100]), R.FIRST_FIT, node_count=[2, 0], domain=[0, 1],
                            max_skew=1)
    assert a.tolist() == [1, 1, 0] and r.tolist() == [0, 0, 0] and cnt.tolist() == [3, 2]
    # two nodes of one domain add up: domain 0 enters at 1 + 1
    a, _, _, _ = SR.place(_cont([10, 10, 10]), _nodes([100, 100, 100]), R.FIRST_FIT, node_count=[1, 1, 0],
                          domain=[0, 0, 1], max_skew=1)
    assert a.tolist() == [2, 2, 0]
    # u32 counts wrap: 0xFFFFFFFF + 1 = 0 makes domain 0 the minimum, and domain 1 is 0xFFFFFFFF above it
    a, r, _, cnt = SR.place(_cont([10, 10]), _nodes([100, 100]), R.SPREAD, node_count=[0xFFFFFFFF, 0xFFFFFFFF],
                            domain=[0, 1], max_skew=1)
    assert a.tolist() == [0, 0] and r.tolist() == [0, 0] and cnt.tolist() == [1, 0xFFFFFFFF]


def test_a_cycle_container_leaves_the_counts_alone():
    trace = []
    a, r, _, cnt = SR.place(_cont([30, 20, 10]), _nodes([100, 100]), R.FIRST_FIT, level=[NONE, 0, 0], domain=[0, 1],
                            max_skew=1, trace=trace)
    assert a.tolist() == [NONE, 0, 1] and r.tolist() == [2, 0, 0] and cnt.tolist() == [1, 1]
    assert [t[0][:2].tolist() for t in trace] == [[1, 0], [1, 1]]


@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("max_skew", [1, 2, 5])
def test_invariant_skew_never_exceeded(strategy, max_skew):
    """From zero entry counts, after every placement max - min over the eligible domains of the
    placements made this call is at most max_skew."""
    cont, nodes, dom = _random_scenario(7, 300, 50, 6)
    trace = []
    a, r, _, _ = SR.place(cont, nodes, strategy, domain=dom, max_skew=max_skew, trace=trace)
    assert len(trace) == (a != NONE).sum() > 50
    for dc, elig in trace:
        assert int(dc[elig].max()) - int(dc[elig].min()) <= max_skew
    placed = np.bincount(dom[a[a != NONE]], minlength=64)
    assert np.array_equal(placed, trace[-1][0])


# ---- the ABI's names ----------------------------------------------------------------------------------
def test_header_binding_and_reference_agree():
    from fleetflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    assert "FP_REASON_CYCLE = 2, FP_REASON_SKEW = 3" in hdr
    assert f"#define FP_SPREAD_MAX_DOMAINS {_lib.FP_SPREAD_MAX_DOMAINS}" in hdr
    assert _lib.REASON_SKEW == SR.REASON_SKEW == 3 and _lib.FP_SPREAD_MAX_DOMAINS == SR.MAX_DOMAINS == 64
    for name in ("fp_place_policy_spread", "fp_place_batch_policy_spread", "fp_dev_place_batch_policy_spread"):
        assert f"int {name}(fp_ctx *ctx" in hdr and name in _lib.SIGNATURES
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    assert "pub const FP_REASON_SKEW: u8 = 3;" in ffi and "pub const FP_SPREAD_MAX_DOMAINS: u32 = 64;" in ffi


# ---- KDL `spread` child of `placement` ------------------------------------------------------------------
KDL = """
project "demo"
server "n0" { capacity cpu=4000 memory=8192; label "region=osaka" }
server "n1" { capacity cpu=4000 memory=8192; label "region=tokyo" }
service "a" { resources cpu=500 memory=512 }
service "b" { resources cpu=500 memory=512 }
stage "live" {
    service "a"
    service "b"
    server "n0"
    server "n1"
    %s
}
"""


def test_kdl_spread_node():
    from fleetflow_amd.flow import PlacementPolicy
    from fleetflow_amd.parser import FlowError, parse_kdl_string
    pol = parse_kdl_string(KDL % 'placement strategy="fill_lowest" { prefer "region=tokyo"; spread "region" max-skew=1 }'
                           ).stages["live"].placement
    assert (pol.strategy, pol.preferred_labels, pol.spread) == ("fill_lowest", {"region": "tokyo"}, ("region", 1))
    pol = parse_kdl_string(KDL % 'placement { spread "zone" max-skew=3 }').stages["live"].placement
    assert (pol.strategy, pol.preferred_labels, pol.spread, pol.active) == (None, {}, ("zone", 3), True)
    # without the child nothing changes
    pol = parse_kdl_string(KDL % 'placement strategy="fill_lowest"').stages["live"].placement
    assert pol.spread is None and pol.spread_topology_key is None and pol.spread_max_skew is None
    for bad in ('spread max-skew=1', 'spread "region"', 'spread "region" max-skew=0', 'spread "region" max-skew="1"',
                'spread "region" max-skew=-1', 'spread "region=tokyo" max-skew=1', 'spread "region" "zone" max-skew=1',
                'spread 3 max-skew=1', 'spread "region" max-skew=4294967296'):
        with pytest.raises(FlowError):
            parse_kdl_string(KDL % ("placement { %s }" % bad))
    # active() needs both fields and max_skew >= 1
    assert not PlacementPolicy(spread_topology_key="region").active
    assert not PlacementPolicy(spread_max_skew=1).active
    assert not PlacementPolicy(spread_topology_key="region", spread_max_skew=0).active
    assert PlacementPolicy(spread_topology_key="region", spread_max_skew=1).active


def test_registry_reads_the_spread_constraint():
    from fleetflow_amd.registry import placement_policy
    row = {"placement_policy": {"strategy": "pack_into_dedicated", "preferred_labels": {"region": "tokyo"},
                                "spread_constraint": {"topology_key": "region", "max_skew": 2}}}
    pol = placement_policy(row)
    assert (pol.strategy, pol.spread_topology_key, pol.spread_max_skew, pol.spread) == ("pack_into_dedicated", "region", 2,
                                                                                       ("region", 2))
    pol = placement_policy({"placement_policy": {"spread_constraint": {"topology_key": "zone", "max_skew": 1}}})
    assert pol.strategy is None and pol.spread == ("zone", 1) and pol.active
    assert placement_policy({"placement_policy": {"spread_constraint": None}}).spread is None
    assert placement_policy({"placement_policy": {"tier": "free"}}).spread is None
    for skew in (0, -1, None, "1", 1.5, True):
        with pytest.raises(ValueError):
            placement_policy({"placement_policy": {"spread_constraint": {"topology_key": "region", "max_skew": skew}}})


# ---- plan_stage's domain derivation -------------------------------------------------------------------
def test_spread_domains_by_first_appearance():
    from fleetflow_amd.flow import Server, spread_domains
    srv = [Server("a", labels=["class=gpu", "region=tokyo"]), Server("b", labels=["region=osaka"]), Server("c", labels=["class=cpu"]),
           Server("d", labels=["region=tokyo"]), Server("e", labels=["regional=x", "region=nagoya"])]
    assert spread_domains(srv, "region") == ([0, 1, 0, 0, 2], [True, True, False, True, True])
    assert spread_domains(srv, "zone") == ([0] * 5, [False] * 5)
    many = [Server(f"s{i}", labels=[f"rack=r{i}"]) for i in range(64)]
    assert spread_domains(many, "rack")[0] == list(range(64))
    with pytest.raises(ValueError, match="rack"):
        spread_domains(many + [Server("x", labels=["rack=one-more"])], "rack")


class _StubPlanner:
    """plan_stage's planner calls, answered by the numpy references: no library, no GPU."""

    def __init__(self):
        self.policy_call = None

    def plan_stage(self, row_ptr, col, has_deps, cont, ntab):
        v = len(has_deps)
        a, r, _, _ = R.place(cont, ntab, R.FIRST_FIT)
        return (np.arange(v, dtype=np.uint32), np.zeros(v, np.uint32), np.arange(v, dtype=np.uint32), 0,
                (np.zeros(v, np.uint32), np.full(v, len(ntab[0]), np.uint32), a, r, None))

    def place_policy(self, cont, nodes, strategy, preferred=0, level=None, node_count=None, *, domain=None, max_skew=0):
        self.policy_call = dict(nodes=nodes, strategy=strategy, domain=domain, max_skew=max_skew)
        return SR.place(cont, nodes, strategy, preferred=preferred, level=level, domain=domain, max_skew=max_skew)


STAGE = """
project "demo"
server "t0" { capacity cpu=4000 memory=8192; label "region=tokyo" }
server "bare" { capacity cpu=64000 memory=65536 }
server "o0" { capacity cpu=1000 memory=8192; label "region=osaka" }
server "t1" { capacity cpu=4000 memory=8192; label "region=tokyo" }
%s
stage "live" {
%s
    server "t0"
    server "bare"
    server "o0"
    server "t1"
    placement { spread "region" max-skew=1 }
}
"""


def _stage(cpus):
    from fleetflow_amd.parser import parse_kdl_string
    svc = "\n".join(f'service "s{i}" {{ resources cpu={c} memory=64 }}' for i, c in enumerate(cpus))
    return parse_kdl_string(STAGE % (svc, "\n".join(f'    service "s{i}"' for i in range(len(cpus)))))


def test_plan_stage_derives_the_domains_and_reports_skew():
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    # s0 and s1 only fit tokyo's servers (and the unlabelled one, which is no candidate)
    flow = _stage([2000, 2000, 500, 500])
    stub = _StubPlanner()
    plan = plan_stage(flow, "live", stub)
    call = stub.policy_call
    assert call["domain"] == [0, 0, 1, 0] and call["max_skew"] == 1 and call["strategy"] == 0
    assert list(call["nodes"][4]) == [1, 0, 1, 1]  # the server without the key: unschedulable for this call only
    assert "bare" not in plan.assignment.values()
    # FFD order s0, s1, s2, s3: s0 -> t0 (tokyo 1, osaka 0); s1 fits tokyo only, which is one ahead: SKEW;
    # s2 -> o0 (1, 1); s3 may go anywhere again and first fit takes t0
    assert plan.assignment == {"s0": "t0", "s2": "o0", "s3": "t0"} and plan.rejected == {"s1": "SKEW"}
    assert (plan.spread_topology_key, plan.spread_max_skew, plan.strategy) == ("region", 1, None)
    # osaka holds 1000 millicores: s1 and s2 fit tokyo only, which stays one ahead until s3 lands in osaka
    flow = _stage([2000, 2000, 2000, 900])
    plan = plan_stage(flow, "live", _StubPlanner())
    assert plan.assignment == {"s0": "t0", "s3": "o0"} and plan.rejected == {"s1": "SKEW", "s2": "SKEW"}
    text = format_up_dry_run(flow, "live", plan)
    assert "    配置先: (配置不可: SKEW)" in text and "  配置分散保証: region (max_skew=1)" in text
    assert "  配置戦略: first_fit" in text
    assert plan_from_json(plan_to_json(plan)) == plan
    assert '"spread": {"topology_key": "region", "max_skew": 1}' in plan_to_json(plan)


def test_plan_output_without_a_constraint_is_unchanged():
    from fleetflow_amd.flow import Plan
    from fleetflow_amd.plan_output import plan_from_json, plan_to_json
    scored = Plan("live", ["a"], {"a": 0}, ["a"], {"a": "n1"}, {}, {"a": (2, "n0")}, "fill_lowest", ["region=tokyo"])
    text = plan_to_json(scored)
    assert '"placement": {"strategy": "fill_lowest", "preferred": ["region=tokyo"]}' in text and "spread" not in text
    assert plan_from_json(text) == scored
    plain = Plan("live", ["a"], {"a": 0}, ["a"], {"a": "n1"}, {}, {"a": (2, "n0")})
    assert "placement" not in plan_to_json(plain) and plan_from_json(plan_to_json(plain)) == plain
    both = Plan("live", ["a"], {"a": 0}, ["a"], {"a": "n1"}, {}, {"a": (2, "n0")}, "fill_lowest", [], "zone", 2)
    assert plan_from_json(plan_to_json(both)) == both and both != scored
