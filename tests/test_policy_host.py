"""CPU tests of the scored placement (SPEC.md 2.6): the numpy reference (tests/policy_ref.py) against
the C oracle and by hand, and the front ends that carry a placement policy (KDL, registry, dry-run)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402

NONE = 0xFFFFFFFF
SEED = 0x5EED0004


def _same_plan(got, exp):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    for i in (0, 1, 3):
        assert np.array_equal(got[2][i], exp[2][i])


# ---- strategy 0 without a preferred mask is SPEC.md 2.3 ---------------------------------------
@pytest.mark.parametrize("C,N,flags", [(600, 70, 7), (1, 1, 7), (300, 64, 0), (300, 65, 7), (2000, 1025, 7)])
def test_first_fit_is_the_oracle(C, N, flags, O):
    cont, nodes = O.gen_scenario(SEED, 3, C, N, flags)
    _same_plan(R.place(cont, nodes, R.FIRST_FIT), O.place(cont, nodes))


def test_first_fit_is_the_oracle_with_cycles(O):
    cont, nodes = O.gen_scenario(SEED, 3, 600, 70, 7)
    level = np.where(np.random.default_rng(1).random(600) < 0.05, NONE, 3).astype(np.uint32)
    got, exp = R.place(cont, nodes, R.FIRST_FIT, level=level), O.place(cont, nodes, level=level)
    _same_plan(got, exp)
    assert (got[1] == 2).sum() == (level == NONE).sum() > 0


def test_strategies_differ_on_the_test_inputs(O):
    """The inputs the GPU tests use tell the strategies apart."""
    cont, nodes = O.gen_scenario(SEED, 3, 600, 70, 7)
    plans = [R.place(cont, nodes, st)[0] for st in R.STRATEGIES]
    for i in range(4):
        for j in range(i):
            assert (plans[i] != plans[j]).sum() > 100
    pref = (1 << 4) | (1 << 8)
    assert (R.place(cont, nodes, R.SPREAD, preferred=pref)[0] != plans[R.SPREAD]).sum() > 100


# ---- the key, by hand -----------------------------------------------------------------------------
def _nodes(cf, mf=None, lab=None, cu=None, sched=None):
    n = len(cf)
    return (np.array(cf, np.uint32), np.array(mf if mf is not None else [1000] * n, np.uint32),
            np.array(lab if lab is not None else [0] * n, np.uint32), np.array(cu if cu is not None else [0] * n, np.uint32),
            np.array(sched if sched is not None else [1] * n, np.uint8))


def _cont(cpu, mem=None, req=None, conf=None):
    c = len(cpu)
    return (np.array(cpu, np.uint32), np.array(mem if mem is not None else [1] * c, np.uint32),
            np.array(req if req is not None else [0] * c, np.uint32), np.array(conf if conf is not None else [0] * c, np.uint32))


def test_identical_nodes_take_the_lowest_index():
    nodes, cont = _nodes([100] * 5), _cont([10] * 7)
    assert R.place(cont, nodes, R.FIRST_FIT)[0].tolist() == [0] * 7
    assert R.place(cont, nodes, R.SPREAD)[0].tolist() == [0, 1, 2, 3, 4, 0, 1]
    assert R.place(cont, nodes, R.PACK)[0].tolist() == [0] * 7          # node 0 has the least left after the first
    assert R.place(cont, nodes, R.FILL_LOWEST)[0].tolist() == [0, 1, 2, 3, 4, 0, 1]  # most free CPU first


def test_pack_is_best_fit_and_fill_lowest_is_most_free():
    nodes = _nodes([50, 12, 30, 11])
    assert R.place(_cont([11]), nodes, R.PACK)[0].tolist() == [3]
    assert R.place(_cont([12]), nodes, R.PACK)[0].tolist() == [1]
    assert R.place(_cont([12]), nodes, R.FILL_LOWEST)[0].tolist() == [0]
    a, r, after, cnt = R.place(_cont([12, 12, 12]), nodes, R.FILL_LOWEST)
    assert a.tolist() == [0, 0, 2] and after[0].tolist() == [26, 12, 18, 11] and cnt.tolist() == [2, 0, 1, 0]


def test_unconstrained_nodes():
    big = 0xFFFFFFFF
    nodes = _nodes([big, 5, big], mf=[big, big, big])
    # PACK: primary = cpu_free - cpu is largest on the unconstrained nodes; FILL_LOWEST: ~cpu_free = 0 there
    assert R.place(_cont([5, 5]), nodes, R.PACK)[0].tolist() == [1, 0]
    assert R.place(_cont([5, 5]), nodes, R.FILL_LOWEST)[0].tolist() == [0, 2]
    a, _, after, _ = R.place(_cont([big], mem=[big]), nodes, R.PACK)
    assert a.tolist() == [0] and after[0][0] == 0 and after[1][0] == 0


def test_preferred_labels_rank_before_the_strategy():
    full = 0xFFFFFFFF
    nodes = _nodes([100] * 4, lab=[0, 0b0110, full, 0b0100])
    # all 32 bits preferred: node 2 misses none; then one miss fewer beats the strategy's own order
    assert R.place(_cont([10]), nodes, R.FIRST_FIT, preferred=full)[0].tolist() == [2]
    assert R.place(_cont([10] * 3), nodes, R.SPREAD, preferred=0b0110)[0].tolist() == [1, 2, 1]
    # preferred labels are soft: a node that misses all of them still takes what fits nowhere else
    a, r, _, _ = R.place(_cont([100, 100, 100, 100, 100]), nodes, R.PACK, preferred=full)
    assert a.tolist() == [2, 1, 3, 0, NONE] and r.tolist() == [0, 0, 0, 0, 1]


def test_node_count_on_entry_and_cordon():
    nodes = _nodes([100] * 4, sched=[1, 1, 0, 1])
    a, _, after, cnt = R.place(_cont([10] * 4), nodes, R.SPREAD, node_count=[5, 3, 0, 4])
    assert a.tolist() == [1, 1, 3, 0]  # 3 -> 4, the tie at 4 goes to node 1, then node 3 (4), then the tie at 5 to node 0
    assert cnt.tolist() == [6, 5, 0, 5] and after[0].tolist() == [90, 80, 100, 90]
    a, _, _, cnt = R.place(_cont([10]), nodes, R.SPREAD, node_count=[NONE, NONE, 0, NONE])
    assert a.tolist() == [0] and cnt[0] == 0  # the count wraps


def test_golden_pins_the_reference():
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_small.json")
    with open(path) as f:
        g = json.load(f)
    from oracle import oracle as O
    for case in g["cases"]:
        cont, nodes = O.gen_scenario(case["seed"], case["scenario"], case["C"], case["N"], case["flags"])
        a, r, after, cnt = R.place(cont, nodes, case["strategy"], preferred=case["preferred"])
        assert a.tolist() == case["assign"] and r.tolist() == case["reason"] and cnt.tolist() == case["node_count"]
        assert after[0].tolist() == case["cpu_free"]


# ---- KDL `placement` node ---------------------------------------------------------------------------
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
stage "plain" { service "a" }
"""


def test_kdl_placement_node():
    from fleetflow_amd.flow import PlacementPolicy
    from fleetflow_amd.parser import FlowError, parse_kdl_string
    flow = parse_kdl_string(KDL % 'placement strategy="spread_across_pool" { prefer "region=tokyo" }')
    assert flow.stages["live"].placement == PlacementPolicy("spread_across_pool", {"region": "tokyo"})
    assert flow.stages["plain"].placement is None
    assert flow.stages["live"].services == ["a", "b"] and flow.stages["live"].servers == ["n0", "n1"]
    flow = parse_kdl_string(KDL % 'placement { prefer "region=tokyo" "class=gpu" }')
    assert flow.stages["live"].placement == PlacementPolicy(None, {"region": "tokyo", "class": "gpu"})
    assert flow.stages["live"].placement.preferred == ["class=gpu", "region=tokyo"]
    assert parse_kdl_string(KDL % "").stages["live"].placement is None
    with pytest.raises(FlowError):
        parse_kdl_string(KDL % 'placement strategy="round_robin"')
    with pytest.raises(FlowError):
        parse_kdl_string(KDL % 'placement strategy="fill_lowest" { prefer "tokyo" }')
    with pytest.raises(ValueError):
        PlacementPolicy("first_fit")


def test_registry_placement_policy():
    from fleetflow_amd.flow import PlacementPolicy
    from fleetflow_amd.registry import placement_policy
    assert placement_policy({"slug": "acme"}) is None
    assert placement_policy({"slug": "acme", "placement_policy": None}) is None
    assert placement_policy(None) is None
    row = {"slug": "acme", "placement_policy": {"tier": "pro", "strategy": "pack_into_dedicated",
                                                "preferred_labels": {"region": "tokyo"},
                                                "spread_constraint": {"topology_key": "region", "max_skew": 1}}}
    assert placement_policy(row) == PlacementPolicy("pack_into_dedicated", {"region": "tokyo"})
    assert placement_policy({"placement_policy": {"tier": "free"}}) == PlacementPolicy(None, {})
    assert not placement_policy({"placement_policy": {"tier": "free"}}).active
    with pytest.raises(ValueError):
        placement_policy({"placement_policy": {"strategy": "binpack"}})


def test_strategy_names():
    from fleetflow_amd import _lib
    from fleetflow_amd.flow import POLICY_STRATEGIES
    from fleetflow_amd.planner import strategy_id
    assert [strategy_id(s) for s in POLICY_STRATEGIES] == [R.SPREAD, R.PACK, R.FILL_LOWEST]
    assert sorted(_lib.POLICY_STRATEGIES) == sorted(POLICY_STRATEGIES)
    assert strategy_id(0) == 0 and strategy_id(4) == 4  # the library refuses 4, not the binding
    with pytest.raises(ValueError):
        strategy_id("first_fit")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fleetplace.h")).read()
    assert "FP_STRATEGY_FIRST_FIT = 0, FP_STRATEGY_SPREAD = 1, FP_STRATEGY_PACK = 2, FP_STRATEGY_FILL_LOWEST = 3" in hdr
    assert f"#define FP_POLICY_MAX_NODES {_lib.FP_POLICY_MAX_NODES}" in hdr


# ---- dry-run output -----------------------------------------------------------------------------------
def test_plan_output_names_the_strategy_only_when_set():
    from fleetflow_amd.flow import Plan
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    flow = parse_kdl_string(KDL % "")
    plain = Plan("live", ["a", "b"], {"a": 0, "b": 0}, ["a", "b"], {"a": "n0", "b": "n0"}, {}, {"a": (2, "n0"), "b": (2, "n0")})
    text = format_up_dry_run(flow, "live", plain)
    assert "配置戦略" not in text and "placement" not in plan_to_json(plain)
    assert text.splitlines()[:4] == ["[dry-run] ステージ 'live' の起動計画:", "", "  ネットワーク: demo-live (作成予定)", ""]
    scored = Plan("live", ["a", "b"], {"a": 0, "b": 0}, ["a", "b"], {"a": "n1", "b": "n0"}, {}, {"a": (2, "n0"), "b": (2, "n0")},
                  "spread_across_pool", ["region=tokyo"])
    stext = format_up_dry_run(flow, "live", scored)
    assert "  配置戦略: spread_across_pool (優先ラベル: region=tokyo)" in stext.splitlines()
    # the strategy line and the changed server are the only differences
    assert [ln for ln in stext.splitlines() if "配置戦略" not in ln and "配置先" not in ln] == \
           [ln for ln in text.splitlines() if "配置先" not in ln]
    assert plan_from_json(plan_to_json(scored)) == scored and plan_from_json(plan_to_json(plain)) == plain
