"""CPU tests of the resource quota (SPEC.md 2.10): the numpy reference stated two ways, and the host layers
(KDL ``quota`` node, registry conversion, PlacementPolicy, plan JSON and dry-run text).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_cases as K  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_quota_ref as QR  # noqa: E402
import policy_ref as R  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd.flow import Flow, Plan, PlacementPolicy, Service, Stage  # noqa: E402
from fleetflow_amd.parser import FlowError, parse_kdl_string  # noqa: E402
from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json  # noqa: E402
from fleetflow_amd.registry import placement_policy  # noqa: E402

U = QR.UNLIMITED
NONE = 0xFFFFFFFF


# ---- the admission test, two ways ------------------------------------------------------------------------
def test_the_two_forms_of_the_admission_test_agree():
    rng = np.random.default_rng(2010)
    edge = [0, 1, 2, 0x7FFFFFFF, 0x80000000, U - 1, U]
    seen = {True: 0, False: 0}
    cases = [(q, u, r) for q in edge for u in edge for r in edge]
    big = rng.integers(0, 1 << 32, (4000, 3), dtype=np.uint64)
    cases += [tuple(int(x) for x in row) for row in big]
    small = rng.integers(0, 8, (2000, 3))  # used > quota, used == quota, r == remainder, r == 0 all occur
    cases += [tuple(int(x) for x in row) for row in small]
    near = rng.integers(0, 1 << 32, 2000, dtype=np.uint64)
    for q in near:  # used and r around a large cap, where a u32 sum would wrap
        u = int(q) - int(rng.integers(0, 3))
        cases.append((int(q), max(u, 0), int(rng.integers(0, 4))))
        cases.append((int(q), int(rng.integers(0, 1 << 32)), U - int(rng.integers(0, 3))))
    for q, u, r in cases:
        b = QR.blocks_sub(q, u, r)
        assert b == QR.blocks_wide(q, u, r), (q, u, r)
        seen[b] += 1
    assert seen[True] > 1000 and seen[False] > 1000
    # the rule's edges, spelled out
    assert not QR.blocks_sub(0, 0, 0) and QR.blocks_sub(0, 0, 1)        # cap 0: a zero request passes
    assert QR.blocks_sub(5, 9, 1) and not QR.blocks_sub(5, 9, 0)        # used > cap: every non-zero request
    assert QR.blocks_sub(5, 5, 1) and not QR.blocks_sub(5, 2, 3) and QR.blocks_sub(5, 2, 4)
    assert not QR.blocks_sub(U, U, U)                                    # unlimited never blocks


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_unlimited_caps_are_the_fallback_reference(strategy):
    C, N = 300, 65
    cont, nodes = K.crafted(C, N)
    rng = np.random.default_rng(5)
    level = np.where(rng.random(C) < 0.1, NONE, 0).astype(np.uint32)
    cnt0 = rng.integers(0, 4, N).astype(np.uint32)
    kw = dict(preferred=(1 << 4) | (1 << 8), level=level, node_count=cnt0, domain=K.spread_domain(N), max_skew=2,
              relax_mask=K.RELAX[2])
    exp = FR.place(cont, nodes, strategy, **kw)
    assert (exp[1] == 3).sum() > 0 and (exp[2] >= 1).sum() > 0 and (exp[1] == 2).sum() > 0
    for form in (QR.blocks_sub, QR.blocks_wide):
        got = QR.place(cont, nodes, strategy, (U, U, U), quota_used=(7, 0xFFFFFFF0, 3), blocks=form, **kw)
        assert all(np.array_equal(g, e) for g, e in zip(got[:3], exp[:3]))
        assert all(np.array_equal(g, e) for g, e in zip(got[3], exp[3])) and np.array_equal(got[4], exp[4])
        assert not got[5].any()
        u = QR.usage(cont, exp[0])
        assert [int(x) for x in got[6]] == [(7 + u[0]) & U, (0xFFFFFFF0 + u[1]) & U, 3 + u[2]]  # u32, wraps


def test_reference_under_caps():
    """A cap bites per container in the FFD order: a large one is refused, smaller ones behind it still go in;
    NOFIT and CYCLE are not charged; both forms give the same plan."""
    from oracle import pyoracle as P
    C, N = 200, 20
    cont = tuple(np.array(x, np.uint32) for x in P.gen_containers(0x5EED0002, C, 7))  # SPEC.md 3.2: memory is random
    nd = P.gen_nodes(0x5EED0002, N)
    nodes = tuple(np.array(x, np.uint32) for x in nd[:4]) + (np.array(nd[4], np.uint8),)
    level = np.zeros(C, np.uint32)
    level[::17] = NONE
    free = FR.place(cont, nodes, R.SPREAD, level=level)
    u = QR.usage(cont, free[0])
    order = list(R.ffd_order(*cont[:2]))
    bits = 0
    for caps in ((u[0] // 2, U, U), (U, u[1] // 3, U), (U, U, u[2] // 2), (u[0] * 4 // 5, u[1] // 3, 50)):
        got = QR.place(cont, nodes, R.SPREAD, caps, level=level)
        a, r, why, used = got[0], got[1], got[5], got[6]
        assert np.array_equal(r == 2, level == NONE) and not why[r != 4].any() and (why[r == 4] != 0).all()
        assert (r == 4).sum() > 20 and (r == 0).sum() > 20
        assert tuple(int(x) for x in used) == QR.usage(cont, a)  # NOFIT, CYCLE and QUOTA are not charged
        assert all(c == U or int(x) <= c for x, c in zip(used, caps))
        assert all(not (why[i] >> d & 1) for i in range(C) for d in range(3) if caps[d] == U)
        if caps[0] == U and caps[2] == U:  # memory is not sorted: smaller containers behind a refused one still go in
            first_quota = next(k for k, i in enumerate(order) if r[i] == 4)
            assert any(r[i] == 0 for i in order[first_quota:])
        wide = QR.place(cont, nodes, R.SPREAD, caps, level=level, blocks=QR.blocks_wide)
        assert all(np.array_equal(got[k], wide[k]) for k in (0, 1, 2, 4, 5, 6))
        assert QR.cost(a, r, 3) >> 40 == (r != 0).sum()  # the cost counts QUOTA as rejected
        bits |= int(np.bitwise_or.reduce(why))
    assert bits == 7  # every dimension refused something


# ---- KDL ------------------------------------------------------------------------------------------------------
KDL = 'service "a" { image "x" }\nstage "s" { service "a"; placement %s }\n'


def _policy(body):
    return parse_kdl_string(KDL % body).stages["s"].placement


def test_kdl_quota_node():
    p = _policy("{ quota cpu=4000 memory=8192 services=10 }")
    assert p.quota == (4000, 8192, 10) and p.active and p.strategy is None
    assert _policy("{ quota services=0 }").quota == (None, None, 0)
    assert _policy("{ quota memory=4294967294 }").quota == (None, 0xFFFFFFFE, None)
    p = _policy('strategy="fill_lowest" { prefer "region=tokyo"; spread "region" max-skew=1; fallback "class"; quota cpu=1 }')
    assert (p.strategy, p.spread, p.fallback, p.quota) == ("fill_lowest", ("region", 1), ("class",), (1, None, None))
    assert _policy('strategy="fill_lowest"').quota is None


@pytest.mark.parametrize("body", [
    "{ quota }",                               # no property
    "{ quota cpu=1 disk=5 }",                  # another property
    "{ quota 4000 }",                          # an argument
    '{ quota "cpu" cpu=1 }',                   # an argument beside a property
    "{ quota cpu=1; quota memory=2 }",         # a second node
    '{ quota cpu="4000" }',                    # non-integers
    "{ quota memory=1.5 }",
    "{ quota services=#true }",
    "{ quota cpu=-1 }",                        # out of 0 .. 0xFFFFFFFE
    "{ quota cpu=4294967295 }",
    "{ quota services=4294967296 }",
])
def test_kdl_quota_errors(body):
    with pytest.raises(FlowError) as e:
        _policy(body)
    assert "stage s" in str(e.value) and "quota" in str(e.value)


# ---- registry ---------------------------------------------------------------------------------------------
def _row(rq, **more):
    return {"placement_policy": {"resource_quota": rq, **more}}


def test_registry_conversion():
    p = placement_policy(_row({"max_stages": 3, "max_services_per_stage": 12, "cpu_cores": 8, "memory_gb": 16}))
    assert p.quota == (8000, 16384, 12) and p.active
    # null and missing fields are no cap; max_stages alone is no quota for the planner
    assert placement_policy(_row({"max_stages": 3, "cpu_cores": None, "memory_gb": 2})).quota == (None, 2048, None)
    p = placement_policy(_row({"max_stages": 3}))
    assert p.quota is None and not p.active
    assert placement_policy(_row(None)).quota is None and placement_policy(_row({})).quota is None
    # the clamp: the largest cap a u32 can say, and past it no cap
    assert placement_policy(_row({"cpu_cores": 4294967})).quota == (4294967000, None, None)
    assert placement_policy(_row({"cpu_cores": 4294968})).quota is None
    assert placement_policy(_row({"memory_gb": 4194303})).quota == (None, 4194303 * 1024, None)
    assert placement_policy(_row({"memory_gb": 4194304, "cpu_cores": 0})).quota == (0, None, None)
    assert placement_policy(_row({"max_services_per_stage": 0xFFFFFFFE})).quota == (None, None, 0xFFFFFFFE)
    assert placement_policy(_row({"max_services_per_stage": 0xFFFFFFFF})).quota is None
    # equality is still strategy and preferred labels only
    a = placement_policy(_row({"cpu_cores": 1}, strategy="fill_lowest"))
    assert a == PlacementPolicy("fill_lowest") and a.quota != PlacementPolicy("fill_lowest").quota


@pytest.mark.parametrize("rq", [{"cpu_cores": -1}, {"memory_gb": 1.5}, {"max_services_per_stage": "10"},
                                {"cpu_cores": True}, [4, 8]])
def test_registry_quota_errors(rq):
    with pytest.raises(ValueError) as e:
        placement_policy(_row(rq))
    assert "resource_quota" in str(e.value)


def test_policy_active_and_validation():
    assert not PlacementPolicy().active and PlacementPolicy().quota is None
    for kw in (dict(quota_cpu_m=0), dict(quota_mem_mib=1), dict(quota_services=5)):
        p = PlacementPolicy(**kw)
        assert p.active and p.quota is not None and p == PlacementPolicy()  # compare=False
    for bad in (-1, 0xFFFFFFFF, 1.0, True, "4"):
        with pytest.raises(ValueError):
            PlacementPolicy(quota_services=bad)


# ---- plan JSON and dry-run --------------------------------------------------------------------------------
def _flow():
    f = Flow(name="demo")
    f.services = {"big": Service(image="x"), "web": Service(image="y")}
    f.stages = {"live": Stage(services=["big", "web"], servers=["n0"])}
    return f


def _plan(quota):
    p = Plan("live", ["big", "web"], {"big": 0, "web": 0}, ["big", "web"], {"web": "n0"}, {"big": "QUOTA" if quota else "NOFIT"},
             {"big": (1, "n0"), "web": (1, "n0")})
    if quota:
        p.quota, p.quota_used, p.quota_why = (4000, None, 10), (100, 64, 1), {"big": ["cpu"]}
    return p


TODAY = """[dry-run] ステージ 'live' の起動計画:

  ネットワーク: demo-live (作成予定)

  サービス: big
    コンテナ: demo-live-big
    イメージ: x
    起動レベル: 0
    配置候補: 1 台 (最初: n0)
    配置先: (配置不可: NOFIT)

  サービス: web
    コンテナ: demo-live-web
    イメージ: y
    起動レベル: 0
    配置候補: 1 台 (最初: n0)
    配置先: n0

[dry-run] 実際の操作は行われません。--dry-run を外して実行してください。
"""


def test_json_round_trip():
    p = _plan(True)
    d = __import__("json").loads(plan_to_json(p))
    assert d["quota"] == {"caps": {"cpu": 4000, "memory": None, "services": 10}, "used": {"cpu": 100, "memory": 64, "services": 1}}
    assert d["quota_why"] == {"big": ["cpu"]} and d["rejected"] == {"big": "QUOTA"}
    assert plan_from_json(plan_to_json(p)) == p
    # without a quota: today's keys, nothing else
    q = _plan(False)
    assert set(__import__("json").loads(plan_to_json(q))) == {"stage", "order", "levels", "level_order", "assign", "rejected",
                                                             "candidates"}
    assert plan_from_json(plan_to_json(q)) == q and plan_from_json(plan_to_json(q)).quota is None


def test_dry_run_lines():
    f = _flow()
    assert format_up_dry_run(f, "live", _plan(False)) == TODAY  # byte for byte what it was
    out = format_up_dry_run(f, "live", _plan(True))
    assert "  配置戦略: first_fit\n  配置クォータ: cpu 100/4000, services 1/10\n" in out
    assert "    配置先: (配置不可: QUOTA)\n    クォータ超過: cpu\n" in out
    rest = [ln for ln in out.splitlines() if "クォータ" not in ln and "配置戦略" not in ln]
    assert rest == [ln.replace("NOFIT", "QUOTA") for ln in TODAY.splitlines()]


def test_constants_mirror_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fleetplace.h")).read()
    assert "FP_REASON_QUOTA = 4" in hdr and _lib.REASON_QUOTA == 4
    assert "FP_QUOTA_CPU = 0, FP_QUOTA_MEM = 1, FP_QUOTA_SERVICES = 2" in hdr
    assert (_lib.QUOTA_CPU, _lib.QUOTA_MEM, _lib.QUOTA_SERVICES, _lib.QUOTA_DIMS) == (0, 1, 2, 3)
    assert "#define FP_QUOTA_UNLIMITED 0xFFFFFFFFu" in hdr and _lib.QUOTA_UNLIMITED == 0xFFFFFFFF
    assert "#define FP_ABI_VERSION 1" in hdr
    for name in ("fp_place_policy_quota", "fp_place_batch_policy_quota", "fp_dev_place_batch_policy_quota"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
