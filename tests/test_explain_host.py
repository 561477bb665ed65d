"""Rejection diagnosis (SPEC.md 2.9) without a GPU: the numpy reference against the oracle and against
tables small enough to check by hand, and the plan's JSON and dry-run text with and without ``why``."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explain_cases as K  # noqa: E402
import explain_ref as ER  # noqa: E402

NONE = 0xFFFFFFFF


@pytest.mark.parametrize("C,N", K.SHAPES)
def test_reference_feasible_is_the_oracle_count(C, N, O):
    cont, nodes = K.crafted(C, N)
    r = K.expected(C, N)
    K.assert_floors(r)
    _, count, _ = O.feasibility(cont, nodes, want_bitmap=False)
    assert np.array_equal(r[:, ER.FEASIBLE], count)
    assert np.array_equal(ER.rows_matrix(cont, nodes), r)  # the matrix form the batch tests use
    assert np.array_equal(ER.rows_matrix(cont, nodes, ignore=0x2078), ER.rows(cont, nodes, ignore=0x2078))
    # why == 0 is exactly "feasible by 2.3": the first feasible node too
    first, _, _ = O.feasibility(cont, nodes, want_bitmap=False)
    for c in (0, C // 2, C - 1):
        z = np.flatnonzero(ER.why(c, cont, nodes) == 0)
        assert (int(z[0]) if z.size else NONE) == int(first[c])


def _closed_form():
    # nodes:        n0 small   n1 cordoned  n2 port 1 busy  n3 other label
    nodes = ([100, 1000, 1000, 1000], [100, 1000, 1000, 1000], [0b01, 0b01, 0b01, 0b10], [0, 0, 0b1, 0], [1, 0, 1, 1])
    # containers:  c0 fits n0 only by size   c1 big, label 0, port 1   c2 wants label bit 2 (nobody has it)   c3 nothing
    cont = ([100, 500, 0, 0], [100, 500, 0, 0], [0b01, 0b01, 0b100, 0], [0, 0b1, 0, 0])
    return cont, nodes


def test_closed_form_by_hand():
    cont, nodes = _closed_form()
    r = ER.rows(cont, nodes)
    row = lambda fail, only, feas, all_, miss, near: fail + only + [feas, all_, miss, near, 0, 0]  # noqa: E731
    # c0: n0 ok, n1 cordon only, n2 ok, n3 label only
    assert r[0].tolist() == row([1, 0, 0, 1, 0], [1, 0, 0, 1, 0], 2, 0, 0, 1)
    # c1: n0 cpu+mem, n1 cordon, n2 conflict, n3 label
    assert r[1].tolist() == row([1, 1, 1, 1, 1], [1, 0, 0, 1, 1], 0, 0, 0, 1)
    # c2: label everywhere, cordon on n1 as well; bit 2 is missing
    assert r[2].tolist() == row([1, 0, 0, 4, 0], [0, 0, 0, 3, 0], 0, ER.LABEL, 0b100, 0)
    # c3: only the cordon
    assert r[3].tolist() == row([1, 0, 0, 0, 0], [1, 0, 0, 0, 0], 3, 0, 0, 1)
    # giving bit 2 up: c2 is c3
    assert ER.rows(cont, nodes, sel=[2], ignore=0b100)[0].tolist() == r[3].tolist()
    # MISSING looks at schedulable nodes only: with n3 cordoned, label bit 1 is missing for a container that asks for it
    nodes2 = (*nodes[:4], [1, 0, 1, 0])
    assert ER.rows(([0], [0], [0b10], [0]), nodes2)[0, ER.MISSING] == 0b10
    assert ER.rows(([0], [0], [0b10], [0]), nodes)[0, ER.MISSING] == 0
    # sel: order and repeats
    assert ER.rows(cont, nodes, sel=[3, 0, 3]).tolist() == [r[3].tolist(), r[0].tolist(), r[3].tolist()]
    h = ER.hist(r)
    assert h.tolist() == [0, 0, 0, 1, 0, 1, 2, 4]  # c2 LABEL; c1 MIXED; c0, c3 FITS


def test_no_nodes():
    cont, _ = K.crafted(300, 64)
    empty = tuple(np.zeros(0, np.uint32) for _ in range(4)) + (np.zeros(0, np.uint8),)
    r = ER.rows(cont, empty, ignore=1 << 13)
    assert (r[:, :ER.ALL] == 0).all() and (r[:, ER.ALL] == 0x1F).all() and (r[:, ER.NEAR] == NONE).all()
    assert np.array_equal(r[:, ER.MISSING], cont[2] & ~np.uint32(1 << 13)) and (r[:, 14:] == 0).all()
    assert ER.hist(r).tolist() == [300] * 5 + [0, 0, 300]
    assert np.array_equal(ER.rows_matrix(cont, empty, ignore=1 << 13), r)


def test_all_cordoned():
    C, N = 300, 65
    cont, nodes = K.all_cordoned(C, N)
    r = ER.rows(cont, nodes)
    assert (r[:, ER.FAIL] == N).all() and (r[:, ER.ALL] & ER.CORDON).all() and (r[:, ER.FEASIBLE] == 0).all()
    assert np.array_equal(r[:, ER.MISSING], cont[2])  # no schedulable node carries anything
    zero = (np.asarray(cont[0]) == 0) & (np.asarray(cont[2]) == 0) & (np.asarray(cont[3]) == 0)
    assert zero.sum() >= 5 and (r[zero, ER.ONLY] == N).all() and (r[zero, ER.NEAR] == 0).all()
    assert ER.hist(r)[0] == C


# ---- the plan's JSON and the dry-run text --------------------------------------------------------------------

STAGE_KDL = """
project "demo"
server "g0" { capacity cpu=1000 memory=8192; label "class=gpu"; label "region=tokyo" }
server "c0" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=tokyo" }
server "c1" { capacity cpu=8000 memory=8192; label "class=cpu"; label "region=osaka" }
service "train" { resources cpu=900 memory=64; require "class=gpu" "region=tokyo" }
service "infer" { resources cpu=800 memory=64; require "class=gpu" "region=tokyo" }
service "web" { resources cpu=100 memory=64; require "region=osaka" }
stage "live" {
    service "train"
    service "infer"
    service "web"
    server "g0"
    server "c0"
    server "c1"
}
"""

# `fleet up --dry-run` of the plan below without a diagnosis: the text before SPEC.md 2.9 existed
TEXT_WITHOUT_WHY = """[dry-run] ステージ 'live' の起動計画:

  ネットワーク: demo-live (作成予定)

  サービス: train
    コンテナ: demo-live-train
    イメージ: (未設定)
    起動レベル: 0
    配置候補: 1 台 (最初: g0)
    配置先: g0

  サービス: infer
    コンテナ: demo-live-infer
    イメージ: (未設定)
    起動レベル: 0
    配置候補: 1 台 (最初: g0)
    配置先: (配置不可: NOFIT)

  サービス: web
    コンテナ: demo-live-web
    イメージ: (未設定)
    起動レベル: 0
    配置候補: 1 台 (最初: c1)
    配置先: c1

[dry-run] 実際の操作は行われません。--dry-run を外して実行してください。
"""
JSON_WITHOUT_WHY = {
    "stage": "live", "order": ["train", "infer", "web"], "levels": {"train": 0, "infer": 0, "web": 0},
    "level_order": ["train", "infer", "web"], "assign": {"train": "g0", "web": "c1"}, "rejected": {"infer": "NOFIT"},
    "candidates": {"train": {"count": 1, "first": "g0"}, "infer": {"count": 1, "first": "g0"},
                   "web": {"count": 1, "first": "c1"}}}


def _plan():
    from fleetflow_amd.flow import Plan
    names = ["train", "infer", "web"]
    return Plan("live", names, {n: 0 for n in names}, list(names), {"train": "g0", "web": "c1"}, {"infer": "NOFIT"},
                {"train": (1, "g0"), "infer": (1, "g0"), "web": (1, "c1")})


def _why():
    from fleetflow_amd.flow import Why
    return Why({"CORDON": 0, "CPU": 1, "MEM": 0, "LABEL": 2, "CONFLICT": 0},
               {"CORDON": 0, "CPU": 1, "MEM": 0, "LABEL": 2, "CONFLICT": 0}, 0, [], [], "g0", 3)


def test_plan_without_why_is_unchanged():
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    flow, plan = parse_kdl_string(STAGE_KDL), _plan()
    assert plan.why == {}
    assert format_up_dry_run(flow, "live", plan) == TEXT_WITHOUT_WHY
    text = plan_to_json(plan)
    assert json.loads(text) == JSON_WITHOUT_WHY and "why" not in text
    assert text == json.dumps(JSON_WITHOUT_WHY, ensure_ascii=False)  # key order included
    assert plan_from_json(text) == plan


def test_plan_with_why_round_trips_and_prints_one_line():
    from fleetflow_amd.flow import Why
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_deploy_dry_run, format_up_dry_run, plan_from_json, plan_to_json
    flow, plan = parse_kdl_string(STAGE_KDL), _plan()
    plan.why = {"infer": _why()}
    back = plan_from_json(plan_to_json(plan))
    assert back == plan and isinstance(back.why["infer"], Why)
    d = json.loads(plan_to_json(plan))
    assert {k: v for k, v in d.items() if k != "why"} == JSON_WITHOUT_WHY
    assert d["why"]["infer"]["fail"] == plan.why["infer"].fail and d["why"]["infer"]["nearest"] == "g0"
    line = "    配置不可の理由: CPU 1/3 台, LABEL 2/3 台 (最も近い: g0)"
    out = format_up_dry_run(flow, "live", plan)
    at = TEXT_WITHOUT_WHY.index("    配置先: (配置不可: NOFIT)\n") + len("    配置先: (配置不可: NOFIT)\n")
    assert out == TEXT_WITHOUT_WHY[:at] + line + "\n" + TEXT_WITHOUT_WHY[at:]
    assert line in format_deploy_dry_run(flow, "live", ["infer"], "default", plan)
    # universal causes are marked, missing labels are named, no nearest server: nothing in its place
    plan.why["infer"] = Why({"CORDON": 1, "CPU": 0, "MEM": 0, "LABEL": 3, "CONFLICT": 0},
                            {"CORDON": 0, "CPU": 0, "MEM": 0, "LABEL": 2, "CONFLICT": 0}, 0, ["LABEL"], ["class=tpu"], None, 3)
    out = format_up_dry_run(flow, "live", plan)
    assert "    配置不可の理由: CORDON 1/3 台, LABEL 3/3 台 (全台) (該当ラベルなし: class=tpu)\n" in out
    # a diagnosis for a service that is not rejected prints nothing
    plan.why = {"train": _why()}
    assert format_up_dry_run(flow, "live", plan) == TEXT_WITHOUT_WHY


def test_why_from_row():
    from fleetflow_amd.flow import LabelDict, Why
    ld = LabelDict(["class=gpu", "region=tokyo", "class=cpu"])  # sorted: class=cpu 0, class=gpu 1, region=tokyo 2
    row = [0, 1, 0, 2, 0, 0, 1, 0, 2, 0, 0, 0, 0b10, 0, 0, 0]
    w = Why.from_row(np.array(row, np.uint32), ld, ["g0", "c0", "c1"])
    assert w == Why({"CORDON": 0, "CPU": 1, "MEM": 0, "LABEL": 2, "CONFLICT": 0},
                    {"CORDON": 0, "CPU": 1, "MEM": 0, "LABEL": 2, "CONFLICT": 0}, 0, [], ["class=gpu"], "g0", 3)
    row[ER.ALL], row[ER.NEAR] = ER.CPU | ER.CONFLICT, NONE
    w = Why.from_row(row, ld, ["g0", "c0", "c1"])
    assert w.universal == ["CPU", "CONFLICT"] and w.nearest is None
