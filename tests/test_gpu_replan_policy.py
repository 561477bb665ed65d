"""GPU tests of re-planning under the policy (SPEC.md 2.14; fleetflow_amd/csrc/fp_replan_policy.hip): the three entry
points against the numpy reference (tests/replan_policy_ref.py).  Every comparison is exact and covers every
output: assign, reason, hops, change, summary, the node table, node_count, quota_why, the usage and the cost."""
import ctypes as ct
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_ref as R  # noqa: E402
import replan_policy_ref as RPP  # noqa: E402
from test_replan_policy_host import HAND_POLICY_CASES, RELAX, gen_case, same  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
UNL = 0xFFFFFFFF
KEPT, NEW, MOVED, LOST, ABSENT = RPP.KEPT, RPP.NEW, RPP.MOVED, RPP.LOST, RPP.ABSENT


def _row4(relax):
    return list(relax) + [0] * (4 - len(relax))


def _both(planner, cont, nodes, prev, kw, scen_base=0, exp=None):
    """fp_replan_batch_policy with one scenario and fp_replan_policy, each against the reference in every output
    (the cost comes from the batch entry).  Returns the reference's answer."""
    exp = exp or RPP.replan(cont, nodes, prev, **kw)
    C, N = len(prev), len(nodes[0])
    sp, fb, qt = "domain" in kw, "relax_mask" in kw, kw.get("quota") is not None
    nh = kw.get("n_hops")
    nh = len(kw["relax_mask"]) if fb and nh is None else nh
    used0 = kw.get("quota_used")
    g = planner.replan_batch_policy(
        1, C, N, cont, nodes, prev, [kw.get("strategy", 0)], [UNL if q is None else q for q in kw["quota"]] if qt else None,
        used0, [kw.get("preferred", 0)], kw.get("level"), kw.get("node_count"), scen_base,
        domain=kw["domain"] if sp else None, max_skew=[kw["max_skew"]] if sp else None,
        relax_mask=_row4(kw["relax_mask"]) if fb else None, n_hops=[nh] if fb else None, want_used=used0 is not None or not qt)
    a, r, h, cost, chg, summ, after, nc, why, used = g
    same((a, r, h, chg, summ[0], after, exp[6] if nc is None else nc, why, exp[8] if used is None or not qt else used), exp)
    assert int(cost[0]) == RPP.cost(exp[0], exp[1], scen_base)
    g = planner.replan_policy(cont, nodes, prev, kw.get("strategy", 0), kw["quota"] if qt else None, used0,
                              kw["relax_mask"] if fb else None, kw.get("preferred", 0), kw.get("level"), kw.get("node_count"),
                              domain=kw["domain"] if sp else None, max_skew=kw["max_skew"] if sp else 0,
                              n_hops=nh if fb else None, want_used=used0 is not None or not qt)
    a, r, h, chg, summ, after, nc, why, used = g
    same((a, r, h, chg, summ, after, exp[6] if nc is None else nc, why, exp[8] if used is None or not qt else used), exp)
    assert (nc is None) == (kw.get("node_count") is None)
    return exp


@functools.lru_cache(maxsize=None)
def _case(seed, C, N, sp=True, fb=True, qt=True):
    return gen_case(seed, C, N, sp, fb, qt)


# ---- geometry: 64 x 1 and 1024 x {1, 2, 4, 8}, on both sides of every switch ----------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("N", [5, 64, 65, 139, 1024, 1025, 2049, 4097, 8192])
def test_every_block_geometry_with_every_guarantee(N, strategy, planner):
    c = _case(N, 200, N)
    kw = dict(c["kw"], strategy=strategy)
    exp = _both(planner, c["grown"], c["nodes2"], c["prev"], kw, scen_base=N % 100)
    assert exp[4][KEPT] > 0 and int(exp[4][:5].sum()) == 200


COMBOS = [(sp, fb, qt) for sp in (0, 1) for fb in (0, 1) for qt in (0, 1) if sp or fb or qt]


@pytest.mark.parametrize("N", [139, 4097])
@pytest.mark.parametrize("sp,fb,qt", COMBOS)
def test_every_combination_of_guarantees(sp, fb, qt, N, planner):
    c = _case(1000 + N + 4 * sp + 2 * fb + qt, 200, N, bool(sp), bool(fb), bool(qt))
    exp = _both(planner, c["grown"], c["nodes2"], c["prev"], c["kw"])
    assert exp[4][KEPT] > 0 and (exp[4][MOVED] + exp[4][LOST] + exp[4][NEW] + exp[4][ABSENT]) > 0


# ---- the named traps, through the ABI ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_POLICY_CASES, ids=[c[0] for c in HAND_POLICY_CASES])
def test_hand_made_cases_through_the_abi(case, planner):
    _, cont, nodes, prev, kw, want = case
    exp = _both(planner, cont, nodes, prev, kw)
    assert exp[0].tolist() == want["assign"] and exp[1].tolist() == want["reason"]


def test_spread_node_count_given_and_null_and_no_constraint_in_one_scenario_of_a_batch(planner):
    c = _case(77, 200, 70, True, False, False)
    kw = dict(c["kw"])
    for cnt in (None, np.arange(70, dtype=np.uint32) % 3):
        kw["node_count"] = cnt
        _both(planner, c["grown"], c["nodes2"], c["prev"], kw)
    # a batch of two: the constraint in scenario 0 only (max_skew 0 in scenario 1, whose domains are junk)
    S, C, N = 2, 200, 70
    cont = tuple(np.tile(x, 2) for x in c["grown"])
    nodes = tuple(np.tile(x, 2) for x in c["nodes2"])
    dom = np.concatenate([kw["domain"], np.full(N, 0xDEAD, np.uint32)])
    kw["node_count"] = None
    e0 = RPP.replan(c["grown"], c["nodes2"], c["prev"], **kw)
    e1 = RPP.replan(c["grown"], c["nodes2"], c["prev"], **dict(kw, max_skew=0))
    g = planner.replan_batch_policy(S, C, N, cont, nodes, np.tile(c["prev"], 2), [kw["strategy"]] * 2, None, None,
                                    [kw["preferred"]] * 2, None if kw["level"] is None else np.tile(kw["level"], 2),
                                    domain=dom, max_skew=[kw["max_skew"], 0])
    for s, e in enumerate((e0, e1)):
        sl = slice(s * C, (s + 1) * C)
        assert np.array_equal(g[0][sl], e[0]) and np.array_equal(g[1][sl], e[1]) and np.array_equal(g[4][sl], e[3])
        assert np.array_equal(g[5][s], e[4]) and int(g[3][s]) == RPP.cost(e[0], e[1], s)
    assert not np.array_equal(e0[0], e1[0])


# ---- skip parity: CYCLE, QUOTA and kept records between reductions ------------------------------------------------
def _runs(n=129):
    keep, run = [], 1
    while len(keep) < n:
        keep += [False] + [True] * run
        run += 1
    return np.array(keep[:n])


_I = np.arange(129)
PATTERNS = {
    "none": np.zeros(129, bool),
    "all": np.ones(129, bool),
    "alternating": _I % 2 == 0,
    "alternating, odd": _I % 2 == 1,
    "a skipped chunk between two placing chunks": (_I >= 64) & (_I < 128),
    "a placing chunk between two skipped chunks": ~((_I >= 64) & (_I < 128)),
    "skipped runs of growing length": _runs(),
    "placing runs of growing length": ~_runs(),
}
KINDS = {"kept": 1, "cycle": 2, "quota": 3}


def _skip_case(kind):
    """129 containers of distinct, falling cpu, so the visiting order is the index order; kind[i]: 0 placed (or
    NOFIT), 1 kept, 2 CYCLE, 3 QUOTA.  Container i runs on node i, which has exactly its request free where it is
    to be kept and nothing otherwise; ten more nodes take four each of the others.  A QUOTA container asks for
    more memory than the cap ever leaves.  139 nodes: the 1024-thread kernel, sixteen waves."""
    C = kind.size
    cpu = np.arange(1000, 1000 - C, -1).astype(np.uint32)
    mem = np.where(kind == 3, 1000, 1).astype(np.uint32)
    cont = (cpu, mem, np.zeros(C, np.uint32), np.zeros(C, np.uint32))
    cf = np.concatenate([np.where(kind == 1, cpu, 0), np.full(10, 4000)]).astype(np.uint32)
    N = cf.size
    nodes = (cf, np.full(N, 1 << 20, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.ones(N, np.uint8))
    prev = np.where(kind == 2, NONE, np.arange(C)).astype(np.uint32)
    prev[(kind == 2) & (np.arange(C) % 2 == 0)] = np.arange(C)[(kind == 2) & (np.arange(C) % 2 == 0)]  # LOST and ABSENT
    kw = dict(level=np.where(kind == 2, NONE, 0).astype(np.uint32), domain=(np.arange(N) % 4).astype(np.uint32), max_skew=40,
              relax_mask=RELAX, n_hops=1, quota=[UNL, 700, UNL], quota_used=[0, 100, 0])
    return cont, nodes, prev, kw


@pytest.mark.parametrize("name", list(PATTERNS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_skip_patterns_along_the_visiting_order(kind, name, planner):
    k = np.where(PATTERNS[name], KINDS[kind], 0)
    cont, nodes, prev, kw = _skip_case(k)
    for strategy in (R.FIRST_FIT, R.SPREAD):
        exp = _both(planner, cont, nodes, prev, dict(kw, strategy=strategy))
        assert np.array_equal(exp[3] == KEPT, k == 1) and np.array_equal(exp[1] == 2, k == 2)
        assert np.array_equal(exp[1] == 4, k == 3) and int((exp[0][k == 0] != NONE).sum()) == min(40, int((k == 0).sum()))


@pytest.mark.parametrize("seed", [1, 2])
def test_skip_kinds_mixed(seed, planner):
    k = np.random.default_rng(seed).integers(0, 4, 129) if seed == 1 else (_I % 4)
    cont, nodes, prev, kw = _skip_case(k)
    exp = _both(planner, cont, nodes, prev, dict(kw, strategy=R.FILL_LOWEST))
    assert np.array_equal(exp[3] == KEPT, k == 1) and np.array_equal(exp[1] == 4, k == 3)


# ---- the theorems on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 2049])
def test_theorem_b_against_the_reference_and_place_batch_policy_quota(N, planner):
    c = _case(500 + N, 200, N)
    kw, C = c["kw"], 200
    none = np.full(C, NONE, np.uint32)
    exp = _both(planner, c["grown"], c["nodes2"], none, kw, scen_base=9)
    a, r, h, cost, after, cnt, why, used = planner.place_batch_policy_quota(
        1, C, N, c["grown"], c["nodes2"], [kw["strategy"]], kw["quota"], kw["quota_used"], [kw["preferred"]], kw["level"],
        kw["node_count"], 9, domain=kw["domain"], max_skew=[kw["max_skew"]], relax_mask=_row4(kw["relax_mask"]),
        n_hops=[kw["n_hops"]])
    same((a, r, h, np.where(a != NONE, NEW, ABSENT), exp[4], after, exp[6] if cnt is None else cnt, why, used), exp)
    assert int(cost[0]) == RPP.cost(exp[0], exp[1], 9) and (r == 4).any() and (a != NONE).any()


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_theorem_d_on_the_device(seed, planner):
    c = _case(seed, 200, 139)
    kw = c["kw"]
    a, r, h, after, cnt, why, used = planner.place_policy_quota(
        c["cont"], c["nodes"], kw["strategy"], kw["quota"], kw["quota_used"], kw["relax_mask"], kw["preferred"], kw["level"],
        kw["node_count"], domain=kw["domain"], max_skew=kw["max_skew"], n_hops=kw["n_hops"])
    assert np.array_equal(a, c["first"][0])
    exp = _both(planner, c["cont"], c["nodes"], a, kw)
    placed = a != NONE
    assert (exp[3][placed] == KEPT).all() and np.array_equal(exp[0][placed], a[placed]) and np.array_equal(exp[2][placed], h[placed])
    assert np.array_equal(exp[1] == 2, r == 2) and (exp[1][r == 4] == 4).all() and np.isin(exp[1][r == 1], (1, 4)).all()
    if not (r == 3).any():
        assert np.array_equal(exp[0], a) and np.array_equal(exp[8], used)


def test_theorem_c_a_replan_is_kept_by_the_next(planner):
    c = _case(11, 200, 139)
    one = _both(planner, c["grown"], c["nodes2"], c["prev"], c["kw"])
    two = _both(planner, c["grown"], c["nodes2"], one[0], c["kw"])
    placed = one[0] != NONE
    assert (two[3][placed] == KEPT).all() and np.array_equal(two[0][placed], one[0][placed])


# ---- entry points ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch3():
    """Three scenarios: every guarantee on; every one idle in its own way (max_skew 0, n_hops 0, three UNLIMITED);
    spread and quota without a chain."""
    S, C, N = 3, 200, 70
    cs = [_case(31, C, N), _case(32, C, N), _case(33, C, N)]
    kws = [dict(cs[0]["kw"]), dict(cs[1]["kw"], max_skew=0, n_hops=0, quota=[UNL] * 3), dict(cs[2]["kw"], n_hops=0)]
    for kw in kws:
        kw["level"] = kw["level"] if kw["level"] is not None else np.zeros(C, np.uint32)
        kw["node_count"] = kw["node_count"] if kw["node_count"] is not None else np.zeros(N, np.uint32)
    exp = [RPP.replan(c["grown"], c["nodes2"], c["prev"], **kw) for c, kw in zip(cs, kws)]
    cat = lambda f: np.concatenate([np.asarray(f(c, kw)) for c, kw in zip(cs, kws)])  # noqa: E731
    b = dict(cont=tuple(cat(lambda c, kw, i=i: c["grown"][i]) for i in range(4)),
             nodes=tuple(cat(lambda c, kw, i=i: c["nodes2"][i]) for i in range(5)), prev=cat(lambda c, kw: c["prev"]),
             strat=[kw["strategy"] for kw in kws], pref=[kw["preferred"] for kw in kws], level=cat(lambda c, kw: kw["level"]),
             cnt=cat(lambda c, kw: kw["node_count"]), dom=cat(lambda c, kw: kw["domain"]), skew=[kw["max_skew"] for kw in kws],
             relax=cat(lambda c, kw: np.array(_row4(kw["relax_mask"]), np.uint32)), nh=[kw["n_hops"] for kw in kws],
             quota=cat(lambda c, kw: np.array(kw["quota"], np.uint32)), used=cat(lambda c, kw: np.array(kw["quota_used"], np.uint32)))
    return S, C, N, b, exp


def _check_batch(g, exp, S, C, N, base):
    a, r, h, cost, chg, summ, after, nc, why, used = g
    for s in range(S):
        c, n, q = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N), slice(3 * s, 3 * s + 3)
        same((a[c], r[c], h[c], chg[c], summ[s], tuple(x[n] for x in after), nc[n], why[c], used[q]), exp[s])
        assert int(cost[s]) == RPP.cost(exp[s][0], exp[s][1], base + s)


def _host_batch(planner, S, C, N, b, base, **kw):
    return planner.replan_batch_policy(S, C, N, b["cont"], b["nodes"], b["prev"], b["strat"], b["quota"], b["used"], b["pref"],
                                       b["level"], b["cnt"], base, domain=b["dom"], max_skew=b["skew"], relax_mask=b["relax"],
                                       n_hops=b["nh"], **kw)


def test_batch_with_guarantees_switched_on_and_off_per_scenario(planner):
    S, C, N, b, exp = _batch3()
    _check_batch(_host_batch(planner, S, C, N, b, 40), exp, S, C, N, 40)
    g = _host_batch(planner, S, C, N, b, 40, want_hops=False, want_why=False, want_change=False, want_summary=False)
    assert g[2] is None and g[4] is None and g[5] is None and g[8] is None
    assert np.array_equal(g[0], np.concatenate([e[0] for e in exp])) and np.array_equal(g[9], np.concatenate([e[8] for e in exp]))
    assert all(e[4][KEPT] and (e[4][MOVED] or e[4][LOST]) for e in exp)


def _dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _pattern32(fill):
    return fill * 0x01010101 - (1 << 32) * (fill >= 0x80)


def _dev_prepare(planner, S, C, N, b, base=0, fill=0x5A, alias=False, plain=False, **over):
    """Copies of the inputs on the device, the outputs pre-filled with ``fill`` bytes, and the dev_replan_batch_policy
    call on them as a function.  ``alias``: prev is the assign buffer itself, filled with b's prev.  ``plain``: no
    domain, chain or quota (the call without a guarantee), hops_t still given."""
    import torch
    from fleetflow_amd.planner import DevBatch
    b = dict(b, **over)
    u32 = lambda x: _dev(np.asarray(x, np.uint32))  # noqa: E731
    f8 = lambda n: torch.full((n,), fill, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    db = DevBatch(S, C, N, base, *(_dev(x) for x in b["cont"]), u32(b["level"]), *(_dev(x) for x in b["nodes"][:4]),
                  _dev(np.asarray(b["nodes"][4], np.uint8)), torch.full((S * C,), _pattern32(fill), dtype=torch.int32, device="cuda:0"),
                  f8(S * C), torch.full((S,), fill * 0x0101010101010101 - (1 << 64) * (fill >= 0x80), dtype=torch.int64, device="cuda:0"))
    t = dict(cnt=u32(b["cnt"]), used=u32(b["used"]), hops=f8(S * C), why=f8(S * C), chg=f8(S * C),
             summ=torch.full((S * 8,), _pattern32(fill), dtype=torch.int32, device="cuda:0"))
    if alias:
        db.assign.copy_(u32(b["prev"]))
    ins = [db.assign if alias else u32(b["prev"]), u32(b["strat"]), None if plain else u32(b["quota"]), t["used"], u32(b["pref"]),
           t["cnt"]]
    kw = dict(hops_t=t["hops"], quota_why_t=t["why"], change_t=t["chg"], summary_t=t["summ"])
    if not plain:
        kw.update(domain_t=u32(b["dom"]), max_skew_t=u32(b["skew"]), relax_mask_t=u32(b["relax"]), n_hops_t=u32(b["nh"]))
    return db, t, lambda: planner.dev_replan_batch_policy(db, *ins, **kw)


def _dev_call(planner, S, C, N, b, base=0, fill=0x5A, **over):
    """dev_replan_batch_policy on copies of the inputs, the outputs pre-filled with ``fill`` bytes."""
    db, t, call = _dev_prepare(planner, S, C, N, b, base, fill, **over)
    call()
    return db, t


def _np_dev(db, t):
    u = lambda x: x.cpu().numpy().view(np.uint32)  # noqa: E731
    return (u(db.assign), db.reason.cpu().numpy(), t["hops"].cpu().numpy(), db.cost.cpu().numpy().view(np.uint64),
            t["chg"].cpu().numpy(), u(t["summ"]).reshape(db.S, 8), (u(db.cf), u(db.mf), u(db.lab), u(db.cu), db.sched.cpu().numpy()),
            u(t["cnt"]), t["why"].cpu().numpy(), u(t["used"]))


def test_device_entry_equals_the_host_entries(planner):
    S, C, N, b, exp = _batch3()
    db, t = _dev_call(planner, S, C, N, b, 40)
    planner.sync()
    got = _np_dev(db, t)
    _check_batch(got, exp, S, C, N, 40)
    host = _host_batch(planner, S, C, N, b, 40)
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9):
        assert np.array_equal(got[i], host[i]), i


def test_no_containers_and_no_scenarios(planner):
    S, C, N, b, _ = _batch3()
    empty = tuple(np.zeros(0, np.uint32) for _ in range(4))
    g = planner.replan_batch_policy(S, 0, N, empty, b["nodes"], [], b["strat"], b["quota"], b["used"], b["pref"], None, b["cnt"],
                                    7, domain=b["dom"], max_skew=b["skew"], relax_mask=b["relax"], n_hops=b["nh"])
    assert g[0].size == 0 and [int(x) for x in g[3]] == [7, 8, 9] and not g[5].any()
    assert np.array_equal(g[9], b["used"]) and np.array_equal(g[7], b["cnt"]) and np.array_equal(g[6][0], b["nodes"][0])
    a, r, h, chg, summ, after, nc, why, used = planner.replan_policy(empty, tuple(x[:N] for x in b["nodes"]), [], 1, [5, 5, 5],
                                                                     [1, 2, 3], RELAX, domain=b["dom"][:N], max_skew=1)
    assert a.size == 0 and not summ.any() and used.tolist() == [1, 2, 3]
    none = tuple(np.zeros(0, np.uint32) for _ in range(5))
    g = planner.replan_batch_policy(0, 5, 5, empty, none, [], [], [], [], domain=[], max_skew=[], relax_mask=[], n_hops=[])
    assert g[0].size == 0 and g[3].size == 0


def test_without_a_guarantee_it_is_fp_replan_with_zero_hops(planner):
    c = _case(21, 200, 139, False, False, False)
    kw = c["kw"]
    ref = planner.replan(c["grown"], c["nodes2"], c["prev"], kw["strategy"], kw["preferred"], kw["level"], kw["node_count"])
    g = planner.replan_policy(c["grown"], c["nodes2"], c["prev"], kw["strategy"], None, [4, 5, 6], None, kw["preferred"],
                              kw["level"], kw["node_count"])
    for i, j in ((0, 0), (1, 1), (3, 2), (4, 3)):
        assert np.array_equal(g[i], ref[j])
    assert not g[2].any() and not g[7].any() and g[8].tolist() == [4, 5, 6]  # hops zero; the usage is not touched
    _both(planner, c["grown"], c["nodes2"], c["prev"], kw)


# ---- errors: nothing is written --------------------------------------------------------------------------------------
def _raw_host(planner, c, kw, prev, strategy=None, alias=False, nodes=None):
    """fp_replan_policy itself, every output and in/out array pre-filled or kept: (rc, everything untouched?)."""
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32).copy()  # noqa: E731
    cont, prev = tuple(u32(x) for x in c["grown"]), u32(prev)
    nodes = nodes or c["nodes2"]
    nodes = tuple(u32(x) for x in nodes[:4]) + (np.ascontiguousarray(nodes[4], dtype=np.uint8).copy(),)
    C, N = prev.size, nodes[0].size
    cnt, used = np.full(N, 7, np.uint32), np.full(3, 0x600D, np.uint32)
    assign = prev if alias else np.full(C, 0xA5A5A5A5, np.uint32)
    b8 = [np.full(C, 0xA5, np.uint8) for _ in range(4)]  # reason, hops, why, change
    summ = np.full(8, 0xA5A5A5A5, np.uint32)
    dom, relax, quota = u32(np.resize(kw["domain"], N)), u32(_row4(kw["relax_mask"])), u32(kw["quota"])
    watched = (*nodes, cnt, used, assign, *b8, summ)
    before = [x.tobytes() for x in watched]
    cs = _lib.FpContainers(C, *(x.ctypes.data for x in cont))
    ns = _lib.FpNodes(N, *(x.ctypes.data for x in nodes))
    p = lambda a, t=_lib.u32p: a.ctypes.data_as(t)  # noqa: E731
    rc = planner._L.fp_replan_policy(planner._ctx, ct.byref(cs), ct.byref(ns), None, p(prev),
                                     kw["strategy"] if strategy is None else strategy, 0, p(cnt), p(dom), kw["max_skew"],
                                     p(relax), kw["n_hops"], p(assign), p(b8[0], _lib.u8p), p(b8[1], _lib.u8p), p(quota),
                                     p(used), p(b8[2], _lib.u8p), p(b8[3], _lib.u8p), p(summ))
    return rc, [x.tobytes() for x in watched] == before


def test_host_entry_errors_write_nothing(planner):
    c = _case(41, 200, 65)
    kw, prev = c["kw"], c["prev"]
    big = tuple(np.resize(x, 8193) for x in c["nodes2"])
    assert _raw_host(planner, c, kw, prev, nodes=big) == (_lib.FP_EOVERFLOW, True)
    assert _raw_host(planner, c, kw, prev, strategy=4) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, c, kw, prev, alias=True) == (_lib.FP_EINVAL, True)
    bad = prev.copy()
    bad[199] = 65
    assert _raw_host(planner, c, kw, bad) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, c, dict(kw, domain=np.where(np.arange(65) == 64, 64, kw["domain"])), prev) == (_lib.FP_EINVAL, True)
    assert _raw_host(planner, c, dict(kw, n_hops=5), prev) == (_lib.FP_EINVAL, True)
    # a domain out of range is legal where max_skew is 0, and the plain call is fine
    assert _raw_host(planner, c, dict(kw, domain=np.full(65, 64), max_skew=0), prev) == (_lib.FP_OK, False)
    assert _raw_host(planner, c, kw, prev) == (_lib.FP_OK, False)


def test_host_batch_entry_errors_write_nothing(planner):
    """fp_replan_batch_policy itself, on caller-owned buffers with a fill pattern: a bad value in one scenario of
    three leaves every scenario's outputs, node tables, counts and usage as they were."""
    S, C, N, b, _ = _batch3()
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32).copy()  # noqa: E731

    def call(**over):
        x = dict(b, **over)
        cont, prev = [u32(v) for v in x["cont"]], u32(x["prev"])
        nodes = [u32(v) for v in x["nodes"][:4]] + [np.ascontiguousarray(x["nodes"][4], np.uint8).copy()]
        cnt, used = u32(x["cnt"]), u32(x["used"])
        assign = prev if over.get("alias") else np.full(S * C, 0xA5A5A5A5, np.uint32)
        b8 = [np.full(S * C, 0xA5, np.uint8) for _ in range(4)]  # reason, hops, why, change
        summ, cost = np.full(S * 8, 0xA5A5A5A5, np.uint32), np.full(S, 0xA5A5A5A5A5A5A5A5, np.uint64)
        ins = [u32(x[k]) for k in ("strat", "pref", "dom", "skew", "relax", "nh", "quota", "level")]
        watched = (*nodes, cnt, used, assign, *b8, summ, cost)
        before = [v.tobytes() for v in watched]
        bt = _lib.FpBatch(S, 0, C, N, *(v.ctypes.data for v in cont), ins[7].ctypes.data, *(v.ctypes.data for v in nodes),
                          assign.ctypes.data, b8[0].ctypes.data, cost.ctypes.data)
        p = lambda a, t=_lib.u32p: a.ctypes.data_as(t)  # noqa: E731
        rc = planner._L.fp_replan_batch_policy(planner._ctx, ct.byref(bt), p(prev), p(ins[0]), p(ins[1]), p(cnt), p(ins[2]),
                                               p(ins[3]), p(ins[4]), p(ins[5]), p(b8[1], _lib.u8p), p(ins[6]), p(used),
                                               p(b8[2], _lib.u8p), p(b8[3], _lib.u8p), p(summ))
        return rc, [v.tobytes() for v in watched] == before

    bad_prev = b["prev"].copy()
    bad_prev[2 * C + 7] = N
    bad_dom = b["dom"].copy()
    bad_dom[5] = 64  # scenario 0, whose max_skew is not 0
    assert call(prev=bad_prev) == (_lib.FP_EINVAL, True)
    assert call(strat=[0, 0, 4]) == (_lib.FP_EINVAL, True)
    assert call(dom=bad_dom) == (_lib.FP_EINVAL, True)
    assert call(nh=[1, 5, 0]) == (_lib.FP_EINVAL, True)
    assert call(alias=True) == (_lib.FP_EINVAL, True)
    assert call() == (_lib.FP_OK, False)


def _dev_untouched(db, t, b, name, assign=None):
    a, r, h, cost, chg, summ, after, nc, why, used = _np_dev(db, t)
    assert np.array_equal(a, assign) if assign is not None else (a == 0xA5A5A5A5).all(), name
    assert all((x == 0xA5).all() for x in (r, h, chg, why)) and (summ == 0xA5A5A5A5).all(), name
    assert (cost == 0xA5A5A5A5A5A5A5A5).all() and np.array_equal(nc, b["cnt"]) and np.array_equal(used, b["used"]), name
    for i in range(5):
        assert np.array_equal(after[i], b["nodes"][i]), name


def test_device_entry_errors_write_nothing_and_the_context_goes_on(planner):
    S, C, N, b, exp = _batch3()
    bad_prev = b["prev"].copy()
    bad_prev[S * C - 1] = N
    bad_dom = b["dom"].copy()
    bad_dom[5] = 64  # scenario 0, whose max_skew is not 0
    cases = [("prev", dict(prev=bad_prev)), ("strategy", dict(strat=[0, 4, 0])), ("domain", dict(dom=bad_dom)),
             ("n_hops", dict(nh=[1, 0, 5]))]
    for name, over in cases:
        db, t = _dev_call(planner, S, C, N, b, fill=0xA5, **over)
        with pytest.raises(_lib.FleetplaceError) as e:
            planner.sync()
        assert e.value.code == _lib.FP_EINVAL, name
        _dev_untouched(db, t, b, name)
        planner.sync()  # reported once, then clear
    # the call without a guarantee has a check of its own in front of its zero fill of hops_t
    for name, over in cases[:2]:
        db, t = _dev_call(planner, S, C, N, b, fill=0xA5, plain=True, **over)
        with pytest.raises(_lib.FleetplaceError) as e:
            planner.sync()
        assert e.value.code == _lib.FP_EINVAL, name
        _dev_untouched(db, t, b, "no guarantee, " + name)
        planner.sync()
    # found on the host: the same buffer read and written (with and without a guarantee), too many nodes
    for plain in (False, True):
        db, t, call = _dev_prepare(planner, S, C, N, b, fill=0xA5, alias=True, plain=plain)
        with pytest.raises(_lib.FleetplaceError) as e:
            call()
        assert e.value.code == _lib.FP_EINVAL
        planner.sync()  # nothing was queued, nothing is pending
        _dev_untouched(db, t, b, "prev == assign", assign=b["prev"])
    big = dict(b, nodes=tuple(np.resize(x, S * 8193) for x in b["nodes"]), cnt=np.zeros(S * 8193, np.uint32),
               dom=np.zeros(S * 8193, np.uint32))
    with pytest.raises(_lib.FleetplaceError) as e:
        _dev_call(planner, S, C, 8193, big)
    assert e.value.code == _lib.FP_EOVERFLOW
    planner.sync()
    db, t = _dev_call(planner, S, C, N, b, 3)  # the context then completes a correct call
    planner.sync()
    _check_batch(_np_dev(db, t), exp, S, C, N, 3)


# ---- from KDL ------------------------------------------------------------------------------------------------------------
def _stage_text(placement, keyless=False):
    servers = "\n".join(
        f'server "n{i}" {{ capacity cpu={2000 + 1000 * (i % 3)} memory={4096 + 2048 * (i % 2)}; '
        + ("" if keyless and i == 7 else f'label "region={"tokyo" if i % 3 == 0 else "osaka"}"; ')
        + f'label "class={"gpu" if i % 4 == 1 else "cpu"}"' + ('; scheduling "cordon"' if i == 2 else "") + " }" for i in range(8))
    services = "\n".join(
        f'service "s{i}" {{ resources cpu={300 + 100 * (i % 4)} memory={512 * (1 + i % 3)}'
        + ('; require "class=gpu"' if i % 5 == 0 else "") + " }" for i in range(24))
    members = "\n".join(f'    service "s{i}"' for i in range(24)) + "\n" + "\n".join(f'    server "n{i}"' for i in range(8))
    return f'project "demo"\n{servers}\n{services}\nstage "live" {{\n{members}\n    {placement}\n}}\n'


PLACEMENT = ('placement strategy="spread_across_pool" { prefer "region=tokyo"; spread "region" max-skew=2; '
             'fallback "class" max-hops=1; quota cpu=11000 memory=40000 services=22 }')


def _reference_replan(flow, plan, pol, quota_used, keyless=False):
    from fleetflow_amd import flow as F
    names = list(flow.stages["live"].services)
    nodes = [flow.servers[s] for s in flow.stages["live"].servers]
    slugs = [n.slug for n in nodes]
    cont, ntab = F._stage_tables(names, flow, nodes, pol.preferred)
    ld = F._stage_labels(names, flow, nodes, pol.preferred)
    domain, has_key = F.replan_domains(nodes, pol.spread[0])
    ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
    prev = [slugs.index(plan.assignment[n]) if n in plan.assignment else NONE for n in names]
    e = RPP.replan(cont, ntab, prev, _lib.POLICY_STRATEGIES[pol.strategy], ld.mask(pol.preferred), None, None, domain,
                   pol.spread[1], [ld.key_mask(k) for k in pol.fallback], None, pol.quota, quota_used)
    return names, slugs, prev, e


@pytest.mark.parametrize("keyless", [False, True])
def test_replan_stage_under_policy_from_kdl(keyless, planner):
    from fleetflow_amd import flow as F
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_replan_report, replan_report_from_json, replan_report_to_json
    flow = parse_kdl_string(_stage_text(PLACEMENT, keyless))
    pol = flow.stages["live"].placement
    plan = F.plan_stage(flow, "live", planner, quota_used=(400, 0, 1))
    assert plan.quota == (11000, 40000, 22) and len(plan.assignment) >= 15 and "QUOTA" in plan.rejected.values()
    with pytest.raises(ValueError, match="would not be applied"):
        F.replan_stage(flow, "live", plan, planner)
    again = F.replan_stage(flow, "live", plan, planner, under_policy=True, quota_used=(400, 0, 1))
    assert sorted(again.kept) == sorted(plan.assignment) and not again.moved and not again.lost
    assert again.plan.relaxed.items() >= plan.relaxed.items() and again.plan.quota == plan.quota
    if "SKEW" not in plan.rejected.values():  # theorem D: only a SKEW rejection may be placed by the re-plan
        assert again.plan.assignment == plan.assignment and again.plan.quota_used == plan.quota_used and not again.new
    # two services grow; the re-plan against the reference, guarantees rebuilt from the plan
    flow.services["s5"].cpu_m = 3500
    flow.services["s2"].cpu_m = 1500
    rep = F.replan_stage(flow, "live", plan, planner, under_policy=True, quota_used=(400, 0, 1))
    names, slugs, prev, e = _reference_replan(flow, plan, pol, (400, 0, 1), keyless)
    assert rep.plan.assignment == {n: slugs[e[0][v]] for v, n in enumerate(names) if e[0][v] != NONE}
    assert rep.plan.rejected == {n: {1: "NOFIT", 3: "SKEW", 4: "QUOTA"}[int(e[1][v])] for v, n in enumerate(names) if e[0][v] == NONE}
    assert rep.kept == [n for v, n in enumerate(names) if e[3][v] == KEPT]
    assert rep.moved == [(n, slugs[prev[v]], slugs[e[0][v]]) for v, n in enumerate(names) if e[3][v] == MOVED]
    assert rep.plan.quota_used == tuple(int(x) for x in e[8]) and set(rep.plan.quota_why) == {n for v, n in enumerate(names) if e[1][v] == 4}
    why = {1: "NOFIT", 2: "CYCLE", 3: "SKEW", 4: "QUOTA"}
    assert rep.lost == [(n, slugs[prev[v]], why[int(e[1][v])]) for v, n in enumerate(names) if e[3][v] == LOST]
    assert rep.lost or rep.moved  # the grown requests cost someone a seat
    assert replan_report_from_json(replan_report_to_json(rep)) == rep
    assert format_replan_report(rep).startswith(f"replan live: {len(rep.kept)} kept, ")
    if keyless:  # n7 has no region: it keeps what ran on it and takes nothing new
        was = {n for n, s in plan.assignment.items() if s == "n7"}
        assert {n for n, s in rep.plan.assignment.items() if s == "n7"} <= was
