"""Re-planning under the policy (SPEC.md 2.14) without a GPU: theorems A to E on the numpy reference
(tests/replan_policy_ref.py) over random small cases, the conditions those cases must meet, hand-made cases for the
named traps (shared with the GPU tests), the Planner wrappers' length checks and what they send to which export,
``replan_stage(under_policy=True)`` through a reference-backed planner, and the report's text and JSON forms."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_quota_ref as QR  # noqa: E402
import replan_policy_ref as RPP  # noqa: E402
import replan_ref as RP  # noqa: E402
from test_replan_host import _addr, _cont, _flow, _nodes, _NoLib, _planner, _Rec, _refused  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402

NONE = 0xFFFFFFFF
UNL = 0xFFFFFFFF
KEPT, NEW, MOVED, LOST, ABSENT = RPP.KEPT, RPP.NEW, RPP.MOVED, RPP.LOST, RPP.ABSENT
CLASS, REGION, ZONE = 0b11, 0b1100, 0b110000  # three label keys of two values each; the chain gives up two
RELAX = (CLASS, REGION)


def same(got, exp):
    """(assign, reason, hops, change, summary, nodes_after, node_count_after, quota_why, quota_used_after)."""
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        assert np.array_equal(got[i], exp[i]), i
    for i in range(5):
        assert np.array_equal(got[5][i], exp[5][i]), ("node table", i)


def gen_case(seed, C, N, sp=True, fb=True, qt=True):
    """One scenario as the keyword arguments of replan_policy_ref.replan, with the plan it ran under: requests,
    a node table of 0.7 to 1.3 times the capacity the requests need (many times more for a large N), 10 % of the nodes
    cordoned; ``first`` = the 2.10 call's answer on it; then 15 % of the requests grow, a tenth of the seats is
    dropped, a twentieth points at some other node, and another tenth of the nodes is cordoned under what runs
    on them."""
    g = np.random.default_rng(seed)
    cpu = (g.integers(1, 9, C) * 100 * (g.random(C) > 0.05)).astype(np.uint32)
    mem = (g.integers(1, 5, C) * 128).astype(np.uint32)
    req = ((g.random(C) < 0.5) * (1 << g.integers(0, 2, C)) | (g.random(C) < 0.3) * (4 << g.integers(0, 2, C))
           | (g.random(C) < 0.1) * (16 << g.integers(0, 2, C))).astype(np.uint32)
    conf = ((g.random(C) < 0.2) * (1 << g.integers(0, 16, C))).astype(np.uint32)
    per = max(300, int((0.7 + 0.2 * (seed % 4)) * int(cpu.sum()) / (1.5 * N)) // 100 * 100)
    cf = (g.integers(0, 4, N) * per).astype(np.uint32)
    mf = (g.integers(1, 4, N) * max(512, int(mem.sum()) // N)).astype(np.uint32)
    lab = ((1 << g.integers(0, 2, N)) | (4 << g.integers(0, 2, N)) | (16 << g.integers(0, 2, N))).astype(np.uint32)
    cu = np.zeros(N, np.uint32)
    sched = (g.random(N) > 0.1).astype(np.uint8)
    D = min(6, N)
    kw = dict(strategy=int(seed % 4), preferred=int(g.integers(0, 64)) if seed % 3 else 0,
              level=np.where(g.random(C) < 0.04, NONE, 1).astype(np.uint32) if seed % 2 else None,
              node_count=g.integers(0, 3, N).astype(np.uint32) if seed % 5 < 3 else None)
    if sp:
        kw.update(domain=g.integers(0, D, N).astype(np.uint32), max_skew=int(1 + seed % 3))
    if fb:
        kw.update(relax_mask=RELAX, n_hops=int(1 + seed % 2))
    if qt:
        frac = 0.4 + 0.2 * (seed % 3)  # tight caps: the quota refuses early, while nodes still fill up
        # the visiting order is by cpu, so the cpu cap refuses the large requests first; a memory or a service
        # cap that bites after it is what makes a QUOTA container's mask grow on the final usage
        caps = [int(frac * int(cpu.sum())), UNL if seed % 2 else int((0.25 + 0.1 * (seed // 2 % 3)) * int(mem.sum())),
                int(C * (0.3 + 0.15 * (seed // 3 % 3)))]
        kw.update(quota=caps, quota_used=[int(g.integers(0, 300)), int(g.integers(0, 300)), int(g.integers(0, 3))])
    cont, nodes = (cpu, mem, req, conf), (cf, mf, lab, cu, sched)
    first = QR.place(cont, nodes, kw["strategy"], kw.get("quota", [UNL] * 3), kw.get("quota_used"),
                     preferred=kw["preferred"], level=kw["level"], node_count=kw["node_count"],
                     domain=kw.get("domain"), max_skew=kw.get("max_skew", 0), relax_mask=kw.get("relax_mask", ()),
                     n_hops=kw.get("n_hops", 0))
    grow = g.random(C) < 0.15
    cpu2 = cpu.copy()
    cpu2[grow] = cpu2[grow] * 3 // 2 + 100
    prev = first[0].copy()
    prev[g.random(C) < 0.1] = NONE
    stray = g.random(C) < 0.05
    prev[stray] = g.integers(0, N, int(stray.sum()))
    sched2 = (sched & (g.random(N) > 0.1)).astype(np.uint8)
    for a in (cpu, cpu2, mem, req, conf, cf, mf, lab, cu, sched, sched2, prev):
        a.setflags(write=False)
    return dict(cont=cont, nodes=nodes, first=first, grown=(cpu2, mem, req, conf), nodes2=(cf, mf, lab, cu, sched2),
                prev=prev, kw=kw)


@functools.lru_cache(maxsize=None)
def small_cases():
    return [gen_case(s, 24 + s % 17, 5 + s % 9) for s in range(200)]


# ---- theorems A to E on the reference --------------------------------------------------------------------------
def test_theorem_a_without_a_guarantee_it_is_2_13():
    for s in range(40):
        c = gen_case(s, 30, 7, sp=False, fb=False, qt=False)
        kw = c["kw"]
        exp = RP.replan(c["grown"], c["nodes2"], c["prev"], kw["strategy"], kw["preferred"], kw["level"], kw["node_count"])
        idle = [{}, dict(domain=np.zeros(7, np.uint32), max_skew=0), dict(relax_mask=(0xFFFFFFFF,) * 4, n_hops=0),
                dict(quota=[UNL] * 3), dict(domain=np.full(7, 99, np.uint32), max_skew=0, relax_mask=RELAX, n_hops=0,
                                            quota=[UNL, None, UNL])]
        for extra in idle:
            got = RPP.replan(c["grown"], c["nodes2"], c["prev"], **kw, **extra)
            assert all(np.array_equal(got[i], exp[j]) for i, j in ((0, 0), (1, 1), (3, 2), (4, 3), (6, 5)))
            assert all(np.array_equal(x, y) for x, y in zip(got[5], exp[4]))
            assert not got[2].any() and not got[7].any()


def test_theorem_b_without_a_prev_it_is_2_10():
    for c in small_cases()[:60]:
        kw = c["kw"]
        got = RPP.replan(c["grown"], c["nodes2"], np.full(c["prev"].size, NONE), **kw)
        a, r, h, after, cnt, why, used = QR.place(c["grown"], c["nodes2"], kw["strategy"], kw["quota"], kw["quota_used"],
                                                  preferred=kw["preferred"], level=kw["level"],
                                                  node_count=kw["node_count"], domain=kw["domain"],
                                                  max_skew=kw["max_skew"], relax_mask=kw["relax_mask"], n_hops=kw["n_hops"])
        same(got, (a, r, h, np.where(a != NONE, NEW, ABSENT), got[4], after, cnt, why, used))
        assert RPP.cost(got[0], got[1], 3) == QR.cost(a, r, 3)


def test_theorem_c_joint_feasibility_keeps_every_seat_and_a_replan_is_kept_by_the_next():
    for c in small_cases()[:60]:
        one = RPP.replan(c["grown"], c["nodes2"], c["prev"], **c["kw"])
        two = RPP.replan(c["grown"], c["nodes2"], one[0], **c["kw"])
        placed = one[0] != NONE
        assert (two[3][placed] == KEPT).all() and np.array_equal(two[0][placed], one[0][placed])
        assert np.array_equal(two[2][placed], one[2][placed])  # the same hop


def test_theorem_d_fixed_point_as_far_as_it_goes():
    skew_placed = nofit_to_quota = why_grew = 0
    for c in small_cases():
        kw = c["kw"]
        a, r, h, after, cnt, why, used = c["first"]
        got = RPP.replan(c["cont"], c["nodes"], a, **kw)
        placed = a != NONE
        assert (got[3][placed] == KEPT).all() and np.array_equal(got[0][placed], a[placed])
        assert np.array_equal(got[2][placed], h[placed])
        assert np.array_equal(got[1] == 2, r == 2)  # CYCLE stays CYCLE
        q = r == 4
        assert (got[1][q] == 4).all() and ((got[7][q] & why[q]) == why[q]).all()  # QUOTA stays, why is a superset
        nf = r == 1
        assert np.isin(got[1][nf], (1, 4)).all()  # NOFIT stays rejected, as NOFIT or QUOTA
        sk = r == 3
        skew_placed += int((got[0][sk] != NONE).sum())
        nofit_to_quota += int((got[1][nf] == 4).sum())
        why_grew += int((got[7][q] != why[q]).sum())
        if not sk.any():
            assert np.array_equal(got[0], a) and np.array_equal(got[6], cnt) and np.array_equal(got[8], used)
            assert all(np.array_equal(x, y) for x, y in zip(got[5], after))
    # the weak cases all occur: a condition on the inputs
    assert skew_placed > 0 and nofit_to_quota > 0 and why_grew > 0, (skew_placed, nofit_to_quota, why_grew)


def test_theorem_e_a_lost_seat_is_never_taken_again():
    for c in small_cases():
        got = RPP.replan(c["grown"], c["nodes2"], c["prev"], **c["kw"])
        had = c["prev"] != NONE
        assert np.array_equal(got[3] == KEPT, had & (got[0] == c["prev"]))
        moved = got[3] == MOVED
        assert (got[0][moved] != c["prev"][moved]).all()


def test_the_random_cases_meet_their_conditions():
    over_cap = relaxed_seat = cordoned_seat = 0
    for c in small_cases():
        kw = c["kw"]
        got = RPP.replan(c["grown"], c["nodes2"], c["prev"], **kw)
        over_cap += any(u > q for u, q in zip(RPP.replan.after_seats, kw["quota"]) if q != UNL)
        kept = got[3] == KEPT
        relaxed_seat += int((kept & (got[2] > 0)).sum())
        cordoned_seat += int((c["nodes2"][4][got[0][kept]] == 0).sum())
    assert over_cap > 0 and relaxed_seat > 0 and cordoned_seat > 0, (over_cap, relaxed_seat, cordoned_seat)


# ---- the named traps, by hand (the GPU tests run them through the ABI) -----------------------------------------
def _hand():
    cases = []
    # quota: the seats put cpu above its cap; every non-zero cpu request is QUOTA, a zero one is admitted
    cases.append(("seats above a cap in one dimension",
                  _cont([600, 500, 300, 0, 200]), _nodes([1000, 1000, 1000]), [0, 1, NONE, NONE, NONE],
                  dict(quota=[1000, UNL, 10], quota_used=[50, 7, 1]),
                  dict(assign=[0, 1, NONE, 0, NONE], reason=[0, 0, 4, 0, 4], why=[0, 0, 1, 0, 1], used=[1150, 10, 4])))
    cases.append(("usage after the seats exactly at the cap",
                  _cont([600, 400, 1, 0]), _nodes([1000, 1000]), [0, 1, NONE, NONE],
                  dict(quota=[1000, UNL, UNL], quota_used=[0, 0, 0]),
                  dict(assign=[0, 1, NONE, 0], reason=[0, 0, 4, 0], why=[0, 0, 1, 0], used=[1000, 3, 3])))
    cases.append(("an unlimited dimension still accumulates",
                  _cont([5, 4], mem=[30, 20]), _nodes([10, 10]), [1, NONE],
                  dict(quota=[UNL, UNL, 2], quota_used=[0xFFFFFFFE, 100, 0]),
                  dict(assign=[1, 0], reason=[0, 0], why=[0, 0], used=[7, 150, 2])))
    cases.append(("quota_used absent", _cont([5, 4, 3]), _nodes([10, 10]), [1, NONE, NONE],
                  dict(quota=[9, UNL, UNL]), dict(assign=[1, 0, NONE], reason=[0, 0, 4], why=[0, 0, 1], used=[9, 2, 2])))
    # spread: three seats in domain 0, beyond max_skew; pass 2 fills the other domains first
    cases.append(("seats all in one domain",
                  _cont([9, 8, 7, 6, 5, 4]), _nodes([100] * 4), [0, 0, 0, NONE, NONE, NONE],
                  dict(domain=[0, 0, 1, 2], max_skew=1),
                  dict(assign=[0, 0, 0, 2, 3, 2], reason=[0] * 6)))
    # a domain whose only node is cordoned keeps its seat and is not eligible: the minimum is over domains 0, 1
    cases.append(("a cordoned domain keeps its seats and is not eligible",
                  _cont([9, 8, 7, 6]), _nodes([100] * 3, sched=[1, 1, 0]), [2, NONE, NONE, NONE],
                  dict(domain=[0, 1, 2], max_skew=1, node_count=[0, 0, 5]),
                  dict(assign=[2, 0, 1, 0], reason=[0] * 4, count=[2, 1, 6])))
    # chain: node 0 carries neither the class nor the region bit asked for; kept at hop 2
    cases.append(("a seat kept at hop 2",
                  _cont([5, 5], req=[0b0101, 0b0101]), _nodes([100, 100], lab=[0b1010, 0b0101]), [0, NONE],
                  dict(relax_mask=RELAX, n_hops=2), dict(assign=[0, 1], reason=[0, 0], hops=[2, 0])))
    cases.append(("a seat lost on a label the chain keeps",
                  _cont([5], req=[0b010001]), _nodes([100, 100], lab=[0b100010, 0b010010]), [0],
                  dict(relax_mask=RELAX, n_hops=2), dict(assign=[1], reason=[0], hops=[1], change=[MOVED])))
    cases.append(("n_hops 0 with junk in relax_mask",
                  _cont([5, 5], req=[1, 1]), _nodes([100, 100], lab=[2, 1]), [0, 1],
                  dict(relax_mask=(0xFFFFFFFF,) * 4, n_hops=0), dict(assign=[1, 1], reason=[0, 0], hops=[0, 0])))
    cases.append(("a container that requires none of the relaxable labels",
                  _cont([5, 5], req=[0b10000, 0b10000]), _nodes([100, 100], lab=[0b100000, 0b010000]), [0, NONE],
                  dict(relax_mask=RELAX, n_hops=2), dict(assign=[1, 1], reason=[0, 0], hops=[0, 0])))
    return cases


HAND_POLICY_CASES = _hand()


@pytest.mark.parametrize("case", HAND_POLICY_CASES, ids=[c[0] for c in HAND_POLICY_CASES])
def test_hand_made_cases_on_the_reference(case):
    _, cont, nodes, prev, kw, exp = case
    got = RPP.replan(cont, nodes, prev, **kw)
    assert got[0].tolist() == exp["assign"] and got[1].tolist() == exp["reason"]
    for key, i in (("hops", 2), ("change", 3), ("count", 6), ("why", 7), ("used", 8)):
        if key in exp:
            assert got[i].tolist() == exp[key], key


# ---- the wrappers ------------------------------------------------------------------------------------------------
def test_replan_policy_length_checks():
    p = _planner(_NoLib())
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    _refused("prev must hold C entries", p.replan_policy, cont, nodes, [0])
    _refused("level must hold C entries", p.replan_policy, cont, nodes, [0, 0], level=[0])
    _refused("node_count must hold N entries", p.replan_policy, cont, nodes, [0, 0], node_count=[0] * 4)
    _refused("domain must hold N entries", p.replan_policy, cont, nodes, [0, 0], domain=[0, 0], max_skew=1)
    _refused("relax_mask holds at most", p.replan_policy, cont, nodes, [0, 0], relax_mask=[1] * 5)
    _refused("quota must hold 1 rows of 3 u32 caps", p.replan_policy, cont, nodes, [0, 0], quota=[1, 2, 3, 4, 5, 6])
    _refused("quota_used must hold 3 entries", p.replan_policy, cont, nodes, [0, 0], quota=[1, 2, 3], quota_used=[0])
    b = (2, 2, 3, tuple(np.tile(x, 2) for x in cont), tuple(np.tile(x, 2) for x in nodes))
    _refused("prev must hold S * C entries", p.replan_batch_policy, *b, [0, 0], [0, 0])
    _refused("strategy and preferred must hold S entries", p.replan_batch_policy, *b, [0] * 4, [0])
    _refused("domain must hold S * N and max_skew S entries", p.replan_batch_policy, *b, [0] * 4, [0, 0],
             domain=[0] * 6, max_skew=[1])
    _refused("relax_mask must hold S * FP_FALLBACK_MAX_HOPS and n_hops S entries", p.replan_batch_policy, *b, [0] * 4,
             [0, 0], relax_mask=[0] * 8, n_hops=[1])
    _refused("quota must hold 2 rows of 3 u32 caps", p.replan_batch_policy, *b, [0] * 4, [0, 0], quota=[1, 2, 3])
    _refused("quota_used must hold S * 3 entries", p.replan_batch_policy, *b, [0] * 4, [0, 0], quota=[1] * 6, quota_used=[0])


def test_replan_policy_call():
    lib = _Rec(peek={4: 2, 8: 3, 10: 4, 15: 3, 16: 3})
    p = _planner(lib)
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    out = p.replan_policy(cont, nodes, [2, NONE], "fill_lowest", [5, None, 7], [1, 2, 3], [3, 12], -1, [0, NONE],
                          [4, 5, 6], domain=[0, 1, 2], max_skew=2)
    (name, args, seen), = lib.calls
    assert name == "fp_replan_policy" and len(args) == 20 == len(_lib.SIGNATURES[name][1]) and _addr(args[0]) == 0x5EED
    assert seen == {4: [2, NONE], 8: [0, 1, 2], 10: [3, 12, 0, 0], 15: [5, UNL, 7], 16: [1, 2, 3]}
    assert args[5:7] == (_lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF) and args[9] == 2 and args[11] == 2
    assign, reason, hops, change, summary, after, nc, why, used = out
    assert [_addr(args[i]) for i in (7, 12, 13, 14, 16, 17, 18, 19)] == [
        x.ctypes.data for x in (nc, assign, reason, hops, used, why, change, summary)]
    lib = _Rec()
    p = _planner(lib)
    out = p.replan_policy(cont, nodes, [0, 1], want_hops=False, want_why=False, want_used=False, want_change=False,
                          want_summary=False)
    args = lib.calls[0][1]
    assert [_addr(args[i]) for i in (3, 7, 8, 10, 14, 15, 16, 17, 18, 19)] == [0] * 10 and args[9] == 0 and args[11] == 0
    assert out[2] is None and out[3] is None and out[4] is None and out[7] is None and out[8] is None


def test_replan_batch_policy_call():
    lib = _Rec(peek={2: 4, 3: 2, 6: 6, 7: 2, 8: 8, 9: 2, 11: 6, 12: 6})
    p = _planner(lib)
    cont, nodes = tuple(np.tile(x, 2) for x in _cont([1, 1])), tuple(np.tile(x, 2) for x in _nodes([9, 9, 9]))
    out = p.replan_batch_policy(2, 2, 3, cont, nodes, [0, NONE, 2, 1], ["pack_into_dedicated", 1], [1, 2, 3, 4, 5, 6],
                                [9] * 6, scen_base=5, domain=[0, 1, 2] * 2, max_skew=[1, 0], relax_mask=[3, 12, 0, 0] * 2,
                                n_hops=[2, 0])
    (name, args, seen), = lib.calls
    assert name == "fp_replan_batch_policy" and len(args) == 16 == len(_lib.SIGNATURES[name][1])
    assert seen == {2: [0, NONE, 2, 1], 3: [_lib.STRATEGY_PACK, 1], 6: [0, 1, 2] * 2, 7: [1, 0], 8: [3, 12, 0, 0] * 2,
                    9: [2, 0], 11: [1, 2, 3, 4, 5, 6], 12: [9] * 6}
    assign, reason, hops, cost, change, summary, after, nc, why, used = out
    b = args[1]._obj
    assert (b.n_scen, b.scen_base, b.assign, b.cost) == (2, 5, assign.ctypes.data, cost.ctypes.data)
    assert [_addr(args[i]) for i in (10, 12, 13, 14, 15)] == [x.ctypes.data for x in (hops, used, why, change, summary)]
    assert summary.shape == (2, 8) and nc is None


def test_dev_replan_batch_policy_call_and_checks():
    torch = pytest.importorskip("torch")
    from fleetflow_amd.planner import DevBatch
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    S, C, N = 2, 3, 4
    db = DevBatch.allocate(S, C, N, "cpu", scen_base=3)
    prev, st, qt, qu, pf, cnt = i32(S * C), i32(S), i32(S * 3), i32(S * 3), i32(S), i32(S * N)
    dom, sk, rm, nh, hp, wy, chg, sm = i32(S * N), i32(S), i32(S * 4), i32(S), u8(S * C), u8(S * C), u8(S * C), i32(S * 8)
    lib = _Rec()
    q = _planner(lib)
    q.dev_replan_batch_policy(db, prev, st, qt, qu, pf, cnt, domain_t=dom, max_skew_t=sk, relax_mask_t=rm, n_hops_t=nh,
                              hops_t=hp, quota_why_t=wy, change_t=chg, summary_t=sm)
    (name, args, _), = lib.calls
    assert name == "fp_dev_replan_batch_policy" and len(args) == 16 == len(_lib.SIGNATURES[name][1])
    assert [_addr(a) for a in args[2:]] == [t.data_ptr() for t in (prev, st, pf, cnt, dom, sk, rm, nh, hp, qt, qu, wy, chg, sm)]
    q.dev_replan_batch_policy(db, prev, st, domain_t=dom)  # half a pair is no pair
    assert [_addr(a) for a in lib.calls[1][1][4:]] == [0] * 12
    fn = _planner(_NoLib()).dev_replan_batch_policy
    _refused("prev_t must hold S * C 32-bit entries", fn, db, i32(S * C - 1), st)
    _refused("quota_t and quota_used_t must hold S * 3 32-bit entries", fn, db, prev, st, i32(S * 3 + 1))
    _refused("quota_why_t must hold S * C bytes", fn, db, prev, st, quota_why_t=i32(S * C))
    _refused("hops_t must hold S * C bytes", fn, db, prev, st, hops_t=u8(S * C + 1))
    _refused("change_t must hold S * C bytes", fn, db, prev, st, change_t=i32(S * C))
    _refused("summary_t must hold S * 8 32-bit entries", fn, db, prev, st, summary_t=i32(S * 8 - 1))


def test_abi_declares_the_replan_policy_entries_everywhere():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fleetplace.h")).read()
    for name in ("fp_replan_policy", "fp_replan_batch_policy", "fp_dev_replan_batch_policy"):
        assert f"int {name}(fp_ctx *ctx" in hdr and name in _lib.SIGNATURES


# ---- the flow level ------------------------------------------------------------------------------------------------
class _RefPolicyPlanner:
    """replan_policy answered by the numpy reference, the graph by the Python oracle; remembers what it was asked."""

    def plan_stage(self, row_ptr, col, has_deps, cont=None, nodes=None):
        from oracle import pyoracle as P
        level, order = P.levelize(len(has_deps), list(row_ptr), list(col), list(has_deps))
        return np.array(P.legacy_order(has_deps)), np.array(level, np.uint32), np.array(order), 0, None

    def replan(self, *a, **kw):
        raise AssertionError("under the policy the call is replan_policy")

    def replan_policy(self, cont, nodes, prev, strategy=0, quota=None, quota_used=None, relax_mask=None, preferred=0,
                      level=None, node_count=None, *, domain=None, max_skew=0):
        self.asked = dict(nodes=nodes, prev=prev, quota=quota, quota_used=quota_used, relax_mask=relax_mask,
                          domain=domain, max_skew=max_skew, strategy=strategy)
        return RPP.replan(cont, nodes, prev, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred, level, node_count,
                          domain, max_skew, relax_mask or (), None, quota, quota_used)


POLICY = dict(strategy="spread_across_pool", spread_topology_key="region", spread_max_skew=1,
              fallback_relax_order=("class",), quota_cpu_m=9000, quota_services=6)


def _policy_plan(f, pol, quota_used=(0, 0, 0)):
    """The stage's first plan under ``pol`` by the 2.10 reference, as plan_stage would fill it."""
    stage = f.stages["live"]
    nodes = [f.servers[s] for s in stage.servers]
    cont, ntab = F._stage_tables(stage.services, f, nodes, pol.preferred)
    ld = F._stage_labels(stage.services, f, nodes, pol.preferred)
    domain, has_key = F.spread_domains(nodes, pol.spread[0])
    ntab = (*ntab[:4], [s if k else 0 for s, k in zip(ntab[4], has_key)])
    a, r, h, _, _, _, used = QR.place(cont, ntab, _lib.POLICY_STRATEGIES[pol.strategy], [UNL if q is None else q for q in pol.quota],
                                      quota_used, domain=domain, max_skew=pol.spread[1],
                                      relax_mask=[ld.key_mask(k) for k in pol.fallback])
    plan = F.Plan("live", [], {}, [], {n: stage.servers[a[v]] for v, n in enumerate(stage.services) if a[v] != NONE},
                  {n: {1: "NOFIT", 3: "SKEW", 4: "QUOTA"}[int(r[v])] for v, n in enumerate(stage.services) if a[v] == NONE})
    plan.strategy, plan.preferred = pol.strategy, pol.preferred
    plan.spread_topology_key, plan.spread_max_skew = pol.spread
    plan.fallback_relax_order, plan.fallback_max_hops = list(pol.fallback_relax_order), pol.fallback_max_hops
    plan.quota, plan.quota_used = pol.quota, tuple(int(x) for x in used)
    return plan


def test_replan_stage_default_still_refuses():
    f = _flow()
    pol = F.PlacementPolicy(**POLICY)
    plan = _policy_plan(f, pol)
    with pytest.raises(ValueError, match="would not be applied"):
        F.replan_stage(f, "live", plan, planner=_RefPolicyPlanner())
    with pytest.raises(ValueError, match="would not be applied"):
        F.replan_stage(f, "live", plan, planner=_RefPolicyPlanner(), policy=pol, under_policy=False, quota_used=(1, 2, 3))


def test_replan_stage_under_policy_rebuilds_the_guarantees_from_the_plan():
    f = _flow()
    pol = F.PlacementPolicy(**POLICY)
    plan = _policy_plan(f, pol, (500, 0, 0))
    assert len(plan.assignment) == 6
    p = _RefPolicyPlanner()
    rep = F.replan_stage(f, "live", plan, planner=p, under_policy=True, quota_used=(500, 0, 0))
    assert sorted(rep.kept) == sorted(plan.assignment) and not (rep.moved or rep.lost or rep.new)
    assert p.asked["quota"] == (9000, None, 6) and p.asked["quota_used"] == (500, 0, 0)  # not plan.quota_used
    assert p.asked["domain"] == [0, 0, 1, 1] and p.asked["max_skew"] == 1
    ld = F._stage_labels(f.stages["live"].services, f, [f.servers[s] for s in f.stages["live"].servers])
    assert p.asked["relax_mask"] == [ld.key_mask("class")]
    new = rep.plan
    assert (new.spread_topology_key, new.spread_max_skew, new.fallback_relax_order, new.quota) == (
        "region", 1, ["class"], (9000, None, 6))
    assert new.quota_used == plan.quota_used == (500 + 8250, 8832, 6) and new.assignment == plan.assignment
    assert rep.skew_excess is None and rep.quota_over == []
    # the same guarantees through an explicit policy; the default base is zero
    rep2 = F.replan_stage(f, "live", plan, planner=p, policy=pol, under_policy=True)
    assert p.asked["quota_used"] == (0, 0, 0) and rep2.plan.quota_used == (8250, 8832, 6)
    # grow one request: over the cpu cap with the base, so the grown service is lost to the quota
    f.services["cache"].cpu_m = 2100
    rep3 = F.replan_stage(f, "live", plan, planner=p, under_policy=True, quota_used=(500, 0, 0))
    assert [x[0] for x in rep3.lost] == ["cache"] and rep3.lost[0][2] == "QUOTA"
    assert rep3.plan.rejected == {"cache": "QUOTA"} and rep3.plan.quota_why == {"cache": ["cpu"]}
    text = PO.format_replan_report(rep3)
    assert "lost (QUOTA)" in text and "spread:" not in text and "quota:" not in text
    assert PO.replan_report_from_json(PO.replan_report_to_json(rep3)) == rep3
    assert "skew_excess" not in PO.replan_report_to_json(rep3) and "quota_over" not in PO.replan_report_to_json(rep3)


def test_replan_stage_reports_what_the_seats_leave_outside_the_guarantees():
    f = _flow()
    plan = F.Plan("live", [], {}, [], {n: "a1" if n != "db" else "a2" for n in ("api", "cache", "cron")}, {})
    plan.assignment = {"api": "a1", "cache": "a1", "cron": "a1"}
    pol = F.PlacementPolicy(spread_topology_key="region", spread_max_skew=1, quota_cpu_m=1500)
    f.stages["live"].services = ["api", "cache", "cron"]
    rep = F.replan_stage(f, "live", plan, planner=_RefPolicyPlanner(), policy=pol, under_policy=True)
    assert rep.kept == ["api", "cache", "cron"] and rep.skew_excess == 3 and rep.quota_over == ["cpu"]
    assert rep.plan.quota_used == (1750, 3200, 3)
    text = PO.format_replan_report(rep)
    assert "spread: skew 3 over region exceeds max_skew 1" in text and "quota: usage above the cap in cpu" in text
    back = PO.replan_report_from_json(PO.replan_report_to_json(rep))
    assert back == rep and back.skew_excess == 3 and back.quota_over == ["cpu"]


def test_keyless_servers_get_a_spare_domain_and_64_values_leave_none():
    f = _flow()
    f.servers["b2"].labels = []  # no region
    p = _RefPolicyPlanner()
    plan = F.Plan("live", [], {}, [], {"cron": "b2"}, {})
    pol = F.PlacementPolicy(spread_topology_key="region", spread_max_skew=1)
    rep = F.replan_stage(f, "live", plan, planner=p, policy=pol, under_policy=True)
    assert p.asked["domain"] == [0, 0, 1, 2] and [int(x) for x in p.asked["nodes"][4]] == [1, 1, 1, 0]
    assert "cron" in rep.kept and rep.plan.assignment["cron"] == "b2"  # the seat stays; nothing new goes there
    assert all(s != "b2" for n, s in rep.plan.assignment.items() if n != "cron")
    assert F.spread_domains([f.servers[s] for s in f.stages["live"].servers], "region")[0] == [0, 0, 1, 0]
    servers = [F.Server(f"n{i}", 1000, 1000, [f"region=r{i}"]) for i in range(64)]
    assert F.replan_domains(servers, "region")[0] == list(range(64))
    with pytest.raises(ValueError, match="spare domain id"):
        F.replan_domains(servers + [F.Server("bare", 1000, 1000, [])], "region")
    assert F.replan_domains(servers[:63] + [F.Server("bare", 1000, 1000, [])], "region")[0] == list(range(63)) + [63]
