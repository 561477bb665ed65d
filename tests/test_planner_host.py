"""Host-side argument checks of the Python mirror (no GPU): every host-pointer call reads its arrays
for the lengths its sizes imply, so a short array is refused with ValueError before the library is
called -- the Rust binding's FP_EINVAL checks (integration/fleetflow-placement/src/lib.rs plan_stage,
place, place_batch).  ADVICE r05: Planner.plan_stage took V from has_deps and memcpy'd (V + 1) words
of row_ptr and V of each container field without checking."""
import ctypes as ct
import re

import numpy as np
import pytest

from fleetflow_amd import _lib
from fleetflow_amd.planner import Planner


class _NoLib:
    def __getattr__(self, name):  # any library call would be a failed check
        raise AssertionError(f"library called: {name}")


@pytest.fixture
def p():
    q = object.__new__(Planner)  # no context, no device: the checks come first
    q._L = _NoLib()
    return q


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def test_plan_stage_row_ptr_length(p):
    with pytest.raises(ValueError, match="row_ptr"):
        p.plan_stage([0, 0], [], [0, 0])
    with pytest.raises(ValueError, match="row_ptr"):
        p.levelize([0, 0, 0, 0], [], [0, 0])


def test_plan_stage_container_and_node_lengths(p):
    rp, col, hd = [0, 0, 0], [], [0, 0]
    nodes = _u([9], [9], [0], [0]) + (np.ones(1, np.uint8),)
    with pytest.raises(ValueError, match="container"):
        p.plan_stage(rp, col, hd, _u([1], [1], [0], [0]), nodes)
    with pytest.raises(ValueError, match="node"):
        p.plan_stage(rp, col, hd, _u([1, 1], [1, 1], [0, 0], [0, 0]), _u([9], [9], [0, 0], [0]) + (np.ones(1, np.uint8),))


def test_place_and_batch_lengths(p):
    nodes = _u([9], [9], [0], [0]) + (np.ones(1, np.uint8),)
    with pytest.raises(ValueError, match="container"):
        p.place(_u([1, 1], [1], [0, 0], [0, 0]), nodes)
    with pytest.raises(ValueError, match="level"):
        p.place(_u([1], [1], [0], [0]), nodes, level=[0, 0])
    with pytest.raises(ValueError, match="node"):
        p.place(_u([1], [1], [0], [0]), _u([9], [9], [0], [0]) + (np.ones(2, np.uint8),))
    with pytest.raises(ValueError, match="container"):
        p.place_batch(2, 1, 1, _u([1], [1], [0], [0]), _u([9, 9], [9, 9], [0, 0], [0, 0]) + (np.ones(2, np.uint8),))
    with pytest.raises(ValueError, match="node"):
        p.place_batch(1, 1, 2, _u([1], [1], [0], [0]), nodes)


# ---- the scored-placement wrappers: length checks and what reaches the C exports -------------------
# Characterisation of the six host policy methods and the three dev_* ones: which export each calls, the
# scalars and null pointers it sends, and that a short array is refused before any library call.

def _cont(n):
    return _u([1] * n, [1] * n, [0] * n, [0] * n)


def _nodes(n):
    return _u([9] * n, [9] * n, [0] * n, [0] * n) + (np.ones(n, np.uint8),)


def _short(t, i):
    return t[:i] + (t[i][:-1],) + t[i + 1:]


_SINGLE = {
    "place_policy": lambda p, cont, nodes, **kw: p.place_policy(cont, nodes, "fill_lowest", **kw),
    "place_policy_fallback": lambda p, cont, nodes, **kw: p.place_policy_fallback(
        cont, nodes, 1, **{"relax_mask": [1], **kw}),
    "place_policy_quota": lambda p, cont, nodes, **kw: p.place_policy_quota(
        cont, nodes, 1, **{"quota": (5, None, 3), **kw}),
}
_BATCH = {
    "place_batch_policy": lambda p, S, C, N, cont, nodes, **kw: p.place_batch_policy(
        S, C, N, cont, nodes, [1] * S, **kw),
    "place_batch_policy_fallback": lambda p, S, C, N, cont, nodes, **kw: p.place_batch_policy_fallback(
        S, C, N, cont, nodes, [1] * S, **kw),
    "place_batch_policy_quota": lambda p, S, C, N, cont, nodes, **kw: p.place_batch_policy_quota(
        S, C, N, cont, nodes, [1] * S, **{"quota": [5, 6, 7] * S, **kw}),
}


def _refused(msg, fn, *a, **kw):
    with pytest.raises(ValueError, match=msg and re.escape(msg)):
        fn(*a, **kw)


@pytest.mark.parametrize("name", list(_SINGLE))
@pytest.mark.parametrize("C,N", [(1, 2), (2, 1), (2, 2)])
def test_single_policy_lengths(p, name, C, N):
    call = _SINGLE[name]
    cont, nodes = _cont(C), _nodes(N)
    for i in range(1, 4):  # cpu sets C: every other field is measured against it
        _refused("every container array must hold C entries", call, p, _short(cont, i), nodes)
    _refused("every container array must hold C entries", call, p, _short(cont, 0), nodes)
    for i in range(1, 5):
        _refused("every node array must hold N entries", call, p, cont, _short(nodes, i))
    _refused("every node array must hold N entries", call, p, cont, _short(nodes, 0))
    _refused("level must hold C entries", call, p, cont, nodes, level=[0] * (C + 1))
    _refused("node_count must hold N entries", call, p, cont, nodes, node_count=[0] * (N - 1))
    _refused("domain must hold N entries", call, p, cont, nodes, domain=[0] * (N + 1), max_skew=1)
    _refused("max_skew must be a u32", call, p, cont, nodes, domain=[0] * N, max_skew=1 << 32)
    _refused("max_skew must be a u32", call, p, cont, nodes, max_skew=-1)
    if name == "place_policy":
        return
    _refused("relax_mask holds at most 4 hops", call, p, cont, nodes, relax_mask=[1, 2, 4, 8, 16])
    _refused("n_hops must be a u32", call, p, cont, nodes, n_hops=-1)
    _refused("n_hops must be a u32", call, p, cont, nodes, n_hops=1 << 32)
    if name == "place_policy_fallback":
        return
    for bad in ([[5, 6, 7], [5, 6, 7]], (5, -1, 3), (5, 1 << 32, 3)):
        _refused("quota must hold 1 rows of 3 u32 caps", call, p, cont, nodes, quota=bad)
    _refused(None, call, p, cont, nodes, quota=[5, 6])  # no whole row: numpy's own ValueError
    _refused("quota_used must hold 3 entries", call, p, cont, nodes, quota_used=[0, 0])
    _refused("quota_used must hold 3 entries", call, p, cont, nodes, quota_used=[0, 0, 0, 0])


@pytest.mark.parametrize("name", list(_BATCH))
@pytest.mark.parametrize("S,C,N", [(1, 2, 1), (2, 1, 2), (2, 2, 2)])
def test_batch_policy_lengths(p, name, S, C, N):
    call = _BATCH[name]
    cont, nodes = _cont(S * C), _nodes(S * N)
    for i in range(4):
        _refused("every container array must hold S * C entries", call, p, S, C, N, _short(cont, i), nodes)
    for i in range(5):
        _refused("every node array must hold S * N entries", call, p, S, C, N, cont, _short(nodes, i))
    _refused("level must hold S * C entries", call, p, S, C, N, cont, nodes, level=[0] * (S * C - 1))
    _refused("strategy and preferred must hold S entries", call, p, S, C, N, cont, nodes, preferred=[0] * (S + 1))
    _refused("node_count must hold S * N entries", call, p, S, C, N, cont, nodes, node_count=[0] * (S * N + 1))
    _refused("domain must hold S * N and max_skew S entries", call, p, S, C, N, cont, nodes,
             domain=[0] * (S * N - 1), max_skew=[1] * S)
    _refused("domain must hold S * N and max_skew S entries", call, p, S, C, N, cont, nodes,
             domain=[0] * (S * N), max_skew=[1] * (S + 1))
    if name == "place_batch_policy":
        return
    msg = "relax_mask must hold S * FP_FALLBACK_MAX_HOPS and n_hops S entries"
    _refused(msg, call, p, S, C, N, cont, nodes, relax_mask=[0] * (S * 4 - 1), n_hops=[1] * S)
    _refused(msg, call, p, S, C, N, cont, nodes, relax_mask=[0] * (S * 3), n_hops=[1] * S)
    _refused(msg, call, p, S, C, N, cont, nodes, relax_mask=[0] * (S * 4), n_hops=[1] * (S - 1))
    if name == "place_batch_policy_fallback":
        return
    for bad in ([5, 6, 7] * (S + 1), [5, 6, 7] * (S - 1), [5, -1, 7] * S, [5, 1 << 32, 7] * S):
        _refused(f"quota must hold {S} rows of 3 u32 caps", call, p, S, C, N, cont, nodes, quota=bad)
    _refused(None, call, p, S, C, N, cont, nodes, quota=[5, 6, 7] * (S - 1) + [5, 6])  # no whole row: numpy's ValueError
    _refused("quota_used must hold S * 3 entries", call, p, S, C, N, cont, nodes, quota_used=[0] * (S * 3 - 1))
    _refused("quota_used must hold S * 3 entries", call, p, S, C, N, cont, nodes, quota_used=[0] * (S * 3 + 1))


def _addr(x):
    """The address an argument carries, whatever ctypes form it was passed in (0 = NULL)."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "_obj"):  # ct.byref(struct)
        return ct.addressof(x._obj)
    return ct.cast(x, ct.c_void_p).value or 0


def _words(x, n, ctype=ct.c_uint32):
    a = _addr(x)
    return None if not a else list(ct.cast(ct.c_void_p(a), ct.POINTER(ctype))[:n])


class _Rec:
    """Stands in for the loaded library: every export records (name, args) and returns 0.  ``peek`` maps an
    argument index to a word count, read while the call's arrays are alive."""

    def __init__(self, **peek):
        self.calls, self.peek = [], {int(k[1:]): v for k, v in peek.items()}

    def __getattr__(self, name):
        def export(*args):
            self.calls.append((name, args, {i: _words(args[i], n) for i, n in self.peek.items()}))
            return 0
        return export


def _rec_planner(**peek):
    q = object.__new__(Planner)
    q._L = _Rec(**peek)
    q._ctx = ct.c_void_p(0x5EED)
    q._tstream = None
    q.device = 0
    q._dev = lambda fn, *a: fn(*a)  # no stream to order with: the call itself
    return q


def _one_call(q, export):
    (name, args, seen), = q._L.calls
    assert name == export and _addr(args[0]) == 0x5EED
    return args, seen


def _nulls(q, args):
    """The indices of the null pointer arguments of the one recorded call."""
    types = _lib.SIGNATURES[q._L.calls[0][0]][1]
    return [i for i, (a, t) in enumerate(zip(args, types)) if t is not ct.c_uint32 and _addr(a) == 0]


def test_place_policy_calls():
    cont, nodes = _cont(2), _nodes(2)
    q = _rec_planner()
    assign, reason, after, nc = q.place_policy(cont, nodes, "pack_into_dedicated", preferred=-1)
    args, _ = _one_call(q, "fp_place_policy")
    assert len(args) == 9 and args[4:6] == (_lib.STRATEGY_PACK, 0xFFFFFFFF) and nc is None
    assert _nulls(q, args) == [3, 6]  # no level, no node_count
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, ns.n) == (2, 2) and ns.cpu_free == after[0].ctypes.data and cs.cpu_m == cont[0].ctypes.data
    assert after[0] is not nodes[0] and ns.labels == after[2].ctypes.data
    assert (_addr(args[7]), _addr(args[8])) == (assign.ctypes.data, reason.ctypes.data)

    q = _rec_planner(a3=2, a6=2, a7=2)
    *_, nc = q.place_policy(cont, nodes, 3, 5, level=[0, 1], node_count=[4, 5], domain=[1, 0], max_skew=2)
    args, seen = _one_call(q, "fp_place_policy_spread")
    assert len(args) == 11 and args[4:6] == (3, 5) and args[8] == 2 and _nulls(q, args) == []
    assert seen == {3: [0, 1], 6: [4, 5], 7: [1, 0]} and _addr(args[6]) == nc.ctypes.data and nc.tolist() == [4, 5]


def test_place_policy_fallback_and_quota_calls():
    cont, nodes = _cont(2), _nodes(2)
    q = _rec_planner(a9=4)
    assign, reason, hops, after, nc = q.place_policy_fallback(cont, nodes, "spread_across_pool", [3, -1], preferred=1 << 32)
    args, seen = _one_call(q, "fp_place_policy_fallback")
    assert len(args) == 14 and args[4:6] == (_lib.STRATEGY_SPREAD, 0) and args[8] == 0 and args[10] == 2
    assert seen[9] == [3, 0xFFFFFFFF, 0, 0] and _nulls(q, args) == [3, 6, 7] and nc is None
    assert (_addr(args[11]), _addr(args[12]), _addr(args[13])) == (assign.ctypes.data, reason.ctypes.data, hops.ctypes.data)
    q = _rec_planner()
    hops = q.place_policy_fallback(cont, nodes, 1, [3, 1], n_hops=1, want_hops=False, domain=[0, 1], max_skew=1)[2]
    args, _ = _one_call(q, "fp_place_policy_fallback")
    assert hops is None and args[10] == 1 and args[8] == 1 and _nulls(q, args) == [3, 6, 13]

    q = _rec_planner(a9=4, a14=3, a15=3)
    out = q.place_policy_quota(cont, nodes, "fill_lowest", (500, None, 3), preferred=6)
    args, seen = _one_call(q, "fp_place_policy_quota")
    assert len(args) == 17 and args[4:6] == (_lib.STRATEGY_FILL_LOWEST, 6) and args[8] == 0 and args[10] == 0
    assert seen == {9: [0, 0, 0, 0], 14: [500, 0xFFFFFFFF, 3], 15: [0, 0, 0]}
    assert _nulls(q, args) == [3, 6, 7]
    assert [_addr(args[i]) for i in (11, 12, 13, 16, 15)] == [out[i].ctypes.data for i in (0, 1, 2, 5, 6)]
    assert out[4] is None and out[5].tolist() == [0, 0]
    q = _rec_planner(a15=3)
    out = q.place_policy_quota(cont, nodes, 1, (1, 2, 3), quota_used=[7, 8, 9], relax_mask=[1], want_hops=False,
                               want_why=False)
    args, seen = _one_call(q, "fp_place_policy_quota")
    assert seen[15] == [7, 8, 9] and args[10] == 1 and _nulls(q, args) == [3, 6, 7, 13, 16]
    assert out[2] is None and out[5] is None and out[6].tolist() == [7, 8, 9]
    q = _rec_planner()
    out = q.place_policy_quota(cont, nodes, 1, None, quota_used=[7, 8, 9], want_used=False)
    args, _ = _one_call(q, "fp_place_policy_quota")
    assert _nulls(q, args) == [3, 6, 7, 14, 15] and out[6] is None


def test_place_batch_policy_calls():
    S, C, N = 2, 2, 1
    cont, nodes = _cont(S * C), _nodes(S * N)
    q = _rec_planner(a2=2, a3=2)
    assign, reason, cost, after, nc = q.place_batch_policy(S, C, N, cont, nodes, ["fill_lowest", 2], preferred=[8, 9],
                                                           scen_base=5)
    args, seen = _one_call(q, "fp_place_batch_policy")
    assert len(args) == 5 and seen == {2: [3, 2], 3: [8, 9]} and _nulls(q, args) == [4] and nc is None
    b = args[1]._obj
    assert (b.n_scen, b.scen_base, b.n_containers, b.n_nodes) == (2, 5, 2, 1) and b.level is None
    assert (b.assign, b.reason, b.cost) == (assign.ctypes.data, reason.ctypes.data, cost.ctypes.data)
    assert (b.cpu_free, b.labels, b.cpu_m) == (after[0].ctypes.data, after[2].ctypes.data, cont[0].ctypes.data)
    # a domain without max_skew is no constraint: the plain export, not the spread one
    q = _rec_planner()
    q.place_batch_policy(S, C, N, cont, nodes, [1, 1], domain=[0, 0], level=[0] * 4)
    args, _ = _one_call(q, "fp_place_batch_policy")
    assert _nulls(q, args) == [3, 4] and args[1]._obj.level is not None
    q = _rec_planner(a5=2, a6=2)
    *_, nc = q.place_batch_policy(S, C, N, cont, nodes, [1, 1], node_count=[3, 4], domain=[1, 2], max_skew=[0, 7])
    args, seen = _one_call(q, "fp_place_batch_policy_spread")
    assert len(args) == 7 and seen == {5: [1, 2], 6: [0, 7]} and _nulls(q, args) == [3]
    assert _addr(args[4]) == nc.ctypes.data and nc.tolist() == [3, 4]


def test_place_batch_policy_fallback_and_quota_calls():
    S, C, N = 2, 1, 2
    cont, nodes = _cont(S * C), _nodes(S * N)
    q = _rec_planner(a7=8, a8=2)
    out = q.place_batch_policy_fallback(S, C, N, cont, nodes, [1, 2], relax_mask=[[1, 2, 0, 0], [4, 0, 0, 0]],
                                        n_hops=[2, 1], domain=[0] * 4)
    args, seen = _one_call(q, "fp_place_batch_policy_fallback")
    assert len(args) == 10 and seen == {7: [1, 2, 0, 0, 4, 0, 0, 0], 8: [2, 1]}
    assert _nulls(q, args) == [3, 4, 5, 6] and _addr(args[9]) == out[2].ctypes.data  # domain alone: both null
    q = _rec_planner()
    out = q.place_batch_policy_fallback(S, C, N, cont, nodes, [1, 2], relax_mask=[0] * 8, want_hops=False)
    args, _ = _one_call(q, "fp_place_batch_policy_fallback")
    assert _nulls(q, args) == [3, 4, 5, 6, 7, 8, 9] and out[2] is None  # masks without n_hops: both null

    q = _rec_planner(a10=6, a11=6)
    out = q.place_batch_policy_quota(S, C, N, cont, nodes, [1, 2], [[5, None, 7], [None, 1, 2]], scen_base=3)
    args, seen = _one_call(q, "fp_place_batch_policy_quota")
    assert len(args) == 13 and seen == {10: [5, 0xFFFFFFFF, 7, 0xFFFFFFFF, 1, 2], 11: [0] * 6}
    assert _nulls(q, args) == [3, 4, 5, 6, 7, 8] and args[1]._obj.scen_base == 3
    assert [_addr(args[i]) for i in (9, 12, 11)] == [out[i].ctypes.data for i in (2, 6, 7)]
    assert out[6].tolist() == [0, 0] and (args[1]._obj.assign, args[1]._obj.cost) == (out[0].ctypes.data, out[3].ctypes.data)
    q = _rec_planner(a11=6)
    out = q.place_batch_policy_quota(S, C, N, cont, nodes, [1, 2], [1] * 6, quota_used=[[1, 2, 3], [4, 5, 6]],
                                     want_hops=False, want_why=False)
    args, seen = _one_call(q, "fp_place_batch_policy_quota")
    assert seen[11] == [1, 2, 3, 4, 5, 6] and _nulls(q, args) == [3, 4, 5, 6, 7, 8, 9, 12]
    assert out[2] is None and out[6] is None and out[7].tolist() == [1, 2, 3, 4, 5, 6]
    q = _rec_planner()
    out = q.place_batch_policy_quota(S, C, N, cont, nodes, [1, 2], None, quota_used=[0] * 6, want_used=False)
    args, _ = _one_call(q, "fp_place_batch_policy_quota")
    assert _nulls(q, args) == [3, 4, 5, 6, 7, 8, 10, 11] and out[7] is None


def test_dev_policy_calls():
    torch = pytest.importorskip("torch")
    from fleetflow_amd.planner import DevBatch
    S, C, N = 2, 3, 2
    db = DevBatch.allocate(S, C, N, "cpu")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    st, pf, cnt, dom, sk, rm, nh = i32(S), i32(S), i32(S * N), i32(S * N), i32(S), i32(S * 4), i32(S)
    hops, why, qt, qu = u8(S * C), u8(S * C), i32(S * 3), i32(S * 3)
    ptrs = lambda *ts: tuple(0 if t is None else t.data_ptr() for t in ts)  # noqa: E731

    def sent(q, export, n):
        args, _ = _one_call(q, export)
        b = args[1]._obj
        assert len(args) == n and (b.n_scen, b.n_containers, b.n_nodes, b.assign) == (S, C, N, db.assign.data_ptr())
        return tuple(_addr(a) for a in args[2:])

    q = _rec_planner()
    assert q.dev_place_batch_policy(db, st, count_t=cnt) is None
    assert sent(q, "fp_dev_place_batch_policy", 5) == ptrs(st, None, cnt)
    q = _rec_planner()
    q.dev_place_batch_policy(db, st, pf, domain_t=dom)  # a domain without max_skew: the plain export
    assert sent(q, "fp_dev_place_batch_policy", 5) == ptrs(st, pf, None)
    q = _rec_planner()
    q.dev_place_batch_policy(db, st, pf, cnt, domain_t=dom, max_skew_t=sk)
    assert sent(q, "fp_dev_place_batch_policy_spread", 7) == ptrs(st, pf, cnt, dom, sk)
    q = _rec_planner()
    assert q.dev_place_batch_policy_fallback(db, st, domain_t=dom, relax_mask_t=rm, n_hops_t=nh, hops_t=hops) is hops
    assert sent(q, "fp_dev_place_batch_policy_fallback", 10) == ptrs(st, None, None, None, None, rm, nh, hops)
    q = _rec_planner()
    assert q.dev_place_batch_policy_fallback(db, st, domain_t=dom, max_skew_t=sk, n_hops_t=nh) is None
    assert sent(q, "fp_dev_place_batch_policy_fallback", 10) == ptrs(st, None, None, dom, sk, None, None, None)
    q = _rec_planner()
    assert q.dev_place_batch_policy_quota(db, st, qt, qu, pf, cnt, domain_t=dom, max_skew_t=sk, relax_mask_t=rm,
                                          n_hops_t=nh, hops_t=hops, quota_why_t=why) == (hops, why, qu)
    assert sent(q, "fp_dev_place_batch_policy_quota", 13) == ptrs(st, pf, cnt, dom, sk, rm, nh, hops, qt, qu, why)
    q = _rec_planner()
    assert q.dev_place_batch_policy_quota(db, st, None, relax_mask_t=rm, max_skew_t=sk) == (None, None, None)
    assert sent(q, "fp_dev_place_batch_policy_quota", 13) == ptrs(st) + (0,) * 10

    q = _rec_planner()
    q._L = _NoLib()
    for name, extra in (("dev_place_batch_policy", {}), ("dev_place_batch_policy_fallback", {}),
                        ("dev_place_batch_policy_quota", {"quota_t": qt})):
        fn = getattr(q, name)
        _refused("strategy_t must hold S entries", fn, db, i32(S + 1), **extra)
        _refused("preferred_t must hold S entries", fn, db, st, preferred_t=i32(S - 1), **extra)
        _refused("count_t must hold S * N entries", fn, db, st, count_t=i32(S * N + 1), **extra)
        _refused("domain_t must hold S * N and max_skew_t S entries", fn, db, st, domain_t=i32(S * N), max_skew_t=i32(1),
                 **extra)
        if name == "dev_place_batch_policy":
            continue
        _refused("relax_mask_t must hold S * FP_FALLBACK_MAX_HOPS and n_hops_t S entries", fn, db, st,
                 relax_mask_t=i32(S * 3), n_hops_t=nh, **extra)
        _refused("hops_t must hold S * C bytes", fn, db, st, hops_t=i32(S * C), **extra)
        _refused("hops_t must hold S * C bytes", fn, db, st, hops_t=u8(S * C - 1), **extra)
    fn = q.dev_place_batch_policy_quota
    _refused("quota_t and quota_used_t must hold S * 3 32-bit entries", fn, db, st, i32(S * 3 + 1))
    _refused("quota_t and quota_used_t must hold S * 3 32-bit entries", fn, db, st, qt, u8(S * 3))
    _refused("quota_why_t must hold S * C bytes", fn, db, st, qt, quota_why_t=i32(S * C))


# ---- the sweep wrappers: drain, scale-in and scale-out, plain and under the policy, host and dev_* ---------------
# Characterisation of the twelve sweep methods: the export each calls, the argument count, every scalar, which
# pointers are null, that the result arrays sent are the ones returned, the contents of the optional arrays, and
# that an array one entry short is refused with its message before any library call.
NONE = 0xFFFFFFFF
NOFIT = 1 << _lib.REASON_NOFIT
SW_C, SW_N, SW_K = 3, 2, 2  # containers, nodes, candidates / variants / templates
SW_ASSIGN, SW_GROUP, SW_TRY = [0, 1, NONE], [0, NONE], [[0, 1], [1, NONE]]
SW_TPL = ([4, 8], [4, 8], [0, 1])
SW_POLICY = dict(domain=[1, 0], max_skew=2, relax_mask=[3, -1])


def _ptrs(*xs):
    return [0 if x is None else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data for x in xs]


def _sent(args, *idx):
    return [_addr(args[i]) for i in idx]


def test_drain_sweep_calls():
    cont, nodes = _cont(SW_C), _nodes(SW_N)
    q = _rec_planner()
    out = q.drain_sweep(cont, nodes, SW_ASSIGN, SW_GROUP, 1)
    args, _ = _one_call(q, "fp_drain_sweep")
    assert len(args) == 12 and args[5:8] == (1, 0, 0) and _nulls(q, args) == [8]
    assert (args[1]._obj.n, args[2]._obj.n) == (SW_C, SW_N) and len(out) == 3
    assert _sent(args, 9, 10, 11) == _ptrs(*out) and [x.shape for x in out] == [(SW_C,), (SW_C,), (1, 8)]
    assert (out[0].dtype, out[1].dtype, out[2].dtype) == (np.uint32, np.uint8, np.uint32)
    q = _rec_planner(a3=3, a4=2, a8=2)
    out = q.drain_sweep(cont, nodes, SW_ASSIGN, SW_GROUP, SW_K, "fill_lowest", -1, [4, 5])
    args, seen = _one_call(q, "fp_drain_sweep")
    assert len(args) == 12 and args[5:8] == (SW_K, _lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF) and _nulls(q, args) == []
    assert seen == {3: SW_ASSIGN, 4: SW_GROUP, 8: [4, 5]} and out[2].shape == (SW_K, 8)

    q = _rec_planner()
    out = q.drain_sweep_policy(cont, nodes, SW_ASSIGN, SW_GROUP, 1)
    args, _ = _one_call(q, "fp_drain_sweep_policy")
    assert len(args) == 18 and args[5:8] == (1, 0, 0) and (args[10], args[12]) == (0, 0)
    assert _nulls(q, args) == [8, 9, 11] and len(out) == 5  # no node_count, no domain, an empty chain: null and 0
    assert _sent(args, 13, 14, 16, 15, 17) == _ptrs(*out)
    assert [x.shape for x in out] == [(SW_C,), (SW_C,), (1, 8), (SW_C,), (1, 4)] and out[3].dtype == np.uint8
    q = _rec_planner(a8=2, a9=2, a11=2)
    out = q.drain_sweep_policy(cont, nodes, SW_ASSIGN, SW_GROUP, SW_K, 2, 1 << 32 | 5, [4, 5], **SW_POLICY)
    args, seen = _one_call(q, "fp_drain_sweep_policy")
    assert len(args) == 18 and args[5:8] == (SW_K, 2, 5) and (args[10], args[12]) == (2, 2) and _nulls(q, args) == []
    assert seen == {8: [4, 5], 9: [1, 0], 11: [3, 0xFFFFFFFF]} and _sent(args, 13, 14, 16, 15, 17) == _ptrs(*out)
    q = _rec_planner()
    q.drain_sweep_policy(cont, nodes, SW_ASSIGN, SW_GROUP, 1, domain=[0, 1], max_skew=1, relax_mask=[])
    args, _ = _one_call(q, "fp_drain_sweep_policy")
    assert (args[10], args[12]) == (1, 0) and _nulls(q, args) == [8, 11]


def test_shrink_sweep_calls():
    cont, nodes = _cont(SW_C), _nodes(SW_N)
    q = _rec_planner(a4=4)
    out = q.shrink_sweep(cont, nodes, SW_ASSIGN, SW_TRY)
    args, seen = _one_call(q, "fp_shrink_sweep")
    assert len(args) == 14 and args[5:9] == (2, 2, 0, 0) and _nulls(q, args) == [9] and seen == {4: [0, 1, 1, NONE]}
    assert _sent(args, 10, 11, 12, 13) == _ptrs(*out) and len(out) == 4
    assert [x.shape for x in out] == [(2, SW_C), (2, SW_N), (2, SW_N), (2, 8)]
    assert [x.dtype for x in out] == [np.uint32, np.uint8, np.uint32, np.uint32]
    q = _rec_planner(a3=3, a9=2)
    q.shrink_sweep(cont, nodes, SW_ASSIGN, [[1]], "pack_into_dedicated", -2, [4, 5])
    args, seen = _one_call(q, "fp_shrink_sweep")
    assert args[5:9] == (1, 1, _lib.STRATEGY_PACK, 0xFFFFFFFE) and _nulls(q, args) == []
    assert seen == {3: SW_ASSIGN, 9: [4, 5]}

    q = _rec_planner()
    out = q.shrink_sweep_policy(cont, nodes, SW_ASSIGN, SW_TRY)
    args, _ = _one_call(q, "fp_shrink_sweep_policy")
    assert len(args) == 21 and args[5:9] == (2, 2, 0, 0) and (args[11], args[13]) == (0, 0)
    assert _nulls(q, args) == [9, 10, 12] and len(out) == 7
    assert _sent(args, 14, 15, 16, 17, 18, 19, 20) == _ptrs(*out)
    assert [x.shape for x in out] == [(2, SW_C), (2, SW_N), (2, SW_N), (2, 8), (2, SW_C), (2, SW_N), (2, 4)]
    assert [x.dtype for x in out[4:]] == [np.uint8, np.uint8, np.uint32]
    q = _rec_planner(a9=2, a10=2, a12=2)
    out = q.shrink_sweep_policy(cont, nodes, SW_ASSIGN, SW_TRY, 3, 9, [4, 5], **SW_POLICY)
    args, seen = _one_call(q, "fp_shrink_sweep_policy")
    assert args[5:9] == (2, 2, 3, 9) and (args[11], args[13]) == (2, 2) and _nulls(q, args) == []
    assert seen == {9: [4, 5], 10: [1, 0], 12: [3, 0xFFFFFFFF]} and _sent(args, 14, 15, 16, 17, 18, 19, 20) == _ptrs(*out)


def test_grow_sweep_calls():
    cont, nodes, reason = _cont(SW_C), _nodes(SW_N), [1, 0, 1]
    q = _rec_planner(a5=2, a6=2, a7=2)
    summary, assign = q.grow_sweep(cont, reason, SW_TPL, 3)
    args, seen = _one_call(q, "fp_grow_sweep")
    assert len(args) == 12 and args[3:5] == (NOFIT, SW_K) and args[9] == 3 and _nulls(q, args) == [8, 11]
    assert args[1]._obj.n == SW_C and args[1]._obj.cpu_m == cont[0].ctypes.data
    assert seen == {5: [4, 8], 6: [4, 8], 7: [0, 1]} and _addr(args[2]) != 0
    assert assign is None and _sent(args, 10) == _ptrs(summary) and summary.shape == (SW_K, 8)
    q = _rec_planner(a8=2)
    summary, assign = q.grow_sweep(cont, reason, SW_TPL, 5, 6, [1, 2], True)
    args, seen = _one_call(q, "fp_grow_sweep")
    assert args[3:5] == (6, SW_K) and args[9] == 5 and _nulls(q, args) == [] and seen == {8: [1, 2]}
    assert _sent(args, 10, 11) == _ptrs(summary, assign) and assign.shape == (SW_K, SW_C) and assign.dtype == np.uint32
    for rs in (reason, None):  # reason_mask 0: every container is pending and reason is not sent
        q = _rec_planner()
        q.grow_sweep(cont, rs, SW_TPL, 3, reason_mask=0)
        args, _ = _one_call(q, "fp_grow_sweep")
        assert args[3] == 0 and _nulls(q, args) == [2, 8, 11]

    q = _rec_planner()
    out = q.grow_sweep_policy(cont, reason, nodes, SW_TPL, 3)
    args, _ = _one_call(q, "fp_grow_sweep_policy")
    assert len(args) == 26 and (args[3], args[6], args[11]) == (NOFIT, SW_K, 3) and args[12:14] == (0, 0)
    assert (args[16], args[18]) == (0, 0) and (args[1]._obj.n, args[4]._obj.n) == (SW_C, SW_N)
    assert _nulls(q, args) == [5, 10, 14, 15, 17, 19, 20, 23, 24, 25]  # want_assign False: three nulls
    assert out[2:] == (None, None, None) and _sent(args, 21, 22) == _ptrs(*out[:2])
    assert [x.shape for x in out[:2]] == [(SW_K, 8), (SW_K, 8)]
    q = _rec_planner(a5=2, a10=2, a14=2, a15=2, a17=1, a19=3, a20=3)
    out = q.grow_sweep_policy(cont, reason, nodes, SW_TPL, 4, 6, [1, 2], "fill_lowest", -1, [4, 5], domain=[1, 0],
                              t_domain=[2, 3], max_skew=2, relax_mask=[7], quota=(5, None, 3), quota_used=[1, 2, 3],
                              want_assign=True)
    args, seen = _one_call(q, "fp_grow_sweep_policy")
    assert (args[3], args[6], args[11]) == (6, SW_K, 4) and args[12:14] == (_lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    assert (args[16], args[18]) == (2, 1) and _nulls(q, args) == []
    assert seen == {5: [4, 5], 10: [1, 2], 14: [1, 0], 15: [2, 3], 17: [7], 19: [5, 0xFFFFFFFF, 3], 20: [1, 2, 3]}
    assert _sent(args, 21, 22, 23, 24, 25) == _ptrs(*out)
    assert [x.shape for x in out[2:]] == [(SW_K, SW_C)] * 3 and [x.dtype for x in out[2:]] == [np.uint32, np.uint8, np.uint8]
    q = _rec_planner()
    q.grow_sweep_policy(cont, reason, nodes, SW_TPL, 3, reason_mask=0, relax_mask=(), want_assign=False)
    args, _ = _one_call(q, "fp_grow_sweep_policy")
    assert (args[3], args[18]) == (0, 0) and _nulls(q, args) == [2, 5, 10, 14, 15, 17, 19, 20, 23, 24, 25]


def test_host_sweep_lengths(p):
    cont, nodes, reason = _cont(SW_C), _nodes(SW_N), [1, 0, 1]
    tables = [("every container array must hold C entries", dict(cont=_short(cont, i))) for i in range(4)]
    tables += [("every node array must hold N entries", dict(nodes=_short(nodes, i))) for i in range(5)]
    policy = [("domain must hold N entries", dict(domain=[0])), ("max_skew must be a u32", dict(max_skew=-1)),
              ("max_skew must be a u32", dict(max_skew=1 << 32)),
              ("relax_mask holds at most 4 hops", dict(relax_mask=[1, 2, 4, 8, 16]))]
    count = [("node_count must hold N entries", dict(node_count=[0] * (SW_N - 1))),
             ("node_count must hold N entries", dict(node_count=[0] * (SW_N + 1)))]

    def run(fn, base, cases):
        for msg, kw in cases:
            _refused(msg, fn, **{**base, **kw})

    drain = dict(cont=cont, nodes=nodes, assign=SW_ASSIGN, group=SW_GROUP, n_cand=SW_K)
    cases = tables + count + [("assign must hold C entries", dict(assign=SW_ASSIGN[:-1])),
                              ("group must hold N entries", dict(group=SW_GROUP[:-1])),
                              ("n_cand must be a u32", dict(n_cand=-1)), ("n_cand must be a u32", dict(n_cand=1 << 32))]
    run(p.drain_sweep, drain, cases)
    run(p.drain_sweep_policy, drain, cases + policy)
    shrink = dict(cont=cont, nodes=nodes, assign=SW_ASSIGN, try_order=SW_TRY)
    cases = tables + count + [("assign must hold C entries", dict(assign=SW_ASSIGN[:-1])),
                              ("try_order must be [n_var, n_try]", dict(try_order=[0, 1])),
                              ("try_order must be [n_var, n_try]", dict(try_order=[[[0]]]))]
    run(p.shrink_sweep, shrink, cases)
    run(p.shrink_sweep_policy, shrink, cases + policy)
    grow = dict(cont=cont, reason=reason, templates=SW_TPL, max_new=3)
    cases = [("every container array must hold C entries", dict(cont=_short(cont, i))) for i in range(4)]
    cases += [("every container array must hold C entries", dict(cont=cont[:3])),
              ("reason must hold C entries", dict(reason=reason[:-1])),
              ("templates must be (t_cpu, t_mem, t_labels)", dict(templates=SW_TPL[:2])),
              ("reason_mask must be a u32", dict(reason_mask=-1)), ("max_new must be a u32", dict(max_new=-1)),
              ("max_new must be a u32", dict(max_new=1 << 32)), ("t_max must hold n_cand entries", dict(t_max=[1]))]
    cases += [("every template array must hold n_cand entries", dict(templates=_short(_u(*SW_TPL), i))) for i in range(3)]
    run(p.grow_sweep, grow, cases)
    cases += [("every node array must hold N entries", dict(nodes=_short(nodes, i))) for i in range(5)]
    cases += count + policy + [("t_domain must hold n_cand entries", dict(t_domain=[0] * (SW_K + 1))),
                               ("quota must hold 1 rows of 3 u32 caps", dict(quota=(5, -1, 3))),
                               ("quota must hold 1 rows of 3 u32 caps", dict(quota=[[5, 6, 7], [5, 6, 7]])),
                               ("quota_used must hold 3 entries", dict(quota_used=[0, 0]))]
    run(p.grow_sweep_policy, {**grow, "nodes": nodes}, cases)


def _sweep_tensors(torch):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    cont_t = tuple(i32(SW_C) for _ in range(4))
    nodes_t = tuple(i32(SW_N) for _ in range(4)) + (u8(SW_N),)
    return i32, u8, cont_t, nodes_t


def _tables_sent(args, cont_t, nodes_t, ns_at=2):
    cs = args[1]._obj
    assert (cs.n, cs.cpu_m, cs.mem_mib, cs.req_labels, cs.conflict) == (SW_C, *_ptrs(*cont_t))
    if nodes_t is not None:
        ns = args[ns_at]._obj
        assert (ns.n, ns.cpu_free, ns.mem_free, ns.labels, ns.conflict_used, ns.schedulable) == (SW_N, *_ptrs(*nodes_t))


def test_dev_drain_and_shrink_sweep_calls():
    torch = pytest.importorskip("torch")
    i32, u8, cont_t, nodes_t = _sweep_tensors(torch)
    asg, grp, cnt, dom = i32(SW_C), i32(SW_N), i32(SW_N), i32(SW_N)
    out, reason, summary, hops, prow = i32(SW_C), u8(SW_C), i32(SW_K * 8), u8(SW_C), i32(SW_K * 4)
    q = _rec_planner()
    assert q.dev_drain_sweep(cont_t, nodes_t, asg, grp, SW_K, out, reason, summary) is None
    args, _ = _one_call(q, "fp_dev_drain_sweep")
    _tables_sent(args, cont_t, nodes_t)
    assert len(args) == 12 and args[5:8] == (SW_K, 0, 0) and _nulls(q, args) == [8]
    assert _sent(args, 3, 4, 9, 10, 11) == _ptrs(asg, grp, out, reason, summary)
    q = _rec_planner()
    q.dev_drain_sweep(cont_t, nodes_t, asg, grp, SW_K, out, reason, summary, "fill_lowest", -1, cnt)
    args, _ = _one_call(q, "fp_dev_drain_sweep")
    assert args[5:8] == (SW_K, 3, 0xFFFFFFFF) and _nulls(q, args) == [] and _sent(args, 8) == _ptrs(cnt)

    q = _rec_planner()
    assert q.dev_drain_sweep_policy(cont_t, nodes_t, asg, grp, SW_K, out, reason, summary) is None
    args, _ = _one_call(q, "fp_dev_drain_sweep_policy")
    _tables_sent(args, cont_t, nodes_t)
    assert len(args) == 18 and args[5:8] == (SW_K, 0, 0) and (args[10], args[12]) == (0, 0)
    assert _nulls(q, args) == [8, 9, 11, 15, 17]
    assert _sent(args, 3, 4, 13, 14, 16) == _ptrs(asg, grp, out, reason, summary)
    q = _rec_planner(a11=2)
    q.dev_drain_sweep_policy(cont_t, nodes_t, asg, grp, SW_K, out, reason, summary, 2, 5, cnt, domain_t=dom, max_skew=2,
                             relax_mask=[3, -1], hops_t=hops, policy_t=prow)
    args, seen = _one_call(q, "fp_dev_drain_sweep_policy")
    assert args[5:8] == (SW_K, 2, 5) and (args[10], args[12]) == (2, 2) and _nulls(q, args) == []
    assert seen == {11: [3, 0xFFFFFFFF]}
    assert _sent(args, 8, 9, 13, 14, 15, 16, 17) == _ptrs(cnt, dom, out, reason, hops, summary, prow)

    tro, vout, state, blocker = i32(SW_K * 2), i32(SW_K * SW_C), u8(SW_K * SW_N), i32(SW_K * SW_N)
    vhops, why = u8(SW_K * SW_C), u8(SW_K * SW_N)
    q = _rec_planner()
    assert q.dev_shrink_sweep(cont_t, nodes_t, asg, tro, SW_K, vout, state, summary) is None
    args, _ = _one_call(q, "fp_dev_shrink_sweep")
    _tables_sent(args, cont_t, nodes_t)
    assert len(args) == 14 and args[5:9] == (SW_K, 2, 0, 0) and _nulls(q, args) == [9, 12]
    assert _sent(args, 3, 4, 10, 11, 13) == _ptrs(asg, tro, vout, state, summary)
    q = _rec_planner()
    q.dev_shrink_sweep(cont_t, nodes_t, asg, tro, SW_K, vout, state, summary, 1, 7, cnt, blocker)
    args, _ = _one_call(q, "fp_dev_shrink_sweep")
    assert args[5:9] == (SW_K, 2, 1, 7) and _nulls(q, args) == [] and _sent(args, 9, 12) == _ptrs(cnt, blocker)
    q = _rec_planner()
    q.dev_shrink_sweep(cont_t, nodes_t, asg, i32(0), 0, i32(0), u8(0), i32(0))  # no variant: n_try 0
    args, _ = _one_call(q, "fp_dev_shrink_sweep")
    assert args[5:7] == (0, 0)

    q = _rec_planner()
    assert q.dev_shrink_sweep_policy(cont_t, nodes_t, asg, tro, SW_K, vout, state, summary) is None
    args, _ = _one_call(q, "fp_dev_shrink_sweep_policy")
    _tables_sent(args, cont_t, nodes_t)
    assert len(args) == 21 and args[5:9] == (SW_K, 2, 0, 0) and (args[11], args[13]) == (0, 0)
    assert _nulls(q, args) == [9, 10, 12, 16, 18, 19, 20]
    assert _sent(args, 3, 4, 14, 15, 17) == _ptrs(asg, tro, vout, state, summary)
    q = _rec_planner(a12=1)
    q.dev_shrink_sweep_policy(cont_t, nodes_t, asg, tro, SW_K, vout, state, summary, 3, -1, cnt, blocker, domain_t=dom,
                              max_skew=4, relax_mask=[9], hops_t=vhops, blocker_reason_t=why, policy_t=prow)
    args, seen = _one_call(q, "fp_dev_shrink_sweep_policy")
    assert args[5:9] == (SW_K, 2, 3, 0xFFFFFFFF) and (args[11], args[13]) == (4, 1) and _nulls(q, args) == []
    assert seen == {12: [9]}
    assert _sent(args, 9, 10, 14, 15, 16, 17, 18, 19, 20) == _ptrs(cnt, dom, vout, state, blocker, summary, vhops, why, prow)


def test_dev_grow_sweep_calls():
    torch = pytest.importorskip("torch")
    i32, u8, cont_t, nodes_t = _sweep_tensors(torch)
    rs, tpl, tm, summary = u8(SW_C), tuple(i32(SW_K) for _ in range(3)), i32(SW_K), i32(SW_K * 8)
    aout, cnt, dom, td, prow = i32(SW_K * SW_C), i32(SW_N), i32(SW_N), i32(SW_K), i32(SW_K * 8)
    hops, rout = u8(SW_K * SW_C), u8(SW_K * SW_C)
    q = _rec_planner()
    assert q.dev_grow_sweep(cont_t, rs, tpl, 3, summary) is None
    args, _ = _one_call(q, "fp_dev_grow_sweep")
    _tables_sent(args, cont_t, None)
    assert len(args) == 12 and args[3:5] == (NOFIT, SW_K) and args[9] == 3 and _nulls(q, args) == [8, 11]
    assert _sent(args, 2, 5, 6, 7, 10) == _ptrs(rs, *tpl, summary)
    q = _rec_planner()
    q.dev_grow_sweep(cont_t, rs, tpl, 5, summary, 6, tm, aout)
    args, _ = _one_call(q, "fp_dev_grow_sweep")
    assert args[3:5] == (6, SW_K) and args[9] == 5 and _nulls(q, args) == [] and _sent(args, 8, 11) == _ptrs(tm, aout)
    q = _rec_planner()
    q.dev_grow_sweep(cont_t, rs, tpl, 3, summary, reason_mask=0)
    args, _ = _one_call(q, "fp_dev_grow_sweep")
    assert args[3] == 0 and _nulls(q, args) == [2, 8, 11]

    q = _rec_planner()
    assert q.dev_grow_sweep_policy(cont_t, rs, nodes_t, tpl, 3, summary) is None
    args, _ = _one_call(q, "fp_dev_grow_sweep_policy")
    _tables_sent(args, cont_t, nodes_t, 4)
    assert len(args) == 26 and (args[3], args[6], args[11]) == (NOFIT, SW_K, 3) and args[12:14] == (0, 0)
    assert (args[16], args[18]) == (0, 0) and _nulls(q, args) == [5, 10, 14, 15, 17, 19, 20, 22, 23, 24, 25]
    assert _sent(args, 2, 7, 8, 9, 21) == _ptrs(rs, *tpl, summary)
    q = _rec_planner(a17=2, a19=3, a20=3)
    q.dev_grow_sweep_policy(cont_t, rs, nodes_t, tpl, 4, summary, 6, tm, "pack_into_dedicated", -1, cnt, domain_t=dom,
                            t_domain_t=td, max_skew=2, relax_mask=[3, -1], quota=(5, None, 3), quota_used=[1, 2, 3],
                            policy_t=prow, assign_out_t=aout, hops_t=hops, reason_out_t=rout)
    args, seen = _one_call(q, "fp_dev_grow_sweep_policy")
    assert (args[3], args[6], args[11]) == (6, SW_K, 4) and args[12:14] == (_lib.STRATEGY_PACK, 0xFFFFFFFF)
    assert (args[16], args[18]) == (2, 2) and _nulls(q, args) == []
    assert seen == {17: [3, 0xFFFFFFFF], 19: [5, 0xFFFFFFFF, 3], 20: [1, 2, 3]}
    assert _sent(args, 5, 10, 14, 15, 21, 22, 23, 24, 25) == _ptrs(cnt, tm, dom, td, summary, prow, aout, hops, rout)
    q = _rec_planner()
    q.dev_grow_sweep_policy(cont_t, rs, nodes_t, tpl, 3, summary, reason_mask=0)
    args, _ = _one_call(q, "fp_dev_grow_sweep_policy")
    assert args[3] == 0 and 2 in _nulls(q, args)


def test_dev_sweep_lengths(p):
    torch = pytest.importorskip("torch")
    i32, u8, cont_t, nodes_t = _sweep_tensors(torch)
    p._dev = lambda fn, *a: fn(*a)
    C, N, K = SW_C, SW_N, SW_K

    def run(fn, base, cases):
        for msg, kw in cases:
            _refused(msg, fn, **{**base, **kw})

    def both(name, n, size, msg):  # one entry short, and the other element size
        return [(msg, {name: (i32 if size == 4 else u8)(n - 1)}), (msg, {name: (u8 if size == 4 else i32)(n)})]

    ctab = [("every container tensor must hold C 32-bit entries", dict(cont_t=_short(cont_t, i))) for i in range(1, 4)]
    ctab += [("every container tensor must hold C 32-bit entries", dict(cont_t=cont_t[:3])),
             ("every container tensor must hold C 32-bit entries", dict(cont_t=cont_t[:3] + (u8(C),)))]
    msg = "every node tensor must hold N entries (schedulable N bytes)"
    ntab = [(msg, dict(nodes_t=_short(nodes_t, i))) for i in range(1, 5)]
    ntab += [(msg, dict(nodes_t=nodes_t[:4])), (msg, dict(nodes_t=nodes_t[:4] + (i32(N),))),
             (msg, dict(nodes_t=(u8(N),) + nodes_t[1:]))]
    policy = both("domain_t", N, 4, "domain_t must hold N 32-bit entries") + [
        ("max_skew must be a u32", dict(max_skew=-1)), ("relax_mask holds at most 4 hops", dict(relax_mask=[1] * 5))]
    count = both("count_t", N, 4, "count_t must hold N 32-bit entries")

    drain = dict(cont_t=cont_t, nodes_t=nodes_t, assign_t=i32(C), group_t=i32(N), n_cand=K, assign_out_t=i32(C),
                 reason_t=u8(C), summary_t=i32(K * 8))
    cases = (ctab + ntab + count + both("assign_t", C, 4, "assign_t must hold C 32-bit entries")
             + both("group_t", N, 4, "group_t must hold N 32-bit entries")
             + both("assign_out_t", C, 4, "assign_out_t must hold C 32-bit entries")
             + both("reason_t", C, 1, "reason_t must hold C bytes")
             + both("summary_t", K * 8, 4, "summary_t must hold n_cand * 8 32-bit entries")
             + [("n_cand must be a u32", dict(n_cand=-1))])
    run(p.dev_drain_sweep, drain, cases)
    run(p.dev_drain_sweep_policy, drain, cases + policy + both("hops_t", C, 1, "hops_t must hold C bytes")
        + both("policy_t", K * 4, 4, "policy_t must hold n_cand * 4 32-bit entries"))

    shrink = dict(cont_t=cont_t, nodes_t=nodes_t, assign_t=i32(C), try_order_t=i32(K * 2), n_var=K,
                  assign_out_t=i32(K * C), state_t=u8(K * N), summary_t=i32(K * 8))
    cases = (ctab + ntab + count + both("assign_t", C, 4, "assign_t must hold C 32-bit entries")
             + both("assign_out_t", K * C, 4, "assign_out_t must hold n_var * C 32-bit entries")
             + both("state_t", K * N, 1, "state_t must hold n_var * N bytes")
             + both("blocker_t", K * N, 4, "blocker_t must hold n_var * N 32-bit entries")
             + both("summary_t", K * 8, 4, "summary_t must hold n_var * 8 32-bit entries")
             + both("try_order_t", K * 2, 4, "try_order_t must hold n_var rows of 32-bit entries")
             + [("n_var must be a u32", dict(n_var=-1)),
                ("try_order_t must hold n_var rows of 32-bit entries", dict(n_var=0, assign_out_t=i32(0), state_t=u8(0),
                                                                            summary_t=i32(0)))])
    run(p.dev_shrink_sweep, shrink, cases)
    run(p.dev_shrink_sweep_policy, shrink, cases + policy
        + both("hops_t", K * C, 1, "hops_t must hold n_var * C bytes")
        + both("blocker_reason_t", K * N, 1, "blocker_reason_t must hold n_var * N bytes")
        + both("policy_t", K * 4, 4, "policy_t must hold n_var * 4 32-bit entries"))

    tpl = tuple(i32(K) for _ in range(3))
    grow = dict(cont_t=cont_t, reason_t=u8(C), templates_t=tpl, max_new=3, summary_t=i32(K * 8))
    cases = (ctab + both("reason_t", C, 1, "reason_t must hold C bytes")
             + both("t_max_t", K, 4, "t_max_t must hold n_cand 32-bit entries")
             + both("summary_t", K * 8, 4, "summary_t must hold n_cand * 8 32-bit entries")
             + both("assign_out_t", K * C, 4, "assign_out_t must hold n_cand * C 32-bit entries")
             + [("templates_t must be (t_cpu, t_mem, t_labels)", dict(templates_t=tpl[:2])),
                ("every template tensor must hold n_cand 32-bit entries", dict(templates_t=_short(tpl, 1))),
                ("every template tensor must hold n_cand 32-bit entries", dict(templates_t=tpl[:2] + (u8(K),))),
                ("reason_mask must be a u32", dict(reason_mask=1 << 32)), ("max_new must be a u32", dict(max_new=-1))])
    run(p.dev_grow_sweep, grow, cases)
    run(p.dev_grow_sweep_policy, {**grow, "nodes_t": nodes_t}, cases + ntab + count + policy
        + both("t_domain_t", K, 4, "t_domain_t must hold n_cand 32-bit entries")
        + both("policy_t", K * 8, 4, "policy_t must hold n_cand * 8 32-bit entries")
        + both("hops_t", K * C, 1, "hops_t must hold n_cand * C bytes")
        + both("reason_out_t", K * C, 1, "reason_out_t must hold n_cand * C bytes")
        + [("quota must hold 1 rows of 3 u32 caps", dict(quota=(5, -1, 3))),
           ("quota_used must hold 3 entries", dict(quota_used=[0, 0]))])


def test_plan_stage_lists_drops_the_handle_on_close(monkeypatch):
    """plan_stage_lists keeps a prebuilt argument tuple between calls; close() destroys the context, so the
    next call must reach the library with a null context (FP_EINVAL, as every other method) and never with
    the destroyed handle."""
    seen = []

    def fp_plan_stage(*args):
        seen.append(_addr(args[0]))
        return _lib.FP_OK if seen[-1] else _lib.FP_EINVAL

    monkeypatch.setattr(_lib, "raw_function", lambda name: fp_plan_stage)
    q = _rec_planner()
    assert q.plan_stage_lists([0, 0, 0], [], [0, 0])[3] == 0
    q.close()
    assert [c[0] for c in q._L.calls] == ["fp_ctx_destroy"]
    with pytest.raises(_lib.FleetplaceError) as e:
        q.plan_stage_lists([0, 0, 0], [], [0, 0])
    assert e.value.code == _lib.FP_EINVAL and seen == [0x5EED, 0]
