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
