"""GPU parity of the packed one-wave FFD kernels' register double buffer (fp_pipe.hip FPP_LOOKAHEAD 3 / 4)
and of the directly mapped workgroup tickets.

The packed one-wave kernels (w12p, bigp) request the next batch's fields one batch early, and a segment
fed by a link looks two slots ahead: the gathers of slot itail + 1 and the words of slot itail + 2.  The
second look-ahead can see a partial slot, END or a slot that no head seen covers yet, so the link cases
run every container count around one, two and three slots, with every publish period, and with the
consumer started beside its producer (lag 1: the gated path and the early path alternate) as well as
after it (lag S).  A bounded ring that wraps consumes positions of slot itail + 1 a batch early while
only slots below itail are released.  Segment 0 requests rows k0 + lane clamped at C.  The u32 kernels
(packed = 0) must behave as before.  With lag == S the v-th workgroup takes segment v / S of scenario
v % S directly; other lags keep the ticket loop.  Every result is the C oracle's, bit for bit:
assignment, reason, packed cost and the node tables after.

Geometry of every case (as tests/test_gpu_pipe_lookahead.py): N = 2200 nodes with pipe_w = 1 and
pipe_seg = 12, three one-wave segments of 12 groups; segment 0 owns the first 768 nodes.  S <= 7 runs
the five-wave kernels (w12p / w12), S = 4096 the six-wave ones (bigp / big).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0A13
N = 2200
HEAD = 768  # the nodes of segment 0 (12 groups)
GEO = (12, 1, 3)  # groups, stages, segments


def _scenarios(O, S, C, base, head):
    """S generator scenarios; head = "cordon": segment 0's nodes unschedulable (it forwards every
    container), "roomy": they take everything (segment 1 sees END only), None: as generated."""
    conts, nodes = [], []
    for s in range(S):
        c, n = O.gen_scenario(SEED + C, base + s, C, N, 7)
        n = [np.array(a) for a in n]
        n[4] = n[4].astype(np.uint8)
        if head == "cordon":
            n[4][:HEAD] = 0
        elif head == "roomy":
            n[0][:HEAD] = 1 << 30
            n[1][:HEAD] = 1 << 30
            n[2][:HEAD] = 0xFFFFFFFF
            n[3][:HEAD] = 0
            n[4][:HEAD] = 1
        conts.append(c)
        nodes.append(n)
    return conts, nodes


def _place(planner, conts, nodes, base):
    S, C = len(conts), conts[0][0].size
    cat = lambda parts, i: np.concatenate([p[i] for p in parts])  # noqa: E731
    return planner.place_batch(S, C, N, [cat(conts, i) for i in range(4)], [cat(nodes, i) for i in range(5)],
                               scen_base=base)


def _check(planner, O, conts, nodes, base):
    S, C = len(conts), conts[0][0].size
    assign, reason, cost, after = _place(planner, conts, nodes, base)
    for s in range(S):
        ea, er, eafter, _ = O.place(conts[s], nodes[s])
        assert np.array_equal(assign[s * C:(s + 1) * C], ea), s
        assert np.array_equal(reason[s * C:(s + 1) * C], er), s
        assert int(cost[s]) == O.cost(ea, N, base + s), s
        for i in (0, 1, 3):
            assert np.array_equal(after[i][s * N:(s + 1) * N], eafter[i]), (s, i)
    return assign


def _geometry(planner, S, C):
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["segments"]) == GEO, geo
    return geo


# slots on the link out of a cordoned segment 0 -- 1 / 63: partial, END; 64: full, END; 65 / 127: full,
# partial, END; 128: two full, END; 129: two full, partial, END; 192: three full, END; 193: three full,
# partial, END.  Roomy: END alone, whatever C
EDGES = [(C, "cordon") for C in (1, 63, 64, 65, 127, 128, 129, 192, 193)] + [(1, "roomy"), (129, "roomy")]


@pytest.mark.parametrize("lag", ["S", 1])
@pytest.mark.parametrize("publish", [1, 8, 1024])
@pytest.mark.parametrize("C,head", EDGES)
def test_link_stream_two_deep(C, head, publish, lag, planner, O, opts):
    S, base = 3, 33
    lagv = S if lag == "S" else lag
    opts(pipe_w=1, pipe_seg=12, pipe_lag=lagv, link_publish=publish)
    geo = _geometry(planner, S, C)
    assert geo["lag"] == lagv and geo["bounded"] == 0, geo
    conts, nodes = _scenarios(O, S, C, base, head)
    assign = _check(planner, O, conts, nodes, base)
    placed = assign[assign != 0xFFFFFFFF]
    if head == "cordon":
        path = planner.place_path()
        assert path["ran"] and path["packed"], path  # w12p, the double-buffered kernel
        assert placed.size and (placed >= HEAD).all()  # everything went over the link
    else:
        assert placed.size == S * C and (placed < HEAD).all()  # nothing did


def test_link_bounded_ring_wraps(planner, O, opts):
    """A forced 8-slot ring (every segment resident, lag 0) that wraps: 577 containers are nine full
    slots, a partial one and END.  The gathers of slot itail + 1 and the words of slot itail + 2 are
    read only below the head seen, which the producer cannot overwrite before the tail passes them."""
    S, C, base = 3, 577, 6
    opts(pipe_w=1, pipe_seg=12, link_slots=8)
    geo = _geometry(planner, S, C)
    assert geo["bounded"] == 1 and geo["link_slots"] == 8 and geo["lag"] == 0, geo
    conts, nodes = _scenarios(O, S, C, base, "cordon")
    _check(planner, O, conts, nodes, base)
    path = planner.place_path()
    assert path["ran"] and path["packed"], path


@pytest.mark.parametrize("C", [1, 64, 65, 200])
def test_segment0_next_rows(C, planner, O, opts):
    """Segment 0 reads the sorted rows one batch early: one container, exactly one batch, one more, and
    a last batch of 8 (the request of the next batch's rows is clamped at C)."""
    S, base = 3, 11
    opts(pipe_w=1, pipe_seg=12)
    _geometry(planner, S, C)
    conts, nodes = _scenarios(O, S, C, base, None)
    _check(planner, O, conts, nodes, base)
    path = planner.place_path()
    assert path["ran"] and path["packed"], path


@pytest.mark.parametrize("packed", [None, 0])
def test_five_wave_kernels(packed, planner, O, opts):
    """S = 3 on w12p (packed auto) and on the u32 kernel w12 (packed = 0), which keeps look-ahead 1."""
    S, C, base = 3, 193, 2
    kw = dict(pipe_w=1, pipe_seg=12)
    if packed is not None:
        kw["packed"] = packed
    opts(**kw)
    _geometry(planner, S, C)
    conts, nodes = _scenarios(O, S, C, base, "cordon")
    _check(planner, O, conts, nodes, base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == (packed is None), path


def _big(O, C):
    """4096 cordoned scenarios of C containers and their oracle plans."""
    S, base = 4096, 0
    conts, nodes = _scenarios(O, S, C, base, "cordon")

    def one(s):
        ea, er, eafter, _ = O.place(conts[s], nodes[s])
        return ea, er, eafter, O.cost(ea, N, base + s)

    with ThreadPoolExecutor(16) as ex:
        plans = list(ex.map(one, range(S)))
    return conts, nodes, plans


@pytest.fixture(scope="module")
def big130(O):
    """C = 130: two full slots, a partial one, END on the first link.  Computed once per module."""
    return _big(O, 130)


@pytest.fixture(scope="module")
def big200(O):
    """C = 200: three full slots, a partial one, END."""
    return _big(O, 200)


def _check_big(planner, big, want_lag, packed):
    """All 4096 costs, and scenarios 0, 2047 and 4095 plan for plan."""
    conts, nodes, plans = big
    S, C, base = len(conts), conts[0][0].size, 0
    geo = _geometry(planner, S, C)
    assert geo["lag"] == want_lag and geo["bounded"] == 0, geo
    assert geo["segments"] * S > geo["resident"], geo
    assign, reason, cost, after = _place(planner, conts, nodes, base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == packed, path
    ecost = np.array([p[3] for p in plans], np.uint64)
    bad = np.nonzero(cost != ecost)[0]
    assert bad.size == 0, f"{bad.size} scenario costs differ, first {bad[:8].tolist()}"
    for s in (0, 2047, 4095):
        ea, er, eafter, _ = plans[s]
        assert np.array_equal(assign[s * C:(s + 1) * C], ea), s
        assert np.array_equal(reason[s * C:(s + 1) * C], er), s
        for i in (0, 1, 3):
            assert np.array_equal(after[i][s * N:(s + 1) * N], eafter[i]), (s, i)


@pytest.mark.parametrize("packed", [None, 0])
@pytest.mark.parametrize("C", [130, 200])
def test_six_wave_kernels(C, packed, request, planner, opts):
    """bigp (packed auto) and big (packed = 0): phased segments (lag = S), unbounded links, more
    segments than resident slots."""
    big = request.getfixturevalue(f"big{C}")
    kw = dict(pipe_w=1, pipe_seg=12)
    if packed is not None:
        kw["packed"] = packed
    opts(**kw)
    _check_big(planner, big, 4096, packed is None)


@pytest.mark.parametrize("lag", ["S", 0])
@pytest.mark.parametrize("S", [1, 2, 7])
def test_direct_tickets_small(S, lag, planner, O, opts):
    """lag == S maps the v-th workgroup to segment v / S of scenario v % S; lag 0 keeps the loop, in
    which every ticket names a scenario."""
    C, base = 200, 17
    lagv = S if lag == "S" else 0
    opts(pipe_w=1, pipe_seg=12, pipe_lag=lagv)
    geo = _geometry(planner, S, C)
    assert geo["lag"] == lagv, geo
    conts, nodes = _scenarios(O, S, C, base, "cordon")
    _check(planner, O, conts, nodes, base)


@pytest.mark.parametrize("lag", ["S", 0])
def test_direct_tickets_4096(lag, big130, planner, opts):
    S = 4096
    lagv = S if lag == "S" else 0
    opts(pipe_w=1, pipe_seg=12, pipe_lag=lagv)
    _check_big(planner, big130, lagv, True)
