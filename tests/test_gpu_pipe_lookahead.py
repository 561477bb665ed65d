"""GPU parity of the one-wave FFD kernels' input look-ahead (fp_pipe.hip FPP_LOOKAHEAD).

A segment fed by a global link requests the next slot's count and position words one batch early,
but only when a head it has already seen covers that slot; segment 0 touches the rows of its next
batch.  The cases sit on the stream's edges: a partial slot then END, exactly full slots, END alone,
a consumer running beside its producer (lag 1: the head seen rarely covers the next slot, so the
gated path runs), every publish period, a bounded ring that wraps, and container counts at and
around one batch in segment 0.  Every result is the C oracle's, bit for bit: assignment, reason,
packed cost and the node tables after.

Geometry of every case: N = 2200 nodes (35 groups, the last one partial) with pipe_w = 1 and
pipe_seg = 12, i.e. three one-wave segments of 12 groups (the planner balances the groups over
ceil(35 / 12) = 3 segments; 25 groups, N = 1600, would balance to 9 per segment and run the
1024-thread kernel, which has no look-ahead).  Segment 0 owns the first 768 nodes.  S = 3 runs the
five-wave kernels (w12 / w12p), S = 4096 the six-wave ones (big / bigp).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0A11
N = 2200
HEAD = 768  # the nodes of segment 0 (12 groups)


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


# (C, head): slots on the link out of segment 0 -- 63: partial, END; 64: full, END; 65: full,
# partial, END; 128: two full, END; 129: two full, partial, END; roomy: END alone
EDGES = [(63, "cordon"), (64, "cordon"), (65, "cordon"), (128, "cordon"), (129, "cordon"), (129, "roomy")]


@pytest.mark.parametrize("lag", ["S", 1])
@pytest.mark.parametrize("publish", [1, 8, 1024])
@pytest.mark.parametrize("C,head", EDGES)
def test_link_stream_edges(C, head, publish, lag, planner, O, opts):
    S, base = 3, 21
    lagv = S if lag == "S" else lag
    opts(pipe_w=1, pipe_seg=12, pipe_lag=lagv, link_publish=publish)
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["segments"]) == (12, 1, 3), geo
    assert geo["lag"] == lagv and geo["bounded"] == 0, geo
    conts, nodes = _scenarios(O, S, C, base, head)
    assign = _check(planner, O, conts, nodes, base)
    placed = assign[assign != 0xFFFFFFFF]
    if head == "cordon":
        assert placed.size and (placed >= HEAD).all()  # everything went over the link
    else:
        assert placed.size == S * C and (placed < HEAD).all()  # nothing did


def test_link_bounded_ring(planner, O, opts):
    """A forced 8-slot ring (every segment resident, lag 0) that wraps: 577 containers are nine full
    slots, a partial one and END.  The look-ahead reads slot itail + 1 only below the head seen, which
    the producer cannot overwrite before the tail passes it."""
    S, C, base = 3, 577, 5
    opts(pipe_w=1, pipe_seg=12, link_slots=8)
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["segments"]) == (12, 1, 3), geo
    assert geo["bounded"] == 1 and geo["link_slots"] == 8 and geo["lag"] == 0, geo
    conts, nodes = _scenarios(O, S, C, base, "cordon")
    _check(planner, O, conts, nodes, base)


@pytest.mark.parametrize("C", [1, 64, 200])
def test_segment0_edges(C, planner, O, opts):
    """Segment 0 reads the sorted rows: one container, exactly one batch, and a last batch of 8 (the
    touch of the next batch's rows is clamped at C)."""
    S, base = 3, 9
    opts(pipe_w=1, pipe_seg=12)
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["segments"]) == (12, 1, 3), geo
    conts, nodes = _scenarios(O, S, C, base, None)
    _check(planner, O, conts, nodes, base)


@pytest.fixture(scope="module")
def big_batch(O):
    """4096 scenarios of 130 containers (two full slots, a partial one, END on the first link) and
    their oracle plans, computed once for both kernels."""
    S, C, base = 4096, 130, 0
    conts, nodes = _scenarios(O, S, C, base, "cordon")

    def one(s):
        ea, er, eafter, _ = O.place(conts[s], nodes[s])
        return ea, er, eafter, O.cost(ea, N, base + s)

    with ThreadPoolExecutor(16) as ex:
        plans = list(ex.map(one, range(S)))
    return conts, nodes, plans


@pytest.mark.parametrize("packed", [None, 0])
def test_six_wave_kernels(packed, big_batch, planner, opts):
    """The six-wave instantiation (bigp, and big with FP_OPT_PACKED = 0): phased segments (lag = S),
    unbounded links, more segments than resident slots.  All 4096 costs, and scenarios 0, 2047 and
    4095 plan for plan."""
    conts, nodes, plans = big_batch
    S, C, base = len(conts), conts[0][0].size, 0
    kw = dict(pipe_w=1, pipe_seg=12)
    if packed is not None:
        kw["packed"] = packed
    opts(**kw)
    geo = planner.geometry(S, C, N)
    assert (geo["groups"], geo["stages"], geo["segments"]) == (12, 1, 3), geo
    assert geo["lag"] == S and geo["bounded"] == 0, geo
    assert geo["segments"] * S > geo["resident"], geo
    assign, reason, cost, after = _place(planner, conts, nodes, base)
    path = planner.place_path()
    assert path["ran"] and path["packed"] == (packed is None), path
    ecost = np.array([p[3] for p in plans], np.uint64)
    bad = np.nonzero(cost != ecost)[0]
    assert bad.size == 0, f"{bad.size} scenario costs differ, first {bad[:8].tolist()}"
    for s in (0, 2047, 4095):
        ea, er, eafter, _ = plans[s]
        assert np.array_equal(assign[s * C:(s + 1) * C], ea), s
        assert np.array_equal(reason[s * C:(s + 1) * C], er), s
        for i in (0, 1, 3):
            assert np.array_equal(after[i][s * N:(s + 1) * N], eafter[i]), (s, i)
