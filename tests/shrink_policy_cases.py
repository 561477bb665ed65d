"""Hand-made traps of SPEC.md 2.17 (the scale-in sweep under the policy), shared by the CPU tests (on the numpy
reference) and the GPU tests (on the device).  TEST INFRASTRUCTURE ONLY.

Every trap is (name, inputs, expected): ``inputs`` are the keyword arguments of ``shrink_policy_ref.sweep`` and of
``Planner.shrink_sweep_policy``, ``expected`` the values worked out by hand in the comments: assign_out, state,
blocker, blocker_reason, the first five summary words (released, tried, failed, moves, moved) and the policy row
(failed_skew, relaxed, skew_before, skew_after), each for variant 0 and over the first nodes only, so that a trap
can be padded with cordoned servers.
"""
import numpy as np

NONE = 0xFFFFFFFF
NEVER, RELEASED, FAILED = 0, 1, 2
NOFIT, SKEW = 1, 3
FIRST_FIT = 0


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def _nodes(cf, lab=None, sched=None):
    n = len(cf)
    return _u(cf, [1 << 20] * n, lab or [0] * n, [0] * n) + (np.array(sched or [1] * n, np.uint8),)


def _cont(cpu, req=None):
    n = len(cpu)
    return _u(cpu, [1] * n, req or [0] * n, [0] * n)


def traps():
    out = []
    # ---- the example the bound rule exists for.  Domains A = {0, 1}, B = {2}, C = {3}; node 0 runs five services,
    # node 1 is empty with room for four, nodes 2 and 3 are charged with 5 and 7 services of other tables.
    # Leaving node 0 out: A = 0, B = 5, C = 7, so under max_skew 2 four services go to node 1 (A = 4); then
    # B passes (5 - 4 < 2) and node 1 is full: the fifth goes to node 2.  A = 4, B = 6, C = 7: skew 3, before it
    # was 7 - 5 = 2.  3 > max_skew and 3 > 2: refused although every move passed; blocker NONE, reason SKEW
    five = dict(cont=_cont([10] * 5), nodes=_nodes([0, 40, 100, 100]), assign=[0] * 5, try_order=[[0]],
                strategy=FIRST_FIT, node_count=[5, 0, 5, 7], domain=[0, 0, 1, 2], relax_mask=())
    out.append(("the A=5/B=5/C=7 example", dict(five, max_skew=2),
                dict(out=[0] * 5, state=[FAILED, NEVER, NEVER, NEVER], blocker=[NONE] * 4, reason=[SKEW, 0, 0, 0],
                     summary=[0, 1, 1, 0, 0], row=[1, 0, 2, 2], hops=[0] * 5)))
    # the same under max_skew 3: the fourth still goes to node 1 (first fit, A passes), the fifth to node 2, and
    # 3 <= max_skew commits
    out.append(("the example within the bound", dict(five, max_skew=3),
                dict(out=[1, 1, 1, 1, 2], state=[RELEASED, NEVER, NEVER, NEVER], blocker=[NONE] * 4, reason=[0] * 4,
                     summary=[1, 1, 0, 5, 5], row=[0, 0, 2, 3], hops=[0] * 5)))
    # ---- an empty server the bound keeps: node_count charges node 0 with three services of other tables.
    # A = {0, 1} = 3 + 0, B = {2} = 3: skew 0.  Without node 0: A = 0, B = 3: skew 3 > max_skew 1 and > 0
    out.append(("an empty server refused by the bound",
                dict(cont=_cont([10]), nodes=_nodes([100, 100, 100]), assign=[2], try_order=[[0]], strategy=FIRST_FIT,
                     node_count=[3, 0, 3], domain=[0, 0, 1], max_skew=1, relax_mask=()),
                dict(out=[2], state=[FAILED, NEVER, NEVER], blocker=[NONE] * 3, reason=[SKEW, 0, 0],
                     summary=[0, 1, 1, 0, 0], row=[1, 0, 0, 0], hops=[0])))
    # ---- a stale domain count.  A = {0, 3}, B = {1}, C = {2}, max_skew 1.  Attempt on node 0 (services 0 and 1):
    # A = 1, B = 0, C = 0; service 0 goes to node 1 (B = 1); service 1 requires label bit 1, which only node 1
    # has, and B no longer passes (1 - 0 < 1 is false): SKEW, undone, B is 0 again.  Attempt on node 3 (service
    # 2): A = 2, B = 0, C = 0 and first fit takes node 1; with B left at 1 it would take node 2.  Bound: before
    # A = 3, B = 0, C = 0 (skew 3), after A = 2, B = 1, C = 0 (skew 2): above max_skew but no further out
    out.append(("a stale domain count after an undone SKEW attempt",
                dict(cont=_cont([20, 10, 10], req=[0, 2, 0]), nodes=_nodes([0, 100, 100, 0], lab=[0, 2, 0, 0]),
                     assign=[0, 0, 3], try_order=[[0, 3]], strategy=FIRST_FIT, node_count=[2, 0, 0, 1],
                     domain=[0, 1, 2, 0], max_skew=1, relax_mask=()),
                dict(out=[0, 0, 1], state=[FAILED, NEVER, NEVER, RELEASED], blocker=[1, NONE, NONE, NONE],
                     reason=[SKEW, 0, 0, 0], summary=[1, 2, 1, 1, 1], row=[1, 0, 3, 2], hops=[0, 0, 0])))
    # ---- hop 1 because the skew test closed the hop-0 pool.  A = {1} charged with 1, B = {2} = 0, C = {0}; the
    # service on node 0 requires label bit 0, which node 1 has; A does not pass (1 - 0 < 1 is false), so hop 0 has
    # no node and hop 1 (bit 0 given up) takes node 2.  Bound: before A = 1, B = 0, C = 1 (skew 1), after A = 1,
    # B = 1 (skew 0)
    hop = dict(cont=_cont([10], req=[1]), nodes=_nodes([0, 100, 100], lab=[1, 1, 0]), assign=[0], try_order=[[0]],
               strategy=FIRST_FIT, node_count=[1, 1, 0], domain=[2, 0, 1], max_skew=1)
    out.append(("hop 1 where the skew test closed the hop-0 pool", dict(hop, relax_mask=(1,)),
                dict(out=[2], state=[RELEASED, NEVER, NEVER], blocker=[NONE] * 3, reason=[0, 0, 0],
                     summary=[1, 1, 0, 1, 1], row=[0, 1, 1, 0], hops=[1])))
    # and without the chain the same service is the SKEW blocker
    out.append(("the same without a chain", dict(hop, relax_mask=()),
                dict(out=[0], state=[FAILED, NEVER, NEVER], blocker=[0, NONE, NONE], reason=[SKEW, 0, 0],
                     summary=[0, 1, 1, 0, 0], row=[1, 0, 1, 1], hops=[0])))
    return out


def padded(inputs, N):
    """The same trap with cordoned, full, empty servers of domain 63 behind it: another block geometry, and a
    domain id in the second mask word."""
    k = N - len(inputs["domain"])
    nodes = tuple(np.concatenate((x, np.zeros(k, x.dtype))) for x in inputs["nodes"])
    return dict(inputs, nodes=nodes, node_count=list(inputs["node_count"]) + [0] * k,
                domain=list(inputs["domain"]) + [63] * k)


def check(got, expected, what=""):
    """``got`` = (assign_out, state, blocker, summary, hops, blocker_reason, rows) of a sweep."""
    out, state, blocker, summary, hops, why, rows = got
    n = len(expected["state"])
    assert out[0].tolist() == expected["out"], what
    assert state[0][:n].tolist() == expected["state"] and not state[0][n:].any(), what
    assert blocker[0][:n].tolist() == expected["blocker"] and (blocker[0][n:] == NONE).all(), what
    assert why[0][:n].tolist() == expected["reason"] and not why[0][n:].any(), what
    assert summary[0][:5].tolist() == expected["summary"], what
    assert rows[0].tolist() == expected["row"], what
    assert hops[0].tolist() == expected["hops"], what
