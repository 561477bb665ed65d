"""Hand-made traps of SPEC.md 2.19 (the rebalance sweep), shared by the CPU tests (on the numpy reference) and the
GPU tests (on the device).  TEST INFRASTRUCTURE ONLY.

Every trap is (name, inputs, expected): ``inputs`` are the keyword arguments of ``rebalance_ref.sweep`` and of
``Planner.rebalance_sweep``, ``expected`` the values worked out by hand in the comments, each for variant 0:
assign_out, hops, reason and the eight summary words (moves, stuck, stuck_skew, relaxed, moved_cpu, moved_mem,
skew_before, skew_after).  Every container asks for 1 MiB, so moved_mem is the number of moves.
"""
import numpy as np

NONE = 0xFFFFFFFF
NOFIT, SKEW = 1, 3
FIRST_FIT = 0


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def _nodes(cf, lab=None, sched=None, cu=None):
    n = len(cf)
    return _u(cf, [1 << 20] * n, lab or [0] * n, cu or [0] * n) + (np.array(sched or [1] * n, np.uint8),)


def _cont(cpu, req=None, conf=None):
    n = len(cpu)
    return _u(cpu, [1] * n, req or [0] * n, conf or [0] * n)


def traps():
    out = []
    # ---- second pass.  Domains A = {0}, M = {1}, L = {2} with 5, 2 and 0 services (M's two belong to other tables:
    # node_count charges them), max_skew 2: only A is heavy (5 - 0 > 2; M's 2 - 0 is not).  Service 0 is big (50)
    # and fits only nodes 0 and 1; L has room for one small service.  Order [0, 1, 0]:
    #   0: lifted, A = 4.  L passes (0 - 0 < 2) and is too small, M fits and fails (2 - 0 < 2 is false), and so
    #      does A itself: SKEW, put back
    #   1: lifted, goes to L: A = 4, M = 2, L = 1, min 1, A still heavy (4 - 1 > 2)
    #   0: lifted, A = 3; now M passes (2 - 1 < 2): the big one goes to node 1.  A = 3, M = 3, L = 1: skew 2
    out.append(("second pass",
                dict(cont=_cont([50, 10, 10, 10, 10]), nodes=_nodes([0, 100, 10]), assign=[0] * 5, victim_order=[[0, 1, 0]],
                     strategy=FIRST_FIT, node_count=[5, 2, 0], domain=[0, 1, 2], max_skew=2, relax_mask=()),
                dict(out=[1, 2, 0, 0, 0], hops=[0] * 5, reason=[0] * 5, summary=[2, 1, 1, 0, 60, 2, 5, 2])))
    # ---- NOFIT.  A = {0 (cordoned), 1 (full)}, L = {2} with room for 10.  A holds three services of 50 on node 0,
    # counts derived: A = 3, L = 0, max_skew 1: heavy, and eligible through node 1.  Service 0 is lifted off the
    # cordoned node, which is no target; node 1 is full; node 2 is too small, also at the last hop (the service
    # requires label bit 0, which the chain gives up and node 2 lacks anyway): NOFIT, not SKEW
    out.append(("NOFIT even at the last hop",
                dict(cont=_cont([50, 50, 50], req=[1, 0, 0]), nodes=_nodes([0, 0, 10], lab=[1, 1, 0], sched=[0, 1, 1]),
                     assign=[0, 0, 0], victim_order=[[0]], strategy=FIRST_FIT, node_count=None, domain=[0, 0, 1],
                     max_skew=1, relax_mask=(1,)),
                dict(out=[0, 0, 0], hops=[0] * 3, reason=[NOFIT, 0, 0], summary=[0, 1, 0, 0, 0, 0, 3, 3])))
    # ---- reversal.  A = {0, 1 (cordoned)}, L = {2} (full).  Node 0's conflict_used is 0b100: it LACKS the bit of
    # service 0 (conflict 0b001), which runs there.  Services 0 (on node 0) and 1 (on node 1) both carry 0b001.
    #   0: lifted (conflict_used stays 0b100, cpu_free 10 -> 20); node 0 fits and fails the skew test, L is full:
    #      SKEW.  The reversal must leave 0b100; `|= conflict` would leave 0b101
    #   1: lifted off the cordoned node 1; node 0 (cpu_free 10, 0b100 & 0b001 == 0) fits and fails the skew test:
    #      SKEW.  With 0b101 on node 0 it would be NOFIT
    out.append(("a reversal restores the conflict word",
                dict(cont=_cont([10, 10], conf=[1, 1]), nodes=_nodes([10, 0, 0], sched=[1, 0, 1], cu=[4, 0, 0]),
                     assign=[0, 1], victim_order=[[0, 1]], strategy=FIRST_FIT, node_count=None, domain=[0, 0, 1],
                     max_skew=1, relax_mask=()),
                dict(out=[0, 1], hops=[0, 0], reason=[SKEW, SKEW], summary=[0, 2, 2, 0, 0, 0, 2, 2])))
    # ---- cordoned heavy zone.  A = {0} is cordoned with five services: not eligible, so never heavy and outside the
    # skew.  M = {1} has three, L = {2} none, max_skew 1: M is heavy.  Order [0, 5, 1, 6]: service 0 (A) is skipped,
    # 5 (M) goes to L (M = 2, L = 1: 2 - 1 is not > 1), 1 and 6 are skipped.  Skew over M and L: 3, then 1
    out.append(("a cordoned heavy zone gives no victims",
                dict(cont=_cont([10] * 8), nodes=_nodes([100, 100, 100], sched=[0, 1, 1]), assign=[0] * 5 + [1] * 3,
                     victim_order=[[0, 5, 1, 6]], strategy=FIRST_FIT, node_count=None, domain=[0, 1, 2], max_skew=1,
                     relax_mask=()),
                dict(out=[0] * 5 + [2, 1, 1], hops=[0] * 8, reason=[0] * 8, summary=[1, 0, 0, 0, 10, 1, 3, 1])))
    # ---- a unique minimum raised.  A = {0} has four, B = {1} three, L = {2} none, max_skew 2: A and B are heavy.
    # Order [0, 4]: service 0 (A) goes to L; the minimum was L's alone and is now 1, so B (3 - 1 = 2) is heavy no
    # more and service 4 (B) is skipped although its lane was a candidate when the chunk began.  Skew 4, then 2
    out.append(("a move raises the unique minimum",
                dict(cont=_cont([10] * 7), nodes=_nodes([100, 100, 100]), assign=[0] * 4 + [1] * 3, victim_order=[[0, 4]],
                     strategy=FIRST_FIT, node_count=None, domain=[0, 1, 2], max_skew=2, relax_mask=()),
                dict(out=[2, 0, 0, 0, 1, 1, 1], hops=[0] * 7, reason=[0] * 7, summary=[1, 0, 0, 0, 10, 1, 4, 2])))
    # ---- the budget, mid-chunk.  A = {0} has ten, L = {1} none, max_skew 1.  Unlimited, five move (5 and 5); with
    # a budget of 2 the variant ends right after the second move: A = 8, L = 2
    ten = dict(cont=_cont([10] * 10), nodes=_nodes([100, 100]), assign=[0] * 10, victim_order=[list(range(10))],
               strategy=FIRST_FIT, node_count=None, domain=[0, 1], max_skew=1, relax_mask=())
    out.append(("the budget ends a variant mid-chunk", dict(ten, max_moves=[2]),
                dict(out=[1, 1] + [0] * 8, hops=[0] * 10, reason=[0] * 10, summary=[2, 0, 0, 0, 20, 2, 10, 6])))
    out.append(("no budget", dict(ten, max_moves=[NONE]),
                dict(out=[1] * 5 + [0] * 5, hops=[0] * 10, reason=[0] * 10, summary=[5, 0, 0, 0, 50, 5, 10, 0])))
    # ---- duplicates.  A = {0} has twelve, L = {1} none, max_skew 1.  The order is 0, 0, 1, 2, 61 holes, 2, 3 (67
    # entries: the second 2 lies in the second chunk of 64).  Service 0 moves; its second entry, in the same chunk,
    # names a service that now sits in L and is skipped (a lane that still held node 0 for it would move it
    # again); 1 and 2 move (A = 9, L = 3); the second 2 reads the row the move wrote and is skipped; 3 moves
    out.append(("a duplicate inside a chunk and one across two",
                dict(cont=_cont([10] * 12), nodes=_nodes([100, 1000]), assign=[0] * 12,
                     victim_order=[[0, 0, 1, 2] + [NONE] * 61 + [2, 3]], strategy=FIRST_FIT, node_count=None,
                     domain=[0, 1], max_skew=1, relax_mask=()),
                dict(out=[1] * 4 + [0] * 8, hops=[0] * 12, reason=[0] * 12, summary=[4, 0, 0, 0, 40, 4, 12, 4])))
    return out
