"""Drain planning (SPEC.md 2.11) without a GPU: the numpy reference's edges spelled out, the Planner wrappers'
length checks and what they send to which export, ``Server.draining`` from registry rows, the live table
``drain_stage`` derives from a plan, and the report's text and JSON forms."""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_ref as D  # noqa: E402
import policy_ref as R  # noqa: E402

from fleetflow_amd import _lib  # noqa: E402
from fleetflow_amd import flow as F  # noqa: E402
from fleetflow_amd import plan_output as PO  # noqa: E402
from fleetflow_amd.planner import Planner  # noqa: E402
from fleetflow_amd.registry import node_table, server_from_row  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _u(*xs):
    return tuple(np.array(x, np.uint32) for x in xs)


def _nodes(cf, mf=None, lab=None, cu=None, sched=None):
    n = len(cf)
    return _u(cf, mf or [10 ** 6] * n, lab or [0] * n, cu or [0] * n) + (np.array(sched or [1] * n, np.uint8),)


def _cont(cpu, mem=None, req=None, conf=None):
    n = len(cpu)
    return _u(cpu, mem or [1] * n, req or [0] * n, conf or [0] * n)


# ---- the reference's edges ------------------------------------------------------------------------------

def test_ref_each_candidate_starts_from_the_same_base_state():
    """Two servers with one container each, one spare that holds exactly one of them: draining either server
    alone moves its container to the spare -- candidate 1 does not see candidate 0's move."""
    cont = _cont([50, 50])
    nodes = _nodes([0, 0, 50])  # live: the two containers are already deducted
    out, reason, s = D.sweep(cont, nodes, [0, 1], [0, 1, 2], 3)
    assert out.tolist() == [2, 2] and reason.tolist() == [0, 0]
    assert s[:, :7].tolist() == [[1, 0, 0, 0, 1, NONE, 1], [1, 0, 0, 0, 1, NONE, 1], [0, 0, 0, 0, 0, NONE, 0]]
    # the same two servers as ONE candidate: the second evictee (index order on the tie) finds the spare full
    out, reason, s = D.sweep(cont, nodes, [0, 1], [0, 0, NONE], 1)
    assert out.tolist() == [2, NONE] and reason.tolist() == [0, 1]
    assert s[0, :7].tolist() == [2, 1, 50, 1, 1, 1, 2]


def test_ref_order_ties_state_and_summary():
    """Visiting order (cpu desc, mem desc, index asc); moves see the state earlier moves left; nothing is
    returned to the drained node; the candidate's own nodes and unschedulable nodes are no targets."""
    cont = _cont([10, 30, 30, 20], mem=[1, 2, 2, 1], conf=[0, 1 << 16, 1 << 16, 0])
    # node 0 is drained; node 1 takes one of the anti-affine pair, node 2 (cordoned) nothing, node 3 the rest
    nodes = _nodes([1000, 45, 1000, 60], sched=[1, 1, 0, 1])
    out, reason, s = D.sweep(cont, nodes, [0, 0, 0, 0], [0, NONE, NONE, NONE], 1)
    # 1 -> node 1 (first fit), 2 conflicts there -> node 3; 3 (cpu 20) finds 15 on node 1 and 30 on node 3;
    # 0 (cpu 10) fits node 1
    assert out.tolist() == [1, 1, 3, 3] and reason.tolist() == [0, 0, 0, 0]
    assert s[0, :7].tolist() == [4, 0, 0, 0, 2, NONE, 1]
    # a smaller node 3: containers 3 and 0 come after the pair and are stranded by what it left
    nodes = _nodes([1000, 30, 1000, 35], sched=[1, 1, 0, 1])
    out, reason, s = D.sweep(cont, nodes, [0, 0, 0, 0], [0, NONE, NONE, NONE], 1)
    assert out.tolist() == [NONE, 1, 3, NONE] and reason.tolist() == [1, 0, 0, 1]
    assert s[0, :7].tolist() == [4, 2, 30, 2, 2, 3, 1]  # first stranded in visiting order: 3 (cpu 20) before 0
    for a in nodes:
        a.setflags(write=False)  # and no input is written
    D.sweep(cont, nodes, [0, 0, 0, 0], [0, NONE, NONE, NONE], 1, strategy=R.SPREAD, node_count=[4, 0, 0, 0])


def test_ref_not_running_no_group_everything_and_unschedulable_sources():
    cont = _cont([5, 5, 5])
    nodes = _nodes([100, 100, 100], sched=[0, 1, 1])
    # container 1 is not running; node 0 is unschedulable and still evacuated
    out, reason, s = D.sweep(cont, nodes, [0, NONE, 2], [0, 1, 2], 3, strategy=R.FILL_LOWEST)
    assert out.tolist() == [1, NONE, 1] and reason.tolist() == [0, 0, 0]
    assert s[:, D.EVICTED].tolist() == [1, 0, 1] and s[:, D.NODES].tolist() == [1, 0, 1]
    # no node belongs to a candidate: the plan stays, rows of zeros
    out, reason, s = D.sweep(cont, nodes, [0, NONE, 2], [NONE] * 3, 2)
    assert out.tolist() == [0, NONE, 2] and not reason.any()
    assert s[:, :7].tolist() == [[0, 0, 0, 0, 0, NONE, 0]] * 2
    # one candidate holds every node: nowhere to go
    out, reason, s = D.sweep(cont, nodes, [0, NONE, 2], [0, 0, 0], 1)
    assert out.tolist() == [NONE, NONE, NONE] and reason.tolist() == [1, 0, 1]
    assert s[0, :7].tolist() == [2, 2, 10, 2, 0, 0, 3]
    # sums wrap
    big = _cont([0xFFFFFFFF, 2], mem=[0x80000000, 0x80000001])
    s = D.sweep(big, _nodes([1, 1]), [0, 0], [0, 0], 1)[2]
    assert s[0, :7].tolist() == [2, 2, 1, 1, 0, 0, 2]


def test_ref_spread_counts_and_preferred_labels():
    cont = _cont([10, 10, 10])
    nodes = _nodes([100] * 4, lab=[0, 1, 2, 2])
    # SPREAD on the given counts (9, 1, 0, 5): node 2 (count 0); then nodes 1 and 2 tie at 1 -> the lower index;
    # then node 2 (1) is below node 1 (2)
    out = D.sweep(cont, nodes, [0, 0, 0], [0, NONE, NONE, NONE], 1, strategy=R.SPREAD, node_count=[9, 1, 0, 5])[0]
    assert out.tolist() == [2, 1, 2]
    # a preferred label outranks the primary key
    out = D.sweep(cont, nodes, [0, 0, 0], [0, NONE, NONE, NONE], 1, strategy=R.SPREAD, preferred=1,
                  node_count=[9, 7, 0, 0])[0]
    assert out.tolist() == [1, 1, 1]


# ---- the wrappers: length checks first, then what reaches the export ---------------------------------------

class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def _addr(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "_obj"):
        return ct.addressof(x._obj)
    return ct.cast(x, ct.c_void_p).value or 0


class _Rec:
    """Stands in for the library: records (name, args, the u32 words of the peeked arguments) and fills the
    outputs of a drain sweep with what ``answer`` gives."""

    def __init__(self, peek=None, answer=None):
        self.calls, self.peek, self.answer = [], peek or {}, answer

    def __getattr__(self, name):
        def export(*args):
            seen = {i: list(ct.cast(ct.c_void_p(_addr(args[i])), ct.POINTER(ct.c_uint32))[:n])
                    for i, n in self.peek.items()}
            self.calls.append((name, args, seen))
            if self.answer is not None:
                self.answer(args)
            return 0
        return export


def _planner(lib):
    q = object.__new__(Planner)
    q._L, q._ctx, q._tstream, q.device = lib, ct.c_void_p(0x5EED), None, 0
    q._dev = lambda fn, *a: fn(*a)
    return q


def _refused(msg, fn, *a, **kw):
    with pytest.raises(ValueError, match=re.escape(msg)):
        fn(*a, **kw)


def test_drain_sweep_length_checks():
    p = _planner(_NoLib())
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    for i in range(4):
        short = cont[:i] + (cont[i][:-1],) + cont[i + 1:]
        _refused("every container array must hold C entries", p.drain_sweep, short, nodes, [0, 0], [0, 1, 2], 3)
    for i in range(5):
        short = nodes[:i] + (nodes[i][:-1],) + nodes[i + 1:]
        _refused("every node array must hold N entries", p.drain_sweep, cont, short, [0, 0], [0, 1, 2], 3)
    _refused("assign must hold C entries", p.drain_sweep, cont, nodes, [0], [0, 1, 2], 3)
    _refused("group must hold N entries", p.drain_sweep, cont, nodes, [0, 0], [0, 1], 3)
    _refused("node_count must hold N entries", p.drain_sweep, cont, nodes, [0, 0], [0, 1, 2], 3, node_count=[0] * 4)
    _refused("n_cand must be a u32", p.drain_sweep, cont, nodes, [0, 0], [0, 1, 2], -1)
    _refused("n_cand must be a u32", p.drain_sweep, cont, nodes, [0, 0], [0, 1, 2], 1 << 32)
    with pytest.raises(ValueError, match="unknown placement strategy"):
        p.drain_sweep(cont, nodes, [0, 0], [0, 1, 2], 3, strategy="round_robin")
    _refused("assign must hold C entries", p.drain, cont, nodes, [0, 0, 0], [1, 0, 0])
    _refused("drain_mask must hold N entries", p.drain, cont, nodes, [0, 0], [1, 0])
    _refused("node_count must hold N entries", p.drain, cont, nodes, [0, 0], [1, 0, 0], node_count=[0, 0])


def test_drain_sweep_call():
    lib = _Rec(peek={3: 2, 4: 3, 8: 3})
    p = _planner(lib)
    cont, nodes = _cont([1, 1]), _nodes([9, 9, 9])
    out, reason, summary = p.drain_sweep(cont, nodes, [0, NONE], [0, 1, NONE], 2, "fill_lowest", -1, [4, 5, 6])
    (name, args, seen), = lib.calls
    assert name == "fp_drain_sweep" and len(args) == 12 == len(_lib.SIGNATURES[name][1]) and _addr(args[0]) == 0x5EED
    assert seen == {3: [0, NONE], 4: [0, 1, NONE], 8: [4, 5, 6]}
    assert args[5:8] == (2, _lib.STRATEGY_FILL_LOWEST, 0xFFFFFFFF)
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, ns.n) == (2, 3) and cs.cpu_m == cont[0].ctypes.data and ns.cpu_free == nodes[0].ctypes.data  # no copy
    assert [_addr(args[i]) for i in (9, 10, 11)] == [out.ctypes.data, reason.ctypes.data, summary.ctypes.data]
    assert (out.dtype, reason.dtype, summary.shape) == (np.uint32, np.uint8, (2, _lib.DRAIN_WORDS))
    lib = _Rec()
    p = _planner(lib)
    p.drain_sweep(cont, nodes, [0, 1], [NONE] * 3, 0)
    args = lib.calls[0][1]
    assert args[5:8] == (0, 0, 0) and _addr(args[8]) == 0  # no node_count: NULL


def test_drain_applies_the_moves_on_the_host():
    """Planner.drain: one candidate from the mask, and the node table and counts after the moves are what
    policy_ref.place leaves when it places the evictees on the masked table."""
    cont = _cont([30, 20, 10, 40], mem=[3, 2, 1, 4], conf=[1, 2, 4, 8])
    nodes = _nodes([100, 100, 25, 100], sched=[1, 1, 1, 0])
    assign, cnt0 = [0, 0, 1, 0], [3, 1, 0, 0]

    def answer(args):
        grp = np.ctypeslib.as_array(ct.cast(args[4], ct.POINTER(ct.c_uint32)), (4,))
        assert grp.tolist() == [0, NONE, NONE, NONE] and args[5] == 1
        o, r, s = D.sweep(cont, nodes, assign, grp, 1, R.PACK, 0, cnt0)
        for dst, src in ((args[9], o), (args[11], s.reshape(-1))):
            ct.memmove(dst, src.ctypes.data, src.nbytes)
        ct.memmove(args[10], r.ctypes.data, r.nbytes)

    p = _planner(_Rec(answer=answer))
    out, reason, after, cnt, row = p.drain(cont, nodes, assign, [1, 0, 0, 0], R.PACK, node_count=cnt0)
    ev, a, r = D.candidate(cont, nodes, assign, [0, NONE, NONE, NONE], 0, R.PACK, 0, cnt0)
    assert ev.tolist() == [0, 1, 3] and a.tolist() == [1, 2, 1] and out.tolist() == [1, 2, 1, 1]
    sched = np.array([0, 1, 1, 0], np.uint8)
    exp = R.place(tuple(x[ev] for x in cont), (*nodes[:4], sched), R.PACK, node_count=cnt0)
    for i in (0, 1, 3):
        assert np.array_equal(after[i], exp[2][i]) and after[i] is not nodes[i]
    assert np.array_equal(cnt, exp[3]) and cnt.tolist() == [3, 3, 1, 0]
    assert nodes[0].tolist() == [100, 100, 25, 100] and cnt0 == [3, 1, 0, 0]
    assert row[:7].tolist() == [3, 0, 0, 0, 2, NONE, 1] and not reason.any()


def test_dev_drain_sweep_call_and_checks():
    torch = pytest.importorskip("torch")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    C, N, K = 3, 2, 2
    cont_t, nodes_t = tuple(i32(C) for _ in range(4)), tuple(i32(N) for _ in range(4)) + (u8(N),)
    asg, grp, cnt, out, rs, sm = i32(C), i32(N), i32(N), i32(C), u8(C), i32(K * 8)
    lib = _Rec()
    q = _planner(lib)  # kept: a planner that goes away closes its context through the library
    q.dev_drain_sweep(cont_t, nodes_t, asg, grp, K, out, rs, sm, "pack_into_dedicated", 6, cnt)
    (name, args, _), = lib.calls
    assert name == "fp_dev_drain_sweep" and len(args) == 12 == len(_lib.SIGNATURES[name][1])
    cs, ns = args[1]._obj, args[2]._obj
    assert (cs.n, cs.cpu_m, cs.conflict) == (C, cont_t[0].data_ptr(), cont_t[3].data_ptr())
    assert (ns.n, ns.cpu_free, ns.schedulable) == (N, nodes_t[0].data_ptr(), nodes_t[4].data_ptr())
    assert args[5:8] == (K, _lib.STRATEGY_PACK, 6)
    assert [_addr(args[i]) for i in (3, 4, 8, 9, 10, 11)] == [t.data_ptr() for t in (asg, grp, cnt, out, rs, sm)]
    fn = _planner(_NoLib()).dev_drain_sweep
    _refused("every container tensor must hold C 32-bit entries", fn, cont_t[:3] + (i32(C + 1),), nodes_t, asg, grp, K,
             out, rs, sm)
    _refused("every node tensor must hold N entries", fn, cont_t, nodes_t[:4] + (i32(N),), asg, grp, K, out, rs, sm)
    _refused("assign_t must hold C 32-bit entries", fn, cont_t, nodes_t, i32(C - 1), grp, K, out, rs, sm)
    _refused("group_t must hold N 32-bit entries", fn, cont_t, nodes_t, asg, u8(N), K, out, rs, sm)
    _refused("count_t must hold N 32-bit entries", fn, cont_t, nodes_t, asg, grp, K, out, rs, sm, count_t=i32(N + 1))
    _refused("assign_out_t must hold C 32-bit entries", fn, cont_t, nodes_t, asg, grp, K, i32(C + 1), rs, sm)
    _refused("reason_t must hold C bytes", fn, cont_t, nodes_t, asg, grp, K, out, i32(C), sm)
    _refused("summary_t must hold n_cand * 8 32-bit entries", fn, cont_t, nodes_t, asg, grp, K, out, rs, i32(K * 8 - 1))


def test_abi_declares_the_drain_entries_everywhere():
    hdr = open(os.path.join(ROOT, "include", "fleetplace.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "integration", "fleetflow-placement", "src", "lib.rs")).read()
    for name in ("fp_drain_sweep", "fp_dev_drain_sweep"):
        assert f"int {name}(fp_ctx *ctx, const fp_containers *c, const fp_nodes *nodes" in hdr
        assert name in _lib.SIGNATURES and f"pub fn {name}(" in ffi
    assert "model.rs:435-442" in hdr and "ffi::fp_drain_sweep(" in lib
    words = dict(re.findall(r"(FP_DRAIN_\w+) = (\d+)", hdr))
    assert words == {"FP_DRAIN_EVICTED": "0", "FP_DRAIN_STRANDED": "1", "FP_DRAIN_STRANDED_CPU": "2",
                     "FP_DRAIN_STRANDED_MEM": "3", "FP_DRAIN_TARGETS": "4", "FP_DRAIN_FIRST_STRANDED": "5",
                     "FP_DRAIN_NODES": "6", "FP_DRAIN_WORDS": "8"}
    for name, val in words.items():
        assert getattr(_lib, name[3:]) == int(val) == getattr(D, name[9:])
        assert re.search(rf"pub const {name}: usize = {val};", ffi), name


# ---- the flow level ------------------------------------------------------------------------------------

def test_server_draining_from_registry_rows():
    assert F.Server("a").draining is False
    rows = [{"slug": "c", "scheduling": "drain"}, {"slug": "a", "scheduling": "cordon"}, {"slug": "b"},
            {"slug": "d", "scheduling": "schedulable"}]
    got = {s.slug: (s.schedulable, s.draining) for s in node_table(rows)}
    assert got == {"a": (False, False), "b": (True, False), "c": (False, True), "d": (True, False)}
    assert server_from_row({"slug": "x", "scheduling": None}).draining is False


class _RefPlanner:
    """drain_sweep answered by the numpy reference; remembers what it was asked."""

    def drain_sweep(self, cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None):
        self.asked = (cont, nodes, assign, group, n_cand, strategy, preferred, node_count)
        return D.sweep(cont, nodes, assign, group, n_cand, _lib.POLICY_STRATEGIES.get(strategy, strategy), preferred,
                       node_count)


def _flow():
    f = F.Flow("shop")
    spec = {"db": (3000, 4096, ["class=ssd"], None), "api": (1000, 1024, [], "web"), "web": (1000, 512, [], "web"),
            "cache": (500, 2048, [], None), "cron": (250, 128, [], None), "batch": (2500, 1024, [], None)}
    for name, (cpu, mem, labels, group) in spec.items():
        f.services[name] = F.Service(cpu_m=cpu, mem_mib=mem, labels=labels, anti_affinity=group)
    servers = [("a1", 4000, 8192, ["region=east", "class=ssd"]), ("a2", 4000, 8192, ["region=east"]),
               ("b1", 4000, 8192, ["region=west"]), ("b2", 2000, 4096, ["region=west"]),
               ("c1", 4000, 8192, [])]
    for slug, cpu, mem, labels in servers:
        f.servers[slug] = F.Server(slug, cpu, mem, labels)
    f.stages["live"] = F.Stage(services=list(spec), servers=[s[0] for s in servers])
    return f


def _plan_by_reference(f, policy):
    """The plan policy_ref.place makes of the stage, as a flow.Plan, and the table it leaves."""
    stage = f.stages["live"]
    nodes = [f.servers[s] for s in stage.servers]
    cont, ntab = F._stage_tables(stage.services, f, nodes, policy.preferred)
    pmask = F._stage_labels(stage.services, f, nodes, policy.preferred).mask(policy.preferred)
    st = _lib.POLICY_STRATEGIES.get(policy.strategy, 0)
    a, r, after, cnt = R.place(cont, ntab, st, pmask)
    plan = F.Plan("live", [], {}, [], {n: stage.servers[a[v]] for v, n in enumerate(stage.services) if a[v] != NONE},
                  {n: "NOFIT" for v, n in enumerate(stage.services) if a[v] == NONE})
    plan.strategy, plan.preferred = policy.strategy, policy.preferred
    return plan, (cont, a, after, cnt, st, pmask)


@pytest.mark.parametrize("strategy", [None, "spread_across_pool", "pack_into_dedicated", "fill_lowest"])
def test_live_table_is_what_the_placement_left(strategy):
    f = _flow()
    policy = F.PlacementPolicy(strategy, {"region": "west"})
    plan, (cont, a, after, cnt, st, pmask) = _plan_by_reference(f, policy)
    names, nodes, lcont, live, assign, count, lstrat, lmask = F.live_tables(f, "live", plan)
    assert names == f.stages["live"].services and [n.slug for n in nodes] == f.stages["live"].servers
    assert [list(x) for x in lcont] == [list(map(int, x)) for x in cont]
    for i in range(5):
        assert list(live[i]) == [int(x) for x in after[i]], i
    assert assign == [int(x) for x in a] and count == [int(x) for x in cnt]
    assert (lstrat, lmask) == (strategy, pmask) and len(plan.assignment) >= 5
    # an explicit policy overrides what the plan was made under
    other = F.PlacementPolicy("fill_lowest")
    assert F.live_tables(f, "live", plan, other)[6:] == ("fill_lowest", 0)
    plan.assignment["db"] = "z9"
    with pytest.raises(ValueError, match="no server of the stage"):
        F.live_tables(f, "live", plan)


def test_drain_stage_groupings_and_report():
    f = _flow()
    policy = F.PlacementPolicy("spread_across_pool")
    plan, (cont, a, after, cnt, st, pmask) = _plan_by_reference(f, policy)
    slugs = f.stages["live"].servers
    p = _RefPlanner()
    # each server on its own
    rep = F.drain_stage(f, "live", plan, planner=p)
    assert p.asked[3] == [0, 1, 2, 3, 4] and p.asked[4] == 5 and p.asked[5] == "spread_across_pool"
    assert p.asked[7] == [int(x) for x in cnt]
    assert [c.name for c in rep.candidates] == slugs and [c.servers for c in rep.candidates] == [[s] for s in slugs]
    assert (rep.stage, rep.by, rep.strategy) == ("live", None, "spread_across_pool")
    out, _, summ = D.sweep(cont, after, a, np.arange(5), 5, st, pmask, cnt)
    for k, c in enumerate(rep.candidates):
        ev = [v for v in R.ffd_order(cont[0], cont[1]) if a[v] == k]  # the visiting order
        assert c.moves == [(f.stages["live"].services[v], slugs[k], slugs[out[v]]) for v in ev if out[v] != NONE]
        assert c.stranded == [f.stages["live"].services[v] for v in ev if out[v] == NONE]
        assert (c.evicted, c.targets, c.stranded_cpu_m, c.stranded_mem_mib) == tuple(
            int(summ[k, i]) for i in (D.EVICTED, D.TARGETS, D.STRANDED_CPU, D.STRANDED_MEM))
    assert sum(c.evicted for c in rep.candidates) == len(plan.assignment)
    assert any(c.stranded for c in rep.candidates) and any(c.moves for c in rep.candidates)  # db needs class=ssd: only a1 has it
    # per value of a topology key: c1 has no region and belongs to no candidate
    rep = F.drain_stage(f, "live", plan, by="region", planner=p)
    assert p.asked[3] == [0, 0, 1, 1, NONE] and p.asked[4] == 2 and rep.by == "region"
    assert [(c.name, c.servers) for c in rep.candidates] == [("region=east", ["a1", "a2"]), ("region=west", ["b1", "b2"])]
    # named servers: one candidate; an explicit policy's strategy
    rep = F.drain_stage(f, "live", plan, servers=["b2", "a1"], planner=p, policy=F.PlacementPolicy("fill_lowest"))
    assert p.asked[3] == [0, NONE, NONE, 0, NONE] and p.asked[4] == 1 and p.asked[5] == "fill_lowest"
    assert [(c.name, c.servers) for c in rep.candidates] == [("a1,b2", ["a1", "b2"])] and rep.strategy == "fill_lowest"
    with pytest.raises(ValueError, match="no servers of stage"):
        F.drain_stage(f, "live", plan, servers=["zz"], planner=p)
    # the default candidate: the servers the registry says are draining
    f.servers["a2"].draining = True
    f.servers["a2"].schedulable = False
    rep = F.drain_stage(f, "live", plan, planner=p)
    assert p.asked[3] == [NONE, 0, NONE, NONE, NONE] and [c.name for c in rep.candidates] == ["a2"]
    assert F.drain_stage(f, "live", plan, by="region", planner=p).by == "region"  # an explicit grouping wins


def test_report_text_and_json_round_trip():
    rep = F.DrainReport("live", "region", "fill_lowest", ["class=ssd"], [
        F.DrainCandidate("region=east", ["a1", "a2"], [("db", "a1", "b1"), ("api", "a2", "c1")], ["batch"], 3, 2500, 1024, 2),
        F.DrainCandidate("region=west", ["b1"], [], [], 0, 0, 0, 0)])
    assert PO.format_drain_report(rep) == (
        "drain region=east: 2 services move to 2 servers, 1 stranded\n"
        "  db: a1 -> b1\n"
        "  api: a2 -> c1\n"
        "  batch: stranded\n"
        "drain region=west: 0 services move to 0 servers, 0 stranded")
    text = PO.drain_report_to_json(rep)
    back = PO.drain_report_from_json(text)
    assert back == rep and isinstance(back.candidates[0].moves[0], tuple)
    assert PO.drain_report_to_json(back) == text and PO.drain_report_to_json(rep, indent=2) != text
    assert PO.drain_report_from_json(PO.drain_report_to_json(F.DrainReport("s"))) == F.DrainReport("s")
    assert PO.format_drain_report(F.DrainReport("s")) == ""
