"""GPU tests of the resource quota (SPEC.md 2.10; k_policy<.., .., .., true> in fleetflow_amd/csrc/fp_policy.hip):
every entry point against the numpy reference (tests/policy_quota_ref.py).  Every comparison is exact: assign,
reason, hops, quota_why, the usage after the call, the three mutated node arrays, node_count and the packed
cost.  Inputs come from the SPEC.md 3.2 generators (oracle/pyoracle.py) unless a test crafts its own."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_fallback_cases as K  # noqa: E402
import policy_fallback_ref as FR  # noqa: E402
import policy_quota_ref as QR  # noqa: E402
import policy_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U = QR.UNLIMITED
QUOTA = QR.REASON_QUOTA
SEED = 0x5EED0007


@functools.lru_cache(maxsize=None)
def _gen(seed, C, N):
    from oracle import pyoracle as P
    cont = tuple(np.array(x, np.uint32) for x in P.gen_containers(seed, C, 7))
    nd = P.gen_nodes(seed, N)
    return cont, tuple(np.array(x, np.uint32) for x in nd[:4]) + (np.array(nd[4], np.uint8),)


def _check(got, exp, sid=None):
    """got: (assign, reason, hops, cost or None, nodes_after, count or None, why or None, used or None); exp: the
    reference's (assign, reason, hops, nodes_after, count, why, used)."""
    assign, reason, hops, cost, after, cnt, why, used = got
    assert np.array_equal(assign, exp[0])
    assert np.array_equal(reason, exp[1])
    assert np.array_equal(hops, exp[2])
    for i in (0, 1, 3):
        assert np.array_equal(after[i], exp[3][i]), i
    if cnt is not None:
        assert np.array_equal(cnt, exp[4])
    if why is not None:
        assert np.array_equal(why, exp[5])
    if used is not None:
        assert np.array_equal(used, exp[6])
    if cost is not None:
        assert int(cost) == QR.cost(exp[0], exp[1], sid)


def _run1(planner, cont, nodes, strategy, quota, used=None, relax=(), domain=None, max_skew=None, preferred=0, level=None,
          node_count=None, sid=0):
    """One scenario through the batch entry (it returns the cost too)."""
    C, N = cont[0].size, nodes[0].size
    a, r, h, cost, after, cnt, why, qu = planner.place_batch_policy_quota(
        1, C, N, cont, nodes, [strategy], quota, used, [preferred], level=level, node_count=node_count, scen_base=sid,
        domain=domain, max_skew=None if max_skew is None else [max_skew],
        relax_mask=K.relax_rows([relax]) if relax else None, n_hops=[len(relax)] if relax else None)
    return a, r, h, cost[0], after, cnt, why, qu


# ---- 1. every variant ---------------------------------------------------------------------------------------
# 64 x 1 and 1024 x {1, 2, 4, 8}, each at an edge; C = 130 crosses two 64-record chunks
MODES = {"plain": (False, False), "spread": (True, False), "chain": (False, True), "both": (True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("N", [5, 64, 65, 1024, 1025, 2049, 4097, 8192])
def test_every_variant_vs_reference(N, strategy, mode, planner):
    C = 130
    cont, nodes = _gen(SEED, C, N)
    sp, fb = MODES[mode]
    kw = dict(preferred=(1 << 4) | (1 << 8), node_count=np.zeros(N, np.uint32))
    if sp:
        kw.update(domain=(np.arange(N) % 5).astype(np.uint32), max_skew=2)
    relax = K.RELAX[2] if fb else ()
    free = FR.place(cont, nodes, strategy, relax_mask=relax, **kw)
    u = QR.usage(cont, free[0])
    # fractions of the unconstrained usage, so the caps bite at every N; the tenant already holds something
    quota, used = (u[0] * 7 // 10 + 100, u[1] * 3 // 5 + 64, u[2] * 4 // 5 + 2), (100, 64, 2)
    exp = QR.place(cont, nodes, strategy, quota, used, relax_mask=relax, **kw)
    assert (exp[1] == QUOTA).sum() >= 1 and (exp[0] != NONE).sum() >= 1  # a condition on the inputs
    got = _run1(planner, cont, nodes, strategy, quota, used, relax, kw.get("domain"), kw.get("max_skew"), kw["preferred"],
                node_count=kw["node_count"], sid=7)
    _check(got, exp, 7)


def test_calibration_of_the_reference():
    """The figures the quota was specified with (a sanity aid for the reference; no GPU work)."""
    cont, nodes = _gen(0x5EED0002, 200, 20)
    e = QR.place(cont, nodes, R.SPREAD, (U, 749056, 171))
    assert ((e[0] != NONE).sum(), (e[1] == 1).sum(), (e[1] == QUOTA).sum()) == (98, 1, 101)
    assert set(e[5][e[1] == QUOTA]) == {2} and tuple(int(x) for x in e[6]) == (300150, 748992, 98)
    cont, nodes = _gen(0x5EED0007, 130, 9)
    assert {4, 5} <= set(QR.place(cont, nodes, R.SPREAD, (150885, 375289, 45))[5])


# ---- 2. skipped reductions ----------------------------------------------------------------------------------
def _crafted(big_at, cycle_at=(), big_mem=8192):
    """C = 193, N = 70 (the 1024-thread block with its LDS slots).  cpu strictly descending: the FFD order is the
    index order.  The containers at ``big_at`` ask for ``big_mem`` MiB, the others for 64; every node takes
    everything.  SPREAD from zero counts sends the k-th placed container to node k % 70.
    (Alternating 4096 / 64 cannot do what this case is for: the 96 small containers ask for 6144 MiB together, so
    a cap that admits them all admits the first large one too.  A large container has to ask for more than all
    the small ones together: 8192.)"""
    C, N = 193, 70
    cpu = (1000 - np.arange(C)).astype(np.uint32)
    mem = np.full(C, 64, np.uint32)
    mem[list(big_at)] = big_mem
    z = np.zeros(C, np.uint32)
    level = np.zeros(C, np.uint32)
    level[list(cycle_at)] = NONE
    nodes = (np.full(N, 10 ** 6, np.uint32), np.full(N, 10 ** 6, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32),
             np.ones(N, np.uint8))
    small = np.ones(C, bool)
    small[list(big_at)] = False
    small[list(cycle_at)] = False
    # the cap is exactly what the small containers ask for: every one of them goes in (the last on an exact
    # remainder) and no large one ever does
    cap = 64 * int(small.sum())
    assert cap < big_mem
    a = np.full(C, NONE, np.uint32)
    a[small] = np.arange(small.sum()) % N
    r = np.zeros(C, np.uint8)
    r[list(big_at)] = QUOTA
    r[list(cycle_at)] = 2
    why = np.where(r == QUOTA, 2, 0).astype(np.uint8)
    used = (int(cpu[small].sum()), cap, int(small.sum()))
    return (cpu, mem, z, z), nodes, level, (U, cap, U), a, r, why, used


@pytest.mark.parametrize("case", ["alternate", "chunk_edges"])
def test_skipped_reductions_closed_form(case, planner):
    """QUOTA containers run no reduction and no barrier: with placements between them the slot parity must
    still count reductions, whatever the number of skipped containers (an even run, an odd run, none)."""
    if case == "alternate":
        big, cyc = range(0, 193, 2), ()
    else:  # QUOTA at the chunk edges of the order, CYCLE containers between them
        big, cyc = (63, 64, 128), (5, 62, 65, 66, 100, 127, 129, 192)
    cont, nodes, level, quota, a, r, why, used = _crafted(big, cyc, 8192 if case == "alternate" else 16384)
    exp = QR.place(cont, nodes, R.SPREAD, quota, level=level)
    assert np.array_equal(exp[0], a) and np.array_equal(exp[1], r) and np.array_equal(exp[5], why)  # the closed form
    assert tuple(int(x) for x in exp[6]) == used
    got = planner.place_policy_quota(cont, nodes, R.SPREAD, quota, level=level, node_count=np.zeros(70, np.uint32))
    ga, gr, gh, after, cnt, gwhy, gused = got
    assert np.array_equal(ga, a) and np.array_equal(gr, r) and np.array_equal(gwhy, why) and not gh.any()
    assert tuple(int(x) for x in gused) == used
    assert np.array_equal(cnt, np.bincount(a[a != NONE], minlength=70))
    _check((ga, gr, gh, None, after, cnt, gwhy, gused), exp)


# ---- 3. the edges of the rule -------------------------------------------------------------------------------
def _small_nodes(N=6, cpu=4000, mem=4096):
    return (np.full(N, cpu, np.uint32), np.full(N, mem, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32),
            np.ones(N, np.uint8))


def _cont(cpu, mem, req=None):
    z = np.zeros(len(cpu), np.uint32)
    return (np.array(cpu, np.uint32), np.array(mem, np.uint32), z if req is None else np.array(req, np.uint32), z)


def _both(planner, cont, nodes, strategy, quota, used=None, **kw):
    exp = QR.place(cont, nodes, strategy, quota, used, **kw)
    rm = kw.pop("relax_mask", ())
    a, r, h, after, cnt, why, qu = planner.place_policy_quota(cont, nodes, strategy, quota, used, rm, **kw)
    _check((a, r, h, None, after, cnt, why, qu), exp)
    return exp


def test_cap_zero_and_zero_requests(planner):
    cont = _cont([500, 0, 300, 0], [64, 128, 0, 0])
    e = _both(planner, cont, _small_nodes(), R.FIRST_FIT, (0, U, U))
    assert list(e[1]) == [QUOTA, 0, QUOTA, 0] and list(e[5]) == [1, 0, 1, 0] and list(e[6]) == [0, 128, 2]
    e = _both(planner, cont, _small_nodes(), R.FIRST_FIT, (0, 0, U))
    assert list(e[1]) == [QUOTA, QUOTA, QUOTA, 0] and list(e[5]) == [3, 2, 1, 0] and list(e[6]) == [0, 0, 1]
    e = _both(planner, cont, _small_nodes(), R.FIRST_FIT, (U, U, 0))  # services: every container asks for one
    assert (e[1] == QUOTA).all() and (e[5] == 4).all() and not e[6].any()


def test_used_against_the_cap_on_entry(planner):
    cont = _cont([500, 400, 300, 200], [64, 0, 64, 0])
    # used > quota: every non-zero request in that dimension is refused, a zero request passes, the usage stays
    e = _both(planner, cont, _small_nodes(), R.SPREAD, (U, 50, U), (7, 100, 3))
    assert list(e[1]) == [QUOTA, 0, QUOTA, 0] and list(e[6]) == [7 + 600, 100, 5]
    # used == quota
    e = _both(planner, cont, _small_nodes(), R.SPREAD, (U, 100, U), (7, 100, 3))
    assert list(e[1]) == [QUOTA, 0, QUOTA, 0] and list(e[6]) == [7 + 600, 100, 5]
    # a request exactly equal to the remainder goes in, the next one does not
    e = _both(planner, cont, _small_nodes(), R.SPREAD, (U, 164, U), (7, 100, 3))
    assert list(e[1]) == [0, 0, QUOTA, 0] and list(e[5]) == [0, 0, 2, 0] and list(e[6]) == [7 + 1100, 164, 6]
    # the usage of an uncapped dimension wraps (u32)
    e = _both(planner, cont, _small_nodes(), R.SPREAD, (U, U, 10), (0xFFFFFF00, 0, 0))
    assert not e[1].any() and list(e[6]) == [(0xFFFFFF00 + 1400) & U, 128, 4]
    # several dimensions at once
    e = _both(planner, cont, _small_nodes(), R.SPREAD, (450, 0, 1))
    assert list(e[5]) == [3, 0, 7, 5] and list(e[6]) == [400, 0, 1]


def test_nofit_and_cycle_are_not_charged(planner):
    cont = _cont([9000, 500, 400, 300], [64, 9000, 64, 64])  # the first two fit no node
    level = np.array([0, 0, NONE, 0], np.uint32)
    e = _both(planner, cont, _small_nodes(), R.PACK, (10000, 10000, 3), level=level)
    assert list(e[1]) == [1, 1, 2, 0] and not e[5].any() and list(e[6]) == [300, 64, 1]
    # under a cap that the NOFIT container would have used up, the one behind it still goes in
    e = _both(planner, cont, _small_nodes(), R.PACK, (9300, U, U), level=level)
    assert list(e[1]) == [1, 1, 2, 0] and list(e[6]) == [300, 64, 1]
    # CYCLE comes first: a CYCLE container over the cap is CYCLE, with quota_why 0
    e = _both(planner, cont, _small_nodes(), R.PACK, (350, U, U), level=level)
    assert list(e[1]) == [QUOTA, QUOTA, 2, 0] and list(e[5]) == [1, 1, 0, 0]
    # the cost counts QUOTA as rejected
    got = _run1(planner, cont, _small_nodes(), R.PACK, (350, U, U), level=level, sid=9)
    assert int(got[3]) >> 40 == 3 and (int(got[3]) >> 16) & 0xFFFFFF == 1 and int(got[3]) & 0xFFFF == 9


def test_quota_under_spread_and_chain(planner):
    """A QUOTA container moves no domain count (the containers placed after it prove that) and its hop is 0."""
    N = 6
    nodes = list(_small_nodes(N))
    nodes[2] = np.array([K.MASK["class"] & -K.MASK["class"]] * 2 + [0] * 4, np.uint32)  # nodes 0, 1 carry one class label
    lab = int(nodes[2][0])
    dom = np.array([0, 0, 1, 1, 2, 2], np.uint32)
    # in order: placed, QUOTA (memory), placed, ... with max_skew 1 every placement has to go to the emptiest domain
    cpu = [900, 800, 700, 600, 500, 400, 300]
    mem = [64, 2048, 64, 2048, 64, 64, 64]
    req = [lab, lab, 0, lab, lab, 0, lab]
    cont = _cont(cpu, mem, req)
    kw = dict(domain=dom, max_skew=1, relax_mask=[K.MASK["class"]], node_count=np.zeros(N, np.uint32))
    e = _both(planner, cont, tuple(nodes), R.FIRST_FIT, (U, 400, U), **kw)
    assert list(e[1]) == [0, QUOTA, 0, QUOTA, 0, 0, 0] and list(e[5]) == [0, 2, 0, 2, 0, 0, 0]
    assert not e[2][e[1] == QUOTA].any() and e[2].any()  # some container relaxes; no QUOTA container has a hop
    free = FR.place(cont, tuple(nodes), R.FIRST_FIT, **kw)
    assert not np.array_equal(free[0], e[0])  # and the quota changes the plan on these inputs


def test_null_outputs(planner):
    cont, nodes = _gen(SEED, 130, 65)
    u = QR.usage(cont, FR.place(cont, nodes, R.SPREAD)[0])
    quota = (u[0] // 2, u[1] // 2, U)
    exp = QR.place(cont, nodes, R.SPREAD, quota)
    a, r, h, after, cnt, why, used = planner.place_policy_quota(cont, nodes, R.SPREAD, quota, (5, 5, 5), want_used=False)
    assert used is None and cnt is None  # quota_used = NULL starts at zero, whatever the caller holds
    _check((a, r, h, None, after, None, why, None), exp)
    a, r, h, after, cnt, why, used = planner.place_policy_quota(cont, nodes, R.SPREAD, quota, want_why=False, want_hops=False)
    assert why is None and h is None and np.array_equal(a, exp[0]) and np.array_equal(r, exp[1]) and np.array_equal(used, exp[6])
    got = planner.place_batch_policy_quota(1, 130, 65, cont, nodes, [R.SPREAD], quota, want_why=False, want_used=False)
    assert got[6] is None and got[7] is None and np.array_equal(got[0], exp[0]) and int(got[3][0]) == QR.cost(exp[0], exp[1], 0)


# ---- 4. inherited behaviour -----------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_no_quota_is_the_fallback_entry(strategy, planner):
    C, N = 300, 200
    cont, nodes = K.crafted(C, N)
    rng = np.random.default_rng(9)
    cnt0 = rng.integers(0, 6, N).astype(np.uint32)
    level = np.where(rng.random(C) < 0.1, NONE, 0).astype(np.uint32)
    dom = (np.arange(N) % 3).astype(np.uint32)
    kw = dict(preferred=(1 << 4) | (1 << 8), level=level, node_count=cnt0, domain=dom, max_skew=3)
    fa, fr, fh, fafter, fcnt = planner.place_policy_fallback(cont, nodes, strategy, K.RELAX[2], **kw)
    assert (fr == 3).sum() + (fr == 1).sum() > 0 and (fh >= 1).sum() > 0 and (fr == 2).sum() > 0
    # quota = NULL: the fallback entry; quota_used is neither read nor written
    a, r, h, after, cnt, why, used = planner.place_policy_quota(cont, nodes, strategy, None, (1, 2, 3), K.RELAX[2], **kw)
    _check((a, r, h, None, after, cnt, why, used), (fa, fr, fh, fafter, fcnt, np.zeros(C, np.uint8), np.array([1, 2, 3], np.uint32)))
    # a row of three UNLIMITED: the same plan, quota_why all zero, usage = the sum over the placed containers
    a, r, h, after, cnt, why, used = planner.place_policy_quota(cont, nodes, strategy, (U, None, U), (1, 2, 3), K.RELAX[2], **kw)
    su = QR.usage(cont, fa)
    _check((a, r, h, None, after, cnt, why, used),
           (fa, fr, fh, fafter, fcnt, np.zeros(C, np.uint8), np.array([1 + su[0], 2 + su[1], 3 + su[2]], np.uint32)))
    # and the batch entries agree, cost included
    fb = planner.place_batch_policy_fallback(1, C, N, cont, nodes, [strategy], [kw["preferred"]], level=level, node_count=cnt0,
                                             scen_base=4, domain=dom, max_skew=[3], relax_mask=K.relax_rows([K.RELAX[2]]),
                                             n_hops=[2])
    for q in (None, [U, U, U]):
        qb = planner.place_batch_policy_quota(1, C, N, cont, nodes, [strategy], q, None, [kw["preferred"]], level=level,
                                              node_count=cnt0, scen_base=4, domain=dom, max_skew=[3],
                                              relax_mask=K.relax_rows([K.RELAX[2]]), n_hops=[2])
        assert all(np.array_equal(x, y) for x, y in zip(qb[:4], fb[:4])) and np.array_equal(qb[5], fb[5])
        assert all(np.array_equal(x, y) for x, y in zip(qb[4], fb[4])) and not qb[6].any()


# ---- 5. batch ---------------------------------------------------------------------------------------------------
def _batch_case(S, C, N):
    """Per-scenario caps (some rows UNLIMITED, some partly), usage on entry, strategy, preferred mask, max_skew
    (0 included) and n_hops (0 included), node counts on entry, CYCLE levels."""
    rng = np.random.default_rng(300 + S)
    scen = [_gen(SEED + (s % 3), C, N) for s in range(S)]
    strat = [int(x) for x in rng.integers(0, 4, S)]
    pref = [int(x) for x in rng.choice([0, (1 << 4) | (1 << 8), 1 << 11], S)]
    skew = [int(x) for x in rng.choice([0, 2, 3], S)]
    nh = [int(x) for x in rng.choice([0, 1, 2], S)]
    relax = [K.RELAX[4] for _ in range(S)]
    cnt0 = rng.integers(0, 3, S * N).astype(np.uint32)
    dom = rng.integers(0, 6, S * N).astype(np.uint32)
    level = np.where(rng.random(S * C) < 0.05, NONE, 0).astype(np.uint32)
    tot = [(int(sc[0][0].sum()), int(sc[0][1].sum()), C) for sc in scen]
    quota = np.array([[int(t * f) for t, f in zip(tot[s], rng.uniform(0.2, 0.7, 3))] for s in range(S)], np.uint32)
    quota[rng.random((S, 3)) < 0.25] = U
    quota[0] = [tot[0][0] // 3, tot[0][1] // 3, C // 2]
    if S > 1:
        quota[1] = U  # a row without a quota beside rows with one
    used0 = (quota.astype(np.uint64) * rng.uniform(0, 0.3, (S, 3))).astype(np.uint32)
    used0[quota == U] = rng.integers(0, 1000, int((quota == U).sum()))
    cat = lambda k, i: np.concatenate([sc[k][i] for sc in scen])  # noqa: E731
    cont, nodes = [cat(0, i) for i in range(4)], [cat(1, i) for i in range(5)]

    def one(s):
        c, n = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N)
        return QR.place(scen[s][0], scen[s][1], strat[s], quota[s], used0[s], preferred=pref[s], level=level[c],
                        node_count=cnt0[n], domain=dom[n], max_skew=skew[s], relax_mask=relax[s], n_hops=nh[s])
    return dict(cont=cont, nodes=nodes, strat=strat, pref=pref, skew=skew, nh=nh, relax=K.relax_rows(relax), cnt0=cnt0,
                dom=dom, level=level, quota=quota.reshape(-1), used0=used0.reshape(-1), one=one)


def _to_dev(b, S, C, N, base, with_level=True):
    import torch
    from fleetflow_amd import DevBatch
    dev = "cuda:0"
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)  # noqa: E731
    db = DevBatch.allocate(S, C, N, dev, scen_base=base, with_level=with_level)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu), (*b["cont"], *b["nodes"][:4])):
        dst.copy_(t32(src))
    if with_level:
        db.level.copy_(t32(b["level"]))
    db.sched.copy_(torch.from_numpy(np.ascontiguousarray(b["nodes"][4])).to(dev))
    return db, t32


@pytest.mark.parametrize("S,C,N", [(1, 130, 65), (3, 130, 65), (300, 40, 9)])
def test_batch_host_and_device(S, C, N, planner):
    import torch
    b = _batch_case(S, C, N)
    base = 1000
    a, r, h, cost, after, cnt, why, used = planner.place_batch_policy_quota(
        S, C, N, b["cont"], b["nodes"], b["strat"], b["quota"], b["used0"], b["pref"], level=b["level"], node_count=b["cnt0"],
        scen_base=base, domain=b["dom"], max_skew=b["skew"], relax_mask=b["relax"], n_hops=b["nh"])
    n_quota = n_placed = 0
    for s in range(S):
        c, n, q = slice(s * C, (s + 1) * C), slice(s * N, (s + 1) * N), slice(3 * s, 3 * s + 3)
        exp = b["one"](s)
        _check((a[c], r[c], h[c], cost[s], tuple(x[n] for x in after), cnt[n], why[c], used[q]), exp, base + s)
        n_quota += int((exp[1] == QUOTA).sum())
        n_placed += int((exp[0] != NONE).sum())
    assert n_quota >= 10 and n_placed >= 10  # on the reference
    db, t32 = _to_dev(b, S, C, N, base)
    cnt_t, used_t = t32(b["cnt0"]), t32(b["used0"])
    hops_t = torch.full((S * C,), 77, dtype=torch.uint8, device="cuda:0")
    why_t = torch.full((S * C,), 77, dtype=torch.uint8, device="cuda:0")
    planner.dev_place_batch_policy_quota(db, t32(b["strat"]), t32(b["quota"]), used_t, t32(b["pref"]), cnt_t,
                                         domain_t=t32(b["dom"]), max_skew_t=t32(b["skew"]), relax_mask_t=t32(b["relax"]),
                                         n_hops_t=t32(b["nh"]), hops_t=hops_t, quota_why_t=why_t)
    planner.sync()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert np.array_equal(u32(db.assign), a) and np.array_equal(db.reason.cpu().numpy(), r)
    assert np.array_equal(hops_t.cpu().numpy(), h) and np.array_equal(why_t.cpu().numpy(), why)
    assert np.array_equal(u32(used_t), used) and np.array_equal(db.cost.cpu().numpy().view(np.uint64), cost)
    for t, x in zip((db.cf, db.mf, db.cu, cnt_t), (after[0], after[1], after[3], cnt)):
        assert np.array_equal(u32(t), x)


def test_tier_what_if(planner):
    """The same cluster under rising caps, one scenario per quota tier: the device entry, then the best tier."""
    import torch
    S, C, N = 6, 130, 65
    cont, nodes = _gen(SEED, C, N)
    u = QR.usage(cont, FR.place(cont, nodes, R.FILL_LOWEST)[0])
    fr = [0.1, 0.25, 0.5, 0.75, 1.0]
    quota = np.array([[int(u[0] * f), int(u[1] * f), int(u[2] * f)] for f in fr] + [[U, U, U]], np.uint32)
    exp = [QR.place(cont, nodes, R.FILL_LOWEST, quota[s]) for s in range(S)]
    rej = [int((e[1] != 0).sum()) for e in exp]
    assert all(x >= y for x, y in zip(rej, rej[1:])) and rej[0] > rej[2] > rej[-1]  # on the reference
    costs = [QR.cost(e[0], e[1], s) for s, e in enumerate(exp)]
    b = dict(cont=[np.tile(x, S) for x in cont], nodes=[np.tile(x, S) for x in nodes])
    db, t32 = _to_dev(b, S, C, N, 0, with_level=False)
    why_t = torch.zeros(S * C, dtype=torch.uint8, device="cuda:0")
    used_t = torch.zeros(S * 3, dtype=torch.int32, device="cuda:0")
    best_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    planner.dev_place_batch_policy_quota(db, t32([R.FILL_LOWEST] * S), t32(quota.reshape(-1)), used_t, quota_why_t=why_t)
    planner.dev_argmin_cost(db.cost, best_t)
    planner.sync()
    assert [int(x) for x in db.cost.cpu().numpy().view(np.uint64)] == costs
    assert int(best_t.item()) == int(np.argmin(np.array(costs, np.uint64)))
    got_a, got_w = db.assign.cpu().numpy().view(np.uint32), why_t.cpu().numpy()
    for s, e in enumerate(exp):
        assert np.array_equal(got_a[s * C:(s + 1) * C], e[0]) and np.array_equal(got_w[s * C:(s + 1) * C], e[5])
        assert np.array_equal(used_t.cpu().numpy().view(np.uint32)[3 * s:3 * s + 3], e[6])


# ---- 6. errors write nothing ------------------------------------------------------------------------------------
def _host_call(planner, b, S, C, N, strat, dom, skew, nh, n_nodes=None):
    """fp_place_batch_policy_quota through ctypes on caller-owned buffers with a fill pattern.  Returns (rc,
    whether every output and in/out array is as it was)."""
    import ctypes as ct
    from fleetflow_amd import _lib
    from fleetflow_amd._lib import FpBatch
    L = _lib.load()
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).copy()  # noqa: E731
    p32 = lambda x: None if x is None else x.ctypes.data_as(_lib.u32p)  # noqa: E731
    p8 = lambda x: x.ctypes.data_as(_lib.u8p)  # noqa: E731
    cont = [u32(x) for x in b["cont"]]
    cf, mf, lab, cu = (u32(x) for x in b["nodes"][:4])
    sched = np.ascontiguousarray(b["nodes"][4], np.uint8).copy()
    cnt = np.full(S * N, 5, np.uint32)
    assign, reason = np.full(S * C, 0xABCDEF01, np.uint32), np.full(S * C, 9, np.uint8)
    hops, why = np.full(S * C, 77, np.uint8), np.full(S * C, 78, np.uint8)
    cost = np.full(S, 0x1234567890ABCDEF, np.uint64)
    used = np.full(S * 3, 0x600D, np.uint32)
    quota = u32(b["quota"])
    st, rm, hp = u32(strat), u32(b["relax"]), u32(nh)
    dm, sk = (u32(dom), u32(skew)) if dom is not None else (None, None)
    outs = (cf, mf, cu, cnt, assign, reason, hops, why, cost, used)
    before = [x.copy() for x in outs]
    bt = FpBatch(S, 0, C, N if n_nodes is None else n_nodes, *(x.ctypes.data for x in cont), None, cf.ctypes.data,
                 mf.ctypes.data, lab.ctypes.data, cu.ctypes.data, sched.ctypes.data, assign.ctypes.data, reason.ctypes.data,
                 cost.ctypes.data)
    rc = L.fp_place_batch_policy_quota(planner._ctx, ct.byref(bt), p32(st), None, p32(cnt), p32(dm), p32(sk), p32(rm), p32(hp),
                                       p8(hops), p32(quota), p32(used), p8(why))
    return rc, all(np.array_equal(x, y) for x, y in zip(before, outs))


def test_errors_write_nothing(planner):
    import torch
    from fleetflow_amd._lib import FP_EINVAL, FP_EOVERFLOW, FleetplaceError
    S, C, N = 3, 130, 65
    b = _batch_case(S, C, N)
    ok = dict(strat=b["strat"], dom=b["dom"], skew=[2, 2, 2], nh=b["nh"])
    bad_dom = b["dom"].copy()
    bad_dom[2 * N + 3] = 64
    cases = {"strategy": dict(ok, strat=[0, 1, 4]), "domain": dict(ok, dom=bad_dom), "n_hops": dict(ok, nh=[0, 5, 1])}
    for name, kw in cases.items():
        rc, untouched = _host_call(planner, b, S, C, N, **kw)
        assert rc == FP_EINVAL and untouched, name
    # N > 8192, without a constraint (whose domains the host would check first, N of them a scenario): refused
    # before any node array is read
    rc, untouched = _host_call(planner, b, S, C, N, n_nodes=8193, **dict(ok, dom=None, skew=None))
    assert rc == FP_EOVERFLOW and untouched
    rc, untouched = _host_call(planner, b, S, C, N, **ok)  # the same call, legal: it does write
    assert rc == 0 and not untouched
    # the device entry: found by the kernels, reported by sync(), nothing written
    for name, kw in cases.items():
        db, t32 = _to_dev(b, S, C, N, 0, with_level=False)
        db.assign.fill_(-7)
        db.reason.fill_(9)
        db.cost.fill_(-1)
        snap = db.node_snapshot()
        cnt_t = torch.full((S * N,), 5, dtype=torch.int32, device="cuda:0")
        used_t = torch.full((S * 3,), 0x600D, dtype=torch.int32, device="cuda:0")
        hops_t = torch.full((S * C,), 77, dtype=torch.uint8, device="cuda:0")
        why_t = torch.full((S * C,), 78, dtype=torch.uint8, device="cuda:0")
        planner.dev_place_batch_policy_quota(db, t32(kw["strat"]), t32(b["quota"]), used_t, None, cnt_t, domain_t=t32(kw["dom"]),
                                             max_skew_t=t32(kw["skew"]), relax_mask_t=t32(b["relax"]), n_hops_t=t32(kw["nh"]),
                                             hops_t=hops_t, quota_why_t=why_t)
        with pytest.raises(FleetplaceError) as e:
            planner.sync()
        assert e.value.code == FP_EINVAL, name
        assert bool((db.assign == -7).all()) and bool((db.reason == 9).all()) and bool((db.cost == -1).all())
        assert bool((hops_t == 77).all()) and bool((why_t == 78).all()) and bool((cnt_t == 5).all())
        assert bool((used_t == 0x600D).all())
        assert all(torch.equal(x, y) for x, y in zip(snap, (db.cf, db.mf, db.cu)))
        planner.sync()  # reported once
    # C == 0: nothing is launched, the in/out usage stays as given
    e0 = tuple(np.zeros(0, np.uint32) for _ in range(4))
    got = planner.place_policy_quota(e0, _small_nodes(), R.SPREAD, (1, 1, 1), (9, 8, 7))
    assert got[0].size == 0 and list(got[6]) == [9, 8, 7]


# ---- 7. diagnosis and front end -----------------------------------------------------------------------------------
def test_explain_batch_selects_the_quota_containers(planner):
    from fleetflow_amd import _lib
    S, C, N = 3, 130, 65
    b = _batch_case(S, C, N)
    a, r, h, cost, after, cnt, why, used = planner.place_batch_policy_quota(
        S, C, N, b["cont"], b["nodes"], b["strat"], b["quota"], b["used0"], level=b["level"])
    hist = planner.explain_batch(S, C, N, b["cont"], after, r, 1 << _lib.REASON_QUOTA)
    n_quota = [int((r[s * C:(s + 1) * C] == QUOTA).sum()) for s in range(S)]
    assert sum(n_quota) >= 10 and [int(x) for x in hist[:, _lib.EXPLAIN_HIST_SELECTED]] == n_quota
    # a QUOTA container was tried on no node: its row says what the nodes would say, and here most still fit
    assert int(hist[:, _lib.EXPLAIN_HIST_FITS].sum()) >= 1
    both = planner.explain_batch(S, C, N, b["cont"], after, r, (1 << _lib.REASON_QUOTA) | (1 << _lib.REASON_NOFIT))
    assert [int(x) for x in both[:, _lib.EXPLAIN_HIST_SELECTED]] == \
        [n + int((r[s * C:(s + 1) * C] == 1).sum()) for s, n in enumerate(n_quota)]


STAGE_KDL = """
project "demo"
server "n0" { capacity cpu=4000 memory=8192 }
server "n1" { capacity cpu=4000 memory=8192 }
service "db" { resources cpu=2000 memory=4096 }
service "api" { resources cpu=1500 memory=1024 }
service "web" { resources cpu=500 memory=256 }
service "cron" { }
service "huge" { resources cpu=100 memory=9000 }
stage "live" {
    service "db"
    service "api"
    service "web"
    service "cron"
    service "huge"
    server "n0"
    server "n1"
    %s
}
"""


def test_plan_stage_from_kdl_with_a_quota_node(planner):
    from fleetflow_amd.flow import plan_stage
    from fleetflow_amd.parser import parse_kdl_string
    from fleetflow_amd.plan_output import format_up_dry_run, plan_from_json, plan_to_json
    flow = parse_kdl_string(STAGE_KDL % "placement { quota cpu=2600 memory=20000 services=3 }")
    plain = parse_kdl_string(STAGE_KDL % "")
    base = plan_stage(plain, "live", planner)
    assert base.rejected == {"huge": "NOFIT"} and base.quota is None and base.quota_why == {}
    plan = plan_stage(flow, "live", planner, explain=True)
    # FFD order: db (2000) in; api (1500) over the cpu cap; web (500) in; huge is admitted, fits no server and is
    # not charged; cron asks for nothing and is held back by the service count alone -- which still has room
    assert plan.assignment == {"db": "n0", "web": "n0", "cron": "n0"}
    assert plan.rejected == {"api": "QUOTA", "huge": "NOFIT"} and plan.quota_why == {"api": ["cpu"]}
    assert plan.quota == (2600, 20000, 3) and plan.quota_used == (2500, 4352, 3)
    assert set(plan.why) == {"huge"}  # explain keeps selecting NOFIT and SKEW only
    out = format_up_dry_run(flow, "live", plan)
    assert "  配置クォータ: cpu 2500/2600, memory 4352/20000, services 3/3\n" in out
    assert "    配置先: (配置不可: QUOTA)\n    クォータ超過: cpu\n" in out
    assert plan_from_json(plan_to_json(plan)) == plan
    # with what the tenant holds already: one service left, and 3500 MiB
    plan = plan_stage(flow, "live", planner, quota_used=(0, 16500, 2))
    assert plan.assignment == {"api": "n0"} and plan.quota_used == (1500, 17524, 3)
    assert plan.rejected == {"db": "QUOTA", "web": "QUOTA", "cron": "QUOTA", "huge": "QUOTA"}
    assert plan.quota_why == {"db": ["memory"], "web": ["services"], "cron": ["services"], "huge": ["memory", "services"]}
    assert (plan.order, plan.levels, plan.level_order, plan.candidates) == (base.order, base.levels, base.level_order, base.candidates)
    assert "クォータ" not in format_up_dry_run(plain, "live", base)
