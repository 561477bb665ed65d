"""Stage-2 feasibility sweep on the GPU (SPEC.md 2.5, k_feas in fp_feas.hip): fp_feasibility, fp_dev_feasibility
and fp_dev_feasibility_batch against the numpy reference of feas_ref.py on the inputs of feas_cases.py.

Every output word is compared -- all scenarios, all containers, the whole bitmap -- and every output starts as
a garbage pattern with a margin on both sides that must come back untouched; node tables must come back as
they were.  The shapes select the kernel's paths (a node range split over blockIdx.y or not, one LDS tile or
several, one scenario or a grid z of them); test_feas_host.py pins the launch each shape is named for.
"""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explain_ref as ER  # noqa: E402
import feas_cases as K  # noqa: E402
import feas_ref as FR  # noqa: E402
from test_feas_host import BATCH_PLANS, DEVICE_SHAPES, GRID_C, GRID_N, PERIOD, SINGLE_PLANS  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MARGIN = 64                        # words of margin on either side of an output
JUNK32, JUNK64 = 0x5A5AA5A5, 0x5A5AA5A55A5AA5A5  # positive as int32 / int64
DEV = "cuda:0"


# ---- outputs with a margin ------------------------------------------------------------------------------------
class HostOut:
    """A numpy output of n words inside a buffer of junk."""

    def __init__(self, n, dtype):
        self.junk = JUNK32 if np.dtype(dtype).itemsize == 4 else JUNK64
        self.buf = np.full(n + 2 * MARGIN, self.junk, dtype)
        self.out = self.buf[MARGIN:MARGIN + n]

    def ptr(self):
        return ct.c_void_p(self.out.ctypes.data if self.out.size else self.buf.ctypes.data + MARGIN * self.buf.itemsize)

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == self.junk).all() and (self.buf[MARGIN + self.out.size:] == self.junk).all())

    def untouched(self):
        return bool((self.buf == self.junk).all())


class DevOut:
    """A device output of n words (int32 or int64 storage) inside a buffer of junk."""

    def __init__(self, n, words64=False):
        import torch
        self.junk = JUNK64 if words64 else JUNK32
        self.buf = torch.full((n + 2 * MARGIN,), self.junk, dtype=torch.int64 if words64 else torch.int32, device=DEV)
        self.out = self.buf[MARGIN:MARGIN + n]
        self.n = n

    def refill(self):
        self.buf.fill_(self.junk)

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == self.junk).all()) and bool((self.buf[MARGIN + self.n:] == self.junk).all())

    def untouched(self):
        return bool((self.buf == self.junk).all())

    def host(self):
        return self.out.cpu().numpy().view(np.uint64 if self.out.element_size() == 8 else np.uint32)


def _t32(x):
    import torch
    return torch.from_numpy(np.array(x, np.uint32).view(np.int32)).to(DEV)


def _host_call(planner, cont, nodes, bitmap=True):
    """fp_feasibility through ctypes on outputs with margins: (rc, first, count, bitmap outputs)."""
    from fleetflow_amd import _lib
    from fleetflow_amd._lib import FpContainers, FpNodes
    arrs = [np.ascontiguousarray(a) for a in (*cont, *nodes)]
    C, N = arrs[0].size, arrs[4].size
    cs = FpContainers(C, *(x.ctypes.data for x in arrs[:4]))
    ns = FpNodes(N, *(x.ctypes.data for x in arrs[4:]))
    first, count, bm = HostOut(C, np.uint32), HostOut(C, np.uint32), HostOut(((C + 63) // 64) * N, np.uint64)
    rc = _lib.load().fp_feasibility(planner._ctx, ct.byref(cs), ct.byref(ns), ct.cast(first.ptr(), _lib.u32p),
                                    ct.cast(count.ptr(), _lib.u32p), ct.cast(bm.ptr(), _lib.u64p) if bitmap else None)
    return rc, first, count, bm


def _dev_batch(S, C, N, cont, nodes, scen_base=0):
    import torch
    from fleetflow_amd import DevBatch
    db = DevBatch.allocate(S, C, N, DEV, scen_base=scen_base)
    for dst, src in zip((db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu), (*cont, *nodes[:4])):
        dst.copy_(_t32(src))
    db.sched.copy_(torch.from_numpy(np.array(nodes[4], np.uint8)).to(DEV))
    return db


def _inputs(db):
    return (db.cpu, db.mem, db.req, db.conf, db.cf, db.mf, db.lab, db.cu, db.sched)


# ---- the edge grid through the host entry ---------------------------------------------------------------------
@pytest.mark.parametrize("N", GRID_N)
@pytest.mark.parametrize("C", GRID_C)
def test_edge_grid_host_entry(C, N, planner):
    """Container counts around the wave, the 256-thread row and the 1024-container block; node counts around
    one range of 64 (N <= 64 is not split) and around two, and one node past 1024.  With C % 64 != 0 the
    table with an accept-all node in every group of 64 runs too: a bitmap bit of an absent lane would show."""
    for mask in ((False, True) if C % 64 else (False,)):
        cont, nodes = K.case(C, N, mask_nodes=mask)
        snap = [np.array(a) for a in (*cont, *nodes)]
        ef, ec, eb = K.expected(C, N, mask_nodes=mask)
        rc, first, count, bm = _host_call(planner, cont, nodes)
        assert rc == 0
        assert np.array_equal(first.out, ef) and np.array_equal(count.out, ec) and np.array_equal(bm.out, eb)
        assert first.margins_intact() and count.margins_intact() and bm.margins_intact()
        rc, first, count, bm = _host_call(planner, cont, nodes, bitmap=False)
        assert rc == 0 and bm.untouched()
        assert np.array_equal(first.out, ef) and np.array_equal(count.out, ec)
        assert first.margins_intact() and count.margins_intact()
        assert all(np.array_equal(a, b) for a, b in zip(snap, (*cont, *nodes)))
        f2, c2, b2 = planner.feasibility(cont, nodes)  # the binding's own buffers
        assert np.array_equal(f2, ef) and np.array_equal(c2, ec) and np.array_equal(b2, eb)


# ---- the device entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", DEVICE_SHAPES)
@pytest.mark.parametrize("mask", [False, True])
def test_device_entry(C, N, mask, planner):
    """fp_dev_feasibility on each scenario of a DevBatch of three through offset pointers, with and without a
    bitmap: the reference, and what the host entry gives."""
    import torch
    S = 3
    scen = [K.case(C, N, seed=s, mask_nodes=mask) for s in range(S)]
    db = _dev_batch(S, C, N, [np.concatenate([sc[0][i] for sc in scen]) for i in range(4)],
                    [np.concatenate([sc[1][i] for sc in scen]) for i in range(5)])
    snap = [t.clone() for t in _inputs(db)]
    WN = ((C + 63) // 64) * N
    first, count, bm = DevOut(C), DevOut(C), DevOut(WN, words64=True)
    for s in range(S):
        ef, ec, eb = K.expected(C, N, seed=s, mask_nodes=mask)
        rc, hf, hc, hb = _host_call(planner, *scen[s])
        assert rc == 0 and np.array_equal(hf.out, ef) and np.array_equal(hc.out, ec) and np.array_equal(hb.out, eb)
        for with_bitmap in (True, False):
            for o in (first, count, bm):
                o.refill()
            planner.dev_feasibility(db, first.out, count.out, bm.out if with_bitmap else None, scenario=s)
            planner.sync()
            assert np.array_equal(first.host(), ef) and np.array_equal(count.host(), ec), (s, with_bitmap)
            assert first.margins_intact() and count.margins_intact()
            if with_bitmap:
                assert np.array_equal(bm.host(), eb) and bm.margins_intact()
            else:
                assert bm.untouched()
    assert all(torch.equal(a, b) for a, b in zip(snap, _inputs(db)))


# ---- the two large single calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", list(SINGLE_PLANS))
def test_single_call_over_several_tiles(C, N, planner):
    """The smallest single calls whose node range holds more than one LDS tile: 1024 container blocks before a
    range reaches 1152 nodes (split in two, tiles [1024, 128] and [1024, 24]), 2048 before the range is not
    split at all ([1024, 65]); one block fewer than that splits again.  The containers repeat a generated
    table of 64 * 37 rows -- no multiple of 256 or 1024, so every block sees another phase of it -- and the
    bitmap (about 290 MB) is compared on the device: row r is the reference's row r mod 37, the ragged last
    row, one container wide, is compared on its own."""
    import torch
    assert FR.feas_plan(None, C, N)[1:] == SINGLE_PLANS[(C, N)]
    WC, R = (C + 63) // 64, PERIOD // 64
    idx = np.arange(C) % PERIOD
    first, count, bm = DevOut(C), DevOut(C), DevOut(WC * N, words64=True)
    for mask in ((False, True) if C % 64 else (False,)):
        cont, nodes = K.case(PERIOD, N, mask_nodes=mask)
        ef, ec, eb = K.expected(PERIOD, N, mask_nodes=mask)
        ok = FR.ok_matrix(cont, nodes)
        db = _dev_batch(1, C, N, [a[idx] for a in cont], nodes)
        snap = [t.clone() for t in _inputs(db)]
        for o in (first, count, bm):
            o.refill()
        planner.dev_feasibility(db, first.out, count.out, bm.out)
        planner.sync()
        assert np.array_equal(first.host(), ef[idx]) and np.array_equal(count.host(), ec[idx])
        assert first.margins_intact() and count.margins_intact() and bm.margins_intact()
        ref = torch.from_numpy(np.array(eb).view(np.int64).reshape(R, N)).to(DEV)
        full = C // 64  # rows of 64 present containers
        rows = bm.out.view(WC, N)
        whole = full // R
        assert bool((rows[:whole * R].view(whole, R, N) == ref[None]).all())
        assert bool((rows[whole * R:full] == ref[:full - whole * R]).all())
        if C % 64:  # the last row: containers full * 64 .. C - 1 in the low bits, nothing above them
            tail = np.zeros(N, np.uint64)
            for b in range(C % 64):
                tail |= ok[(full * 64 + b) % PERIOD].astype(np.uint64) << np.uint64(b)
            assert np.array_equal(rows[full].cpu().numpy().view(np.uint64), tail)
        assert all(torch.equal(a, b) for a, b in zip(snap, _inputs(db)))
        del db, snap, ref, rows
    del first, count, bm
    torch.cuda.empty_cache()


# ---- the batch ------------------------------------------------------------------------------------------------
def _run_batch(planner, S, C, N, scen_base=0):
    import torch
    cont, nodes, _ = K.batch(S, C, N)
    db = _dev_batch(S, C, N, cont, nodes, scen_base=scen_base)
    snap = [t.clone() for t in _inputs(db)]
    first, count = DevOut(S * C), DevOut(S * C)
    planner.dev_feasibility_batch(db, first.out, count.out)
    planner.sync()
    assert first.margins_intact() and count.margins_intact()
    assert all(torch.equal(a, b) for a, b in zip(snap, _inputs(db)))
    return first, count


@pytest.mark.parametrize("S,C,N", list(BATCH_PLANS))
def test_batch_paths(S, C, N, planner):
    """(2048, 70, 2120), (1024, 1030, 2120) and (2048, 16, 5000): the unsplit range over several tiles, the
    benchmark's path, the last with the benchmark's five tiles; the second has two container blocks, the
    later one with 6 containers.  (2047, 70, 2120): split in two, two tiles each.  (1, 70, 2120): no grid z,
    no rebase.  (2, 1100, 64), (3, 1100, 64): unsplit single tile with a rebase.  (5, 1100, 0): memsets only.
    (5, 0, 40): nothing to write.  Scenario s is pool scenario s % P: all S * C outputs are compared."""
    assert FR.feas_plan(S, C, N)[1:] == BATCH_PLANS[(S, C, N)]
    first, count = _run_batch(planner, S, C, N)
    if C == 0:
        assert first.untouched() and count.untouched()
        return
    ef, ec = K.batch_expected(S, C, N)
    assert np.array_equal(first.host(), ef) and np.array_equal(count.host(), ec)
    if N == 0:
        assert (ef == NONE).all() and (ec == 0).all()


@pytest.mark.parametrize("S,C,N", [(3, 1100, 64), (2047, 70, 2120)])
def test_batch_scen_base_changes_nothing(S, C, N, planner):
    ef, ec = K.batch_expected(S, C, N)
    first, count = _run_batch(planner, S, C, N, scen_base=11)
    assert np.array_equal(first.host(), ef) and np.array_equal(count.host(), ec)


# ---- errors ---------------------------------------------------------------------------------------------------
def test_errors_write_nothing(planner):
    from fleetflow_amd import DevBatch, _lib
    from fleetflow_amd._lib import FP_EINVAL, FP_EOVERFLOW, FpContainers, FpNodes
    L = _lib.load()
    C, N = 300, 65
    cont, nodes = K.case(C, N)
    ef, ec, eb = K.expected(C, N)
    WN = ((C + 63) // 64) * N
    first, count, bm = DevOut(C), DevOut(C), DevOut(WN, words64=True)

    def works():
        for o in (first, count, bm):
            o.refill()
        planner.dev_feasibility(db, first.out, count.out, bm.out)
        planner.sync()
        assert np.array_equal(first.host(), ef) and np.array_equal(count.host(), ec) and np.array_equal(bm.host(), eb)
        for o in (first, count, bm):
            o.refill()

    db = _dev_batch(1, C, N, cont, nodes)
    works()
    # a grid z of 65 536 scenarios: one container on one node each, every array as long as the sizes say
    big = DevBatch.allocate(65536, 1, 1, DEV)
    for t in _inputs(big):
        t.zero_()
    bf, bc = DevOut(65536), DevOut(65536)
    assert L.fp_dev_feasibility_batch(planner._ctx, ct.byref(big.struct()), bf.out.data_ptr(), bc.out.data_ptr()) == FP_EOVERFLOW
    planner.sync()
    assert bf.untouched() and bc.untouched()
    works()
    # a null first with C > 0: the batch, the single device call and the host call
    st = db.struct()
    assert L.fp_dev_feasibility_batch(planner._ctx, ct.byref(st), None, count.out.data_ptr()) == FP_EINVAL
    cs = FpContainers(C, *(t.data_ptr() for t in (db.cpu, db.mem, db.req, db.conf)))
    ns = FpNodes(N, *(t.data_ptr() for t in (db.cf, db.mf, db.lab, db.cu, db.sched)))
    assert L.fp_dev_feasibility(planner._ctx, ct.byref(cs), ct.byref(ns), None, count.out.data_ptr(),
                                bm.out.data_ptr()) == FP_EINVAL
    planner.sync()
    assert count.untouched() and bm.untouched()
    works()
    # a null node column with N > 0
    st = db.struct()
    st.labels = None
    assert L.fp_dev_feasibility_batch(planner._ctx, ct.byref(st), first.out.data_ptr(), count.out.data_ptr()) == FP_EINVAL
    ns_bad = FpNodes(N, db.cf.data_ptr(), db.mf.data_ptr(), db.lab.data_ptr(), None, db.sched.data_ptr())
    assert L.fp_dev_feasibility(planner._ctx, ct.byref(cs), ct.byref(ns_bad), first.out.data_ptr(), count.out.data_ptr(),
                                bm.out.data_ptr()) == FP_EINVAL
    planner.sync()
    assert first.untouched() and count.untouched() and bm.untouched()
    # the host entry: the same two, on numpy outputs
    arrs = [np.ascontiguousarray(a) for a in (*cont, *nodes)]
    hcs = FpContainers(C, *(x.ctypes.data for x in arrs[:4]))
    hns = FpNodes(N, *(x.ctypes.data for x in arrs[4:]))
    hns_bad = FpNodes(N, arrs[4].ctypes.data, arrs[5].ctypes.data, arrs[6].ctypes.data, arrs[7].ctypes.data, None)
    hf, hc, hb = HostOut(C, np.uint32), HostOut(C, np.uint32), HostOut(WN, np.uint64)
    p32, p64 = (lambda o: ct.cast(o.ptr(), _lib.u32p)), (lambda o: ct.cast(o.ptr(), _lib.u64p))
    assert L.fp_feasibility(planner._ctx, ct.byref(hcs), ct.byref(hns), None, p32(hc), p64(hb)) == FP_EINVAL
    assert L.fp_feasibility(planner._ctx, ct.byref(hcs), ct.byref(hns_bad), p32(hf), p32(hc), p64(hb)) == FP_EINVAL
    assert hf.untouched() and hc.untouched() and hb.untouched()
    assert L.fp_feasibility(planner._ctx, ct.byref(hcs), ct.byref(hns), p32(hf), p32(hc), p64(hb)) == 0
    assert np.array_equal(hf.out, ef) and np.array_equal(hc.out, ec) and np.array_equal(hb.out, eb)
    works()


# ---- the neighbours -------------------------------------------------------------------------------------------
def test_agrees_with_explain(planner):
    """fp_explain's FEASIBLE word is this sweep's count, and it is 0 exactly where there is no first node."""
    C, N = 1100, 1089
    cont, nodes = K.case(C, N)
    ef, ec, _ = K.expected(C, N)
    first, count, _ = planner.feasibility(cont, nodes, bitmap=False)
    rows = planner.explain(cont, nodes)
    assert np.array_equal(first, ef) and np.array_equal(count, ec)
    assert np.array_equal(rows[:, ER.FEASIBLE], count)
    assert np.array_equal(rows[:, ER.FEASIBLE] == 0, first == NONE) and (first == NONE).sum() >= 50
