"""Host-side wrappers over the C ABI (include/fleetplace.h).

``Planner`` owns one ``fp_ctx`` (one HIP stream on one MI355X).  The numpy
methods use the synchronous host-pointer entry points (the drop-in boundary a
Rust/cgo caller would use); ``DevBatch`` + the ``dev_*`` methods run the same
kernels on device-resident tensors (torch is only the HBM allocator here).
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import FpBatch, FpContainers, FpGraph, FpNodes, check

NONE = _lib.FP_NONE


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ptr(a):
    """A numpy array's address for a pointer field of a struct (None = NULL); the caller keeps the array."""
    return None if a is None else a.ctypes.data


_POINTER = {1: _lib.u8p, 4: _lib.u32p, 8: _lib.u64p}


def _arg(a):
    """A pointer argument of an export: None (NULL), a device tensor's address, or a typed pointer into a
    numpy array (which it keeps alive)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data_as(_POINTER[a.itemsize])


# Every array is read (or written) for the length the call's sizes imply, so a shorter one would be
# read out of bounds by the library: refused with ValueError first, as lib.rs returns FP_EINVAL.
def _need(cond, what):
    if not cond:
        raise ValueError(what)


def _tables(cont, nodes, n_cont, n_node, copy_mutable, names=("C", "N")):
    """The container table (cpu_m, mem_mib, req_labels, conflict) and the node table (cpu_free, mem_free,
    labels, conflict_used, schedulable) as contiguous arrays of ``n_cont`` and ``n_node`` entries (None = as
    many as the first array holds); ``names`` is how the messages call the two sizes.  ``copy_mutable``
    copies the node fields a placement updates, so the caller's stay as they were."""
    cont = tuple(_u32(x) for x in cont)
    cf, mf, lab, cu = (_u32(x) for x in nodes[:4])
    if copy_mutable:
        cf, mf, cu = cf.copy(), mf.copy(), cu.copy()
    nodes = (cf, mf, lab, cu, _u8(nodes[4]))
    C = cont[0].size if n_cont is None else n_cont
    N = cf.size if n_node is None else n_node
    _need(all(x.size == C for x in cont), f"every container array must hold {names[0]} entries")
    _need(all(x.size == N for x in nodes), f"every node array must hold {names[1]} entries")
    return cont, nodes


def _pair(cont, nodes):
    return (FpContainers(cont[0].size, *(_ptr(x) for x in cont)), FpNodes(nodes[0].size, *(_ptr(x) for x in nodes)))


def _batch(S, scen_base, C, N, cont, level, nodes, assign, reason, cost):
    return FpBatch(S, scen_base, C, N, *(_ptr(x) for x in cont + (level,) + nodes + (assign, reason, cost)))


def _relax_row(relax_mask):
    """One scenario's relax masks as the FP_FALLBACK_MAX_HOPS words of the ABI (zero-padded)."""
    row = [int(m) & 0xFFFFFFFF for m in relax_mask]
    if len(row) > _lib.FP_FALLBACK_MAX_HOPS:
        raise ValueError(f"relax_mask holds at most {_lib.FP_FALLBACK_MAX_HOPS} hops")
    return row + [0] * (_lib.FP_FALLBACK_MAX_HOPS - len(row))


def _quota_rows(quota, S):
    """[S * 3] u32 caps from S rows of (cpu_m, mem_mib, services); None in a row = QUOTA_UNLIMITED."""
    rows = np.asarray([[_lib.QUOTA_UNLIMITED if x is None else int(x) for x in row]
                       for row in np.asarray(quota, dtype=object).reshape(-1, _lib.QUOTA_DIMS)], dtype=np.int64)
    if rows.shape[0] != S or rows.min(initial=0) < 0 or rows.max(initial=0) > 0xFFFFFFFF:
        raise ValueError(f"quota must hold {S} rows of {_lib.QUOTA_DIMS} u32 caps")
    return rows.astype(np.uint32).reshape(-1)


def _policy_call(dims, cont, nodes, strategy, preferred, level, node_count, domain=None, max_skew=None,
                 relax_mask=None, n_hops=None, quota=None, quota_used=None, want_hops=False, want_why=False,
                 want_used=False):
    """Everything a host scored-placement call sends, checked: ``dims`` is (S, C, N, scen_base) for the batch
    methods and None for the single-scenario ones (S = 1, sizes from the tables, strategy / preferred /
    max_skew / n_hops scalars, one relax row).  Returns a namespace: the converted inputs, the outputs
    (hops / why / qu None unless wanted) and, as the export's arguments, ``head`` = the tables up to
    node_count, ``spread`` = (domain, max_skew) and ``chain`` = (relax_mask, n_hops).  In a batch either one
    of a pair None means both None."""
    o = SimpleNamespace()
    batch = dims is not None
    S, C, N, scen_base = dims if batch else (1, None, None, 0)
    by = "S * " if batch else ""
    o.cont, o.nodes = _tables(cont, nodes, S * C if batch else None, S * N if batch else None, True,
                              (by + "C", by + "N"))
    if not batch:
        C, N = o.cont[0].size, o.nodes[0].size
    o.lv = _u32(level) if level is not None else None
    o.nc = _u32(node_count).copy() if node_count is not None else None
    _need(o.lv is None or o.lv.size == S * C, f"level must hold {by}C entries")
    o.dom = o.sk = o.rm = o.nh = None
    if batch:
        o.st = _u32([strategy_id(x) for x in strategy])
        o.pf = _u32(preferred) if preferred is not None else None
        _need(o.st.size == S and (o.pf is None or o.pf.size == S), "strategy and preferred must hold S entries")
        _need(o.nc is None or o.nc.size == S * N, "node_count must hold S * N entries")
        if domain is not None and max_skew is not None:
            o.dom, o.sk = _u32(domain), _u32(max_skew)
            _need(o.dom.size == S * N and o.sk.size == S, "domain must hold S * N and max_skew S entries")
        if relax_mask is not None and n_hops is not None:
            o.rm, o.nh = _u32(relax_mask).reshape(-1), _u32(n_hops)
            _need(o.rm.size == S * _lib.FP_FALLBACK_MAX_HOPS and o.nh.size == S,
                  "relax_mask must hold S * FP_FALLBACK_MAX_HOPS and n_hops S entries")
        o.spread, o.chain = (_arg(o.dom), _arg(o.sk)), (_arg(o.rm), _arg(o.nh))
    else:
        _need(o.nc is None or o.nc.size == N, "node_count must hold N entries")
        o.dom = _u32(domain) if domain is not None else None
        _need(o.dom is None or o.dom.size == N, "domain must hold N entries")
        o.sk = int(max_skew)
        _need(0 <= o.sk <= 0xFFFFFFFF, "max_skew must be a u32")
        if relax_mask is not None:
            o.rm = _u32(_relax_row(relax_mask))
            o.nh = len(relax_mask) if n_hops is None else int(n_hops)
            _need(0 <= o.nh <= 0xFFFFFFFF, "n_hops must be a u32")
        o.spread, o.chain = (_arg(o.dom), o.sk), (_arg(o.rm), o.nh)
    o.qt = _quota_rows(quota, S) if quota is not None else None
    o.qu = None
    if want_used:
        o.qu = (np.zeros(S * _lib.QUOTA_DIMS, np.uint32) if quota_used is None
                else _u32(quota_used).reshape(-1).copy())
        _need(o.qu.size == S * _lib.QUOTA_DIMS, f"quota_used must hold {by}3 entries")
    o.assign = np.empty(S * C, np.uint32)
    o.reason = np.empty(S * C, np.uint8)
    o.hops = np.empty(S * C, np.uint8) if want_hops else None
    o.why = np.zeros(S * C, np.uint8) if want_why else None
    if batch:
        o.cost = np.empty(S, np.uint64)
        o.b = _batch(S, scen_base, C, N, o.cont, o.lv, o.nodes, o.assign, o.reason, o.cost)
        o.head = (ct.byref(o.b), _arg(o.st), _arg(o.pf), _arg(o.nc))
    else:
        o.cs, o.ns = _pair(o.cont, o.nodes)
        o.head = (ct.byref(o.cs), ct.byref(o.ns), _arg(o.lv), strategy_id(strategy), int(preferred) & 0xFFFFFFFF,
                  _arg(o.nc))
    return o


def _dev_policy_checks(db, strategy_t, preferred_t, count_t, domain_t, max_skew_t, relax_mask_t=None, n_hops_t=None,
                       hops_t=None):
    """The tensor sizes of a dev_place_batch_policy* call; returns (domain_t, max_skew_t, relax_mask_t,
    n_hops_t) with either one of a pair None made both None."""
    _need(strategy_t.numel() == db.S, "strategy_t must hold S entries")
    _need(preferred_t is None or preferred_t.numel() == db.S, "preferred_t must hold S entries")
    _need(count_t is None or count_t.numel() == db.S * db.N, "count_t must hold S * N entries")
    if domain_t is None or max_skew_t is None:
        domain_t = max_skew_t = None
    else:
        _need(domain_t.numel() == db.S * db.N and max_skew_t.numel() == db.S,
              "domain_t must hold S * N and max_skew_t S entries")
    if relax_mask_t is None or n_hops_t is None:
        relax_mask_t = n_hops_t = None
    else:
        _need(relax_mask_t.numel() == db.S * _lib.FP_FALLBACK_MAX_HOPS and n_hops_t.numel() == db.S,
              "relax_mask_t must hold S * FP_FALLBACK_MAX_HOPS and n_hops_t S entries")
    _need(hops_t is None or (hops_t.numel() == db.S * db.C and hops_t.element_size() == 1),
          "hops_t must hold S * C bytes")
    return domain_t, max_skew_t, relax_mask_t, n_hops_t


def _containers(cont):
    """The container table alone (the scale-out sweep has no node table of its own), as ``_tables`` checks it."""
    cont = tuple(_u32(x) for x in cont)
    _need(len(cont) == 4 and all(x.size == cont[0].size for x in cont), "every container array must hold C entries")
    return cont


def _opt_n(a, n, what, size="N"):
    """An optional u32 array of ``n`` entries (node_count, domain, t_max, ..): None stays None."""
    if a is None:
        return None
    a = _u32(a).reshape(-1)
    _need(a.size == n, f"{what} must hold {size} entries")
    return a


def _relax(relax_mask):
    """A sweep's fallback chain: the masks as a list and as the u32 array the export reads (None when empty)."""
    relax = [int(m) & 0xFFFFFFFF for m in relax_mask]
    _need(len(relax) <= _lib.FP_FALLBACK_MAX_HOPS, f"relax_mask holds at most {_lib.FP_FALLBACK_MAX_HOPS} hops")
    return relax, _u32(relax) if relax else None


def _skew_chain(max_skew, relax_mask):
    """The scalar guarantees of a sweep under the policy, checked: (max_skew, relax_mask array or None, n_hops)."""
    max_skew = int(max_skew)
    _need(0 <= max_skew <= 0xFFFFFFFF, "max_skew must be a u32")
    relax, rm = _relax(relax_mask)
    return max_skew, rm, len(relax)


def _tensor(name, t, n, holds, size=4, optional=False):
    """A device tensor of ``n`` entries of ``size`` bytes (``optional``: or None); ``holds`` is how the message
    writes ``n``."""
    _need((optional and t is None) or (t.numel() == n and t.element_size() == size),
          f"{name} must hold {holds} " + ("32-bit entries" if size == 4 else "bytes"))


def _dev_tables_checks(cont_t, nodes_t=None):
    """The container and node tensors of a dev_*_sweep call, checked: (C, N, FpContainers, FpNodes); without
    ``nodes_t`` N and the node struct are None."""
    C = cont_t[0].numel()
    N = nodes_t[0].numel() if nodes_t is not None else None
    _need(len(cont_t) == 4 and all(t.numel() == C and t.element_size() == 4 for t in cont_t),
          "every container tensor must hold C 32-bit entries")
    cs = FpContainers(C, *(t.data_ptr() for t in cont_t))
    if nodes_t is None:
        return C, None, cs, None
    _need(len(nodes_t) == 5 and all(t.numel() == N and t.element_size() == 4 for t in nodes_t[:4])
          and nodes_t[4].numel() == N and nodes_t[4].element_size() == 1,
          "every node tensor must hold N entries (schedulable N bytes)")
    return C, N, cs, FpNodes(N, *(t.data_ptr() for t in nodes_t))


def strategy_id(strategy) -> int:
    """An fp_strategy value from an int or one of the control plane's policy strings
    (``spread_across_pool``, ``pack_into_dedicated``, ``fill_lowest``).  An int is passed on as it is
    (the library refuses values that are no fp_strategy); an unknown string is a ValueError."""
    if isinstance(strategy, str):
        if strategy not in _lib.POLICY_STRATEGIES:
            raise ValueError(f"unknown placement strategy '{strategy}' (expected "
                             + "|".join(_lib.POLICY_STRATEGIES) + ")")
        return _lib.POLICY_STRATEGIES[strategy]
    return int(strategy)


class Planner:
    def __init__(self, device: int = 0):
        self._L = _lib.load()
        h = ct.c_void_p()
        check(self._L.fp_ctx_create(ct.byref(h), device), "fp_ctx_create")
        self._ctx = h
        self.device = device
        self._tstream = None  # torch view of the stream the dev_* calls launch on (see _dev)

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            if getattr(self, "_tstream", None) is not None:
                self._L.fp_ctx_reset_stream(self._ctx)  # off the torch stream before it can go away
                self._tstream = None
            self._L.fp_ctx_destroy(self._ctx)
            self._ctx = None
            self._fs = None  # plan_stage_lists' prebuilt call holds the handle

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream_handle: int):
        """Launch on this hipStream_t handle; 0 is the HIP null (default) stream."""
        check(self._L.fp_ctx_set_stream(self._ctx, ct.c_void_p(int(hip_stream_handle))), "fp_ctx_set_stream")
        import torch
        self._tstream = torch.cuda.ExternalStream(int(hip_stream_handle), device=torch.device("cuda", self.device))

    def reset_stream(self):
        check(self._L.fp_ctx_reset_stream(self._ctx), "fp_ctx_reset_stream")
        self._tstream = None

    def _dev(self, fn, *args):
        """Run one fp_dev_* call ordered with torch's current stream on both sides: the call
        waits for work queued there before it (a restore_nodes copy, a tensor fill) and later
        work there waits for the call (a snapshot, a comparison).  Stream-ordered, no host
        sync.  The context launches on a torch-created stream unless set_stream chose one."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if self._tstream is None:
            st = torch.cuda.Stream(device=torch.device("cuda", self.device))
            check(self._L.fp_ctx_set_stream(self._ctx, ct.c_void_p(st.cuda_stream)), "fp_ctx_set_stream")
            self._tstream = st
        if self._tstream.cuda_stream == cur.cuda_stream:
            return fn(*args)
        self._tstream.wait_stream(cur)
        try:
            return fn(*args)
        finally:
            cur.wait_stream(self._tstream)

    def sync(self):
        check(self._L.fp_ctx_sync(self._ctx), "fp_ctx_sync")

    def profile(self, enable=True):
        check(self._L.fp_ctx_profile(self._ctx, int(enable)), "fp_ctx_profile")

    def set_option(self, name: str, value: int = _lib.FP_OPT_AUTO):
        """fp_ctx_set_option by name (_lib.OPTIONS); FP_OPT_AUTO (-1) restores the default."""
        check(self._L.fp_ctx_set_option(self._ctx, _lib.OPTIONS[name], int(value)), f"fp_ctx_set_option({name})")

    def get_option(self, name: str) -> int:
        v = ct.c_int64()
        check(self._L.fp_ctx_get_option(self._ctx, _lib.OPTIONS[name], ct.byref(v)), f"fp_ctx_get_option({name})")
        return int(v.value)

    def reset_options(self):
        for name in _lib.OPTIONS:
            self.set_option(name, _lib.FP_OPT_AUTO)

    def geometry(self, S: int, C: int, N: int) -> dict:
        """The placement pipeline a batch of S x C x N runs on this context (fp_place_geometry)."""
        out = (ct.c_uint32 * len(_lib.GEOM_FIELDS))()
        check(self._L.fp_place_geometry(self._ctx, S, C, N, out), "fp_place_geometry")
        return dict(zip(_lib.GEOM_FIELDS, (int(x) for x in out)))

    def place_path(self) -> dict:
        """The FFD kernel the last placement ran (fp_ctx_place_path; waits for the stream):
        {"or_cpu", "or_mem", "packed"} -- packed is True for the packed (cpu, mem) records; prepacked when
        they were fed by prepacked demand rows (FP_OPT_PREPACK); repaired when the u32 kernel ran on rows the
        repair pass unpacked."""
        out = (ct.c_uint32 * 3)()
        check(self._L.fp_ctx_place_path(self._ctx, out), "fp_ctx_place_path")
        k = int(out[2])
        return {"or_cpu": int(out[0]), "or_mem": int(out[1]), "packed": k in (2, 3), "ran": k != 0,
                "prepacked": k == 3, "repaired": k == 4}

    def kernel_stats(self, kernel_id: int):
        ms = ct.c_double()
        n = ct.c_uint64()
        check(self._L.fp_ctx_kernel_stats(self._ctx, kernel_id, ct.byref(ms), ct.byref(n)), "kernel_stats")
        return ms.value, n.value

    # -- host-pointer API ------------------------------------------------------------
    _need = staticmethod(_need)
    _relax_row = staticmethod(_relax_row)
    _quota_rows = staticmethod(_quota_rows)

    def legacy_order(self, has_deps):
        """engine.rs:67-85 on indices: has_deps[i] = known && depends_on non-empty."""
        hd = _u8(has_deps)
        out = np.empty(hd.size, np.uint32)
        g = FpGraph(hd.size, 0, None, None, _ptr(hd))
        check(self._L.fp_legacy_order(self._ctx, ct.byref(g), out.ctypes.data_as(_lib.u32p)), "fp_legacy_order")
        return out

    def levelize(self, row_ptr, col, has_deps):
        rp, cl, hd = _u32(row_ptr), _u32(col), _u8(has_deps)
        V = hd.size
        self._need(V == 0 or rp.size == V + 1, "row_ptr must hold V + 1 entries")
        level = np.empty(V, np.uint32)
        order = np.empty(V, np.uint32)
        ncyc = ct.c_uint32()
        g = FpGraph(V, cl.size, _ptr(rp), _ptr(cl) if cl.size else None, _ptr(hd))
        check(self._L.fp_levelize(self._ctx, ct.byref(g), level.ctypes.data_as(_lib.u32p),
                                  order.ctypes.data_as(_lib.u32p), ct.byref(ncyc)), "fp_levelize")
        return level, order, ncyc.value

    def plan_stage_lists(self, row_ptr, col, has_deps):
        """fp_plan_stage without servers for a graph given as Python sequences (a fleet.kdl stage;
        BASELINE config 1 is timed per plan, where numpy conversions and ctypes argument conversion
        cost more than the GPU work): the inputs go into ctypes buffers kept between calls, the call
        is one prebuilt foreign call, and the results come back as lists.  Returns (perm, level,
        order, n_cycle).  Same checks and errors as plan_stage."""
        V, E = len(has_deps), len(col)
        self._need(V == 0 or len(row_ptr) == V + 1, "row_ptr must hold V + 1 entries")
        fs = getattr(self, "_fs", None)
        if fs is None or V > fs["V"] or E > fs["E"] or fs["args"][0] is not self._ctx:
            cv, ce = max(64, V), max(256, E)
            rp, cl, hd = (ct.c_uint32 * (cv + 1))(), (ct.c_uint32 * ce)(), (ct.c_uint8 * cv)()
            out, ncyc = (ct.c_uint32 * (3 * cv))(), ct.c_uint32()
            g = FpGraph(0, 0, ct.addressof(rp), ct.addressof(cl), ct.addressof(hd))
            a = ct.addressof(out)
            args = (self._ctx, ct.byref(g), None, None, ct.c_void_p(a), ct.c_void_p(a + 4 * cv),
                    ct.c_void_p(a + 8 * cv), ct.byref(ncyc), None, None, None, None)
            fs = self._fs = {"V": cv, "E": ce, "rp": rp, "col": cl, "hd": hd, "out": out, "ncyc": ncyc, "g": g,
                             "args": args, "fn": _lib.raw_function("fp_plan_stage")}
        if V == 0:
            return [], [], [], 0
        fs["rp"][:V + 1] = row_ptr
        if E:
            fs["col"][:E] = col
        fs["hd"][:V] = has_deps
        g = fs["g"]
        g.n_vertices = V
        g.n_edges = E
        check(fs["fn"](*fs["args"]), "fp_plan_stage")
        out, cv = fs["out"], fs["V"]
        return out[:V], out[cv:cv + V], out[2 * cv:2 * cv + V], fs["ncyc"].value

    def plan_stage(self, row_ptr, col, has_deps, cont=None, nodes=None):
        """fp_plan_stage: one stage's A1 legacy order, A2 levels and start order and, with ``nodes``
        (container v = vertex v), the stage-2 candidates on the pristine table and the FFD plan gated
        by the levels' CYCLE -- one call (one kernel for a fleet.kdl-sized stage).  Returns
        (perm, level, order, n_cycle, placed) with placed = None or (first, count, assign, reason,
        nodes_after)."""
        rp, cl, hd = _u32(row_ptr), _u32(col), _u8(has_deps)
        V = hd.size
        self._need(V == 0 or rp.size == V + 1, "row_ptr must hold V + 1 entries")
        out = np.empty(3 * V, np.uint32)  # perm, level, order: one allocation, passed as addresses
        perm, level, order = out[:V], out[V:2 * V], out[2 * V:]
        o = out.ctypes.data
        ncyc = ct.c_uint32()
        g = FpGraph(V, cl.size, rp.ctypes.data, cl.ctypes.data if cl.size else None, hd.ctypes.data)
        if nodes is None:
            check(self._L.fp_plan_stage(self._ctx, ct.byref(g), None, None, o, o + 4 * V, o + 8 * V, ct.byref(ncyc),
                                        None, None, None, None), "fp_plan_stage")
            return perm, level, order, ncyc.value, None
        cont, nodes = _tables(cont, nodes, V, None, True, ("V", "N"))
        first = np.empty(V, np.uint32)
        count = np.empty(V, np.uint32)
        assign = np.empty(V, np.uint32)
        reason = np.empty(V, np.uint8)
        cs, ns = _pair(cont, nodes)
        check(self._L.fp_plan_stage(self._ctx, ct.byref(g), ct.byref(cs), ct.byref(ns), o, o + 4 * V, o + 8 * V,
                                    ct.byref(ncyc), first.ctypes.data, count.ctypes.data, assign.ctypes.data,
                                    reason.ctypes.data), "fp_plan_stage")
        return perm, level, order, ncyc.value, (first, count, assign, reason, nodes)

    def place(self, cont, nodes, level=None):
        """cont = (cpu_m, mem_mib, req_labels, conflict); nodes = (cpu_free, mem_free,
        labels, conflict_used, schedulable).  Inputs are not mutated; the updated node
        state is returned.  Returns (assign, reason, nodes_after)."""
        cont, nodes = _tables(cont, nodes, None, None, True)
        C = cont[0].size
        lv = _u32(level) if level is not None else None
        self._need(lv is None or lv.size == C, "level must hold C entries")
        assign = np.empty(C, np.uint32)
        reason = np.empty(C, np.uint8)
        cs, ns = _pair(cont, nodes)
        check(self._L.fp_place(self._ctx, ct.byref(cs), ct.byref(ns), _arg(lv), _arg(assign), _arg(reason)), "fp_place")
        return assign, reason, nodes

    def place_batch(self, S, C, N, cont, nodes, level=None, scen_base=0):
        """Scenario-major arrays ([S*C] containers, [S*N] nodes).  Returns
        (assign, reason, cost, nodes_after)."""
        cont, nodes = _tables(cont, nodes, S * C, S * N, True, ("S * C", "S * N"))
        lv = _u32(level) if level is not None else None
        self._need(lv is None or lv.size == S * C, "level must hold S * C entries")
        assign = np.empty(S * C, np.uint32)
        reason = np.empty(S * C, np.uint8)
        cost = np.empty(S, np.uint64)
        b = _batch(S, scen_base, C, N, cont, lv, nodes, assign, reason, cost)
        check(self._L.fp_place_batch(self._ctx, ct.byref(b)), "fp_place_batch")
        return assign, reason, cost, nodes

    def place_policy(self, cont, nodes, strategy, preferred=0, level=None, node_count=None, *, domain=None,
                     max_skew=0):
        """Scored placement (SPEC.md 2.6, fp_place_policy): ``strategy`` is an fp_strategy value or one
        of the control plane's policy strings, ``preferred`` the soft preferred-label mask,
        ``node_count`` the containers already on each node (None = zero).  ``domain`` ([N] topology
        domain ids below FP_SPREAD_MAX_DOMAINS) with ``max_skew`` >= 1 is the hard topology spread of
        SPEC.md 2.7 (fp_place_policy_spread): a container some node fits but none within the skew comes
        back with reason REASON_SKEW.  No domain, or max_skew = 0, is no constraint.  Inputs are not
        mutated.  Returns (assign, reason, nodes_after, node_count_after); the last is None without
        node_count."""
        o = _policy_call(None, cont, nodes, strategy, preferred, level, node_count, domain, max_skew)
        if o.dom is not None:
            check(self._L.fp_place_policy_spread(self._ctx, *o.head, *o.spread, _arg(o.assign), _arg(o.reason)),
                  "fp_place_policy_spread")
        else:
            check(self._L.fp_place_policy(self._ctx, *o.head, _arg(o.assign), _arg(o.reason)), "fp_place_policy")
        return o.assign, o.reason, o.nodes, o.nc

    def place_batch_policy(self, S, C, N, cont, nodes, strategy, preferred=None, level=None, node_count=None,
                           scen_base=0, *, domain=None, max_skew=None):
        """place_batch under per-scenario strategies ([S] ints or policy strings), preferred-label masks
        ([S] or None) and node counts ([S*N] or None).  ``domain`` ([S*N]) with ``max_skew`` ([S], 0 = no
        constraint in that scenario) is the topology spread of SPEC.md 2.7; either one None is no
        constraint anywhere.  Returns (assign, reason, cost, nodes_after, node_count_after)."""
        o = _policy_call((S, C, N, scen_base), cont, nodes, strategy, preferred, level, node_count, domain,
                         max_skew)
        if o.dom is not None:
            check(self._L.fp_place_batch_policy_spread(self._ctx, *o.head, *o.spread), "fp_place_batch_policy_spread")
        else:
            check(self._L.fp_place_batch_policy(self._ctx, *o.head), "fp_place_batch_policy")
        return o.assign, o.reason, o.cost, o.nodes, o.nc

    def place_policy_fallback(self, cont, nodes, strategy, relax_mask, preferred=0, level=None, node_count=None, *,
                              domain=None, max_skew=0, n_hops=None, want_hops=True):
        """place_policy under a fallback chain (SPEC.md 2.8, fp_place_policy_fallback): ``relax_mask`` holds,
        per hop, the required-label bits that hop gives up (at most FP_FALLBACK_MAX_HOPS masks), ``n_hops``
        the number of hops (None = every mask given; the library refuses more than FP_FALLBACK_MAX_HOPS).  A
        container goes to the feasible node of the smallest (hop, key); it gives a requirement up only when
        no node of an earlier hop is feasible.  ``domain`` / ``max_skew`` as in place_policy.  Returns
        (assign, reason, hops, nodes_after, node_count_after): hops[c] is the winner's hop (0 when rejected),
        or None with ``want_hops`` False."""
        o = _policy_call(None, cont, nodes, strategy, preferred, level, node_count, domain, max_skew,
                         relax_mask, n_hops, want_hops=want_hops)
        check(self._L.fp_place_policy_fallback(self._ctx, *o.head, *o.spread, *o.chain, _arg(o.assign), _arg(o.reason),
                                               _arg(o.hops)), "fp_place_policy_fallback")
        return o.assign, o.reason, o.hops, o.nodes, o.nc

    def place_batch_policy_fallback(self, S, C, N, cont, nodes, strategy, preferred=None, level=None, node_count=None,
                                    scen_base=0, *, domain=None, max_skew=None, relax_mask=None, n_hops=None,
                                    want_hops=True):
        """place_batch_policy under per-scenario fallback chains (SPEC.md 2.8): ``relax_mask``
        ([S * FP_FALLBACK_MAX_HOPS], scenario-major) with ``n_hops`` ([S], 0 = no fallback in that scenario);
        either one None is no fallback anywhere.  Returns (assign, reason, hops, cost, nodes_after,
        node_count_after); hops is [S*C] u8, or None with ``want_hops`` False."""
        o = _policy_call((S, C, N, scen_base), cont, nodes, strategy, preferred, level, node_count, domain,
                         max_skew, relax_mask, n_hops, want_hops=want_hops)
        check(self._L.fp_place_batch_policy_fallback(self._ctx, *o.head, *o.spread, *o.chain, _arg(o.hops)),
              "fp_place_batch_policy_fallback")
        return o.assign, o.reason, o.hops, o.cost, o.nodes, o.nc

    def place_policy_quota(self, cont, nodes, strategy, quota, quota_used=None, relax_mask=(), preferred=0, level=None,
                           node_count=None, *, domain=None, max_skew=0, n_hops=None, want_hops=True, want_why=True,
                           want_used=True):
        """place_policy_fallback under a resource quota (SPEC.md 2.10, fp_place_policy_quota): ``quota`` =
        (cpu millicores, memory MiB, services), None or QUOTA_UNLIMITED in a dimension = no cap there;
        ``quota_used`` what the tenant holds already (None = zeros).  A container the quota refuses comes back
        with reason REASON_QUOTA and the mask of the blocking dimensions in quota_why; it is tried on no node.
        ``quota`` None is no quota: the fallback entry's result, quota_why all zero, usage as given.  Returns
        (assign, reason, hops, nodes_after, node_count_after, quota_why, quota_used_after); quota_why is None
        with ``want_why`` False, and with ``want_used`` False the library gets no quota_used (usage starts at
        zero whatever was passed) and None comes back."""
        o = _policy_call(None, cont, nodes, strategy, preferred, level, node_count, domain, max_skew,
                         relax_mask, n_hops, quota, quota_used, want_hops, want_why, want_used)
        check(self._L.fp_place_policy_quota(self._ctx, *o.head, *o.spread, *o.chain, _arg(o.assign), _arg(o.reason),
                                            _arg(o.hops), _arg(o.qt), _arg(o.qu), _arg(o.why)), "fp_place_policy_quota")
        return o.assign, o.reason, o.hops, o.nodes, o.nc, o.why, o.qu

    def place_batch_policy_quota(self, S, C, N, cont, nodes, strategy, quota, quota_used=None, preferred=None,
                                 level=None, node_count=None, scen_base=0, *, domain=None, max_skew=None,
                                 relax_mask=None, n_hops=None, want_hops=True, want_why=True, want_used=True):
        """place_batch_policy_fallback under per-scenario quotas (SPEC.md 2.10): ``quota`` [S * 3] (rows of
        cpu, memory, services; QUOTA_UNLIMITED = no cap), ``quota_used`` [S * 3] or None = zeros; ``quota``
        None is no quota anywhere.  Returns (assign, reason, hops, cost, nodes_after, node_count_after,
        quota_why [S*C], quota_used_after [S*3]); the ``want_*`` switches as in place_policy_quota."""
        o = _policy_call((S, C, N, scen_base), cont, nodes, strategy, preferred, level, node_count, domain,
                         max_skew, relax_mask, n_hops, quota, quota_used, want_hops, want_why, want_used)
        check(self._L.fp_place_batch_policy_quota(self._ctx, *o.head, *o.spread, *o.chain, _arg(o.hops), _arg(o.qt),
                                                  _arg(o.qu), _arg(o.why)), "fp_place_batch_policy_quota")
        return o.assign, o.reason, o.hops, o.cost, o.nodes, o.nc, o.why, o.qu

    def replan(self, cont, nodes, prev, strategy=0, preferred=0, level=None, node_count=None, *, want_change=True,
               want_summary=True):
        """Re-plan a running stage (SPEC.md 2.13, fp_replan): ``nodes`` is the base table (everything deducted
        except these containers' own requests), ``prev`` [C] the node each container runs on now (NONE = none).
        A container keeps its node while it still fits there (a cordoned node keeps what runs on it); the
        others are placed as place_policy places them, on the state the seats left.  ``prev`` all NONE is
        place_policy.  Inputs are not mutated.  Returns (assign, reason, change, summary, nodes_after,
        node_count_after): change [C] u8 holds _lib.CHANGE_* values and summary [8] the _lib.REPLAN_* words
        (None with ``want_change`` / ``want_summary`` False); node_count_after is None without node_count."""
        o = _policy_call(None, cont, nodes, strategy, preferred, level, node_count, max_skew=0)
        C = o.cont[0].size
        pv = _u32(prev).reshape(-1)
        self._need(pv.size == C, "prev must hold C entries")
        change = np.empty(C, np.uint8) if want_change else None
        summary = np.empty(_lib.REPLAN_WORDS, np.uint32) if want_summary else None
        check(self._L.fp_replan(self._ctx, *o.head[:3], _arg(pv), *o.head[3:], _arg(o.assign), _arg(o.reason),
                                _arg(change), _arg(summary)), "fp_replan")
        return o.assign, o.reason, change, summary, o.nodes, o.nc

    def replan_batch(self, S, C, N, cont, nodes, prev, strategy, preferred=None, level=None, node_count=None,
                     scen_base=0, *, want_change=True, want_summary=True):
        """replan over scenario-major arrays (fp_replan_batch): ``prev`` [S*C], ``strategy`` [S] ints or policy
        strings, ``preferred`` [S] or None, ``node_count`` [S*N] or None.  Returns (assign, reason, cost, change
        [S*C], summary [S, 8], nodes_after, node_count_after); change and summary are None when not wanted."""
        o = _policy_call((S, C, N, scen_base), cont, nodes, strategy, preferred, level, node_count)
        pv = _u32(prev).reshape(-1)
        self._need(pv.size == S * C, "prev must hold S * C entries")
        change = np.empty(S * C, np.uint8) if want_change else None
        summary = np.empty((S, _lib.REPLAN_WORDS), np.uint32) if want_summary else None
        check(self._L.fp_replan_batch(self._ctx, o.head[0], _arg(pv), *o.head[1:], _arg(change), _arg(summary)),
              "fp_replan_batch")
        return o.assign, o.reason, o.cost, change, summary, o.nodes, o.nc

    def replan_policy(self, cont, nodes, prev, strategy=0, quota=None, quota_used=None, relax_mask=None, preferred=0,
                      level=None, node_count=None, *, domain=None, max_skew=0, n_hops=None, want_hops=True,
                      want_why=True, want_used=True, want_change=True, want_summary=True):
        """replan under the policy's guarantees (SPEC.md 2.14, fp_replan_policy): ``domain`` / ``max_skew``,
        ``relax_mask`` / ``n_hops`` and ``quota`` / ``quota_used`` as in place_policy_quota, each one optional.
        A container keeps its node while it fits there under the labels the whole chain still asks for; seats
        are neither tested against the skew bound or the quota nor evicted, but they count in their domains and
        are charged.  The others are placed as place_policy_quota places them, on the counts and the usage the
        seats left.  Without a guarantee it is replan; ``prev`` all NONE is place_policy_quota.  Returns (assign,
        reason, hops, change, summary, nodes_after, node_count_after, quota_why, quota_used_after); the
        ``want_*`` switches as in place_policy_quota and replan."""
        o = _policy_call(None, cont, nodes, strategy, preferred, level, node_count, domain, max_skew,
                         relax_mask, n_hops, quota, quota_used, want_hops, want_why, want_used)
        C = o.cont[0].size
        pv = _u32(prev).reshape(-1)
        self._need(pv.size == C, "prev must hold C entries")
        change = np.empty(C, np.uint8) if want_change else None
        summary = np.empty(_lib.REPLAN_WORDS, np.uint32) if want_summary else None
        chain = o.chain if o.rm is not None else (None, 0)
        check(self._L.fp_replan_policy(self._ctx, *o.head[:3], _arg(pv), *o.head[3:], *o.spread, *chain, _arg(o.assign),
                                       _arg(o.reason), _arg(o.hops), _arg(o.qt), _arg(o.qu), _arg(o.why), _arg(change),
                                       _arg(summary)), "fp_replan_policy")
        return o.assign, o.reason, o.hops, change, summary, o.nodes, o.nc, o.why, o.qu

    def replan_batch_policy(self, S, C, N, cont, nodes, prev, strategy, quota=None, quota_used=None, preferred=None,
                            level=None, node_count=None, scen_base=0, *, domain=None, max_skew=None, relax_mask=None,
                            n_hops=None, want_hops=True, want_why=True, want_used=True, want_change=True,
                            want_summary=True):
        """replan_policy over scenario-major arrays (fp_replan_batch_policy): the arrays of replan_batch and of
        place_batch_policy_quota.  Returns (assign, reason, hops, cost, change [S*C], summary [S, 8], nodes_after,
        node_count_after, quota_why [S*C], quota_used_after [S*3])."""
        o = _policy_call((S, C, N, scen_base), cont, nodes, strategy, preferred, level, node_count, domain,
                         max_skew, relax_mask, n_hops, quota, quota_used, want_hops, want_why, want_used)
        pv = _u32(prev).reshape(-1)
        self._need(pv.size == S * C, "prev must hold S * C entries")
        change = np.empty(S * C, np.uint8) if want_change else None
        summary = np.empty((S, _lib.REPLAN_WORDS), np.uint32) if want_summary else None
        check(self._L.fp_replan_batch_policy(self._ctx, o.head[0], _arg(pv), *o.head[1:], *o.spread, *o.chain,
                                             _arg(o.hops), _arg(o.qt), _arg(o.qu), _arg(o.why), _arg(change),
                                             _arg(summary)), "fp_replan_batch_policy")
        return o.assign, o.reason, o.hops, o.cost, change, summary, o.nodes, o.nc, o.why, o.qu

    def feasibility(self, cont, nodes, bitmap=True):
        cont, nodes = _tables(cont, nodes, None, None, False)
        C, N = cont[0].size, nodes[0].size
        first = np.empty(C, np.uint32)
        count = np.empty(C, np.uint32)
        bm = np.empty(((C + 63) // 64) * N, np.uint64) if bitmap else None
        cs, ns = _pair(cont, nodes)
        check(self._L.fp_feasibility(self._ctx, ct.byref(cs), ct.byref(ns), _arg(first), _arg(count), _arg(bm)),
              "fp_feasibility")
        return first, count, bm

    def explain(self, cont, nodes, sel=None, ignore_labels=0):
        """Rejection diagnosis (SPEC.md 2.9, fp_explain): one row of EXPLAIN_WORDS u32 per explained
        container on the given node table -- ``sel`` container indices (repeats allowed) or None = every
        container in order; ``ignore_labels`` the required-label bits given up.  Nothing is placed.
        Returns an ndarray [M, 16] (word indices: _lib.EXPLAIN_*)."""
        cont, nodes = _tables(cont, nodes, None, None, False)
        sl = _u32(sel).reshape(-1) if sel is not None else None
        M = cont[0].size if sl is None else sl.size
        rows = np.empty((M, _lib.EXPLAIN_WORDS), np.uint32)
        if M == 0:  # an empty sel must not reach the library as NULL (= every container)
            return rows
        cs, ns = _pair(cont, nodes)
        check(self._L.fp_explain(self._ctx, ct.byref(cs), ct.byref(ns), _arg(sl), M, int(ignore_labels) & 0xFFFFFFFF,
                                 _arg(rows)), "fp_explain")
        return rows

    def explain_batch(self, S, C, N, cont, nodes, reason, reason_mask, ignore_labels=None):
        """Per-scenario cause histograms (SPEC.md 2.9, fp_explain_batch) over scenario-major arrays:
        ``reason_mask`` bit r selects the containers with reason r (0 = every container, ``reason`` may be
        None), ``ignore_labels`` [S] or None.  Returns an ndarray [S, 8] (word indices 0..4 = the causes,
        _lib.EXPLAIN_HIST_*)."""
        cont, nodes = _tables(cont, nodes, S * C, S * N, False, ("S * C", "S * N"))
        rs = _u8(reason) if reason is not None else None
        ig = _u32(ignore_labels) if ignore_labels is not None else None
        self._need(int(reason_mask) == 0 or (rs is not None and rs.size == S * C), "reason must hold S * C entries")
        self._need(ig is None or ig.size == S, "ignore_labels must hold S entries")
        hist = np.empty((S, _lib.EXPLAIN_HIST_WORDS), np.uint32)
        b = _batch(S, 0, C, N, cont, None, nodes, None, rs, None)
        check(self._L.fp_explain_batch(self._ctx, ct.byref(b), int(reason_mask) & 0xFFFFFFFF, _arg(ig), _arg(hist)),
              "fp_explain_batch")
        return hist

    # The sweeps: a plain method and its policy twin share one body.  ``policy`` is what the twin's signature adds
    # (None for the plain method); the plain call differs only in the export and in the absence of the policy
    # suffix of arguments and results.
    def _call(self, export, *args, dev=False):
        fn = lambda: check(getattr(self._L, export)(self._ctx, *args), export)  # noqa: E731
        return self._dev(fn) if dev else fn()

    def _drain_host(self, cont, nodes, assign, group, n_cand, strategy, preferred, node_count, policy=None):
        cont, nodes = _tables(cont, nodes, None, None, False)
        C, N = cont[0].size, nodes[0].size
        asg, grp = _u32(assign), _u32(group)
        n_cand, strategy = int(n_cand), strategy_id(strategy)
        _need(asg.size == C, "assign must hold C entries")
        _need(grp.size == N, "group must hold N entries")
        nc = _opt_n(node_count, N, "node_count")
        dom = _opt_n(policy[0], N, "domain") if policy else None
        _need(0 <= n_cand <= 0xFFFFFFFF, "n_cand must be a u32")
        out, reason = np.empty(C, np.uint32), np.empty(C, np.uint8)
        summary = np.empty((n_cand, _lib.DRAIN_WORDS), np.uint32)
        cs, ns = _pair(cont, nodes)
        head = (ct.byref(cs), ct.byref(ns), _arg(asg), _arg(grp), n_cand, strategy, int(preferred) & 0xFFFFFFFF, _arg(nc))
        if policy is None:
            self._call("fp_drain_sweep", *head, _arg(out), _arg(reason), _arg(summary))
            return out, reason, summary
        max_skew, rm, n_hops = _skew_chain(*policy[1:])
        hops, rows = np.empty(C, np.uint8), np.empty((n_cand, _lib.DRAIN_POLICY_WORDS), np.uint32)
        self._call("fp_drain_sweep_policy", *head, _arg(dom), max_skew, _arg(rm), n_hops, _arg(out), _arg(reason),
                   _arg(hops), _arg(summary), _arg(rows))
        return out, reason, summary, hops, rows

    def _shrink_host(self, cont, nodes, assign, try_order, strategy, preferred, node_count, policy=None):
        cont, nodes = _tables(cont, nodes, None, None, False)
        C, N = cont[0].size, nodes[0].size
        asg, tro = _u32(assign), _u32(try_order)
        _need(tro.ndim == 2, "try_order must be [n_var, n_try]")
        n_var, n_try = tro.shape
        strategy = strategy_id(strategy)
        _need(asg.size == C, "assign must hold C entries")
        nc = _opt_n(node_count, N, "node_count")
        out, state = np.empty((n_var, C), np.uint32), np.empty((n_var, N), np.uint8)
        blocker, summary = np.empty((n_var, N), np.uint32), np.empty((n_var, _lib.SHRINK_WORDS), np.uint32)
        cs, ns = _pair(cont, nodes)
        head = (ct.byref(cs), ct.byref(ns), _arg(asg), _arg(tro), n_var, n_try, strategy, int(preferred) & 0xFFFFFFFF,
                _arg(nc))
        outs = (_arg(out), _arg(state), _arg(blocker), _arg(summary))
        if policy is None:
            self._call("fp_shrink_sweep", *head, *outs)
            return out, state, blocker, summary
        dom = _opt_n(policy[0], N, "domain")
        max_skew, rm, n_hops = _skew_chain(*policy[1:])
        hops, why = np.empty((n_var, C), np.uint8), np.empty((n_var, N), np.uint8)
        rows = np.empty((n_var, _lib.SHRINK_POLICY_WORDS), np.uint32)
        self._call("fp_shrink_sweep_policy", *head, _arg(dom), max_skew, _arg(rm), n_hops, *outs, _arg(hops), _arg(why),
                   _arg(rows))
        return out, state, blocker, summary, hops, why, rows

    def _grow_host(self, cont, reason, templates, max_new, reason_mask, t_max, want_assign, policy=None):
        cont = _containers(cont)
        C = cont[0].size
        if policy is not None:
            nodes, strategy, preferred, node_count, domain, t_domain, max_skew, relax_mask, quota, quota_used = policy
            cont, live = _tables(cont, nodes, None, None, False)
            N = live[0].size
        tpl = tuple(_u32(x).reshape(-1) for x in templates)
        _need(len(tpl) == 3, "templates must be (t_cpu, t_mem, t_labels)")
        n_cand = tpl[0].size
        _need(all(x.size == n_cand for x in tpl), "every template array must hold n_cand entries")
        rs = _u8(reason) if reason is not None else None
        reason_mask, max_new = int(reason_mask), int(max_new)
        _need(0 <= reason_mask <= 0xFFFFFFFF, "reason_mask must be a u32")
        _need(reason_mask == 0 or rs is None or rs.size == C, "reason must hold C entries")
        _need(0 <= max_new <= 0xFFFFFFFF, "max_new must be a u32")
        tm = _opt_n(t_max, n_cand, "t_max", "n_cand")
        summary = np.empty((n_cand, _lib.GROW_WORDS), np.uint32)
        assign = np.empty((n_cand, C), np.uint32) if want_assign else None
        cs = FpContainers(C, *(_ptr(x) for x in cont))
        head = (ct.byref(cs), _arg(rs if reason_mask else None), reason_mask)
        tail = (n_cand, _arg(tpl[0]), _arg(tpl[1]), _arg(tpl[2]), _arg(tm), max_new)
        if policy is None:
            self._call("fp_grow_sweep", *head, *tail, _arg(summary), _arg(assign))
            return summary, assign
        nc = _opt_n(node_count, N, "node_count")
        dom, td = _opt_n(domain, N, "domain"), _opt_n(t_domain, n_cand, "t_domain", "n_cand")
        max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)
        qt = _quota_rows(quota, 1) if quota is not None else None
        qu = _opt_n(quota_used, _lib.QUOTA_DIMS, "quota_used", "3")
        rows = np.empty((n_cand, _lib.GROW_POLICY_WORDS), np.uint32)
        hops = np.empty((n_cand, C), np.uint8) if want_assign else None
        why = np.empty((n_cand, C), np.uint8) if want_assign else None
        ns = FpNodes(N, *(_ptr(x) for x in live))
        self._call("fp_grow_sweep_policy", *head, ct.byref(ns), _arg(nc), *tail, strategy_id(strategy),
                   int(preferred) & 0xFFFFFFFF, _arg(dom), _arg(td), max_skew, _arg(rm), n_hops, _arg(qt), _arg(qu),
                   _arg(summary), _arg(rows), _arg(assign), _arg(hops), _arg(why))
        return summary, rows, assign, hops, why

    def drain_sweep(self, cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None):
        """Drain what-if sweep (SPEC.md 2.11, fp_drain_sweep): ``nodes`` is the live table, ``assign`` [C] the
        node each container runs on (NONE = not running), ``group`` [N] the candidate each node belongs to
        (< ``n_cand``, NONE = none).  Every candidate's evictees are re-placed, independently and from the
        same base state, on the schedulable nodes outside the candidate under ``strategy`` / ``preferred``
        (SPEC.md 2.6) and ``node_count`` ([N] or None = zeros).  Inputs are not mutated.  Returns
        (assign_out [C], reason [C], summary [n_cand, 8]); summary's word indices are _lib.DRAIN_*."""
        return self._drain_host(cont, nodes, assign, group, n_cand, strategy, preferred, node_count)

    def drain_sweep_policy(self, cont, nodes, assign, group, n_cand, strategy=0, preferred=0, node_count=None, *,
                           domain=None, max_skew=0, relax_mask=()):
        """The drain sweep under the policy (SPEC.md 2.15, fp_drain_sweep_policy): ``drain_sweep`` with every
        move held to the spread constraint (``domain`` [N] ids below 64 and ``max_skew``; None or 0 = none,
        ``domain`` is then not read) and the fallback chain (``relax_mask``: per hop the label bits it gives
        up, at most 4; empty = none).  Each candidate's domain counts leave its own nodes out and a domain is
        eligible when it has a target.  There is no quota: a move releases and retakes the same request.
        Returns (assign_out [C], reason [C] with REASON_SKEW beside REASON_NOFIT, summary [n_cand, 8], hops
        [C], policy_rows [n_cand, 4]); the policy rows' word indices are _lib.DRAIN_STRANDED_SKEW, .."""
        return self._drain_host(cont, nodes, assign, group, n_cand, strategy, preferred, node_count,
                                (domain, max_skew, relax_mask))

    def drain(self, cont, nodes, assign, drain_mask, strategy=0, preferred=0, node_count=None):
        """Evacuate the nodes of ``drain_mask`` ([N], non-zero = drained) from a live plan: one drain_sweep
        with a single candidate, and its moves applied on the host to copies of the node table and of the
        counts (a move deducts the request on its target as SPEC.md 2.6 does; nothing is returned to the
        drained nodes).  Returns (assign_after, reason, nodes_after, node_count_after, summary_row);
        node_count_after starts from zeros without ``node_count``."""
        cont, nodes = _tables(cont, nodes, None, None, True)
        C, N = cont[0].size, nodes[0].size
        asg = _u32(assign)
        mask = np.ascontiguousarray(drain_mask).reshape(-1) != 0
        self._need(asg.size == C, "assign must hold C entries")
        self._need(mask.size == N, "drain_mask must hold N entries")
        nc = _u32(node_count).copy() if node_count is not None else np.zeros(N, np.uint32)
        self._need(nc.size == N, "node_count must hold N entries")
        group = np.where(mask, 0, NONE).astype(np.uint32)
        out, reason, summary = self.drain_sweep(cont, nodes, asg, group, 1, strategy, preferred, nc)
        cf, mf, _, cu, _ = nodes
        running = asg != NONE
        moved = np.flatnonzero(running & mask[np.where(running, asg, 0)] & (out != NONE)) if N else np.empty(0, np.int64)
        for c in moved:  # u32, wraps as the library's own update does
            n = int(out[c])
            cf[n:n + 1] -= cont[0][c]
            mf[n:n + 1] -= cont[1][c]
            cu[n] |= cont[3][c]
            nc[n:n + 1] += np.uint32(1)
        return out, reason, nodes, nc, summary[0]

    def shrink_sweep(self, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None):
        """Scale-in sweep (SPEC.md 2.16, fp_shrink_sweep): ``nodes`` is the live table, ``assign`` [C] the node
        each container runs on (NONE = not running), ``try_order`` [n_var, n_try] one release order per row (node
        indices; NONE entries are skipped, so rows may be ragged).  Every variant starts from the base state and
        tries its nodes in order: the containers now on the node are re-placed on the schedulable nodes that are
        not released under ``strategy`` / ``preferred`` (SPEC.md 2.6) and ``node_count`` ([N] or None = zeros);
        when all fit the node is released, otherwise the attempt is undone.  Inputs are not mutated.  Returns
        (assign_out [n_var, C], state [n_var, N] of _lib.SHRINK_STATE_*, blocker [n_var, N], summary [n_var, 8]);
        summary's word indices are _lib.SHRINK_*."""
        return self._shrink_host(cont, nodes, assign, try_order, strategy, preferred, node_count)

    def shrink_sweep_policy(self, cont, nodes, assign, try_order, strategy=0, preferred=0, node_count=None, *,
                            domain=None, max_skew=0, relax_mask=()):
        """The scale-in sweep under the policy (SPEC.md 2.17, fp_shrink_sweep_policy): ``shrink_sweep`` with every
        move held to the spread constraint (``domain`` [N] ids below 64 and ``max_skew``; None or 0 = none,
        ``domain`` is then not read) and the fallback chain (``relax_mask``: per hop the label bits it gives
        up, at most 4; empty = none).  The domain counts leave the released nodes and the attempt's own node
        out, a domain is eligible while it holds a target, and under a constraint an attempt whose containers
        all found a target commits only when the skew it leaves is within ``max_skew`` or no larger than before
        (the bound rule).  There is no quota: a move releases and retakes the same request.  Returns (assign_out
        [n_var, C], state [n_var, N], blocker [n_var, N], summary [n_var, 8], hops [n_var, C], blocker_reason
        [n_var, N] with REASON_SKEW beside REASON_NOFIT, policy_rows [n_var, 4]); the policy rows' word indices
        are _lib.SHRINK_FAILED_SKEW, .."""
        return self._shrink_host(cont, nodes, assign, try_order, strategy, preferred, node_count,
                                 (domain, max_skew, relax_mask))

    def rebalance_sweep(self, cont, nodes, assign, victim_order, strategy=0, preferred=0, node_count=None, *,
                        domain=None, max_skew=0, relax_mask=(), max_moves=None, want_hops=True, want_reason=True):
        """Rebalance sweep (SPEC.md 2.19, fp_rebalance_sweep): ``nodes`` is the live table, ``assign`` [C] the node
        each container runs on (NONE = not running), ``victim_order`` [n_var, n_try] one victim order per row
        (container indices; NONE entries are skipped, so rows may be ragged), ``max_moves`` [n_var] the move budget
        of each (NONE = unlimited; None = unlimited everywhere).  ``node_count`` None means derived from ``assign``,
        not zeros.  Every variant starts from the base state and visits its entries in order: a container whose
        node lies in a heavy domain (eligible, count - min > ``max_skew``) is lifted off its node and placed as the
        only container of a place_policy_fallback call under ``strategy`` / ``preferred``, the spread constraint
        (``domain`` [N] ids below 64 and ``max_skew``; None or 0 = nothing is heavy, ``domain`` is then not read)
        and the fallback chain (``relax_mask``, at most 4 hops; empty = none); a rejected attempt leaves the state
        exactly as it was.  Inputs are not mutated.  Returns (assign_out [n_var, C], hops [n_var, C], reason [n_var,
        C] with REASON_NOFIT / REASON_SKEW where the container's last attempt was rejected, summary [n_var, 8]);
        hops and reason are None when not wanted; summary's word indices are _lib.REBAL_*."""
        cont, nodes = _tables(cont, nodes, None, None, False)
        C, N = cont[0].size, nodes[0].size
        asg, vo = _u32(assign), _u32(victim_order)
        _need(vo.ndim == 2, "victim_order must be [n_var, n_try]")
        n_var, n_try = vo.shape
        strategy = strategy_id(strategy)
        _need(asg.size == C, "assign must hold C entries")
        mm = _opt_n(max_moves, n_var, "max_moves", "n_var")
        nc, dom = _opt_n(node_count, N, "node_count"), _opt_n(domain, N, "domain")
        max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)
        out, summary = np.empty((n_var, C), np.uint32), np.empty((n_var, _lib.REBAL_WORDS), np.uint32)
        hops = np.empty((n_var, C), np.uint8) if want_hops else None
        why = np.empty((n_var, C), np.uint8) if want_reason else None
        cs, ns = _pair(cont, nodes)
        self._call("fp_rebalance_sweep", ct.byref(cs), ct.byref(ns), _arg(asg), _arg(vo), n_var, n_try, _arg(mm), strategy,
                   int(preferred) & 0xFFFFFFFF, _arg(nc), _arg(dom), max_skew, _arg(rm), n_hops, _arg(out), _arg(hops),
                   _arg(why), _arg(summary))
        return out, hops, why, summary

    def grow_sweep(self, cont, reason, templates, max_new, reason_mask=1 << _lib.REASON_NOFIT, t_max=None,
                   want_assign=False):
        """Scale-out sweep (SPEC.md 2.12, fp_grow_sweep): the pending containers are those of ``cont`` whose
        ``reason`` [C] has its bit set in ``reason_mask`` (0 = every container, ``reason`` may be None);
        ``templates`` = (t_cpu, t_mem, t_labels), one entry per candidate server template.  Every candidate
        is computed independently: first fit of the pending containers on ``t_max[k]`` (None = ``max_new``
        everywhere; ``max_new`` <= GROW_MAX_NEW) empty servers of the template.  Inputs are not mutated.
        Returns (summary [n_cand, 8], assign): summary's word indices are _lib.GROW_*, and assign is
        [n_cand, C] with ``want_assign`` (the ordinal of the new server of a placed pending container, NONE
        for every other one), else None."""
        return self._grow_host(cont, reason, templates, max_new, reason_mask, t_max, want_assign)

    def grow_sweep_policy(self, cont, reason, nodes, templates, max_new, reason_mask=1 << _lib.REASON_NOFIT,
                          t_max=None, strategy=0, preferred=0, node_count=None, *, domain=None, t_domain=None,
                          max_skew=0, relax_mask=(), quota=None, quota_used=None, want_assign=False):
        """The scale-out sweep under the policy (SPEC.md 2.18, fp_grow_sweep_policy): ``grow_sweep`` where
        candidate k is one ``place_policy_quota`` of the pending containers on the live table ``nodes`` (read
        only, N may be 0; ``node_count`` [N] or None = zeros) followed by ``t_max[k]`` empty servers of the
        template, under ``strategy`` / ``preferred`` (SPEC.md 2.6), the spread constraint (``domain`` [N] and
        ``t_domain`` [n_cand] ids below 64, ``max_skew``; ``t_domain`` None or ``max_skew`` 0 = none, neither is
        then read), the fallback chain (``relax_mask``, at most 4 hops; empty = none) and the quota (``quota`` =
        (cpu_m, mem_mib, services) with None = no cap, ``quota_used`` what the tenant holds, read only; None = no
        quota).  N + ``max_new`` <= FP_POLICY_MAX_NODES.  Inputs are not mutated.  Returns (summary [n_cand, 8],
        policy_rows [n_cand, 8], assign, hops, reason): the policy rows' word indices are _lib.GROW_ON_LIVE, ..;
        the last three are [n_cand, C] with ``want_assign`` (assign = the node in the combined table, N + j the
        j-th new server, NONE for every container that is not pending or not placed), else None."""
        return self._grow_host(cont, reason, templates, max_new, reason_mask, t_max, want_assign,
                               (nodes, strategy, preferred, node_count, domain, t_domain, max_skew, relax_mask, quota,
                                quota_used))

    # -- device-pointer API -------------------------------------------------------------
    def _grow_dev(self, cont_t, reason_t, templates_t, max_new, summary_t, reason_mask, t_max_t, assign_out_t,
                  policy=None):
        if policy is None:
            C, _, cs, _ = _dev_tables_checks(cont_t)
        else:
            (nodes_t, strategy, preferred, count_t, domain_t, t_domain_t, max_skew, relax_mask, quota, quota_used,
             policy_t, hops_t, reason_out_t) = policy
            C, N, cs, ns = _dev_tables_checks(cont_t, nodes_t)
        _need(len(templates_t) == 3, "templates_t must be (t_cpu, t_mem, t_labels)")
        n_cand = templates_t[0].numel()
        _need(all(t.numel() == n_cand and t.element_size() == 4 for t in templates_t),
              "every template tensor must hold n_cand 32-bit entries")
        reason_mask, max_new = int(reason_mask), int(max_new)
        _need(0 <= reason_mask <= 0xFFFFFFFF, "reason_mask must be a u32")
        _need(reason_mask == 0 or reason_t is None or (reason_t.numel() == C and reason_t.element_size() == 1),
              "reason_t must hold C bytes")
        _need(0 <= max_new <= 0xFFFFFFFF, "max_new must be a u32")
        _tensor("t_max_t", t_max_t, n_cand, "n_cand", optional=True)
        _tensor("summary_t", summary_t, n_cand * _lib.GROW_WORDS, "n_cand * 8")
        _tensor("assign_out_t", assign_out_t, n_cand * C, "n_cand * C", optional=True)
        head = (ct.byref(cs), _arg(reason_t if reason_mask else None), reason_mask)
        tail = (n_cand, *(_arg(t) for t in templates_t), _arg(t_max_t), max_new)
        if policy is None:
            return self._call("fp_dev_grow_sweep", *head, *tail, _arg(summary_t), _arg(assign_out_t), dev=True)
        _tensor("count_t", count_t, N, "N", optional=True)
        _tensor("domain_t", domain_t, N, "N", optional=True)
        _tensor("t_domain_t", t_domain_t, n_cand, "n_cand", optional=True)
        max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)  # the three host arrays are read during the call
        _tensor("policy_t", policy_t, n_cand * _lib.GROW_POLICY_WORDS, "n_cand * 8", optional=True)
        _tensor("hops_t", hops_t, n_cand * C, "n_cand * C", 1, True)
        _tensor("reason_out_t", reason_out_t, n_cand * C, "n_cand * C", 1, True)
        qt = _quota_rows(quota, 1) if quota is not None else None
        qu = _opt_n(quota_used, _lib.QUOTA_DIMS, "quota_used", "3")
        self._call("fp_dev_grow_sweep_policy", *head, ct.byref(ns), _arg(count_t), *tail, strategy_id(strategy),
                   int(preferred) & 0xFFFFFFFF, _arg(domain_t), _arg(t_domain_t), max_skew, _arg(rm), n_hops, _arg(qt),
                   _arg(qu), _arg(summary_t), _arg(policy_t), _arg(assign_out_t), _arg(hops_t), _arg(reason_out_t),
                   dev=True)

    def _drain_dev(self, cont_t, nodes_t, assign_t, group_t, n_cand, assign_out_t, reason_t, summary_t, strategy,
                   preferred, count_t, policy=None):
        n_cand, strategy = int(n_cand), strategy_id(strategy)
        C, N, cs, ns = _dev_tables_checks(cont_t, nodes_t)
        _tensor("assign_t", assign_t, C, "C")
        _tensor("group_t", group_t, N, "N")
        _tensor("count_t", count_t, N, "N", optional=True)
        if policy is not None:
            domain_t, max_skew, relax_mask, hops_t, policy_t = policy
            _tensor("domain_t", domain_t, N, "N", optional=True)
        _need(0 <= n_cand <= 0xFFFFFFFF, "n_cand must be a u32")
        if policy is not None:
            max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)  # rm is read during the call
        _tensor("assign_out_t", assign_out_t, C, "C")
        _tensor("reason_t", reason_t, C, "C", 1)
        _tensor("summary_t", summary_t, n_cand * _lib.DRAIN_WORDS, "n_cand * 8")
        head = (ct.byref(cs), ct.byref(ns), _arg(assign_t), _arg(group_t), n_cand, strategy, int(preferred) & 0xFFFFFFFF,
                _arg(count_t))
        if policy is None:
            return self._call("fp_dev_drain_sweep", *head, _arg(assign_out_t), _arg(reason_t), _arg(summary_t), dev=True)
        _tensor("hops_t", hops_t, C, "C", 1, True)
        _tensor("policy_t", policy_t, n_cand * _lib.DRAIN_POLICY_WORDS, "n_cand * 4", optional=True)
        self._call("fp_dev_drain_sweep_policy", *head, _arg(domain_t), max_skew, _arg(rm), n_hops, _arg(assign_out_t),
                   _arg(reason_t), _arg(hops_t), _arg(summary_t), _arg(policy_t), dev=True)

    def _shrink_dev(self, cont_t, nodes_t, assign_t, try_order_t, n_var, assign_out_t, state_t, summary_t, strategy,
                    preferred, count_t, blocker_t, policy=None):
        n_var, strategy = int(n_var), strategy_id(strategy)
        C, N, cs, ns = _dev_tables_checks(cont_t, nodes_t)
        _tensor("assign_t", assign_t, C, "C")
        _need(0 <= n_var <= 0xFFFFFFFF, "n_var must be a u32")
        _need(try_order_t.element_size() == 4 and (try_order_t.numel() % n_var == 0 if n_var
                                                   else try_order_t.numel() == 0),
              "try_order_t must hold n_var rows of 32-bit entries")
        n_try = try_order_t.numel() // n_var if n_var else 0
        _tensor("count_t", count_t, N, "N", optional=True)
        if policy is not None:
            domain_t, max_skew, relax_mask, hops_t, blocker_reason_t, policy_t = policy
            _tensor("domain_t", domain_t, N, "N", optional=True)
            max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)  # rm is read during the call
        _tensor("assign_out_t", assign_out_t, n_var * C, "n_var * C")
        _tensor("state_t", state_t, n_var * N, "n_var * N", 1)
        _tensor("blocker_t", blocker_t, n_var * N, "n_var * N", optional=True)
        _tensor("summary_t", summary_t, n_var * _lib.SHRINK_WORDS, "n_var * 8")
        head = (ct.byref(cs), ct.byref(ns), _arg(assign_t), _arg(try_order_t), n_var, n_try, strategy,
                int(preferred) & 0xFFFFFFFF, _arg(count_t))
        outs = (_arg(assign_out_t), _arg(state_t), _arg(blocker_t), _arg(summary_t))
        if policy is None:
            return self._call("fp_dev_shrink_sweep", *head, *outs, dev=True)
        _tensor("hops_t", hops_t, n_var * C, "n_var * C", 1, True)
        _tensor("blocker_reason_t", blocker_reason_t, n_var * N, "n_var * N", 1, True)
        _tensor("policy_t", policy_t, n_var * _lib.SHRINK_POLICY_WORDS, "n_var * 4", optional=True)
        self._call("fp_dev_shrink_sweep_policy", *head, _arg(domain_t), max_skew, _arg(rm), n_hops, *outs, _arg(hops_t),
                   _arg(blocker_reason_t), _arg(policy_t), dev=True)

    def dev_grow_sweep_policy(self, cont_t, reason_t, nodes_t, templates_t, max_new, summary_t,
                              reason_mask=1 << _lib.REASON_NOFIT, t_max_t=None, strategy=0, preferred=0, count_t=None, *,
                              domain_t=None, t_domain_t=None, max_skew=0, relax_mask=(), quota=None, quota_used=None,
                              policy_t=None, assign_out_t=None, hops_t=None, reason_out_t=None):
        """fp_dev_grow_sweep_policy on device tensors: ``dev_grow_sweep``'s arguments, ``nodes_t`` = the live table
        (cpu_free, mem_free, labels, conflict_used [N] int32 storage, schedulable [N] uint8) with ``count_t`` [N]
        or None, ``domain_t`` [N] and ``t_domain_t`` [n_cand] or None, and the optional results ``policy_t``
        [n_cand * 8], ``assign_out_t`` [n_cand * C], ``hops_t`` and ``reason_out_t`` [n_cand * C] uint8.
        ``max_new``, ``max_skew``, ``relax_mask``, ``quota`` and ``quota_used`` are host values.  A t_max above
        max_new or a domain value out of range is found on the device: nothing is written and sync() raises
        FP_EINVAL."""
        self._grow_dev(cont_t, reason_t, templates_t, max_new, summary_t, reason_mask, t_max_t, assign_out_t,
                       (nodes_t, strategy, preferred, count_t, domain_t, t_domain_t, max_skew, relax_mask, quota,
                        quota_used, policy_t, hops_t, reason_out_t))

    def dev_grow_sweep(self, cont_t, reason_t, templates_t, max_new, summary_t, reason_mask=1 << _lib.REASON_NOFIT,
                       t_max_t=None, assign_out_t=None):
        """fp_dev_grow_sweep on device tensors: ``cont_t`` = (cpu, mem, req, conf) [C] each (int32 storage of
        u32 values), ``reason_t`` [C] uint8 or None (``reason_mask`` 0), ``templates_t`` = (t_cpu, t_mem,
        t_labels) [n_cand] each, ``t_max_t`` [n_cand] or None; out: ``summary_t`` [n_cand * 8] and
        ``assign_out_t`` [n_cand * C] or None.  ``max_new`` is a host value.  A t_max above max_new is found
        on the device: nothing is written and sync() raises FP_EINVAL."""
        self._grow_dev(cont_t, reason_t, templates_t, max_new, summary_t, reason_mask, t_max_t, assign_out_t)

    def dev_drain_sweep(self, cont_t, nodes_t, assign_t, group_t, n_cand, assign_out_t, reason_t, summary_t, strategy=0,
                        preferred=0, count_t=None):
        """fp_dev_drain_sweep on device tensors: ``cont_t`` = (cpu, mem, req, conf) [C] each and ``nodes_t`` =
        (cpu_free, mem_free, labels, conflict_used [N] int32 storage, schedulable [N] uint8), ``assign_t``
        [C], ``group_t`` [N], ``count_t`` [N] or None; out: ``assign_out_t`` [C], ``reason_t`` [C] uint8,
        ``summary_t`` [n_cand * 8].  A group or assign value out of range is found on the device: nothing is
        written and sync() raises FP_EINVAL."""
        self._drain_dev(cont_t, nodes_t, assign_t, group_t, n_cand, assign_out_t, reason_t, summary_t, strategy,
                        preferred, count_t)

    def dev_shrink_sweep(self, cont_t, nodes_t, assign_t, try_order_t, n_var, assign_out_t, state_t, summary_t,
                         strategy=0, preferred=0, count_t=None, blocker_t=None):
        """fp_dev_shrink_sweep on device tensors: ``cont_t``, ``nodes_t``, ``assign_t`` and ``count_t`` as in
        ``dev_drain_sweep``, ``try_order_t`` [n_var * n_try]; out: ``assign_out_t`` [n_var * C], ``state_t``
        [n_var * N] uint8, ``summary_t`` [n_var * 8] and ``blocker_t`` [n_var * N] or None.  An assign or
        try_order value out of range is found on the device: nothing is written and sync() raises FP_EINVAL."""
        self._shrink_dev(cont_t, nodes_t, assign_t, try_order_t, n_var, assign_out_t, state_t, summary_t, strategy,
                         preferred, count_t, blocker_t)

    def dev_shrink_sweep_policy(self, cont_t, nodes_t, assign_t, try_order_t, n_var, assign_out_t, state_t, summary_t,
                                strategy=0, preferred=0, count_t=None, blocker_t=None, *, domain_t=None, max_skew=0,
                                relax_mask=(), hops_t=None, blocker_reason_t=None, policy_t=None):
        """fp_dev_shrink_sweep_policy on device tensors: ``dev_shrink_sweep``'s arguments, then ``domain_t`` [N] or
        None, ``max_skew``, ``relax_mask`` (host values, at most 4) and the optional results ``hops_t`` [n_var * C]
        uint8, ``blocker_reason_t`` [n_var * N] uint8 and ``policy_t`` [n_var * 4].  An assign, try_order or
        domain value out of range is found on the device: nothing is written and sync() raises FP_EINVAL."""
        self._shrink_dev(cont_t, nodes_t, assign_t, try_order_t, n_var, assign_out_t, state_t, summary_t, strategy,
                         preferred, count_t, blocker_t, (domain_t, max_skew, relax_mask, hops_t, blocker_reason_t,
                                                         policy_t))

    def dev_rebalance_sweep(self, cont_t, nodes_t, assign_t, victim_order_t, n_var, assign_out_t, summary_t, strategy=0,
                            preferred=0, count_t=None, *, domain_t=None, max_skew=0, relax_mask=(), max_moves_t=None,
                            hops_t=None, reason_t=None):
        """fp_dev_rebalance_sweep on device tensors: ``cont_t``, ``nodes_t``, ``assign_t`` and ``count_t`` (None =
        derived from ``assign_t``) as in ``dev_drain_sweep``, ``victim_order_t`` [n_var * n_try], ``max_moves_t``
        [n_var] or None, ``domain_t`` [N] or None, ``max_skew`` and ``relax_mask`` (host values, at most 4); out:
        ``assign_out_t`` [n_var * C], ``summary_t`` [n_var * 8] and the optional ``hops_t`` and ``reason_t``
        [n_var * C] uint8.  An assign, victim_order or domain value out of range is found on the device: nothing is
        written and sync() raises FP_EINVAL."""
        n_var, strategy = int(n_var), strategy_id(strategy)
        C, N, cs, ns = _dev_tables_checks(cont_t, nodes_t)
        _tensor("assign_t", assign_t, C, "C")
        _need(0 <= n_var <= 0xFFFFFFFF, "n_var must be a u32")
        _need(victim_order_t.element_size() == 4 and (victim_order_t.numel() % n_var == 0 if n_var
                                                      else victim_order_t.numel() == 0),
              "victim_order_t must hold n_var rows of 32-bit entries")
        n_try = victim_order_t.numel() // n_var if n_var else 0
        _tensor("max_moves_t", max_moves_t, n_var, "n_var", optional=True)
        _tensor("count_t", count_t, N, "N", optional=True)
        _tensor("domain_t", domain_t, N, "N", optional=True)
        max_skew, rm, n_hops = _skew_chain(max_skew, relax_mask)  # rm is read during the call
        _tensor("assign_out_t", assign_out_t, n_var * C, "n_var * C")
        _tensor("hops_t", hops_t, n_var * C, "n_var * C", 1, True)
        _tensor("reason_t", reason_t, n_var * C, "n_var * C", 1, True)
        _tensor("summary_t", summary_t, n_var * _lib.REBAL_WORDS, "n_var * 8")
        self._call("fp_dev_rebalance_sweep", ct.byref(cs), ct.byref(ns), _arg(assign_t), _arg(victim_order_t), n_var,
                   n_try, _arg(max_moves_t), strategy, int(preferred) & 0xFFFFFFFF, _arg(count_t), _arg(domain_t),
                   max_skew, _arg(rm), n_hops, _arg(assign_out_t), _arg(hops_t), _arg(reason_t), _arg(summary_t),
                   dev=True)

    def dev_drain_sweep_policy(self, cont_t, nodes_t, assign_t, group_t, n_cand, assign_out_t, reason_t, summary_t,
                               strategy=0, preferred=0, count_t=None, *, domain_t=None, max_skew=0, relax_mask=(),
                               hops_t=None, policy_t=None):
        """fp_dev_drain_sweep_policy on device tensors: ``dev_drain_sweep``'s arguments, then ``domain_t`` [N] or
        None, ``max_skew``, ``relax_mask`` (host values, at most 4: the one array of a dev_* call that is not a
        tensor) and the optional results ``hops_t`` [C] uint8 and ``policy_t`` [n_cand * 4].  A group, assign or
        domain value out of range is found on the device: nothing is written and sync() raises FP_EINVAL."""
        self._drain_dev(cont_t, nodes_t, assign_t, group_t, n_cand, assign_out_t, reason_t, summary_t, strategy,
                        preferred, count_t, (domain_t, max_skew, relax_mask, hops_t, policy_t))

    def dev_explain(self, db: "DevBatch", rows_t, sel_t=None, ignore_labels=0, scenario=0):
        """fp_dev_explain on one scenario of ``db`` (offset pointers, as dev_feasibility): ``rows_t``
        [M * 16] int32 storage, ``sel_t`` [M] container indices or None = every container.  A sel index
        >= C is found on the device: no row is written and sync() raises FP_ECORRUPT."""
        C, N = db.C, db.N
        o, p = scenario * C, scenario * N
        M = C if sel_t is None else sel_t.numel()
        self._need(rows_t.numel() >= M * _lib.EXPLAIN_WORDS, "rows_t must hold M * 16 entries")
        cs = FpContainers(C, db.cpu[o:].data_ptr(), db.mem[o:].data_ptr(), db.req[o:].data_ptr(),
                          db.conf[o:].data_ptr())
        ns = FpNodes(N, db.cf[p:].data_ptr(), db.mf[p:].data_ptr(), db.lab[p:].data_ptr(), db.cu[p:].data_ptr(),
                     db.sched[p:].data_ptr())
        self._dev(lambda: check(self._L.fp_dev_explain(
            self._ctx, ct.byref(cs), ct.byref(ns), sel_t.data_ptr() if sel_t is not None else None, M,
            int(ignore_labels) & 0xFFFFFFFF, rows_t.data_ptr()), "fp_dev_explain"))

    def dev_explain_batch(self, db: "DevBatch", reason_mask, ignore_t, hist_t):
        """fp_dev_explain_batch over every scenario of ``db`` (its containers, node state and reason):
        ``ignore_t`` [S] or None, ``hist_t`` [S * 8] out (int32 storage of u32 values)."""
        self._need(ignore_t is None or ignore_t.numel() == db.S, "ignore_t must hold S entries")
        self._need(hist_t.numel() == db.S * _lib.EXPLAIN_HIST_WORDS, "hist_t must hold S * 8 entries")
        self._dev(lambda: check(self._L.fp_dev_explain_batch(
            self._ctx, ct.byref(db.struct()), int(reason_mask) & 0xFFFFFFFF,
            ignore_t.data_ptr() if ignore_t is not None else None, hist_t.data_ptr()), "fp_dev_explain_batch"))

    def dev_gen_batch(self, seed, db: "DevBatch", flags=7):
        self._dev(lambda: check(self._L.fp_dev_gen_batch(self._ctx, ct.c_uint64(seed), ct.byref(db.struct()), flags),
                                "fp_dev_gen_batch"))

    def dev_place_batch(self, db: "DevBatch"):
        self._dev(lambda: check(self._L.fp_dev_place_batch(self._ctx, ct.byref(db.struct())), "fp_dev_place_batch"))

    def dev_place_batch_policy(self, db: "DevBatch", strategy_t, preferred_t=None, count_t=None, *, domain_t=None,
                               max_skew_t=None):
        """fp_dev_place_batch_policy: ``strategy_t`` [S] (int32 storage of fp_strategy values),
        ``preferred_t`` [S] or None, ``count_t`` [S*N] in/out or None -- device tensors.  ``domain_t``
        [S*N] with ``max_skew_t`` [S] (int32 storage of u32 values) is the topology spread of SPEC.md 2.7
        (fp_dev_place_batch_policy_spread); either one None is no constraint."""
        domain_t, max_skew_t, _, _ = _dev_policy_checks(db, strategy_t, preferred_t, count_t, domain_t, max_skew_t)
        head = (self._ctx, ct.byref(db.struct()), _arg(strategy_t), _arg(preferred_t), _arg(count_t))
        if domain_t is not None:
            self._dev(lambda: check(self._L.fp_dev_place_batch_policy_spread(*head, _arg(domain_t), _arg(max_skew_t)),
                                    "fp_dev_place_batch_policy_spread"))
        else:
            self._dev(lambda: check(self._L.fp_dev_place_batch_policy(*head), "fp_dev_place_batch_policy"))

    def dev_place_batch_policy_fallback(self, db: "DevBatch", strategy_t, preferred_t=None, count_t=None, *,
                                        domain_t=None, max_skew_t=None, relax_mask_t=None, n_hops_t=None, hops_t=None):
        """fp_dev_place_batch_policy_fallback: dev_place_batch_policy under the fallback chains of SPEC.md
        2.8 -- ``relax_mask_t`` [S * FP_FALLBACK_MAX_HOPS] with ``n_hops_t`` [S] (int32 storage of u32
        values; either one None is no fallback), ``hops_t`` [S*C] uint8 out or None.  An n_hops above
        FP_FALLBACK_MAX_HOPS is found on the device: nothing is written and sync() raises FP_EINVAL.
        Returns hops_t."""
        pairs = _dev_policy_checks(db, strategy_t, preferred_t, count_t, domain_t, max_skew_t, relax_mask_t, n_hops_t,
                                   hops_t)
        args = [_arg(t) for t in (strategy_t, preferred_t, count_t, *pairs, hops_t)]
        self._dev(lambda: check(self._L.fp_dev_place_batch_policy_fallback(self._ctx, ct.byref(db.struct()), *args),
                                "fp_dev_place_batch_policy_fallback"))
        return hops_t

    def dev_place_batch_policy_quota(self, db: "DevBatch", strategy_t, quota_t, quota_used_t=None, preferred_t=None,
                                     count_t=None, *, domain_t=None, max_skew_t=None, relax_mask_t=None, n_hops_t=None,
                                     hops_t=None, quota_why_t=None):
        """fp_dev_place_batch_policy_quota: dev_place_batch_policy_fallback under the quotas of SPEC.md 2.10
        -- ``quota_t`` [S * 3] (int32 storage of u32 caps, -1 = QUOTA_UNLIMITED; None = no quota anywhere),
        ``quota_used_t`` [S * 3] in/out or None (usage starts at zero and is not returned), ``quota_why_t``
        [S*C] uint8 out or None.  Returns (hops_t, quota_why_t, quota_used_t)."""
        pairs = _dev_policy_checks(db, strategy_t, preferred_t, count_t, domain_t, max_skew_t, relax_mask_t, n_hops_t,
                                   hops_t)
        for t in (quota_t, quota_used_t):
            self._need(t is None or (t.numel() == db.S * _lib.QUOTA_DIMS and t.element_size() == 4),
                       "quota_t and quota_used_t must hold S * 3 32-bit entries")
        self._need(quota_why_t is None or (quota_why_t.numel() == db.S * db.C and quota_why_t.element_size() == 1),
                   "quota_why_t must hold S * C bytes")
        args = [_arg(t) for t in (strategy_t, preferred_t, count_t, *pairs, hops_t, quota_t, quota_used_t, quota_why_t)]
        self._dev(lambda: check(self._L.fp_dev_place_batch_policy_quota(self._ctx, ct.byref(db.struct()), *args),
                                "fp_dev_place_batch_policy_quota"))
        return hops_t, quota_why_t, quota_used_t

    def dev_replan_batch(self, db: "DevBatch", prev_t, strategy_t, preferred_t=None, count_t=None, change_t=None,
                         summary_t=None):
        """fp_dev_replan_batch (SPEC.md 2.13) on device tensors: ``prev_t`` [S*C] (int32 storage of u32 values,
        -1 = NONE), ``strategy_t`` [S], ``preferred_t`` [S] or None, ``count_t`` [S*N] in/out or None; out:
        ``change_t`` [S*C] uint8 or None and ``summary_t`` [S * 8] or None.  ``db``'s node tables are the base
        tables and are updated in place.  A strategy that is no fp_strategy value and a prev value out of range
        are found on the device: nothing is written and sync() raises FP_EINVAL."""
        _dev_policy_checks(db, strategy_t, preferred_t, count_t, None, None)
        self._need(prev_t.numel() == db.S * db.C and prev_t.element_size() == 4, "prev_t must hold S * C 32-bit entries")
        self._need(change_t is None or (change_t.numel() == db.S * db.C and change_t.element_size() == 1),
                   "change_t must hold S * C bytes")
        self._need(summary_t is None or (summary_t.numel() == db.S * _lib.REPLAN_WORDS and summary_t.element_size() == 4),
                   "summary_t must hold S * 8 32-bit entries")
        args = [_arg(t) for t in (prev_t, strategy_t, preferred_t, count_t, change_t, summary_t)]
        self._dev(lambda: check(self._L.fp_dev_replan_batch(self._ctx, ct.byref(db.struct()), *args),
                                "fp_dev_replan_batch"))

    def dev_replan_batch_policy(self, db: "DevBatch", prev_t, strategy_t, quota_t=None, quota_used_t=None,
                                preferred_t=None, count_t=None, *, domain_t=None, max_skew_t=None, relax_mask_t=None,
                                n_hops_t=None, hops_t=None, quota_why_t=None, change_t=None, summary_t=None):
        """fp_dev_replan_batch_policy (SPEC.md 2.14) on device tensors: the tensors of dev_replan_batch and of
        dev_place_batch_policy_quota.  A strategy, prev, domain or n_hops value out of range is found on the
        device: nothing is written, ``quota_used_t`` included, and sync() raises FP_EINVAL.  Returns (hops_t,
        quota_why_t, quota_used_t)."""
        pairs = _dev_policy_checks(db, strategy_t, preferred_t, count_t, domain_t, max_skew_t, relax_mask_t, n_hops_t,
                                   hops_t)
        self._need(prev_t.numel() == db.S * db.C and prev_t.element_size() == 4, "prev_t must hold S * C 32-bit entries")
        for t in (quota_t, quota_used_t):
            self._need(t is None or (t.numel() == db.S * _lib.QUOTA_DIMS and t.element_size() == 4),
                       "quota_t and quota_used_t must hold S * 3 32-bit entries")
        self._need(quota_why_t is None or (quota_why_t.numel() == db.S * db.C and quota_why_t.element_size() == 1),
                   "quota_why_t must hold S * C bytes")
        self._need(change_t is None or (change_t.numel() == db.S * db.C and change_t.element_size() == 1),
                   "change_t must hold S * C bytes")
        self._need(summary_t is None or (summary_t.numel() == db.S * _lib.REPLAN_WORDS and summary_t.element_size() == 4),
                   "summary_t must hold S * 8 32-bit entries")
        args = [_arg(t) for t in (prev_t, strategy_t, preferred_t, count_t, *pairs, hops_t, quota_t, quota_used_t,
                                  quota_why_t, change_t, summary_t)]
        self._dev(lambda: check(self._L.fp_dev_replan_batch_policy(self._ctx, ct.byref(db.struct()), *args),
                                "fp_dev_replan_batch_policy"))
        return hops_t, quota_why_t, quota_used_t

    def dev_argmin_cost(self, cost_t, out_t):
        self._dev(lambda: check(self._L.fp_dev_argmin_cost(self._ctx, cost_t.data_ptr(), cost_t.numel(),
                                                           out_t.data_ptr()), "fp_dev_argmin_cost"))

    def dev_feasibility(self, db: "DevBatch", first_t, count_t, bitmap_t=None, scenario=0):
        C, N = db.C, db.N
        o, p = scenario * C, scenario * N
        cs = FpContainers(C, db.cpu[o:].data_ptr(), db.mem[o:].data_ptr(), db.req[o:].data_ptr(),
                          db.conf[o:].data_ptr())
        ns = FpNodes(N, db.cf[p:].data_ptr(), db.mf[p:].data_ptr(), db.lab[p:].data_ptr(), db.cu[p:].data_ptr(),
                     db.sched[p:].data_ptr())
        self._dev(lambda: check(self._L.fp_dev_feasibility(
            self._ctx, ct.byref(cs), ct.byref(ns), first_t.data_ptr(), count_t.data_ptr(),
            bitmap_t.data_ptr() if bitmap_t is not None else None), "fp_dev_feasibility"))

    def place_ws_bytes(self, S: int, C: int, N: int) -> int:
        """Device workspace bytes a place batch of S x C x N takes on this context."""
        out = ct.c_uint64(0)
        check(self._L.fp_place_ws_bytes(self._ctx, S, C, N, ct.byref(out)), "fp_place_ws_bytes")
        return int(out.value)

    def dev_feasibility_batch(self, db: "DevBatch", first_t, count_t):
        """Stage 2 over every scenario of ``db`` ([S*C] outputs, scenario-major)."""
        self._dev(lambda: check(self._L.fp_dev_feasibility_batch(self._ctx, ct.byref(db.struct()), first_t.data_ptr(),
                                                                 count_t.data_ptr()), "fp_dev_feasibility_batch"))

    def dev_legacy_order(self, has_deps_t, perm_t):
        """fp_dev_legacy_order (engine.rs:67-85) on a device-resident has_deps vector."""
        g = FpGraph(has_deps_t.numel(), 0, None, None, has_deps_t.data_ptr())
        self._dev(lambda: check(self._L.fp_dev_legacy_order(self._ctx, ct.byref(g), perm_t.data_ptr()),
                                "fp_dev_legacy_order"))

    def dev_levelize(self, row_ptr_t, col_t, has_deps_t, level_t, order_t, ncyc_t):
        V = has_deps_t.numel()
        g = FpGraph(V, col_t.numel(), row_ptr_t.data_ptr(), col_t.data_ptr() if col_t.numel() else None,
                    has_deps_t.data_ptr())
        self._dev(lambda: check(self._L.fp_dev_levelize(self._ctx, ct.byref(g), level_t.data_ptr(), order_t.data_ptr(),
                                                        ncyc_t.data_ptr()), "fp_dev_levelize"))


@dataclass
class DevBatch:
    """Device-resident scenario batch (torch tensors on one GPU, int32 storage
    reinterpreted as uint32 by the kernels)."""
    S: int
    C: int
    N: int
    scen_base: int
    cpu: object
    mem: object
    req: object
    conf: object
    level: object
    cf: object
    mf: object
    lab: object
    cu: object
    sched: object
    assign: object
    reason: object
    cost: object

    @classmethod
    def allocate(cls, S, C, N, device, scen_base=0, with_level=False):
        import torch

        def i32(n):
            return torch.empty(n, dtype=torch.int32, device=device)

        return cls(S, C, N, scen_base, i32(S * C), i32(S * C), i32(S * C), i32(S * C),
                   i32(S * C) if with_level else None, i32(S * N), i32(S * N), i32(S * N), i32(S * N),
                   torch.empty(S * N, dtype=torch.uint8, device=device), i32(S * C),
                   torch.empty(S * C, dtype=torch.uint8, device=device),
                   torch.empty(S, dtype=torch.int64, device=device))

    def struct(self):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return FpBatch(self.S, self.scen_base, self.C, self.N, p(self.cpu), p(self.mem), p(self.req),
                       p(self.conf), p(self.level), p(self.cf), p(self.mf), p(self.lab), p(self.cu),
                       p(self.sched), p(self.assign), p(self.reason), p(self.cost))

    def node_snapshot(self):
        """Copies of the node fields a plan mutates (free cpu, free memory, usage count).
        labels and schedulable are const inputs at the boundary (include/fleetplace.h:99-101),
        so they are neither copied nor restored."""
        return tuple(t.clone() for t in (self.cf, self.mf, self.cu))

    def restore_nodes(self, snap):
        for dst, src in zip((self.cf, self.mf, self.cu), snap):
            dst.copy_(src)
