// fp_ctx.hip -- context lifetime, device arenas, profiling and the synchronous
// host-pointer entry points of include/fleetplace.h.
//
// The host API copies caller arrays into a device staging arena, runs the same
// device pipeline as fp_dev_*, and copies results back only when every kernel
// succeeded ("no partial writes on error").
#include "fp_internal.h"
#include <string.h>
#include <stdlib.h>

int fp_hip_fail(hipError_t e) {
    (void)e;
    if (e == hipErrorOutOfMemory) return FP_ENOMEM;
    return FP_EDEVICE;
}

extern "C" const char *fp_strerror(int code) {
    switch (code) {
    case FP_OK: return "ok";
    case FP_EINVAL: return "invalid argument";
    case FP_ENOMEM: return "out of memory";
    case FP_EDEVICE: return "no gfx950 device or HIP runtime error";
    case FP_EOVERFLOW: return "count overflow";
    case FP_ECORRUPT: return "input violates an invariant";
    default: return "unknown error";
    }
}

extern "C" int fp_abi_version(void) { return FP_ABI_VERSION; }

extern "C" int fp_ctx_create(fp_ctx **out, int device) {
    if (!out) return FP_EINVAL;
    *out = nullptr;
    if (device < 0) return FP_EINVAL;  // no CPU backend by design
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return FP_EDEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FP_EDEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FP_EDEVICE;
    fp_ctx *c = new fp_ctx();
    c->device = device;
    for (int k = 0; k < FP_OPT_COUNT; ++k) c->opt[k] = FP_OPT_AUTO;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->d_err_base, 256) != hipSuccess ||
        hipEventCreateWithFlags(&c->last_ev, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&c->h_small, 4096, hipHostMallocDefault) != hipSuccess) {
        fp_ctx_destroy(c);
        return FP_EDEVICE;
    }
    if (hipMemset(c->d_err_base, 0, 256) != hipSuccess) {
        fp_ctx_destroy(c);
        return FP_EDEVICE;
    }
    c->d_err = c->d_err_base;
    c->stream = c->own_stream;
    *out = c;
    return FP_OK;
}

extern "C" void fp_ctx_destroy(fp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->last_ev) (void)hipEventSynchronize(c->last_ev);
    for (auto &r : c->pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->ws) (void)hipFree(c->ws);
    if (c->stage) (void)hipFree(c->stage);
    if (c->d_err_base) (void)hipFree(c->d_err_base);
    if (c->last_ev) (void)hipEventDestroy(c->last_ev);
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_in_ev) (void)hipEventSynchronize(c->h_in_ev);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_in_ev) (void)hipEventDestroy(c->h_in_ev);
    if (c->h_map) (void)hipHostFree(c->h_map);
    if (c->h_tiny) (void)hipHostFree(c->h_tiny);
    if (c->lvl_q) (void)hipFree(c->lvl_q);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

// Switching streams first waits for this context's work on the old one: the workspace arena
// is reset by every call, so it must not overlap a call on the new stream.  It waits on the
// event the last fp_dev_* call recorded, never on the old stream handle itself, which the
// caller may already have destroyed.
extern "C" int fp_ctx_set_stream(fp_ctx *c, void *s) {
    if (!c) return FP_EINVAL;
    if ((hipStream_t)s != c->stream) {
        FP_HIP(hipSetDevice(c->device));
        FP_HIP(hipEventSynchronize(c->last_ev));
    }
    c->stream = (hipStream_t)s;  // NULL = HIP null stream
    return FP_OK;
}

extern "C" int fp_ctx_set_option(fp_ctx *c, int k, int64_t v) {
    if (!c || k < 0 || k >= FP_OPT_COUNT || v < FP_OPT_AUTO) return FP_EINVAL;
    c->opt[k] = v;
    return FP_OK;
}

extern "C" int fp_ctx_get_option(fp_ctx *c, int k, int64_t *v) {
    if (!c || !v || k < 0 || k >= FP_OPT_COUNT) return FP_EINVAL;
    *v = c->opt[k];
    return FP_OK;
}

extern "C" int fp_ctx_reset_stream(fp_ctx *c) {
    return fp_ctx_set_stream(c, c ? (void *)c->own_stream : nullptr);
}

// Waits for every fp_dev_* call queued on the context's stream and reports the first
// kernel-side error any of them raised since the last report (then clears it).
extern "C" int fp_ctx_sync(fp_ctx *c) {
    if (!c) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    c->d_err = c->d_err_base;
    return fp_take_err(c);
}

// the end of every fp_dev_* entry point: remember where this context's work ends
int fp_dev_done(fp_ctx *c, int rc) {
    if (hipEventRecord(c->last_ev, c->stream) != hipSuccess && rc == FP_OK) rc = FP_EDEVICE;
    return rc;
}

// ---- arenas ----------------------------------------------------------------
// c->last_rng points into the arena: whoever recycles or frees it forgets the pointer
void fp_ws_reset(fp_ctx *c) {
    c->ws_top = 0;
    c->last_rng = nullptr;
}
int fp_ws_reserve(fp_ctx *c, size_t bytes) {
    if (bytes <= c->ws_cap) return FP_OK;
    c->last_rng = nullptr;
    FP_HIP(hipStreamSynchronize(c->stream));
    if (c->ws) (void)hipFree(c->ws);
    c->ws = nullptr;
    c->ws_cap = 0;
    size_t cap = fp_align256(bytes + bytes / 4 + 4096);
    FP_HIP(hipMalloc(&c->ws, cap));
    c->ws_cap = cap;
    return FP_OK;
}
void *fp_ws_take(fp_ctx *c, size_t bytes) {
    const size_t end = fp_take_end(c->ws_top, bytes);
    if (end > c->ws_cap) return nullptr;
    c->ws_top = end;
    return c->ws + (end - bytes);
}
void fp_stage_reset(fp_ctx *c) { c->stage_top = 0; }
int fp_stage_reserve(fp_ctx *c, size_t bytes) {
    if (bytes <= c->stage_cap) return FP_OK;
    FP_HIP(hipStreamSynchronize(c->stream));
    if (c->stage) (void)hipFree(c->stage);
    c->stage = nullptr;
    c->stage_cap = 0;
    size_t cap = fp_align256(bytes + bytes / 4 + 4096);
    FP_HIP(hipMalloc(&c->stage, cap));
    c->stage_cap = cap;
    return FP_OK;
}
void *fp_stage_take(fp_ctx *c, size_t bytes) {
    const size_t end = fp_take_end(c->stage_top, bytes);
    if (end > c->stage_cap) return nullptr;
    c->stage_top = end;
    return c->stage + (end - bytes);
}

int fp_take_err(fp_ctx *c) {
    FP_HIP(hipMemcpyAsync(c->h_small, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    FP_HIP(hipStreamSynchronize(c->stream));
    const uint32_t e = ((const uint32_t *)c->h_small)[0];
    if (!e) return FP_OK;
    FP_HIP(hipMemsetAsync(c->d_err, 0, 4, c->stream));
    FP_HIP(hipStreamSynchronize(c->stream));
    return -(int)e;
}

// ---- profiling ---------------------------------------------------------------
static hipEvent_t ev_get(fp_ctx *c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void fp_prof_begin(fp_ctx *c, int kid, hipEvent_t *a) {
    (void)kid;
    *a = nullptr;
    if (!c->profile) return;
    *a = ev_get(c);
    (void)hipEventRecord(*a, c->stream);
}
void fp_prof_end(fp_ctx *c, int kid, hipEvent_t a) {
    if (!c->profile || !a) return;
    hipEvent_t b = ev_get(c);
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({kid, a, b});
}
extern "C" int fp_ctx_profile(fp_ctx *c, int enable) {
    if (!c) return FP_EINVAL;
    c->profile = enable != 0;
    for (int k = 0; k < FP_K_COUNT; ++k) { c->total_ms[k] = 0; c->launches[k] = 0; }
    return FP_OK;
}
extern "C" int fp_ctx_kernel_stats(fp_ctx *c, int kid, double *total_ms, uint64_t *launches) {
    if (!c || kid < 0 || kid >= FP_K_COUNT) return FP_EINVAL;
    for (auto &r : c->pending) {
        float ms = 0.f;
        FP_HIP(hipEventSynchronize(r.b));
        FP_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        c->total_ms[r.kid] += ms;
        c->launches[r.kid] += 1;
        c->pool.push_back(r.a);
        c->pool.push_back(r.b);
    }
    c->pending.clear();
    if (total_ms) *total_ms = c->total_ms[kid];
    if (launches) *launches = c->launches[kid];
    return FP_OK;
}

// ---- device-pointer entry points ----------------------------------------------
extern "C" int fp_dev_place_batch(fp_ctx *c, const fp_batch *b) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_place_batch_impl(c, b));
}
extern "C" int fp_dev_levelize(fp_ctx *c, const fp_graph *g, uint32_t *level, uint32_t *order,
                               uint32_t *n_cycle_dev) {
    if (!c || !g) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_levelize_impl(c, g, level, order, n_cycle_dev));
}
extern "C" int fp_dev_legacy_order(fp_ctx *c, const fp_graph *g, uint32_t *perm) {
    if (!c || !g) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_legacy_order_impl(c, g, perm));
}
extern "C" int fp_place_ws_bytes(fp_ctx *c, uint32_t n_scen, uint32_t n_containers, uint32_t n_nodes,
                                 uint64_t *bytes_out) {
    if (!c || !bytes_out) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_place_ws_bytes_impl(c, n_scen, n_containers, n_nodes, bytes_out);
}
extern "C" int fp_place_geometry(fp_ctx *c, uint32_t n_scen, uint32_t n_containers, uint32_t n_nodes,
                                 uint32_t *out) {
    if (!c || !out) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_place_geometry_impl(c, n_scen, n_containers, n_nodes, out);
}
extern "C" int fp_dev_feasibility_batch(fp_ctx *c, const fp_batch *b, uint32_t *first, uint32_t *count) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_feasibility_batch_impl(c, b, first, count));
}
extern "C" int fp_dev_feasibility(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns,
                                  uint32_t *first, uint32_t *count, uint64_t *bitmap) {
    if (!c || !cs || !ns) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_feasibility_impl(c, cs, ns, first, count, bitmap));
}

// ---- host-pointer entry points -------------------------------------------------
// Every device buffer of a host-pointer call is one fp_row (fp_layout.h; the lists are in fp_rows.h): its host
// source, its host destination, its size and where the device pointer goes.  The rows of a call, in the order of
// its takes, are all that describes its staging: stage_rows sizes the arena from them, takes and copies in;
// copy_back_all and copy_back_span copy out.

// a pinned host buffer of at least `need` bytes: grown with headroom, the old content dropped
static int grow_pinned(char **buf, size_t *cap, size_t need) {
    if (need <= *cap) return FP_OK;
    if (*buf) (void)hipHostFree(*buf);
    *buf = nullptr;
    *cap = 0;
    const size_t grown = fp_align256(need + need / 4 + 4096);
    FP_HIP(hipHostMalloc(buf, grown, hipHostMallocDefault));
    *cap = grown;
    return FP_OK;
}

// Reserves exactly what the rows take, takes it, hands out the device pointers and issues the copies in: one
// per input that has bytes.
// packed: small host-pointer calls (a fleet.kdl stage: config 1) pay per HIP call, not per byte.  Their inputs,
// which are the leading rows, go through one pinned buffer and ONE host-to-device copy, and copy_back_span
// brings the results and the call's error word back in ONE device-to-host copy (6 HIP calls per fp_levelize
// instead of 10), so the word's slot behind the rows is reserved here too.
static int stage_rows(fp_ctx *c, const fp_row *r, int n, bool packed) {
    size_t off[FP_MAX_ROWS];
    if (n > FP_MAX_ROWS) return FP_EINVAL;
    const size_t end = fp_rows_layout(r, n, 0, off);
    if (int rc = fp_stage_reserve(c, packed ? fp_take_end(end, 4) : end)) return rc;
    fp_stage_reset(c);
    char *base = (char *)fp_stage_take(c, end);
    if (!base) return FP_ENOMEM;
    fp_rows_point(r, n, base, off);
    size_t in_end = 0;  // where the last input that is there ends
    for (int i = 0; i < n; ++i)
        if (r[i].in) in_end = off[i] + r[i].bytes + FP_STAGE_PAD;
    if (!packed) {
        for (int i = 0; i < n; ++i)
            if (r[i].in && r[i].bytes)
                FP_HIP(hipMemcpyAsync(*r[i].dev, r[i].in, r[i].bytes, hipMemcpyHostToDevice, c->stream));
        return FP_OK;
    }
    if (!in_end) return FP_OK;
    if (c->h_in_ev) FP_HIP(hipEventSynchronize(c->h_in_ev));  // the previous copy out of h_in is done
    if (int rc = grow_pinned(&c->h_in, &c->h_in_cap, in_end)) return rc;
    if (!c->h_in_ev) FP_HIP(hipEventCreateWithFlags(&c->h_in_ev, hipEventDisableTiming));
    for (int i = 0; i < n; ++i)
        if (r[i].in) memcpy(c->h_in + off[i], r[i].in, r[i].bytes);
    FP_HIP(hipMemcpyAsync(base, c->h_in, in_end, hipMemcpyHostToDevice, c->stream));
    FP_HIP(hipEventRecord(c->h_in_ev, c->stream));
    return FP_OK;
}
template <int N>
static int stage_rows(fp_ctx *c, const fp_row (&r)[N], bool packed = false) {
    return stage_rows(c, r, N, packed);
}

// Results of a host-pointer call: every device buffer goes to pinned staging first; the caller's buffers are
// written only after the kernels' error word and every copy came back clean ("on error nothing is written",
// fleetplace.h).
static int copy_back_all(fp_ctx *c, const fp_row *r, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i)
        if (r[i].out && r[i].bytes) total += fp_align256(r[i].bytes);
    if (int rc = grow_pinned(&c->h_stage, &c->h_stage_cap, total)) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (!r[i].out || !r[i].bytes) continue;
        FP_HIP(hipMemcpyAsync(c->h_stage + off, *r[i].dev, r[i].bytes, hipMemcpyDeviceToHost, c->stream));
        off += fp_align256(r[i].bytes);
    }
    const int rc = fp_take_err(c);  // synchronises the copies too
    if (rc) return rc;
    off = 0;
    for (int i = 0; i < n; ++i) {
        if (!r[i].out || !r[i].bytes) continue;
        memcpy(r[i].out, c->h_stage + off, r[i].bytes);
        off += fp_align256(r[i].bytes);
    }
    return FP_OK;
}
// The results of a packed call (stage_rows): the rows from the first result on are a contiguous span of the
// staging arena.  The call's error word is copied behind them on the device, the span comes back in one copy,
// and the caller's buffers are written only when that word is clean.
static int copy_back_span(fp_ctx *c, const fp_row *r, int n) {
    const char *lo = nullptr;
    for (int i = 0; i < n && !lo; ++i)
        if (r[i].out || r[i].take) lo = (const char *)*r[i].dev;
    uint32_t *slot = (uint32_t *)fp_stage_take(c, 4);
    if (!slot) return FP_ENOMEM;
    if (!lo) lo = (const char *)slot;
    const size_t span = (size_t)((const char *)slot + 4 - lo);
    if (int rc = grow_pinned(&c->h_stage, &c->h_stage_cap, span)) return rc;
    FP_HIP(hipMemcpyAsync(slot, c->d_err, 4, hipMemcpyDeviceToDevice, c->stream));
    FP_HIP(hipMemcpyAsync(c->h_stage, lo, span, hipMemcpyDeviceToHost, c->stream));
    FP_HIP(hipStreamSynchronize(c->stream));
    const uint32_t e = *(const uint32_t *)(c->h_stage + ((const char *)slot - lo));
    if (e) {
        FP_HIP(hipMemsetAsync(c->d_err, 0, 4, c->stream));
        FP_HIP(hipStreamSynchronize(c->stream));
        return -(int)e;
    }
    for (int i = 0; i < n; ++i)
        if (r[i].out && r[i].bytes) memcpy(r[i].out, c->h_stage + ((const char *)*r[i].dev - lo), r[i].bytes);
    return FP_OK;
}
template <int N>
static int copy_back_all(fp_ctx *c, const fp_row (&r)[N]) { return copy_back_all(c, r, N); }
template <int N>
static int copy_back_span(fp_ctx *c, const fp_row (&r)[N]) { return copy_back_span(c, r, N); }

extern "C" int fp_legacy_order(fp_ctx *c, const fp_graph *g, uint32_t *perm_out) {
    if (!c || !g || (g->n_vertices && (!g->has_deps || !perm_out))) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    const size_t V = g->n_vertices;
    fp_graph dg = *g;
    dg.row_ptr = nullptr;
    dg.col = nullptr;
    uint32_t *dperm = nullptr;
    const fp_row rows[] = {fp_row_in(g->has_deps, V, &dg.has_deps), fp_row_out(perm_out, V, &dperm)};
    if (int rc = stage_rows(c, rows, true)) return rc;
    if (int rc = fp_dev_legacy_order_impl(c, &dg, dperm)) return rc;
    return copy_back_span(c, rows);
}

extern "C" int fp_levelize(fp_ctx *c, const fp_graph *g, uint32_t *level_out, uint32_t *order_out,
                           uint32_t *n_cycle_out) {
    if (!c || !g) return FP_EINVAL;
    const size_t V = g->n_vertices, E = g->n_edges;
    if (V && (!g->has_deps || !g->row_ptr || !level_out || !order_out)) return FP_EINVAL;
    if (E && !g->col) return FP_EINVAL;
    if (V == 0) {
        if (E) return FP_ECORRUPT;
        if (n_cycle_out) *n_cycle_out = 0;
        return FP_OK;
    }
    // the CSR is validated on the device (k_check_csr, k_indeg): FP_ECORRUPT
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_graph dg = *g;
    uint32_t *dlev = nullptr, *dord = nullptr, *dcyc = nullptr;
    const fp_row rows[] = {fp_row_in(g->row_ptr, V + 1, &dg.row_ptr), fp_row_in(E ? g->col : nullptr, E, &dg.col),
                           fp_row_in(g->has_deps, V, &dg.has_deps), fp_row_out(level_out, V, &dlev),
                           fp_row_out(order_out, V, &dord), fp_row_out(n_cycle_out, 1, &dcyc)};
    if (int rc = stage_rows(c, rows, true)) return rc;
    if (int rc = fp_dev_levelize_impl(c, &dg, dlev, dord, dcyc)) return rc;
    return copy_back_span(c, rows);
}

// ---- placement: fp_place*, fp_place*_policy* --------------------------------------
static bool batch_has_tables(const fp_batch *b) {
    if (b->n_scen && b->n_containers && (!fp_has_cont(b) || !b->assign || !b->reason)) return false;
    return !(b->n_scen && b->n_nodes) || fp_has_nodes(b);
}

// one scenario's tables as a batch of one (no cost)
static fp_batch single_batch(const fp_containers *cs, const fp_nodes *ns, const uint32_t *level, uint32_t *assign_out,
                             uint8_t *reason_out) {
    fp_batch b = {};
    b.n_scen = 1;
    b.n_containers = cs->n;
    b.n_nodes = ns->n;
    b.cpu_m = cs->cpu_m;
    b.mem_mib = cs->mem_mib;
    b.req_labels = cs->req_labels;
    b.conflict = cs->conflict;
    b.level = level;
    b.cpu_free = ns->cpu_free;
    b.mem_free = ns->mem_free;
    b.labels = ns->labels;
    b.conflict_used = ns->conflict_used;
    b.schedulable = ns->schedulable;
    b.assign = assign_out;
    b.reason = reason_out;
    return b;
}

// A host batch through the staging arena (fp_batch_rows, fp_rows.h): first fit when `o` is null, else scored
static int batch_run(fp_ctx *c, const fp_batch *b, const fp_policy_opts *o) {
    if (!batch_has_tables(b)) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_batch d;
    fp_policy_opts dopt;
    const int n = fp_batch_rows(b, o, &d, &dopt, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = o ? fp_dev_place_batch_policy_impl(c, &d, dopt) : fp_dev_place_batch_impl(c, &d)) return rc;
    return copy_back_all(c, rows, n);
}

extern "C" int fp_place_batch(fp_ctx *c, const fp_batch *b) {
    if (!c || !b) return FP_EINVAL;
    return batch_run(c, b, nullptr);
}

extern "C" int fp_place(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                        uint32_t *assign_out, uint8_t *reason_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    return batch_run(c, &b, nullptr);
}

// The guarantees of a host scored call (host memory: refused before anything is staged): a pair with one half
// null is dropped, a domain id out of range in a constrained scenario and an n_hops above FP_FALLBACK_MAX_HOPS
// are FP_EINVAL, and without quota neither quota_used nor quota_why is touched
static int policy_guarantees(fp_policy_opts &o, size_t S, size_t N) {
    if (!o.domain || !o.max_skew) o.domain = o.max_skew = nullptr;
    for (size_t s = 0; o.max_skew && s < S; ++s)
        if (o.max_skew[s] != 0u && !fp_domains_ok(o.domain + s * N, N)) return FP_EINVAL;
    if (!o.relax_mask || !o.n_hops) o.relax_mask = o.n_hops = nullptr;
    for (size_t s = 0; o.n_hops && s < S; ++s)
        if (o.n_hops[s] > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (!o.quota) o.quota_used = nullptr, o.quota_why = nullptr;
    return FP_OK;
}

// Scored placement (SPEC.md 2.6): fp_place_batch's staging with the per-scenario strategy and
// preferred-label words and the optional node counts.  The strategies are host memory here, so a
// value that is no fp_strategy is refused before anything is staged, and so are the guarantees' (SPEC.md 2.7,
// 2.8, 2.10: policy_guarantees).  hops (nullable) receives the winners' hops; quota_used (nullable) goes in and
// comes back; quota_why (nullable) comes back.
static int batch_policy_host(fp_ctx *c, const fp_batch *b, fp_policy_opts o) {
    const size_t S = b->n_scen, C = b->n_containers, N = b->n_nodes, SC = S * C;
    if (S && !o.strategy) return FP_EINVAL;
    for (size_t s = 0; s < S; ++s)
        if (o.strategy[s] > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (int rc = policy_guarantees(o, S, N)) return rc;
    if ((uint64_t)b->scen_base + S > 65536ull || N > FP_POLICY_MAX_NODES || SC > 0xFFFFFFFFull) return FP_EOVERFLOW;
    return batch_run(c, b, &o);
}

// The twelve exports set the fields their signature has.  A single-scenario export points the per-scenario
// words at its scalar arguments; one that has no domain (or no relax_mask) leaves both of the pair null.
static fp_policy_opts policy_opts(const uint32_t *strategy, const uint32_t *preferred, uint32_t *node_count) {
    fp_policy_opts o;
    o.strategy = strategy;
    o.preferred = preferred;
    o.node_count = node_count;
    return o;
}

extern "C" int fp_place_batch_policy(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                     const uint32_t *preferred_labels, uint32_t *node_count) {
    if (!c || !b) return FP_EINVAL;
    return batch_policy_host(c, b, policy_opts(strategy, preferred_labels, node_count));
}

extern "C" int fp_place_batch_policy_spread(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                            const uint32_t *preferred_labels, uint32_t *node_count,
                                            const uint32_t *domain, const uint32_t *max_skew) {
    if (!c || !b) return FP_EINVAL;
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    return batch_policy_host(c, b, o);
}

extern "C" int fp_place_batch_policy_fallback(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                              const uint32_t *preferred_labels, uint32_t *node_count,
                                              const uint32_t *domain, const uint32_t *max_skew,
                                              const uint32_t *relax_mask, const uint32_t *n_hops, uint8_t *hops_out) {
    if (!c || !b) return FP_EINVAL;
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    return batch_policy_host(c, b, o);
}

extern "C" int fp_place_batch_policy_quota(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                           const uint32_t *preferred_labels, uint32_t *node_count,
                                           const uint32_t *domain, const uint32_t *max_skew, const uint32_t *relax_mask,
                                           const uint32_t *n_hops, uint8_t *hops_out, const uint32_t *quota,
                                           uint32_t *quota_used, uint8_t *quota_why_out) {
    if (!c || !b) return FP_EINVAL;
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return batch_policy_host(c, b, o);
}

extern "C" int fp_place_policy(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                               uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                               uint32_t *assign_out, uint8_t *reason_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    return batch_policy_host(c, &b, policy_opts(&strategy, &preferred_labels, node_count));
}

extern "C" int fp_place_policy_spread(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                                      uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                                      const uint32_t *domain, uint32_t max_skew, uint32_t *assign_out,
                                      uint8_t *reason_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    fp_policy_opts o = policy_opts(&strategy, &preferred_labels, node_count);
    o.domain = domain; o.max_skew = &max_skew;
    return batch_policy_host(c, &b, o);
}

extern "C" int fp_place_policy_fallback(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                                        uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                                        const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask,
                                        uint32_t n_hops, uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    fp_policy_opts o = policy_opts(&strategy, &preferred_labels, node_count);
    o.domain = domain; o.max_skew = &max_skew;
    o.relax_mask = relax_mask; o.n_hops = &n_hops; o.hops = hops_out;
    return batch_policy_host(c, &b, o);
}

extern "C" int fp_place_policy_quota(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                                     uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                                     const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask,
                                     uint32_t n_hops, uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out,
                                     const uint32_t *quota, uint32_t *quota_used, uint8_t *quota_why_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    fp_policy_opts o = policy_opts(&strategy, &preferred_labels, node_count);
    o.domain = domain; o.max_skew = &max_skew;
    o.relax_mask = relax_mask; o.n_hops = &n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return batch_policy_host(c, &b, o);
}

static int dev_policy(fp_ctx *c, const fp_batch *b, const fp_policy_opts &o) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_place_batch_policy_impl(c, b, o));
}

extern "C" int fp_dev_place_batch_policy(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                         const uint32_t *preferred_labels, uint32_t *node_count) {
    return dev_policy(c, b, policy_opts(strategy, preferred_labels, node_count));
}

extern "C" int fp_dev_place_batch_policy_spread(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                                const uint32_t *preferred_labels, uint32_t *node_count,
                                                const uint32_t *domain, const uint32_t *max_skew) {
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    return dev_policy(c, b, o);
}

extern "C" int fp_dev_place_batch_policy_fallback(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                                  const uint32_t *preferred_labels, uint32_t *node_count,
                                                  const uint32_t *domain, const uint32_t *max_skew,
                                                  const uint32_t *relax_mask, const uint32_t *n_hops, uint8_t *hops_out) {
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    return dev_policy(c, b, o);
}

extern "C" int fp_dev_place_batch_policy_quota(fp_ctx *c, const fp_batch *b, const uint32_t *strategy,
                                               const uint32_t *preferred_labels, uint32_t *node_count,
                                               const uint32_t *domain, const uint32_t *max_skew,
                                               const uint32_t *relax_mask, const uint32_t *n_hops, uint8_t *hops_out,
                                               const uint32_t *quota, uint32_t *quota_used, uint8_t *quota_why_out) {
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return dev_policy(c, b, o);
}

// ---- re-planning a running stage (SPEC.md 2.13, fp_replan.hip) --------------------
// A scored batch's staging (batch_run's row list) with prev and the two optional results behind it.  Everything
// the device entry finds on the device is host memory here and refused before anything is staged: replan_checks
// is what both host forms test first, replan_run their staging, run and copy back around the impl of each.
static int replan_checks(const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o) {
    const size_t S = b->n_scen, N = b->n_nodes, SC = S * b->n_containers;
    if (S && !o.strategy) return FP_EINVAL;
    if ((uint64_t)b->scen_base + S > 65536ull || N > FP_POLICY_MAX_NODES || SC > 0xFFFFFFFFull) return FP_EOVERFLOW;
    for (size_t s = 0; s < S; ++s)
        if (o.strategy[s] > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (!batch_has_tables(b) || (SC && !prev)) return FP_EINVAL;
    if (SC && prev == b->assign) return FP_EINVAL;
    return fp_below_or_none(prev, SC, N) ? FP_OK : FP_EINVAL;
}

typedef int replan_impl(fp_ctx *, const fp_batch *, const uint32_t *, const fp_policy_opts &, uint8_t *, uint32_t *);
static int replan_run(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o, uint8_t *change_out,
                      uint32_t *summary_out, replan_impl *impl) {
    if (b->n_scen == 0) return FP_OK;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_batch d;
    fp_policy_opts dopt;
    fp_replan_dev dr;
    const int n = fp_replan_rows(b, &o, prev, change_out, summary_out, &d, &dopt, &dr, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = impl(c, &d, dr.prev, dopt, dr.change, dr.summary)) return rc;
    return copy_back_all(c, rows, n);
}

static int replan_host(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o, uint8_t *change_out,
                       uint32_t *summary_out) {
    if (int rc = replan_checks(b, prev, o)) return rc;
    return replan_run(c, b, prev, o, change_out, summary_out, fp_dev_replan_batch_impl);
}

extern "C" int fp_replan_batch(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                               const uint32_t *preferred_labels, uint32_t *node_count, uint8_t *change_out,
                               uint32_t *summary_out) {
    if (!c || !b) return FP_EINVAL;
    return replan_host(c, b, prev, policy_opts(strategy, preferred_labels, node_count), change_out, summary_out);
}

extern "C" int fp_replan(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level, const uint32_t *prev,
                         uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count, uint32_t *assign_out,
                         uint8_t *reason_out, uint8_t *change_out, uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    return replan_host(c, &b, prev, policy_opts(&strategy, &preferred_labels, node_count), change_out, summary_out);
}

extern "C" int fp_dev_replan_batch(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                                   const uint32_t *preferred_labels, uint32_t *node_count, uint8_t *change_out,
                                   uint32_t *summary_out) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_replan_batch_impl(c, b, prev, policy_opts(strategy, preferred_labels, node_count),
                                                   change_out, summary_out));
}

// ---- re-planning under the policy (SPEC.md 2.14, fp_replan_policy.hip) -------------
// replan_host's checks and batch_policy_host's, all before anything is staged; the rows are fp_replan_rows with
// every policy option (27 rows).
static int replan_policy_host(fp_ctx *c, const fp_batch *b, const uint32_t *prev, fp_policy_opts o, uint8_t *change_out,
                              uint32_t *summary_out) {
    if (int rc = replan_checks(b, prev, o)) return rc;
    if (int rc = policy_guarantees(o, b->n_scen, b->n_nodes)) return rc;
    return replan_run(c, b, prev, o, change_out, summary_out, fp_dev_replan_batch_policy_impl);
}

extern "C" int fp_replan_batch_policy(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                                      const uint32_t *preferred_labels, uint32_t *node_count, const uint32_t *domain,
                                      const uint32_t *max_skew, const uint32_t *relax_mask, const uint32_t *n_hops,
                                      uint8_t *hops_out, const uint32_t *quota, uint32_t *quota_used,
                                      uint8_t *quota_why_out, uint8_t *change_out, uint32_t *summary_out) {
    if (!c || !b) return FP_EINVAL;
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return replan_policy_host(c, b, prev, o, change_out, summary_out);
}

extern "C" int fp_replan_policy(fp_ctx *c, const fp_containers *cs, fp_nodes *ns, const uint32_t *level,
                                const uint32_t *prev, uint32_t strategy, uint32_t preferred_labels, uint32_t *node_count,
                                const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out, const uint32_t *quota,
                                uint32_t *quota_used, uint8_t *quota_why_out, uint8_t *change_out, uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const fp_batch b = single_batch(cs, ns, level, assign_out, reason_out);
    fp_policy_opts o = policy_opts(&strategy, &preferred_labels, node_count);
    o.domain = domain; o.max_skew = &max_skew;
    o.relax_mask = relax_mask; o.n_hops = &n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return replan_policy_host(c, &b, prev, o, change_out, summary_out);
}

extern "C" int fp_dev_replan_batch_policy(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const uint32_t *strategy,
                                          const uint32_t *preferred_labels, uint32_t *node_count,
                                          const uint32_t *domain, const uint32_t *max_skew, const uint32_t *relax_mask,
                                          const uint32_t *n_hops, uint8_t *hops_out, const uint32_t *quota,
                                          uint32_t *quota_used, uint8_t *quota_why_out, uint8_t *change_out,
                                          uint32_t *summary_out) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_policy_opts o = policy_opts(strategy, preferred_labels, node_count);
    o.domain = domain; o.max_skew = max_skew;
    o.relax_mask = relax_mask; o.n_hops = n_hops; o.hops = hops_out;
    o.quota = quota; o.quota_used = quota_used; o.quota_why = quota_why_out;
    return fp_dev_done(c, fp_dev_replan_batch_policy_impl(c, b, prev, o, change_out, summary_out));
}

// ---- feasibility and rejection diagnosis -----------------------------------------
extern "C" int fp_feasibility(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns,
                              uint32_t *first_out, uint32_t *count_out, uint64_t *bitmap_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t C = cs->n, N = ns->n, WC = (C + 63) / 64;
    if (C && (!fp_has_cont(cs) || !first_out || !count_out)) return FP_EINVAL;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_containers dc;
    fp_nodes dn;
    uint32_t *dfirst = nullptr, *dcount = nullptr;
    uint64_t *dbits = nullptr;
    int n = fp_tables_rows(cs, ns, &dc, &dn, rows);
    rows[n++] = fp_row_out(first_out, C, &dfirst);
    rows[n++] = fp_row_out(count_out, C, &dcount);
    rows[n++] = fp_row_opt(bitmap_out, WC * N, &dbits);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = fp_dev_feasibility_impl(c, &dc, &dn, dfirst, dcount, dbits)) return rc;
    return copy_back_all(c, rows, n);
}

// rejection diagnosis (SPEC.md 2.9, fp_explain.hip)
extern "C" int fp_dev_explain(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *sel,
                              uint32_t n_sel, uint32_t ignore_labels, uint32_t *rows_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_explain_impl(c, cs, ns, sel, n_sel, ignore_labels, rows_out));
}

extern "C" int fp_dev_explain_batch(fp_ctx *c, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                                    uint32_t *hist_out) {
    if (!c || !b) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_explain_batch_impl(c, b, reason_mask, ignore_labels, hist_out));
}

extern "C" int fp_explain(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *sel, uint32_t n_sel,
                          uint32_t ignore_labels, uint32_t *rows_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t C = cs->n, N = ns->n;
    if (!sel) n_sel = cs->n;
    const size_t M = n_sel;
    if (M == 0) return FP_OK;
    if (!fp_has_cont(cs) || !rows_out) return FP_EINVAL;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    for (size_t i = 0; sel && i < M; ++i)
        if (sel[i] >= C) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_containers dc;
    fp_nodes dn;
    const uint32_t *dsel = nullptr;
    uint32_t *drows = nullptr;  // 256-byte aligned
    int n = fp_tables_rows(cs, ns, &dc, &dn, rows);
    rows[n++] = fp_row_in(sel, M, &dsel);
    rows[n++] = fp_row_out(rows_out, M * FP_EXPLAIN_WORDS, &drows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = fp_dev_explain_impl(c, &dc, &dn, dsel, n_sel, ignore_labels, drows)) return rc;
    return copy_back_all(c, rows, n);
}

extern "C" int fp_explain_batch(fp_ctx *c, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                                uint32_t *hist_out) {
    if (!c || !b) return FP_EINVAL;
    const size_t S = b->n_scen, C = b->n_containers, N = b->n_nodes;
    const size_t SC = S * C, SN = S * N;
    if (S == 0) return FP_OK;
    if (S > 65535u) return FP_EOVERFLOW;
    if (!hist_out) return FP_EINVAL;
    if (C && (!fp_has_cont(b) || (reason_mask && !b->reason))) return FP_EINVAL;
    if (C && N && !fp_has_nodes(b)) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_batch d = *b;
    d.level = nullptr; d.assign = nullptr; d.cost = nullptr;
    const uint32_t *dign = nullptr;
    uint32_t *dhist = nullptr;
    const size_t SNc = C ? SN : 0;  // without containers the node tables are not read
    const fp_row rows[] = {fp_row_in(b->cpu_m, SC, &d.cpu_m), fp_row_in(b->mem_mib, SC, &d.mem_mib),
                           fp_row_in(b->req_labels, SC, &d.req_labels), fp_row_in(b->conflict, SC, &d.conflict),
                           fp_row_in(b->cpu_free, SNc, &d.cpu_free), fp_row_in(b->mem_free, SNc, &d.mem_free),
                           fp_row_in(b->labels, SNc, &d.labels), fp_row_in(b->conflict_used, SNc, &d.conflict_used),
                           fp_row_in(b->schedulable, SNc, &d.schedulable),
                           fp_row_in(reason_mask ? b->reason : nullptr, SC, &d.reason),
                           fp_row_in(ignore_labels, S, &dign),
                           fp_row_out(hist_out, S * FP_EXPLAIN_HIST_WORDS, &dhist)};
    if (int rc = stage_rows(c, rows)) return rc;
    if (int rc = fp_dev_explain_batch_impl(c, &d, reason_mask, dign, dhist)) return rc;
    return copy_back_all(c, rows);
}

// ---- the what-if sweeps (SPEC.md 2.11, 2.12, 2.15 to 2.18) ----------------------------------------------------
// A plain sweep is the sweep under the policy with an empty policy: each family has ONE host function, which
// takes what the policy export's signature adds as an fp_*_policy (fp_internal.h).  The export's arguments fill
// it (drain_policy, shrink_policy, grow_policy: used by the host and the fp_dev_* export alike), and the host
// function swaps the staged device pointers in before it calls the same *_impl the device export calls.
// relax_mask (and the scale-out sweep's quota and quota_used) are host arrays in both entries.
static fp_drain_policy drain_policy(const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask,
                                    uint32_t n_hops, uint8_t *hops_out, uint32_t *policy_out) {
    fp_drain_policy p;
    p.domain = domain; p.max_skew = max_skew; p.relax_mask = relax_mask; p.n_hops = n_hops;
    p.hops_out = hops_out; p.policy_out = policy_out;
    return p;
}

// drain what-if sweep (SPEC.md 2.11 and 2.15, fp_drain.hip).  Without a domain and an optional result
// fp_drain_policy_rows lays out as fp_drain_rows does: the three further rows take nothing
static int drain_host(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                      const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                      const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out, uint32_t *summary_out,
                      fp_drain_policy pol) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t C = cs->n, N = ns->n;
    if (N > FP_POLICY_MAX_NODES || n_cand > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (pol.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (C && (!fp_has_cont(cs) || !assign || !assign_out || !reason_out)) return FP_EINVAL;
    if (N && (!fp_has_nodes(ns) || !group)) return FP_EINVAL;
    if (n_cand && !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;
    if (!fp_below_or_none(group, N, n_cand) || !fp_below_or_none(assign, C, N)) return FP_EINVAL;
    if (!pol.domain || pol.max_skew == 0u) pol.domain = nullptr;  // otherwise domain is not read
    if (pol.domain && !fp_domains_ok(pol.domain, N)) return FP_EINVAL;
    if (C == 0 && n_cand == 0) return FP_OK;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_drain_dev d;
    fp_drain_policy_dev dp;
    const int n = fp_drain_policy_rows(cs, ns, assign, group, n_cand, node_count, pol.domain, assign_out, reason_out,
                                       pol.hops_out, summary_out, pol.policy_out, &d, &dp, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    pol.domain = dp.domain; pol.hops_out = dp.hops_out; pol.policy_out = dp.policy_out;
    if (int rc = fp_dev_drain_sweep_impl(c, &d.cs, &d.ns, d.assign, d.group, n_cand, strategy, preferred_labels,
                                         d.node_count, d.assign_out, d.reason_out, d.summary, pol))
        return rc;
    return copy_back_all(c, rows, n);
}

extern "C" int fp_dev_drain_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                  const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                                  const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                                  uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_drain_sweep_impl(c, cs, ns, assign, group, n_cand, strategy, preferred_labels,
                                                  node_count, assign_out, reason_out, summary_out));
}

extern "C" int fp_drain_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                              const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred_labels,
                              const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                              uint32_t *summary_out) {
    return drain_host(c, cs, ns, assign, group, n_cand, strategy, preferred_labels, node_count, assign_out, reason_out,
                      summary_out, fp_drain_policy());
}

extern "C" int fp_dev_drain_sweep_policy(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                         const uint32_t *group, uint32_t n_cand, uint32_t strategy,
                                         uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                                         uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                         uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out,
                                         uint32_t *summary_out, uint32_t *policy_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    if (n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_drain_sweep_impl(c, cs, ns, assign, group, n_cand, strategy, preferred_labels,
                                                  node_count, assign_out, reason_out, summary_out,
                                                  drain_policy(domain, max_skew, relax_mask, n_hops, hops_out, policy_out)));
}

extern "C" int fp_drain_sweep_policy(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                     const uint32_t *group, uint32_t n_cand, uint32_t strategy,
                                     uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                                     uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                     uint32_t *assign_out, uint8_t *reason_out, uint8_t *hops_out,
                                     uint32_t *summary_out, uint32_t *policy_out) {
    return drain_host(c, cs, ns, assign, group, n_cand, strategy, preferred_labels, node_count, assign_out, reason_out,
                      summary_out, drain_policy(domain, max_skew, relax_mask, n_hops, hops_out, policy_out));
}

// scale-in sweep (SPEC.md 2.16 and 2.17, fp_shrink.hip)
static fp_shrink_policy shrink_policy(const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask,
                                      uint32_t n_hops, uint8_t *hops_out, uint8_t *blocker_reason_out,
                                      uint32_t *policy_out) {
    fp_shrink_policy p;
    p.domain = domain; p.max_skew = max_skew; p.relax_mask = relax_mask; p.n_hops = n_hops;
    p.hops_out = hops_out; p.blocker_reason_out = blocker_reason_out; p.policy_out = policy_out;
    return p;
}

// no variant is nothing to do, whatever the tables are: found before them.  Without a domain and an optional
// result fp_shrink_policy_rows lays out as fp_shrink_rows does
static int shrink_host(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                       const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                       uint32_t preferred_labels, const uint32_t *node_count, uint32_t *assign_out, uint8_t *state_out,
                       uint32_t *blocker_out, uint32_t *summary_out, fp_shrink_policy pol) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t C = cs->n, N = ns->n;
    if (N > FP_POLICY_MAX_NODES || n_var > 65535u || C > FP_SHRINK_MAX_CONTAINERS) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (pol.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (n_var == 0) return FP_OK;
    if (C && (!fp_has_cont(cs) || !assign || !assign_out)) return FP_EINVAL;
    if (N && (!fp_has_nodes(ns) || !state_out)) return FP_EINVAL;
    if ((n_try && !try_order) || !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;
    if (!fp_below_or_none(assign, C, N) || !fp_below_or_none(try_order, (size_t)n_var * n_try, N)) return FP_EINVAL;
    if (!pol.domain || pol.max_skew == 0u) pol.domain = nullptr;  // otherwise domain is not read
    if (pol.domain && !fp_domains_ok(pol.domain, N)) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_shrink_dev d;
    fp_shrink_policy_dev dp;
    const int n = fp_shrink_policy_rows(cs, ns, assign, try_order, n_var, n_try, node_count, pol.domain, assign_out,
                                        state_out, blocker_out, summary_out, pol.hops_out, pol.blocker_reason_out,
                                        pol.policy_out, &d, &dp, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    pol.domain = dp.domain; pol.hops_out = dp.hops_out; pol.blocker_reason_out = dp.blocker_reason_out;
    pol.policy_out = dp.policy_out;
    if (int rc = fp_dev_shrink_sweep_impl(c, &d.cs, &d.ns, d.assign, d.try_order, n_var, n_try, strategy,
                                          preferred_labels, d.node_count, d.assign_out, d.state_out, d.blocker_out,
                                          d.summary, pol))
        return rc;
    return copy_back_all(c, rows, n);
}

extern "C" int fp_dev_shrink_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                   const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                                   uint32_t preferred_labels, const uint32_t *node_count, uint32_t *assign_out,
                                   uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_shrink_sweep_impl(c, cs, ns, assign, try_order, n_var, n_try, strategy, preferred_labels,
                                                   node_count, assign_out, state_out, blocker_out, summary_out));
}

extern "C" int fp_shrink_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                               const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                               uint32_t preferred_labels, const uint32_t *node_count, uint32_t *assign_out,
                               uint8_t *state_out, uint32_t *blocker_out, uint32_t *summary_out) {
    return shrink_host(c, cs, ns, assign, try_order, n_var, n_try, strategy, preferred_labels, node_count, assign_out,
                       state_out, blocker_out, summary_out, fp_shrink_policy());
}

extern "C" int fp_dev_shrink_sweep_policy(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                          const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                                          uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                                          uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                          uint32_t *assign_out, uint8_t *state_out, uint32_t *blocker_out,
                                          uint32_t *summary_out, uint8_t *hops_out, uint8_t *blocker_reason_out,
                                          uint32_t *policy_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    if (n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_shrink_sweep_impl(c, cs, ns, assign, try_order, n_var, n_try, strategy, preferred_labels,
                                                   node_count, assign_out, state_out, blocker_out, summary_out,
                                                   shrink_policy(domain, max_skew, relax_mask, n_hops, hops_out,
                                                                 blocker_reason_out, policy_out)));
}

extern "C" int fp_shrink_sweep_policy(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                      const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                                      uint32_t preferred_labels, const uint32_t *node_count, const uint32_t *domain,
                                      uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                      uint32_t *assign_out, uint8_t *state_out, uint32_t *blocker_out,
                                      uint32_t *summary_out, uint8_t *hops_out, uint8_t *blocker_reason_out,
                                      uint32_t *policy_out) {
    return shrink_host(c, cs, ns, assign, try_order, n_var, n_try, strategy, preferred_labels, node_count, assign_out,
                       state_out, blocker_out, summary_out,
                       shrink_policy(domain, max_skew, relax_mask, n_hops, hops_out, blocker_reason_out, policy_out));
}

// rebalance sweep (SPEC.md 2.19, fp_rebalance.hip)
static fp_rebalance_opts rebalance_opts(const uint32_t *node_count, const uint32_t *domain, uint32_t max_skew,
                                        const uint32_t *relax_mask, uint32_t n_hops) {
    fp_rebalance_opts o;
    o.node_count = node_count; o.domain = domain; o.max_skew = max_skew; o.relax_mask = relax_mask; o.n_hops = n_hops;
    return o;
}

extern "C" int fp_dev_rebalance_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                      const uint32_t *victim_order, uint32_t n_var, uint32_t n_try,
                                      const uint32_t *max_moves, uint32_t strategy, uint32_t preferred_labels,
                                      const uint32_t *node_count, const uint32_t *domain, uint32_t max_skew,
                                      const uint32_t *relax_mask, uint32_t n_hops, uint32_t *assign_out,
                                      uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_rebalance_sweep_impl(c, cs, ns, assign, victim_order, n_var, n_try, max_moves, strategy,
                                                      preferred_labels,
                                                      rebalance_opts(node_count, domain, max_skew, relax_mask, n_hops),
                                                      assign_out, hops_out, reason_out, summary_out));
}

// no variant is nothing to do, whatever the tables are: found before them, as in shrink_host
extern "C" int fp_rebalance_sweep(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                  const uint32_t *victim_order, uint32_t n_var, uint32_t n_try, const uint32_t *max_moves,
                                  uint32_t strategy, uint32_t preferred_labels, const uint32_t *node_count,
                                  const uint32_t *domain, uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                  uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t C = cs->n, N = ns->n;
    if (N > FP_POLICY_MAX_NODES || n_var > 65535u || C > FP_SHRINK_MAX_CONTAINERS) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (n_var == 0) return FP_OK;
    if (C && (!fp_has_cont(cs) || !assign || !assign_out)) return FP_EINVAL;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    if ((n_try && !victim_order) || !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;
    if (!fp_below_or_none(assign, C, N) || !fp_below_or_none(victim_order, (size_t)n_var * n_try, C)) return FP_EINVAL;
    if (!domain || max_skew == 0u) domain = nullptr;  // otherwise domain is not read
    if (domain && !fp_domains_ok(domain, N)) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_rebalance_dev d;
    const int n = fp_rebalance_rows(cs, ns, assign, victim_order, n_var, n_try, max_moves, node_count, domain, assign_out,
                                    hops_out, reason_out, summary_out, &d, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = fp_dev_rebalance_sweep_impl(c, &d.cs, &d.ns, d.assign, d.victim_order, n_var, n_try, d.max_moves,
                                             strategy, preferred_labels,
                                             rebalance_opts(d.node_count, d.domain, max_skew, relax_mask, n_hops),
                                             d.assign_out, d.hops_out, d.reason_out, d.summary))
        return rc;
    return copy_back_all(c, rows, n);
}

// scale-out sweep (SPEC.md 2.12 and 2.18, fp_grow.hip): the two kernels differ, so each export keeps its impl.
// What both host exports ask of the pending containers and the templates, after their own FP_EOVERFLOW tests;
// t_max is host memory here, so a value above max_new is refused before anything is staged
static int grow_checks(const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask, uint32_t n_cand,
                       const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels, const uint32_t *t_max,
                       uint32_t max_new, const uint32_t *summary_out) {
    if (reason_mask && !reason) return FP_EINVAL;
    if (cs->n && !fp_has_cont(cs)) return FP_EINVAL;
    if (n_cand && (!t_cpu || !t_mem || !t_labels || !summary_out)) return FP_EINVAL;
    for (size_t k = 0; t_max && k < n_cand; ++k)
        if (t_max[k] > max_new) return FP_EINVAL;
    return FP_OK;
}

extern "C" int fp_dev_grow_sweep(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                 uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                                 const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out) {
    if (!c || !cs) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    return fp_dev_done(c, fp_dev_grow_sweep_impl(c, cs, reason, reason_mask, n_cand, t_cpu, t_mem, t_labels, t_max,
                                                 max_new, summary_out, assign_out));
}

extern "C" int fp_grow_sweep(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                             uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                             const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out) {
    if (!c || !cs) return FP_EINVAL;
    if (n_cand > 65535u || max_new > FP_GROW_MAX_NEW) return FP_EOVERFLOW;
    if (int rc = grow_checks(cs, reason, reason_mask, n_cand, t_cpu, t_mem, t_labels, t_max, max_new, summary_out))
        return rc;
    if (n_cand == 0) return FP_OK;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_grow_dev d;
    const int n = fp_grow_rows(cs, reason, reason_mask, n_cand, t_cpu, t_mem, t_labels, t_max, summary_out, assign_out,
                               &d, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    if (int rc = fp_dev_grow_sweep_impl(c, &d.cs, d.reason, reason_mask, n_cand, d.t_cpu, d.t_mem, d.t_labels, d.t_max,
                                        max_new, d.summary, d.assign_out))
        return rc;
    return copy_back_all(c, rows, n);
}

static fp_grow_policy grow_policy(const uint32_t *node_count, uint32_t strategy, uint32_t preferred_labels,
                                  const uint32_t *domain, const uint32_t *t_domain, uint32_t max_skew,
                                  const uint32_t *relax_mask, uint32_t n_hops, const uint32_t *quota,
                                  const uint32_t *quota_used, uint32_t *policy_out, uint8_t *hops_out,
                                  uint8_t *reason_out) {
    fp_grow_policy p;
    p.node_count = node_count; p.strategy = strategy; p.preferred = preferred_labels;
    p.domain = domain; p.t_domain = t_domain; p.max_skew = max_skew;
    p.relax_mask = relax_mask; p.n_hops = n_hops; p.quota = quota; p.quota_used = quota_used;
    p.policy_out = policy_out; p.hops_out = hops_out; p.reason_out = reason_out;
    return p;
}

extern "C" int fp_dev_grow_sweep_policy(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                        const fp_nodes *ns, const uint32_t *node_count, uint32_t n_cand,
                                        const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                                        const uint32_t *t_max, uint32_t max_new, uint32_t strategy,
                                        uint32_t preferred_labels, const uint32_t *domain, const uint32_t *t_domain,
                                        uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                        const uint32_t *quota, const uint32_t *quota_used, uint32_t *summary_out,
                                        uint32_t *policy_out, uint32_t *assign_out, uint8_t *hops_out,
                                        uint8_t *reason_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    FP_HIP(hipSetDevice(c->device));
    const fp_grow_policy pol = grow_policy(node_count, strategy, preferred_labels, domain, t_domain, max_skew, relax_mask,
                                           n_hops, quota, quota_used, policy_out, hops_out, reason_out);
    return fp_dev_done(c, fp_dev_grow_sweep_policy_impl(c, cs, reason, reason_mask, ns, n_cand, t_cpu, t_mem, t_labels,
                                                        t_max, max_new, summary_out, assign_out, pol));
}

extern "C" int fp_grow_sweep_policy(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                    const fp_nodes *ns, const uint32_t *node_count, uint32_t n_cand,
                                    const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                                    const uint32_t *t_max, uint32_t max_new, uint32_t strategy,
                                    uint32_t preferred_labels, const uint32_t *domain, const uint32_t *t_domain,
                                    uint32_t max_skew, const uint32_t *relax_mask, uint32_t n_hops,
                                    const uint32_t *quota, const uint32_t *quota_used, uint32_t *summary_out,
                                    uint32_t *policy_out, uint32_t *assign_out, uint8_t *hops_out, uint8_t *reason_out) {
    if (!c || !cs || !ns) return FP_EINVAL;
    const size_t N = ns->n;
    if (n_cand > 65535u || max_new > FP_GROW_MAX_NEW || N + max_new > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (int rc = grow_checks(cs, reason, reason_mask, n_cand, t_cpu, t_mem, t_labels, t_max, max_new, summary_out))
        return rc;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    if (!t_domain || max_skew == 0u) domain = t_domain = nullptr;  // otherwise neither domain array is read
    if (N && t_domain && !domain) return FP_EINVAL;
    if (t_domain && (!fp_domains_ok(t_domain, n_cand) || !fp_domains_ok(domain, N))) return FP_EINVAL;
    if (n_cand == 0) return FP_OK;
    FP_HIP(hipSetDevice(c->device));
    fp_host_err_scope es(c);
    if (es.rc) return es.rc;
    fp_row rows[FP_MAX_ROWS];
    fp_grow_dev d;
    fp_grow_policy_dev dp;
    const int n = fp_grow_policy_rows(cs, reason, reason_mask, ns, node_count, n_cand, t_cpu, t_mem, t_labels, t_max,
                                      domain, t_domain, summary_out, policy_out, assign_out, hops_out, reason_out, &d,
                                      &dp, rows);
    if (int rc = stage_rows(c, rows, n, false)) return rc;
    const fp_grow_policy pol = grow_policy(dp.node_count, strategy, preferred_labels, dp.domain, dp.t_domain, max_skew,
                                           relax_mask, n_hops, quota, quota_used, dp.policy_out, dp.hops_out,
                                           dp.reason_out);
    if (int rc = fp_dev_grow_sweep_policy_impl(c, &d.cs, d.reason, reason_mask, &dp.ns, n_cand, d.t_cpu, d.t_mem,
                                               d.t_labels, d.t_max, max_new, d.summary, d.assign_out, pol))
        return rc;
    return copy_back_all(c, rows, n);
}
