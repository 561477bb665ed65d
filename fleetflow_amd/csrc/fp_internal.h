// fp_internal.h -- shared internals of libfleetplace.so (HIP, gfx950 only).
#pragma once
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <vector>
#include "../../include/fleetplace.h"
#include "fp_rows.h"

#define FP_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return fp_hip_fail(e_);  \
    } while (0)

int fp_hip_fail(hipError_t e);

// A word that only gains bits (the batch OR words of the packed-record decision, fp_pipe_pk.h): the
// atomic only when this block adds a bit.  Most blocks find every bit set already, and atomics on one
// word serialise: config 4 issued 2 per scenario block from each of three kernels.
__device__ __forceinline__ void fp_or_new_bits(uint32_t *w, uint32_t bits) {
    if (bits & ~*(volatile uint32_t *)w) atomicOr(w, bits);
}

struct fp_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // kernel-side error words (a CSR index out of range, the pipeline's deadlock guard):
    // kernels atomicMax into the CURRENT word `d_err`.  fp_dev_* calls use the async word
    // (d_err_base[0]): sticky until fp_ctx_sync reports and clears it.  A host-pointer call
    // switches to its own word (d_err_base[HOST_ERR]) for its duration and reports only that
    // one, so an earlier async failure neither fails an unrelated synchronous call nor gets
    // cleared by it
    static constexpr uint32_t HOST_ERR = 32;
    uint32_t *d_err_base = nullptr;
    uint32_t *d_err = nullptr;
    // per-context options (fp_ctx_set_option; FP_OPT_AUTO = production default)
    int64_t opt[FP_OPT_COUNT];
    // recorded on the launch stream at the end of every fp_dev_* call: fp_ctx_set_stream
    // waits on it instead of synchronising a stream handle the caller may have destroyed
    hipEvent_t last_ev = nullptr;
    // device workspace: a bump arena reset at the start of every API call
    char *ws = nullptr;
    size_t ws_cap = 0, ws_top = 0;
    // host-API staging arena (device memory holding copies of host inputs)
    char *stage = nullptr;
    size_t stage_cap = 0, stage_top = 0;
    // pinned host bounce buffer for small read-backs
    uint64_t *h_small = nullptr;
    // pinned host staging of host-API results: copied to the caller only when every
    // kernel and every device-to-host copy succeeded (all-or-nothing)
    char *h_stage = nullptr;
    size_t h_stage_cap = 0;
    // pinned host staging of host-API inputs (one host-to-device copy per call); h_in_ev marks the
    // last copy out of it, waited on before the buffer is written again
    char *h_in = nullptr;
    size_t h_in_cap = 0;
    hipEvent_t h_in_ev = nullptr;
    // mapped pinned host memory of fp_plan_stage's one-launch path (fp_small.hip): the kernel reads
    // its inputs from and writes its results to it (h_map on the host, d_map on the device)
    char *h_map = nullptr;
    void *d_map = nullptr;
    size_t h_map_cap = 0;
    // fp_plan_stage's one-wave path for stages of <= 64 services (k_plan_tiny): its tagged result
    // words in mapped pinned host memory, and the tag of the last call (1..255)
    char *h_tiny = nullptr;
    void *d_tiny = nullptr;
    uint32_t tiny_tag = 0;
    // the asynchronous levelizer's work queues (fp_order.hip), kept between calls: a clean finish
    // leaves them empty, and the flag in their last 256 bytes tells the next call whether to refill
    void *lvl_q = nullptr;
    // the last placement's range words (CN_ORC.. of its workspace: OR cpu, OR mem, kernel path), read by
    // fp_ctx_place_path.  They live in the workspace arena: fp_ws_reset and fp_ws_reserve clear the
    // pointer, so it is never read after another call reused or freed the arena
    uint32_t *last_rng = nullptr;
    size_t lvl_q_cap = 0;
    // profiling
    bool profile = false;
    struct Rec { int kid; hipEvent_t a, b; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[FP_K_COUNT] = {0};
    uint64_t launches[FP_K_COUNT] = {0};
};

// arena helpers (return nullptr on failure; callers map to FP_ENOMEM)
void fp_ws_reset(fp_ctx *c);                 // also forgets last_rng, which points into the arena
int fp_ws_reserve(fp_ctx *c, size_t bytes);  // ensure capacity (may sync + realloc)
void *fp_ws_take(fp_ctx *c, size_t bytes);   // 256-B aligned slice
void fp_stage_reset(fp_ctx *c);
int fp_stage_reserve(fp_ctx *c, size_t bytes);
void *fp_stage_take(fp_ctx *c, size_t bytes);

// profiling brackets around a launch on ctx->stream
void fp_prof_begin(fp_ctx *c, int kid, hipEvent_t *a);
void fp_prof_end(fp_ctx *c, int kid, hipEvent_t a);

// synchronise the stream, read the current kernel error word and clear it (0 or -FP_E*)
int fp_take_err(fp_ctx *c);
// the end of every fp_dev_* entry point (fp_ctx.hip): records c->last_ev on the context's stream,
// which fp_ctx_set_stream waits on before a switch; returns rc (FP_EDEVICE if the record failed)
int fp_dev_done(fp_ctx *c, int rc);

// option value, or `dflt` when the option is FP_OPT_AUTO
static inline int64_t fp_opt(const fp_ctx *c, int k, int64_t dflt) {
    return (c && c->opt[k] != FP_OPT_AUTO) ? c->opt[k] : dflt;
}

// a host-pointer call's own kernel error word for its duration (fp_internal.h fp_ctx)
// The word is cleared on entry (stream-ordered), so an error a previous host call's kernels
// raised after that call exited early (a HIP failure, ENOMEM mid-call) is not reported here.
// Built after hipSetDevice(c->device) (the clear is issued on the context's device); `rc` is the
// clear's result, which the caller returns when it failed.
struct fp_host_err_scope {
    fp_ctx *c;
    int rc;
    explicit fp_host_err_scope(fp_ctx *cc) : c(cc) {
        c->d_err = c->d_err_base + fp_ctx::HOST_ERR;
        const hipError_t e = hipMemsetAsync(c->d_err, 0, 4, c->stream);
        rc = e == hipSuccess ? FP_OK : fp_hip_fail(e);
    }
    ~fp_host_err_scope() { c->d_err = c->d_err_base; }
};

// ---- what the entry points and the *_impl functions ask of their arguments (host only) ----
// t is an fp_containers, an fp_nodes or an fp_batch: its four container arrays / its five node arrays are there
template <class T>
static inline bool fp_has_cont(const T *t) { return t->cpu_m && t->mem_mib && t->req_labels && t->conflict; }
template <class T>
static inline bool fp_has_nodes(const T *t) {
    return t->cpu_free && t->mem_free && t->labels && t->conflict_used && t->schedulable;
}
// host arrays: every entry is below `bound` or FP_NONE; every domain id is below FP_SPREAD_MAX_DOMAINS
static inline bool fp_below_or_none(const uint32_t *x, size_t n, size_t bound) {
    for (size_t i = 0; i < n; ++i)
        if (x[i] >= bound && x[i] != FP_NONE) return false;
    return true;
}
static inline bool fp_domains_ok(const uint32_t *domain, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS) return false;
    return true;
}
// The sweeps' fallback chain: keep[h] = ~cum[h + 1] over the HOST array relax_mask; past n_hops the last one
// repeats (k_policy's keep), and without a chain (`fb` false) every keep is ~0
static inline void fp_keep_masks(const uint32_t *relax_mask, uint32_t n_hops, bool fb, uint32_t *keep) {
    uint32_t cum = 0;
    for (uint32_t h = 0; h < FP_FALLBACK_MAX_HOPS; ++h) {
        if (fb && h < n_hops) cum |= relax_mask[h];
        keep[h] = ~cum;
    }
}
// f(SP, FB) with the two host flags as std::bool_constant values: the sweeps' kernels are templates over them
template <class F>
static inline void fp_with_flags(bool sp, bool fb, F f) {
    if (sp && fb) f(std::true_type(), std::true_type());
    else if (sp) f(std::true_type(), std::false_type());
    else if (fb) f(std::false_type(), std::true_type());
    else f(std::false_type(), std::false_type());
}

static inline uint32_t fp_bitwidth(uint64_t v) {
    uint32_t b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// blocks of `block` threads for a grid-stride loop over n items
static inline unsigned grid_for(size_t n, unsigned block) {
    size_t g = (n + block - 1) / block;
    if (g > 65535u * 4) g = 65535u * 4;
    return (unsigned)(g ? g : 1);
}

// The radix FFD order (fp_ffd_order.hip): key (~cpu << 32 | ~mem), value = the index in the scenario, and a
// stable rocprim radix sort over all 64 bits -- device-wide for one scenario, segmented for several -- give
// (cpu desc, mem desc, index asc) per scenario.  S * C < 2^32, C > 0.
struct fp_ffd_order {
    size_t bytes;      // workspace fp_ffd_order_run takes: 24 bytes per container, the offsets, the scratch
    size_t tmp_bytes;  // the sort's scratch, at least what the caller asked for
    // filled by fp_ffd_order_run: the sorted keys are in keys_out and the order in `order`; keys_in and vals_in
    // are the sort's inputs, free for the caller afterwards, and so is tmp
    uint64_t *keys_in, *keys_out;
    uint32_t *vals_in, *order;
    void *tmp;
};
// min_tmp: scratch bytes the caller wants for a sort of its own through the same buffers (0: none)
int fp_ffd_order_size(fp_ctx *c, uint32_t S, uint32_t C, size_t min_tmp, fp_ffd_order *fo);
// takes fo->bytes from the workspace and launches the key kernel, the offsets kernel (S > 1) and the sort.
// rng: null, or [2] words that receive the OR of every cpu / mem value (one atomic per block and word)
int fp_ffd_order_run(fp_ctx *c, uint32_t S, uint32_t C, const uint32_t *cpu, const uint32_t *mem, uint32_t *rng,
                     fp_ffd_order *fo);

// ---- entry points shared between translation units ----
int fp_dev_place_batch_impl(fp_ctx *c, const fp_batch *b);
int fp_dev_levelize_impl(fp_ctx *c, const fp_graph *g, uint32_t *level, uint32_t *order,
                         uint32_t *n_cycle_dev);
int fp_dev_legacy_order_impl(fp_ctx *c, const fp_graph *g, uint32_t *perm);
int fp_dev_feasibility_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns,
                            uint32_t *first, uint32_t *count, uint64_t *bitmap);
int fp_dev_feasibility_batch_impl(fp_ctx *c, const fp_batch *b, uint32_t *first, uint32_t *count);
// rejection diagnosis (fp_explain.hip, SPEC.md 2.9); every pointer is device memory
int fp_dev_explain_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *sel, uint32_t n_sel,
                        uint32_t ignore_labels, uint32_t *rows);
int fp_dev_explain_batch_impl(fp_ctx *c, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                              uint32_t *hist);
// scored placement (fp_policy.hip, SPEC.md 2.6 to 2.10; fp_policy_opts: fp_rows.h)
// every pointer is device memory
int fp_dev_place_batch_policy_impl(fp_ctx *c, const fp_batch *b, const fp_policy_opts &o);

// drain what-if sweep (fp_drain.hip, SPEC.md 2.11); every pointer is device memory.  group and assign values
// out of range are found on the device (FP_EINVAL in the context's error word, nothing written)
// The sweep under the policy (SPEC.md 2.15): domain [N] device memory, relax_mask [n_hops] HOST memory (read
// during the call, like the scalars); hops_out [C] and policy_out [n_cand][FP_DRAIN_POLICY_WORDS] device
// memory, nullable.  All null / zero (the default) is 2.11.  n_hops above FP_FALLBACK_MAX_HOPS is FP_EINVAL at
// once; a domain id of 64 or more under max_skew != 0 is found on the device with the group and assign values
struct fp_drain_policy {
    const uint32_t *domain = nullptr;
    uint32_t max_skew = 0;
    const uint32_t *relax_mask = nullptr;
    uint32_t n_hops = 0;
    uint8_t *hops_out = nullptr;
    uint32_t *policy_out = nullptr;
};
int fp_dev_drain_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                            const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred,
                            const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                            uint32_t *summary_out, const fp_drain_policy &pol = fp_drain_policy());

// what a scale-in sweep under the policy has besides the sweep's own arguments (SPEC.md 2.17).  Not ABI: the
// exports of fp_ctx.hip fill it in.  domain and the three results are device memory, relax_mask a HOST array
struct fp_shrink_policy {
    const uint32_t *domain = nullptr;      // [N]; null or max_skew == 0: no constraint
    uint32_t max_skew = 0;
    const uint32_t *relax_mask = nullptr;  // [n_hops]; null or n_hops == 0: no chain
    uint32_t n_hops = 0;
    uint8_t *hops_out = nullptr;           // [n_var][C] or null
    uint8_t *blocker_reason_out = nullptr; // [n_var][N] or null
    uint32_t *policy_out = nullptr;        // [n_var][FP_SHRINK_POLICY_WORDS] or null
};
// scale-in sweep (fp_shrink.hip, SPEC.md 2.16); every pointer is device memory.  assign and try_order values out
// of range are found on the device (FP_EINVAL in the context's error word, nothing written).  pol (SPEC.md 2.17):
// the spread constraint, the fallback chain and the three further results; domain and the results are device
// memory, relax_mask a host array
// the most containers a call takes: the scan's positions, rounded up to a whole step, stay below 2^31
constexpr uint32_t FP_SHRINK_MAX_CONTAINERS = 0x7FFF0000u;
int fp_dev_shrink_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                             const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                             uint32_t preferred, const uint32_t *node_count, uint32_t *assign_out, uint8_t *state_out,
                             uint32_t *blocker_out, uint32_t *summary_out, const fp_shrink_policy &pol = fp_shrink_policy());

// what a rebalance sweep is held to (SPEC.md 2.19).  Not ABI: the exports of fp_ctx.hip fill it in.  node_count
// and domain are device memory, relax_mask a HOST array
struct fp_rebalance_opts {
    const uint32_t *node_count = nullptr;  // [N]; null: derived from assign
    const uint32_t *domain = nullptr;      // [N]; null or max_skew == 0: nothing is heavy
    uint32_t max_skew = 0;
    const uint32_t *relax_mask = nullptr;  // [n_hops]; null or n_hops == 0: no chain
    uint32_t n_hops = 0;
};
// rebalance sweep (fp_rebalance.hip, SPEC.md 2.19); every pointer but o.relax_mask is device memory.  assign,
// victim_order and domain values out of range are found on the device (FP_EINVAL in the context's error word,
// nothing written).  hops_out and reason_out are nullable
int fp_dev_rebalance_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                const uint32_t *victim_order, uint32_t n_var, uint32_t n_try, const uint32_t *max_moves,
                                uint32_t strategy, uint32_t preferred, const fp_rebalance_opts &o, uint32_t *assign_out,
                                uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out);

// scale-out sweep (fp_grow.hip, SPEC.md 2.12); every pointer is device memory, max_new a host value.  A t_max
// value above max_new is found on the device (FP_EINVAL in the context's error word, nothing written)
int fp_dev_grow_sweep_impl(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                           uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                           const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out);

// what a scale-out sweep under the policy has besides the sweep's own arguments (SPEC.md 2.18).  Not ABI: the
// exports of fp_ctx.hip fill it in.  node_count, the domains and the three results are device memory; relax_mask,
// quota and quota_used are HOST arrays, read during the call
struct fp_grow_policy {
    const uint32_t *node_count = nullptr;  // [N] or null (zeros)
    uint32_t strategy = 0, preferred = 0;
    const uint32_t *domain = nullptr;      // [N]
    const uint32_t *t_domain = nullptr;    // [n_cand]; null or max_skew == 0: no constraint
    uint32_t max_skew = 0;
    const uint32_t *relax_mask = nullptr;  // [n_hops]; null or n_hops == 0: no chain
    uint32_t n_hops = 0;
    const uint32_t *quota = nullptr;       // [3] or null: no quota
    const uint32_t *quota_used = nullptr;  // [3] or null (zeros); read only
    uint32_t *policy_out = nullptr;        // [n_cand][FP_GROW_POLICY_WORDS] or null
    uint8_t *hops_out = nullptr;           // [n_cand][C] or null
    uint8_t *reason_out = nullptr;         // [n_cand][C] or null
};
// the scale-out sweep under the policy (fp_grow.hip, SPEC.md 2.18): ns is the live table (device memory, read
// only).  A t_max value above max_new and, under a constraint, a domain or t_domain value of 64 or more are found
// on the device (FP_EINVAL in the context's error word, nothing written)
int fp_dev_grow_sweep_policy_impl(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                  const fp_nodes *ns, uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem,
                                  const uint32_t *t_labels, const uint32_t *t_max, uint32_t max_new,
                                  uint32_t *summary_out, uint32_t *assign_out, const fp_grow_policy &pol);

// re-planning a running stage (fp_replan.hip, SPEC.md 2.13); every pointer is device memory.  Of `o` the call
// reads strategy, preferred and node_count.  A strategy that is no fp_strategy value and a prev value out of
// range are found on the device (FP_EINVAL in the context's error word, nothing written)
int fp_dev_replan_batch_impl(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o,
                             uint8_t *change_out, uint32_t *summary_out);
// the same under the policy's guarantees (fp_replan_policy.hip, SPEC.md 2.14): of `o` the call reads every field.
// A domain id out of range in a constrained scenario and an n_hops above FP_FALLBACK_MAX_HOPS are found on the
// device with the strategy and prev values.  Without a guarantee it is fp_dev_replan_batch_impl
int fp_dev_replan_batch_policy_impl(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o,
                                    uint8_t *change_out, uint32_t *summary_out);

// tile-pipeline FFD (fp_pipe.hip)
bool fp_pipe_plan(const fp_ctx *c, uint32_t S, uint32_t N, uint32_t *G_out, uint32_t *W_out, uint32_t *B_out,
                  size_t *lds_out);
int fp_place_geometry_impl(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N, uint32_t *out);
size_t fp_pipe_ws_bytes(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N);
int fp_place_ws_bytes_impl(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N, uint64_t *bytes);
// bucket thresholds of the candidate masks: K ascending values, T[0] = 0
constexpr int FP_BUCKETS = 32;
// geometric from lo to hi (host and device: fp_place.hip k_thresholds)
__host__ __device__ inline void fp_thresholds(uint32_t lo, uint32_t hi, uint32_t *T) {
    T[0] = 0;
    if (lo == 0) lo = 1;
    if (hi < lo) hi = lo;
    const double r = pow((double)hi / (double)lo, 1.0 / (double)(FP_BUCKETS - 2));
    double v = (double)lo;
    for (int k = 1; k < FP_BUCKETS; ++k) {
        uint32_t x = k == FP_BUCKETS - 1 ? hi : (uint32_t)ceil(v);
        if (x < T[k - 1]) x = T[k - 1];
        if (x > hi) x = hi;
        T[k] = x;
        v *= r;
    }
}
// the FFD-sorted SoA [S][C] the pipeline streams (fp_pipe.hip)
struct fp_pipe_soa {
    uint32_t *s_cpu, *s_mem, *s_req, *s_conf, *s_idx;
    // set by the fused sort (fp_place.hip): k_node_summary ran ahead of it (summ: its rows, null without the
    // screen) and the sort's last phase wrote s_req, s_conf and the skip bits, so fp_pipe_launch runs neither
    uint32_t *summ = nullptr;
    bool payload_done = false;
    // set by the fused sort's prepack mode: the per-scenario header [S][4] = {sc_c, sc_m, packs_s, 0}.  A
    // scenario with packs_s = 1 has ONE demand row, s_w = packed (cpu, mem) | skip << 31, in its s_cpu row, and
    // nothing in its s_mem / s_idx rows (fp_pipe_launch: k_unpack_rows, the prepacked-input kernel)
    uint32_t *pkhdr = nullptr;
};
int fp_pipe_soa_take(fp_ctx *c, size_t SC, fp_pipe_soa *soa);
// Prepack mode of the fused sort for S x C x N on this context: the launch will be the 4096-scenario pair
// (big / its packed no-mask twin) and FP_OPT_PREPACK allows it.  The same test decides in fp_pipe_launch
// which packed kernel runs, so the caller sets fp_pipe_soa::pkhdr exactly when this holds.
bool fp_pipe_prepack(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N);
// The shifts of packed (cpu, mem) records for the OR words of a value set, and whether the set packs
// (fp_pipe_pk.h): k_ffd_pipe's rule for the batch, k_scen_sort's for a scenario
__host__ __device__ static inline bool fp_pk_shifts(uint32_t orc, uint32_t orm, uint32_t *sc_c, uint32_t *sc_m) {
    *sc_c = orc ? (uint32_t)__builtin_ctz(orc) : 0u;
    *sc_m = orm ? (uint32_t)__builtin_ctz(orm) : 0u;
    return (orc >> *sc_c) <= 0x7FFFu && (orm >> *sc_m) <= 0x7FFFu;
}
// 1 when the position word carries the bucket indices (bits 21-30)
uint32_t fp_pipe_kpack(const fp_ctx *c, uint32_t C);
// ready: the per-scenario LDS sort already wrote order, s_cpu, s_mem and s_idx (only the
// req / conf / CYCLE gather remains); null: gather everything from order + sorted keys.
// thr: the pipeline's bucket thresholds in device memory ([FP_BUCKETS] cpu, then mem)
// rng: [2] the OR of every container cpu / mem value of the batch (the sort kernels wrote it); the
// pipeline adds the nodes' and runs the packed kernel when the values pack (null: u32 kernels only)
// the stage-2 screen's summary rows ([S][4] from the workspace into *summ; null without nodes or the screen)
// and the nodes' share of rng, enqueued on the context's stream
int fp_pipe_node_summary(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N, const fp_batch *b, uint32_t *rng,
                         uint32_t **summ);
// the largest C whose payload gather runs through LDS chunks (0: FP_OPT_PAYLOAD_LDS = 0)
uint32_t fp_pipe_payload_lds_max_c(const fp_ctx *c);
int fp_pipe_launch(fp_ctx *c, uint32_t S, uint32_t C, uint32_t N, uint32_t scen_base, const uint32_t *order,
                   const void *skeys, uint32_t key_bytes, uint32_t mbits, uint64_t cmax, uint64_t mmax,
                   const uint32_t *cval, const uint32_t *mval, const fp_batch *b, const uint32_t *thr,
                   const fp_pipe_soa *ready, uint32_t *rng);

// ---- device helpers ----
namespace fpd {

constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ull;
constexpr uint64_t TAG_CONT = 0xC0C0C0C0C0C0C0C0ull;
constexpr uint64_t TAG_NODE = 0x5E5E5E5E5E5E5E5Eull;

// SPEC.md 3.1: draw(seed, k) = (k+1)-th SplitMix64 output from state `seed`.
__host__ __device__ inline uint64_t draw(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * GAMMA;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t scenario_seed(uint64_t seed, uint32_t s) {
    return seed ^ ((uint64_t)s * GAMMA);
}

// Single node-fit predicate (SPEC.md 2.3); sched handled by callers.
__device__ __forceinline__ bool fits(uint32_t cpu, uint32_t mem, uint32_t req, uint32_t conf,
                                     uint32_t cf, uint32_t mf, uint32_t lab, uint32_t cu) {
    return (cf >= cpu) & (mf >= mem) & ((lab & req) == req) & ((cu & conf) == 0u);
}

__device__ __forceinline__ uint64_t pack_cost(uint32_t rej, uint32_t used, uint32_t id) {
    uint64_t r = rej > 0xFFFFFFu ? 0xFFFFFFu : rej;
    uint64_t u = used > 0xFFFFFFu ? 0xFFFFFFu : used;
    return (r << 40) | (u << 16) | (uint64_t)(id & 0xFFFFu);
}

}  // namespace fpd
