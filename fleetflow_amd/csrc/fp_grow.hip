// fp_grow.hip -- the scale-out sweep (SPEC.md 2.12; under the policy, 2.18): for every candidate (one server template) the new servers
// of that template the pending containers of a plan need, every candidate from the same pending list.
// One workgroup owns one candidate; the blocks share only the read-only list.
//
// Per fp_dev_grow_sweep call (asynchronous, nothing is read back):
//   1. the pending list, once per call (grow_front): the radix FFD order (fp_ffd_order.hip) is the 2.3 order of all
//                       containers (cpu desc, mem desc, index asc); a stable rocprim select keeps the
//                       containers whose reason is in reason_mask (reason_mask == 0: the order itself) and
//                       leaves their number in the workspace; k_grow_records gathers them into the dense SoA
//                       (cpu, mem, req, conflict, index) every block streams.  The records live in the two key
//                       buffers of the sort, which are free by then
//   2. k_grow_check   : sets the call's "bad" word for a t_max[k] above max_new, and FP_EINVAL in the context's
//                       error word; every later kernel that writes an output returns on the word first
//   3. k_grow_init    : assign_out = FP_NONE (only when the caller asked for assign_out)
//   4. k_grow_sweep<BLK,K>: one workgroup per candidate.  The nodes are identical at the start, so the state
//                       is three words a node (cpu_free, mem_free, conflict_used) and the labels one uniform
//                       word; thread t owns nodes t + BLK * j, row j a fixed register up to 4 rows and a
//                       register addressed by a scalar index above.  Records are
//                       loaded 64 per wave a chunk ahead and broadcast with v_readlane.  A container the
//                       template can never take (UNPLACEABLE) is decided on the broadcast record alone.  For
//                       the others only nodes [0, opened] can be feasible (the prefix property): a wave scans
//                       its share of them row by row, a ballot and its first set bit give the wave's lowest
//                       feasible node, and one parity-double-buffered LDS word per wave and one barrier give
//                       the block's.  The owner updates its registers; thread 0 stores assign_out.
//
// Under the policy (SPEC.md 2.18, fp_dev_grow_sweep_policy) the same front feeds k_grow_policy<BLK,K,SP,FB>: the
// live node table in front of the template's servers, and every pending container's (hop, key) argmin over the
// combined table, under the strategy, the preferred labels, the spread constraint (SP), the fallback chain (FB)
// and the quota.  The kernel is described where it stands.
//
// No device-wide synchronisation and no spin waits: the kernels cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>
#include <rocprim/device/device_select.hpp>

namespace {

using fpd::bcast;

// behind a memset of *bad on the stream; only ever sets it
__global__ __launch_bounds__(256) void k_grow_check(const uint32_t *__restrict__ t_max, uint32_t n_cand,
                                                    uint32_t max_new, uint32_t *__restrict__ bad,
                                                    uint32_t *__restrict__ err) {
    bool b = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cand; i += (size_t)gridDim.x * blockDim.x)
        b |= t_max[i] > max_new;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// the pending predicate over container indices (2.9's convention: bit r of the mask selects reason r)
struct GrowPending {
    const uint8_t *reason;
    uint32_t mask;
    __host__ __device__ bool operator()(const uint32_t &o) const {
        const uint32_t r = reason[o];
        return r < 32u && ((mask >> r) & 1u);
    }
};

__global__ void k_grow_count(uint32_t *__restrict__ cnt, uint32_t v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = v;
}

// the records of sel[0 .. *cnt) (container indices in visiting order), dense
__global__ __launch_bounds__(256) void k_grow_records(const uint32_t *__restrict__ sel, const uint32_t *__restrict__ cnt,
                                                      uint32_t C, const uint32_t *__restrict__ cpu,
                                                      const uint32_t *__restrict__ mem, const uint32_t *__restrict__ req,
                                                      const uint32_t *__restrict__ conf, uint32_t *__restrict__ r_cpu,
                                                      uint32_t *__restrict__ r_mem, uint32_t *__restrict__ r_req,
                                                      uint32_t *__restrict__ r_conf, uint32_t *__restrict__ r_idx) {
    const uint32_t n = *cnt < C ? *cnt : C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t o = sel[i];
        if (o >= C) continue;  // never: sel holds values of the order
        r_cpu[i] = cpu[o];
        r_mem[i] = mem[o];
        r_req[i] = req[o];
        r_conf[i] = conf[o];
        r_idx[i] = o;
    }
}

__global__ __launch_bounds__(256) void k_grow_init(uint32_t *__restrict__ assign_out, size_t n,
                                                   const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        assign_out[i] = FP_NONE;
}

struct GrowArgs {
    uint32_t C, max_new;
    const uint32_t *cnt;                                   // the number pending
    const uint32_t *r_cpu, *r_mem, *r_req, *r_conf, *r_idx;  // [C] the pending records in visiting order
    const uint32_t *t_cpu, *t_mem, *t_lab;                 // [n_cand]
    const uint32_t *t_max;                                 // [n_cand] or null (max_new)
    uint32_t *summary;                                     // [n_cand][FP_GROW_WORDS]
    uint32_t *assign_out;                                  // [n_cand][C] or null
    const uint32_t *bad;
};

template <int BLK, int K>
__global__ __launch_bounds__(BLK) void k_grow_sweep(const GrowArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    static_assert(K <= 32, "a row vector is at most 32 registers");
    constexpr uint32_t NW = BLK / 64;
    if (*a.bad) return;  // a t_max above max_new somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));  // the wave's number, in a scalar register
    const uint32_t k = blockIdx.x;
    const uint32_t np = *a.cnt < a.C ? *a.cnt : a.C;  // uniform
    const uint32_t tc = a.t_cpu[k], tm = a.t_mem[k], tl = a.t_lab[k];
    uint32_t M = a.t_max ? a.t_max[k] : a.max_new;  // this candidate's nodes are [0, M)
    if (M > a.max_new) M = a.max_new;               // (checked: *bad) the launch holds max_new nodes, never more
    if (M > (uint32_t)(BLK * K)) M = (uint32_t)(BLK * K);

    // ---- the new servers, in registers: all alike until something lands on them ----
    // one register a row and word, as vectors: with more than 4 rows row j is addressed by a scalar index
    // (s_set_gpr_idx), in the scan loop and in the winner's update alike
    using row_t = uint32_t __attribute__((ext_vector_type(K)));
    row_t cf = tc, mf = tm, cu = 0u;

    __shared__ uint32_t slot[2][NW];
    uint32_t par = 0;
    // the same in every thread
    uint32_t opened = 0, placed_n = 0, unpl_n = 0, capped_n = 0, first = FP_NONE;
    uint32_t *asg = a.assign_out ? a.assign_out + (size_t)k * a.C : nullptr;

    // ---- pending records, 64 per chunk, one chunk ahead ----
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;
    auto load = [&](uint32_t i) {
        const bool in = i < np;
        r_cpu = in ? a.r_cpu[i] : 0u;
        r_mem = in ? a.r_mem[i] : 0u;
        r_req = in ? a.r_req[i] : 0u;
        r_conf = in ? a.r_conf[i] : 0u;
        r_idx = in ? a.r_idx[i] : 0u;
    };
    load(lane);

    for (uint32_t i0 = 0; i0 < np; i0 += 64u) {
        const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx;
        if (i0 + 64u < np) load(i0 + 64u + lane);
        const uint32_t nu = np - i0 < 64u ? np - i0 : 64u;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t idx = bcast(c_idx, u);
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // no number of this template helps: decided on the record, the same in every wave
            const bool unpl = (cpu > tc) | (mem > tm) | ((tl & req) != req);
            uint32_t n = FP_NONE;
            if (!unpl && M != 0u) {
                // ---- the lowest feasible node among [0, lim): the opened ones and the next empty one ----
                const uint32_t lim = opened < M ? opened + 1u : M;  // uniform
                uint32_t mine = FP_NONE;                            // this wave's, uniform in the wave
                if constexpr (K <= 4) {
                    // few rows: unrolled, every row a fixed register
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const uint32_t wbase = (uint32_t)BLK * j + w * 64u;  // this wave's lowest node of row j
                        if (mine == FP_NONE && wbase < lim) {
                            const bool ok =
                                wbase + lane < lim && (cf[j] >= cpu) & (mf[j] >= mem) & ((cu[j] & conf) == 0u);
                            const uint64_t bal = __builtin_amdgcn_ballot_w64(ok);
                            if (bal) mine = wbase + (uint32_t)__builtin_ctzll(bal);
                        }
                    }
                } else {
                    // a real loop: the row registers are addressed by the scalar j, and the loop ends at the
                    // first row that has a feasible node or lies above the prefix
                    for (uint32_t j = 0; j < (uint32_t)K; ++j) {
                        const uint32_t wbase = (uint32_t)BLK * j + w * 64u;
                        if (wbase >= lim) break;  // uniform: the rows above hold no candidate
                        const bool ok =
                            wbase + lane < lim && (cf[j] >= cpu) & (mf[j] >= mem) & ((cu[j] & conf) == 0u);
                        const uint64_t bal = __builtin_amdgcn_ballot_w64(ok);
                        if (bal) {
                            mine = wbase + (uint32_t)__builtin_ctzll(bal);
                            break;
                        }
                    }
                }
                if (NW > 1) {
                    if (lane == 0) slot[par][w] = mine;
                    __syncthreads();
#pragma unroll
                    for (uint32_t ww = 0; ww < NW; ++ww) {
                        const uint32_t s = slot[par][ww];
                        n = s < n ? s : n;
                    }
                    n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
                    par ^= 1u;
                } else {
                    n = mine;
                }
            }

            // ---- the winner ----
            if (n != FP_NONE) {
                // the winner's row J is uniform.  Few rows: a select a row and word; many: the owner updates
                // registers J of the three vectors in place (indirect register addressing)
                const uint32_t J = n / (uint32_t)BLK;
                const bool owner = (n & (uint32_t)(BLK - 1)) == t;
                if constexpr (K <= 4) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((uint32_t)j == J && owner) {
                            cf[j] -= cpu;
                            mf[j] -= mem;
                            cu[j] |= conf;
                        }
                    }
                } else if (owner) {
                    cf[J] -= cpu;
                    mf[J] -= mem;
                    cu[J] |= conf;
                }
                opened += n == opened ? 1u : 0u;  // n <= opened: the prefix property
                ++placed_n;
                if (asg && t == 0 && idx < a.C) asg[idx] = n;
            } else {
                if (first == FP_NONE) first = idx;
                if (unpl) ++unpl_n;
                else ++capped_n;
            }
        }
    }

    // ---- the candidate's row: what is left on the opened servers ----
    uint32_t lc = 0, lm = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool in = (uint32_t)BLK * j + t < opened;
        lc += in ? cf[j] : 0u;  // u32, wraps
        lm += in ? mf[j] : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lc += (uint32_t)__shfl_xor((int)lc, o);
        lm += (uint32_t)__shfl_xor((int)lm, o);
    }
    if (NW > 1) {
        __shared__ uint32_t lcw[NW], lmw[NW];
        if (lane == 0) {
            lcw[w] = lc;
            lmw[w] = lm;
        }
        __syncthreads();
        lc = 0;
        lm = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < NW; ++ww) {
            lc += lcw[ww];
            lm += lmw[ww];
        }
    }
    if (t == 0) {
        uint32_t *row = a.summary + (size_t)k * FP_GROW_WORDS;
        row[FP_GROW_PENDING] = np;
        row[FP_GROW_PLACED] = placed_n;
        row[FP_GROW_OPENED] = opened;
        row[FP_GROW_UNPLACEABLE] = unpl_n;
        row[FP_GROW_CAPPED] = capped_n;
        row[FP_GROW_LEFT_CPU] = lc;
        row[FP_GROW_LEFT_MEM] = lm;
        row[FP_GROW_FIRST_UNPLACED] = first;
    }
}

// the geometry follows max_new alone, a host value: nothing is read back to choose it
void launch_grow(const GrowArgs &a, uint32_t n_cand, hipStream_t st) {
    const uint32_t m = a.max_new;
    if (m <= 64) k_grow_sweep<64, 1><<<n_cand, 64, 0, st>>>(a);
    else if (m <= 1024) k_grow_sweep<256, 4><<<n_cand, 256, 0, st>>>(a);
    else if (m <= 2048) k_grow_sweep<256, 8><<<n_cand, 256, 0, st>>>(a);
    else if (m <= 4096) k_grow_sweep<256, 16><<<n_cand, 256, 0, st>>>(a);
    else k_grow_sweep<256, 32><<<n_cand, 256, 0, st>>>(a);
}

// The pending list of one call, shared by the sweep and the sweep under the policy: the workspace's bad word
// (zeroed on the stream) and count, and the dense records in visiting order.  Nothing a caller sees is written.
struct GrowFront {
    uint32_t *bad, *cnt;
    const uint32_t *r_cpu, *r_mem, *r_req, *r_conf, *r_idx;  // null with C == 0
};
int grow_front(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask, GrowFront *f) {
    const uint32_t C = cs->n;
    hipStream_t st = c->stream;
    size_t tmp2 = 0;
    fp_ffd_order fo = {};
    const GrowPending pred{reason, reason_mask};
    if (C) {
        if (reason_mask)
            FP_HIP(rocprim::select(nullptr, tmp2, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)C,
                                   pred, st));
        if (int rc = fp_ffd_order_size(c, 1, C, tmp2, &fo)) return rc;
    }
    // the bad word, the count, the FFD order (whose buffers hold the list afterwards), the records' indices
    if (int rc = fp_ws_reserve(c, 2 * 256 + fo.bytes + fp_align256((size_t)C * 4))) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    uint32_t *cnt = (uint32_t *)fp_ws_take(c, 4);
    if (!bad || !cnt) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    *f = {};
    f->bad = bad; f->cnt = cnt;
    if (C == 0) {
        k_grow_count<<<1, 64, 0, st>>>(cnt, 0u);
        FP_HIP(hipGetLastError());
        return FP_OK;
    }
    // ---- the pending list: 2.3 order, the stable selection, the records ----
    uint32_t *r_idx = (uint32_t *)fp_ws_take(c, (size_t)C * 4);
    if (!r_idx) return FP_ENOMEM;
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_SORT, &ev);
    if (int rc = fp_ffd_order_run(c, 1, C, cs->cpu_m, cs->mem_mib, nullptr, &fo)) return rc;
    const uint32_t *sel = fo.order;
    if (reason_mask) {
        size_t t = fo.tmp_bytes;
        FP_HIP(rocprim::select(fo.tmp, t, fo.order, fo.vals_in, cnt, (size_t)C, pred, st));
        sel = fo.vals_in;
    } else {
        k_grow_count<<<1, 64, 0, st>>>(cnt, C);
        FP_HIP(hipGetLastError());
    }
    // the sort's key buffers (8 bytes per container each) are free: two record arrays in each
    uint32_t *ka = (uint32_t *)fo.keys_in, *kb = (uint32_t *)fo.keys_out;
    k_grow_records<<<grid_for(C, 256), 256, 0, st>>>(sel, cnt, C, cs->cpu_m, cs->mem_mib, cs->req_labels,
                                                     cs->conflict, ka, ka + C, kb, kb + C, r_idx);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_SORT, ev);
    f->r_cpu = ka; f->r_mem = ka + C; f->r_req = kb; f->r_conf = kb + C; f->r_idx = r_idx;
    return FP_OK;
}

// ---- the sweep under the policy (SPEC.md 2.18) ----

using fpd::DOM_BITS;
using fpd::KEY_HOP_SHIFT;
using fpd::KEY_NODE_BITS;
using fpd::KEY_NODE_BITS_FB;
using fpd::KEY_NONE;
using fpd::KEY_SKEW;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min32;
using fpd::wave_min64;
static_assert((1u << DOM_BITS) == FP_SPREAD_MAX_DOMAINS && FP_SPREAD_MAX_DOMAINS == 64, "one domain per lane");
static_assert((uint64_t)FP_POLICY_MAX_NODES << DOM_BITS <= (1ull << KEY_NODE_BITS_FB), "node << 6 | domain fits the node field");
static_assert(FP_FALLBACK_MAX_HOPS == 4 && FP_FALLBACK_MAX_HOPS < (1u << (64 - KEY_HOP_SHIFT)), "the hop fits its field");
static_assert(FP_QUOTA_DIMS == 3, "three quota lanes");

// behind a memset of *bad on the stream; only ever sets it.  t_max: null or [n_cand].  domain / t_dom: null, or
// (a call under a spread constraint) the [N] and [n_cand] domain ids, every one of which has to be below
// FP_SPREAD_MAX_DOMAINS, whatever t_max[k] is
__global__ __launch_bounds__(256) void k_grow_policy_check(const uint32_t *__restrict__ t_max, uint32_t n_cand,
                                                           uint32_t max_new, const uint32_t *__restrict__ domain,
                                                           uint32_t N, const uint32_t *__restrict__ t_dom,
                                                           uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cand; i += stride)
        b |= (t_max && t_max[i] > max_new) || (t_dom && t_dom[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        b |= domain && domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// what every container that is not pending, or not placed, keeps: assign FP_NONE, hop 0, reason 0 (each nullable)
__global__ __launch_bounds__(256) void k_grow_policy_init(uint32_t *__restrict__ assign_out, uint8_t *__restrict__ hops_out,
                                                          uint8_t *__restrict__ reason_out, size_t n,
                                                          const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (assign_out) assign_out[i] = FP_NONE;
        if (hops_out) hops_out[i] = 0;
        if (reason_out) reason_out[i] = (uint8_t)FP_REASON_OK;
    }
}

struct GrowPolicyArgs {
    uint32_t C, N, max_new, strategy, preferred;
    const uint32_t *cnt;                                     // the number pending
    const uint32_t *r_cpu, *r_mem, *r_req, *r_conf, *r_idx;  // [C] the pending records in visiting order
    const uint32_t *cpu_free, *mem_free, *conflict_used;     // [N] the live table: read only
    const uint32_t *labels;                                  // [N]
    const uint8_t *schedulable;                              // [N]
    const uint32_t *node_count;                              // [N] or null (zeros)
    const uint32_t *t_cpu, *t_mem, *t_lab;                   // [n_cand]
    const uint32_t *t_max;                                   // [n_cand] or null (max_new)
    const uint32_t *domain, *t_dom;                          // [N], [n_cand]; read by <.., true, ..>
    uint32_t max_skew;                                       // not 0 in <.., true, ..>
    uint32_t keep[FP_FALLBACK_MAX_HOPS];                     // ~cum[h + 1]; entries past n_hops repeat the last one
    uint32_t qrem[FP_QUOTA_DIMS];                            // cap - used on entry (0 when used is above the cap)
    uint32_t qlim;                                           // bit d: dimension d has a cap
    uint32_t *summary;                                       // [n_cand][FP_GROW_WORDS]
    uint32_t *policy;                                        // [n_cand][FP_GROW_POLICY_WORDS] or null
    uint32_t *assign_out;                                    // [n_cand][C] or null
    uint8_t *hops, *reason;                                  // [n_cand][C] or null
    const uint32_t *bad;
};

// One workgroup per candidate, built the way k_drain_sweep<.., SP, FB> is (fp_drain.hip; the argument for one
// barrier per container is in fp_policy.hip's header).  The combined table -- the live nodes [0, N), then
// M = t_max[k] template nodes -- lives in registers, thread t owning nodes t + BLK * j: a live node is loaded
// from the shared read-only table, a template node is made of the candidate's three words and never loaded.
// The quota (SPEC.md 2.10) is k_policy's: what each dimension still admits in three lanes of one register of
// every wave, tested on the broadcast record before the node search; a QUOTA container leaves by a uniform
// continue in front of the reduction, so the parity still counts reductions.  A call without a quota passes
// no cap (qlim = 0) and the test is three scalar compares that never hold.
template <int BLK, int K, bool SP, bool FB>
__global__ __launch_bounds__(BLK) void k_grow_policy(const GrowPolicyArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    if (*a.bad) return;  // a t_max or domain value out of range somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t k = blockIdx.x, N = a.N, C = a.C;
    const uint32_t np = *a.cnt < C ? *a.cnt : C;  // uniform
    uint32_t *row = a.summary + (size_t)k * FP_GROW_WORDS;
    uint32_t *prow = a.policy ? a.policy + (size_t)k * FP_GROW_POLICY_WORDS : nullptr;
    if (np == 0) {  // nothing pending: rows of zeros
        if (t < FP_GROW_WORDS) row[t] = t == FP_GROW_FIRST_UNPLACED ? FP_NONE : 0u;
        if (prow && t < FP_GROW_POLICY_WORDS) prow[t] = 0u;
        return;
    }
    const uint32_t strat = a.strategy, pref = a.preferred;
    const uint32_t tc = a.t_cpu[k], tm = a.t_mem[k], tl = a.t_lab[k];
    uint32_t M = a.t_max ? a.t_max[k] : a.max_new;  // this candidate's new nodes are [N, N + M)
    if (M > a.max_new) M = a.max_new;               // (checked: *bad) the launch holds N + max_new nodes, never more
    if (N + M > (uint32_t)(BLK * K)) M = (uint32_t)(BLK * K) - N;  // never: the geometry follows N + max_new
    const uint32_t T = N + M;

    // ---- the combined table, in registers ----
    // As in k_policy with a quota, 1024 x 8 under the spread is past the 128 registers of a 1024-thread block
    // with pmh in registers of its own: those variants keep pref_miss in nd[j], above the node field
    constexpr bool KEEP_PMH = !(SP && K == 8);
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[KEEP_PMH ? K : 1];  // pmh = pref_miss << NB: the key's high word
    uint32_t sched = 0, touched = 0;
    // ---- SPEC.md 2.7 as in k_drain_sweep: nd[j] = n << 6 | domain(n), lane d of dcnt = dom_count[d] (all-ones in
    // a domain without a schedulable node), bit j of pbits = node j's domain passes, h5 bit j = domain(j) >= 32 ----
    uint32_t nd[SP ? K : 1];
    uint32_t dcnt = 0, h5 = 0, pbits = ~0u;
    __shared__ uint32_t dtab[SP ? FP_SPREAD_MAX_DOMAINS + 2 : 1];  // counts, then the eligible mask's two words
    uint32_t el0 = 0, el1 = 0;
    uint32_t td = 0;
    if constexpr (SP) {
        td = a.t_dom[k] & (FP_SPREAD_MAX_DOMAINS - 1u);  // (checked: *bad)
        for (uint32_t i = t; i < FP_SPREAD_MAX_DOMAINS + 2; i += (uint32_t)BLK) dtab[i] = 0u;
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t n = t + (uint32_t)BLK * j;
        const bool live = n < N, fresh = !live && n < T;
        cf[j] = live ? a.cpu_free[n] : fresh ? tc : 0u;
        mf[j] = live ? a.mem_free[n] : fresh ? tm : 0u;
        cu[j] = live ? a.conflict_used[n] : 0u;
        lab[j] = live ? a.labels[n] : fresh ? tl : 0u;
        cnt[j] = live && a.node_count ? a.node_count[n] : 0u;
        if ((live && a.schedulable[n]) || fresh) sched |= 1u << j;
        if constexpr (KEEP_PMH) pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
        if constexpr (SP) {
            // k_grow_policy_check refused a value >= 64 before this kernel; the mask keeps the LDS index in
            // bounds whatever the memory holds
            const uint32_t d = live ? a.domain[n] & (FP_SPREAD_MAX_DOMAINS - 1u) : fresh ? td : 0u;
            nd[j] = n << DOM_BITS | d;
            if constexpr (!KEEP_PMH) nd[j] |= (uint32_t)__popc(pref & ~lab[j]) << NB;
            h5 |= (d >> 5) << j;
            if (cnt[j]) atomicAdd(&dtab[d], cnt[j]);  // u32, wraps; a new node starts at 0
            if ((sched >> j) & 1u) {  // schedulable: its domain is eligible (the template's as soon as M >= 1)
                if (d < 32u) el0 |= 1u << d;
                else el1 |= 1u << (d - 32u);
            }
        }
    }
    const uint32_t mskew = a.max_skew;
    auto skew_bits = [&]() {
        const uint64_t m = __ballot(dcnt - wave_min32(dcnt) < mskew);
        uint32_t x = 0, y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            x |= __builtin_amdgcn_ubfe((uint32_t)m, nd[j], 1u) << j;
            y |= __builtin_amdgcn_ubfe((uint32_t)(m >> 32), nd[j], 1u) << j;
        }
        pbits = (x & ~h5) | (y & h5);
    };
    // max - min of the counts over the eligible domains, 0 without one (uniform; all 64 lanes active)
    auto skew_now = [&]() -> uint32_t {
        const bool elig = (dtab[FP_SPREAD_MAX_DOMAINS + (lane >> 5)] >> (lane & 31u)) & 1u;
        const uint32_t mx = ~wave_min32(elig ? ~dcnt : ~0u);
        return __ballot(elig) != 0ull ? mx - wave_min32(dcnt) : 0u;
    };
    uint32_t before = 0;
    if constexpr (SP) {
        if (el0) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS], el0);
        if (el1) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS + 1], el1);
        __syncthreads();
        const bool elig = (dtab[FP_SPREAD_MAX_DOMAINS + (lane >> 5)] >> (lane & 31u)) & 1u;
        dcnt = elig ? dtab[lane] : ~0u;
        before = skew_now();
        skew_bits();
    }

    // ---- SPEC.md 2.10: lane d < 3 of qv = what dimension d still admits (k_policy) ----
    uint32_t qv = lane == FP_QUOTA_CPU ? a.qrem[FP_QUOTA_CPU] : lane == FP_QUOTA_MEM ? a.qrem[FP_QUOTA_MEM] : a.qrem[FP_QUOTA_SERVICES];
    const uint32_t qlim = a.qlim;
    auto q_blocks = [&](uint32_t d, uint32_t r) { return ((qlim >> d) & 1u) != 0u && r > bcast(qv, d); };

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0;
    // the same in every thread
    uint32_t placed_n = 0, unpl_n = 0, capped_n = 0, first = FP_NONE;
    uint32_t on_live = 0, n_relaxed = 0, n_skew = 0, n_quota = 0;
    const size_t ob = (size_t)k * C;

    // ---- pending records, 64 per chunk, one chunk ahead ----
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;
    auto load = [&](uint32_t i) {
        const bool in = i < np;
        r_cpu = in ? a.r_cpu[i] : 0u;
        r_mem = in ? a.r_mem[i] : 0u;
        r_req = in ? a.r_req[i] : 0u;
        r_conf = in ? a.r_conf[i] : 0u;
        r_idx = in ? a.r_idx[i] : 0u;
    };
    load(lane);

    for (uint32_t i0 = 0; i0 < np; i0 += 64u) {
        const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx;
        if (i0 + 64u < np) load(i0 + 64u + lane);
        const uint32_t nu = np - i0 < 64u ? np - i0 : 64u;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t idx = bcast(c_idx, u);
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // ---- SPEC.md 2.10: admission before scheduling (uniform; no barrier, par stays) ----
            if (q_blocks(FP_QUOTA_CPU, cpu) || q_blocks(FP_QUOTA_MEM, mem) || q_blocks(FP_QUOTA_SERVICES, 1u)) {
                if (first == FP_NONE) first = idx;
                ++n_quota;
                if (t == 0 && a.reason && idx < C) a.reason[ob + idx] = (uint8_t)FP_REASON_QUOTA;
                continue;
            }

            // ---- this thread's min key (SPEC.md 2.6) ----
            uint64_t best = KEY_NONE;
            // the node field's mask, opaque per container: taking nd[j] apart is loop-invariant, and hoisted out
            // of the container loop it would cost the K registers that packing saved (k_policy)
            uint32_t nmask = (1u << NB) - 1u;
            if constexpr (!KEEP_PMH) asm volatile("" : "+s"(nmask));
            auto local_min = [&](auto strat_c, auto relax_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
                constexpr bool RX = decltype(relax_c)::value;  // the container may relax (FB only)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (K > 1 && (uint32_t)BLK * j >= T) break;  // a slot row past N + M holds no node (uniform)
                    bool ok;
                    uint32_t hoph = 0;  // hop << 29: the key's high word
                    if constexpr (RX) {
                        // 2.3 under req_{n_hops}; the hop counts the earlier requirements the node misses
                        const uint32_t miss = req & ~lab[j];
                        ok = ((sched >> j) & 1u) && fpd::fits(cpu, mem, 0u, conf, cf[j], mf[j], 0u, cu[j]) &&
                             (miss & a.keep[3]) == 0u;
                        hoph = ((miss != 0u ? 1u : 0u) + ((miss & a.keep[0]) != 0u ? 1u : 0u) +
                                ((miss & a.keep[1]) != 0u ? 1u : 0u) + ((miss & a.keep[2]) != 0u ? 1u : 0u))
                               << (KEY_HOP_SHIFT - 32);
                    } else {
                        ok = ((sched >> j) & 1u) && fpd::fits(cpu, mem, req, conf, cf[j], mf[j], lab[j], cu[j]);
                    }
                    const uint32_t prim = ST == FP_STRATEGY_SPREAD        ? cnt[j]
                                          : ST == FP_STRATEGY_PACK        ? cf[j] - cpu
                                          : ST == FP_STRATEGY_FILL_LOWEST ? ~cf[j]
                                                                          : 0u;
                    uint32_t hi;
                    if constexpr (KEEP_PMH) hi = pmh[j] | (prim >> (32 - NB));
                    else hi = (nd[j] & ~nmask) | (prim >> (32 - NB));
                    if constexpr (RX) hi |= hoph;
                    if constexpr (SP) {
                        const uint32_t lo = (prim << NB) | (KEEP_PMH ? nd[j] : nd[j] & nmask);
                        const uint64_t key = ((uint64_t)hi << 32) | lo;
                        best = min64(best, ok ? ((pbits >> j) & 1u ? key : KEY_SKEW) : KEY_NONE);
                    } else {
                        const uint32_t lo = (prim << NB) | (t + (uint32_t)BLK * j);
                        best = min64(best, ok ? ((uint64_t)hi << 32) | lo : KEY_NONE);
                    }
                }
            };
            auto by_strategy = [&](auto relax_c) {
                switch (strat) {  // uniform
                case FP_STRATEGY_SPREAD: local_min(std::integral_constant<uint32_t, FP_STRATEGY_SPREAD>{}, relax_c); break;
                case FP_STRATEGY_PACK: local_min(std::integral_constant<uint32_t, FP_STRATEGY_PACK>{}, relax_c); break;
                case FP_STRATEGY_FILL_LOWEST: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FILL_LOWEST>{}, relax_c); break;
                default: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FIRST_FIT>{}, relax_c); break;
                }
            };
            if constexpr (FB) {
                // a container that requires none of the bits the chain gives up cannot relax (uniform): the
                // 2.6 loop, hop 0 in every key
                if ((req & ~a.keep[3]) != 0u) by_strategy(std::true_type{});
                else by_strategy(std::false_type{});
            } else {
                by_strategy(std::false_type{});
            }

            // ---- wave min, then block min over the per-wave slots ----
            best = wave_min64(best);
            if (NW > 1) {
                static_assert(NW == 1 || NW == 16, "one slot per lane of a 16-lane row");
                if (lane == 0) slot[par][w] = best;
                __syncthreads();
                best = row_min64(slot[par][lane & (NW - 1)]);  // every row of 16 lanes holds all 16 slots
                par ^= 1u;
            }

            // ---- the winner ----
            const bool placed = SP ? best < KEY_SKEW : best != KEY_NONE;
            const uint32_t nf = (uint32_t)best & ((1u << NB) - 1u);
            const uint32_t n = SP ? nf >> DOM_BITS : nf;
            if (placed && (n & (uint32_t)(BLK - 1)) == t) {
                const uint32_t J = n / (uint32_t)BLK;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if ((uint32_t)j == J) {
                        cf[j] -= cpu;
                        mf[j] -= mem;
                        cu[j] |= conf;
                        cnt[j] += 1u;
                        touched |= 1u << j;
                    }
                }
            }
            if constexpr (SP) {
                if (placed) {  // every wave: the winner's domain gains one, the mask follows
                    dcnt += lane == (nf & (FP_SPREAD_MAX_DOMAINS - 1u)) ? 1u : 0u;
                    skew_bits();
                }
            }
            uint32_t hop = 0;
            if (placed) {
                // lane d's request; what the lanes from 3 up hold is never read
                qv -= lane == FP_QUOTA_CPU ? cpu : lane == FP_QUOTA_MEM ? mem : 1u;  // u32, wraps
                ++placed_n;
                on_live += n < N ? 1u : 0u;
                if constexpr (FB) {
                    hop = (uint32_t)(best >> KEY_HOP_SHIFT);
                    n_relaxed += hop != 0u ? 1u : 0u;
                }
            } else {
                if (first == FP_NONE) first = idx;
                const uint32_t rl = FB ? req & a.keep[3] : req;  // the requirement of the last hop
                if (SP && best == KEY_SKEW) ++n_skew;
                else if ((cpu > tc) | (mem > tm) | ((tl & rl) != rl)) ++unpl_n;  // no number of this template helps
                else ++capped_n;
            }
            if (t == 0 && idx < C) {
                if (placed) {
                    if (a.assign_out) a.assign_out[ob + idx] = n;
                    if constexpr (FB) {
                        if (a.hops && hop) a.hops[ob + idx] = (uint8_t)hop;
                    }
                } else if (a.reason) {
                    a.reason[ob + idx] = (uint8_t)(SP && best == KEY_SKEW ? FP_REASON_SKEW : FP_REASON_NOFIT);
                }
            }
        }
    }

    // ---- the candidate's rows: the new servers that received a container and what is left on them ----
    uint32_t opened = 0, lc = 0, lm = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool in = ((touched >> j) & 1u) && t + (uint32_t)BLK * j >= N;
        opened += in ? 1u : 0u;
        lc += in ? cf[j] : 0u;  // u32, wraps
        lm += in ? mf[j] : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        opened += (uint32_t)__shfl_xor((int)opened, o);
        lc += (uint32_t)__shfl_xor((int)lc, o);
        lm += (uint32_t)__shfl_xor((int)lm, o);
    }
    if (NW > 1) {
        __shared__ uint32_t opw[NW], lcw[NW], lmw[NW];
        if (lane == 0) {
            opw[w] = opened;
            lcw[w] = lc;
            lmw[w] = lm;
        }
        __syncthreads();
        opened = 0;
        lc = 0;
        lm = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < NW; ++ww) {
            opened += opw[ww];
            lc += lcw[ww];
            lm += lmw[ww];
        }
    }
    // dtab still holds the prologue's eligible mask: nothing wrote to it since
    uint32_t after = 0;
    if constexpr (SP) after = skew_now();
    if (t == 0) {
        row[FP_GROW_PENDING] = np;
        row[FP_GROW_PLACED] = placed_n;
        row[FP_GROW_OPENED] = opened;
        row[FP_GROW_UNPLACEABLE] = unpl_n;
        row[FP_GROW_CAPPED] = capped_n;
        row[FP_GROW_LEFT_CPU] = lc;
        row[FP_GROW_LEFT_MEM] = lm;
        row[FP_GROW_FIRST_UNPLACED] = first;
        if (prow) {
            prow[FP_GROW_ON_LIVE] = on_live;
            prow[FP_GROW_RELAXED] = n_relaxed;
            prow[FP_GROW_STUCK_SKEW] = n_skew;
            prow[FP_GROW_STUCK_QUOTA] = n_quota;
            prow[FP_GROW_SKEW_BEFORE] = before;
            prow[FP_GROW_SKEW_AFTER] = after;
            prow[6] = 0u;
            prow[7] = 0u;
        }
    }
}

// the geometry follows N + max_new, both host values, through the five shapes of the drain sweep
template <bool SP, bool FB>
void launch_grow_policy(const GrowPolicyArgs &a, uint32_t n_cand, hipStream_t st) {
    const uint32_t T = a.N + a.max_new;
    if (T <= 64) k_grow_policy<64, 1, SP, FB><<<n_cand, 64, 0, st>>>(a);
    else if (T <= 1024) k_grow_policy<1024, 1, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else if (T <= 2048) k_grow_policy<1024, 2, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else if (T <= 4096) k_grow_policy<1024, 4, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else k_grow_policy<1024, 8, SP, FB><<<n_cand, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_grow_sweep_impl(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                           uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                           const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out) {
    const uint32_t C = cs->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (n_cand > 65535u || max_new > FP_GROW_MAX_NEW) return FP_EOVERFLOW;
    if (reason_mask && !reason) return FP_EINVAL;
    if (C && !fp_has_cont(cs)) return FP_EINVAL;
    if (n_cand && (!t_cpu || !t_mem || !t_labels || !summary_out)) return FP_EINVAL;
    if (n_cand == 0) return FP_OK;
    hipStream_t st = c->stream;

    GrowFront f;
    if (int rc = grow_front(c, cs, reason, reason_mask, &f)) return rc;
    if (t_max) {
        k_grow_check<<<grid_for(n_cand, 256), 256, 0, st>>>(t_max, n_cand, max_new, f.bad, c->d_err);
        FP_HIP(hipGetLastError());
    }

    GrowArgs a = {};
    a.C = C; a.max_new = max_new; a.cnt = f.cnt;
    a.r_cpu = f.r_cpu; a.r_mem = f.r_mem; a.r_req = f.r_req; a.r_conf = f.r_conf; a.r_idx = f.r_idx;
    a.t_cpu = t_cpu; a.t_mem = t_mem; a.t_lab = t_labels; a.t_max = t_max;
    a.summary = summary_out; a.assign_out = C ? assign_out : nullptr;
    a.bad = f.bad;
    if (C && assign_out) {
        const size_t n = (size_t)n_cand * C;
        k_grow_init<<<grid_for(n, 256), 256, 0, st>>>(assign_out, n, f.bad);
        FP_HIP(hipGetLastError());
    }
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    launch_grow(a, n_cand, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}

int fp_dev_grow_sweep_policy_impl(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                                  const fp_nodes *ns, uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem,
                                  const uint32_t *t_labels, const uint32_t *t_max, uint32_t max_new,
                                  uint32_t *summary_out, uint32_t *assign_out, const fp_grow_policy &pol) {
    const uint32_t C = cs->n, N = ns->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (n_cand > 65535u || max_new > FP_GROW_MAX_NEW || (uint64_t)N + max_new > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    if (pol.strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (pol.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    if (reason_mask && !reason) return FP_EINVAL;
    const bool sp = pol.t_domain && pol.max_skew != 0u;  // SPEC.md 2.18: otherwise neither domain array is read
    const bool fb = pol.relax_mask && pol.n_hops != 0u;  // relax_mask is a HOST array, read here
    if (C && !fp_has_cont(cs)) return FP_EINVAL;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    if (N && sp && !pol.domain) return FP_EINVAL;
    if (n_cand && (!t_cpu || !t_mem || !t_labels || !summary_out)) return FP_EINVAL;
    if (n_cand == 0) return FP_OK;
    hipStream_t st = c->stream;

    GrowFront f;
    if (int rc = grow_front(c, cs, reason, reason_mask, &f)) return rc;
    if (t_max || sp) {
        const size_t n = n_cand > N ? n_cand : N;
        k_grow_policy_check<<<grid_for(n, 256), 256, 0, st>>>(t_max, n_cand, max_new, sp ? pol.domain : nullptr,
                                                              sp ? N : 0u, sp ? pol.t_domain : nullptr, f.bad, c->d_err);
        FP_HIP(hipGetLastError());
    }

    GrowPolicyArgs a = {};
    a.C = C; a.N = N; a.max_new = max_new; a.strategy = pol.strategy; a.preferred = pol.preferred;
    a.cnt = f.cnt;
    a.r_cpu = f.r_cpu; a.r_mem = f.r_mem; a.r_req = f.r_req; a.r_conf = f.r_conf; a.r_idx = f.r_idx;
    a.cpu_free = ns->cpu_free; a.mem_free = ns->mem_free; a.conflict_used = ns->conflict_used;
    a.labels = ns->labels; a.schedulable = ns->schedulable; a.node_count = pol.node_count;
    a.t_cpu = t_cpu; a.t_mem = t_mem; a.t_lab = t_labels; a.t_max = t_max;
    a.domain = sp ? pol.domain : nullptr; a.t_dom = sp ? pol.t_domain : nullptr; a.max_skew = sp ? pol.max_skew : 0u;
    fp_keep_masks(pol.relax_mask, pol.n_hops, fb, a.keep);
    // quota and quota_used are HOST arrays of three words: an absent quota is three caps of UNLIMITED
    for (uint32_t d = 0; d < FP_QUOTA_DIMS; ++d) {
        const uint32_t cap = pol.quota ? pol.quota[d] : FP_QUOTA_UNLIMITED;
        const uint32_t use = pol.quota && pol.quota_used ? pol.quota_used[d] : 0u;
        a.qrem[d] = use <= cap ? cap - use : 0u;
        if (cap != FP_QUOTA_UNLIMITED) a.qlim |= 1u << d;
    }
    a.summary = summary_out; a.policy = pol.policy_out;
    a.assign_out = C ? assign_out : nullptr;
    a.hops = C ? pol.hops_out : nullptr; a.reason = C ? pol.reason_out : nullptr;
    a.bad = f.bad;
    if (a.assign_out || a.hops || a.reason) {
        const size_t n = (size_t)n_cand * C;
        k_grow_policy_init<<<grid_for(n, 256), 256, 0, st>>>(a.assign_out, a.hops, a.reason, n, f.bad);
        FP_HIP(hipGetLastError());
    }
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    fp_with_flags(sp, fb, [&](auto SP, auto FB) {
        launch_grow_policy<decltype(SP)::value, decltype(FB)::value>(a, n_cand, st);
    });
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
