// fp_drain.hip -- the drain what-if sweep (SPEC.md 2.11): for every candidate (one server, or one topology
// domain) the plan that evacuates it from a live placement, every candidate from the same base state.
// One workgroup owns one candidate and shares the one base node table with all the others.
//
// Per fp_dev_drain_sweep call (asynchronous, nothing is read back):
//   1. k_drain_check  : sets the call's "bad" word for a group[n] that is neither < n_cand nor FP_NONE and for
//                       an assign[c] that is neither < N nor FP_NONE, and FP_EINVAL in the context's error
//                       word; every later kernel that writes an output returns on the word first
//   2. bucketing      : the radix FFD order (fp_ffd_order.hip) is the 2.3 order of all containers
//                       (cpu desc, mem desc, index asc), k_drain_cand keys that order by the candidate of each
//                       container's node (n_cand = no candidate) and a second stable sort over those few bits
//                       leaves each candidate's evictees contiguous and still in the 2.3 order;
//                       k_drain_offsets finds where each candidate starts: a CSR of evictee lists
//   3. k_drain_init   : assign_out = assign, reason_out = 0 (what every container that is no evictee keeps)
//   4. k_drain_sweep<BLK,K>: one workgroup per candidate, built the way k_policy is (fp_policy.hip): the base
//                       node table in registers (thread t owns nodes t + BLK * j, indexed by the unrolled j
//                       only), the candidate's own nodes masked out of `sched`, evictee records gathered 64
//                       per wave a chunk ahead and broadcast with v_readlane, the block argmin by DPP row
//                       reductions and one parity-double-buffered LDS slot per wave (one barrier per evictee;
//                       the argument is in fp_policy.hip's header), the winner's owner updating its registers.
//                       Thread 0 stores assign_out / reason_out at the evictee's original index and the
//                       candidate's summary row at the end.  Nothing is written back to the node table.
//
// A candidate without evictees costs its block two loads and one row store; a container on a node of no
// candidate costs nothing beyond the sorts.  No device-wide synchronisation and no spin waits: the kernels
// cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

using fpd::KEY_NODE_BITS;
using fpd::KEY_NONE;
using fpd::bcast;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min64;

// behind a memset of *bad on the stream; only ever sets it
__global__ __launch_bounds__(256) void k_drain_check(const uint32_t *__restrict__ assign, uint32_t C,
                                                     const uint32_t *__restrict__ group, uint32_t N, uint32_t n_cand,
                                                     uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride)
        b |= assign[i] >= N && assign[i] != FP_NONE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        b |= group[i] >= n_cand && group[i] != FP_NONE;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// cand[i] = the candidate of the i-th container of the 2.3 order; n_cand = not an evictee of any.  The range
// tests keep the loads in bounds whatever the memory holds (a bad value was found by k_drain_check)
__global__ __launch_bounds__(256) void k_drain_cand(const uint32_t *__restrict__ order, uint32_t C,
                                                    const uint32_t *__restrict__ assign,
                                                    const uint32_t *__restrict__ group, uint32_t N, uint32_t n_cand,
                                                    uint32_t *__restrict__ cand) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t n = assign[order[i]];
        const uint32_t g = n < N ? group[n] : FP_NONE;
        cand[i] = g < n_cand ? g : n_cand;
    }
}

// off[k] = the first position of the sorted candidate keys that holds k or more, k <= n_cand
__global__ __launch_bounds__(256) void k_drain_offsets(const uint32_t *__restrict__ cand, uint32_t C, uint32_t n_cand,
                                                       uint32_t *__restrict__ off) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_cand) return;
    uint32_t lo = 0, hi = C;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cand[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    off[k] = lo;
}

__global__ __launch_bounds__(256) void k_drain_init(const uint32_t *__restrict__ assign, uint32_t C,
                                                    uint32_t *__restrict__ assign_out, uint8_t *__restrict__ reason_out,
                                                    const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += (size_t)gridDim.x * blockDim.x) {
        assign_out[i] = assign[i];
        reason_out[i] = (uint8_t)FP_REASON_OK;
    }
}

// the rows of a call without containers: no candidate has an evictee
__global__ __launch_bounds__(256) void k_drain_empty_rows(uint32_t n_cand, uint32_t *__restrict__ summary,
                                                          const uint32_t *__restrict__ bad) {
    if (*bad) return;
    const size_t n = (size_t)n_cand * FP_DRAIN_WORDS;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        summary[i] = i % FP_DRAIN_WORDS == FP_DRAIN_FIRST_STRANDED ? FP_NONE : 0u;
}

struct DrainArgs {
    uint32_t C, N, strategy, preferred;
    const uint32_t *order;                                // evictees grouped by candidate, each group in 2.3 order
    const uint32_t *off;                                  // [n_cand + 1] where each group starts
    const uint32_t *cpu, *mem, *req, *conf;               // [C]
    const uint32_t *cpu_free, *mem_free, *conflict_used;  // [N] the base table: read only
    const uint32_t *labels;                               // [N]
    const uint8_t *schedulable;                           // [N]
    const uint32_t *node_count;                           // [N] or null (zeros)
    const uint32_t *group;                                // [N]
    uint32_t *assign_out;                                 // [C]
    uint8_t *reason_out;                                  // [C]
    uint32_t *summary;                                    // [n_cand][FP_DRAIN_WORDS]
    const uint32_t *bad;
};

template <int BLK, int K>
__global__ __launch_bounds__(BLK) void k_drain_sweep(const DrainArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = KEY_NODE_BITS;
    if (*a.bad) return;  // a bad group or assign value somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t k = blockIdx.x, N = a.N;
    const uint32_t e0 = a.off[k], ne = a.off[k + 1] - e0;  // uniform
    uint32_t *row = a.summary + (size_t)k * FP_DRAIN_WORDS;
    if (ne == 0) {  // nothing runs on this candidate (or it has no node): a row of zeros
        if (t < FP_DRAIN_WORDS) row[t] = t == FP_DRAIN_FIRST_STRANDED ? FP_NONE : 0u;
        return;
    }
    const uint32_t strat = a.strategy, pref = a.preferred;

    // ---- the base node table, in registers; the candidate's own nodes are no targets ----
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K], pmh[K];  // pmh = pref_miss << NB: the key's high word
    uint32_t sched = 0, touched = 0, own = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t n = t + (uint32_t)BLK * j;
        const bool in = n < N;
        cf[j] = in ? a.cpu_free[n] : 0u;
        mf[j] = in ? a.mem_free[n] : 0u;
        cu[j] = in ? a.conflict_used[n] : 0u;
        lab[j] = in ? a.labels[n] : 0u;
        cnt[j] = in && a.node_count ? a.node_count[n] : 0u;
        const bool mine = in && a.group[n] == k;
        if (in && a.schedulable[n] && !mine) sched |= 1u << j;
        own += mine ? 1u : 0u;
        pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
    }

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0;
    // the same in every thread
    uint32_t stranded = 0, s_cpu = 0, s_mem = 0, first = FP_NONE;

    // ---- evictee records, 64 per chunk, one chunk ahead ----
    const uint32_t *ord = a.order + e0;
    auto ld_ord = [&](uint32_t i) -> uint32_t { return i < ne ? ord[i] : 0u; };
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;
    auto gather = [&](uint32_t i, uint32_t o) {
        const bool in = i < ne;
        r_cpu = in ? a.cpu[o] : 0u;
        r_mem = in ? a.mem[o] : 0u;
        r_req = in ? a.req[o] : 0u;
        r_conf = in ? a.conf[o] : 0u;
        r_idx = o;
    };
    gather(lane, ld_ord(lane));
    uint32_t o_next = ld_ord(64u + lane);

    for (uint32_t i0 = 0; i0 < ne; i0 += 64u) {
        const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx;
        if (i0 + 64u < ne) {  // the next chunk's records and the order of the one after it
            gather(i0 + 64u + lane, o_next);
            o_next = ld_ord(i0 + 128u + lane);
        }
        const uint32_t nu = ne - i0 < 64u ? ne - i0 : 64u;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t idx = bcast(c_idx, u);
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // ---- this thread's min key (SPEC.md 2.6) ----
            uint64_t best = KEY_NONE;
            auto local_min = [&](auto strat_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (K > 1 && (uint32_t)BLK * j >= N) break;  // a slot row past N holds no node (uniform)
                    const bool ok = ((sched >> j) & 1u) && fpd::fits(cpu, mem, req, conf, cf[j], mf[j], lab[j], cu[j]);
                    const uint32_t prim = ST == FP_STRATEGY_SPREAD        ? cnt[j]
                                          : ST == FP_STRATEGY_PACK        ? cf[j] - cpu
                                          : ST == FP_STRATEGY_FILL_LOWEST ? ~cf[j]
                                                                          : 0u;
                    const uint32_t hi = pmh[j] | (prim >> (32 - NB));
                    const uint32_t lo = (prim << NB) | (t + (uint32_t)BLK * j);
                    best = min64(best, ok ? ((uint64_t)hi << 32) | lo : KEY_NONE);
                }
            };
            switch (strat) {  // uniform
            case FP_STRATEGY_SPREAD: local_min(std::integral_constant<uint32_t, FP_STRATEGY_SPREAD>{}); break;
            case FP_STRATEGY_PACK: local_min(std::integral_constant<uint32_t, FP_STRATEGY_PACK>{}); break;
            case FP_STRATEGY_FILL_LOWEST: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FILL_LOWEST>{}); break;
            default: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FIRST_FIT>{}); break;
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
            const bool placed = best != KEY_NONE;
            const uint32_t n = (uint32_t)best & ((1u << NB) - 1u);
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
            if (!placed) {
                if (stranded == 0) first = idx;
                ++stranded;
                s_cpu += cpu;  // u32, wraps
                s_mem += mem;
            }
            if (t == 0) {
                a.assign_out[idx] = placed ? n : FP_NONE;
                a.reason_out[idx] = (uint8_t)(placed ? FP_REASON_OK : FP_REASON_NOFIT);
            }
        }
    }

    // ---- the candidate's row: the nodes that received an evictee and the candidate's own size ----
    uint32_t used = (uint32_t)__popc(touched);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        used += (uint32_t)__shfl_xor((int)used, o);
        own += (uint32_t)__shfl_xor((int)own, o);
    }
    if (NW > 1) {
        __shared__ uint32_t usedw[NW], ownw[NW];
        if (lane == 0) {
            usedw[w] = used;
            ownw[w] = own;
        }
        __syncthreads();
        used = 0;
        own = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < NW; ++ww) {
            used += usedw[ww];
            own += ownw[ww];
        }
    }
    if (t == 0) {
        row[FP_DRAIN_EVICTED] = ne;
        row[FP_DRAIN_STRANDED] = stranded;
        row[FP_DRAIN_STRANDED_CPU] = s_cpu;
        row[FP_DRAIN_STRANDED_MEM] = s_mem;
        row[FP_DRAIN_TARGETS] = used;
        row[FP_DRAIN_FIRST_STRANDED] = first;
        row[FP_DRAIN_NODES] = own;
        row[7] = 0u;
    }
}

void launch_drain(const DrainArgs &a, uint32_t n_cand, uint32_t N, hipStream_t st) {
    if (N <= 64) k_drain_sweep<64, 1><<<n_cand, 64, 0, st>>>(a);
    else if (N <= 1024) k_drain_sweep<1024, 1><<<n_cand, 1024, 0, st>>>(a);
    else if (N <= 2048) k_drain_sweep<1024, 2><<<n_cand, 1024, 0, st>>>(a);
    else if (N <= 4096) k_drain_sweep<1024, 4><<<n_cand, 1024, 0, st>>>(a);
    else k_drain_sweep<1024, 8><<<n_cand, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_drain_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                            const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred,
                            const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                            uint32_t *summary_out) {
    const uint32_t C = cs->n, N = ns->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (N > FP_POLICY_MAX_NODES || n_cand > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (C && (!cs->cpu_m || !cs->mem_mib || !cs->req_labels || !cs->conflict || !assign || !assign_out || !reason_out))
        return FP_EINVAL;
    if (N && (!ns->cpu_free || !ns->mem_free || !ns->labels || !ns->conflict_used || !ns->schedulable || !group))
        return FP_EINVAL;
    if (n_cand && !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;  // every candidate reads the same base assignment
    if (C == 0 && n_cand == 0) return FP_OK;
    hipStream_t st = c->stream;

    const uint32_t cand_bits = fp_bitwidth(n_cand);  // the keys are 0..n_cand
    size_t tmp2 = 0;
    fp_ffd_order fo = {};
    if (C) {
        if (cand_bits)
            FP_HIP(rocprim::radix_sort_pairs(nullptr, tmp2, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, C, 0, cand_bits, st));
        if (int rc = fp_ffd_order_size(c, 1, C, tmp2, &fo)) return rc;
    }
    // the bad word, the FFD order (whose buffers the candidate sort reuses), off
    if (int rc = fp_ws_reserve(c, 256 + fo.bytes + fp_align256(((size_t)n_cand + 1) * 4))) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    const size_t CN = C > N ? C : N;
    if (CN) {
        k_drain_check<<<grid_for(CN, 256), 256, 0, st>>>(assign, C, group, N, n_cand, bad, c->d_err);
        FP_HIP(hipGetLastError());
    }
    if (C == 0) {
        k_drain_empty_rows<<<grid_for((size_t)n_cand * FP_DRAIN_WORDS, 256), 256, 0, st>>>(n_cand, summary_out, bad);
        FP_HIP(hipGetLastError());
        return FP_OK;
    }
    k_drain_init<<<grid_for(C, 256), 256, 0, st>>>(assign, C, assign_out, reason_out, bad);
    FP_HIP(hipGetLastError());
    if (n_cand == 0) return FP_OK;

    // ---- the evictee lists: 2.3 order, then stable by candidate.  The 64-bit key buffers are free after the
    // first sort and hold the candidate keys of the second ----
    uint32_t *off = (uint32_t *)fp_ws_take(c, ((size_t)n_cand + 1) * 4);
    if (!off) return FP_ENOMEM;
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_SORT, &ev);
    if (int rc = fp_ffd_order_run(c, 1, C, cs->cpu_m, cs->mem_mib, nullptr, &fo)) return rc;
    uint32_t *cand_a = (uint32_t *)fo.keys_in, *cand_b = (uint32_t *)fo.keys_out;
    k_drain_cand<<<grid_for(C, 256), 256, 0, st>>>(fo.order, C, assign, group, N, n_cand, cand_a);
    FP_HIP(hipGetLastError());
    FP_HIP(rocprim::radix_sort_pairs(fo.tmp, tmp2, cand_a, cand_b, fo.order, fo.vals_in, C, 0, cand_bits, st));
    k_drain_offsets<<<(n_cand + 1 + 255) / 256, 256, 0, st>>>(cand_b, C, n_cand, off);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_SORT, ev);

    DrainArgs a;
    a.C = C; a.N = N; a.strategy = strategy; a.preferred = preferred;
    a.order = fo.vals_in; a.off = off;
    a.cpu = cs->cpu_m; a.mem = cs->mem_mib; a.req = cs->req_labels; a.conf = cs->conflict;
    a.cpu_free = ns->cpu_free; a.mem_free = ns->mem_free; a.conflict_used = ns->conflict_used;
    a.labels = ns->labels; a.schedulable = ns->schedulable;
    a.node_count = node_count; a.group = group;
    a.assign_out = assign_out; a.reason_out = reason_out; a.summary = summary_out;
    a.bad = bad;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    launch_drain(a, n_cand, N, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
