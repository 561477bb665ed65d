// fp_drain.hip -- the drain what-if sweep (SPEC.md 2.11; under the policy, 2.15): for every candidate (one
// server, or one topology domain) the plan that evacuates it from a live placement, every candidate from the
// same base state.
// One workgroup owns one candidate and shares the one base node table with all the others.
//
// Per fp_dev_drain_sweep call (asynchronous, nothing is read back):
//   1. k_drain_check  : sets the call's "bad" word for a group[n] that is neither < n_cand nor FP_NONE and for
//                       an assign[c] that is neither < N nor FP_NONE (and, under a spread constraint, for a
//                       domain[n] of 64 or more), and FP_EINVAL in the context's error word; every later
//                       kernel that writes an output returns on the word first
//   2. bucketing      : the radix FFD order (fp_ffd_order.hip) is the 2.3 order of all containers
//                       (cpu desc, mem desc, index asc), k_drain_cand keys that order by the candidate of each
//                       container's node (n_cand = no candidate) and a second stable sort over those few bits
//                       leaves each candidate's evictees contiguous and still in the 2.3 order;
//                       k_drain_offsets finds where each candidate starts: a CSR of evictee lists
//   3. k_drain_init   : assign_out = assign, reason_out = 0, hops_out = 0 where the call has one (what every
//                       container that is no evictee keeps)
//   4. k_drain_sweep<BLK,K>: one workgroup per candidate, built the way k_policy is (fp_policy.hip): the base
//                       node table in registers (thread t owns nodes t + BLK * j, indexed by the unrolled j
//                       only), the candidate's own nodes masked out of `sched`, evictee records gathered 64
//                       per wave a chunk ahead and broadcast with v_readlane, the block argmin by DPP row
//                       reductions and one parity-double-buffered LDS slot per wave (one barrier per evictee;
//                       the argument is in fp_policy.hip's header), the winner's owner updating its registers.
//                       Thread 0 stores assign_out / reason_out at the evictee's original index and the
//                       candidate's summary row at the end.  Nothing is written back to the node table.
//
//
// Under the policy (SPEC.md 2.15, fp_dev_drain_sweep_policy) the same kernel runs as k_drain_sweep<BLK,K,SP,FB>:
// SP with the tenant's spread constraint, FB with its fallback chain, both exactly as k_policy has them
// (fp_policy.hip's header): the 64 domain counts in one register of every wave (lane d = domain d), their
// DPP minimum and the ballot of `count - min < max_skew` as the mask of the domains that pass, nd[j] =
// n << 6 | domain in the key's node field, KEY_SKEW = KEY_NONE - 1 so that the one reduction tells SKEW from
// NOFIT, the hop above pref_miss in the 23-bit-node layout, and the shortcut for an evictee that requires
// none of the relaxable bits.  What is the drain's own is the base state, which is per candidate: the LDS
// table of the prologue is built by every block for itself, sums node_count only over the nodes outside the
// candidate and takes a domain for eligible when it has a TARGET (`sched` after the candidate's nodes were
// masked out), so a drained zone never holds the minimum down.  SKEW_BEFORE is taken there, SKEW_AFTER and
// the three counters in the epilogue.  max_skew and the chain's cumulative masks are host scalars and reach
// the kernel by value.  Neither SP nor FB adds a barrier or LDS traffic per evictee, so the parity argument
// of fp_policy.hip's header carries over unchanged: one barrier per evictee, the slots double-buffered by
// the parity of the reductions run so far.  <.., false, false> is the 2.11 kernel, instruction for
// instruction what it was before the policy variants existed (64 x 1 and 1024 x 1 with two vector registers
// exchanged), and all that fp_dev_drain_sweep launches.
//
// A candidate without evictees costs its block two loads and one row store; a container on a node of no
// candidate costs nothing beyond the sorts.  No device-wide synchronisation and no spin waits: the kernels
// cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

using fpd::DOM_BITS;
using fpd::KEY_HOP_SHIFT;
using fpd::KEY_NODE_BITS;
using fpd::KEY_NODE_BITS_FB;
using fpd::KEY_NONE;
using fpd::KEY_SKEW;
using fpd::bcast;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min32;
using fpd::wave_min64;
static_assert((1u << DOM_BITS) == FP_SPREAD_MAX_DOMAINS && FP_SPREAD_MAX_DOMAINS == 64, "one domain per lane");
static_assert((uint64_t)FP_POLICY_MAX_NODES << DOM_BITS <= (1ull << KEY_NODE_BITS_FB), "node << 6 | domain fits the node field");
static_assert(FP_FALLBACK_MAX_HOPS == 4 && FP_FALLBACK_MAX_HOPS < (1u << (64 - KEY_HOP_SHIFT)), "the hop fits its field");

// behind a memset of *bad on the stream; only ever sets it.  domain: null, or (SPEC.md 2.15, a call under a
// spread constraint) the [N] domain ids, every one of which has to be below FP_SPREAD_MAX_DOMAINS
__global__ __launch_bounds__(256) void k_drain_check(const uint32_t *__restrict__ assign, uint32_t C,
                                                     const uint32_t *__restrict__ group, uint32_t N, uint32_t n_cand,
                                                     const uint32_t *__restrict__ domain, uint32_t *__restrict__ bad,
                                                     uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride)
        b |= assign[i] >= N && assign[i] != FP_NONE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        b |= (group[i] >= n_cand && group[i] != FP_NONE) || (domain && domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS);
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
                                                    uint8_t *__restrict__ hops_out, const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += (size_t)gridDim.x * blockDim.x) {
        assign_out[i] = assign[i];
        reason_out[i] = (uint8_t)FP_REASON_OK;
        if (hops_out) hops_out[i] = 0;  // SPEC.md 2.15: what every container but a relaxed move keeps
    }
}

// SPEC.md 2.15: the policy rows of a call without evictees, or without a guarantee: zeros
__global__ __launch_bounds__(256) void k_drain_zero_policy(uint32_t n_cand, uint32_t *__restrict__ policy,
                                                           const uint32_t *__restrict__ bad) {
    if (*bad) return;
    const size_t n = (size_t)n_cand * FP_DRAIN_POLICY_WORDS;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        policy[i] = 0u;
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
    // SPEC.md 2.15, read by the SP / FB variants only.  Behind everything else, so that <.., false, false>
    // loads its arguments from where it always did
    const uint32_t *domain;                               // [N] topology domain; read by <.., true, ..>
    uint32_t max_skew;                                    // not 0 in <.., true, ..>
    uint32_t keep[FP_FALLBACK_MAX_HOPS];                  // ~cum[h + 1]; entries past n_hops repeat the last one
    uint8_t *hops;                                        // [C] or null: a moved evictee's hop
    uint32_t *policy;                                     // [n_cand][FP_DRAIN_POLICY_WORDS] or null
};

// SP: under the spread constraint of SPEC.md 2.7 on the candidate's own base counts (2.15).  FB: under the
// fallback chain of 2.8.  Neither: SPEC.md 2.11, and the code it was before 2.15 existed.
template <int BLK, int K, bool SP, bool FB>
__global__ __launch_bounds__(BLK) void k_drain_sweep(const DrainArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    if (*a.bad) return;  // a bad group or assign value somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t k = blockIdx.x, N = a.N;
    const uint32_t e0 = a.off[k], ne = a.off[k + 1] - e0;  // uniform
    uint32_t *row = a.summary + (size_t)k * FP_DRAIN_WORDS;
    if (ne == 0) {  // nothing runs on this candidate (or it has no node): a row of zeros
        if (t < FP_DRAIN_WORDS) row[t] = t == FP_DRAIN_FIRST_STRANDED ? FP_NONE : 0u;
        if constexpr (SP || FB) {
            if (a.policy && t < FP_DRAIN_POLICY_WORDS) a.policy[(size_t)k * FP_DRAIN_POLICY_WORDS + t] = 0u;
        }
        return;
    }
    const uint32_t strat = a.strategy, pref = a.preferred;

    // ---- the base node table, in registers; the candidate's own nodes are no targets ----
    // As in k_policy, 1024 x 8 under both the spread and the chain is past the 128 registers of a 1024-thread
    // block with pmh in registers of its own: that variant keeps pref_miss in nd[j], above the 23-bit node
    // field (where it sits in the key's high word)
    constexpr bool KEEP_PMH = !(SP && FB && K == 8);
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[KEEP_PMH ? K : 1];  // pmh = pref_miss << NB: the key's high word
    uint32_t sched = 0, touched = 0, own = 0;
    // ---- SPEC.md 2.15 on 2.7: nd[j] = n << 6 | domain(n) is the key's node field of each owned node; lane d of
    // dcnt = dom_count[d] of this candidate, all-ones in a domain without a target; bit j of pbits = node j's
    // domain passes the skew test, h5 bit j = domain(j) >= 32 (k_policy's skew_bits) ----
    uint32_t nd[SP ? K : 1];
    uint32_t dcnt = 0, h5 = 0, pbits = ~0u;
    __shared__ uint32_t dtab[SP ? FP_SPREAD_MAX_DOMAINS + 2 : 1];  // counts, then the eligible mask's two words
    uint32_t el0 = 0, el1 = 0;
    if constexpr (SP) {
        for (uint32_t i = t; i < FP_SPREAD_MAX_DOMAINS + 2; i += (uint32_t)BLK) dtab[i] = 0u;
        __syncthreads();
    }
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
        if constexpr (KEEP_PMH) pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
        if constexpr (SP) {
            // k_drain_check refused a value >= 64 before this kernel; the mask keeps the LDS index in bounds
            // whatever the memory holds
            const uint32_t d = in ? a.domain[n] & (FP_SPREAD_MAX_DOMAINS - 1u) : 0u;
            nd[j] = n << DOM_BITS | d;
            if constexpr (!KEEP_PMH) nd[j] |= (uint32_t)__popc(pref & ~lab[j]) << NB;
            h5 |= (d >> 5) << j;
            // the candidate's own nodes count for nothing: what runs there is leaving
            if (in && !mine && cnt[j]) atomicAdd(&dtab[d], cnt[j]);  // u32, wraps
            if ((sched >> j) & 1u) {  // a target: its domain is eligible
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
    if constexpr (SP) {
        if (el0) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS], el0);
        if (el1) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS + 1], el1);
        __syncthreads();
        const bool elig = (dtab[FP_SPREAD_MAX_DOMAINS + (lane >> 5)] >> (lane & 31u)) & 1u;
        dcnt = elig ? dtab[lane] : ~0u;
        const uint32_t before = skew_now();
        if (t == 0 && a.policy) a.policy[(size_t)k * FP_DRAIN_POLICY_WORDS + FP_DRAIN_SKEW_BEFORE] = before;
        skew_bits();
    }

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0;
    // the same in every thread
    uint32_t stranded = 0, s_cpu = 0, s_mem = 0, first = FP_NONE;
    uint32_t n_skew = 0, n_relaxed = 0;  // SPEC.md 2.15: stranded on SKEW, moved at a hop >= 1

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
            // the node field's mask, opaque per evictee: taking nd[j] apart is loop-invariant, and hoisted out
            // of the evictee loop it would cost the K registers that packing saved (k_policy)
            uint32_t nmask = (1u << NB) - 1u;
            if constexpr (!KEEP_PMH) asm volatile("" : "+s"(nmask));
            auto local_min = [&](auto strat_c, auto relax_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
                constexpr bool RX = decltype(relax_c)::value;  // the evictee may relax (FB only)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (K > 1 && (uint32_t)BLK * j >= N) break;  // a slot row past N holds no node (uniform)
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
                // an evictee that requires none of the bits the chain gives up cannot relax (uniform): the
                // 2.6 loop, hop 0 in every key
                if ((req & ~a.keep[3]) != 0u) by_strategy(std::true_type{});
                else by_strategy(std::false_type{});
            } else {
                // a plain switch at this level, as in k_policy: the FB = false kernels keep their layout
                switch (strat) {  // uniform
                case FP_STRATEGY_SPREAD: local_min(std::integral_constant<uint32_t, FP_STRATEGY_SPREAD>{}, std::false_type{}); break;
                case FP_STRATEGY_PACK: local_min(std::integral_constant<uint32_t, FP_STRATEGY_PACK>{}, std::false_type{}); break;
                case FP_STRATEGY_FILL_LOWEST: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FILL_LOWEST>{}, std::false_type{}); break;
                default: local_min(std::integral_constant<uint32_t, FP_STRATEGY_FIRST_FIT>{}, std::false_type{}); break;
                }
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
            if (!placed) {
                if (stranded == 0) first = idx;
                ++stranded;
                s_cpu += cpu;  // u32, wraps
                s_mem += mem;
                if constexpr (SP) n_skew += best == KEY_SKEW ? 1u : 0u;
            }
            uint32_t hop = 0;
            if constexpr (FB) {
                hop = placed ? (uint32_t)(best >> KEY_HOP_SHIFT) : 0u;
                n_relaxed += hop != 0u ? 1u : 0u;
            }
            if (t == 0) {
                a.assign_out[idx] = placed ? n : FP_NONE;
                a.reason_out[idx] = (uint8_t)(placed ? FP_REASON_OK : SP && best == KEY_SKEW ? FP_REASON_SKEW : FP_REASON_NOFIT);
                if constexpr (FB) {
                    if (a.hops) a.hops[idx] = (uint8_t)hop;  // k_drain_init left 0 everywhere else
                }
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
    if constexpr (SP || FB) {
        // dtab still holds the prologue's eligible mask: nothing wrote to it since
        uint32_t after = 0;
        if constexpr (SP) after = skew_now();
        if (t == 0 && a.policy) {
            uint32_t *prow = a.policy + (size_t)k * FP_DRAIN_POLICY_WORDS;
            prow[FP_DRAIN_STRANDED_SKEW] = n_skew;
            prow[FP_DRAIN_RELAXED] = n_relaxed;
            if constexpr (!SP) prow[FP_DRAIN_SKEW_BEFORE] = 0u;
            prow[FP_DRAIN_SKEW_AFTER] = after;
        }
    }
}

template <bool SP, bool FB>
void launch_drain(const DrainArgs &a, uint32_t n_cand, uint32_t N, hipStream_t st) {
    if (N <= 64) k_drain_sweep<64, 1, SP, FB><<<n_cand, 64, 0, st>>>(a);
    else if (N <= 1024) k_drain_sweep<1024, 1, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else if (N <= 2048) k_drain_sweep<1024, 2, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else if (N <= 4096) k_drain_sweep<1024, 4, SP, FB><<<n_cand, 1024, 0, st>>>(a);
    else k_drain_sweep<1024, 8, SP, FB><<<n_cand, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_drain_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                            const uint32_t *group, uint32_t n_cand, uint32_t strategy, uint32_t preferred,
                            const uint32_t *node_count, uint32_t *assign_out, uint8_t *reason_out,
                            uint32_t *summary_out, const fp_drain_policy &pol) {
    const uint32_t C = cs->n, N = ns->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (N > FP_POLICY_MAX_NODES || n_cand > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (pol.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    const bool sp = pol.domain && pol.max_skew != 0u;   // SPEC.md 2.15: otherwise domain is not read
    const bool fb = pol.relax_mask && pol.n_hops != 0u;  // relax_mask is a HOST array, read here
    if (C && (!fp_has_cont(cs) || !assign || !assign_out || !reason_out)) return FP_EINVAL;
    if (N && (!fp_has_nodes(ns) || !group)) return FP_EINVAL;
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
        k_drain_check<<<grid_for(CN, 256), 256, 0, st>>>(assign, C, group, N, n_cand, sp ? pol.domain : nullptr, bad,
                                                         c->d_err);
        FP_HIP(hipGetLastError());
    }
    if (C == 0) {
        k_drain_empty_rows<<<grid_for((size_t)n_cand * FP_DRAIN_WORDS, 256), 256, 0, st>>>(n_cand, summary_out, bad);
        FP_HIP(hipGetLastError());
        if (pol.policy_out) {
            k_drain_zero_policy<<<grid_for((size_t)n_cand * FP_DRAIN_POLICY_WORDS, 256), 256, 0, st>>>(n_cand, pol.policy_out, bad);
            FP_HIP(hipGetLastError());
        }
        return FP_OK;
    }
    k_drain_init<<<grid_for(C, 256), 256, 0, st>>>(assign, C, assign_out, reason_out, pol.hops_out, bad);
    FP_HIP(hipGetLastError());
    if (n_cand == 0) return FP_OK;
    if (!sp && !fb && pol.policy_out) {  // without a guarantee the sweep is 2.11's and the rows are zeros
        k_drain_zero_policy<<<grid_for((size_t)n_cand * FP_DRAIN_POLICY_WORDS, 256), 256, 0, st>>>(n_cand, pol.policy_out, bad);
        FP_HIP(hipGetLastError());
    }

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
    a.domain = sp ? pol.domain : nullptr; a.max_skew = sp ? pol.max_skew : 0u;
    fp_keep_masks(pol.relax_mask, pol.n_hops, fb, a.keep);
    a.hops = pol.hops_out; a.policy = pol.policy_out;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    fp_with_flags(sp, fb, [&](auto SP, auto FB) {
        launch_drain<decltype(SP)::value, decltype(FB)::value>(a, n_cand, N, st);
    });
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
