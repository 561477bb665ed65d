// fp_replan_policy.hip -- re-planning a running stage under the tenant's policy (SPEC.md 2.14): the seats of
// SPEC.md 2.13 first, then the scored placement of 2.6 under the hard topology spread (2.7), the fallback chain
// (2.8) and the resource quota (2.10) on the state the seats left, batched over what-if scenarios.  One workgroup
// owns one scenario.  fp_replan.hip is the same call without a guarantee and fp_policy.hip the same placement
// without seats; this unit is written the way those two are and shares fp_argmin.h and the radix FFD order with
// them, and nothing else (what shared helpers do to the k_policy kernels).
//
// Per fp_dev_replan_batch_policy call (asynchronous, nothing is read back):
//   1. k_rp_check      : behind a memset of the call's "bad" word; sets it for a strategy that is no fp_strategy
//                        value, a prev[c] that is neither < N nor FP_NONE, a domain id of 64 or more in a scenario
//                        whose max_skew is not 0 and an n_hops above FP_FALLBACK_MAX_HOPS, and FP_EINVAL in the
//                        context's error word.  Every later kernel that writes returns on the word first
//   2. the radix FFD order (fp_ffd_order.hip): cpu desc, mem desc, index asc per scenario
//   3. k_replan_policy<BLK,K,SP,FB,QT>: both passes, in launch_policy's geometries (fp_policy.hip)
//   4. k_replan_report : change_out and the summary row, when the caller asks for either
// A call without any guarantee (no domain / max_skew, no relax_mask / n_hops, no quota) is fp_replan.hip's.
//
// Pass 1 is k_replan's rule, walked a wave at a time: each wave scans order and prev and visits only the records
// whose prev is one of its own nodes (the comment at the loop).  The owner of node prev, one thread, tests its
// registers -- the 2.3 predicate without `schedulable`, under FB with the labels the whole chain
// still asks for, req & ~cum[n_hops] -- updates them and stores assign / reason / hops / quota_why of a kept
// container and strikes the container from pass 2's order: order2[i] = FP_NONE (i = the position in the visiting
// order; order2 is the call's second copy of the FFD order, which pass 1 itself never reads -- its waves run
// chunks apart without a barrier).  No skew test and no quota test (SPEC.md 2.14: the guarantees gate admission,
// they never evict), hence no reduction and no barrier per seat.  Under QT each thread sums the requests of what
// it kept (three u32, wrapping).
//
// Between the passes: ONE barrier (it orders the order2 stores before the loads below and the zeroing of the two
// LDS tables before the atomics into them), then the prologues k_policy runs at kernel start, on the post-seat
// registers: the SP domain table from cnt[j] and sched, and the QT lanes from quota_used plus the block sum of the
// kept charges; a second barrier in front of the reads of the two tables.  Skew counts and usage are reductions
// of state pass 1 already holds per thread, which is why pass 1 needs nothing per seat.
//
// Pass 2 is k_policy's loop (its header has the key layouts, the domain register, the chain's masks and the
// quota's lanes).  A kept record arrives with the index FP_NONE like a CYCLE one and leaves by the same uniform
// `continue`; what tells them apart -- a kept container is not rejected -- is settled a chunk at a time by a
// ballot when the records are gathered, so the loop carries nothing per record that k_policy's does not.
//
// The slots of the block minimum are double-buffered by the parity of the REDUCTIONS run so far.  Reduction r
// writes buffer r & 1 before barrier B_r and reads it after; the next writer of that buffer is reduction r + 2,
// which a wave reaches only past B_(r+1), and every wave arrives at B_(r+1) after its reads of reduction r (the
// keys of r + 1 depend on the winner of r).  So no write overtakes a read of the same buffer, and B_r orders every
// write before every read.  Three kinds of container run no reduction: CYCLE, QUOTA and kept.  All three leave by
// a uniform `continue` in front of the reduction, and `par` is toggled nowhere but behind the reduction's
// barrier.  So whatever lies between two reductions -- nothing, a run of skipped containers of any length and any
// mix of the three kinds, whole chunks -- consecutive reductions use different buffers and the same two barriers
// separate a buffer's reads from its next write: the argument counts reductions, never containers.  The two
// barriers between the passes are in front of reduction 0.
//
// change_out and the summary row are not computed here: the 1024 x 8 variants of k_policy sit at the 128
// registers of a 1024-thread block, and k_replan's prev / kind / counter registers do not fit beside them.
// k_replan_report derives both from prev, assign, reason, cpu and mem after the placer (KEPT <=> assign == prev !=
// FP_NONE, SPEC.md 2.14 theorem E).
//
// No device-wide synchronisation, no spin waits: the kernels cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>

namespace {

using fpd::KEY_NONE;
using fpd::KEY_NODE_BITS;  // key = pref_miss << 58 | primary << 26 | node
using fpd::bcast;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min64;
// SPEC.md 2.8, the FB variants: key = hop << 61 | pref_miss << 55 | primary << 23 | node (fp_policy.hip)
constexpr uint32_t KEY_NODE_BITS_FB = 23;
constexpr uint32_t KEY_HOP_SHIFT = 61;
// SPEC.md 2.7: a node that fits by 2.3 and fails the skew test; above every real key, below KEY_NONE
constexpr uint64_t KEY_SKEW = KEY_NONE - 1;
constexpr uint32_t DOM_BITS = 6;  // FP_SPREAD_MAX_DOMAINS = 64: a domain id is one lane of a wave
static_assert((1u << DOM_BITS) == FP_SPREAD_MAX_DOMAINS && FP_SPREAD_MAX_DOMAINS == 64, "one domain per lane");
static_assert((uint64_t)FP_POLICY_MAX_NODES << DOM_BITS <= (1ull << KEY_NODE_BITS_FB), "node << 6 | domain fits the node field");
static_assert(FP_FALLBACK_MAX_HOPS == 4 && FP_FALLBACK_MAX_HOPS < (1u << (64 - KEY_HOP_SHIFT)), "the hop fits its field");
static_assert(FP_REPLAN_KEPT == FP_CHANGE_KEPT && FP_REPLAN_NEW == FP_CHANGE_NEW && FP_REPLAN_MOVED == FP_CHANGE_MOVED &&
                  FP_REPLAN_LOST == FP_CHANGE_LOST && FP_REPLAN_ABSENT == FP_CHANGE_ABSENT && FP_REPLAN_WORDS == 8,
              "summary word d counts change value d");

// behind a memset of *bad on the stream; only ever sets it.  domain / max_skew and n_hops are null when the call
// has no constraint / no chain
__global__ __launch_bounds__(256) void k_rp_check(const uint32_t *__restrict__ strategy, uint32_t S,
                                                  const uint32_t *__restrict__ prev, size_t SC, uint32_t N,
                                                  const uint32_t *__restrict__ domain,
                                                  const uint32_t *__restrict__ max_skew,
                                                  const uint32_t *__restrict__ n_hops, uint32_t *__restrict__ bad,
                                                  uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = first; i < S; i += stride) {
        b |= strategy[i] > (uint32_t)FP_STRATEGY_FILL_LOWEST;
        if (n_hops) b |= n_hops[i] > (uint32_t)FP_FALLBACK_MAX_HOPS;
    }
    for (size_t i = first; i < SC; i += stride) b |= prev[i] >= N && prev[i] != FP_NONE;
    if (domain && N) {
        const size_t SN = (size_t)S * N;
        for (size_t i = first; i < SN; i += stride)
            b |= domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS && max_skew[i / N] != 0u;
    }
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// a call without containers: every scenario costs (0 rejected, 0 nodes used) and changes nothing; the usage stays
__global__ __launch_bounds__(256) void k_rp_empty(uint32_t S, uint32_t scen_base, const uint32_t *__restrict__ bad,
                                                  uint64_t *__restrict__ cost, uint32_t *__restrict__ summary) {
    if (*bad) return;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (cost) cost[s] = fpd::pack_cost(0, 0, scen_base + s);
    if (summary)
        for (uint32_t d = 0; d < FP_REPLAN_WORDS; ++d) summary[(size_t)s * FP_REPLAN_WORDS + d] = 0u;
}

// hops of a call that asks for them without a fallback chain: every hop is 0
__global__ __launch_bounds__(256) void k_rp_zero_hops(uint8_t *__restrict__ hops, size_t n,
                                                      const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) hops[i] = 0;
}

// SPEC.md 2.13's change values and summary row, from what the placer left.  One block per scenario.  KEPT is
// assign == prev != FP_NONE: a container that loses its seat never lands on prev again (SPEC.md 2.14 theorem E)
__global__ __launch_bounds__(256) void k_replan_report(uint32_t C, const uint32_t *__restrict__ prev,
                                                       const uint32_t *__restrict__ assign,
                                                       const uint8_t *__restrict__ reason,
                                                       const uint32_t *__restrict__ cpu, const uint32_t *__restrict__ mem,
                                                       uint8_t *__restrict__ change, uint32_t *__restrict__ summary,
                                                       const uint32_t *__restrict__ bad) {
    if (*bad) return;
    __shared__ uint32_t row[FP_REPLAN_WORDS];
    const uint32_t t = threadIdx.x, s = blockIdx.x;
    const size_t cb = (size_t)s * C;
    if (t < FP_REPLAN_WORDS) row[t] = 0u;
    __syncthreads();
    uint32_t n[5] = {0, 0, 0, 0, 0}, mc = 0, mm = 0;
    for (uint32_t i = t; i < C; i += blockDim.x) {
        const uint32_t pv = prev[cb + i], as = assign[cb + i];
        const bool had = pv != FP_NONE, placed = reason[cb + i] == (uint8_t)FP_REASON_OK;
        const uint32_t chg = placed ? (!had ? FP_CHANGE_NEW : as == pv ? FP_CHANGE_KEPT : FP_CHANGE_MOVED)
                                    : (had ? FP_CHANGE_LOST : FP_CHANGE_ABSENT);
        if (change) change[cb + i] = (uint8_t)chg;
#pragma unroll
        for (uint32_t d = 0; d < 5; ++d) n[d] += chg == d ? 1u : 0u;
        if (chg == FP_CHANGE_MOVED) {
            mc += cpu[cb + i];  // u32, wraps
            mm += mem[cb + i];
        }
    }
    if (!summary) return;
#pragma unroll
    for (uint32_t d = 0; d < 5; ++d)
        if (n[d]) atomicAdd(&row[d], n[d]);
    if (mc) atomicAdd(&row[FP_REPLAN_MOVED_CPU], mc);
    if (mm) atomicAdd(&row[FP_REPLAN_MOVED_MEM], mm);
    __syncthreads();
    if (t < FP_REPLAN_WORDS) summary[(size_t)s * FP_REPLAN_WORDS + t] = row[t];  // word 7 stays 0
}

struct ReplanPolicyArgs {
    uint32_t C, N, scen_base;
    const uint32_t *order;                          // [S][C] FFD order (index in the scenario)
    const uint32_t *cpu, *mem, *req, *conf;         // [S][C]
    const uint32_t *level;                          // [S][C] or null
    const uint32_t *prev;                           // [S][C] the node each container runs on, FP_NONE = none
    uint32_t *cpu_free, *mem_free, *conflict_used;  // [S][N] in/out
    const uint32_t *labels;                         // [S][N]
    const uint8_t *schedulable;                     // [S][N]
    uint32_t *node_count;                           // [S][N] in/out or null
    const uint32_t *strategy, *preferred;           // [S]; preferred nullable
    const uint32_t *domain;                         // [S][N] topology domain (SPEC.md 2.7); read under SP
    const uint32_t *max_skew;                       // [S], 0 = no constraint in that scenario
    uint32_t *assign;                               // [S][C]
    uint8_t *reason;                                // [S][C]
    uint64_t *cost;                                 // [S] or null
    uint32_t *order2;                               // [S][C] a copy of order; pass 1 stores FP_NONE where it kept
    const uint32_t *bad;                            // k_rp_check's word
    const uint32_t *relax_mask;                     // [S][4] label bits hop h + 1 gives up; read under FB
    const uint32_t *n_hops;                         // [S], 0 = no fallback in that scenario
    uint8_t *hops;                                  // [S][C] or null
    const uint32_t *quota;                          // [S][3] caps; read under QT
    uint32_t *quota_used;                           // [S][3] in/out or null (null starts at zero)
    uint8_t *quota_why;                             // [S][C] or null
};

// the min of fp_argmin.h over 32-bit values (the domain counts of SPEC.md 2.7)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t min32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
    v = min32(v, dpp32<0xB1>(v));
    v = min32(v, dpp32<0x4E>(v));
    v = min32(v, dpp32<0x141>(v));
    v = min32(v, dpp32<0x140>(v));
    return min32(min32(bcast(v, 0), bcast(v, 16)), min32(bcast(v, 32), bcast(v, 48)));
}

// SP / FB / QT: as k_policy's (fp_policy.hip).  At least one of them is set: the call without a guarantee is
// k_replan's.
template <int BLK, int K, bool SP, bool FB, bool QT>
__global__ __launch_bounds__(BLK) void k_replan_policy(const ReplanPolicyArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    static_assert(SP || FB || QT, "no guarantee: k_replan");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    if (*a.bad) return;  // a bad value somewhere in the batch: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t s = blockIdx.x, C = a.C, N = a.N;
    const size_t cb = (size_t)s * C, nb = (size_t)s * N;
    const uint32_t strat = a.strategy[s];
    const uint32_t pref = a.preferred ? a.preferred[s] : 0u;

    // ---- the scenario's node state, in registers (k_policy's, with its packing of pref_miss into nd[j] in
    // the variants that would otherwise pass the 128 registers of a 1024-thread block) ----
    constexpr bool KEEP_PMH = !((FB || QT) && SP && K == 8);
    constexpr bool PMH_REGS = KEEP_PMH;
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[PMH_REGS ? K : 1];  // pmh = pref_miss << NB: the key's high word; set between the passes
    auto pref_hi = [&](uint32_t l) { return (uint32_t)__popc(pref & ~l) << NB; };
    uint32_t sched = 0, touched = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t n = t + (uint32_t)BLK * j;
        const bool in = n < N;
        cf[j] = in ? a.cpu_free[nb + n] : 0u;
        mf[j] = in ? a.mem_free[nb + n] : 0u;
        cu[j] = in ? a.conflict_used[nb + n] : 0u;
        lab[j] = in ? a.labels[nb + n] : 0u;
        cnt[j] = in && a.node_count ? a.node_count[nb + n] : 0u;
        if (in && a.schedulable[nb + n]) sched |= 1u << j;
    }

    // ---- SPEC.md 2.8.  keep[h] = ~cum[h + 1], uniform: the required bits hop h + 1 still asks for.  Entries
    // past n_hops repeat the last one, so keep[3] is the test under req_{n_hops} whatever n_hops is (n_hops = 0:
    // all ones, and relax_mask is not read), and a node's hop is the number of h in 0..3 whose requirement it
    // misses.  n_hops was checked before this kernel; the clamp keeps the loop at four whatever the memory holds
    uint32_t keep[FB ? FP_FALLBACK_MAX_HOPS : 1];
    if constexpr (FB) {
        const uint32_t nh = min32(a.n_hops[s], (uint32_t)FP_FALLBACK_MAX_HOPS);
        uint32_t cum = 0;
#pragma unroll
        for (uint32_t h = 0; h < FP_FALLBACK_MAX_HOPS; ++h) {
            if (h < nh) cum |= a.relax_mask[(size_t)s * FP_FALLBACK_MAX_HOPS + h];
            keep[h] = ~cum;
        }
    }

    // the two LDS tables of the prologues between the passes, zeroed here: the barrier behind pass 1 is in front
    // of the atomics into them
    __shared__ uint32_t dtab[SP ? FP_SPREAD_MAX_DOMAINS + 2 : 1];  // counts, then the eligible mask's two words
    __shared__ uint32_t qsum[QT ? FP_QUOTA_DIMS : 1];              // what the seats charge
    if constexpr (SP)
        for (uint32_t i = t; i < FP_SPREAD_MAX_DOMAINS + 2; i += (uint32_t)BLK) dtab[i] = 0u;
    if constexpr (QT)
        if (t < FP_QUOTA_DIMS) qsum[t] = 0u;

    // ---- the FFD order (both passes) and pass 2's container records, 64 per chunk, one chunk ahead ----
    const uint32_t *ord = a.order + cb;
    auto ld_ord = [&](uint32_t i) -> uint32_t { return i < C ? ord[i] : 0u; };
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;  // r_idx = FP_NONE: skipped (CYCLE or kept)

    // ================= pass 1: seats =================
    // Only the owner of node prev does anything for a seat, so a wave needs only the records whose prev is one of
    // its own nodes (node n belongs to thread n & (BLK - 1), wave (n & (BLK - 1)) >> 6).  Every wave scans order and
    // prev of a chunk (lane l = visiting position i0 + l; prev one chunk ahead, order two), ballots the records that
    // are its own, gathers the other four words for those lanes only, and visits the set bits in ascending order:
    // the visiting order, restricted to its nodes.  A chunk without a seat of the wave costs it the scan alone --
    // with no prev anywhere, that is all of pass 1.  The waves run apart; nothing here meets a barrier.
    {
        uint32_t q_cpu = 0, q_mem = 0, q_n = 0;  // QT: the requests of the seats this thread kept (u32, wrap)
        // prev of the record at position i, FP_NONE past C and for a CYCLE container (no seat to keep, either way)
        auto ld_prev = [&](uint32_t i, uint32_t o) -> uint32_t {
            if (i >= C) return FP_NONE;
            if (a.level && a.level[cb + o] == FP_NONE) return FP_NONE;
            return a.prev[cb + o];
        };
        uint32_t o_cur = ld_ord(lane), o_next = ld_ord(64u + lane);
        uint32_t pv_next = ld_prev(lane, o_cur);
        for (uint32_t i0 = 0; i0 < C; i0 += 64u) {
            const uint32_t c_o = o_cur, c_prev = pv_next;
            if (i0 + 64u < C) {
                o_cur = o_next;
                pv_next = ld_prev(i0 + 64u + lane, o_cur);
                o_next = ld_ord(i0 + 128u + lane);
            }
            // FP_NONE is above every N; so is a value k_rp_check refused, whatever the memory holds
            const bool mine = c_prev < N && ((c_prev & (uint32_t)(BLK - 1)) >> 6) == w;
            uint64_t todo = __ballot(mine);
            if (todo == 0) continue;  // uniform over the wave
            const uint32_t c_cpu = mine ? a.cpu[cb + c_o] : 0u, c_mem = mine ? a.mem[cb + c_o] : 0u;
            const uint32_t c_req = mine ? a.req[cb + c_o] : 0u, c_conf = mine ? a.conf[cb + c_o] : 0u;
            while (todo) {
                const uint32_t u = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                const uint32_t idx = bcast(c_o, u), pv = bcast(c_prev, u);
                const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);
                if ((pv & (uint32_t)(BLK - 1)) == t) {  // the owner of node pv; pv < N <= BLK * K, so J < K
                    const uint32_t J = pv / (uint32_t)BLK;
                    // SPEC.md 2.14: the labels under req_L = req & ~cum[n_hops]; no skew test, no quota test
                    uint32_t rq = req;
                    if constexpr (FB) rq &= keep[3];
                    bool kept = false;
                    uint32_t hop = 0;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((uint32_t)j == J && fpd::fits(cpu, mem, rq, conf, cf[j], mf[j], lab[j], cu[j])) {
                            cf[j] -= cpu;
                            mf[j] -= mem;
                            cu[j] |= conf;
                            cnt[j] += 1u;
                            touched |= 1u << j;
                            kept = true;
                            if constexpr (FB) {  // 2.8's hop(n): the requirements of the earlier hops it misses
                                const uint32_t miss = req & ~lab[j];
                                hop = (miss != 0u ? 1u : 0u) + ((miss & keep[0]) != 0u ? 1u : 0u) +
                                      ((miss & keep[1]) != 0u ? 1u : 0u) + ((miss & keep[2]) != 0u ? 1u : 0u);
                            }
                        }
                    }
                    if (kept) {
                        a.order2[cb + i0 + u] = FP_NONE;
                        a.assign[cb + idx] = pv;
                        a.reason[cb + idx] = (uint8_t)FP_REASON_OK;
                        if constexpr (FB) {
                            if (a.hops) a.hops[cb + idx] = (uint8_t)hop;
                        }
                        if constexpr (QT) {  // charged, never tested
                            q_cpu += cpu;
                            q_mem += mem;
                            q_n += 1u;
                            if (a.quota_why) a.quota_why[cb + idx] = 0;
                        }
                    }
                }
            }
        }
        // the owners' order2 stores before every load of them below, and the zeroed tables before the atomics
        __syncthreads();
        if constexpr (QT) {
            if (q_cpu) atomicAdd(&qsum[FP_QUOTA_CPU], q_cpu);
            if (q_mem) atomicAdd(&qsum[FP_QUOTA_MEM], q_mem);
            if (q_n) atomicAdd(&qsum[FP_QUOTA_SERVICES], q_n);
        }
    }

    // ================= between the passes: k_policy's prologues, on the post-seat registers =================
    if constexpr (PMH_REGS) {
#pragma unroll
        for (int j = 0; j < K; ++j) pmh[j] = pref_hi(lab[j]);
    }
    // ---- SPEC.md 2.7 (fp_policy.hip): nd[j] = n << 6 | domain(n); lane d of dcnt = dom_count[d], all-ones in a
    // domain without a schedulable node; pbits bit j = node j passes the skew test.  The counts include the
    // seats, on cordoned nodes too: dom_count is derived from node_count ----
    uint32_t nd[SP ? K : 1];
    uint32_t dcnt = 0, mskew = 0, h5 = 0, pbits = ~0u;
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
    if constexpr (SP) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            nd[j] = (t + (uint32_t)BLK * j) << DOM_BITS;
            if constexpr (!KEEP_PMH) nd[j] |= pref_hi(lab[j]);
        }
        mskew = a.max_skew[s];
        if (mskew != 0u) {  // uniform over the block; 0 is 2.6: the domains are not read
            uint32_t e0 = 0, e1 = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t n = t + (uint32_t)BLK * j;
                if (n < N) {
                    // k_rp_check refused a value >= 64 before this kernel; the mask keeps the LDS index in
                    // bounds whatever the memory holds
                    const uint32_t d = a.domain[nb + n] & (FP_SPREAD_MAX_DOMAINS - 1u);
                    nd[j] |= d;
                    h5 |= (d >> 5) << j;
                    if (cnt[j]) atomicAdd(&dtab[d], cnt[j]);  // u32, wraps
                    if ((sched >> j) & 1u) {
                        if (d < 32u) e0 |= 1u << d;
                        else e1 |= 1u << (d - 32u);
                    }
                }
            }
            if (e0) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS], e0);
            if (e1) atomicOr(&dtab[FP_SPREAD_MAX_DOMAINS + 1], e1);
        }
    }
    // the usage on entry, read by every wave in front of the barrier: wave 0 stores the usage after the seats to
    // the same words behind it
    uint32_t q_cap = FP_QUOTA_UNLIMITED, q_use = 0;
    if constexpr (QT) {
        if (lane < FP_QUOTA_DIMS) {
            q_cap = a.quota[(size_t)s * FP_QUOTA_DIMS + lane];
            if (a.quota_used) q_use = a.quota_used[(size_t)s * FP_QUOTA_DIMS + lane];
        }
    }
    if constexpr (SP || QT) __syncthreads();  // the atomics above, before the reads below
    if constexpr (SP) {
        if (mskew != 0u) {
            const bool elig = (dtab[FP_SPREAD_MAX_DOMAINS + (lane >> 5)] >> (lane & 31u)) & 1u;
            dcnt = elig ? dtab[lane] : ~0u;
            skew_bits();
        }
    }

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0, rejected = 0;  // rejected is the same in every thread

    // ---- SPEC.md 2.10 (fp_policy.hip): lane d < 3 of qv holds what dimension d still admits, cap - used, 0 when
    // used is above the cap -- and here `used` is the usage after the seats, which were charged without a test
    // and can have put it there.  That usage goes to quota_used now: the epilogue finds there what k_policy's
    // finds on entry, and a dimension above its cap keeps it ----
    uint32_t qv = 0, qlim = 0;
    if constexpr (QT) {
        if (lane < FP_QUOTA_DIMS) {
            q_use += qsum[lane];  // u32, wraps
            if (w == 0 && a.quota_used) a.quota_used[(size_t)s * FP_QUOTA_DIMS + lane] = q_use;
        }
        qv = q_use <= q_cap ? q_cap - q_use : 0u;
        qlim = (uint32_t)__ballot(q_cap != FP_QUOTA_UNLIMITED);
    }
    auto q_blocks = [&](uint32_t d, uint32_t r) { return ((qlim >> d) & 1u) != 0u && r > bcast(qv, d); };

    // ================= pass 2: placement =================
    ord = a.order2 + cb;  // from here on ld_ord reads the order pass 1 struck the kept containers from
    auto gather = [&](uint32_t i, uint32_t o) {
        const bool kept = i < C && o == FP_NONE;
        const bool in = i < C && o != FP_NONE;
        r_cpu = in ? a.cpu[cb + o] : 0u;
        r_mem = in ? a.mem[cb + o] : 0u;
        r_req = in ? a.req[cb + o] : 0u;
        r_conf = in ? a.conf[cb + o] : 0u;
        const bool cyc = in && a.level && a.level[cb + o] == FP_NONE;
        r_idx = cyc || kept ? FP_NONE : o;
        // the loop below counts every record that arrives with FP_NONE as rejected; a kept one is not.  Taken
        // back here, a chunk at a time (u32, wraps for a moment), so that no record carries a flag for it
        rejected -= (uint32_t)__popcll(__ballot(kept));
        if (cyc && w == 0) {  // CYCLE: reported here, skipped below
            a.assign[cb + o] = FP_NONE;
            a.reason[cb + o] = (uint8_t)FP_REASON_CYCLE;
            if constexpr (FB) {
                if (a.hops) a.hops[cb + o] = 0;
            }
            if constexpr (QT) {
                if (a.quota_why) a.quota_why[cb + o] = 0;
            }
        }
    };
    gather(lane, ld_ord(lane));
    uint32_t o_next = ld_ord(64u + lane);

    for (uint32_t i0 = 0; i0 < C; i0 += 64u) {
        const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx;
        if (i0 + 64u < C) {  // the next chunk's records and the order of the one after it
            gather(i0 + 64u + lane, o_next);
            o_next = ld_ord(i0 + 128u + lane);
        }
        const uint32_t nu = C - i0 < 64u ? C - i0 : 64u;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t idx = bcast(c_idx, u);
            // CYCLE or kept (uniform): no reduction, no barrier, and par stays -- the parity counts reductions
            if (idx == FP_NONE) { ++rejected; continue; }
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // ---- SPEC.md 2.10: admission before scheduling, against the usage the seats and the earlier
            // placements left.  A QUOTA container leaves like a CYCLE or a kept one ----
            if constexpr (QT) {
                const uint32_t why = (q_blocks(FP_QUOTA_CPU, cpu) ? 1u << FP_QUOTA_CPU : 0u) |
                                     (q_blocks(FP_QUOTA_MEM, mem) ? 1u << FP_QUOTA_MEM : 0u) |
                                     (q_blocks(FP_QUOTA_SERVICES, 1u) ? 1u << FP_QUOTA_SERVICES : 0u);
                if (why != 0u) {  // uniform
                    ++rejected;
                    if (t == 0) {
                        a.assign[cb + idx] = FP_NONE;
                        a.reason[cb + idx] = (uint8_t)FP_REASON_QUOTA;
                        if constexpr (FB) {
                            if (a.hops) a.hops[cb + idx] = 0;
                        }
                        if (a.quota_why) a.quota_why[cb + idx] = (uint8_t)why;
                    }
                    continue;
                }
            }

            // ---- this thread's min key ----
            uint64_t best = KEY_NONE;
            // the node field's mask, opaque per container: taking nd[j] apart is loop-invariant, and hoisted
            // out of the container loop it would cost the K registers that packing saved
            uint32_t nmask = (1u << NB) - 1u;
            if constexpr (!KEEP_PMH) asm volatile("" : "+s"(nmask));
            // 1024 x 8 under the chain without the spread: the first-fit key of a node (pref_miss, node) is
            // loop-invariant, and hoisted out of the container loop its eight register pairs put that variant
            // 12 to 20 bytes into scratch.  The thread index, opaque per container, keeps the keys in the loop:
            // one more VALU operation a node
            uint32_t tn = t;
            if constexpr (FB && !SP && K == 8) asm volatile("" : "+v"(tn));
            auto local_min = [&](auto strat_c, auto relax_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
                constexpr bool RX = decltype(relax_c)::value;  // the container may relax (FB only)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (K > 1 && (uint32_t)BLK * j >= N) break;  // a slot row past N holds no node (uniform)
                    bool ok;
                    uint32_t hoph = 0;  // hop << 29: the key's high word
                    if constexpr (RX) {
                        // 2.3 under req_{n_hops}; the hop counts the earlier requirements the node misses
                        const uint32_t miss = req & ~lab[j];
                        ok = ((sched >> j) & 1u) && fpd::fits(cpu, mem, 0u, conf, cf[j], mf[j], 0u, cu[j]) &&
                             (miss & keep[3]) == 0u;
                        hoph = ((miss != 0u ? 1u : 0u) + ((miss & keep[0]) != 0u ? 1u : 0u) +
                                ((miss & keep[1]) != 0u ? 1u : 0u) + ((miss & keep[2]) != 0u ? 1u : 0u))
                               << (KEY_HOP_SHIFT - 32);
                    } else {
                        ok = ((sched >> j) & 1u) && fpd::fits(cpu, mem, req, conf, cf[j], mf[j], lab[j], cu[j]);
                    }
                    const uint32_t prim = ST == FP_STRATEGY_SPREAD        ? cnt[j]
                                          : ST == FP_STRATEGY_PACK        ? cf[j] - cpu
                                          : ST == FP_STRATEGY_FILL_LOWEST ? ~cf[j]
                                                                          : 0u;
                    uint32_t hi;
                    if constexpr (PMH_REGS) hi = pmh[j] | (prim >> (32 - NB));
                    else if constexpr (KEEP_PMH) hi = pref_hi(lab[j]) | (prim >> (32 - NB));
                    else hi = (nd[j] & ~nmask) | (prim >> (32 - NB));
                    if constexpr (RX) hi |= hoph;
                    if constexpr (SP) {
                        const uint32_t lo = (prim << NB) | (KEEP_PMH ? nd[j] : nd[j] & nmask);
                        const uint64_t key = ((uint64_t)hi << 32) | lo;
                        best = min64(best, ok ? ((pbits >> j) & 1u ? key : KEY_SKEW) : KEY_NONE);
                    } else {
                        const uint32_t lo = (prim << NB) | (tn + (uint32_t)BLK * j);
                        const uint64_t key = ((uint64_t)hi << 32) | lo;
                        best = min64(best, ok ? key : KEY_NONE);
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
                // a container that requires none of the bits the chain gives up cannot relax (uniform):
                // the 2.6 loop, hop 0 in every key
                if ((req & ~keep[3]) != 0u) by_strategy(std::true_type{});
                else by_strategy(std::false_type{});
            } else {
                // a plain switch at this level, as in k_policy
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
                if (placed && mskew != 0u) {  // every wave: the winner's domain gains one, the mask follows
                    dcnt += lane == (nf & (FP_SPREAD_MAX_DOMAINS - 1u)) ? 1u : 0u;
                    skew_bits();
                }
            }
            if (!placed) ++rejected;
            if constexpr (QT) {
                // lane d's request; what the lanes from 3 up hold is never read
                const uint32_t rq = lane == FP_QUOTA_CPU ? cpu : lane == FP_QUOTA_MEM ? mem : 1u;
                if (placed) qv -= rq;  // u32, wraps; under a cap the test above excludes it
            }
            if (t == 0) {
                a.assign[cb + idx] = placed ? n : FP_NONE;
                a.reason[cb + idx] = (uint8_t)(placed ? FP_REASON_OK : SP && best == KEY_SKEW ? FP_REASON_SKEW : FP_REASON_NOFIT);
                if constexpr (FB) {
                    if (a.hops) a.hops[cb + idx] = (uint8_t)(placed ? (uint32_t)(best >> KEY_HOP_SHIFT) : 0u);
                }
                if constexpr (QT) {
                    if (a.quota_why) a.quota_why[cb + idx] = 0;
                }
            }
        }
    }

    // ---- final node state, cost ----
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t n = t + (uint32_t)BLK * j;
        if (n < N && ((touched >> j) & 1u)) {
            a.cpu_free[nb + n] = cf[j];
            a.mem_free[nb + n] = mf[j];
            a.conflict_used[nb + n] = cu[j];
            if (a.node_count) a.node_count[nb + n] = cnt[j];
        }
    }
    if (a.cost) {
        uint32_t used = (uint32_t)__popc(touched);  // nodes that received a container in either pass
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) used += (uint32_t)__shfl_xor((int)used, o);
        if (NW > 1) {
            __shared__ uint32_t usedw[NW];
            if (lane == 0) usedw[w] = used;
            __syncthreads();
            used = 0;
#pragma unroll
            for (uint32_t ww = 0; ww < NW; ++ww) used += usedw[ww];
        }
        if (t == 0) a.cost[s] = fpd::pack_cost(rejected, used, a.scen_base + s);
    }
    if constexpr (QT) {
        if (t < FP_QUOTA_DIMS && a.quota_used) {  // wave 0's lanes 0..2, each its own dimension
            // what this thread stored between the passes: the usage after the seats.  A dimension that is above
            // its cap there admitted only zero requests: its usage stays
            const uint32_t cap = a.quota[(size_t)s * FP_QUOTA_DIMS + t];
            if (a.quota_used[(size_t)s * FP_QUOTA_DIMS + t] <= cap) a.quota_used[(size_t)s * FP_QUOTA_DIMS + t] = cap - qv;
        }
    }
}

template <bool SP, bool FB, bool QT>
void launch_replan_policy(const ReplanPolicyArgs &a, uint32_t S, uint32_t N, hipStream_t st) {
    if (N <= 64) k_replan_policy<64, 1, SP, FB, QT><<<S, 64, 0, st>>>(a);
    else if (N <= 1024) k_replan_policy<1024, 1, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else if (N <= 2048) k_replan_policy<1024, 2, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else if (N <= 4096) k_replan_policy<1024, 4, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else k_replan_policy<1024, 8, SP, FB, QT><<<S, 1024, 0, st>>>(a);
}
void launch_replan_policy_by(bool sp, bool fb, bool qt, const ReplanPolicyArgs &a, uint32_t S, uint32_t N, hipStream_t st) {
    if (qt) {
        if (sp && fb) launch_replan_policy<true, true, true>(a, S, N, st);
        else if (sp) launch_replan_policy<true, false, true>(a, S, N, st);
        else if (fb) launch_replan_policy<false, true, true>(a, S, N, st);
        else launch_replan_policy<false, false, true>(a, S, N, st);
    } else {
        if (sp && fb) launch_replan_policy<true, true, false>(a, S, N, st);
        else if (sp) launch_replan_policy<true, false, false>(a, S, N, st);
        else launch_replan_policy<false, true, false>(a, S, N, st);  // fb: the caller has one of the three
    }
}

}  // namespace

int fp_dev_replan_batch_policy_impl(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o,
                                    uint8_t *change_out, uint32_t *summary_out) {
    const uint32_t S = b->n_scen, C = b->n_containers, N = b->n_nodes;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (S == 0) return FP_OK;
    if (!o.strategy) return FP_EINVAL;
    if ((uint64_t)b->scen_base + S > 65536ull) return FP_EOVERFLOW;  // SPEC.md 2.4: 16-bit scenario id
    if (N > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    const size_t SC = (size_t)S * C;
    if (SC > 0xFFFFFFFFull) return FP_EOVERFLOW;  // rocprim segmented sort takes u32 sizes
    if (C && (!b->cpu_m || !b->mem_mib || !b->req_labels || !b->conflict || !b->assign || !b->reason || !prev))
        return FP_EINVAL;
    if (C && N && (!b->cpu_free || !b->mem_free || !b->labels || !b->conflict_used || !b->schedulable)) return FP_EINVAL;
    if (C && prev == b->assign) return FP_EINVAL;  // the same buffer read and written
    hipStream_t st = c->stream;
    const bool sp = o.domain && o.max_skew;    // SPEC.md 2.7: either pointer null = no constraint anywhere
    const bool fb = o.relax_mask && o.n_hops;  // SPEC.md 2.8: either pointer null = no fallback anywhere
    const bool qt = o.quota != nullptr;        // SPEC.md 2.10: null = no quota anywhere

    fp_ffd_order fo = {};
    if (C)
        if (int rc = fp_ffd_order_size(c, S, C, 0, &fo)) return rc;
    if (!sp && !fb && !qt) {
        // what fp_replan.hip takes (the bad word, the FFD order, its keep flags), and behind it the second bad
        // word of the zero fill below: reserved here, so that fp_replan.hip's own reserve leaves the arena alone
        if (o.hops && SC)
            if (int rc = fp_ws_reserve(c, 256 + fo.bytes + fp_align256(SC) + 256)) return rc;
        // SPEC.md 2.14 theorem A: no guarantee anywhere is exactly 2.13, and fp_replan.hip's kernels run it.
        // Without a chain every hop is 0 (2.8); quota_used and quota_why are not touched (2.10)
        if (int rc = fp_dev_replan_batch_impl(c, b, prev, o, change_out, summary_out)) return rc;
        if (o.hops && SC) {
            // that call's bad word is its own: the values are checked once more into a word of this call, which
            // the workspace reserved above has room for behind what fp_replan.hip took
            uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
            if (!bad) return FP_ENOMEM;
            FP_HIP(hipMemsetAsync(bad, 0, 4, st));
            k_rp_check<<<grid_for(SC > S ? SC : S, 256), 256, 0, st>>>(o.strategy, S, prev, SC, N, nullptr, nullptr,
                                                                        nullptr, bad, c->d_err);
            FP_HIP(hipGetLastError());
            k_rp_zero_hops<<<grid_for(SC, 256), 256, 0, st>>>(o.hops, SC, bad);
            FP_HIP(hipGetLastError());
        }
        return FP_OK;
    }

    // the bad word and the FFD order; order2 is the sort's input values, free after the sort
    if (int rc = fp_ws_reserve(c, 256 + fo.bytes)) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    {
        const size_t SN = sp ? (size_t)S * N : 0;
        size_t most = SC > S ? SC : S;
        if (SN > most) most = SN;
        k_rp_check<<<grid_for(most, 256), 256, 0, st>>>(o.strategy, S, prev, SC, N, sp ? o.domain : nullptr,
                                                        sp ? o.max_skew : nullptr, fb ? o.n_hops : nullptr, bad, c->d_err);
        FP_HIP(hipGetLastError());
    }
    if (C == 0) {  // nothing to seat or place; quota_used stays as given
        if (b->cost || summary_out) {
            k_rp_empty<<<(S + 255) / 256, 256, 0, st>>>(S, b->scen_base, bad, b->cost, summary_out);
            FP_HIP(hipGetLastError());
        }
        return FP_OK;
    }
    // ---- FFD order ----
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_SORT, &ev);
    if (int rc = fp_ffd_order_run(c, S, C, b->cpu_m, b->mem_mib, nullptr, &fo)) return rc;
    fp_prof_end(c, FP_K_SORT, ev);
    FP_HIP(hipMemcpyAsync(fo.vals_in, fo.order, SC * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));

    // ---- seats, then placement under the policy ----
    ReplanPolicyArgs a;
    a.C = C; a.N = N; a.scen_base = b->scen_base;
    a.order = fo.order;
    a.cpu = b->cpu_m; a.mem = b->mem_mib; a.req = b->req_labels; a.conf = b->conflict;
    a.level = b->level; a.prev = prev;
    a.cpu_free = b->cpu_free; a.mem_free = b->mem_free; a.conflict_used = b->conflict_used;
    a.labels = b->labels; a.schedulable = b->schedulable;
    a.node_count = o.node_count;
    a.strategy = o.strategy; a.preferred = o.preferred;
    a.domain = sp ? o.domain : nullptr; a.max_skew = sp ? o.max_skew : nullptr;
    a.relax_mask = fb ? o.relax_mask : nullptr; a.n_hops = fb ? o.n_hops : nullptr;
    a.assign = b->assign; a.reason = b->reason; a.cost = b->cost;
    a.hops = fb ? o.hops : nullptr;
    a.quota = o.quota; a.quota_used = qt ? o.quota_used : nullptr; a.quota_why = qt ? o.quota_why : nullptr;
    a.order2 = fo.vals_in; a.bad = bad;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    launch_replan_policy_by(sp, fb, qt, a, S, N, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    if (o.hops && !fb) {
        k_rp_zero_hops<<<grid_for(SC, 256), 256, 0, st>>>(o.hops, SC, bad);
        FP_HIP(hipGetLastError());
    }
    if (change_out || summary_out) {
        k_replan_report<<<S, 256, 0, st>>>(C, prev, b->assign, b->reason, b->cpu_m, b->mem_mib, change_out, summary_out, bad);
        FP_HIP(hipGetLastError());
    }
    return FP_OK;
}
