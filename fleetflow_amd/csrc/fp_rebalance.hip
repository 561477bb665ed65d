// fp_rebalance.hip -- the rebalance sweep (SPEC.md 2.19): for every victim order (a variant) the seats a live plan
// gives up, one at a time, to bring the skew of a spread constraint back within max_skew, and where each one goes.
// One workgroup owns one variant and shares the one base node table with all the others.
//
// Per fp_dev_rebalance_sweep call (asynchronous, nothing is read back):
//   1. k_rebal_check : sets the call's "bad" word for an assign[c] that is neither < N nor FP_NONE, a victim_order
//                      entry that is neither < C nor FP_NONE and, under a spread constraint, a domain[n] of 64 or
//                      more, and FP_EINVAL in the context's error word (k_shrink_check's pattern); every later
//                      kernel that stores to the caller's memory returns on the word first
//   2. k_rebal_count : only where node_count is absent: node_count[n] = |{c : assign[c] == n}| into the workspace
//   3. k_rebal_sweep<BLK,K,FB>: one workgroup per variant, built the way k_shrink_sweep<BLK,K,true,FB> is
//                      (fp_shrink.hip): the node table in registers (thread t owns nodes t + BLK * j, indexed by
//                      the unrolled j only), the block argmin of fp_argmin.h with the (hop, key) layouts and
//                      KEY_SKEW of fp_policy.hip, the domain counts in one register of every wave (lane d = domain
//                      d), the winner's owner updating its registers.  Without a constraint (domain null or
//                      max_skew 0) nothing is heavy: k_rebal_plain copies the plan into every row and writes zeros.
//
// What a rebalance variant has that a scale-in variant has not:
//   * The pass over the victim order.  Most entries are skipped (their container's domain is not heavy), so the
//     order is taken 64 entries per wave at a time: lane l loads entry i0 + l (one chunk ahead), cur of it and the
//     domain of that node -- two dependent loads per 64 entries, not per entry.  The heavy domains are one 64-bit
//     ballot over the domain lanes, a lane is a candidate when (heavy >> domain) & 1, and the candidates are one
//     more ballot, walked by its lowest set bit.  Only candidate lanes load their container's record.  After a
//     move the heavy mask is taken again and the remaining lanes re-balloted: an unmoved container's domain has
//     not changed, the moved one is dropped by its index (theorem C: it is never heavy again), and no domain
//     becomes heavy through a move (theorem B), so a lane that was no candidate at the chunk's start is none
//     later.  After a rejection the state is what it was and the ballot stands.  The pass ends when the mask is 0
//     or the budget is spent.
//   * Lift and its reversal are done by the source node's owner, who keeps the conflict word it had (a live
//     table's word may lack the victim's bits, so `|= conflict` would not restore it).  Every wave takes the
//     source's one seat out of its copy of the domain counts and puts it back on a rejection, together with the
//     pass bits it saved.
//   * The variant's cur row IS its assign_out row, copied from assign in the prologue and written on a move only.
//     There is no undo log: an attempt is one move or nothing.
//
// Barriers.  Every barrier sits in block-uniform control flow: every wave loads the same 64 entries, the same cur
// words and the same domains, holds the same domain counts, and so computes the same ballots; the block minimum
// `best` is the same in every thread (every row of 16 lanes reduces all 16 slots), hence so are the move count,
// the budget test and the candidate mask that the loops branch on.  Per chunk, in this order:
//     attempts : one barrier each, between the store of slot[par][w] and the loads of slot[par][*]
//     M        : at the chunk's end when it moved something: thread 0's stores to cur are complete before any
//                wave loads cur for the next chunk (a repeated entry reads the row the move wrote)
// The parity argument of fp_policy.hip's header holds for slot: a wave writes slot[par] for reduction r + 2 only
// after it passed the barrier of reduction r + 1, which every wave reaches after its loads of reduction r; M is
// one more barrier between two reductions, which never hurts.  A chunk's loads of cur are consumed by its first
// ballot, before the chunk's first reduction, so thread 0's store behind that reduction cannot overtake them.
//
// No device-wide synchronisation and no spin waits: the kernels cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>

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

// behind a memset of *bad on the stream; only ever sets it.  domain: null, or the [N] domain ids of a call under a
// spread constraint, every one of which has to be below FP_SPREAD_MAX_DOMAINS
__global__ __launch_bounds__(256) void k_rebal_check(const uint32_t *__restrict__ assign, uint32_t C,
                                                     const uint32_t *__restrict__ victim, size_t n_ent, uint32_t N,
                                                     const uint32_t *__restrict__ domain, uint32_t *__restrict__ bad,
                                                     uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride)
        b |= assign[i] >= N && assign[i] != FP_NONE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ent; i += stride)
        b |= victim[i] >= C && victim[i] != FP_NONE;
    if (domain)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
            b |= domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// node_count absent means derived: behind a memset of count[0 .. N) on the stream.  count is workspace, so the
// kernel need not wait for the bad word; the bound test keeps a refused assign value out
__global__ __launch_bounds__(256) void k_rebal_count(const uint32_t *__restrict__ assign, uint32_t C, uint32_t N,
                                                     uint32_t *__restrict__ count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride) {
        const uint32_t n = assign[i];
        if (n < N) atomicAdd(&count[n], 1u);
    }
}

// SPEC.md 2.19's degenerate form: nothing is heavy, every row is the plan and every other result is 0
__global__ __launch_bounds__(256) void k_rebal_plain(const uint32_t *__restrict__ assign, uint32_t C, uint32_t n_var,
                                                     uint32_t *__restrict__ assign_out, uint8_t *__restrict__ hops,
                                                     uint8_t *__restrict__ reason, uint32_t *__restrict__ summary,
                                                     const uint32_t *__restrict__ bad) {
    if (*bad) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)n_var * C;
    for (size_t i = i0; i < n; i += stride) {
        assign_out[i] = assign[i % C];
        if (hops) hops[i] = 0;
        if (reason) reason[i] = 0;
    }
    for (size_t i = i0; i < (size_t)n_var * FP_REBAL_WORDS; i += stride) summary[i] = 0u;
}

struct RebalArgs {
    uint32_t C, N, n_try, strategy, preferred;
    uint32_t max_skew;                                    // not 0
    uint32_t keep[FP_FALLBACK_MAX_HOPS];                  // ~cum[h + 1]; entries past n_hops repeat the last one
    const uint32_t *cpu, *mem, *req, *conf;               // [C]
    const uint32_t *cpu_free, *mem_free, *conflict_used;  // [N] the base table: read only
    const uint32_t *labels;                               // [N]
    const uint8_t *schedulable;                           // [N]
    const uint32_t *node_count;                           // [N]: the caller's, or k_rebal_count's
    const uint32_t *domain;                               // [N]
    const uint32_t *assign;                               // [C]
    const uint32_t *victim;                               // [n_var][n_try]
    const uint32_t *max_moves;                            // [n_var] or null (unlimited)
    uint32_t *assign_out;                                 // [n_var][C]: the variants' cur rows
    uint8_t *hops, *reason;                               // [n_var][C] each, or null
    uint32_t *summary;                                    // [n_var][FP_REBAL_WORDS]
    const uint32_t *bad;
};

// FB: under the fallback chain of SPEC.md 2.8.  The spread constraint of 2.7 is what the sweep is about: always
template <int BLK, int K, bool FB>
__global__ __launch_bounds__(BLK) void k_rebal_sweep(const RebalArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    static_assert(NW == 1 || NW == 16, "one slot per lane of a 16-lane row");
    if (*a.bad) return;  // a bad assign, victim_order or domain value somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t v = blockIdx.x, N = a.N, C = a.C, n_try = a.n_try;
    // the variant's row.  Written and read by this block only, across barriers: no __restrict__, no const
    uint32_t *cur = a.assign_out + (size_t)v * C;
    uint8_t *hops = a.hops ? a.hops + (size_t)v * C : nullptr;
    uint8_t *rsn = a.reason ? a.reason + (size_t)v * C : nullptr;
    const uint32_t *vo = a.victim + (size_t)v * n_try;
    const uint32_t strat = a.strategy, pref = a.preferred, mskew = a.max_skew;

    // ---- the base node table, in registers ----
    // 1024 x 8 has no registers for pmh: pref_miss sits in nd[j], above the node field (where it
    // sits in the key's high word), as in k_shrink_sweep<1024, 8, true, ..>
    constexpr bool KEEP_PMH = K != 8;
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[KEEP_PMH ? K : 1];  // pmh = pref_miss << NB: the key's high word
    uint32_t sched = 0;
    // ---- SPEC.md 2.19 on 2.7: nd[j] = n << 6 | domain(n) is the key's node field of each owned node; lane d of
    // draw = dom_count[d] of the variant's state, over all nodes of the domain; elig (lane d) = domain d has a
    // schedulable node, fixed for the call; bit j of pbits = node j's domain passes the skew test, h5 bit j =
    // domain(j) >= 32 (k_policy's skew_bits).  The same in every wave ----
    uint32_t nd[K];
    uint32_t draw = 0, h5 = 0, pbits = ~0u;
    constexpr uint32_t DT_ELIG = FP_SPREAD_MAX_DOMAINS;
    __shared__ uint32_t dtab[DT_ELIG + 2];  // counts, then the eligible mask's two words
    for (uint32_t i = t; i < DT_ELIG + 2; i += (uint32_t)BLK) dtab[i] = 0u;
    __syncthreads();
    {
        uint32_t e0 = 0, e1 = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint32_t n = t + (uint32_t)BLK * j;
            const bool in = n < N;
            cf[j] = in ? a.cpu_free[n] : 0u;
            mf[j] = in ? a.mem_free[n] : 0u;
            cu[j] = in ? a.conflict_used[n] : 0u;
            lab[j] = in ? a.labels[n] : 0u;
            cnt[j] = in ? a.node_count[n] : 0u;
            if (in && a.schedulable[n]) sched |= 1u << j;
            if constexpr (KEEP_PMH) pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
            // k_rebal_check refused a value >= 64 before this kernel; the mask keeps the LDS index in bounds
            // whatever the memory holds
            const uint32_t d = in ? a.domain[n] & (FP_SPREAD_MAX_DOMAINS - 1u) : 0u;
            nd[j] = n << DOM_BITS | d;
            if constexpr (!KEEP_PMH) nd[j] |= (uint32_t)__popc(pref & ~lab[j]) << NB;
            h5 |= (d >> 5) << j;
            if (in && cnt[j]) atomicAdd(&dtab[d], cnt[j]);  // u32, wraps; every node counts, schedulable or not
            if ((sched >> j) & 1u) {
                if (d < 32u) e0 |= 1u << d;
                else e1 |= 1u << (d - 32u);
            }
        }
        if (e0) atomicOr(&dtab[DT_ELIG], e0);
        if (e1) atomicOr(&dtab[DT_ELIG + 1], e1);
    }
    // ---- the variant's own copy of the plan: its result row ----
    for (uint32_t c = t; c < C; c += (uint32_t)BLK) {
        cur[c] = a.assign[c];
        if (hops) hops[c] = 0;  // what every container but a relaxed move keeps
        if (rsn) rsn[c] = (uint8_t)FP_REASON_OK;
    }
    __syncthreads();
    const bool elig = (dtab[DT_ELIG + (lane >> 5)] >> (lane & 31u)) & 1u;
    draw = dtab[lane];

    // pbits from draw (k_policy's skew_bits), and the mask of the heavy domains: eligible, count - min > max_skew
    // (uniform; all 64 lanes active)
    auto eval = [&]() -> uint64_t {
        const uint32_t dc = elig ? draw : ~0u;  // a domain without a schedulable node holds no minimum
        const uint32_t mn = wave_min32(dc);
        const uint64_t m = __ballot(dc - mn < mskew);
        uint32_t x = 0, y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            x |= __builtin_amdgcn_ubfe((uint32_t)m, nd[j], 1u) << j;
            y |= __builtin_amdgcn_ubfe((uint32_t)(m >> 32), nd[j], 1u) << j;
        }
        pbits = (x & ~h5) | (y & h5);
        return __ballot(elig && draw - mn > mskew);
    };
    // SPEC.md 2.19's skew(S): max - min of the counts over the eligible domains, 0 without one (uniform)
    auto skew_of = [&]() -> uint32_t {
        const uint32_t mx = ~wave_min32(elig ? ~draw : ~0u);
        const uint32_t mn = wave_min32(elig ? draw : ~0u);
        return __ballot(elig) != 0ull ? mx - mn : 0u;
    };

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0;
    // the same in every thread
    uint32_t moves = 0, stuck = 0, stuck_skew = 0, relaxed = 0, m_cpu = 0, m_mem = 0;
    const uint32_t budget = a.max_moves ? a.max_moves[v] : FP_NONE;  // moves <= C < FP_NONE: all-ones never ends it
    const uint32_t skew_before = skew_of();
    uint64_t heavy = eval();

    uint32_t e_next = lane < n_try ? vo[lane] : FP_NONE;
    for (uint64_t i0 = 0; i0 < n_try && heavy != 0ull && moves != budget; i0 += 64u) {
        // ---- 64 entries: the entry (loaded a chunk ahead), cur of it, the domain of that node ----
        const uint32_t ent = e_next;
        {
            const uint64_t i = i0 + 64u + lane;
            e_next = i < n_try ? vo[i] : FP_NONE;
        }
        const uint32_t s_l = ent < C ? cur[ent] : FP_NONE;  // FP_NONE: skipped (k_rebal_check refused every other value)
        const bool seated = s_l < N;
        const uint32_t dm = seated ? a.domain[s_l] & (FP_SPREAD_MAX_DOMAINS - 1u) : 0u;
        bool cand = seated && ((heavy >> dm) & 1ull) != 0ull;
        // only a candidate's record is ever broadcast, and a lane that is none now is none later in the chunk
        const uint32_t c_cpu = cand ? a.cpu[ent] : 0u, c_mem = cand ? a.mem[ent] : 0u;
        const uint32_t c_req = cand ? a.req[ent] : 0u, c_conf = cand ? a.conf[ent] : 0u;
        uint64_t pend = __ballot(cand);  // uniform: every wave holds the same chunk
        bool chunk_moved = false;

        while (pend != 0ull && moves != budget) {
            const uint32_t u = (uint32_t)__builtin_ctzll(pend);
            const uint32_t idx = bcast(ent, u), s = bcast(s_l, u), ds = bcast(dm, u);
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // ---- lift: the source's owner gives the request back and keeps the conflict word it had; every
            // wave takes the seat out of its domain counts ----
            const bool own_s = (s & (uint32_t)(BLK - 1)) == t;
            const uint32_t Js = s / (uint32_t)BLK;
            uint32_t sv_cu = 0;
            if (own_s) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if ((uint32_t)j == Js) {
                        cf[j] += cpu;
                        mf[j] += mem;
                        sv_cu = cu[j];
                        cu[j] &= ~conf;
                        cnt[j] -= 1u;
                    }
                }
            }
            const uint32_t sv_pbits = pbits;
            draw -= lane == ds ? 1u : 0u;
            eval();

            // ---- this thread's min key (SPEC.md 2.6 under 2.7 and 2.8) ----
            uint64_t best = KEY_NONE;
            // the node field's mask, opaque per attempt: taking nd[j] apart is loop-invariant, and hoisted out of
            // the loop it would cost the K registers that packing saved (k_policy)
            uint32_t nmask = (1u << NB) - 1u;
            if constexpr (!KEEP_PMH) asm volatile("" : "+s"(nmask));
            auto local_min = [&](auto strat_c, auto relax_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
                constexpr bool RX = decltype(relax_c)::value;  // the victim may relax (FB only)
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
                    const uint32_t lo = (prim << NB) | (KEEP_PMH ? nd[j] : nd[j] & nmask);
                    const uint64_t key = ((uint64_t)hi << 32) | lo;
                    best = min64(best, ok ? ((pbits >> j) & 1u ? key : KEY_SKEW) : KEY_NONE);
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
                // a victim that requires none of the bits the chain gives up cannot relax (uniform): the 2.6
                // loop, hop 0 in every key
                if ((req & ~a.keep[3]) != 0u) by_strategy(std::true_type{});
                else by_strategy(std::false_type{});
            } else {
                by_strategy(std::false_type{});
            }

            // ---- wave min, then block min over the per-wave slots ----
            best = wave_min64(best);
            if (NW > 1) {
                if (lane == 0) slot[par][w] = best;
                __syncthreads();
                best = row_min64(slot[par][lane & (NW - 1)]);  // every row of 16 lanes holds all 16 slots
                par ^= 1u;
            }

            if (best >= KEY_SKEW) {
                // ---- rejection: the state is exactly what it was before the lift ----
                if (own_s) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((uint32_t)j == Js) {
                            cf[j] -= cpu;
                            mf[j] -= mem;
                            cu[j] = sv_cu;  // saved, not recomputed: the word may have lacked the victim's bits
                            cnt[j] += 1u;
                        }
                    }
                }
                draw += lane == ds ? 1u : 0u;
                pbits = sv_pbits;  // the counts are what they were, and so are the bits taken from them
                const uint32_t why = best == KEY_SKEW ? FP_REASON_SKEW : FP_REASON_NOFIT;
                ++stuck;
                stuck_skew += why == FP_REASON_SKEW ? 1u : 0u;
                if (t == 0 && rsn) rsn[idx] = (uint8_t)why;
                pend &= pend - 1ull;
            } else {
                // ---- the move ----
                const uint32_t nf = (uint32_t)best & ((1u << NB) - 1u);
                const uint32_t tn = nf >> DOM_BITS;
                draw += lane == (nf & (FP_SPREAD_MAX_DOMAINS - 1u)) ? 1u : 0u;  // every wave: the winner's domain gains one
                heavy = eval();
                if ((tn & (uint32_t)(BLK - 1)) == t) {
                    const uint32_t J = tn / (uint32_t)BLK;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((uint32_t)j == J) {
                            cf[j] -= cpu;
                            mf[j] -= mem;
                            cu[j] |= conf;
                            cnt[j] += 1u;
                        }
                    }
                }
                const uint32_t hop = FB ? (uint32_t)(best >> KEY_HOP_SHIFT) : 0u;
                ++moves;
                relaxed += hop != 0u ? 1u : 0u;
                m_cpu += cpu;  // u32, wraps
                m_mem += mem;
                if (t == 0) {
                    cur[idx] = tn;
                    if (hops) hops[idx] = (uint8_t)hop;
                    if (rsn) rsn[idx] = (uint8_t)FP_REASON_OK;
                }
                chunk_moved = true;
                // the lanes behind u: the moved container's other entries go, and what is no longer heavy
                cand = cand && lane > u && ent != idx && ((heavy >> dm) & 1ull) != 0ull;
                pend = __ballot(cand);
            }
        }
        if (chunk_moved) __syncthreads();  // M
    }

    const uint32_t skew_after = skew_of();
    if (t == 0) {
        uint32_t *row = a.summary + (size_t)v * FP_REBAL_WORDS;
        row[FP_REBAL_MOVES] = moves;
        row[FP_REBAL_STUCK] = stuck;
        row[FP_REBAL_STUCK_SKEW] = stuck_skew;
        row[FP_REBAL_RELAXED] = relaxed;
        row[FP_REBAL_MOVED_CPU] = m_cpu;
        row[FP_REBAL_MOVED_MEM] = m_mem;
        row[FP_REBAL_SKEW_BEFORE] = skew_before;
        row[FP_REBAL_SKEW_AFTER] = skew_after;
    }
}

// launch_shrink's geometries
template <bool FB>
void launch_rebal(const RebalArgs &a, uint32_t n_var, uint32_t N, hipStream_t st) {
    if (N <= 64) k_rebal_sweep<64, 1, FB><<<n_var, 64, 0, st>>>(a);
    else if (N <= 1024) k_rebal_sweep<1024, 1, FB><<<n_var, 1024, 0, st>>>(a);
    else if (N <= 2048) k_rebal_sweep<1024, 2, FB><<<n_var, 1024, 0, st>>>(a);
    else if (N <= 4096) k_rebal_sweep<1024, 4, FB><<<n_var, 1024, 0, st>>>(a);
    else k_rebal_sweep<1024, 8, FB><<<n_var, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_rebalance_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                                const uint32_t *victim_order, uint32_t n_var, uint32_t n_try, const uint32_t *max_moves,
                                uint32_t strategy, uint32_t preferred, const fp_rebalance_opts &o, uint32_t *assign_out,
                                uint8_t *hops_out, uint8_t *reason_out, uint32_t *summary_out) {
    const uint32_t C = cs->n, N = ns->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (N > FP_POLICY_MAX_NODES || n_var > 65535u || C > FP_SHRINK_MAX_CONTAINERS) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (o.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    const bool sp = o.domain && o.max_skew != 0u;    // SPEC.md 2.19: otherwise nothing is heavy, domain is not read
    const bool fb = o.relax_mask && o.n_hops != 0u;  // relax_mask is a HOST array, read here
    if (n_var == 0) return FP_OK;
    if (C && (!fp_has_cont(cs) || !assign || !assign_out)) return FP_EINVAL;
    if (N && !fp_has_nodes(ns)) return FP_EINVAL;
    if ((n_try && !victim_order) || !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;  // every variant reads the same base assignment
    hipStream_t st = c->stream;

    // the bad word, the derived counts
    const bool derive = sp && !o.node_count && N;
    const size_t cnt_bytes = derive ? fp_align256((size_t)N * 4) : 0;
    if (int rc = fp_ws_reserve(c, 256 + cnt_bytes)) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    const size_t n_ent = (size_t)n_var * n_try;
    const size_t n_chk = sp && N > (C > n_ent ? C : n_ent) ? N : C > n_ent ? C : n_ent;
    if (n_chk) {
        k_rebal_check<<<grid_for(n_chk, 256), 256, 0, st>>>(assign, C, victim_order, n_ent, N, sp ? o.domain : nullptr, bad,
                                                            c->d_err);
        FP_HIP(hipGetLastError());
    }
    hipEvent_t ev;
    if (!sp) {
        fp_prof_begin(c, FP_K_PLACE, &ev);
        const size_t most = (size_t)n_var * (C > FP_REBAL_WORDS ? C : FP_REBAL_WORDS);
        k_rebal_plain<<<grid_for(most, 256), 256, 0, st>>>(assign, C, n_var, assign_out, hops_out, reason_out, summary_out,
                                                           bad);
        FP_HIP(hipGetLastError());
        fp_prof_end(c, FP_K_PLACE, ev);
        return FP_OK;
    }
    const uint32_t *count = o.node_count;
    if (derive) {
        uint32_t *dc = (uint32_t *)fp_ws_take(c, cnt_bytes);
        if (!dc) return FP_ENOMEM;
        FP_HIP(hipMemsetAsync(dc, 0, (size_t)N * 4, st));
        if (C) {
            k_rebal_count<<<grid_for(C, 256), 256, 0, st>>>(assign, C, N, dc);
            FP_HIP(hipGetLastError());
        }
        count = dc;
    }

    RebalArgs a;
    a.C = C; a.N = N; a.n_try = n_try; a.strategy = strategy; a.preferred = preferred;
    a.max_skew = o.max_skew;
    fp_keep_masks(o.relax_mask, o.n_hops, fb, a.keep);
    a.cpu = cs->cpu_m; a.mem = cs->mem_mib; a.req = cs->req_labels; a.conf = cs->conflict;
    a.cpu_free = ns->cpu_free; a.mem_free = ns->mem_free; a.conflict_used = ns->conflict_used;
    a.labels = ns->labels; a.schedulable = ns->schedulable;
    a.node_count = count; a.domain = o.domain;
    a.assign = assign; a.victim = victim_order; a.max_moves = max_moves;
    a.assign_out = assign_out; a.hops = hops_out; a.reason = reason_out; a.summary = summary_out;
    a.bad = bad;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    if (fb) launch_rebal<true>(a, n_var, N, st);
    else launch_rebal<false>(a, n_var, N, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
