// fp_policy.hip -- scored placement (SPEC.md 2.6): spread / pack / fill-lowest placers and soft
// preferred labels, batched over what-if scenarios, and the same under a hard topology spread
// (SPEC.md 2.7, the PlacementPolicy's SpreadConstraint) and under a fallback chain that gives required
// labels up hop by hop (SPEC.md 2.8, the PlacementPolicy's FallbackPolicy).  One workgroup owns one scenario.
//
// First fit (fp_place.hip, fp_pipe.hip) prunes and pipelines on monotonicity.  A scored rule picks the
// feasible node with the smallest key, on state that changes after every placement, so every container
// needs an argmin over every node: a different kernel.
//
// Per fp_dev_place_batch_policy call (asynchronous, nothing is read back):
//   1. k_policy_check : one word, set when any scenario's strategy is not an fp_strategy value; every
//                       later kernel of the call returns on it before writing (all-or-nothing), and
//                       FP_EINVAL goes into the context's error word.  With a spread constraint,
//                       k_policy_check_domain sets the same word for a domain id of 64 or more in a
//                       scenario whose max_skew is not 0, and with a fallback chain k_policy_check_hops
//                       sets it for an n_hops above FP_FALLBACK_MAX_HOPS
//   2. the radix FFD order (fp_ffd_order.hip): cpu desc, mem desc, index asc per scenario
//   3. k_policy<BLK,K,SP,FB,QT>: the placer (SP: with the spread constraint; launched when the call gives
//                       domain and max_skew.  FB: with the fallback chain; launched when the call gives
//                       relax_mask and n_hops).  The scenario's node state lives in registers for the whole
//                       kernel: thread t of a BLK-thread block owns nodes t + BLK * j, j < K, five
//                       words each (cpu_free, mem_free, conflict_used, count, labels) plus the static
//                       preferred-label miss count, a per-thread schedulable mask and a "touched" mask.
//                       The node arrays are only ever indexed by the unrolled j (a runtime index would
//                       send them to scratch); the winner's update is an unrolled `if (j == J)`.
//
// Per container: each thread takes the min key of its K nodes (an infeasible node is all-ones), the wave
// takes its min across lanes, lane 0 writes it to the wave's LDS slot, ONE barrier, every thread takes
// the min of the per-wave slots, the owner of the winning node updates its registers and thread 0
// stores assign / reason at the container's original index.
//
// One barrier per container suffices because the slots are double-buffered by the parity of the
// reductions run so far.  Reduction r writes buffer r & 1 before barrier B_r and reads it after.  The
// next writer of that buffer is reduction r + 2, and a wave gets there only past B_(r+1), which opens
// only when every wave has arrived at it -- and a wave arrives at B_(r+1) after it has consumed its
// reads of reduction r (the keys of reduction r + 1 depend on the winner of r).  So no write can
// overtake a read of the same buffer (WAR), and B_r orders every write before every read (RAW).  The
// parity counts reductions, not containers: a CYCLE container runs none, and two reductions with only a
// skipped container between them must still use different buffers.
//
// The spread constraint (SP) adds no barrier and no LDS traffic per container, so the argument above
// holds as it stands.  Every wave keeps the 64 domain counts in one register (lane d = domain d), takes
// their minimum with the DPP row operations of the key reduction, and ballots `count - min < max_skew`
// into a wave-uniform mask of the domains that pass; a thread looks its K nodes up in that mask once per
// placement (the mask changes only then), not once per container.  A node that fits and fails the skew
// test contributes KEY_SKEW = KEY_NONE - 1, so the one reduction also tells SKEW from NOFIT.  The key's
// node field carries n << 6 | domain: the same order, and the winner's domain reaches every wave with
// the winner, where each wave adds one to that lane of its own copy.  The only LDS the constraint uses is
// a 66-word table in the prologue (the domain sums of node_count and the eligible-domain mask).
//
// The fallback chain (FB) adds no barrier and no LDS traffic either.  The scenario's cumulative relax
// masks are uniform and live in scalar registers; a node's hop for a container is four compares on
// `req & ~labels` and goes into the key above pref_miss, so the one reduction picks the smallest
// (hop, key) and the winner's hop arrives with the winner.  64 bits are full in the 2.6 layout, but the
// node field needs only 19 of its 26 bits (n << 6 | domain), so the FB variants use
// hop:3 | pref_miss:6 | primary:32 | node:23 -- the same order, and still below KEY_SKEW.  A container
// that requires none of the labels the scenario may give up (uniform over the block) cannot relax and
// skips the hop arithmetic.
//
// The container record (cpu, mem, req, conf, original index, CYCLE flag) is uniform across the block.
// Each wave gathers 64 records at a time into registers (lane l holds record i0 + l, loaded a chunk
// ahead) and broadcasts container u with v_readlane, so the record arrives in scalar registers and no
// lane ever issues a per-container load.
//
// The resource quota (QT; SPEC.md 2.10, the PlacementPolicy's ResourceQuota; launched when the call gives
// quota) is tested on that record before anything else happens to the container: what each dimension still
// admits sits in three lanes of one vector register of every wave and is read like the record, with no LDS
// and no barrier.  A container over a cap is FP_REASON_QUOTA and takes the CYCLE container's way out, a
// uniform continue in front of the reduction.  That makes the number of skipped containers between two
// reductions data-dependent; the parity argument above never counted containers, only reductions, and par
// changes nowhere but behind a barrier.
//
// No device-wide synchronisation, no spin waits, no links: the kernel cannot deadlock and has no guard.
// N <= FP_POLICY_MAX_NODES (1024 threads x 8 nodes): past one workgroup the argmin per dependent
// container would need a grid-wide synchronisation per placement.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>

namespace {

// the 2.6 key layout and the 64-bit cross-lane min, shared with the drain sweep (fp_drain.hip)
using fpd::KEY_NONE;
using fpd::KEY_NODE_BITS;  // key = pref_miss << 58 | primary << 26 | node
using fpd::bcast;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min64;
// the 2.7 and 2.8 layouts (fp_argmin.h): the FB variants' key = hop << 61 | pref_miss << 55 | primary << 23 | node
using fpd::DOM_BITS;
using fpd::KEY_HOP_SHIFT;
using fpd::KEY_NODE_BITS_FB;
using fpd::KEY_SKEW;  // a node that fits by 2.3 and fails the skew test: SKEW, where KEY_NONE says NOFIT
using fpd::min32;
using fpd::wave_min32;
static_assert((1u << DOM_BITS) == FP_SPREAD_MAX_DOMAINS && FP_SPREAD_MAX_DOMAINS == 64, "one domain per lane");
static_assert((uint64_t)FP_POLICY_MAX_NODES << DOM_BITS <= (1ull << KEY_NODE_BITS_FB), "node << 6 | domain fits the node field");
static_assert(FP_FALLBACK_MAX_HOPS == 4 && FP_FALLBACK_MAX_HOPS < (1u << (64 - KEY_HOP_SHIFT)), "the hop fits its field");

__global__ __launch_bounds__(256) void k_policy_check(const uint32_t *__restrict__ strategy, uint32_t S,
                                                      uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) b |= strategy[s] > (uint32_t)FP_STRATEGY_FILL_LOWEST;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0) {
        *bad = any ? 1u : 0u;
        if (any) atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// SPEC.md 2.7: a domain id of FP_SPREAD_MAX_DOMAINS or more in a scenario whose max_skew is not 0.  Runs
// behind k_policy_check on the stream (which initialises the word) and only ever sets it.
__global__ __launch_bounds__(256) void k_policy_check_domain(const uint32_t *__restrict__ domain,
                                                             const uint32_t *__restrict__ max_skew, size_t SN, uint32_t N,
                                                             uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < SN; i += (size_t)gridDim.x * blockDim.x)
        b |= domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS && max_skew[i / N] != 0u;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// SPEC.md 2.8: an n_hops above FP_FALLBACK_MAX_HOPS.  Behind k_policy_check, like the domain check.
__global__ __launch_bounds__(256) void k_policy_check_hops(const uint32_t *__restrict__ n_hops, uint32_t S,
                                                           uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) b |= n_hops[s] > (uint32_t)FP_FALLBACK_MAX_HOPS;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// hops of a call that asks for them without a fallback chain: every winner's hop is 0
__global__ __launch_bounds__(256) void k_policy_zero_hops(uint8_t *__restrict__ hops, size_t n,
                                                          const uint32_t *__restrict__ bad) {
    if (*bad) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) hops[i] = 0;
}

__global__ void k_policy_fill_cost(uint32_t S, uint32_t scen_base, const uint32_t *__restrict__ bad,
                                   uint64_t *__restrict__ cost) {
    if (*bad) return;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) cost[s] = fpd::pack_cost(0, 0, scen_base + s);
}

struct PolicyArgs {
    uint32_t C, N, scen_base;
    const uint32_t *order;                        // [S][C] FFD order (index in the scenario)
    const uint32_t *cpu, *mem, *req, *conf;       // [S][C]
    const uint32_t *level;                        // [S][C] or null
    uint32_t *cpu_free, *mem_free, *conflict_used;  // [S][N] in/out
    const uint32_t *labels;                       // [S][N]
    const uint8_t *schedulable;                   // [S][N]
    uint32_t *node_count;                         // [S][N] in/out or null
    const uint32_t *strategy, *preferred;         // [S]; preferred nullable
    const uint32_t *domain;                       // [S][N] topology domain (SPEC.md 2.7); read by k_policy<.., true>
    const uint32_t *max_skew;                     // [S], 0 = no constraint in that scenario
    uint32_t *assign;                             // [S][C]
    uint8_t *reason;                              // [S][C]
    uint64_t *cost;                               // [S] or null
    const uint32_t *bad;                          // k_policy_check's word
    // SPEC.md 2.8, read by k_policy<.., .., true> only.  Behind everything else, so that the other variants
    // load their arguments from where they always did
    const uint32_t *relax_mask;                   // [S][4] label bits hop h + 1 gives up
    const uint32_t *n_hops;                       // [S], 0 = no fallback in that scenario
    uint8_t *hops;                                // [S][C] or null: the winner's hop
    // SPEC.md 2.10, read by k_policy<.., .., .., true> only, and behind the rest for the same reason
    const uint32_t *quota;                        // [S][3] caps, FP_QUOTA_UNLIMITED = none in that dimension
    uint32_t *quota_used;                         // [S][3] in/out or null (null starts at zero)
    uint8_t *quota_why;                           // [S][C] or null: the mask of the blocking dimensions
};

// SP: the hard topology spread of SPEC.md 2.7 (a.domain and a.max_skew given).  SP = false is 2.6 and
// compiles to what it did before the constraint existed.
// FB: the fallback chain of SPEC.md 2.8 (a.relax_mask and a.n_hops given).  FB = false compiles to what
// it did before the chain existed.
// QT: the resource quota of SPEC.md 2.10 (a.quota given).  QT = false compiles to what it did before the
// quota existed.
template <int BLK, int K, bool SP, bool FB, bool QT>
__global__ __launch_bounds__(BLK) void k_policy(const PolicyArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    if (*a.bad) return;  // an invalid strategy somewhere in the batch: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t s = blockIdx.x, C = a.C, N = a.N;
    const size_t cb = (size_t)s * C, nb = (size_t)s * N;
    const uint32_t strat = a.strategy[s];
    const uint32_t pref = a.preferred ? a.preferred[s] : 0u;

    // ---- the scenario's node state, in registers ----
    // 1024 x 8 under both the spread and the chain is past the 128 registers of a 1024-thread block with
    // pmh in registers of its own: that variant keeps pref_miss in nd[j], above the 23-bit node field (where
    // it sits in the key's high word), and takes the two apart with one more VALU operation a node
    // The quota's one register is one too many for 1024 x 8 under the spread alone as well (28 bytes of
    // scratch): with QT that variant packs the same way, above its 26-bit node field
    constexpr bool KEEP_PMH = !((FB || QT) && SP && K == 8);
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[KEEP_PMH ? K : 1];  // pmh = pref_miss << NB: the key's high word
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
        if constexpr (KEEP_PMH) pmh[j] = pref_hi(lab[j]);
    }

    // ---- SPEC.md 2.8.  keep[h] = ~cum[h + 1], uniform: the required bits hop h + 1 still asks for.  Entries
    // past n_hops repeat the last one, so keep[3] is the test under req_{n_hops} whatever n_hops is, and a
    // node's hop is the number of h in 0..3 whose requirement it misses.  n_hops was checked before this
    // kernel; the clamp keeps the loop at four whatever the memory holds ----
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

    // ---- SPEC.md 2.7.  nd[j] = n << 6 | domain(n) is the key's node field of each owned node.  Every wave
    // keeps its own copy of the domain counts in one register: lane d = dom_count[d], all-ones in a domain
    // without a schedulable node (no feasible node is in one, so what its lane says never matters).  After
    // every placement the wave takes the minimum (DPP), the ballot of `count - min < max_skew` is the
    // wave-uniform mask of the domains that pass, and each thread looks up its K nodes in it: bit j of
    // pbits = node j passes.  v_bfe_u32 reads the low five bits of its offset operand, so it takes nd[j] as
    // it is; h5 (bit j = domain(j) >= 32) picks the mask's word.  Nothing per node is derived from the
    // domain alone, which the compiler would hoist into K more registers ----
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
            __shared__ uint32_t dtab[FP_SPREAD_MAX_DOMAINS + 2];  // counts, then the eligible mask's two words
            for (uint32_t i = t; i < FP_SPREAD_MAX_DOMAINS + 2; i += (uint32_t)BLK) dtab[i] = 0u;
            __syncthreads();
            uint32_t e0 = 0, e1 = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t n = t + (uint32_t)BLK * j;
                if (n < N) {
                    // k_policy_check_domain refused a value >= 64 before this kernel; the mask keeps the
                    // LDS index in bounds whatever the memory holds
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
            __syncthreads();
            const bool elig = (dtab[FP_SPREAD_MAX_DOMAINS + (lane >> 5)] >> (lane & 31u)) & 1u;
            dcnt = elig ? dtab[lane] : ~0u;
            skew_bits();
        }
    }

    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0, rejected = 0;  // rejected is the same in every thread

    // ---- SPEC.md 2.10.  The quota's state is uniform, and it lives where the container records live: in the
    // lanes of one vector register of every wave.  Lane d < 3 of qv holds what dimension d still admits,
    // cap - used (0 when used is above the cap on entry: every non-zero request blocks), and v_readlane brings
    // it to a scalar register for the test, as it brings the record.  "r != 0 and not (used <= cap and
    // r <= cap - used)" is then r > qv[d].  qlim (scalar, fixed for the kernel) has bit d set when dimension d
    // has a cap.  A placement takes r from qv[d] in every dimension, capped or not: modulo 2^32 that is
    // used += r, and the epilogue gets the usage back as cap - qv[d].
    // Three scalars carried round the container loop would be the obvious home.  The compiler moves them to
    // three vector registers: the loop's skip paths (CYCLE, QUOTA) give the structurised loop phis with an
    // undefined input, which instruction selection materialises in a vector register, and a scalar phi with
    // a vector input is rewritten for the vector unit with everything computed from it ----
    uint32_t qv = 0, qlim = 0;
    if constexpr (QT) {
        uint32_t cap = FP_QUOTA_UNLIMITED, use = 0;
        if (lane < FP_QUOTA_DIMS) {
            cap = a.quota[(size_t)s * FP_QUOTA_DIMS + lane];
            if (a.quota_used) use = a.quota_used[(size_t)s * FP_QUOTA_DIMS + lane];
        }
        qv = use <= cap ? cap - use : 0u;
        qlim = (uint32_t)__ballot(cap != FP_QUOTA_UNLIMITED);
    }
    auto q_blocks = [&](uint32_t d, uint32_t r) { return ((qlim >> d) & 1u) != 0u && r > bcast(qv, d); };

    // ---- container records, 64 per chunk, one chunk ahead ----
    const uint32_t *ord = a.order + cb;
    auto ld_ord = [&](uint32_t i) -> uint32_t { return i < C ? ord[i] : 0u; };
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;  // r_idx = FP_NONE: a CYCLE container
    auto gather = [&](uint32_t i, uint32_t o) {
        const bool in = i < C;
        r_cpu = in ? a.cpu[cb + o] : 0u;
        r_mem = in ? a.mem[cb + o] : 0u;
        r_req = in ? a.req[cb + o] : 0u;
        r_conf = in ? a.conf[cb + o] : 0u;
        r_idx = in && a.level && a.level[cb + o] == FP_NONE ? FP_NONE : o;
        if (in && r_idx == FP_NONE && w == 0) {  // CYCLE: reported here, skipped below
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
            if (idx == FP_NONE) { ++rejected; continue; }  // CYCLE (uniform)
            const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

            // ---- SPEC.md 2.10: admission before scheduling.  A QUOTA container leaves like a CYCLE one, by a
            // uniform continue before the reduction: no barrier, and par stays, so the parity still counts
            // reductions (the header's argument) however the skipped containers fall ----
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
            auto local_min = [&](auto strat_c, auto relax_c) {
                constexpr uint32_t ST = decltype(strat_c)::value;
                constexpr bool RX = decltype(relax_c)::value;  // the container may relax (FB only)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    // a slot row past N holds no node (uniform): N = 5000 evaluates 5 of K = 8 rows.
                    // The kernel is bound by VALU issue (4 waves a SIMD, ~18 instructions a node)
                    if (K > 1 && (uint32_t)BLK * j >= N) break;
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
                    if constexpr (KEEP_PMH) hi = pmh[j] | (prim >> (32 - NB));
                    else hi = (nd[j] & ~nmask) | (prim >> (32 - NB));
                    if constexpr (RX) hi |= hoph;
                    if constexpr (SP) {
                        // the node field carries n << 6 | domain: the same order (the domain is a function
                        // of n), and the winner's domain reaches every thread with the winner
                        const uint32_t lo = (prim << NB) | (KEEP_PMH ? nd[j] : nd[j] & nmask);
                        const uint64_t key = ((uint64_t)hi << 32) | lo;
                        best = min64(best, ok ? ((pbits >> j) & 1u ? key : KEY_SKEW) : KEY_NONE);
                    } else {
                        const uint32_t lo = (prim << NB) | (t + (uint32_t)BLK * j);
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
                // The same switch as by_strategy, spelled out on purpose: keep it a plain switch at this
                // level.  Routed through the lambda, the compiler laid the SP = true kernels out
                // differently (branches where the selects were) and they measured 1 to 4 % slower; written
                // like this the FB = false kernels are, instruction for instruction, the kernels from
                // before the chain existed.  After a change here, compare their assembly
                // and their time with the build before it
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
        uint32_t used = (uint32_t)__popc(touched);
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
            // a dimension above its cap on entry admitted only zero requests: its usage stays
            const uint32_t cap = a.quota[(size_t)s * FP_QUOTA_DIMS + t];
            if (a.quota_used[(size_t)s * FP_QUOTA_DIMS + t] <= cap) a.quota_used[(size_t)s * FP_QUOTA_DIMS + t] = cap - qv;
        }
    }
}

template <bool SP, bool FB, bool QT>
void launch_policy(const PolicyArgs &a, uint32_t S, uint32_t N, hipStream_t st) {
    if (N <= 64) k_policy<64, 1, SP, FB, QT><<<S, 64, 0, st>>>(a);
    else if (N <= 1024) k_policy<1024, 1, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else if (N <= 2048) k_policy<1024, 2, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else if (N <= 4096) k_policy<1024, 4, SP, FB, QT><<<S, 1024, 0, st>>>(a);
    else k_policy<1024, 8, SP, FB, QT><<<S, 1024, 0, st>>>(a);
}
template <bool QT>
void launch_policy_by(bool sp, bool fb, const PolicyArgs &a, uint32_t S, uint32_t N, hipStream_t st) {
    if (sp && fb) launch_policy<true, true, QT>(a, S, N, st);
    else if (sp) launch_policy<true, false, QT>(a, S, N, st);
    else if (fb) launch_policy<false, true, QT>(a, S, N, st);
    else launch_policy<false, false, QT>(a, S, N, st);
}

}  // namespace

int fp_dev_place_batch_policy_impl(fp_ctx *c, const fp_batch *b, const fp_policy_opts &o) {
    const uint32_t S = b->n_scen, C = b->n_containers, N = b->n_nodes;
    c->last_rng = nullptr;  // a placement call starts with nothing run (fp_ctx_place_path)
    if (S == 0) return FP_OK;
    if (!o.strategy) return FP_EINVAL;
    if ((uint64_t)b->scen_base + S > 65536ull) return FP_EOVERFLOW;  // SPEC.md 2.4: 16-bit scenario id
    if (N > FP_POLICY_MAX_NODES) return FP_EOVERFLOW;
    const size_t SC = (size_t)S * C;
    if (SC > 0xFFFFFFFFull) return FP_EOVERFLOW;  // rocprim segmented sort takes u32 sizes
    if (C && (!b->cpu_m || !b->mem_mib || !b->req_labels || !b->conflict || !b->assign || !b->reason)) return FP_EINVAL;
    if (C && N && (!b->cpu_free || !b->mem_free || !b->labels || !b->conflict_used || !b->schedulable)) return FP_EINVAL;
    hipStream_t st = c->stream;
    const bool sp = o.domain && o.max_skew;  // SPEC.md 2.7: either pointer null = no constraint anywhere
    const bool fb = o.relax_mask && o.n_hops;  // SPEC.md 2.8: either pointer null = no fallback anywhere
    const bool qt = o.quota != nullptr;    // SPEC.md 2.10: null = no quota anywhere; any u32 is a legal cap

    fp_ffd_order fo = {};
    if (C)
        if (int rc = fp_ffd_order_size(c, S, C, 0, &fo)) return rc;
    if (int rc = fp_ws_reserve(c, 256 + fo.bytes)) return rc;  // the bad word, the FFD order
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    k_policy_check<<<1, 256, 0, st>>>(o.strategy, S, bad, c->d_err);
    FP_HIP(hipGetLastError());
    if (sp && N) {
        k_policy_check_domain<<<grid_for((size_t)S * N, 256), 256, 0, st>>>(o.domain, o.max_skew, (size_t)S * N, N, bad,
                                                                            c->d_err);
        FP_HIP(hipGetLastError());
    }
    if (fb) {
        k_policy_check_hops<<<1, 256, 0, st>>>(o.n_hops, S, bad, c->d_err);
        FP_HIP(hipGetLastError());
    }
    if (C == 0) {  // nothing to place: every scenario costs (0 rejected, 0 nodes used)
        if (b->cost) {
            k_policy_fill_cost<<<(S + 255) / 256, 256, 0, st>>>(S, b->scen_base, bad, b->cost);
            FP_HIP(hipGetLastError());
        }
        return FP_OK;
    }
    // ---- FFD order ----
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_SORT, &ev);
    if (int rc = fp_ffd_order_run(c, S, C, b->cpu_m, b->mem_mib, nullptr, &fo)) return rc;
    fp_prof_end(c, FP_K_SORT, ev);

    // ---- placement ----
    PolicyArgs a;
    a.C = C; a.N = N; a.scen_base = b->scen_base;
    a.order = fo.order;
    a.cpu = b->cpu_m; a.mem = b->mem_mib; a.req = b->req_labels; a.conf = b->conflict;
    a.level = b->level;
    a.cpu_free = b->cpu_free; a.mem_free = b->mem_free; a.conflict_used = b->conflict_used;
    a.labels = b->labels; a.schedulable = b->schedulable;
    a.node_count = o.node_count;
    a.strategy = o.strategy; a.preferred = o.preferred;
    a.domain = sp ? o.domain : nullptr; a.max_skew = sp ? o.max_skew : nullptr;
    a.relax_mask = fb ? o.relax_mask : nullptr; a.n_hops = fb ? o.n_hops : nullptr;
    a.assign = b->assign; a.reason = b->reason; a.cost = b->cost;
    a.hops = fb ? o.hops : nullptr;
    a.quota = o.quota; a.quota_used = qt ? o.quota_used : nullptr; a.quota_why = qt ? o.quota_why : nullptr;
    a.bad = bad;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    if (qt) launch_policy_by<true>(sp, fb, a, S, N, st);
    else launch_policy_by<false>(sp, fb, a, S, N, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    if (o.hops && !fb) {
        k_policy_zero_hops<<<grid_for(SC, 256), 256, 0, st>>>(o.hops, SC, bad);
        FP_HIP(hipGetLastError());
    }
    return FP_OK;
}
