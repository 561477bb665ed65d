// fp_shrink.hip -- the scale-in sweep (SPEC.md 2.16; under the policy, 2.17): for every release order (a variant) the servers a live
// plan can give back when they are tried one after the other, and the moves that free them.
// One workgroup owns one variant and shares the one base node table and the one FFD order with all the others.
//
// Per fp_dev_shrink_sweep call (asynchronous, nothing is read back):
//   1. k_shrink_check : sets the call's "bad" word for an assign[c] or a try_order entry that is neither < N nor
//                       FP_NONE (and, under a spread constraint, for a domain[n] of 64 or more), and FP_EINVAL
//                       in the context's error word; the sweep kernel, which does every store of the call,
//                       returns on the word first
//   2. the radix FFD order (fp_ffd_order.hip), once for all variants: order[p] = the container at position p of
//                       the 2.3 order (cpu desc, mem desc, index asc)
//   3. k_shrink_sweep<BLK,K>: one workgroup per variant, built the way k_drain_sweep<BLK,K,false,false> is
//                       (fp_drain.hip): the node table in registers (thread t owns nodes t + BLK * j, indexed by
//                       the unrolled j only), evictee records gathered 64 per wave a chunk ahead and broadcast
//                       with v_readlane, the block argmin by DPP row reductions and one parity-double-buffered
//                       LDS slot per wave, the winner's owner updating its registers.
//
// What a variant has that a drain candidate has not:
//   * Its state lives on from attempt to attempt.  Three workspace rows of C words each belong to the variant:
//       cur_p[p]  the node of the container at FFD position p (FP_NONE: not running), written on commit only;
//                 the row is padded with FP_NONE to a whole scan step, so the scan loads without a bound test
//       ev[i]     the FFD positions of the current attempt's evictees, ascending: the 2.3 order
//       mlog[i]   the target that evictee i of the current attempt moved to
//     and rcnt[n] in LDS counts the containers on node n (all-ones: n was released; nothing moves to a released
//     node, so the mark is never incremented).
//   * The evictee list is found per attempt: the block scans cur_p in steps of BLK * SCAN_U positions, wave w
//     taking SCAN_U rows of 64 behind wave w - 1's, so that positions stay ascending; hits are compacted by
//     ballot and prefix popcount, the waves' offsets by one LDS count per wave.  rcnt[n] says how many there
//     are: an empty node skips the scan and the scan stops once all are found.
//   * Undo.  A committed move required (conflict_used & conflict) == 0 on its target, so the bits it set are
//     exactly `conflict` and `&= ~conflict` restores the word; cpu_free and mem_free are restored by adding what
//     was subtracted (u32, exact), node_count by subtracting the 1.  At a blocker every wave reads the log 64
//     moves at a time (target and the evictee's record, by lane), broadcasts them and the target's owner
//     reverses them; the order does not matter, the four updates commute.  cur_p, rcnt and assign_out are
//     written on commit only, so a failed attempt leaves them as they were.
//
// Barriers.  Every barrier sits in block-uniform control flow: the try-order entry n, rcnt[n], the scan's
// running count `nev`, the block minimum `best` (every row of 16 lanes reduces all 16 slots) and hence
// `fail` and the move count are the same in every thread.  Per attempt, in this order:
//     scan steps : one barrier each, between the store of wcnt[spar][w] and the loads of wcnt[spar][*]
//     S          : after the scan (ev is complete before any wave gathers through it)
//     evictees   : one barrier each, between the store of slot[par][w] and the loads of slot[par][*]
//     B1         : after the moves (thread 0's mlog is complete; every thread has read rcnt[n])
//     B2         : after the undo or the commit (cur_p, rcnt, assign_out are complete)
// The parity argument of fp_policy.hip's header holds for both double-buffered arrays, each with a parity of its
// own that is never reset: a wave writes slot[par] for reduction r + 2 only after it passed the barrier of
// reduction r + 1, or, where the attempt ended at r or r + 1, the barriers B1 and B2 and whatever the next
// attempt puts before its first evictee; every wave arrives at any of those only after its loads of reduction r.
// More barriers between two reductions never hurt, and an attempt that ends early ends for all waves at the same
// reduction.  The same holds for wcnt and spar with "scan step" for "reduction".  rcnt[n] is read at the top of
// an attempt and written by the commit: B1 lies between the two within the attempt, B2 between the commit and the
// next attempt's read.
//
// Under the policy (SPEC.md 2.17, fp_dev_shrink_sweep_policy) the same kernel runs as k_shrink_sweep<BLK,K,SP,FB>:
// SP with the tenant's spread constraint, FB with its fallback chain, both as k_drain_sweep<.., SP, FB> and
// k_policy have them (fp_policy.hip's header): the key layouts, KEY_SKEW = KEY_NONE - 1 so that the one reduction
// tells SKEW from NOFIT, nd[j] = n << 6 | domain in the key's node field, skew_bits, the hop above pref_miss in
// the 23-bit-node layout, the shortcut for an evictee that requires none of the relaxable bits, and pref_miss
// packed into nd[j] for 1024 x 8 (here under the constraint with or without the chain; under the chain alone
// that geometry counts pref_miss again for every key).  What is scale-in's own:
//   * The domain state lives on from attempt to attempt, in two registers of every wave, lane d = domain d:
//     draw, the sum of the running node_count over the unreleased nodes of the domain, and dtgt, the number of
//     targets it holds.  The effective count of the skew test is all-ones where dtgt is 0.  The prologue builds
//     both through LDS atomics (dtab), as the drain does, every node counting and every schedulable one a target.
//   * Attempt start.  n's own count leaves and n is no target: n's owner publishes n's running count and
//     domain | was-a-target << 6 in two LDS words, barrier A, and every wave takes them out of its registers.
//   * Undo.  draw and dtgt are restored from the snapshot taken behind barrier A (one register each), on top of
//     the move log; the log's word carries the hop above the 13 bits of the node, so that the commit can write
//     hops_out.
//   * The bound rule.  The attempt's running registers ARE the state the commit would leave (n out, its moves
//     in) and the snapshot IS the state before, so `after` and `before` are two block-uniform skew evaluations
//     on registers, made before B1 when every evictee found a target.  after > max_skew && after > before is a
//     late failure: the undo runs with made == nev and the blocker stays FP_NONE.
// Barriers under the policy.  A sits in block-uniform control flow like the others (the two `continue`s above it
// depend on the try-order entry and rcnt[n] alone) and orders the owner's two stores before every wave's two
// loads.  The next attempt's owner stores again only behind B1 and B2 of this attempt, which every wave reaches
// after its loads: the two words need no parity.  The draw / dtgt updates are register arithmetic on values
// that are the same in every wave (the published words and the block minimum), so the domain state needs no
// barrier of its own, and neither SP nor FB adds LDS traffic per evictee: the parity argument above carries over
// with A as one more barrier between two reductions.  The late failure changes `fail` before B1, from values
// that are the same in every thread, so B1, the undo and B2 stay block-uniform; it ends the attempt at the
// same reduction for all waves (after the last one), as a blocker does.  <.., false, false> is the 2.16 kernel
// and all that fp_dev_shrink_sweep launches; k_shrink_plain_policy derives the three further results of a 2.17
// call without a guarantee from the state bytes that kernel wrote.
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
// SPEC.md 2.17: a move's log word is hop << MLOG_HOP_SHIFT | target
constexpr uint32_t MLOG_HOP_SHIFT = 13;
static_assert(FP_POLICY_MAX_NODES <= (1u << MLOG_HOP_SHIFT), "a node index leaves the log word's high bits to the hop");

constexpr uint32_t SCAN_U = 16;          // rows of 64 positions a wave scans between two barriers
constexpr uint32_t RC_RELEASED = ~0u;    // rcnt of a released node
static_assert((uint64_t)FP_SHRINK_MAX_CONTAINERS + 1024u * SCAN_U <= (1ull << 31), "a padded row's positions stay below 2^31");

// behind a memset of *bad on the stream; only ever sets it.  domain: null, or (SPEC.md 2.17, a call under a
// spread constraint) the [N] domain ids, every one of which has to be below FP_SPREAD_MAX_DOMAINS
__global__ __launch_bounds__(256) void k_shrink_check(const uint32_t *__restrict__ assign, uint32_t C,
                                                      const uint32_t *__restrict__ try_order, size_t n_ent, uint32_t N,
                                                      const uint32_t *__restrict__ domain, uint32_t *__restrict__ bad,
                                                      uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride)
        b |= assign[i] >= N && assign[i] != FP_NONE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ent; i += stride)
        b |= try_order[i] >= N && try_order[i] != FP_NONE;
    if (domain)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
            b |= domain[i] >= (uint32_t)FP_SPREAD_MAX_DOMAINS;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

struct ShrinkArgs {
    uint32_t C, N, n_try, strategy, preferred;
    uint32_t cstride;                                     // cur_p's row length: C rounded up to a whole scan step
    const uint32_t *order;                                // [C] the 2.3 order; null with C == 0
    const uint32_t *cpu, *mem, *req, *conf;               // [C]
    const uint32_t *cpu_free, *mem_free, *conflict_used;  // [N] the base table: read only
    const uint32_t *labels;                               // [N]
    const uint8_t *schedulable;                           // [N]
    const uint32_t *node_count;                           // [N] or null (zeros)
    const uint32_t *assign;                               // [C]
    const uint32_t *try_order;                            // [n_var][n_try]
    uint32_t *cur_p, *ev, *mlog;                          // [n_var][C] each: the variants' workspace rows
    uint32_t *assign_out;                                 // [n_var][C]
    uint8_t *state;                                       // [n_var][N]
    uint32_t *blocker;                                    // [n_var][N] or null
    uint32_t *summary;                                    // [n_var][FP_SHRINK_WORDS]
    const uint32_t *bad;
    // SPEC.md 2.17, read by the SP / FB variants only.  Behind everything else, so that <.., false, false>
    // loads its arguments from where it always did
    const uint32_t *domain;                               // [N] topology domain; read by <.., true, ..>
    uint32_t max_skew;                                    // not 0 in <.., true, ..>
    uint32_t keep[FP_FALLBACK_MAX_HOPS];                  // ~cum[h + 1]; entries past n_hops repeat the last one
    uint8_t *hops;                                        // [n_var][C] or null
    uint8_t *breason;                                     // [n_var][N] or null
    uint32_t *policy;                                     // [n_var][FP_SHRINK_POLICY_WORDS] or null
};

// SPEC.md 2.17 without a guarantee: the sweep was 2.16's; its three further results follow from the state bytes
__global__ __launch_bounds__(256) void k_shrink_plain_policy(size_t n_hops_out, size_t n_state, uint32_t n_var,
                                                             const uint8_t *__restrict__ state, uint8_t *__restrict__ hops,
                                                             uint8_t *__restrict__ breason, uint32_t *__restrict__ policy,
                                                             const uint32_t *__restrict__ bad) {
    if (*bad) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (hops)
        for (size_t i = i0; i < n_hops_out; i += stride) hops[i] = 0;
    if (breason)
        for (size_t i = i0; i < n_state; i += stride)
            breason[i] = (uint8_t)(state[i] == FP_SHRINK_STATE_FAILED ? FP_REASON_NOFIT : FP_REASON_OK);
    if (policy)
        for (size_t i = i0; i < (size_t)n_var * FP_SHRINK_POLICY_WORDS; i += stride) policy[i] = 0u;
}

// SP: under the spread constraint of SPEC.md 2.7 with the bound rule of 2.17.  FB: under the fallback chain of
// 2.8.  Neither: SPEC.md 2.16, and the code it was before 2.17 existed.
template <int BLK, int K, bool SP, bool FB>
__global__ __launch_bounds__(BLK) void k_shrink_sweep(const ShrinkArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = FB ? KEY_NODE_BITS_FB : KEY_NODE_BITS;  // pref_miss sits at bit 32 + NB in both layouts
    static_assert(NW == 1 || NW == 16, "one slot per lane of a 16-lane row");
    if (*a.bad) return;  // a bad assign, try_order or domain value somewhere: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t v = blockIdx.x, N = a.N, C = a.C;
    // the variant's rows.  Written and read by this block only, across barriers: no __restrict__, no const
    uint32_t *cur_p = a.cur_p + (size_t)v * a.cstride, *ev = a.ev + (size_t)v * C, *mlog = a.mlog + (size_t)v * C;
    uint32_t *aout = a.assign_out + (size_t)v * C;
    uint8_t *state = a.state + (size_t)v * N;
    uint32_t *blk = a.blocker ? a.blocker + (size_t)v * N : nullptr;
    const uint32_t *tro = a.try_order + (size_t)v * a.n_try;
    const uint32_t strat = a.strategy, pref = a.preferred;

    // ---- the base node table, in registers ----
    // 1024 x 8 under the policy has no registers for pmh.  Under the spread constraint pref_miss
    // sits in nd[j], above the node field (where it sits in the key's high word), as in k_drain_sweep
    constexpr bool KEEP_PMH = !((SP || FB) && K == 8);
    // 1024 x 8 under the chain alone has no nd[j] to pack into: pref_miss is counted again for every key
    constexpr bool PMH_FLY = FB && !SP && K == 8;
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K];
    uint32_t pmh[KEEP_PMH ? K : 1];  // pmh = pref_miss << NB: the key's high word
    uint32_t sched = 0;
    __shared__ uint32_t rcnt[BLK * K];
    // ---- SPEC.md 2.17 on 2.7: nd[j] = n << 6 | domain(n) is the key's node field of each owned node; lane d of
    // draw = dom_count[d] of the variant's state (unreleased nodes, n of the running attempt left out), lane d of
    // dtgt = the targets domain d holds; bit j of pbits = node j's domain passes the skew test, h5 bit j =
    // domain(j) >= 32 (k_policy's skew_bits).  The same in every wave ----
    uint32_t nd[SP ? K : 1];
    uint32_t draw = 0, dtgt = 0, h5 = 0, pbits = ~0u;
    constexpr uint32_t DT_TGT = FP_SPREAD_MAX_DOMAINS, DT_PUB = 2 * FP_SPREAD_MAX_DOMAINS;
    __shared__ uint32_t dtab[SP ? DT_PUB + 2 : 1];  // counts, targets, the two words an attempt's owner publishes
    uint8_t *hops = nullptr, *brs = nullptr;
    if constexpr (SP || FB) {
        hops = a.hops ? a.hops + (size_t)v * C : nullptr;
        brs = a.breason ? a.breason + (size_t)v * N : nullptr;
    }
    if constexpr (SP) {
        for (uint32_t i = t; i < DT_PUB + 2; i += (uint32_t)BLK) dtab[i] = 0u;
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
        if (in && a.schedulable[n]) sched |= 1u << j;
        if constexpr (KEEP_PMH) pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
        rcnt[n] = 0u;
        if (in) {
            state[n] = (uint8_t)FP_SHRINK_STATE_NEVER;
            if (blk) blk[n] = FP_NONE;
            if constexpr (SP || FB) {
                if (brs) brs[n] = (uint8_t)FP_REASON_OK;
            }
        }
        if constexpr (SP) {
            // k_shrink_check refused a value >= 64 before this kernel; the mask keeps the LDS index in bounds
            // whatever the memory holds
            const uint32_t d = in ? a.domain[n] & (FP_SPREAD_MAX_DOMAINS - 1u) : 0u;
            nd[j] = n << DOM_BITS | d;
            if constexpr (!KEEP_PMH) nd[j] |= (uint32_t)__popc(pref & ~lab[j]) << NB;
            h5 |= (d >> 5) << j;
            if (in && cnt[j]) atomicAdd(&dtab[d], cnt[j]);  // u32, wraps; every node counts, target or not
            if ((sched >> j) & 1u) atomicAdd(&dtab[DT_TGT + d], 1u);
        }
    }
    const uint32_t mskew = a.max_skew;
    auto skew_bits = [&]() {
        const uint32_t dc = dtgt != 0u ? draw : ~0u;  // a domain without a target holds no minimum
        const uint64_t m = __ballot(dc - wave_min32(dc) < mskew);
        uint32_t x = 0, y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            x |= __builtin_amdgcn_ubfe((uint32_t)m, nd[j], 1u) << j;
            y |= __builtin_amdgcn_ubfe((uint32_t)(m >> 32), nd[j], 1u) << j;
        }
        pbits = (x & ~h5) | (y & h5);
    };
    // SPEC.md 2.17's skew(S): max - min of the counts over the domains that hold a target, 0 without one
    // (uniform; all 64 lanes active)
    auto skew_of = [&](uint32_t raw, uint32_t tgt) -> uint32_t {
        const bool elig = tgt != 0u;
        const uint32_t mx = ~wave_min32(elig ? ~raw : ~0u);
        const uint32_t mn = wave_min32(elig ? raw : ~0u);
        return __ballot(elig) != 0ull ? mx - mn : 0u;
    };
    __syncthreads();
    if constexpr (SP) {
        draw = dtab[lane];
        dtgt = dtab[DT_TGT + lane];
        const uint32_t before = skew_of(draw, dtgt);
        if (t == 0 && a.policy) a.policy[(size_t)v * FP_SHRINK_POLICY_WORDS + FP_SHRINK_SKEW_BEFORE] = before;
        skew_bits();
    }
    // ---- the variant's own copy of the plan: by position for the scans, by container for the result ----
    for (uint32_t p = t; p < C; p += (uint32_t)BLK) {
        const uint32_t n = a.assign[a.order[p]];
        cur_p[p] = n;
        if (n < N) atomicAdd(&rcnt[n], 1u);
        aout[p] = a.assign[p];
        if constexpr (SP || FB) {
            if (hops) hops[p] = 0;  // what every container but a relaxed move keeps
        }
    }
    for (uint32_t p = C + t; p < a.cstride; p += (uint32_t)BLK) cur_p[p] = FP_NONE;  // matches no node
    __syncthreads();

    __shared__ uint64_t slot[2][NW];
    __shared__ uint32_t wcnt[2][NW];
    uint32_t par = 0, spar = 0;
    // the same in every thread
    uint32_t released = 0, tried = 0, failed = 0, moves = 0, first_failed = FP_NONE;
    uint32_t n_fskew = 0, n_relaxed = 0;  // SPEC.md 2.17: attempts undone on SKEW, committed moves at a hop >= 1

    for (uint32_t ti = 0; ti < a.n_try; ++ti) {
        const uint32_t n = tro[ti];  // uniform
        if (n >= N) continue;        // FP_NONE: skipped (k_shrink_check refused every other value)
        const uint32_t ne = rcnt[n];
        if (ne == RC_RELEASED) continue;  // released earlier in this order: skipped, not counted
        ++tried;
        // n is no target of its own attempt
        const uint32_t nbit = (n & (uint32_t)(BLK - 1)) == t ? 1u << (n / (uint32_t)BLK) : 0u;
        const uint32_t was = sched & nbit;
        sched &= ~nbit;
        uint32_t nev = 0, made = 0, blocker = FP_NONE;
        bool fail = false;
        // SPEC.md 2.17: the reason of a failure, the relaxed moves of this attempt, the snapshot the undo restores
        uint32_t why = FP_REASON_NOFIT, rel_att = 0, s_draw = 0, s_dtgt = 0;
        if constexpr (SP) {
            // what runs on n is leaving and n is no target: its owner publishes n's running count, its domain
            // and whether it was a target, every wave takes them out of its registers
            if (nbit) {
                uint32_t c_n = 0, d_n = 0;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if ((nbit >> j) & 1u) {
                        c_n = cnt[j];
                        d_n = nd[j] & (FP_SPREAD_MAX_DOMAINS - 1u);
                    }
                }
                dtab[DT_PUB] = c_n;
                dtab[DT_PUB + 1] = d_n | (was ? FP_SPREAD_MAX_DOMAINS : 0u);
            }
            __syncthreads();  // A
            const uint32_t c_n = dtab[DT_PUB], x = dtab[DT_PUB + 1];
            s_draw = draw;
            s_dtgt = dtgt;
            const bool at = lane == (x & (FP_SPREAD_MAX_DOMAINS - 1u));
            draw -= at ? c_n : 0u;
            dtgt -= at ? x >> DOM_BITS : 0u;
            skew_bits();
        }

        if (ne != 0u) {
            // ---- the evictee list: the positions p with cur_p[p] == n, ascending ----
            for (uint32_t base = 0; base < C && nev < ne; base += (uint32_t)BLK * SCAN_U) {
                const uint32_t p0 = base + w * 64u * SCAN_U + lane;
                uint32_t hits = 0, wc = 0;  // bit u of hits: this lane's position of row u is an evictee
#pragma unroll
                for (uint32_t u = 0; u < SCAN_U; ++u) {
                    // no bound test: the row is padded with FP_NONE up to a whole step, and n < N
                    const bool h = cur_p[p0 + u * 64u] == n;
                    hits |= (h ? 1u : 0u) << u;
                    wc += (uint32_t)__popcll(__ballot(h));
                }
                uint32_t before = 0, total = wc;
                if (NW > 1) {
                    if (lane == 0) wcnt[spar][w] = wc;
                    __syncthreads();
                    total = 0;
#pragma unroll
                    for (uint32_t ww = 0; ww < NW; ++ww) {
                        const uint32_t x = wcnt[spar][ww];
                        before += ww < w ? x : 0u;
                        total += x;
                    }
                    spar ^= 1u;
                }
                if (wc != 0u) {  // wave-uniform; most waves of most steps hold no evictee
                    uint32_t off = nev + before;
#pragma unroll
                    for (uint32_t u = 0; u < SCAN_U; ++u) {
                        const bool h = (hits >> u) & 1u;
                        const uint64_t b = __ballot(h);
                        // at most C hits exist, and every one is stored below the number of hits before it
                        if (h) ev[off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = p0 + u * 64u;
                        off += (uint32_t)__popcll(b);
                    }
                }
                nev += total;
            }
            __syncthreads();  // S

            // ---- evictee records, 64 per chunk, one chunk ahead ----
            auto ld_ord = [&](uint32_t i) -> uint32_t { return i < nev ? a.order[ev[i]] : 0u; };
            uint32_t r_cpu, r_mem, r_req, r_conf, r_idx;
            auto gather = [&](uint32_t i, uint32_t o) {
                const bool in = i < nev;
                r_cpu = in ? a.cpu[o] : 0u;
                r_mem = in ? a.mem[o] : 0u;
                r_req = in ? a.req[o] : 0u;
                r_conf = in ? a.conf[o] : 0u;
                r_idx = o;
            };
            gather(lane, ld_ord(lane));
            uint32_t o_next = ld_ord(64u + lane);

            for (uint32_t i0 = 0; i0 < nev && !fail; i0 += 64u) {
                const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx;
                if (i0 + 64u < nev) {  // the next chunk's records and the order of the one after it
                    gather(i0 + 64u + lane, o_next);
                    o_next = ld_ord(i0 + 128u + lane);
                }
                const uint32_t nu = nev - i0 < 64u ? nev - i0 : 64u;
                for (uint32_t u = 0; u < nu; ++u) {
                    const uint32_t idx = bcast(c_idx, u);
                    const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);

                    // ---- this thread's min key (SPEC.md 2.6) ----
                    uint64_t best = KEY_NONE;
                    // the node field's mask, opaque per evictee: taking nd[j] apart is loop-invariant, and hoisted
                    // out of the evictee loop it would cost the K registers that packing saved (k_policy)
                    uint32_t nmask = (1u << NB) - 1u;
                    if constexpr (!KEEP_PMH) asm volatile("" : "+s"(nmask));
                    // opaque per evictee for the same reason: hoisted, the eight counts are the pmh registers again
                    uint32_t prefv = pref;
                    if constexpr (PMH_FLY) asm volatile("" : "+s"(prefv));
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
                            else if constexpr (PMH_FLY) hi = ((uint32_t)__popc(prefv & ~lab[j]) << NB) | (prim >> (32 - NB));
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
                        // a plain switch at this level: the FB = false kernels keep their layout
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
                        if (lane == 0) slot[par][w] = best;
                        __syncthreads();
                        best = row_min64(slot[par][lane & (NW - 1)]);  // every row of 16 lanes holds all 16 slots
                        par ^= 1u;
                    }

                    if (SP ? best >= KEY_SKEW : best == KEY_NONE) {  // the blocker: the attempt ends here, for every thread
                        blocker = idx;
                        fail = true;
                        if constexpr (SP) why = best == KEY_SKEW ? FP_REASON_SKEW : FP_REASON_NOFIT;
                        break;
                    }
                    // ---- the winner ----
                    const uint32_t nf = (uint32_t)best & ((1u << NB) - 1u);
                    const uint32_t tn = SP ? nf >> DOM_BITS : nf;
                    if constexpr (SP) {  // every wave: the winner's domain gains one, the mask follows
                        draw += lane == (nf & (FP_SPREAD_MAX_DOMAINS - 1u)) ? 1u : 0u;
                        skew_bits();
                    }
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
                    if constexpr (FB) {
                        const uint32_t hop = (uint32_t)(best >> KEY_HOP_SHIFT);
                        rel_att += hop != 0u ? 1u : 0u;
                        if (t == 0) mlog[i0 + u] = hop << MLOG_HOP_SHIFT | tn;
                    } else {
                        if (t == 0) mlog[i0 + u] = tn;
                    }
                    ++made;
                }
            }
        }
        if constexpr (SP) {
            // ---- the bound rule: the attempt's running counts are the state the commit would leave, the
            // snapshot the state before the attempt.  A late failure: made == nev, no blocker ----
            if (!fail) {
                const uint32_t after = skew_of(draw, dtgt), before = skew_of(s_draw, s_dtgt);
                if (!(after <= mskew || after <= before)) {
                    fail = true;
                    why = FP_REASON_SKEW;
                }
            }
        }
        __syncthreads();  // B1

        if (fail) {
            // ---- undo: every wave walks the log, the target's owner reverses the move ----
            for (uint32_t i0 = 0; i0 < made; i0 += 64u) {
                const uint32_t i = i0 + lane;
                const bool in = i < made;
                const uint32_t o = in ? a.order[ev[i]] : 0u;
                const uint32_t l_t = in ? (FB ? mlog[i] & ((1u << MLOG_HOP_SHIFT) - 1u) : mlog[i]) : 0u;
                const uint32_t l_cpu = in ? a.cpu[o] : 0u, l_mem = in ? a.mem[o] : 0u, l_conf = in ? a.conf[o] : 0u;
                const uint32_t nu = made - i0 < 64u ? made - i0 : 64u;
                for (uint32_t u = 0; u < nu; ++u) {
                    const uint32_t tn = bcast(l_t, u);
                    const uint32_t cpu = bcast(l_cpu, u), mem = bcast(l_mem, u), conf = bcast(l_conf, u);
                    if ((tn & (uint32_t)(BLK - 1)) == t) {
                        const uint32_t J = tn / (uint32_t)BLK;
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            if ((uint32_t)j == J) {
                                cf[j] += cpu;
                                mf[j] += mem;
                                cu[j] &= ~conf;  // the move required (cu & conf) == 0: it set exactly these bits
                                cnt[j] -= 1u;
                            }
                        }
                    }
                }
            }
            sched |= was;  // n stays a target
            if constexpr (SP) {  // and counts again: the domain registers are what they were
                draw = s_draw;
                dtgt = s_dtgt;
                skew_bits();
                n_fskew += why == FP_REASON_SKEW ? 1u : 0u;
            }
            if (t == 0) {
                state[n] = (uint8_t)FP_SHRINK_STATE_FAILED;
                if (blk) blk[n] = blocker;
                if constexpr (SP || FB) {
                    if (brs) brs[n] = (uint8_t)why;
                }
            }
            ++failed;
            if (first_failed == FP_NONE) first_failed = n;
        } else {
            // ---- commit: the evictees' new nodes, the targets' counts; n is released ----
            for (uint32_t i = t; i < nev; i += (uint32_t)BLK) {
                const uint32_t p = ev[i];
                uint32_t tn = mlog[i];
                if constexpr (FB) {
                    if (hops) hops[a.order[p]] = (uint8_t)(tn >> MLOG_HOP_SHIFT);
                    tn &= (1u << MLOG_HOP_SHIFT) - 1u;
                }
                cur_p[p] = tn;
                aout[a.order[p]] = tn;
                atomicAdd(&rcnt[tn], 1u);
            }
            if (t == 0) {
                rcnt[n] = RC_RELEASED;
                state[n] = (uint8_t)FP_SHRINK_STATE_RELEASED;
                if (blk) blk[n] = FP_NONE;
                if constexpr (SP || FB) {
                    if (brs) brs[n] = (uint8_t)FP_REASON_OK;
                }
            }
            ++released;
            moves += nev;
            if constexpr (FB) n_relaxed += rel_att;
        }
        __syncthreads();  // B2
    }

    // ---- the variant's row: the containers that ended somewhere else ----
    uint32_t moved = 0, m_cpu = 0, m_mem = 0;
    for (uint32_t c = t; c < C; c += (uint32_t)BLK) {
        if (aout[c] != a.assign[c]) {
            ++moved;
            m_cpu += a.cpu[c];  // u32, wraps
            m_mem += a.mem[c];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        moved += (uint32_t)__shfl_xor((int)moved, o);
        m_cpu += (uint32_t)__shfl_xor((int)m_cpu, o);
        m_mem += (uint32_t)__shfl_xor((int)m_mem, o);
    }
    if (NW > 1) {
        __shared__ uint32_t red[3][NW];
        if (lane == 0) {
            red[0][w] = moved;
            red[1][w] = m_cpu;
            red[2][w] = m_mem;
        }
        __syncthreads();
        moved = 0;
        m_cpu = 0;
        m_mem = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < NW; ++ww) {
            moved += red[0][ww];
            m_cpu += red[1][ww];
            m_mem += red[2][ww];
        }
    }
    if (t == 0) {
        uint32_t *row = a.summary + (size_t)v * FP_SHRINK_WORDS;
        row[FP_SHRINK_RELEASED] = released;
        row[FP_SHRINK_TRIED] = tried;
        row[FP_SHRINK_FAILED] = failed;
        row[FP_SHRINK_MOVES] = moves;
        row[FP_SHRINK_MOVED] = moved;
        row[FP_SHRINK_MOVED_CPU] = m_cpu;
        row[FP_SHRINK_MOVED_MEM] = m_mem;
        row[FP_SHRINK_FIRST_FAILED] = first_failed;
    }
    if constexpr (SP || FB) {
        uint32_t after = 0;
        if constexpr (SP) after = skew_of(draw, dtgt);  // no attempt is open: the final state's
        if (t == 0 && a.policy) {
            uint32_t *prow = a.policy + (size_t)v * FP_SHRINK_POLICY_WORDS;
            prow[FP_SHRINK_FAILED_SKEW] = n_fskew;
            prow[FP_SHRINK_RELAXED] = n_relaxed;
            if constexpr (!SP) prow[FP_SHRINK_SKEW_BEFORE] = 0u;
            prow[FP_SHRINK_SKEW_AFTER] = after;
        }
    }
}

template <bool SP, bool FB>
void launch_shrink(const ShrinkArgs &a, uint32_t n_var, uint32_t N, hipStream_t st) {
    if (N <= 64) k_shrink_sweep<64, 1, SP, FB><<<n_var, 64, 0, st>>>(a);
    else if (N <= 1024) k_shrink_sweep<1024, 1, SP, FB><<<n_var, 1024, 0, st>>>(a);
    else if (N <= 2048) k_shrink_sweep<1024, 2, SP, FB><<<n_var, 1024, 0, st>>>(a);
    else if (N <= 4096) k_shrink_sweep<1024, 4, SP, FB><<<n_var, 1024, 0, st>>>(a);
    else k_shrink_sweep<1024, 8, SP, FB><<<n_var, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_shrink_sweep_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *assign,
                             const uint32_t *try_order, uint32_t n_var, uint32_t n_try, uint32_t strategy,
                             uint32_t preferred, const uint32_t *node_count, uint32_t *assign_out, uint8_t *state_out,
                             uint32_t *blocker_out, uint32_t *summary_out, const fp_shrink_policy &pol) {
    const uint32_t C = cs->n, N = ns->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (N > FP_POLICY_MAX_NODES || n_var > 65535u) return FP_EOVERFLOW;
    if (C > FP_SHRINK_MAX_CONTAINERS) return FP_EOVERFLOW;
    if (strategy > (uint32_t)FP_STRATEGY_FILL_LOWEST) return FP_EINVAL;
    if (pol.n_hops > (uint32_t)FP_FALLBACK_MAX_HOPS) return FP_EINVAL;
    const bool sp = pol.domain && pol.max_skew != 0u;   // SPEC.md 2.17: otherwise domain is not read
    const bool fb = pol.relax_mask && pol.n_hops != 0u;  // relax_mask is a HOST array, read here
    if (n_var == 0) return FP_OK;
    if (C && (!fp_has_cont(cs) || !assign || !assign_out)) return FP_EINVAL;
    if (N && (!fp_has_nodes(ns) || !state_out)) return FP_EINVAL;
    if ((n_try && !try_order) || !summary_out) return FP_EINVAL;
    if (C && assign_out == assign) return FP_EINVAL;  // every variant reads the same base assignment
    hipStream_t st = c->stream;

    fp_ffd_order fo = {};
    if (C) {
        if (int rc = fp_ffd_order_size(c, 1, C, 0, &fo)) return rc;
    }
    // the bad word, the FFD order, the variants' three rows
    const size_t row_bytes = fp_align256((size_t)n_var * C * 4);
    const uint32_t step = (N <= 64 ? 64u : 1024u) * SCAN_U;  // launch_shrink's block size
    const uint32_t cstride = (C + step - 1) / step * step;
    const size_t cur_bytes = fp_align256((size_t)n_var * cstride * 4);
    if (int rc = fp_ws_reserve(c, 256 + fo.bytes + cur_bytes + 2 * row_bytes)) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    const size_t n_ent = (size_t)n_var * n_try;
    const size_t n_chk = sp && N > (C > n_ent ? C : n_ent) ? N : C > n_ent ? C : n_ent;
    if (n_chk) {
        k_shrink_check<<<grid_for(n_chk, 256), 256, 0, st>>>(assign, C, try_order, n_ent, N, sp ? pol.domain : nullptr, bad,
                                                             c->d_err);
        FP_HIP(hipGetLastError());
    }

    ShrinkArgs a;
    a.C = C; a.N = N; a.n_try = n_try; a.strategy = strategy; a.preferred = preferred;
    a.cstride = cstride;
    a.order = nullptr; a.cur_p = nullptr; a.ev = nullptr; a.mlog = nullptr;
    hipEvent_t ev;
    if (C) {
        fp_prof_begin(c, FP_K_SORT, &ev);
        if (int rc = fp_ffd_order_run(c, 1, C, cs->cpu_m, cs->mem_mib, nullptr, &fo)) return rc;
        fp_prof_end(c, FP_K_SORT, ev);
        a.order = fo.order;
        a.cur_p = (uint32_t *)fp_ws_take(c, cur_bytes);
        a.ev = (uint32_t *)fp_ws_take(c, row_bytes);
        a.mlog = (uint32_t *)fp_ws_take(c, row_bytes);
        if (!a.cur_p || !a.ev || !a.mlog) return FP_ENOMEM;
    }
    a.cpu = cs->cpu_m; a.mem = cs->mem_mib; a.req = cs->req_labels; a.conf = cs->conflict;
    a.cpu_free = ns->cpu_free; a.mem_free = ns->mem_free; a.conflict_used = ns->conflict_used;
    a.labels = ns->labels; a.schedulable = ns->schedulable;
    a.node_count = node_count; a.assign = assign; a.try_order = try_order;
    a.assign_out = assign_out; a.state = state_out; a.blocker = blocker_out; a.summary = summary_out;
    a.bad = bad;
    a.domain = sp ? pol.domain : nullptr; a.max_skew = sp ? pol.max_skew : 0u;
    fp_keep_masks(pol.relax_mask, pol.n_hops, fb, a.keep);
    a.hops = pol.hops_out; a.breason = pol.blocker_reason_out; a.policy = pol.policy_out;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    fp_with_flags(sp, fb, [&](auto SP, auto FB) {
        launch_shrink<decltype(SP)::value, decltype(FB)::value>(a, n_var, N, st);
    });
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    if (!sp && !fb && (pol.hops_out || pol.blocker_reason_out || pol.policy_out)) {
        // without a guarantee the sweep was 2.16's: zeros, and NOFIT on the nodes whose attempt failed
        const size_t nh = (size_t)n_var * C, nst = (size_t)n_var * N;
        const size_t most = nh > nst ? nh : nst;
        k_shrink_plain_policy<<<grid_for(most > 4 * (size_t)n_var ? most : 4 * (size_t)n_var, 256), 256, 0, st>>>(
            nh, nst, n_var, state_out, pol.hops_out, pol.blocker_reason_out, pol.policy_out, bad);
        FP_HIP(hipGetLastError());
    }
    return FP_OK;
}
