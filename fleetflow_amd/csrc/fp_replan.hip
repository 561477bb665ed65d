// fp_replan.hip -- re-planning a running stage (SPEC.md 2.13): every container that still fits the node it
// runs on keeps it (pass 1, seats), the others are placed by the scored rule of SPEC.md 2.6 on the state the
// seats left (pass 2), batched over what-if scenarios.  One workgroup owns one scenario.
//
// Per fp_dev_replan_batch call (asynchronous, nothing is read back):
//   1. k_replan_check : behind a memset of the call's "bad" word; sets it for a strategy that is no fp_strategy
//                       value and for a prev[c] that is neither < N nor FP_NONE, and FP_EINVAL in the context's
//                       error word.  Every later kernel that writes returns on the word first (all-or-nothing)
//   2. the radix FFD order (fp_ffd_order.hip): cpu desc, mem desc, index asc per scenario
//   3. k_replan<BLK,K>: both passes.  Built the way k_policy is (fp_policy.hip): the scenario's node state in
//                       registers for the whole kernel (thread t owns nodes t + BLK * j, indexed by the unrolled
//                       j only; the update is an unrolled `if (j == J)`), container records gathered 64 per
//                       wave a chunk ahead and broadcast with v_readlane.
//
// Pass 1 walks the containers in the 2.3 order.  The record and prev are uniform, so every thread knows the
// owner of node prev: that one thread tests its registers (the 2.3 predicate without `schedulable`), updates
// them, and stores assign / reason / change of a kept container.  No reduction and no barrier per container:
// a seat depends only on the earlier seats of the same node, and those sit in the same thread's registers.
// The owner also stores one byte, keep[i] (i = the container's position in the visiting order), in a flag array
// of the context's workspace: 1 kept, 0 seat lost.  Owners of different nodes store different bytes; a position
// without an owner (CYCLE, prev == FP_NONE) is never stored and never loaded.
//
// One __syncthreads() separates the passes: it orders the owners' flag stores before the loads below (same
// workgroup, so the barrier's workgroup-scope release / acquire covers global memory).
//
// Pass 2 gathers the records again, with keep[i], and is k_policy's loop without the spread constraint, the
// fallback chain and the quota: each thread's min key over its K nodes, the wave min by DPP, lane 0 to the
// wave's LDS slot, ONE barrier, the min of the slots, the winner's owner updates its registers, thread 0 stores.
// A kept container leaves like a CYCLE one: its record arrives with the index FP_NONE and it takes the uniform
// `continue` in front of the reduction.
//
// The slots are double-buffered by the parity of the REDUCTIONS run so far, as in k_policy (the argument is in
// fp_policy.hip's header): reduction r writes buffer r & 1 before barrier B_r and reads it after; the next
// writer of that buffer is reduction r + 2, which a wave reaches only past B_(r+1), and every wave arrives at
// B_(r+1) after its reads of reduction r.  The skip path changes nothing in that: `par` is toggled nowhere but
// behind a barrier, so however many kept or CYCLE containers lie between two reductions -- none, a run of odd
// or even length, whole chunks -- consecutive reductions use different buffers and the same two barriers
// separate a buffer's reads from its next write.  The barrier between the passes is in front of reduction 0.
//
// The change counts and the migration volume are uniform.  They live in the lanes of one vector register of
// every wave (lane d = summary word d), the way k_policy keeps its quota: scalars carried round a loop with skip
// paths end up in vector registers one each.  KEPT and the CYCLE containers are counted a chunk
// at a time by ballot, the placed and rejected ones as they are decided.  Lanes 0..7 of wave 0 store the row.
//
// No device-wide synchronisation, no spin waits: the kernel cannot deadlock and has no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
#include <type_traits>

namespace {

using fpd::KEY_NODE_BITS;
using fpd::KEY_NONE;
using fpd::bcast;
using fpd::min64;
using fpd::row_min64;
using fpd::wave_min64;

static_assert(FP_REPLAN_KEPT == FP_CHANGE_KEPT && FP_REPLAN_NEW == FP_CHANGE_NEW && FP_REPLAN_MOVED == FP_CHANGE_MOVED &&
                  FP_REPLAN_LOST == FP_CHANGE_LOST && FP_REPLAN_ABSENT == FP_CHANGE_ABSENT && FP_REPLAN_WORDS == 8,
              "summary word d counts change value d");

// behind a memset of *bad on the stream; only ever sets it
__global__ __launch_bounds__(256) void k_replan_check(const uint32_t *__restrict__ strategy, uint32_t S,
                                                      const uint32_t *__restrict__ prev, size_t SC, uint32_t N,
                                                      uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += stride)
        b |= strategy[i] > (uint32_t)FP_STRATEGY_FILL_LOWEST;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < SC; i += stride)
        b |= prev[i] >= N && prev[i] != FP_NONE;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_EINVAL));
    }
}

// a call without containers: every scenario costs (0 rejected, 0 nodes used) and changes nothing
__global__ __launch_bounds__(256) void k_replan_empty(uint32_t S, uint32_t scen_base, const uint32_t *__restrict__ bad,
                                                      uint64_t *__restrict__ cost, uint32_t *__restrict__ summary) {
    if (*bad) return;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (cost) cost[s] = fpd::pack_cost(0, 0, scen_base + s);
    if (summary)
        for (uint32_t d = 0; d < FP_REPLAN_WORDS; ++d) summary[(size_t)s * FP_REPLAN_WORDS + d] = 0u;
}

struct ReplanArgs {
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
    uint32_t *assign;                               // [S][C]
    uint8_t *reason;                                // [S][C]
    uint8_t *change;                                // [S][C] or null
    uint32_t *summary;                              // [S][FP_REPLAN_WORDS] or null
    uint64_t *cost;                                 // [S] or null
    uint8_t *keep;                                  // [S][C] workspace: pass 1's verdict by visiting position
    const uint32_t *bad;                            // k_replan_check's word
};

template <int BLK, int K>
__global__ __launch_bounds__(BLK) void k_replan(const ReplanArgs a) {
    static_assert(BLK % 64 == 0 && (BLK & (BLK - 1)) == 0, "block of whole waves, power of two");
    constexpr uint32_t NW = BLK / 64;
    constexpr uint32_t NB = KEY_NODE_BITS;
    if (*a.bad) return;  // a bad strategy or prev somewhere in the batch: nothing is written
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t s = blockIdx.x, C = a.C, N = a.N;
    const size_t cb = (size_t)s * C, nb = (size_t)s * N;
    const uint32_t strat = a.strategy[s];
    const uint32_t pref = a.preferred ? a.preferred[s] : 0u;

    // ---- the scenario's node state, in registers ----
    uint32_t cf[K], mf[K], cu[K], cnt[K], lab[K], pmh[K];  // pmh = pref_miss << NB: the key's high word
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
        pmh[j] = (uint32_t)__popc(pref & ~lab[j]) << NB;
    }

    // ---- container records, 64 per chunk, one chunk ahead (both passes) ----
    const uint32_t *ord = a.order + cb;
    uint8_t *keep = a.keep + cb;
    auto ld_ord = [&](uint32_t i) -> uint32_t { return i < C ? ord[i] : 0u; };
    uint32_t r_cpu, r_mem, r_req, r_conf, r_idx, r_prev;  // r_idx = FP_NONE: skipped (CYCLE; pass 2: or kept)

    // ================= pass 1: seats =================
    {
        auto gather = [&](uint32_t i, uint32_t o) {
            const bool in = i < C;
            r_cpu = in ? a.cpu[cb + o] : 0u;
            r_mem = in ? a.mem[cb + o] : 0u;
            r_req = in ? a.req[cb + o] : 0u;
            r_conf = in ? a.conf[cb + o] : 0u;
            r_prev = in ? a.prev[cb + o] : FP_NONE;
            r_idx = in && a.level && a.level[cb + o] == FP_NONE ? FP_NONE : o;
        };
        gather(lane, ld_ord(lane));
        uint32_t o_next = ld_ord(64u + lane);
        for (uint32_t i0 = 0; i0 < C; i0 += 64u) {
            const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx, c_prev = r_prev;
            if (i0 + 64u < C) {
                gather(i0 + 64u + lane, o_next);
                o_next = ld_ord(i0 + 128u + lane);
            }
            const uint32_t nu = C - i0 < 64u ? C - i0 : 64u;
            for (uint32_t u = 0; u < nu; ++u) {
                const uint32_t idx = bcast(c_idx, u), pv = bcast(c_prev, u);
                // CYCLE, or no seat to keep (FP_NONE is above every N; so is a value k_replan_check refused,
                // whatever the memory holds) -- uniform
                if (idx == FP_NONE || pv >= N) continue;
                const uint32_t cpu = bcast(c_cpu, u), mem = bcast(c_mem, u), req = bcast(c_req, u), conf = bcast(c_conf, u);
                if ((pv & (uint32_t)(BLK - 1)) == t) {  // the owner of node pv; pv < N <= BLK * K, so J < K
                    const uint32_t J = pv / (uint32_t)BLK;
                    bool kept = false;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((uint32_t)j == J && fpd::fits(cpu, mem, req, conf, cf[j], mf[j], lab[j], cu[j])) {
                            cf[j] -= cpu;
                            mf[j] -= mem;
                            cu[j] |= conf;
                            cnt[j] += 1u;
                            touched |= 1u << j;
                            kept = true;
                        }
                    }
                    keep[i0 + u] = kept ? 1 : 0;
                    if (kept) {
                        a.assign[cb + idx] = pv;
                        a.reason[cb + idx] = (uint8_t)FP_REASON_OK;
                        if (a.change) a.change[cb + idx] = (uint8_t)FP_CHANGE_KEPT;
                    }
                }
            }
        }
    }

    // the owners' keep[] stores, before every load of them below
    __syncthreads();

    // ================= pass 2: placement =================
    __shared__ uint64_t slot[2][NW];
    uint32_t par = 0;
    uint32_t acc = 0;  // lane d < 8: summary word d (the same in every wave)
    uint32_t r_kind;   // per record: 0 to place, else the change value it is counted under
    auto gather = [&](uint32_t i, uint32_t o) {
        const bool in = i < C;
        r_cpu = in ? a.cpu[cb + o] : 0u;
        r_mem = in ? a.mem[cb + o] : 0u;
        r_req = in ? a.req[cb + o] : 0u;
        r_conf = in ? a.conf[cb + o] : 0u;
        r_prev = in ? a.prev[cb + o] : FP_NONE;
        const bool cyc = in && a.level && a.level[cb + o] == FP_NONE;
        // keep[i] was stored exactly where pass 1 had an owner
        const bool kept = in && !cyc && r_prev < N && keep[i] != 0;
        r_kind = cyc ? (r_prev != FP_NONE ? 1u + FP_CHANGE_LOST : 1u + FP_CHANGE_ABSENT) : kept ? 1u + FP_CHANGE_KEPT : 0u;
        r_idx = cyc || kept ? FP_NONE : o;
        if (cyc && w == 0) {  // CYCLE: reported here, skipped below
            a.assign[cb + o] = FP_NONE;
            a.reason[cb + o] = (uint8_t)FP_REASON_CYCLE;
            if (a.change) a.change[cb + o] = (uint8_t)(r_kind - 1u);
        }
    };
    gather(lane, ld_ord(lane));
    uint32_t o_next = ld_ord(64u + lane);

    for (uint32_t i0 = 0; i0 < C; i0 += 64u) {
        const uint32_t c_cpu = r_cpu, c_mem = r_mem, c_req = r_req, c_conf = r_conf, c_idx = r_idx, c_prev = r_prev;
        {  // the chunk's skipped records, counted by ballot: lanes past C hold kind 0
            const uint32_t nk = (uint32_t)__popcll(__ballot(r_kind == 1u + FP_CHANGE_KEPT));
            const uint32_t nl = (uint32_t)__popcll(__ballot(r_kind == 1u + FP_CHANGE_LOST));
            const uint32_t na = (uint32_t)__popcll(__ballot(r_kind == 1u + FP_CHANGE_ABSENT));
            acc += lane == FP_REPLAN_KEPT ? nk : lane == FP_REPLAN_LOST ? nl : lane == FP_REPLAN_ABSENT ? na : 0u;
        }
        if (i0 + 64u < C) {  // the next chunk's records and the order of the one after it
            gather(i0 + 64u + lane, o_next);
            o_next = ld_ord(i0 + 128u + lane);
        }
        const uint32_t nu = C - i0 < 64u ? C - i0 : 64u;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t idx = bcast(c_idx, u);
            // kept or CYCLE (uniform): no reduction, no barrier, and par stays -- the parity counts reductions
            if (idx == FP_NONE) continue;
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
            // ---- what became of it (uniform), counted in the lanes of acc ----
            const bool had = bcast(c_prev, u) != FP_NONE;
            const uint32_t chg = placed ? (had ? FP_CHANGE_MOVED : FP_CHANGE_NEW) : (had ? FP_CHANGE_LOST : FP_CHANGE_ABSENT);
            uint32_t add = lane == chg ? 1u : 0u;
            if (chg == FP_CHANGE_MOVED) add = lane == FP_REPLAN_MOVED_CPU ? cpu : lane == FP_REPLAN_MOVED_MEM ? mem : add;
            acc += add;  // u32, wraps
            if (t == 0) {
                a.assign[cb + idx] = placed ? n : FP_NONE;
                a.reason[cb + idx] = (uint8_t)(placed ? FP_REASON_OK : FP_REASON_NOFIT);
                if (a.change) a.change[cb + idx] = (uint8_t)chg;
            }
        }
    }

    // ---- final node state, summary, cost ----
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
    if (a.summary && t < FP_REPLAN_WORDS) a.summary[(size_t)s * FP_REPLAN_WORDS + t] = t < 7u ? acc : 0u;
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
        // rejected = NOFIT + CYCLE: every container that is LOST or ABSENT
        if (t == 0) a.cost[s] = fpd::pack_cost(bcast(acc, FP_REPLAN_LOST) + bcast(acc, FP_REPLAN_ABSENT), used, a.scen_base + s);
    }
}

void launch_replan(const ReplanArgs &a, uint32_t S, uint32_t N, hipStream_t st) {
    if (N <= 64) k_replan<64, 1><<<S, 64, 0, st>>>(a);
    else if (N <= 1024) k_replan<1024, 1><<<S, 1024, 0, st>>>(a);
    else if (N <= 2048) k_replan<1024, 2><<<S, 1024, 0, st>>>(a);
    else if (N <= 4096) k_replan<1024, 4><<<S, 1024, 0, st>>>(a);
    else k_replan<1024, 8><<<S, 1024, 0, st>>>(a);
}

}  // namespace

int fp_dev_replan_batch_impl(fp_ctx *c, const fp_batch *b, const uint32_t *prev, const fp_policy_opts &o,
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

    fp_ffd_order fo = {};
    if (C)
        if (int rc = fp_ffd_order_size(c, S, C, 0, &fo)) return rc;
    // the bad word, the FFD order, the keep flags
    if (int rc = fp_ws_reserve(c, 256 + fo.bytes + fp_align256(SC))) return rc;
    fp_ws_reset(c);
    uint32_t *bad = (uint32_t *)fp_ws_take(c, 4);
    if (!bad) return FP_ENOMEM;
    FP_HIP(hipMemsetAsync(bad, 0, 4, st));
    k_replan_check<<<grid_for(SC > S ? SC : S, 256), 256, 0, st>>>(o.strategy, S, prev, SC, N, bad, c->d_err);
    FP_HIP(hipGetLastError());
    if (C == 0) {
        if (b->cost || summary_out) {
            k_replan_empty<<<(S + 255) / 256, 256, 0, st>>>(S, b->scen_base, bad, b->cost, summary_out);
            FP_HIP(hipGetLastError());
        }
        return FP_OK;
    }
    // ---- FFD order ----
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_SORT, &ev);
    if (int rc = fp_ffd_order_run(c, S, C, b->cpu_m, b->mem_mib, nullptr, &fo)) return rc;
    fp_prof_end(c, FP_K_SORT, ev);
    uint8_t *keep = (uint8_t *)fp_ws_take(c, SC);
    if (!keep) return FP_ENOMEM;

    // ---- seats, then placement ----
    ReplanArgs a;
    a.C = C; a.N = N; a.scen_base = b->scen_base;
    a.order = fo.order;
    a.cpu = b->cpu_m; a.mem = b->mem_mib; a.req = b->req_labels; a.conf = b->conflict;
    a.level = b->level; a.prev = prev;
    a.cpu_free = b->cpu_free; a.mem_free = b->mem_free; a.conflict_used = b->conflict_used;
    a.labels = b->labels; a.schedulable = b->schedulable;
    a.node_count = o.node_count;
    a.strategy = o.strategy; a.preferred = o.preferred;
    a.assign = b->assign; a.reason = b->reason; a.change = change_out; a.summary = summary_out; a.cost = b->cost;
    a.keep = keep; a.bad = bad;
    fp_prof_begin(c, FP_K_PLACE, &ev);
    launch_replan(a, S, N, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
