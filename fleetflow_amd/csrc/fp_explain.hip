// fp_explain.hip -- rejection diagnosis (SPEC.md 2.9): a containers x nodes sweep in the family of
// k_feas (fp_feas.hip) that says, per explained container, WHICH of the 2.3 predicates fail on how
// many nodes of the given node state.  Nothing is placed or mutated.
//
//   k_explain<true>   rows: one lane owns one selected container (kPerRows per thread), the node tile
//                     is staged in LDS and read as wave-uniform broadcasts; per node the 5-bit
//                     `why` mask, 5 + 5 + 1 counters, the AND and the minimum.  A row leaves as one
//                     aligned 64-byte store, or -- when a small grid splits the node range over
//                     blockIdx.y -- as atomicAdd / atomicAnd / atomicMin into rows k_explain_rows_init
//                     initialised.
//   k_explain<false>  batch: the histogram needs only ALL and FEASIBLE > 0 of a row, so this
//                     instance carries those six bits (the "digest") and none of the counters.  A
//                     large grid adds each block's histogram contribution once; a split grid
//                     atomicAnds the digest words and k_explain_hist counts the merged words.
//   k_explain_select  batch selection: per scenario the indices of the containers whose reason is
//                     in reason_mask, compacted on the device (order free: the histogram is a sum).
//                     Blocks past a scenario's count leave at once, so lanes work on selected
//                     containers only.
//   k_explain_check   fp_dev_explain: a sel index >= C sets the check word and FP_ECORRUPT; every
//                     later kernel of the call returns on the word before it writes anything.
//
// No kernel waits on another block: every merge is a commutative atomic on an initialised word.
#include "fp_internal.h"

namespace {

constexpr int kBlock = 256;   // threads per block (4 waves)
constexpr int kPerRows = 2;   // containers per thread, rows instance (13 accumulators + 5 inputs each)
constexpr int kPerHist = 4;   // containers per thread, batch instance (2 accumulators each; k_feas carries 4 too)
constexpr int kTile = 1024;   // nodes per LDS chunk
constexpr uint32_t kDigNoFeas = 1u << 5;  // digest: bits 0..4 ALL, bit 5 "no node feasible"
constexpr uint32_t kDigMask = 0x3Fu;

struct alignas(16) NodeRec {
    uint32_t cf, mf, lab, cu;  // lab holds ~labels in the LDS tile
};

struct ExArgs {
    uint32_t C, N, node_span;   // node_span: nodes per blockIdx.y (multiple of 64)
    uint32_t n_sel;             // selected containers (when cnt is null)
    const uint32_t *cnt;        // [S] selected containers per scenario, or null
    const uint32_t *sel;        // [S][C] (stride C per scenario) selected indices, or null = identity
    const uint32_t *ign;        // [S] label bits given up, or null = ign0
    uint32_t ign0;
    // scenario blockIdx.z: containers advance by C per scenario, nodes by N
    const uint32_t *cpu, *mem, *req, *conf;
    const uint32_t *cf, *mf, *lab, *cu;
    const uint8_t *sched;
    const uint32_t *bad;        // k_explain_check's word, or null
    uint32_t *rows;             // [n_sel][16]                (rows instance)
    uint32_t *dig;              // [S][C] digest words        (batch instance, split)
    uint32_t *hist;             // [S][8]                     (batch instance)
    int split;
};

// One block's share of a scenario histogram: ballots per category, one LDS add per wave and
// category, then at most FP_EXPLAIN_HIST_WORDS global atomics for the block.  hsum is zeroed and
// a barrier passed before the call; every thread of the block calls it.
__device__ __forceinline__ void hist_add(bool valid, uint32_t d, uint32_t *hsum, uint32_t *hist) {
    const uint32_t lane = threadIdx.x & 63;
    bool cat[FP_EXPLAIN_HIST_WORDS];
#pragma unroll
    for (int k = 0; k < 5; ++k) cat[k] = valid && ((d >> k) & 1u);
    cat[FP_EXPLAIN_HIST_MIXED] = valid && (d & kDigMask) == kDigNoFeas;
    cat[FP_EXPLAIN_HIST_FITS] = valid && !(d & kDigNoFeas);
    cat[FP_EXPLAIN_HIST_SELECTED] = valid;
#pragma unroll
    for (int k = 0; k < FP_EXPLAIN_HIST_WORDS; ++k) {
        const uint32_t n = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cat[k]));
        if (lane == 0 && n) atomicAdd(&hsum[k], n);
    }
}

template <bool ROWS, int PER>
__global__ __launch_bounds__(kBlock) void k_explain(ExArgs a) {
    __shared__ NodeRec rec[kTile];   // cf, mf, ~lab, cu
    __shared__ uint32_t sch[kTile];
    __shared__ uint32_t hsum[FP_EXPLAIN_HIST_WORDS];
    if (a.bad && *a.bad) return;     // a corrupt sel: nothing is written (block-uniform)
    const uint32_t z = blockIdx.z;
    const uint32_t nsel = a.cnt ? a.cnt[z] : a.n_sel;
    const uint32_t m0 = blockIdx.x * (kBlock * PER);
    if (m0 >= nsel) return;          // past the scenario's compacted list (block-uniform)
    {
        const size_t sc = (size_t)z * a.C, sn = (size_t)z * a.N;
        a.cpu += sc; a.mem += sc; a.req += sc; a.conf += sc;
        if (a.sel) a.sel += sc;
        a.cf += sn; a.mf += sn; a.lab += sn; a.cu += sn; a.sched += sn;
    }
    const uint32_t ign = a.ign ? a.ign[z] : a.ign0;
    if (!ROWS && !a.split) {
        if (threadIdx.x < FP_EXPLAIN_HIST_WORDS) hsum[threadIdx.x] = 0;
        __syncthreads();
    }
    uint32_t cpu[PER], mem[PER], req[PER], conf[PER], midx[PER];
    bool cin[PER];
    uint32_t all[PER], feas[PER], near[PER], fail[PER][5], only[PER][5];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint32_t m = m0 + k * kBlock + threadIdx.x;
        midx[k] = m;
        uint32_t c = 0;
        cin[k] = m < nsel;
        if (cin[k]) c = a.sel ? a.sel[m] : m;
        cin[k] = cin[k] && c < a.C;  // k_explain_check refused such an index; this keeps the loads in bounds
        cpu[k] = cin[k] ? a.cpu[c] : 0u;
        mem[k] = cin[k] ? a.mem[c] : 0u;
        req[k] = cin[k] ? a.req[c] & ~ign : 0u;
        conf[k] = cin[k] ? a.conf[c] : 0u;
        all[k] = 0x1Fu;
        feas[k] = 0;
        near[k] = FP_NONE;
#pragma unroll
        for (int j = 0; j < 5; ++j) fail[k][j] = only[k][j] = 0;
    }
    uint32_t nor = 0xFFFFFFFFu;  // ~(OR of labels over the schedulable nodes of this node range)
    const uint32_t y0 = blockIdx.y * a.node_span;
    const uint32_t y1 = min(a.N, y0 + a.node_span);
    for (uint32_t n0 = y0; n0 < y1; n0 += kTile) {
        const uint32_t len = min((uint32_t)kTile, y1 - n0);
        for (uint32_t i = threadIdx.x; i < len; i += kBlock) {
            NodeRec r;
            r.cf = a.cf[n0 + i]; r.mf = a.mf[n0 + i]; r.lab = ~a.lab[n0 + i]; r.cu = a.cu[n0 + i];
            rec[i] = r;
            sch[i] = a.sched[n0 + i];
        }
        __syncthreads();
        for (uint32_t i = 0; i < len; ++i) {
            const NodeRec r = rec[i];
            const uint32_t s = sch[i];
            const uint32_t cordon = s ? 0u : (uint32_t)FP_WHY_CORDON;  // every bit on every node, cordoned included
            nor &= s ? r.lab : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const uint32_t why = cordon | (r.cf < cpu[k] ? (uint32_t)FP_WHY_CPU : 0u) |
                                     (r.mf < mem[k] ? (uint32_t)FP_WHY_MEM : 0u) |
                                     ((req[k] & r.lab) ? (uint32_t)FP_WHY_LABEL : 0u) |
                                     ((r.cu & conf[k]) ? (uint32_t)FP_WHY_CONFLICT : 0u);
                all[k] &= why;
                feas[k] += why == 0u ? 1u : 0u;
                if (ROWS) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        fail[k][j] += (why >> j) & 1u;
                        only[k][j] += why == (1u << j) ? 1u : 0u;
                    }
                    const bool one = why != 0u && (why & (why - 1u)) == 0u;
                    near[k] = min(near[k], one ? n0 + i : FP_NONE);
                }
            }
        }
        __syncthreads();
    }
    if (ROWS) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!cin[k]) continue;
            uint32_t *row = a.rows + (size_t)midx[k] * FP_EXPLAIN_WORDS;
            if (a.split) {  // into the row k_explain_rows_init wrote: MISSING starts at req'
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    if (fail[k][j]) atomicAdd(&row[FP_EXPLAIN_FAIL + j], fail[k][j]);
                    if (only[k][j]) atomicAdd(&row[FP_EXPLAIN_ONLY + j], only[k][j]);
                }
                if (feas[k]) atomicAdd(&row[FP_EXPLAIN_FEASIBLE], feas[k]);
                if (all[k] != 0x1Fu) atomicAnd(&row[FP_EXPLAIN_ALL], all[k]);
                if (req[k] & ~nor) atomicAnd(&row[FP_EXPLAIN_MISSING], nor);
                if (near[k] != FP_NONE) atomicMin(&row[FP_EXPLAIN_NEAR], near[k]);
            } else {
                uint4 *r4 = (uint4 *)row;  // rows are 64-byte aligned (checked by the entry point)
                r4[0] = make_uint4(fail[k][0], fail[k][1], fail[k][2], fail[k][3]);
                r4[1] = make_uint4(fail[k][4], only[k][0], only[k][1], only[k][2]);
                r4[2] = make_uint4(only[k][3], only[k][4], feas[k], all[k]);
                r4[3] = make_uint4(req[k] & nor, near[k], 0u, 0u);
            }
        }
    } else {
        uint32_t *hist = a.hist + (size_t)z * FP_EXPLAIN_HIST_WORDS;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t d = all[k] | (feas[k] ? 0u : kDigNoFeas);
            if (a.split) {
                if (cin[k] && d != kDigMask) atomicAnd(&a.dig[(size_t)z * a.C + midx[k]], d);
            } else {
                hist_add(cin[k], d, hsum, hist);
            }
        }
        if (!a.split) {
            __syncthreads();
            if (threadIdx.x < FP_EXPLAIN_HIST_WORDS && hsum[threadIdx.x])
                atomicAdd(&hist[threadIdx.x], hsum[threadIdx.x]);
        }
    }
}

// The rows a split k_explain<true> merges into: counters 0, ALL = 0x1F, MISSING = req', NEAR = FP_NONE.
__global__ __launch_bounds__(kBlock) void k_explain_rows_init(ExArgs a) {
    if (a.bad && *a.bad) return;
    const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= a.n_sel) return;
    const uint32_t c = a.sel ? a.sel[m] : m;
    if (c >= a.C) return;
    uint4 *r4 = (uint4 *)(a.rows + (size_t)m * FP_EXPLAIN_WORDS);
    r4[0] = make_uint4(0u, 0u, 0u, 0u);
    r4[1] = make_uint4(0u, 0u, 0u, 0u);
    r4[2] = make_uint4(0u, 0u, 0u, 0x1Fu);
    r4[3] = make_uint4(a.req[c] & ~a.ign0, FP_NONE, 0u, 0u);
}

// fp_dev_explain: any sel index >= C.  `bad` is zeroed on the stream before the launch.
__global__ __launch_bounds__(kBlock) void k_explain_check(const uint32_t *__restrict__ sel, uint32_t n_sel, uint32_t C,
                                                          uint32_t *__restrict__ bad, uint32_t *__restrict__ err) {
    bool b = false;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_sel; i += (size_t)gridDim.x * kBlock)
        b |= sel[i] >= C;
    const bool any = __syncthreads_or(b);
    if (threadIdx.x == 0 && any) {
        atomicOr(bad, 1u);
        atomicMax(err, (uint32_t)(-FP_ECORRUPT));
    }
}

// Batch selection: scenario blockIdx.y, containers blockIdx.x * kBlock ..; list[s][0 .. cnt[s]) receives
// the containers whose reason is in `mask`, one atomicAdd per wave on the scenario's count.
__global__ __launch_bounds__(kBlock) void k_explain_select(const uint8_t *__restrict__ reason, uint32_t C, uint32_t mask,
                                                           uint32_t *__restrict__ list, uint32_t *__restrict__ cnt) {
    const uint32_t s = blockIdx.y, c = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63;
    bool pick = false;
    if (c < C) {
        const uint32_t r = reason[(size_t)s * C + c];
        pick = r < 32u && ((mask >> r) & 1u);
    }
    const uint64_t bal = __builtin_amdgcn_ballot_w64(pick);
    if (bal == 0) return;  // wave-uniform
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&cnt[s], (uint32_t)__popcll(bal));
    base = __shfl(base, 0);
    if (pick) list[(size_t)s * C + base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = c;
}

// The histogram of a split batch call, from the merged digest words.
__global__ __launch_bounds__(kBlock) void k_explain_hist(const uint32_t *__restrict__ dig, const uint32_t *__restrict__ cnt,
                                                         uint32_t C, uint32_t *__restrict__ hist) {
    __shared__ uint32_t hsum[FP_EXPLAIN_HIST_WORDS];
    const uint32_t s = blockIdx.y, m = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t nsel = cnt ? cnt[s] : C;
    if (blockIdx.x * kBlock >= nsel) return;  // block-uniform
    if (threadIdx.x < FP_EXPLAIN_HIST_WORDS) hsum[threadIdx.x] = 0;
    __syncthreads();
    const bool valid = m < nsel;
    hist_add(valid, valid ? dig[(size_t)s * C + m] : 0u, hsum, hist + (size_t)s * FP_EXPLAIN_HIST_WORDS);
    __syncthreads();
    if (threadIdx.x < FP_EXPLAIN_HIST_WORDS && hsum[threadIdx.x])
        atomicAdd(&hist[(size_t)s * FP_EXPLAIN_HIST_WORDS + threadIdx.x], hsum[threadIdx.x]);
}

// node-range split as k_feas: only while the whole grid is small, ranges of a multiple of 64 nodes
void split_plan(uint64_t blocks, uint32_t N, uint32_t *ysplit_out, uint32_t *span_out) {
    uint32_t ysplit = 1;
    const uint32_t max_split = N ? (N + 63) / 64 : 1;
    while (blocks * ysplit < 2048 && ysplit < max_split) ysplit *= 2;
    if (ysplit > max_split) ysplit = max_split;
    uint32_t span = N ? (N + ysplit - 1) / ysplit : 0;
    span = (span + 63) & ~63u;
    if (span == 0) span = 64;
    *ysplit_out = N ? (N + span - 1) / span : 1;
    *span_out = span;
}

}  // namespace

int fp_dev_explain_impl(fp_ctx *c, const fp_containers *cs, const fp_nodes *ns, const uint32_t *sel, uint32_t n_sel,
                        uint32_t ignore_labels, uint32_t *rows) {
    const uint32_t C = cs->n, N = ns->n;
    if (!sel) n_sel = C;
    if (n_sel == 0) return FP_OK;
    if (!cs->cpu_m || !cs->mem_mib || !cs->req_labels || !cs->conflict || !rows) return FP_EINVAL;
    if (((uintptr_t)rows & 63u) != 0) return FP_EINVAL;  // a row is one aligned 64-byte store
    if (N && (!ns->cpu_free || !ns->mem_free || !ns->labels || !ns->conflict_used || !ns->schedulable))
        return FP_EINVAL;
    hipStream_t st = c->stream;
    uint32_t *bad = nullptr;
    if (sel) {
        if (int rc = fp_ws_reserve(c, 256)) return rc;
        fp_ws_reset(c);
        bad = (uint32_t *)fp_ws_take(c, 4);
        if (!bad) return FP_ENOMEM;
        FP_HIP(hipMemsetAsync(bad, 0, 4, st));
        const uint64_t nb = ((uint64_t)n_sel + kBlock - 1) / kBlock;
        const uint32_t cb = nb < 1024 ? (uint32_t)nb : 1024u;  // grid-stride past that
        k_explain_check<<<cb, kBlock, 0, st>>>(sel, n_sel, C, bad, c->d_err);
        FP_HIP(hipGetLastError());
    }
    const uint32_t xb = (uint32_t)(((uint64_t)n_sel + kBlock * kPerRows - 1) / (kBlock * kPerRows));
    uint32_t ysplit, span;
    split_plan(xb, N, &ysplit, &span);
    ExArgs a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.N = N; a.node_span = span; a.n_sel = n_sel; a.sel = sel; a.ign0 = ignore_labels;
    a.cpu = cs->cpu_m; a.mem = cs->mem_mib; a.req = cs->req_labels; a.conf = cs->conflict;
    a.cf = ns->cpu_free; a.mf = ns->mem_free; a.lab = ns->labels; a.cu = ns->conflict_used;
    a.sched = ns->schedulable;
    a.bad = bad; a.rows = rows;
    a.split = ysplit > 1;
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_FEAS, &ev);
    if (a.split) {
        k_explain_rows_init<<<(uint32_t)(((uint64_t)n_sel + kBlock - 1) / kBlock), kBlock, 0, st>>>(a);
        FP_HIP(hipGetLastError());
    }
    k_explain<true, kPerRows><<<dim3(xb, ysplit), kBlock, 0, st>>>(a);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_FEAS, ev);
    return FP_OK;
}

int fp_dev_explain_batch_impl(fp_ctx *c, const fp_batch *b, uint32_t reason_mask, const uint32_t *ignore_labels,
                              uint32_t *hist) {
    const uint32_t S = b->n_scen, C = b->n_containers, N = b->n_nodes;
    if (S == 0) return FP_OK;
    if (S > 65535u) return FP_EOVERFLOW;  // grid z
    if (!hist) return FP_EINVAL;
    if (C && (!b->cpu_m || !b->mem_mib || !b->req_labels || !b->conflict || (reason_mask && !b->reason)))
        return FP_EINVAL;
    if (C && N && (!b->cpu_free || !b->mem_free || !b->labels || !b->conflict_used || !b->schedulable))
        return FP_EINVAL;
    hipStream_t st = c->stream;
    FP_HIP(hipMemsetAsync(hist, 0, (size_t)S * FP_EXPLAIN_HIST_WORDS * 4, st));
    if (C == 0) return FP_OK;
    const size_t SC = (size_t)S * C;
    const uint32_t xb = (C + kBlock * kPerHist - 1) / (kBlock * kPerHist);
    uint32_t ysplit, span;
    split_plan((uint64_t)xb * S, N, &ysplit, &span);
    const bool split = ysplit > 1;
    // workspace: the compacted lists (4 bytes per container, with a reason_mask), the digest words
    // (4 bytes per container, split grids only) and one count per scenario
    uint32_t *list = nullptr, *cnt = nullptr, *dig = nullptr;
    if (reason_mask || split) {
        if (int rc = fp_ws_reserve(c, (reason_mask ? SC * 4 + (size_t)S * 4 : 0) + (split ? SC * 4 : 0) + 4 * 256))
            return rc;
        fp_ws_reset(c);
        if (reason_mask) {
            list = (uint32_t *)fp_ws_take(c, SC * 4);
            cnt = (uint32_t *)fp_ws_take(c, (size_t)S * 4);
            if (!list || !cnt) return FP_ENOMEM;
        }
        if (split) {
            dig = (uint32_t *)fp_ws_take(c, SC * 4);
            if (!dig) return FP_ENOMEM;
        }
    }
    hipEvent_t ev;
    fp_prof_begin(c, FP_K_FEAS, &ev);
    const uint32_t cb = (C + kBlock - 1) / kBlock;
    if (reason_mask) {
        FP_HIP(hipMemsetAsync(cnt, 0, (size_t)S * 4, st));
        k_explain_select<<<dim3(cb, S), kBlock, 0, st>>>(b->reason, C, reason_mask, list, cnt);
        FP_HIP(hipGetLastError());
    }
    if (split) FP_HIP(hipMemsetAsync(dig, 0xFF, SC * 4, st));
    ExArgs a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.N = N; a.node_span = span; a.n_sel = C; a.cnt = cnt; a.sel = list; a.ign = ignore_labels;
    a.cpu = b->cpu_m; a.mem = b->mem_mib; a.req = b->req_labels; a.conf = b->conflict;
    a.cf = b->cpu_free; a.mf = b->mem_free; a.lab = b->labels; a.cu = b->conflict_used;
    a.sched = b->schedulable;
    a.dig = dig; a.hist = hist;
    a.split = split;
    k_explain<false, kPerHist><<<dim3(xb, ysplit, S), kBlock, 0, st>>>(a);
    FP_HIP(hipGetLastError());
    if (split) {
        k_explain_hist<<<dim3(cb, S), kBlock, 0, st>>>(dig, cnt, C, hist);
        FP_HIP(hipGetLastError());
    }
    fp_prof_end(c, FP_K_FEAS, ev);
    return FP_OK;
}
