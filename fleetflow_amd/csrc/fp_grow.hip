// fp_grow.hip -- the scale-out sweep (SPEC.md 2.12): for every candidate (one server template) the new servers
// of that template the pending containers of a plan need, every candidate from the same pending list.
// One workgroup owns one candidate; the blocks share only the read-only list.
//
// Per fp_dev_grow_sweep call (asynchronous, nothing is read back):
//   1. k_grow_check   : sets the call's "bad" word for a t_max[k] above max_new, and FP_EINVAL in the context's
//                       error word; every later kernel that writes an output returns on the word first
//   2. the pending list, once per call: the radix FFD order (fp_ffd_order.hip) is the 2.3 order of all
//                       containers (cpu desc, mem desc, index asc); a stable rocprim select keeps the
//                       containers whose reason is in reason_mask (reason_mask == 0: the order itself) and
//                       leaves their number in the workspace; k_grow_records gathers them into the dense SoA
//                       (cpu, mem, req, conflict, index) every block streams.  The records live in the two key
//                       buffers of the sort, which are free by then
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
// No device-wide synchronisation and no spin waits: the kernels cannot deadlock and have no guard.
#include "fp_internal.h"
#include "fp_argmin.h"
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

}  // namespace

int fp_dev_grow_sweep_impl(fp_ctx *c, const fp_containers *cs, const uint8_t *reason, uint32_t reason_mask,
                           uint32_t n_cand, const uint32_t *t_cpu, const uint32_t *t_mem, const uint32_t *t_labels,
                           const uint32_t *t_max, uint32_t max_new, uint32_t *summary_out, uint32_t *assign_out) {
    const uint32_t C = cs->n;
    c->last_rng = nullptr;  // this call recycles the workspace the last placement's range words live in
    if (n_cand > 65535u || max_new > FP_GROW_MAX_NEW) return FP_EOVERFLOW;
    if (reason_mask && !reason) return FP_EINVAL;
    if (C && (!cs->cpu_m || !cs->mem_mib || !cs->req_labels || !cs->conflict)) return FP_EINVAL;
    if (n_cand && (!t_cpu || !t_mem || !t_labels || !summary_out)) return FP_EINVAL;
    if (n_cand == 0) return FP_OK;
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
    if (t_max) {
        k_grow_check<<<grid_for(n_cand, 256), 256, 0, st>>>(t_max, n_cand, max_new, bad, c->d_err);
        FP_HIP(hipGetLastError());
    }

    GrowArgs a = {};
    a.C = C; a.max_new = max_new; a.cnt = cnt;
    a.t_cpu = t_cpu; a.t_mem = t_mem; a.t_lab = t_labels; a.t_max = t_max;
    a.summary = summary_out; a.assign_out = C ? assign_out : nullptr;
    a.bad = bad;

    hipEvent_t ev;
    if (C == 0) {
        k_grow_count<<<1, 64, 0, st>>>(cnt, 0u);
        FP_HIP(hipGetLastError());
    } else {
        // ---- the pending list: 2.3 order, the stable selection, the records ----
        uint32_t *r_idx = (uint32_t *)fp_ws_take(c, (size_t)C * 4);
        if (!r_idx) return FP_ENOMEM;
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
        a.r_cpu = ka; a.r_mem = ka + C; a.r_req = kb; a.r_conf = kb + C; a.r_idx = r_idx;
        if (assign_out) {
            const size_t n = (size_t)n_cand * C;
            k_grow_init<<<grid_for(n, 256), 256, 0, st>>>(assign_out, n, bad);
            FP_HIP(hipGetLastError());
        }
    }
    fp_prof_begin(c, FP_K_PLACE, &ev);
    launch_grow(a, n_cand, st);
    FP_HIP(hipGetLastError());
    fp_prof_end(c, FP_K_PLACE, ev);
    return FP_OK;
}
