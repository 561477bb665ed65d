// fp_payload.h -- the by-field payload gather of the sorted SoA (req, conf, the CYCLE / screen bit of
// s_idx), as a device function two kernels share: k_payload_lds (fp_pipe.hip), which takes the container
// indices from the `order` row a finished sort kernel left in HBM, and phase P of the fused
// k_scen_sort (fp_place.hip), whose workgroup still holds the order in LDS.
//
// One workgroup of PL_THREADS per scenario.  Each thread owns the sorted positions t + 1024 j, keeps
// their container indices in registers, streams the scenario's inputs through LDS in chunks of PL_FIELD_CHUNK
// and picks its positions' values out of the chunk that holds them (level first, for the CYCLE bits).
#pragma once
#include "fp_internal.h"

// FPP_PAYLOAD_BY_FIELD (A/B switch): 1 = the passes of k_payload_lds are split by field, and order, level,
// conf and req are each read once per scenario; 0 = round 3's kernel, split by position half, which reads
// (req, conf) and level once per half (fp_pipe.hip; the sort is then never fused).
#ifndef FPP_PAYLOAD_BY_FIELD
#define FPP_PAYLOAD_BY_FIELD 1
#endif

namespace fpl {

constexpr uint32_t PL_THREADS = 1024, PL_H = 25, PL_MAX_C = PL_THREADS * PL_H * 2;
// s_idx bit 31 (fp_pipe.hip CYC): the container never enters the pipeline
constexpr uint32_t PL_SKIP = 0x80000000u;
// By field: a thread keeps the container indices of all its 2 PL_H positions for the whole kernel, as u16
// pairs (PL_H registers: an index is below C <= PL_MAX_C < 0xFFFF, and 0xFFFF marks a position past
// C, which no chunk holds).  level, conf and req then take one pass each through LDS in chunks of
// PL_FIELD_CHUNK words: level leaves a CYCLE bit per position, conf is written as soon as its last chunk
// has been picked and leaves the bit (conf & summ[1]) != 0, req joins the bits and is written with the
// reason codes.  Per container 4 B of order (none in the fused sort) and 4 B per field are read, 8 B
// written and the skip-bit row touched where the bit is set.
// The skip-bit row (`s_skip` below) is s_idx -- or, for a scenario the fused sort's prepack mode wrote as one
// packed demand row (fp_place.hip), that row s_w, whose bit 31 is a guard bit of the packed word and clear
// by construction: the same bit, the same store / barrier / agent-scope load order.
constexpr uint32_t PL_ROWS = 2 * PL_H;
constexpr uint32_t PL_FIELD_CHUNK = 36 * 1024;  // words of one field: 144 KB of LDS
constexpr size_t PL_FIELD_LDS_BYTES = (size_t)PL_FIELD_CHUNK * 4;
static_assert(PL_MAX_C < 0xFFFFu, "container indices are kept in 16 bits, 0xFFFF = no position");

// where a workgroup's container indices come from
enum pl_source {
    PL_ORDER = 0,        // the `order` row, written by an earlier kernel
    PL_ORDER_SAME_WG,    // the `order` row and the s_idx words, written by other waves of this workgroup
    PL_LDS_X             // the sort's X[0, C) (u16) in LDS; the s_idx words as PL_ORDER_SAME_WG
};

// the two indices of pair j, less the chunk's base.  The empty asm keeps the unpacking inside the chunk loop:
// hoisted out of it, the 2 PL_H unpacked indices live beside the 2 PL_H values and the kernel spills.
__device__ __forceinline__ void pl_index(uint32_t w, uint32_t a0, uint32_t &d0, uint32_t &d1) {
    asm volatile("" : "+v"(w));
    d0 = (w & 0xFFFFu) - a0;
    d1 = (w >> 16) - a0;
}
__device__ __forceinline__ void pl_load_chunk(uint32_t *pl_lds, const uint32_t *__restrict__ src, uint32_t n) {
    __syncthreads();  // the previous chunk's picks are done
#pragma unroll 8
    for (uint32_t i = threadIdx.x; i < n; i += PL_THREADS) pl_lds[i] = __builtin_nontemporal_load(&src[i]);
    __syncthreads();
}
__device__ __forceinline__ void pl_pick_field(uint32_t *pl_lds, const uint32_t *__restrict__ field, uint32_t C,
                                              const uint32_t (&o)[PL_H], uint32_t (&v)[PL_ROWS]) {
    for (uint32_t a0 = 0; a0 < C; a0 += PL_FIELD_CHUNK) {
        const uint32_t n = C - a0 < PL_FIELD_CHUNK ? C - a0 : PL_FIELD_CHUNK;
        pl_load_chunk(pl_lds, field + a0, n);
#pragma unroll
        for (uint32_t j = 0; j < PL_H; ++j) {
            uint32_t d0, d1;
            pl_index(o[j], a0, d0, d1);
            if (d0 < n) v[2 * j] = pl_lds[d0];
            if (d1 < n) v[2 * j + 1] = pl_lds[d1];
        }
    }
}

// The container indices of thread t's positions t + 1024 j as u16 pairs.  PL_ORDER_SAME_WG: the row was stored
// by other waves of this workgroup, which drained their stores (s_waitcnt vmcnt(0)) before a barrier this
// thread has passed; the loads are agent-scope (sc1: served by L2, never by a stale line of this CU's L1),
// as ss_generic (fp_place.hip) reads its own passes back.  PL_LDS_X: X holds the order; the caller puts a
// barrier between these reads and the first chunk load, which overwrites X (pl_load_chunk begins with one).
template <pl_source SRC>
__device__ __forceinline__ void pl_indices(uint32_t C, const uint32_t *ord, const uint16_t *X,
                                           uint32_t (&o)[PL_H]) {
    const uint32_t t = threadIdx.x;
    uint32_t i[PL_ROWS];  // every load in flight at once; past C the last element, not used
#pragma unroll
    for (uint32_t j = 0; j < PL_ROWS; ++j) {
        const uint32_t p = t + PL_THREADS * j;
        const uint32_t q = p < C ? p : C - 1;
        const uint32_t x = SRC == PL_LDS_X ? (uint32_t)X[q]
                           : SRC == PL_ORDER_SAME_WG
                               ? __hip_atomic_load(&ord[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : __builtin_nontemporal_load(&ord[q]);
        i[j] = p < C ? x & 0xFFFFu : 0xFFFFu;
    }
#pragma unroll
    for (uint32_t j = 0; j < PL_H; ++j) o[j] = i[2 * j] | i[2 * j + 1] << 16;
}

// The whole gather for one scenario (blockIdx.x): its summ words, the indices, then the level, conf and req
// passes and the stores.  pl_lds: PL_FIELD_LDS_BYTES of LDS.  SAME_WG = false: the indices come from `order`,
// which an earlier kernel wrote (k_payload_lds).  SAME_WG = true (the fused sort): from X when from_x (uniform
// in the workgroup), else from `order`; the row, and the words of s_skip (s_idx or s_w, above) the skip bit is ORed into, were stored by
// other waves of this workgroup (drained before a barrier, see pl_indices) and are read at agent scope.
template <bool SAME_WG>
__device__ __forceinline__ void pl_by_field(uint32_t *pl_lds, uint32_t C, const uint32_t *order, const uint16_t *X,
                                            bool from_x, const uint32_t *req, const uint32_t *conf,
                                            const uint32_t *level, const uint32_t *summ, uint32_t *s_req,
                                            uint32_t *s_conf, uint32_t *s_skip) {
    const uint32_t t = threadIdx.x;
    const size_t cb = (size_t)blockIdx.x * C;
    const uint32_t sm0 = summ ? summ[(size_t)blockIdx.x * 4] : 0xFFFFFFFFu;
    const uint32_t sm1 = summ ? summ[(size_t)blockIdx.x * 4 + 1] : 0u;
    uint32_t o[PL_H];
    if (!SAME_WG) pl_indices<PL_ORDER>(C, order + cb, nullptr, o);
    else if (from_x) pl_indices<PL_LDS_X>(C, nullptr, X, o);
    else pl_indices<PL_ORDER_SAME_WG>(C, order + cb, nullptr, o);
    // bit j % 32 of cy0 / cy1 (j < 32 / the rest): position t + 1024 j is a CYCLE member; sc0 / sc1 the same
    // for (conf & summ[1]) != 0
    uint32_t cy0 = 0, cy1 = 0;
    if (level) {
        for (uint32_t a0 = 0; a0 < C; a0 += PL_FIELD_CHUNK) {
            const uint32_t n = C - a0 < PL_FIELD_CHUNK ? C - a0 : PL_FIELD_CHUNK;
            pl_load_chunk(pl_lds, level + cb + a0, n);
#pragma unroll
            for (uint32_t j = 0; j < PL_H; ++j) {
                uint32_t d0, d1;
                pl_index(o[j], a0, d0, d1);
                if (d0 < n) (j < 16 ? cy0 : cy1) |= (uint32_t)(pl_lds[d0] == FP_NONE) << ((2 * j) & 31u);
                if (d1 < n) (j < 16 ? cy0 : cy1) |= (uint32_t)(pl_lds[d1] == FP_NONE) << ((2 * j + 1) & 31u);
            }
        }
    }
    uint32_t v[PL_ROWS];
    uint32_t sc0 = 0, sc1 = 0;
    pl_pick_field(pl_lds, conf + cb, C, o, v);
    // (each phase takes its positions and their bound from copies of t and C that the compiler cannot see
    // through: it kept the order loads' 2 PL_H positions, as 64-bit indices in scratch, and their
    // 2 PL_H lane masks p < C, in spilled SGPRs, for the stores)
    uint32_t tc = t, Cc = C;
    asm volatile("" : "+v"(tc), "+s"(Cc));
    uint32_t *const d_conf = s_conf + cb;
#pragma unroll
    for (uint32_t j = 0; j < PL_ROWS; ++j) {
        const uint32_t p = tc + PL_THREADS * j;
        if (p < Cc) {
            __builtin_nontemporal_store(v[j], &d_conf[p]);
            (j < 32 ? sc0 : sc1) |= (uint32_t)((v[j] & sm1) != 0u) << (j & 31u);
        }
    }
    pl_pick_field(pl_lds, req + cb, C, o, v);
    uint32_t tr = t, Cr = C;
    asm volatile("" : "+v"(tr), "+s"(Cr));
    uint32_t *const d_req = s_req + cb, *const d_idx = s_skip + cb;
#pragma unroll
    for (uint32_t j = 0; j < PL_ROWS; ++j) {
        const uint32_t p = tr + PL_THREADS * j;
        if (p < Cr) {
            uint32_t r = v[j];
            const bool c = ((j < 32 ? cy0 : cy1) >> (j & 31u)) & 1u;
            const bool x = (r & ~sm0) != 0u || (((j < 32 ? sc0 : sc1) >> (j & 31u)) & 1u);
            if (c) r = FP_REASON_CYCLE;
            else if (summ && x) r = FP_REASON_NOFIT;
            __builtin_nontemporal_store(r, &d_req[p]);
            if (c || (summ && x)) {
                if (SAME_WG) d_idx[p] = __hip_atomic_load(&d_idx[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | PL_SKIP;
                else d_idx[p] |= PL_SKIP;
            }
        }
    }
}

}  // namespace fpl
