// fp_argmin.h -- the block argmin over 64-bit placement keys that the scored placer (fp_policy.hip,
// SPEC.md 2.6) and the drain sweep (fp_drain.hip, SPEC.md 2.11 and 2.15) share: the key layouts of 2.6, 2.7
// and 2.8 and the cross-lane helpers.  Device code only; every function is forced inline.
// This header is where sharing between k_policy and k_drain_sweep stops: moving any more of them into shared
// functions (the strategy's primary score, the block min with its slots and parity, the winner's update)
// changes the code of k_policy's instantiations, by reordered opcodes up to hundreds of instructions
// (DESIGN.md 4.11 has the table).  Compare with tools/isa_compare.py before believing otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fpd {

constexpr uint64_t KEY_NONE = ~0ull;    // an infeasible node
constexpr uint32_t KEY_NODE_BITS = 26;  // key = pref_miss << 58 | primary << 26 | node

// SPEC.md 2.8, the variants with a fallback chain: key = hop << 61 | pref_miss << 55 | primary << 23 | node
constexpr uint32_t KEY_NODE_BITS_FB = 23;
constexpr uint32_t KEY_HOP_SHIFT = 61;
// SPEC.md 2.7: a node that fits by 2.3 and fails the skew test.  Real keys are below 0x84 << 56
// (pref_miss <= 32; with a fallback chain hop <= 4 as well: below 0x91 << 56), so a block minimum of
// KEY_SKEW says SKEW and one of KEY_NONE says NOFIT
constexpr uint64_t KEY_SKEW = KEY_NONE - 1;
constexpr uint32_t DOM_BITS = 6;  // FP_SPREAD_MAX_DOMAINS = 64: a domain id is one lane of a wave

__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// wave-uniform value of lane `l` (l uniform): the record broadcast
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

// Cross-lane min of the 64-bit keys on the VALU (DPP), not through the LDS crossbar: with 16 waves a
// block, 12 ds_bpermute a wave and container kept the LDS pipe busier than the key evaluation.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}
// the min over each row of 16 lanes, in every lane of the row (all 64 lanes active).  min is idempotent,
// so the mirrors serve as butterflies: quads, then the two quads of a half row, then the two halves
__device__ __forceinline__ uint64_t row_min64(uint64_t v) {
    v = min64(v, dpp64<0xB1>(v));   // quad_perm [1, 0, 3, 2]
    v = min64(v, dpp64<0x4E>(v));   // quad_perm [2, 3, 0, 1]
    v = min64(v, dpp64<0x141>(v));  // row_half_mirror
    v = min64(v, dpp64<0x140>(v));  // row_mirror
    return v;
}
__device__ __forceinline__ uint64_t lane64(uint64_t v, int l) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}
// the min over the wave, uniform: the four row mins meet in scalar registers
__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
    v = row_min64(v);
    return min64(min64(lane64(v, 0), lane64(v, 16)), min64(lane64(v, 32), lane64(v, 48)));
}

// the same min over 32-bit values (the domain counts of SPEC.md 2.7), uniform
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

}  // namespace fpd
