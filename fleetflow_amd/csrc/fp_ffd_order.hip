// fp_ffd_order.hip -- the radix FFD order (fp_internal.h fp_ffd_order): the one place that builds the keys,
// the segment offsets and the rocprim sort with its scratch.  First fit's radix path (fp_place.hip step 3b), the
// scored placer (fp_policy.hip) and the drain sweep (fp_drain.hip) all order their containers through it.
#include "fp_internal.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace {

// Keys (~cpu << 32) | ~mem (descending demands sort ascending), value = the index in the scenario.
// RNG: also ORs every value into rng[0] (cpu) / rng[1] (mem), one atomic per block and word (first fit's
// packed-capacity decision, fp_pipe_pk.h); the other callers do not pay for it.
template <bool RNG>
__global__ __launch_bounds__(256) void k_ffd_keys(const uint32_t *__restrict__ cpu, const uint32_t *__restrict__ mem,
                                                  size_t n, uint32_t C, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals, uint32_t *__restrict__ rng) {
    uint32_t oc = 0, om = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)i / C, j = (uint32_t)i - s * C;  // n = S * C < 2^32
        const uint32_t c = cpu[i], m = mem[i];
        keys[i] = ((uint64_t)~c << 32) | (uint32_t)~m;
        vals[i] = j;
        oc |= c;
        om |= m;
    }
    if constexpr (RNG) {
        for (int o = 32; o > 0; o >>= 1) {
            oc |= (uint32_t)__shfl_xor((int)oc, o);
            om |= (uint32_t)__shfl_xor((int)om, o);
        }
        __shared__ uint32_t red[2];
        if (threadIdx.x < 2) red[threadIdx.x] = 0u;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
            atomicOr(&red[0], oc);
            atomicOr(&red[1], om);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            fp_or_new_bits(&rng[0], red[0]);
            fp_or_new_bits(&rng[1], red[1]);
        }
    }
}

__global__ void k_ffd_offsets(uint32_t S, uint32_t C, uint32_t *__restrict__ off) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= S) off[i] = i * C;
}

// the sort of S scenarios of C containers: the size query with tmp = null, else the sort itself
int ffd_sort(hipStream_t st, uint32_t S, size_t SC, void *tmp, size_t &tmp_bytes, const fp_ffd_order *fo,
             uint32_t *offs) {
    uint64_t *ki = tmp ? fo->keys_in : nullptr, *ko = tmp ? fo->keys_out : nullptr;
    uint32_t *vi = tmp ? fo->vals_in : nullptr, *vo = tmp ? fo->order : nullptr;
    if (S == 1) {
        FP_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, ki, ko, vi, vo, SC, 0, 64, st));
    } else {
        FP_HIP(rocprim::segmented_radix_sort_pairs(tmp, tmp_bytes, ki, ko, vi, vo, (unsigned)SC, S, offs, offs + 1, 0,
                                                   64, st));
    }
    return FP_OK;
}

}  // namespace

int fp_ffd_order_size(fp_ctx *c, uint32_t S, uint32_t C, size_t min_tmp, fp_ffd_order *fo) {
    const size_t SC = (size_t)S * C;
    size_t t = 0;
    if (int rc = ffd_sort(c->stream, S, SC, nullptr, t, fo, nullptr)) return rc;
    fo->tmp_bytes = t > min_tmp ? t : min_tmp;
    // the takes of fp_ffd_order_run, in its order
    size_t top = 0;
    top = fp_take_end(top, SC * 8);
    top = fp_take_end(top, SC * 8);
    top = fp_take_end(top, SC * 4);
    top = fp_take_end(top, SC * 4);
    top = fp_take_end(top, ((size_t)S + 1) * 4);
    top = fp_take_end(top, fo->tmp_bytes + 16);
    fo->bytes = fp_align256(top);  // wherever the caller's arena stands when the takes begin
    return FP_OK;
}

int fp_ffd_order_run(fp_ctx *c, uint32_t S, uint32_t C, const uint32_t *cpu, const uint32_t *mem, uint32_t *rng,
                     fp_ffd_order *fo) {
    hipStream_t st = c->stream;
    const size_t SC = (size_t)S * C;
    fo->keys_in = (uint64_t *)fp_ws_take(c, SC * 8);
    fo->keys_out = (uint64_t *)fp_ws_take(c, SC * 8);
    fo->vals_in = (uint32_t *)fp_ws_take(c, SC * 4);
    fo->order = (uint32_t *)fp_ws_take(c, SC * 4);
    uint32_t *offs = (uint32_t *)fp_ws_take(c, ((size_t)S + 1) * 4);
    fo->tmp = fp_ws_take(c, fo->tmp_bytes + 16);
    if (!fo->keys_in || !fo->keys_out || !fo->vals_in || !fo->order || !offs || !fo->tmp) return FP_ENOMEM;
    if (rng) k_ffd_keys<true><<<grid_for(SC, 256), 256, 0, st>>>(cpu, mem, SC, C, fo->keys_in, fo->vals_in, rng);
    else k_ffd_keys<false><<<grid_for(SC, 256), 256, 0, st>>>(cpu, mem, SC, C, fo->keys_in, fo->vals_in, nullptr);
    FP_HIP(hipGetLastError());
    if (S > 1) {
        k_ffd_offsets<<<(S + 1 + 255) / 256, 256, 0, st>>>(S, C, offs);
        FP_HIP(hipGetLastError());
    }
    size_t t = fo->tmp_bytes;
    return ffd_sort(st, S, SC, fo->tmp, t, fo, offs);
}
