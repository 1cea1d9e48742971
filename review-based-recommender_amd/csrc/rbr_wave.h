// rbr_wave.h -- the wave-level reductions and the wave-level scan of librbr_hip.so (wave64), stated once.
//
// wave_sum / wave_max: xor butterfly over groups of WIDTH consecutive lanes (WIDTH a power of two <= 64, the group aligned to
// WIDTH): every lane of the group ends with the group's result.  The order of the additions is fixed -- partner WIDTH/2 first,
// partner 1 last -- and the kernels whose results are tested for bit-reproducibility rely on exactly that order.
// wave_incl_scan: inclusive prefix sum over the 64 lanes (__shfl_up ladder); lane 63 holds the total.
// The cross-wave step of a block reduction stays with its kernel: the sites add their four wave sums in different orders.
#pragma once

#include <hip/hip_runtime.h>

namespace rbr {

template <int WIDTH = 64, typename T>      // T: float, int or long
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int WIDTH = 64>
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

}  // namespace rbr
