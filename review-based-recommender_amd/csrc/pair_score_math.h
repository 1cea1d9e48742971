// pair_score_math.h -- the one arithmetic of a (user, item) score from cached tower latents and the one ordering key built from
// it, stated once for every file that scores a pair: pair_score.hip (ids / dense / topk / rank) and neg_sample.hip (the hard-
// negative sampler scores its candidates).  Explicit fmaf / __fmul_rn / __fadd_rn, k ascending: the same pair has the same bits
// wherever it is scored, and tests compare those bits.
//   RBR_SCORE_FM : relu(ul[u,:] * il[i,:]) . h + ub[u] + ib[i] + g
//   RBR_SCORE_DOT: sum_k ul[u,k] * il[i,k]
//   key          : (order-preserving bits of the score) << 32 | (2^32 - 1 - item) -- distinct per item, "larger" is "score
//                  descending, then item ascending"; never 0 for a score that is not NaN
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/rbr_hip.h"

namespace rbr {

template <int MODE> __device__ __forceinline__ float score_step(float acc, float u, float i, float h) {
    if (MODE == RBR_SCORE_FM) return fmaf(fmaxf(__fmul_rn(u, i), 0.f), h, acc);
    return fmaf(u, i, acc);
}
template <int MODE> __device__ __forceinline__ float score_finish(float acc, float ub, float ib, float g) {
    if (MODE == RBR_SCORE_FM) return __fadd_rn(__fadd_rn(__fadd_rn(acc, ub), ib), g);
    return acc;
}
template <int MODE>
__device__ __forceinline__ float score_pair(const float* __restrict__ u, const float* __restrict__ i, const float* __restrict__ h, int K,
                                            float ub, float ib, float g) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = score_step<MODE>(acc, u[k], i[k], MODE == RBR_SCORE_FM ? h[k] : 0.f);
    return score_finish<MODE>(acc, ub, ib, g);
}

__device__ __forceinline__ unsigned long long make_key(float s, int item) {
    unsigned b = __float_as_uint(s);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (0xFFFFFFFFu - (unsigned)item);
}
__device__ __forceinline__ float key_score(unsigned long long key) {
    unsigned b = (unsigned)(key >> 32);
    b = (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b;
    return __uint_as_float(b);
}
__device__ __forceinline__ int key_item(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)key); }

}  // namespace rbr
