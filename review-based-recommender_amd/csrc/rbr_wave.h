// rbr_wave.h -- the wave-level reductions and the wave-level scan of librbr_hip.so (wave64), stated once.
//
// wave_sum / wave_max: xor butterfly over groups of WIDTH consecutive lanes (WIDTH a power of two <= 64, the group aligned to
// WIDTH): every lane of the group ends with the group's result.  The order of the additions is fixed -- partner WIDTH/2 first,
// partner 1 last -- and the kernels whose results are tested for bit-reproducibility rely on exactly that order.
// wave_sum_n: wave_sum for a group width that is a kernel argument (sentence_feed.hip); also over an array of independent values
// (siamese_saliency.hip).
// wave_incl_scan: inclusive prefix sum over the 64 lanes (__shfl_up ladder); lane 63 holds the total.
// The cross-wave step of a block reduction stays with its kernel: the sites add their four wave sums in different orders.
//
// block_rank_256: the in-block ranking of the distinct-token row maps, for a workgroup of 256 threads (4 waves), every thread
// of which makes the call.  Users: gp_count_kernel, gp_compact_kernel (datt_gates.hip), compact_block<KEPT> (textcnn_prod.hip).
// Contract -- u = the thread's mark (non-zero: marked), s_n = the caller's own __shared__ int[4]:
//   inside   ballot of the marks, s_n[w] = marked threads of wave w (written by lane 0), ONE barrier, then the prefix over the
//            earlier waves.  After the call s_n holds the four wave counts for every thread.
//   returns  rank  = marked threads of the workgroup below this one (-1 for an unmarked thread): with `base` marked tokens below
//                    the block, the thread's row is base + rank, rows ascending with the thread index;
//            total = marked threads of the workgroup.
//   barriers the one inside also publishes whatever the caller wrote to LDS before the call -- that is how each caller's
//            partial sums of `base` reach all its threads without a barrier of their own.  None behind: a caller that writes
//            s_n (or calls again) afterwards puts its own barrier in front.
// `base` itself stays with the caller (block counts of an earlier launch in the gates, popcounts of byte marks in the conv), and
// so does whoever writes the row counter.
#pragma once

#include <hip/hip_runtime.h>

namespace rbr {

template <int WIDTH = 64, typename T>      // T: float, int or long
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// wave_sum with a group width known only at run time (a power of two <= 64, the same for the whole wave): the same butterfly in
// the same order.  Every lane of the wave makes the call.
template <typename T>
__device__ __forceinline__ T wave_sum_n(T v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// wave_sum_n of N independent values at once, each in the order of the scalar form: the N butterflies advance step by step together,
// so that a step costs one shuffle latency instead of N (siamese_saliency.hip).  Every lane of the wave makes the call.
template <int N, typename T>
__device__ __forceinline__ void wave_sum_n(T (&v)[N], int width) {
    for (int o = width >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o);
    }
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

struct BlockRank { int rank, total; };
__device__ __forceinline__ BlockRank block_rank_256(int u, int* s_n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(u);
    if (lane == 0) s_n[wave] = __popcll(b);
    __syncthreads();
    int below = 0;
    for (int k = 0; k < wave; ++k) below += s_n[k];
    const int rank = u ? below + (int)__popcll(b & ((1ull << lane) - 1)) : -1;
    return {rank, s_n[0] + s_n[1] + s_n[2] + s_n[3]};
}

}  // namespace rbr
