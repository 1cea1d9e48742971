// datt_saliency.hip -- per-position contributions (gradient x input) of one D-ATT tower, THROUGH both attention gates:
// rbr_datt_saliency.  The formula stands in rbr_hip.h; x[t] = table[ids[t]], banks [0, k) sit under the local gate gate_l[t],
// the rest under the document's global gate gate_g.
//
// Two launches on one stream, no workspace beyond the outputs, no atomics:
//   1. datt_raw_kernel: saliency_kernel's scheme (textcnn_saliency.hip) with the gates taken OUT of the tap values -- one
//      workgroup per document; phase 1 is the shared code of saliency_taps.h and leaves g[c] * <x[t], W_w[c, :, j]>; in phase 2 the
//      owner of a position keeps TWO sums, raw_l over the entries of the local banks and raw_g over the others (entries are in
//      channel order, so one entry index splits them), and writes fixed[t] = gate_l[t] * raw_l + gate_g * raw_g and
//      d_gate_l[t] = raw_l.  Every thread adds up the raw_g of its own positions in position order; after the last pass the
//      workgroup reduces those 256 sums with a butterfly per wave and the four waves in order: d_gate_g[doc].
//   2. datt_through_kernel: one thread per position t, lanes along t.  A thread reads its row x[t] once and keeps win + 1 dot
//      products of length E with it: against the win taps of w_l (wave-uniform addresses) and against w_g[:, t] (w_g[e * L + t]:
//      coalesced over the lanes).  through[t] = sum_j dpre_l[t - j + (win-1)/2] * <x[t], w_l[:, j]> + dpre_g * <x[t], w_g[:, t]>
//      with dpre = d_gate * gate * (1 - gate) from what launch 1 left in d_gate_l / d_gate_g.
// A row of the outputs depends on its own document only and every sum has a fixed order: the same bits on every run, in every
// batch.  Every output element is written once with a plain store.
#include "saliency_taps.h"

namespace rbr {

constexpr int kThroughThreads = 64;                 // positions per workgroup of launch 2 (one wave)
constexpr int kMaxGateWin = 9;                      // widest local-attention window of launch 2

// Phase 2 over four entries that sit under ONE gate: the owner of a position adds those that target it, in index order (an
// entry that does not target the position adds 0.0f, which changes nothing; position -1 matches nobody).
__device__ __forceinline__ void add_entries(float (&acc)[kSalOwn], const int4& p, const float4& v, int t0, int tid) {
#pragma unroll
    for (int k = 0; k < kSalOwn; ++k) {
        const int tk = t0 + tid + k * kSalThreads;
        acc[k] += (p.x == tk) ? v.x : 0.f;
        acc[k] += (p.y == tk) ? v.y : 0.f;
        acc[k] += (p.z == tk) ? v.z : 0.f;
        acc[k] += (p.w == tk) ? v.w : 0.f;
    }
}

template <bool VEC4>
__global__ __launch_bounds__(kSalThreads) void datt_raw_kernel(const SalArgs A, int split_ch, const long long* __restrict__ ids,
                                                                const float* __restrict__ gate, const float* __restrict__ table,
                                                                const PtrArray W, const float* __restrict__ feat,
                                                                const int* __restrict__ argmax, const float* __restrict__ d_feat,
                                                                float* __restrict__ fixed, float* __restrict__ d_gate_l,
                                                                float* __restrict__ d_gate_g) {
    __shared__ __align__(16) float s_val[kSalChunk * kMaxKF];
    __shared__ __align__(16) int s_pos[kSalChunk * kMaxKF];
    __shared__ float s_g[kSalChunk];                // g = d_feat * act'(feat) and the argmax of the chunk's channels
    __shared__ int s_p[kSalChunk];
    __shared__ float s_wave[kSalThreads / kWave];
    const int doc = blockIdx.x;
    const int tid = threadIdx.x;
    const int grp = tid / A.G, sl = tid % A.G, ngrp = kSalThreads / A.G;
    const long row0 = (long)doc * A.L;              // first position of the document in ids / gate planes / outputs
    const long ch0 = (long)doc * A.C;               // first channel of the document in feat / argmax / d_feat
    const float* gate_l = gate + row0;
    const float gate_g = gate[(long)A.n_docs * A.L + row0];     // one scalar per document: its plane repeats it over L
    float sum_g = 0.f;                              // raw_g over this thread's positions, in position order

    for (int t0 = 0; t0 < A.L; t0 += kSalPass) {
        const int t1 = min(A.L, t0 + kSalPass);
        float raw_l[kSalOwn], raw_g[kSalOwn];
#pragma unroll
        for (int k = 0; k < kSalOwn; ++k) raw_l[k] = raw_g[k] = 0.f;

        for (int c0 = 0; c0 < A.C; c0 += kSalChunk) {
            const int c1 = min(A.C, c0 + kSalChunk);
            const int n_ent = (c1 - c0) * A.KF;     // entry e = (channel c0 + e / KF, tap e % KF)
            const int n_ent4 = (n_ent + 3) & ~3;    // phase 2 reads four entries at a time
            const int e_split = min(n_ent, max(0, split_ch - c0) * A.KF);      // entries below it belong to the local banks
            for (int e = tid; e < n_ent4; e += kSalThreads) s_pos[e] = -1;
            if (tid < c1 - c0) {
                s_g[tid] = act_grad(A.act, feat[ch0 + c0 + tid], d_feat[ch0 + c0 + tid]);
                s_p[tid] = argmax[ch0 + c0 + tid];
            }
            __syncthreads();
            // ---- phase 1: un-masked, un-gated tap values g * <x[t], W_w[c, :, j]>
            chunk_taps<VEC4>(A, ids, nullptr, nullptr, table, W, s_g, s_p, c0, c1, row0, t0, t1, grp, ngrp, sl, s_val, s_pos);
            __syncthreads();
            // ---- phase 2: entries are in channel order, so a group of four sits under the local gate, under the global one, or
            // (once per chunk at most) across the boundary; the branch is uniform over the workgroup
            for (int e4 = 0; e4 < n_ent4 / 4; ++e4) {
                const int4 p = reinterpret_cast<const int4*>(s_pos)[e4];
                const float4 v = reinterpret_cast<const float4*>(s_val)[e4];
                const int e = 4 * e4;
                if (e + 4 <= e_split) {
                    add_entries(raw_l, p, v, t0, tid);
                } else if (e >= e_split) {
                    add_entries(raw_g, p, v, t0, tid);
                } else {
                    const bool l1 = e + 1 < e_split, l2 = e + 2 < e_split;      // entry e is local, entry e + 3 global
#pragma unroll
                    for (int k = 0; k < kSalOwn; ++k) {
                        const int tk = t0 + tid + k * kSalThreads;
                        const float a0 = (p.x == tk) ? v.x : 0.f, a1 = (p.y == tk) ? v.y : 0.f;
                        const float a2 = (p.z == tk) ? v.z : 0.f, a3 = (p.w == tk) ? v.w : 0.f;
                        raw_l[k] += a0;
                        raw_l[k] += l1 ? a1 : 0.f;  raw_g[k] += l1 ? 0.f : a1;
                        raw_l[k] += l2 ? a2 : 0.f;  raw_g[k] += l2 ? 0.f : a2;
                        raw_g[k] += a3;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kSalOwn; ++k) {
            const int t = t0 + tid + k * kSalThreads;
            if (t < t1) {
                fixed[row0 + t] = gate_l[t] * raw_l[k] + gate_g * raw_g[k];
                d_gate_l[row0 + t] = raw_l[k];
                sum_g += raw_g[k];
            }
        }
    }
    // ---- d_gate_g[doc] = sum_t raw_g[t]: butterfly inside a wave, then the waves in order
    for (int off = kWave >> 1; off > 0; off >>= 1) sum_g += __shfl_xor(sum_g, off);
    if (tid % kWave == 0) s_wave[tid / kWave] = sum_g;
    __syncthreads();
    if (tid == 0) {
        float s = s_wave[0];
        for (int w = 1; w < kSalThreads / kWave; ++w) s += s_wave[w];
        d_gate_g[doc] = s;
    }
}

// d_gate * gate * (1 - gate): exactly 0 for a saturated sigmoid (gate == 0.0f or 1.0f)
__device__ __forceinline__ float gate_dpre(float d_gate, float gate) { return d_gate * gate * (1.f - gate); }

// Launch 2: a thread per position, lanes along t.  (Staging the tile's rows through LDS in 128-byte pieces with four waves per
// tile was measured at 55 us against 25 us for this form at cfg4: the 20 MB table sits in L2 / Infinity Cache, and the
// extra barriers cost more than the wider loads save.)
template <int WIN, bool VEC4>
__global__ __launch_bounds__(kThroughThreads) void datt_through_kernel(int n_docs, int L, int E, int V,
                                                                        const long long* __restrict__ ids,
                                                                        const float* __restrict__ gate,
                                                                        const float* __restrict__ table,
                                                                        const float* __restrict__ w_l, const float* __restrict__ w_g,
                                                                        const float* __restrict__ d_gate_l,
                                                                        const float* __restrict__ d_gate_g,
                                                                        float* __restrict__ through) {
    const int tiles = (L + kThroughThreads - 1) / kThroughThreads;
    const int doc = blockIdx.x / tiles;
    const int t = (blockIdx.x % tiles) * kThroughThreads + threadIdx.x;
    if (t >= L) return;
    const long row0 = (long)doc * L;
    const long long tok = ids[row0 + t];
    float out = 0.f;
    if (tok >= 0 && tok < (long long)V) {           // never index the table with an id outside it: such a row counts as zero
        const float* x = table + (long)tok * E;
        const float* wg = w_g + t;                  // w_g[e * L + t]
        float acc[WIN], acc_g = 0.f;
#pragma unroll
        for (int j = 0; j < WIN; ++j) acc[j] = 0.f;
        if (VEC4) {
            for (int e = 0; e < E; e += 4) {
                const float4 xv = *reinterpret_cast<const float4*>(x + e);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < WIN; ++j) acc[j] = fmaf(xs[i], w_l[(e + i) * WIN + j], acc[j]);
                    acc_g = fmaf(xs[i], wg[(long)(e + i) * L], acc_g);
                }
            }
        } else {
            for (int e = 0; e < E; ++e) {
                const float xe = x[e];
#pragma unroll
                for (int j = 0; j < WIN; ++j) acc[j] = fmaf(xe, w_l[e * WIN + j], acc[j]);
                acc_g = fmaf(xe, wg[(long)e * L], acc_g);
            }
        }
        const float* gate_l = gate + row0;
        const float* dl = d_gate_l + row0;
#pragma unroll
        for (int j = 0; j < WIN; ++j) {             // gate_l[s] read x[t] through tap j: s = t - j + (WIN - 1) / 2
            const int s = t - j + (WIN - 1) / 2;
            if (s >= 0 && s < L) out = fmaf(gate_dpre(dl[s], gate_l[s]), acc[j], out);
        }
        out = fmaf(gate_dpre(d_gate_g[doc], gate[(long)n_docs * L + row0]), acc_g, out);
    }
    through[row0 + t] = out;
}

}  // namespace rbr

using namespace rbr;

extern "C" int rbr_datt_saliency(const rbr_textcnn_desc* d, const int64_t* ids, const float* gate, const float* table,
                                 const float* const* W, const float* feat, const int32_t* argmax, const float* d_feat, int32_t win,
                                 const float* w_l, const float* w_g, float* fixed, float* through, float* d_gate_l, float* d_gate_g,
                                 void* stream) {
    static_assert(kMaxKF == 9, "the width switch of chunk_taps covers 1..9");
    if (!d) { set_error("rbr_datt_saliency: null descriptor"); return RBR_ERR_BAD_ARG; }
    if (d->n_docs == 0) return 0;
    for (int w = 0; w < d->n_widths && w < RBR_MAX_WIDTHS; ++w)
        if (d->kz[w] > kMaxKF) { set_error("rbr_datt_saliency: conv width %d of bank %d is above %d", d->kz[w], w, kMaxKF); return RBR_ERR_UNSUPPORTED; }
    if (!desc_valid(d)) return RBR_ERR_BAD_ARG;
    const int split = RBR_CONV_GATE_SPLIT_OF(d->flags);
    if (split < 1 || split >= d->n_widths) {
        set_error("rbr_datt_saliency: needs RBR_CONV_GATE_SPLIT(k) with 1 <= k < n_widths = %d, got k = %d", d->n_widths, split);
        return RBR_ERR_BAD_ARG;
    }
    if (win < 1 || win % 2 == 0) { set_error("rbr_datt_saliency: the local window must be odd and at least 1, got win = %d", win); return RBR_ERR_BAD_ARG; }
    if (win > kMaxGateWin) { set_error("rbr_datt_saliency: local window win = %d is above %d", win, kMaxGateWin); return RBR_ERR_UNSUPPORTED; }
    if (!ids || !gate || !table || !W || !feat || !argmax || !d_feat || !w_l || !w_g || !fixed || !through || !d_gate_l || !d_gate_g) {
        set_error("rbr_datt_saliency: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    SalArgs A;
    PtrArray Wp;
    bool vec4;
    if (!sal_args_of(d, table, W, "rbr_datt_saliency", &A, &Wp, &vec4)) return RBR_ERR_BAD_ARG;
    const int split_ch = A.ch_off[split];           // first channel under the global gate
    const long long* ids64 = reinterpret_cast<const long long*>(ids);
    hipStream_t st = (hipStream_t)stream;
    if (vec4)
        hipLaunchKernelGGL(datt_raw_kernel<true>, dim3((unsigned)A.n_docs), dim3(kSalThreads), 0, st, A, split_ch, ids64, gate, table,
                           Wp, feat, argmax, d_feat, fixed, d_gate_l, d_gate_g);
    else
        hipLaunchKernelGGL(datt_raw_kernel<false>, dim3((unsigned)A.n_docs), dim3(kSalThreads), 0, st, A, split_ch, ids64, gate, table,
                           Wp, feat, argmax, d_feat, fixed, d_gate_l, d_gate_g);
    RBR_CHECK_LAUNCH("datt saliency launch 1");
    // launch 2 reads rows only: float4 when the table's rows start on 16-byte boundaries.  n_docs * L < 2^31 (desc_valid), so the
    // tile count fits a one-dimensional grid
    const bool row4 = (A.D % 4 == 0) && ((((uintptr_t)table) & 15) == 0);
    const dim3 grid((unsigned)((long)A.n_docs * ((A.L + kThroughThreads - 1) / kThroughThreads)));
#define RBR_THROUGH_CASE(WN)                                                                                                          \
    case WN:                                                                                                                          \
        if (row4)                                                                                                                     \
            hipLaunchKernelGGL((datt_through_kernel<WN, true>), grid, dim3(kThroughThreads), 0, st, A.n_docs, A.L, A.D, A.V, ids64, gate, \
                               table, w_l, w_g, d_gate_l, d_gate_g, through);                                                         \
        else                                                                                                                          \
            hipLaunchKernelGGL((datt_through_kernel<WN, false>), grid, dim3(kThroughThreads), 0, st, A.n_docs, A.L, A.D, A.V, ids64, gate, \
                               table, w_l, w_g, d_gate_l, d_gate_g, through);                                                         \
        break;
    switch (win) {
        RBR_THROUGH_CASE(1) RBR_THROUGH_CASE(3) RBR_THROUGH_CASE(5) RBR_THROUGH_CASE(7) RBR_THROUGH_CASE(9)
        default: break;                             // unreachable: win is odd and in 1..kMaxGateWin
    }
#undef RBR_THROUGH_CASE
    RBR_CHECK_LAUNCH("datt saliency launch 2");
    return 0;
}
