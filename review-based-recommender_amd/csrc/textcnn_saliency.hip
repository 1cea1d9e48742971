// textcnn_saliency.hip -- per-position contributions (gradient x input) of the fused TextCNN encoder: rbr_textcnn_saliency.
//
// For a gradient d_feat on the pooled features, the max-pool routes g[c] = d_feat[c] * act'(feat[c]) to the ONE window argmax[c]
// of channel c; tap j of that window sits on position t = pos(argmax[c], j) and contributes
//     g[c] * mask[t] * gate[t] * <table[ids[t], :], W_w[c, :, j]>
// to sal[doc, t].  A document has sum_w ch_w * kz_w such tap values, each a dot product over D, and L outputs.
//
// One workgroup per document, two phases per chunk of kSalChunk channels (whose g and argmax are staged in LDS first):
//   1. groups of G lanes (G = 8 .. 64 by D: at most five rounds over a row) take the channels of the chunk in turn, bank by bank.
//      A group reads its channel's weights W_w[c, :, :] -- contiguous in memory -- once, and the kz rows of the window beside
//      them, keeps kz partial dot products per lane and reduces them with a butterfly (the same order on every run); its first
//      lane leaves each tap's value and target position in LDS.  What cannot contribute is dropped BEFORE any row is read: a
//      channel with g == 0 or an argmax outside the pooled range, a tap outside the document or on a masked token;
//   2. thread i owns the positions i, i + 256, ... of the current pass and scans the entries in index order, adding those that
//      target one of its positions (the LDS reads are broadcasts).
// Every sal[doc, t] is written once, by its owner, with a plain store: no atomics, and a row depends on nothing but its own
// document -- the same bits on every run and in every batch.  A pass covers kSalOwn * 256 positions; longer documents take several
// passes, each computing only the taps that land inside it.
#include "saliency_taps.h"

namespace rbr {

template <bool VEC4>
__global__ __launch_bounds__(kSalThreads) void saliency_kernel(const SalArgs A, const long long* __restrict__ ids,
                                                                const unsigned char* __restrict__ mask,
                                                                const float* __restrict__ gate, const float* __restrict__ table,
                                                                const PtrArray W, const float* __restrict__ feat,
                                                                const int* __restrict__ argmax, const float* __restrict__ d_feat,
                                                                float* __restrict__ sal) {
    __shared__ __align__(16) float s_val[kSalChunk * kMaxKF];
    __shared__ __align__(16) int s_pos[kSalChunk * kMaxKF];
    __shared__ float s_g[kSalChunk];                // g = d_feat * act'(feat) and the argmax of the chunk's channels
    __shared__ int s_p[kSalChunk];
    const int doc = blockIdx.x;
    const int tid = threadIdx.x;
    const int grp = tid / A.G, sl = tid % A.G, ngrp = kSalThreads / A.G;
    const long row0 = (long)doc * A.L;              // first position of the document in ids / mask / gate / sal
    const long ch0 = (long)doc * A.C;               // first channel of the document in feat / argmax / d_feat

    for (int t0 = 0; t0 < A.L; t0 += kSalPass) {
        const int t1 = min(A.L, t0 + kSalPass);
        float acc[kSalOwn];
#pragma unroll
        for (int k = 0; k < kSalOwn; ++k) acc[k] = 0.f;

        for (int c0 = 0; c0 < A.C; c0 += kSalChunk) {
            const int c1 = min(A.C, c0 + kSalChunk);
            const int n_ent = (c1 - c0) * A.KF;     // entry e = (channel c0 + e / KF, tap e % KF)
            const int n_ent4 = (n_ent + 3) & ~3;    // phase 2 reads four entries at a time
            for (int e = tid; e < n_ent4; e += kSalThreads) s_pos[e] = -1;
            if (tid < c1 - c0) {
                s_g[tid] = act_grad(A.act, feat[ch0 + c0 + tid], d_feat[ch0 + c0 + tid]);
                s_p[tid] = argmax[ch0 + c0 + tid];
            }
            __syncthreads();
            // ---- phase 1: the channels of the chunk, bank by bank (the width is uniform over the workgroup)
            chunk_taps<VEC4>(A, ids, mask, gate, table, W, s_g, s_p, c0, c1, row0, t0, t1, grp, ngrp, sl, s_val, s_pos);
            __syncthreads();
            // ---- phase 2: the owner of a position adds the entries that target it, in index order
            // (an entry that does not target the position adds 0.0f, which changes nothing; position -1 matches nobody, so the
            // value behind it is never looked at)
            for (int e4 = 0; e4 < n_ent4 / 4; ++e4) {
                const int4 p = reinterpret_cast<const int4*>(s_pos)[e4];
                const float4 v = reinterpret_cast<const float4*>(s_val)[e4];
#pragma unroll
                for (int k = 0; k < kSalOwn; ++k) {
                    const int tk = t0 + tid + k * kSalThreads;
                    acc[k] += (p.x == tk) ? v.x : 0.f;
                    acc[k] += (p.y == tk) ? v.y : 0.f;
                    acc[k] += (p.z == tk) ? v.z : 0.f;
                    acc[k] += (p.w == tk) ? v.w : 0.f;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kSalOwn; ++k) {
            const int t = t0 + tid + k * kSalThreads;
            if (t < t1) sal[row0 + t] = acc[k];
        }
    }
}

}  // namespace rbr

using namespace rbr;

extern "C" int rbr_textcnn_saliency(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                                    const float* table, const float* const* W, const float* feat, const int32_t* argmax,
                                    const float* d_feat, float* sal, void* stream) {
    static_assert(kMaxKF == 9, "the width switch of saliency_kernel covers 1..9");
    if (!d) { set_error("rbr_textcnn_saliency: null descriptor"); return RBR_ERR_BAD_ARG; }
    if (d->n_docs == 0) return 0;
    if (!desc_valid(d)) return RBR_ERR_BAD_ARG;
    if (RBR_CONV_GATE_SPLIT_OF(d->flags)) { set_error("rbr_textcnn_saliency: RBR_CONV_GATE_SPLIT is not supported (one gate plane)"); return RBR_ERR_UNSUPPORTED; }
    if (!ids || !table || !W || !feat || !argmax || !d_feat || !sal) { set_error("rbr_textcnn_saliency: null pointer"); return RBR_ERR_BAD_ARG; }
    SalArgs A;
    PtrArray Wp;
    bool vec4;
    if (!sal_args_of(d, table, W, "rbr_textcnn_saliency", &A, &Wp, &vec4)) return RBR_ERR_BAD_ARG;
    const long long* ids64 = reinterpret_cast<const long long*>(ids);
    if (vec4)
        hipLaunchKernelGGL(saliency_kernel<true>, dim3((unsigned)A.n_docs), dim3(kSalThreads), 0, (hipStream_t)stream, A, ids64, mask,
                           gate, table, Wp, feat, argmax, d_feat, sal);
    else
        hipLaunchKernelGGL(saliency_kernel<false>, dim3((unsigned)A.n_docs), dim3(kSalThreads), 0, (hipStream_t)stream, A, ids64, mask,
                           gate, table, Wp, feat, argmax, d_feat, sal);
    RBR_CHECK_LAUNCH("textcnn saliency launch");
    return 0;
}
