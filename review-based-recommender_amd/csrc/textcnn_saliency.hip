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
#include "rbr_common.h"

namespace rbr {

constexpr int kSalThreads = 256;
constexpr int kSalChunk = 64;                       // channels per LDS chunk (x KF taps each)
constexpr int kSalOwn = 4;                          // positions a thread owns per pass
constexpr int kSalPass = kSalThreads * kSalOwn;

struct SalArgs {
    int n_docs, L, D, V, C, KF;
    int pad_mode, act, n_widths;
    int G;                                          // lanes per channel: 8, 16, 32 or 64
    int kz[RBR_MAX_WIDTHS], ch[RBR_MAX_WIDTHS], ch_off[RBR_MAX_WIDTHS];
};

// acc[j] += <x[j][:], wc[:, j]> over this lane's share of D (sub-lane sl of G); x[j] == nullptr: the tap does not contribute.
// wc = W_w[c, :, :], D * KZ contiguous floats: a lane's four consecutive d are 4 * KZ contiguous floats, read as KZ float4.
template <int KZ, bool VEC4>
__device__ __forceinline__ void tap_dots(const float* (&x)[KZ], const float* __restrict__ wc, int D, int sl, int G,
                                         float (&acc)[KZ]) {
    if (VEC4) {
        for (int d4 = sl; d4 < D / 4; d4 += G) {
            float wf[4 * KZ];
            const float4* wq = reinterpret_cast<const float4*>(wc + (long)(4 * d4) * KZ);
#pragma unroll
            for (int q = 0; q < KZ; ++q) {
                const float4 v = wq[q];
                wf[4 * q] = v.x; wf[4 * q + 1] = v.y; wf[4 * q + 2] = v.z; wf[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < KZ; ++j) {
                if (x[j] != nullptr) {                                  // uniform over the group
                    const float4 xv = *reinterpret_cast<const float4*>(x[j] + 4 * d4);
                    float s = acc[j];
                    s = fmaf(xv.x, wf[j], s);
                    s = fmaf(xv.y, wf[KZ + j], s);
                    s = fmaf(xv.z, wf[2 * KZ + j], s);
                    s = fmaf(xv.w, wf[3 * KZ + j], s);
                    acc[j] = s;
                }
            }
        }
    } else {
        for (int d = sl; d < D; d += G) {
#pragma unroll
            for (int j = 0; j < KZ; ++j)
                if (x[j] != nullptr) acc[j] = fmaf(x[j][d], wc[(long)d * KZ + j], acc[j]);
        }
    }
}

// One channel of a bank of width KZ, by one group of G lanes: the taps that land in [t0, t1) go to s_val / s_pos[e0 + j].
template <int KZ, bool VEC4>
__device__ __forceinline__ void channel_taps(const SalArgs& A, const long long* __restrict__ ids, const unsigned char* __restrict__ mask,
                                             const float* __restrict__ gate, const float* __restrict__ table,
                                             const float* __restrict__ wc, float g, int p, long row0, int t0, int t1, int sl,
                                             float* s_val, int* s_pos, int e0) {
    const int pooled = (A.pad_mode == RBR_PAD_SAME) ? A.L : A.L - KZ + 1;
    if (g == 0.f || p < 0 || p >= pooled) return;                      // nothing is indexed with such an argmax
    const int first = p - ((A.pad_mode == RBR_PAD_SAME) ? (KZ - 1) / 2 : 0);
    const float* x[KZ];
    int t[KZ];
    bool any = false;
#pragma unroll
    for (int j = 0; j < KZ; ++j) {
        // the loads of all taps are independent of each other (one round trip): a tap outside the pass reads position t0 instead
        const int q = first + j;
        const bool in_pass = q >= t0 && q < t1;
        const long at = row0 + (in_pass ? q : t0);
        const long long tok = ids[at];
        const bool open = mask == nullptr || mask[at] != 0;
        x[j] = nullptr;
        t[j] = -1;
        if (in_pass && open && tok >= 0 && tok < (long long)A.V) {      // never index the table with an id outside it
            x[j] = table + (long)tok * A.D;
            t[j] = q;
            any = true;
        }
    }
    if (!any) return;
    float acc[KZ];
#pragma unroll
    for (int j = 0; j < KZ; ++j) acc[j] = 0.f;
    tap_dots<KZ, VEC4>(x, wc, A.D, sl, A.G, acc);
#pragma unroll
    for (int j = 0; j < KZ; ++j) {
        if (t[j] >= 0) {                                                // uniform over the group
            float s = acc[j];
            for (int off = A.G >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (sl == 0) {
                const float gg = (gate != nullptr) ? g * gate[row0 + t[j]] : g;
                s_val[e0 + j] = gg * s;
                s_pos[e0 + j] = t[j];
            }
        }
    }
}

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
            for (int w = 0; w < A.n_widths; ++w) {
                const int lo = max(c0, A.ch_off[w]), hi = min(c1, A.ch_off[w] + A.ch[w]);
                const int kz = A.kz[w];
                for (int c = lo + grp; c < hi; c += ngrp) {
                    const float g = s_g[c - c0];
                    const int p = s_p[c - c0];
                    const float* wc = W.p[w] + (long)(c - A.ch_off[w]) * A.D * kz;
                    const int e0 = (c - c0) * A.KF;
#define RBR_SAL_CASE(K) case K: channel_taps<K, VEC4>(A, ids, mask, gate, table, wc, g, p, row0, t0, t1, sl, s_val, s_pos, e0); break;
                    switch (kz) {
                        RBR_SAL_CASE(1) RBR_SAL_CASE(2) RBR_SAL_CASE(3) RBR_SAL_CASE(4) RBR_SAL_CASE(5)
                        RBR_SAL_CASE(6) RBR_SAL_CASE(7) RBR_SAL_CASE(8) RBR_SAL_CASE(9)
                        default: break;
                    }
#undef RBR_SAL_CASE
                }
            }
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
    memset(&A, 0, sizeof(A));
    A.n_docs = d->n_docs; A.L = d->L; A.D = d->D; A.V = d->V;
    A.pad_mode = d->pad_mode; A.act = d->act; A.n_widths = d->n_widths;
    PtrArray Wp{};
    // float4 rows when every row of the table and of the weights starts on a 16-byte boundary, as the conv decides it
    bool vec4 = (A.D % 4 == 0) && ((((uintptr_t)table) & 15) == 0);
    for (int w = 0; w < d->n_widths; ++w) {
        if (!W[w]) { set_error("rbr_textcnn_saliency: null conv weight %d", w); return RBR_ERR_BAD_ARG; }
        A.kz[w] = d->kz[w]; A.ch[w] = d->ch[w]; A.ch_off[w] = A.C;
        A.C += d->ch[w]; A.KF = std::max(A.KF, d->kz[w]);
        Wp.p[w] = W[w];
        vec4 = vec4 && ((((uintptr_t)W[w]) & 15) == 0);
    }
    // lanes per channel: the smallest group that covers a row in at most five rounds (a function of D alone, so that a document's
    // summation order never depends on the batch)
    const int per_row = vec4 ? A.D / 4 : A.D;
    A.G = 8;
    while (A.G < kWave && (per_row + A.G - 1) / A.G > 5) A.G *= 2;
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
