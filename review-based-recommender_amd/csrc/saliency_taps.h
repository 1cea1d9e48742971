// saliency_taps.h -- phase 1 of the saliency kernels (textcnn_saliency.hip, datt_saliency.hip): the tap values of one channel.
//
// For a gradient d_feat on the pooled features, the max-pool routes g[c] = d_feat[c] * act'(feat[c]) to the ONE window argmax[c]
// of channel c; tap j of that window sits on position t = pos(argmax[c], j) and contributes
//     g[c] * mask[t] * gate[t] * <table[ids[t], :], W_w[c, :, j]>
// A group of G lanes (G = 8 .. 64 by D: at most five rounds over a row) takes one channel: it reads the channel's weights
// W_w[c, :, :] -- contiguous in memory -- once, and the kz rows of the window beside them, keeps kz partial dot products per lane
// and reduces them with a butterfly (the same order on every run); its first lane leaves each tap's value and target position in
// LDS.  What cannot contribute is dropped BEFORE any row is read: a channel with g == 0 or an argmax outside the pooled range, a
// tap outside the document or on a masked token.  Both kernels share this code, so a tap has the same bits in either.
#pragma once
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

// The kernel arguments of a descriptor: shape, banks, weight pointers and G.  float4 rows (*vec4) when every row of the table
// and of the weights starts on a 16-byte boundary, as the conv decides it.  G, the lanes per channel, is the smallest group that
// covers a row in at most five rounds (a function of D and the alignment alone, so that a document's summation order never
// depends on the batch).  False, with the error text set, when a conv weight is null.
inline bool sal_args_of(const rbr_textcnn_desc* d, const float* table, const float* const* W, const char* who, SalArgs* A,
                        PtrArray* Wp, bool* vec4) {
    memset(A, 0, sizeof(*A));
    memset(Wp, 0, sizeof(*Wp));
    A->n_docs = d->n_docs; A->L = d->L; A->D = d->D; A->V = d->V;
    A->pad_mode = d->pad_mode; A->act = d->act; A->n_widths = d->n_widths;
    *vec4 = (A->D % 4 == 0) && ((((uintptr_t)table) & 15) == 0);
    for (int w = 0; w < d->n_widths; ++w) {
        if (!W[w]) { set_error("%s: null conv weight %d", who, w); return false; }
        A->kz[w] = d->kz[w]; A->ch[w] = d->ch[w]; A->ch_off[w] = A->C;
        A->C += d->ch[w]; A->KF = std::max(A->KF, d->kz[w]);
        Wp->p[w] = W[w];
        *vec4 = *vec4 && ((((uintptr_t)W[w]) & 15) == 0);
    }
    const int per_row = *vec4 ? A->D / 4 : A->D;
    A->G = 8;
    while (A->G < kWave && (per_row + A->G - 1) / A->G > 5) A->G *= 2;
    return true;
}

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

// Phase 1 over one LDS chunk [c0, c1) of channels, bank by bank (the width is uniform over the workgroup): group grp of ngrp
// takes the chunk's channels in turn; s_g / s_p hold g and the argmax of the chunk's channels.
template <bool VEC4>
__device__ __forceinline__ void chunk_taps(const SalArgs& A, const long long* __restrict__ ids, const unsigned char* __restrict__ mask,
                                           const float* __restrict__ gate, const float* __restrict__ table, const PtrArray& W,
                                           const float* s_g, const int* s_p, int c0, int c1, long row0, int t0, int t1, int grp,
                                           int ngrp, int sl, float* s_val, int* s_pos) {
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
}

}  // namespace rbr
