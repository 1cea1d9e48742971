// ahn_tail.h -- steps 1-4 of AHN's pair tail (the user side's co-attention over one item), stated once for the two kernels that
// run them: ahn_pair_kernel (ahn_pair.hip: cached tables -> a score) and ahn_attend_fwd_kernel (ahn_attend.hip: the training op).
//   1. s[n]    = max_j X[n] . Ks[j]                     over ALL Ri*Si rows of the item (the reference masks nothing there)
//   2. w[r, :] = softmax_s(m[r, s] ? s[r, s] : -1e8)
//   3. p[r]    = relu(sum_s w[r, s] X'[r, s] + bt)
//   4. t[r]    = max_j p[r] . Kr[j];  v = softmax_r(M[r] ? t[r] : -1e8);  z = sum_r v[r] p[r]
// Step 1 is a [Ri*Si, F] x [F, Ru*Su] product on v_mfma_f32_32x32x2_f32 (exact f32 fma chains): F is streamed in slices of
// kAhnKS columns through LDS (both operands, rows beyond the operand and columns beyond F zero-filled), wave w keeps the up to
// four 32 x 32 accumulators of user rows [32 w, 32 w + 32) in registers, and the score matrix is never stored: the item's
// sentences are the MFMA's A rows, so a lane holds 16 item sentences of ONE user sentence per tile and the row max is 16 in-lane
// maxima and one exchange between the wave's halves.  Steps 2-4 are wave reductions (rbr_wave.h) in a fixed order.
//
// kSave: the training op also wants WHICH item row attained each maximum (js [NU], jr [Ru]; the backward routes through them).
// Ties go to the lowest index: a lane walks its item rows in ascending order and takes a later one only when it is strictly
// larger, and the exchange between the halves compares (value, index).  The values -- s, t and everything behind them -- are
// computed by the same instructions either way, so a pair has the same bits with and without kSave.
//
// Rules kept: every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; no atomics; every sum has
// one fixed order that depends on the shape alone.
#pragma once

#include "rbr_common.h"
#include "rbr_wave.h"

#include <cmath>
#include <cstdint>

namespace rbr {

constexpr int kAhnRows = 128;                      // cap on Ru*Su and on Ri*Si: four 32-row MFMA tiles each
constexpr int kAhnKS = 32;                         // columns of F per LDS slice
constexpr int kAhnLd = kAhnKS + 4;                 // LDS row pitch in floats (16-byte aligned rows, 4 * odd)
constexpr int kAhnTile = 4;                        // pairs per workgroup
constexpr int kAhnLds = 2 * kAhnRows * kAhnLd;     // floats: the two operand slices, later p [Ru, F] and z [F]
constexpr int kAhnSuMax = 64, kAhnRuMax = 64;      // one wave holds a review's sentences / a user's reviews in its lanes
constexpr int kAhnFMax = 2048;
constexpr float kAhnMaskFill = -1e8f;              // the reference's fill of masked scores (utils.py:13)

typedef float ahn_f32x16 __attribute__((ext_vector_type(16)));

struct AhnTail {
    const float *X, *Xt;                           // user state
    const unsigned char *usm, *urm;
    const float *Ks, *Kr;                          // item state
    const float* bt;
    float *w_out, *v_out;                          // [pairs, NU] / [pairs, Ru]; each may be null
    int *js_out, *jr_out;                          // kSave: [pairs, NU] / [pairs, Ru]
    int Ru, Su, NU, NJ, Ri, F;                     // NU = Ru * Su, NJ = Ri * Si
    int vec;
};

// One pair: user state row u, item state row i, output slot q.  Every thread of the workgroup (256) makes the call; smem holds
// kAhnLds floats, 16-byte aligned.  On return p [Ru, F] stands at smem and z [F] at smem + Ru * F, behind a barrier.
template <bool kSave>
__device__ __forceinline__ void ahn_tail(const AhnTail& A, long long u, long long i, long long q, float* __restrict__ smem,
                                         float* __restrict__ s_s, float* __restrict__ w_s, float* __restrict__ t_s,
                                         float* __restrict__ v_s) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int F = A.F, NU = A.NU, NJ = A.NJ, Ru = A.Ru, Su = A.Su, Ri = A.Ri;
    const float* __restrict__ Xu = A.X + (size_t)u * NU * F;
    const float* __restrict__ Ki = A.Ks + (size_t)i * NJ * F;
    float* As = smem;                              // item sentences: the MFMA's A rows
    float* Bs = smem + kAhnRows * kAhnLd;          // user sentences: the MFMA's B columns
    const int nct = (NJ + 31) >> 5;                // item tiles
    const bool mine = wave * 32 < NU;              // wave-uniform: this wave's user rows exist

    // ---- 1. s[n] = max_j X[n] . Ks[j]
    ahn_f32x16 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    for (int k0 = 0; k0 < F; k0 += kAhnKS) {
        __syncthreads();                           // the previous slice's (the previous pair's) LDS reads are done
        if (A.vec) {                               // F % 4 == 0, 16-byte aligned tables: 8 lanes per row
            for (int e = tid; e < kAhnRows * (kAhnKS / 4); e += 256) {
                const int row = e >> 3, kk = (e & 7) * 4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (k0 + kk < F) {
                    if (row < NJ) a = *reinterpret_cast<const float4*>(Ki + (size_t)row * F + k0 + kk);
                    if (row < NU) b = *reinterpret_cast<const float4*>(Xu + (size_t)row * F + k0 + kk);
                }
                *reinterpret_cast<float4*>(As + row * kAhnLd + kk) = a;
                *reinterpret_cast<float4*>(Bs + row * kAhnLd + kk) = b;
            }
        } else {
            for (int e = tid; e < kAhnRows * kAhnKS; e += 256) {
                const int row = e >> 5, kk = e & 31;
                const bool in = k0 + kk < F;
                As[row * kAhnLd + kk] = (in && row < NJ) ? Ki[(size_t)row * F + k0 + kk] : 0.f;
                Bs[row * kAhnLd + kk] = (in && row < NU) ? Xu[(size_t)row * F + k0 + kk] : 0.f;
            }
        }
        __syncthreads();
        if (mine) {
            // lane (col, half) supplies k = 8 q + 4 half + {0, 1, 2, 3} of its row: one 16-byte LDS read per operand and 8 k
            const int steps = (min(kAhnKS, F - k0) + 7) >> 3;
            const float* pb = Bs + (wave * 32 + col) * kAhnLd + 4 * half;
            const float* pa = As + col * kAhnLd + 4 * half;
            for (int qd = 0; qd < steps; ++qd) {
                const float4 b = *reinterpret_cast<const float4*>(pb + 8 * qd);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (ct < nct) {
                        const float4 a = *reinterpret_cast<const float4*>(pa + ct * 32 * kAhnLd + 8 * qd);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[ct], 0, 0, 0);
                    }
                }
            }
        }
    }
    {   // register r of tile ct is item sentence ct * 32 + (r & 3) + 8 (r >> 2) + 4 half of user sentence wave * 32 + col:
        // ascending in (ct, r), so "strictly larger" keeps the lane's lowest index
        float mx = -INFINITY;
        int jx = 0;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (j < NJ) {
                    if (kSave && acc[ct][r] > mx) jx = j;
                    mx = fmaxf(mx, acc[ct][r]);
                }
            }
        const float ox = __shfl_xor(mx, 32);
        if (kSave) {                               // the halves hold interleaved rows: compare (value, index)
            const int oj = __shfl_xor(jx, 32);
            if (ox > mx || (ox == mx && oj < jx)) jx = oj;
        }
        mx = fmaxf(mx, ox);
        const int n = wave * 32 + col;
        if (half == 0 && n < NU) {
            s_s[n] = mx;
            if (kSave) A.js_out[(size_t)q * NU + n] = jx;
        }
    }
    __syncthreads();                               // s is complete, and the slices are free: p and z take their place

    // ---- 2. w[r, :] = softmax over the review's sentences, a wave per review
    const unsigned char* __restrict__ sm = A.usm + (size_t)u * NU;
    for (int r = wave; r < Ru; r += 4) {
        const bool in = lane < Su;
        const int n = r * Su + (in ? lane : 0);
        const float x = in ? (sm[n] ? s_s[n] : kAhnMaskFill) : -INFINITY;
        const float m = wave_max(x);
        const float e = in ? expf(x - m) : 0.f;
        const float w = e / wave_sum(e);
        if (in) {
            w_s[n] = w;
            if (A.w_out) A.w_out[(size_t)q * NU + n] = w;
        }
    }
    __syncthreads();

    // ---- 3. p[r] = relu(sum_s w[r, s] X'[r, s] + bt), s ascending
    float* p_s = smem;
    float* z_s = smem + Ru * F;
    const float* __restrict__ Xtu = A.Xt + (size_t)u * NU * F;
    for (int idx = tid; idx < Ru * F; idx += 256) {
        const int r = idx / F, f = idx - r * F;
        float a = 0.f;
        for (int s = 0; s < Su; ++s) a = fmaf(w_s[r * Su + s], Xtu[(size_t)(r * Su + s) * F + f], a);
        a += A.bt[f];
        p_s[idx] = (a < 0.f) ? 0.f : a;            // not fmaxf: it would turn NaN into 0 (torch.relu(NaN) is NaN)
    }
    __syncthreads();

    // ---- 4. t[r] = max_j p[r] . Kr[j], a wave per review; v = softmax over the reviews; z = sum_r v[r] p[r]
    const float* __restrict__ Kri = A.Kr + (size_t)i * Ri * F;
    for (int r = wave; r < Ru; r += 4) {
        float t = -INFINITY;
        int jt = 0;
        for (int j = 0; j < Ri; ++j) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(p_s[r * F + f], Kri[(size_t)j * F + f], d);
            const float dj = wave_sum(d);
            if (kSave && dj > t) jt = j;
            t = fmaxf(t, dj);
        }
        if (lane == 0) {
            t_s[r] = t;
            if (kSave) A.jr_out[(size_t)q * Ru + r] = jt;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const bool in = lane < Ru;
        const int r = in ? lane : 0;
        const float x = in ? (A.urm[(size_t)u * Ru + r] ? t_s[r] : kAhnMaskFill) : -INFINITY;
        const float m = wave_max(x);
        const float e = in ? expf(x - m) : 0.f;
        const float v = e / wave_sum(e);
        if (in) {
            v_s[r] = v;
            if (A.v_out) A.v_out[(size_t)q * Ru + r] = v;
        }
    }
    __syncthreads();
    for (int f = tid; f < F; f += 256) {
        float a = 0.f;
        for (int r = 0; r < Ru; ++r) a = fmaf(v_s[r], p_s[r * F + f], a);
        z_s[f] = a;
    }
    __syncthreads();
}

}  // namespace rbr
