// ahn_attend.hip -- AHN's user-side co-attention as ONE differentiable op for training: steps 1-4 of the pair tail (ahn_tail.h,
// the arithmetic and summation order of ahn_pair.hip) forward, and their backward.
//
// Grouped layout: G = 1 + n_neg groups of B pairs; pair p = g * B + b reads user row b and item row p -- sample_negatives'
// layout, rows [0, B) the observed pairs, then the slabs of negatives.  A user is encoded once and attends to G items.
//
// Forward (ahn_attend_fwd_kernel): ahn_pair_kernel's work split -- a workgroup of 4 waves walks kAhnTile consecutive pairs --
// with ahn_tail<true>, which also records WHICH item row attained each of the two maxima (js [P, NU], jr [P, Ru]; ties to the
// lowest index), and p [P, Ru, F] and z [P, F] copied out of LDS.
//
// Backward (ahn_attend_bwd_kernel): ONE workgroup per user walks its pairs g = 0 .. G-1 in order, so the user-side gradients
// dX / dXt [B, NU, F] are the sum over a user's pairs in that order, by the thread that owns the element (stored at g = 0, added
// to afterwards), and so is the user's partial of dbt (registers; [B, F] partials, which the caller adds up over the users).
// Per pair, from dz [F]:
//   dv[r] = dz . p[r];  c = sum_r v[r] dv[r];  dt[r] = M[r] ? v[r] (dv[r] - c) : 0
//   da[r] = p[r] > 0 ? v[r] dz + dt[r] Kr[jr[r]] : 0                              (LDS, [Ru, F])
//   dKr[j] = sum_{r: jr[r] = j} dt[r] p[r], r ascending
//   e[n] = da[r(n)] . Xt[n];  cs[r] = sum_s w[r, s] e[r, s];  ds[n] = m[n] ? w[n] (e[n] - cs[r]) : 0
//   dXt[n] += w[n] da[r(n)];  dX[n] += ds[n] Ks[js[n]]
//   dKs[j] = sum_{n: js[n] = j} ds[n] X[n], n ascending -- over a per-row list (head / next in LDS, built by the row's own thread)
// dKs / dKr are overwritten whole: a row nobody selected is zeros.  js / jr come back from memory as row indices and are clamped
// into [0, NJ) / [0, Ri) before they address anything.
//
// Rules kept: no float atomics; every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; every
// sum has one order that the shape fixes, so the same inputs give the same bits on every run and a pair's dKs / dKr do not
// depend on where it stands in the launch.
//
// LDS of the backward: dz [F] and da [Ru, F] -- (Ru + 1) * F floats, the forward's own cap of 9216 (36 KB) -- beside 3 KB of
// per-row scalars.  The caps are therefore the forward's: Ru, Su <= 64, NU, NJ <= 128, F <= 2048, (Ru + 1) * F <= 9216.
#include "ahn_tail.h"

namespace rbr {

struct AhnAttend {
    AhnTail T;
    const float *w, *v, *p, *dz;                   // backward: the forward's outputs and the incoming gradient
    const int *js, *jr;
    float *z, *p_out;                              // forward
    float *dX, *dXt, *dKs, *dKr, *dbt_part;        // backward
    int B, G;
};

__global__ __launch_bounds__(256) void ahn_attend_fwd_kernel(const AhnAttend A) {
    __shared__ __attribute__((aligned(16))) float smem[kAhnLds];
    __shared__ float s_s[kAhnRows], w_s[kAhnRows], t_s[kAhnRuMax], v_s[kAhnRuMax];
    const long long P = (long long)A.B * A.G;
    const int RF = A.T.Ru * A.T.F, F = A.T.F;
    // the trip count depends on the block alone: whole workgroups reach the barriers of ahn_tail
    for (int t = 0; t < kAhnTile; ++t) {
        const long long q = (long long)blockIdx.x * kAhnTile + t;
        if (q >= P) break;
        ahn_tail<true>(A.T, q % A.B, q, q, smem, s_s, w_s, t_s, v_s);
        // p [Ru, F] and z [F] stand in LDS behind a barrier; the next pair's first barrier keeps them until these reads are done
        for (int idx = threadIdx.x; idx < RF; idx += 256) A.p_out[(size_t)q * RF + idx] = smem[idx];
        for (int f = threadIdx.x; f < F; f += 256) A.z[(size_t)q * F + f] = smem[RF + f];
    }
}

__global__ __launch_bounds__(256) void ahn_attend_bwd_kernel(const AhnAttend A) {
    __shared__ __attribute__((aligned(16))) float smem[kAhnLds];           // dz [F], da [Ru, F]
    __shared__ float w_s[kAhnRows], e_s[kAhnRows], ds_s[kAhnRows], v_s[kAhnRuMax], dv_s[kAhnRuMax], dt_s[kAhnRuMax];
    __shared__ int js_s[kAhnRows], next_s[kAhnRows], head_s[kAhnRows], jr_s[kAhnRuMax];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int F = A.T.F, NU = A.T.NU, NJ = A.T.NJ, Ru = A.T.Ru, Su = A.T.Su, Ri = A.T.Ri, B = A.B;
    const int b = blockIdx.x;
    float* dz_s = smem;
    float* da_s = smem + F;
    const float* __restrict__ Xu = A.T.X + (size_t)b * NU * F;
    const float* __restrict__ Xtu = A.T.Xt + (size_t)b * NU * F;
    const unsigned char* __restrict__ sm = A.T.usm + (size_t)b * NU;
    const unsigned char* __restrict__ rm = A.T.urm + (size_t)b * Ru;
    float* __restrict__ dXu = A.dX + (size_t)b * NU * F;
    float* __restrict__ dXtu = A.dXt + (size_t)b * NU * F;
    float dbt[kAhnFMax / 256];                     // this thread's columns f = tid + 256 k of the user's dbt partial
#pragma unroll
    for (int k = 0; k < kAhnFMax / 256; ++k) dbt[k] = 0.f;

    for (int g = 0; g < A.G; ++g) {                // G is the launch's: every workgroup makes the same trips
        const size_t q = (size_t)g * B + b;
        const float* __restrict__ pq = A.p + q * Ru * F;
        const float* __restrict__ Ksq = A.T.Ks + q * NJ * F;
        const float* __restrict__ Krq = A.T.Kr + q * Ri * F;
        float* __restrict__ dKsq = A.dKs + q * NJ * F;
        float* __restrict__ dKrq = A.dKr + q * Ri * F;
        __syncthreads();                           // the previous pair's LDS reads are done
        for (int f = tid; f < F; f += 256) dz_s[f] = A.dz[q * F + f];
        if (tid < NU) {
            w_s[tid] = A.w[q * NU + tid];
            js_s[tid] = min(max(A.js[q * NU + tid], 0), NJ - 1);
        }
        if (tid < Ru) {
            v_s[tid] = A.v[q * Ru + tid];
            jr_s[tid] = min(max(A.jr[q * Ru + tid], 0), Ri - 1);
        }
        __syncthreads();

        // ---- dv[r] = dz . p[r], a wave per review; the item rows' lists: head[j] -> next[n] -> ..., n ascending
        for (int r = wave; r < Ru; r += 4) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(dz_s[f], pq[r * F + f], d);
            d = wave_sum(d);
            if (lane == 0) dv_s[r] = d;
        }
        if (tid < NJ) {
            int head = -1;
            for (int n = NU - 1; n >= 0; --n)
                if (js_s[n] == tid) { next_s[n] = head; head = n; }
            head_s[tid] = head;
        }
        __syncthreads();

        // ---- dt[r] = M[r] ? v[r] (dv[r] - c) : 0 with c = sum_r v[r] dv[r], r ascending
        if (tid < Ru) {
            float c = 0.f;
            for (int r = 0; r < Ru; ++r) c = fmaf(v_s[r], dv_s[r], c);
            dt_s[tid] = rm[tid] ? v_s[tid] * (dv_s[tid] - c) : 0.f;
        }
        __syncthreads();

        // ---- da[r] = relu'(p[r]) (v[r] dz + dt[r] Kr[jr[r]])
        for (int idx = tid; idx < Ru * F; idx += 256) {
            const int r = idx / F, f = idx - r * F;
            const float dp = fmaf(dt_s[r], Krq[(size_t)jr_s[r] * F + f], v_s[r] * dz_s[f]);
            da_s[idx] = pq[idx] > 0.f ? dp : 0.f;
        }
        __syncthreads();

        // ---- dbt += sum_r da[r];  dKr[j] = sum_{r: jr[r] = j} dt[r] p[r];  e[n] = da[r(n)] . Xt[n], a wave per sentence
#pragma unroll
        for (int k = 0; k < kAhnFMax / 256; ++k) {
            const int f = tid + 256 * k;
            if (f < F) {
                float a = 0.f;
                for (int r = 0; r < Ru; ++r) a += da_s[r * F + f];
                dbt[k] += a;
            }
        }
        for (int idx = tid; idx < Ri * F; idx += 256) {
            const int j = idx / F, f = idx - j * F;
            float a = 0.f;
            for (int r = 0; r < Ru; ++r)
                if (jr_s[r] == j) a = fmaf(dt_s[r], pq[r * F + f], a);
            dKrq[idx] = a;
        }
        for (int n = wave; n < NU; n += 4) {
            const int r = n / Su;
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(da_s[r * F + f], Xtu[(size_t)n * F + f], d);
            d = wave_sum(d);
            if (lane == 0) e_s[n] = d;
        }
        __syncthreads();

        // ---- ds[n] = m[n] ? w[n] (e[n] - cs[r]) : 0 with cs[r] = sum_s w[r, s] e[r, s], s ascending
        if (tid < NU) {
            const int r = tid / Su;
            float cs = 0.f;
            for (int s = 0; s < Su; ++s) cs = fmaf(w_s[r * Su + s], e_s[r * Su + s], cs);
            ds_s[tid] = sm[tid] ? w_s[tid] * (e_s[tid] - cs) : 0.f;
        }
        __syncthreads();

        // ---- dXt[n] += w[n] da[r(n)];  dX[n] += ds[n] Ks[js[n]]: the element's own thread, g ascending
        for (int idx = tid; idx < NU * F; idx += 256) {
            const int n = idx / F, f = idx - n * F;
            const float a = w_s[n] * da_s[(n / Su) * F + f];
            const float x = ds_s[n] * Ksq[(size_t)js_s[n] * F + f];
            if (g == 0) { dXtu[idx] = a; dXu[idx] = x; }
            else { dXtu[idx] += a; dXu[idx] += x; }
        }
        // ---- dKs[j] = sum_{n: js[n] = j} ds[n] X[n], along the row's list
        for (int idx = tid; idx < NJ * F; idx += 256) {
            const int j = idx / F, f = idx - j * F;
            float a = 0.f;
            for (int n = head_s[j]; n >= 0; n = next_s[n]) a = fmaf(ds_s[n], Xu[(size_t)n * F + f], a);
            dKsq[idx] = a;
        }
    }
#pragma unroll
    for (int k = 0; k < kAhnFMax / 256; ++k) {
        const int f = tid + 256 * k;
        if (f < F) A.dbt_part[(size_t)b * F + f] = dbt[k];
    }
}

static int attend_args_ok(const char* what, const rbr_ahn_shape* s, int32_t B, int32_t G) {
    if (!s) { set_error("%s: null shape", what); return RBR_ERR_BAD_ARG; }
    if (s->Ru <= 0 || s->Su <= 0 || s->Ri <= 0 || s->Si <= 0 || s->F <= 0) {
        set_error("%s: bad shape Ru=%d Su=%d Ri=%d Si=%d F=%d", what, s->Ru, s->Su, s->Ri, s->Si, s->F);
        return RBR_ERR_BAD_ARG;
    }
    if (s->Ru > kAhnRuMax || s->Su > kAhnSuMax || (long long)s->Ru * s->Su > kAhnRows || (long long)s->Ri * s->Si > kAhnRows ||
        s->F > kAhnFMax || ((long long)s->Ru + 1) * s->F > kAhnLds) {
        set_error("%s: shape Ru=%d Su=%d Ri=%d Si=%d F=%d is outside the caps Ru <= %d, Su <= %d, Ru*Su <= %d, Ri*Si <= %d, F <= %d, "
                  "(Ru + 1) * F <= %d", what, s->Ru, s->Su, s->Ri, s->Si, s->F, kAhnRuMax, kAhnSuMax, kAhnRows, kAhnRows, kAhnFMax,
                  kAhnLds);
        return RBR_ERR_BAD_ARG;
    }
    if (B < 0 || G < 1) { set_error("%s: B=%d must be at least 0 and G=%d at least 1", what, B, G); return RBR_ERR_BAD_ARG; }
    if ((long long)B * G > 0x7fffffffLL) {
        set_error("%s: P = G * B = %d * %d pairs must stay below 2^31", what, G, B);
        return RBR_ERR_BAD_ARG;
    }
    return 0;
}

static void attend_fill(AhnAttend& A, const rbr_ahn_shape* s, int32_t B, int32_t G, const float* X, const float* Xt,
                        const uint8_t* sent_mask, const uint8_t* rev_mask, const float* Ks, const float* Kr) {
    A = AhnAttend{};
    A.T.X = X; A.T.Xt = Xt; A.T.usm = sent_mask; A.T.urm = rev_mask; A.T.Ks = Ks; A.T.Kr = Kr;
    A.T.Ru = s->Ru; A.T.Su = s->Su; A.T.NU = s->Ru * s->Su; A.T.NJ = s->Ri * s->Si; A.T.Ri = s->Ri; A.T.F = s->F;
    const auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
    A.T.vec = (s->F % 4 == 0 && aligned(X) && aligned(Ks)) ? 1 : 0;
    A.B = B; A.G = G;
}

}  // namespace rbr

extern "C" int rbr_ahn_pair_attend_fwd(const rbr_ahn_shape* shape, int32_t B, int32_t G, const float* X, const float* Xt,
                                       const uint8_t* sent_mask, const uint8_t* rev_mask, const float* Ks, const float* Kr,
                                       const float* bt, float* z, float* w, float* v, int32_t* js, int32_t* jr, float* p,
                                       void* stream) {
    using namespace rbr;
    const char* what = "rbr_ahn_pair_attend_fwd";
    if (int e = attend_args_ok(what, shape, B, G)) return e;
    if (!X || !Xt || !sent_mask || !rev_mask || !Ks || !Kr || !bt || !z || !w || !v || !js || !jr || !p) {
        set_error("%s: null pointer", what);
        return RBR_ERR_BAD_ARG;
    }
    if (B == 0) return 0;
    AhnAttend A;
    attend_fill(A, shape, B, G, X, Xt, sent_mask, rev_mask, Ks, Kr);
    A.T.bt = bt; A.T.w_out = w; A.T.v_out = v; A.T.js_out = js; A.T.jr_out = jr;
    A.z = z; A.p_out = p;
    const long long P = (long long)B * G;
    hipLaunchKernelGGL(ahn_attend_fwd_kernel, dim3((unsigned)((P + kAhnTile - 1) / kAhnTile)), dim3(256), 0, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("ahn_pair_attend_fwd launch");
    return 0;
}

extern "C" int rbr_ahn_pair_attend_bwd(const rbr_ahn_shape* shape, int32_t B, int32_t G, const float* X, const float* Xt,
                                       const uint8_t* sent_mask, const uint8_t* rev_mask, const float* Ks, const float* Kr,
                                       const float* w, const float* v, const int32_t* js, const int32_t* jr, const float* p,
                                       const float* dz, float* dX, float* dXt, float* dKs, float* dKr, float* dbt_part,
                                       void* stream) {
    using namespace rbr;
    const char* what = "rbr_ahn_pair_attend_bwd";
    if (int e = attend_args_ok(what, shape, B, G)) return e;
    if (!X || !Xt || !sent_mask || !rev_mask || !Ks || !Kr || !w || !v || !js || !jr || !p || !dz || !dX || !dXt || !dKs || !dKr ||
        !dbt_part) {
        set_error("%s: null pointer", what);
        return RBR_ERR_BAD_ARG;
    }
    if (B == 0) return 0;
    AhnAttend A;
    attend_fill(A, shape, B, G, X, Xt, sent_mask, rev_mask, Ks, Kr);
    A.w = w; A.v = v; A.js = js; A.jr = jr; A.p = p; A.dz = dz;
    A.dX = dX; A.dXt = dXt; A.dKs = dKs; A.dKr = dKr; A.dbt_part = dbt_part;
    hipLaunchKernelGGL(ahn_attend_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("ahn_pair_attend_bwd launch");
    return 0;
}
