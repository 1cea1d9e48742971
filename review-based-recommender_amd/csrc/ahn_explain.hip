// ahn_explain.hip -- why an AHN pair scored as it did, from the cached per-id sentence tables of ahn_pair.hip, one launch per
// block of pairs: the score kernel's forward and, behind it, gradient x input of every sentence and review, reduced to scalars.
//
// Forward: ahn_tail<true> (steps 1-4 and the max routing js [NU], jr [Ru]) and ahn_fm<true> (step 5 and xv [K]) -- the
// instructions of ahn_pair_kernel, so score, w and v have its bits, and js, jr those of ahn_attend_fwd_kernel.
//
// Backward, per pair.  The FM is a closed form, so with xv[k] = (z . VzT[k] + fm_u[k]) + fm_i[k]
//   dz[f] = sum_k xv[k] VzT[k, f] - z[f] vz2[f] + lz[f]
//   dq[f] = sum_k xv[k] VqT[k, f] - q[f] vq2[f] + lq[f]          q = sum_i beta[i] r'[i], the item's own pooled vector
// and the user side is ahn_attend_bwd_kernel's chain with every vector gradient replaced by its dot with the vector it belongs to:
//   dv[r] = dz . p[r];  c = sum_r v[r] dv[r];  dt[r] = M[r] ? v[r] (dv[r] - c) : 0
//   da[r] = [p[r] > 0] (v[r] dz + dt[r] Kr[jr[r]])  -- formed on the fly while a wave walks sentence n's row of Xt, never stored
//   e[n] = da[r(n)] . Xt[n];  cs[r] = sum_s w[r, s] e[r, s];  ds[n] = m[n] ? w[n] (e[n] - cs[r]) : 0
//   user_sentences[n]       = w[n] e[n] + ds[n] s[n]             (= <dX[n], X[n]> + <dXt[n], Xt[n]>: s[n] = X[n] . Ks[js[n]])
//   user_sentences_fixed[n] = w[n] <[p[r] > 0] v[r] dz, Xt[n]>   (both attention weightings held constant)
//   user_reviews[r] = v[r] dv[r];  user_text = dz . z
//   item_sentence_match[j] = sum_{n: js[n] = j} ds[n] s[n], n ascending     (= <dKs[j], Ks[j]>)
//   item_review_match[k]   = sum_{r: jr[r] = k} dt[r] t[r], r ascending     (= <dKr[k], Kr[k]>: t[r] = p[r] . Kr[jr[r]])
//   item_reviews[i] = beta[i] <dq, r'[i]>;  item_text = dq . q              (the item's own attention weights held constant)
// No [pairs, rows, F] gradient is written: the explanation costs the score's forward plus one more pass over the user's Xt
// (NU * F floats, what step 3 already reads) and Ri * F floats of r'.
//
// Work split: ahn_pair_kernel's -- a workgroup of 4 waves walks kAhnTile consecutive pairs.  LDS: the tail's kAhnLds floats
// (36 KB; p and z, later q), dz [kAhnFMax] (8 KB; later dq) and 4 KB of per-row scalars: 48 KB static.
//
// Rules kept: every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; no atomics but the id
// error record; every sum has one fixed order that depends on the shape alone, so a pair has the same bits in every tile
// position, in a launch of any length and on every run.
#include "ahn_pair.h"

namespace rbr {

struct AhnExplain : AhnPair {
    const float *Rp, *beta;                        // item rows: r' [I, Ri, F], beta [I, Ri]
    const float *VqT, *vq2, *lq;                   // block 2 of the FM
    float *us_out, *usf_out, *ur_out, *ut_out;     // user_sentences, user_sentences_fixed [P, NU]; user_reviews [P, Ru]; user_text [P]
    float *ism_out, *irm_out, *ir_out, *it_out;    // item_sentence_match [P, NJ]; item_review_match, item_reviews [P, Ri]; item_text [P]
};

// two waves per SIMD: the saved routing costs registers (254 without the hint, one wave per SIMD); 256 fit with no scratch
__global__ __launch_bounds__(256, 2) void ahn_explain_kernel(const AhnExplain A) {
    __shared__ __attribute__((aligned(16))) float smem[kAhnLds];
    __shared__ float dz_s[kAhnFMax];
    __shared__ float s_s[kAhnRows], w_s[kAhnRows], e_s[kAhnRows], ef_s[kAhnRows], dss_s[kAhnRows];
    __shared__ float t_s[kAhnRuMax], v_s[kAhnRuMax], dv_s[kAhnRuMax], dt_s[kAhnRuMax], red_s[kAhnKMax + 2], xv_s[kAhnKMax];
    __shared__ int js_s[kAhnRows], jr_s[kAhnRuMax];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int F = A.F, K = A.K, NU = A.NU, NJ = A.NJ, Ru = A.Ru, Su = A.Su, Ri = A.Ri;
    // the trip count depends on the block alone: whole workgroups reach the barriers below
    for (int tile = 0; tile < kAhnTile; ++tile) {
        const long long q = (long long)blockIdx.x * kAhnTile + tile;
        if (q >= A.P) break;
        const long long u = ahn_checked(ahn_row(A.u_rows, q, A.idx64), A.U, 0, A.err);
        const long long i = ahn_checked(ahn_row(A.i_rows, q, A.idx64), A.I, 1, A.err);
        ahn_tail<true>(A, u, i, q, smem, s_s, w_s, t_s, v_s);         // ---- 1-4: p [Ru, F] and z [F] in LDS, behind a barrier
        const float* p_s = smem;
        const float* z_s = smem + Ru * F;
        ahn_fm<true>(A, u, i, q, z_s, red_s, xv_s);                   // ---- 5: the score; xv [K] behind the barrier inside

        // ---- dz[f] = sum_k xv[k] VzT[k, f] - z[f] vz2[f] + lz[f], k ascending; the routing comes back from the pair's own rows
        for (int f = tid; f < F; f += 256) {
            float a = 0.f;
            for (int k = 0; k < K; ++k) a = fmaf(xv_s[k], A.VzT[(size_t)k * F + f], a);
            dz_s[f] = (a - z_s[f] * A.vz2[f]) + A.lz[f];
        }
        if (tid < NU) js_s[tid] = min(max(A.js_out[(size_t)q * NU + tid], 0), NJ - 1);
        if (tid < Ru) jr_s[tid] = min(max(A.jr_out[(size_t)q * Ru + tid], 0), Ri - 1);
        __syncthreads();

        // ---- dv[r] = dz . p[r], a wave per review; user_text = dz . z
        for (int r = wave; r < Ru; r += 4) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(dz_s[f], p_s[r * F + f], d);
            d = wave_sum(d);
            if (lane == 0) dv_s[r] = d;
        }
        if (wave == 0) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(dz_s[f], z_s[f], d);
            d = wave_sum(d);
            if (lane == 0) A.ut_out[q] = d;
        }
        __syncthreads();

        // ---- dt[r] = M[r] ? v[r] (dv[r] - c) : 0 with c = sum_r v[r] dv[r], r ascending
        if (tid < Ru) {
            float c = 0.f;
            for (int r = 0; r < Ru; ++r) c = fmaf(v_s[r], dv_s[r], c);
            dt_s[tid] = A.urm[(size_t)u * Ru + tid] ? v_s[tid] * (dv_s[tid] - c) : 0.f;
            A.ur_out[(size_t)q * Ru + tid] = v_s[tid] * dv_s[tid];
        }
        __syncthreads();

        // ---- item_review_match[k] = sum_{r: jr[r] = k} dt[r] t[r]; e[n] = da[r(n)] . Xt[n] and its fixed part, a wave per sentence
        if (tid < Ri) {
            float a = 0.f;
            for (int r = 0; r < Ru; ++r)
                if (jr_s[r] == tid) a = fmaf(dt_s[r], t_s[r], a);
            A.irm_out[(size_t)q * Ri + tid] = a;
        }
        const float* __restrict__ Xtu = A.Xt + (size_t)u * NU * F;
        const float* __restrict__ Kri = A.Kr + (size_t)i * Ri * F;
        for (int n = wave; n < NU; n += 4) {
            const int r = n / Su;
            const float vr = v_s[r], dtr = dt_s[r];
            const float* __restrict__ kr = Kri + (size_t)jr_s[r] * F;
            float d = 0.f, df = 0.f;
            for (int f = lane; f < F; f += 64) {
                const float fixed = vr * dz_s[f];
                const float dp = fmaf(dtr, kr[f], fixed);
                const bool live = p_s[r * F + f] > 0.f;
                const float x = Xtu[(size_t)n * F + f];
                d = fmaf(live ? dp : 0.f, x, d);
                df = fmaf(live ? fixed : 0.f, x, df);
            }
            d = wave_sum(d);
            df = wave_sum(df);
            if (lane == 0) { e_s[n] = d; ef_s[n] = df; }
        }
        __syncthreads();                           // p and dz are read no more: q and dq take their place

        // ---- ds[n] = m[n] ? w[n] (e[n] - cs[r]) : 0 with cs[r] = sum_s w[r, s] e[r, s], s ascending; the two sentence outputs
        if (tid < NU) {
            const int r = tid / Su;
            float cs = 0.f;
            for (int s = 0; s < Su; ++s) cs = fmaf(w_s[r * Su + s], e_s[r * Su + s], cs);
            const float ds = A.usm[(size_t)u * NU + tid] ? w_s[tid] * (e_s[tid] - cs) : 0.f;
            const float routed = ds * s_s[tid];
            dss_s[tid] = routed;
            A.us_out[(size_t)q * NU + tid] = fmaf(w_s[tid], e_s[tid], routed);
            A.usf_out[(size_t)q * NU + tid] = w_s[tid] * ef_s[tid];
        }
        // ---- q[f] = sum_i beta[i] r'[i, f], i ascending; dq[f] = sum_k xv[k] VqT[k, f] - q[f] vq2[f] + lq[f]
        float* q_s = smem;
        float* dq_s = dz_s;
        const float* __restrict__ Rpi = A.Rp + (size_t)i * Ri * F;
        const float* __restrict__ bi = A.beta + (size_t)i * Ri;
        for (int f = tid; f < F; f += 256) {
            float qf = 0.f;
            for (int r = 0; r < Ri; ++r) qf = fmaf(bi[r], Rpi[(size_t)r * F + f], qf);
            float a = 0.f;
            for (int k = 0; k < K; ++k) a = fmaf(xv_s[k], A.VqT[(size_t)k * F + f], a);
            q_s[f] = qf;
            dq_s[f] = (a - qf * A.vq2[f]) + A.lq[f];
        }
        __syncthreads();

        // ---- item_sentence_match[j] = sum_{n: js[n] = j} ds[n] s[n], n ascending; item_reviews[i] = beta[i] <dq, r'[i]>, a wave
        //      per review; item_text = dq . q
        if (tid < NJ) {
            float a = 0.f;
            for (int n = 0; n < NU; ++n)
                if (js_s[n] == tid) a += dss_s[n];
            A.ism_out[(size_t)q * NJ + tid] = a;
        }
        for (int r = wave; r < Ri; r += 4) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(dq_s[f], Rpi[(size_t)r * F + f], d);
            d = wave_sum(d);
            if (lane == 0) A.ir_out[(size_t)q * Ri + r] = bi[r] * d;
        }
        if (wave == 0) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(dq_s[f], q_s[f], d);
            d = wave_sum(d);
            if (lane == 0) A.it_out[q] = d;
        }
        // the next pair's ahn_tail opens with a barrier before it writes LDS
    }
}

}  // namespace rbr

extern "C" int rbr_ahn_pair_explain_ids(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                                        const rbr_ahn_head* head, const rbr_ahn_explain_rows* extra, int64_t P, const void* u_rows,
                                        const void* i_rows, int32_t index_bits, const rbr_ahn_explain_out* out, int64_t* err,
                                        void* stream) {
    using namespace rbr;
    const char* what = "rbr_ahn_pair_explain_ids";
    if (int e = ahn_args_ok(what, shape, user, item, head)) return e;
    if (!extra || !out) { set_error("%s: null argument struct", what); return RBR_ERR_BAD_ARG; }
    if (P <= 0 || P > (int64_t)0x7fffffff) { set_error("%s: P=%lld must be in 1 .. 2^31 - 1", what, (long long)P); return RBR_ERR_BAD_ARG; }
    if (index_bits != 32 && index_bits != 64) { set_error("%s: index_bits=%d must be 32 or 64", what, index_bits); return RBR_ERR_BAD_ARG; }
    if (!u_rows || !i_rows || !extra->Rp || !extra->beta || !extra->VqT || !extra->vq2 || !extra->lq) {
        set_error("%s: null pointer", what);
        return RBR_ERR_BAD_ARG;
    }
    if (!out->score || !out->w || !out->v || !out->js || !out->jr || !out->user_sentences || !out->user_sentences_fixed ||
        !out->user_reviews || !out->user_text || !out->item_sentence_match || !out->item_review_match || !out->item_reviews ||
        !out->item_text) {
        set_error("%s: null output", what);
        return RBR_ERR_BAD_ARG;
    }
    AhnExplain A;
    ahn_fill(A, shape, user, item, head);
    A.u_rows = u_rows; A.i_rows = i_rows; A.idx64 = index_bits == 64;
    A.out = out->score; A.w_out = out->w; A.v_out = out->v; A.js_out = out->js; A.jr_out = out->jr;
    A.err = reinterpret_cast<long long*>(err);
    A.P = P;
    A.Rp = extra->Rp; A.beta = extra->beta; A.VqT = extra->VqT; A.vq2 = extra->vq2; A.lq = extra->lq;
    A.us_out = out->user_sentences; A.usf_out = out->user_sentences_fixed; A.ur_out = out->user_reviews; A.ut_out = out->user_text;
    A.ism_out = out->item_sentence_match; A.irm_out = out->item_review_match; A.ir_out = out->item_reviews; A.it_out = out->item_text;
    const unsigned grid = (unsigned)((P + kAhnTile - 1) / kAhnTile);
    hipLaunchKernelGGL(ahn_explain_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("ahn_pair_explain_ids launch");
    return 0;
}
