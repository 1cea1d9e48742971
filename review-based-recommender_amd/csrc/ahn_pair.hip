// ahn_pair.hip -- AHN's pair-dependent tail from cached per-id sentence tables, one launch per score block.
//
// AHN's co-attention is asymmetric (models/ahn/ahn_layers.py: UnbalancedCoAttentionAggregator / ...Review): the item side is pooled
// by GatedAttention alone, and only the user side looks at the pair.  With F = hidden_dim, a user of Ru reviews x Su sentences and
// an item of Ri x Si, the per-id state is
//   user u: X  [Ru*Su, F]  the encoder's sentence vectors           item i: Ks [Ri*Si, F] = (a * Y) @ Ws^T   (a: all-sentence weights)
//           X' [Ru*Su, F]  = X @ Wt^T (no bias)                             Kr [Ri, F]    = r' @ Wr^T
//           sentence masks [Ru*Su], review masks [Ru] (bytes)               fm [K + 2]
//           fm [K + 2]: the id's part of the FM (below)
// and a pair (u, i) is
//   1. s[n]    = max_j X[n] . Ks[j]                     over ALL Ri*Si rows of the item (the reference masks nothing there)
//   2. w[r, :] = softmax_s(m[r, s] ? s[r, s] : -1e8)
//   3. p[r]    = relu(sum_s w[r, s] X'[r, s] + bt)
//   4. t[r]    = max_j p[r] . Kr[j];  v = softmax_r(M[r] ? t[r] : -1e8);  z = sum_r v[r] p[r]
//   5. score   = 0.5 * (sum_k (z Vz + fm_u + fm_i)_k^2 - z^2 . vz2 - fm_u[K] - fm_i[K]) + z . lz + fm_u[K+1] + fm_i[K+1] + lin_b
//      -- the FM over x = [z, e_u, q, e_i] with the three per-id blocks of x V, x^2 V^2 and x . lin_w hoisted into fm_u / fm_i.
//
// Work split.  A workgroup of 4 waves owns kAhnTile consecutive pairs of the launch and walks them one after the other; in the
// dense entry these are one user against kAhnTile neighbouring items and blockIdx runs over the items first, so the workgroups
// that are resident together read the same user's X (L2 hits after the first).  Step 1 is a [Ri*Si, F] x [F, Ru*Su] product on
// v_mfma_f32_32x32x2_f32 (exact f32 fma chains): F is streamed in slices of kAhnKS columns through LDS (both operands, rows
// beyond the operand and columns beyond F zero-filled), wave w keeps the up to four 32 x 32 accumulators of user rows
// [32 w, 32 w + 32) in registers, and the score matrix is never stored: the item's sentences are the MFMA's A rows, so a lane
// holds 16 item sentences of ONE user sentence per tile and the row max is 16 in-lane maxima and one exchange between the wave's
// halves.  Steps 2-5 are a few hundred kFLOP: wave reductions (rbr_wave.h) in a fixed order, p and z in the LDS the slices used.
//
// Rules kept: every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; no atomics but the id
// error record; every sum has one fixed order that depends on the shape alone, so a pair has the same bits in both entries,
// in every tile position and on every run.
#include "rbr_common.h"

#include <cmath>
#include <cstdint>

namespace rbr {

constexpr int kAhnRows = 128;                      // cap on Ru*Su and on Ri*Si: four 32-row MFMA tiles each
constexpr int kAhnKS = 32;                         // columns of F per LDS slice
constexpr int kAhnLd = kAhnKS + 4;                 // LDS row pitch in floats (16-byte aligned rows, 4 * odd)
constexpr int kAhnTile = 4;                        // pairs per workgroup
constexpr int kAhnLds = 2 * kAhnRows * kAhnLd;     // floats: the two operand slices, later p [Ru, F] and z [F]
constexpr int kAhnSuMax = 64, kAhnRuMax = 64;      // one wave holds a review's sentences / a user's reviews in its lanes
constexpr int kAhnFMax = 2048, kAhnKMax = 64;
constexpr float kAhnMaskFill = -1e8f;              // the reference's fill of masked scores (utils.py:13)

typedef float ahn_f32x16 __attribute__((ext_vector_type(16)));

struct AhnPair {
    const float *X, *Xt, *ufm;                     // user state
    const unsigned char *usm, *urm;
    const float *Ks, *Kr, *ifm;                    // item state
    const float *bt, *VzT, *vz2, *lz, *lin_b;      // head
    const void *u_rows, *i_rows;                   // ids entry: P row indices each; dense entry: u_rows [Nu] or null
    float *out, *w_out, *v_out;
    long long* err;
    long long P;                                   // ids entry: pairs
    int U, I;                                      // rows of the user / item state tables
    int Nu;                                        // dense entry: user rows of the block
    int Ru, Su, NU, NJ, Ri, F, K;                  // NU = Ru * Su, NJ = Ri * Si
    int idx64, dense, ntiles, vec;
};

__device__ __forceinline__ long long ahn_row(const void* rows, long long q, int idx64) {
    return idx64 ? static_cast<const long long*>(rows)[q] : (long long)static_cast<const int*>(rows)[q];
}

// a row index outside its table is never dereferenced: row 0 stands in and err is updated as rbr::sanitize_id does
__device__ __forceinline__ long long ahn_checked(long long v, int rows, int set, long long* __restrict__ err) {
    if ((unsigned long long)v >= (unsigned long long)rows) {
        if (err && threadIdx.x == 0) {
            err[1] = v; err[2] = set;                 // any one offender (benign race)
            atomicAdd(reinterpret_cast<unsigned long long*>(err), 1ull);
        }
        v = 0;
    }
    return v;
}

// One pair: user state row u, item state row i, output slot q.  Every thread of the workgroup makes the call.
__device__ __forceinline__ void ahn_pair_body(const AhnPair& A, long long u, long long i, long long q, float* __restrict__ smem,
                                              float* __restrict__ s_s, float* __restrict__ w_s, float* __restrict__ t_s,
                                              float* __restrict__ v_s, float* __restrict__ red_s) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int F = A.F, NU = A.NU, NJ = A.NJ, Ru = A.Ru, Su = A.Su, Ri = A.Ri, K = A.K;
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
    {   // register r of tile ct is item sentence ct * 32 + (r & 3) + 8 (r >> 2) + 4 half of user sentence wave * 32 + col
        float mx = -INFINITY;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (j < NJ) mx = fmaxf(mx, acc[ct][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const int n = wave * 32 + col;
        if (half == 0 && n < NU) s_s[n] = mx;
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
        for (int j = 0; j < Ri; ++j) {
            float d = 0.f;
            for (int f = lane; f < F; f += 64) d = fmaf(p_s[r * F + f], Kri[(size_t)j * F + f], d);
            t = fmaxf(t, wave_sum(d));
        }
        if (lane == 0) t_s[r] = t;
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

    // ---- 5. the FM: a wave per factor, then one thread adds the K squares in factor order
    const float* __restrict__ fu = A.ufm + (size_t)u * (K + 2);
    const float* __restrict__ fi = A.ifm + (size_t)i * (K + 2);
    for (int k = wave; k < K; k += 4) {
        float d = 0.f;
        for (int f = lane; f < F; f += 64) d = fmaf(z_s[f], A.VzT[(size_t)k * F + f], d);
        const float xv = (wave_sum(d) + fu[k]) + fi[k];
        if (lane == 0) red_s[k] = xv * xv;
    }
    if (wave == 0) {
        float a = 0.f, b = 0.f;
        for (int f = lane; f < F; f += 64) {
            const float zf = z_s[f];
            a = fmaf(zf * zf, A.vz2[f], a);
            b = fmaf(zf, A.lz[f], b);
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) { red_s[kAhnKMax] = a; red_s[kAhnKMax + 1] = b; }
    }
    __syncthreads();
    if (tid == 0) {
        float sq = 0.f;
        for (int k = 0; k < K; ++k) sq += red_s[k];
        A.out[q] = 0.5f * (((sq - red_s[kAhnKMax]) - fu[K]) - fi[K]) + (((red_s[kAhnKMax + 1] + fu[K + 1]) + fi[K + 1]) + A.lin_b[0]);
    }
}

__global__ __launch_bounds__(256) void ahn_pair_kernel(const AhnPair A) {
    __shared__ __attribute__((aligned(16))) float smem[kAhnLds];
    __shared__ float s_s[kAhnRows], w_s[kAhnRows], t_s[kAhnRuMax], v_s[kAhnRuMax], red_s[kAhnKMax + 2];
    // the trip count depends on the block alone: whole workgroups reach the barriers of ahn_pair_body
    for (int t = 0; t < kAhnTile; ++t) {
        long long u, i, q;
        if (A.dense) {
            const long long row = blockIdx.x / A.ntiles;
            i = (long long)(blockIdx.x % A.ntiles) * kAhnTile + t;
            if (i >= A.I) break;
            q = row * A.I + i;
            u = A.u_rows ? ahn_checked(ahn_row(A.u_rows, row, A.idx64), A.U, 0, i == 0 ? A.err : nullptr) : row;
        } else {
            q = (long long)blockIdx.x * kAhnTile + t;
            if (q >= A.P) break;
            u = ahn_checked(ahn_row(A.u_rows, q, A.idx64), A.U, 0, A.err);
            i = ahn_checked(ahn_row(A.i_rows, q, A.idx64), A.I, 1, A.err);
        }
        ahn_pair_body(A, u, i, q, smem, s_s, w_s, t_s, v_s, red_s);
    }
}

static int ahn_args_ok(const char* what, const rbr_ahn_shape* s, const rbr_ahn_user_state* us, const rbr_ahn_item_state* is,
                       const rbr_ahn_head* h) {
    if (!s || !us || !is || !h) { set_error("%s: null argument struct", what); return RBR_ERR_BAD_ARG; }
    if (s->Ru <= 0 || s->Su <= 0 || s->Ri <= 0 || s->Si <= 0 || s->F <= 0 || s->K <= 0) {
        set_error("%s: bad shape Ru=%d Su=%d Ri=%d Si=%d F=%d K=%d", what, s->Ru, s->Su, s->Ri, s->Si, s->F, s->K);
        return RBR_ERR_BAD_ARG;
    }
    if (s->Ru > kAhnRuMax || s->Su > kAhnSuMax || (long long)s->Ru * s->Su > kAhnRows || (long long)s->Ri * s->Si > kAhnRows ||
        s->F > kAhnFMax || s->K > kAhnKMax || ((long long)s->Ru + 1) * s->F > kAhnLds) {
        set_error("%s: shape Ru=%d Su=%d Ri=%d Si=%d F=%d K=%d is outside the caps Ru <= %d, Su <= %d, Ru*Su <= %d, Ri*Si <= %d, "
                  "F <= %d, (Ru + 1) * F <= %d, K <= %d", what, s->Ru, s->Su, s->Ri, s->Si, s->F, s->K, kAhnRuMax, kAhnSuMax,
                  kAhnRows, kAhnRows, kAhnFMax, kAhnLds, kAhnKMax);
        return RBR_ERR_BAD_ARG;
    }
    if (us->rows <= 0 || is->rows <= 0) { set_error("%s: bad table rows U=%d I=%d", what, us->rows, is->rows); return RBR_ERR_BAD_ARG; }
    if (!us->X || !us->Xt || !us->sent_mask || !us->rev_mask || !us->fm || !is->Ks || !is->Kr || !is->fm || !h->bt || !h->VzT ||
        !h->vz2 || !h->lz || !h->lin_b) {
        set_error("%s: null pointer", what);
        return RBR_ERR_BAD_ARG;
    }
    return 0;
}

static void ahn_fill(AhnPair& A, const rbr_ahn_shape* s, const rbr_ahn_user_state* us, const rbr_ahn_item_state* is,
                     const rbr_ahn_head* h) {
    A.X = us->X; A.Xt = us->Xt; A.ufm = us->fm; A.usm = us->sent_mask; A.urm = us->rev_mask;
    A.Ks = is->Ks; A.Kr = is->Kr; A.ifm = is->fm;
    A.bt = h->bt; A.VzT = h->VzT; A.vz2 = h->vz2; A.lz = h->lz; A.lin_b = h->lin_b;
    A.U = us->rows; A.I = is->rows;
    A.Ru = s->Ru; A.Su = s->Su; A.NU = s->Ru * s->Su; A.NJ = s->Ri * s->Si; A.Ri = s->Ri; A.F = s->F; A.K = s->K;
    const auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
    A.vec = (s->F % 4 == 0 && aligned(us->X) && aligned(is->Ks)) ? 1 : 0;
    A.u_rows = A.i_rows = nullptr;
    A.out = A.w_out = A.v_out = nullptr;
    A.err = nullptr;
    A.P = 0; A.Nu = 0; A.idx64 = 1; A.dense = 0; A.ntiles = 1;
}

}  // namespace rbr

extern "C" int rbr_ahn_pair_score_ids(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                                      const rbr_ahn_head* head, int64_t P, const void* u_rows, const void* i_rows,
                                      int32_t index_bits, float* out, float* w_out, float* v_out, int64_t* err, void* stream) {
    using namespace rbr;
    const char* what = "rbr_ahn_pair_score_ids";
    if (int e = ahn_args_ok(what, shape, user, item, head)) return e;
    if (P <= 0 || P > (int64_t)0x7fffffff) { set_error("%s: P=%lld must be in 1 .. 2^31 - 1", what, (long long)P); return RBR_ERR_BAD_ARG; }
    if (index_bits != 32 && index_bits != 64) { set_error("%s: index_bits=%d must be 32 or 64", what, index_bits); return RBR_ERR_BAD_ARG; }
    if (!u_rows || !i_rows || !out) { set_error("%s: null pointer", what); return RBR_ERR_BAD_ARG; }
    AhnPair A;
    ahn_fill(A, shape, user, item, head);
    A.u_rows = u_rows; A.i_rows = i_rows; A.idx64 = index_bits == 64;
    A.out = out; A.w_out = w_out; A.v_out = v_out;
    A.err = reinterpret_cast<long long*>(err);
    A.P = P;
    const unsigned grid = (unsigned)((P + kAhnTile - 1) / kAhnTile);
    hipLaunchKernelGGL(ahn_pair_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("ahn_pair_score_ids launch");
    return 0;
}

extern "C" int rbr_ahn_pair_score_dense(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                                        const rbr_ahn_head* head, int32_t Nu, const void* u_rows, int32_t index_bits, float* out,
                                        int64_t* err, void* stream) {
    using namespace rbr;
    const char* what = "rbr_ahn_pair_score_dense";
    if (int e = ahn_args_ok(what, shape, user, item, head)) return e;
    if (Nu <= 0) { set_error("%s: Nu=%d must be at least 1", what, Nu); return RBR_ERR_BAD_ARG; }
    if (index_bits != 32 && index_bits != 64) { set_error("%s: index_bits=%d must be 32 or 64", what, index_bits); return RBR_ERR_BAD_ARG; }
    if (!u_rows && Nu > user->rows) {
        set_error("%s: Nu=%d rows asked of a user table of %d and no u_rows given", what, Nu, user->rows);
        return RBR_ERR_BAD_ARG;
    }
    if (!out) { set_error("%s: null output", what); return RBR_ERR_BAD_ARG; }
    const long long ntiles = ((long long)item->rows + kAhnTile - 1) / kAhnTile;
    if (ntiles * Nu > 0x7fffffffLL) {
        set_error("%s: Nu=%d x I=%d overflows the grid (Nu * ceil(I / %d) must stay below 2^31)", what, Nu, item->rows, kAhnTile);
        return RBR_ERR_BAD_ARG;
    }
    AhnPair A;
    ahn_fill(A, shape, user, item, head);
    A.u_rows = u_rows; A.idx64 = index_bits == 64;
    A.out = out;
    A.err = reinterpret_cast<long long*>(err);
    A.Nu = Nu; A.dense = 1; A.ntiles = (int)ntiles;
    hipLaunchKernelGGL(ahn_pair_kernel, dim3((unsigned)(ntiles * Nu)), dim3(256), 0, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("ahn_pair_score_dense launch");
    return 0;
}
