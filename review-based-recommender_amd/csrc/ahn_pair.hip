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
// that are resident together read the same user's X (L2 hits after the first).  Steps 1-4 are ahn_tail.h's (shared with the
// training op of ahn_attend.hip): step 1 on v_mfma_f32_32x32x2_f32 with F streamed through LDS, the score matrix never stored.
// Steps 2-5 are a few hundred kFLOP: wave reductions (rbr_wave.h) in a fixed order, p and z in the LDS the slices used.
//
// Rules kept: every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; no atomics but the id
// error record; every sum has one fixed order that depends on the shape alone, so a pair has the same bits in both entries,
// in every tile position and on every run.
#include "ahn_tail.h"

namespace rbr {

constexpr int kAhnKMax = 64;

struct AhnPair : AhnTail {
    const float *ufm, *ifm;                        // the ids' parts of the FM
    const float *VzT, *vz2, *lz, *lin_b;           // head
    const void *u_rows, *i_rows;                   // ids entry: P row indices each; dense entry: u_rows [Nu] or null
    float* out;
    long long* err;
    long long P;                                   // ids entry: pairs
    int U, I;                                      // rows of the user / item state tables
    int Nu;                                        // dense entry: user rows of the block
    int K;
    int idx64, dense, ntiles;
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
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int F = A.F, K = A.K;
    ahn_tail<false>(A, u, i, q, smem, s_s, w_s, t_s, v_s);            // ---- 1-4: z [F] behind p [Ru, F], behind a barrier
    const float* z_s = smem + A.Ru * F;

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
    A.js_out = A.jr_out = nullptr;
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
