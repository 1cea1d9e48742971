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
// Steps 2-5 are a few hundred kFLOP: wave reductions (rbr_wave.h) in a fixed order, p and z in the LDS the slices used.  Step 5
// is ahn_pair.h's ahn_fm, shared with the explanation of ahn_explain.hip.
//
// Rules kept: every loop in front of a barrier or shuffle has a workgroup- (wave-) uniform trip count; no atomics but the id
// error record; every sum has one fixed order that depends on the shape alone, so a pair has the same bits in both entries,
// in every tile position and on every run.
#include "ahn_pair.h"

namespace rbr {

// One pair: user state row u, item state row i, output slot q.  Every thread of the workgroup makes the call.
__device__ __forceinline__ void ahn_pair_body(const AhnPair& A, long long u, long long i, long long q, float* __restrict__ smem,
                                              float* __restrict__ s_s, float* __restrict__ w_s, float* __restrict__ t_s,
                                              float* __restrict__ v_s, float* __restrict__ red_s) {
    ahn_tail<false>(A, u, i, q, smem, s_s, w_s, t_s, v_s);            // ---- 1-4: z [F] behind p [Ru, F], behind a barrier
    ahn_fm<false>(A, u, i, q, smem + A.Ru * A.F, red_s, nullptr);     // ---- 5. the FM (ahn_pair.h)
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
