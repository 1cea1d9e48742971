// ahn_pair.h -- what the kernels over AHN's cached sentence tables share beyond ahn_tail.h's steps 1-4: the argument block, the
// checked row index, the argument validation of the entries, and step 5 of the pair tail, the FM, stated once for the two
// kernels that run it: ahn_pair_kernel (ahn_pair.hip: a score) and ahn_explain_kernel (ahn_explain.hip: a score and what every
// sentence and review adds to it).
//   5. score   = 0.5 * (sum_k (z Vz + fm_u + fm_i)_k^2 - z^2 . vz2 - fm_u[K] - fm_i[K]) + z . lz + fm_u[K+1] + fm_i[K+1] + lin_b
//      -- the FM over x = [z, e_u, q, e_i] with the three per-id blocks of x V, x^2 V^2 and x . lin_w hoisted into fm_u / fm_i.
// kSave: the explanation also wants xv[k] = (z . VzT[k] + fm_u[k]) + fm_i[k] itself (the FM's gradient is a closed form of it).
// The score is computed by the same instructions either way, so a pair has the same bits in both kernels.
#pragma once

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

// Step 5 of one pair, behind ahn_tail: z [F] stands in LDS behind a barrier.  Every thread of the workgroup (256) makes the call;
// red_s holds kAhnKMax + 2 floats, xv_s (kSave) kAhnKMax.  A wave per factor, then one thread adds the K squares in factor order.
// On return out[q] is written by thread 0 and xv_s [K] (kSave) stands behind the barrier inside.
template <bool kSave>
__device__ __forceinline__ void ahn_fm(const AhnPair& A, long long u, long long i, long long q, const float* __restrict__ z_s,
                                       float* __restrict__ red_s, float* __restrict__ xv_s) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int F = A.F, K = A.K;
    const float* __restrict__ fu = A.ufm + (size_t)u * (K + 2);
    const float* __restrict__ fi = A.ifm + (size_t)i * (K + 2);
    for (int k = wave; k < K; k += 4) {
        float d = 0.f;
        for (int f = lane; f < F; f += 64) d = fmaf(z_s[f], A.VzT[(size_t)k * F + f], d);
        const float xv = (wave_sum(d) + fu[k]) + fi[k];
        if (lane == 0) {
            red_s[k] = xv * xv;
            if (kSave) xv_s[k] = xv;
        }
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

// host: the caps and the pointers every entry over the tables checks before a launch
static inline int ahn_args_ok(const char* what, const rbr_ahn_shape* s, const rbr_ahn_user_state* us, const rbr_ahn_item_state* is,
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

static inline void ahn_fill(AhnPair& A, const rbr_ahn_shape* s, const rbr_ahn_user_state* us, const rbr_ahn_item_state* is,
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
