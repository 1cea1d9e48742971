// neg_sample.hip -- negatives for a pairwise (BPR) objective on top of the id feed: for every observed pair (u, i+) of a batch,
// n_neg items of [item_lo, I) the user has not rated, drawn on the device and rejected against the seen-items CSR that the ranking
// evaluation already uses (recommend.Recommender.seen_from, the exclusion form of rbr_pair_score_topk).  One launch, one lane per
// draw, no host synchronisation: it sits in front of the id feed's gather inside a recorded step and draws a new set on every
// replay (the call number lives in device memory, as in rbr_dropout_multiplier).  The reference has no ranking objective at all.
//
// The draw is fixed by include/rbr_hip.h (rbr_sample_negatives) so that a host restatement gives the same integers:
//   draw d = b * n_neg + j, attempt t: word (t & 3) of philox4x32_10(quad = d * 16 + (t >> 2), call = state[0], seed),
//   candidate = item_lo + ((uint64)word * (I - item_lo) >> 32); after max_tries rejections a cyclic walk from the last candidate.
//
// rbr_sample_hard_negatives (dynamic negative sampling): n_cand such draws per negative, draw index d * n_cand + m, each scored
// from cached latent rows by the arithmetic of pair_score.hip (pair_score_math.h); the candidate with the largest key -- score
// descending, then item ascending -- is the negative.  One lane per candidate, a draw is a group of W = 2^ceil(log2 n_cand)
// consecutive lanes, the group's maximum an xor butterfly on the two halves of the key; only the winner is encoded afterwards.
#include "rbr_common.h"
#include "item_csr.h"
#include "pair_score_math.h"

namespace rbr {

struct NegSample {
    const long long* u_ids;
    const long long* i_ids;
    ItemCsr seen;                  // row u: the items user u has seen (item_csr.h)
    long long* u_out;              // [(1 + n_neg) * B]
    long long* i_out;
    float* valid;                  // [n_neg * B]
    unsigned long long seed;
    long long replace;
    int B, n_neg, I, item_lo, max_tries;
};

// a negative may be any item but the pair's own and those of the user's seen row [a, e)
__device__ __forceinline__ bool neg_acceptable(const int* __restrict__ seen_item, long long c, long long pos, long long a, long long e) {
    return c != pos && !csr_has(seen_item, a, e, c);
}

// THE DRAW of include/rbr_hip.h for draw index d under call number `call`: the item, and whether it is acceptable at all
__device__ __forceinline__ bool draw_negative(const NegSample& S, unsigned long long d, unsigned long long call, long long u, long long pos,
                                              long long& c) {
    long long a, e;
    csr_row(S.seen, u, a, e);
    const unsigned long long range = (unsigned long long)(S.I - S.item_lo);
    c = S.item_lo;
    bool found = false;
    unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    for (int t = 0; t < S.max_tries && !found; ++t) {
        if ((t & 3) == 0) philox4x32_10(d * 16ull + (unsigned long long)(t >> 2), call, S.seed, w0, w1, w2, w3);
        const unsigned word = (t & 3) == 0 ? w0 : (t & 3) == 1 ? w1 : (t & 3) == 2 ? w2 : w3;
        c = (long long)S.item_lo + (long long)(((unsigned long long)word * range) >> 32);
        found = neg_acceptable(S.seen.item, c, pos, a, e);
    }
    // crowded row: walk on from the last candidate, cyclically, to the first acceptable item (`range` steps visit every item)
    for (unsigned long long s = 0; s < range && !found; ++s) {
        c = (long long)S.item_lo + (long long)(((unsigned long long)(c - S.item_lo) + 1ull) % range);
        found = neg_acceptable(S.seen.item, c, pos, a, e);
    }
    return found;
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(const NegSample S, unsigned long long* __restrict__ state) {
    const unsigned long long call = state[0];       // every lane, before anything else: the last workgroup advances it
    const long long n = (long long)S.B * S.n_neg;
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d < n) {
        const int b = (int)(d / S.n_neg), j = (int)(d - (long long)b * S.n_neg);
        const long long u = S.u_ids[b], pos = S.i_ids[b];
        long long c;
        const bool found = draw_negative(S, (unsigned long long)d, call, u, pos, c);
        const long long r = (long long)(j + 1) * S.B + b;
        S.u_out[r] = u;
        S.i_out[r] = found ? c : S.replace;
        S.valid[(long long)j * S.B + b] = found ? 1.f : 0.f;
        if (j == 0) {       // slab 0: the observed pairs themselves
            S.u_out[b] = u;
            S.i_out[b] = pos;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) rng_advance_call(state, call);
}

struct HardNeg {
    NegSample S;
    const float* ul; const float* il;     // [U, K] / [I, K]
    const float* h; const float* g;       // [K], [1] (FM)
    const float* ub; const float* ib;     // [U], [I] or null (FM)
    long long* cand_out;           // [n_neg * B * n_cand] or null
    float* cand_score;             // [n_neg * B * n_cand] or null
    int U;                         // rows of ul / ub AND of the seen CSR
    int K, n_cand, log_w;          // a draw is 1 << log_w consecutive lanes, the first n_cand of them live
};

template <int MODE>
__global__ __launch_bounds__(256) void sample_hard_negatives_kernel(const HardNeg A, unsigned long long* __restrict__ state) {
    const unsigned long long call = state[0];       // every lane, before anything else: the last workgroup advances it
    const NegSample& S = A.S;
    const long long n = (long long)S.B * S.n_neg;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long d = t >> A.log_w;
    const int m = (int)(t & ((1 << A.log_w) - 1));
    const bool first = d < n && m == 0;
    unsigned long long key = 0ull;                  // lanes past n_cand or past the last draw never win
    int b = 0, j = 0;
    long long u = 0, c = 0;
    bool found = false;
    if (d < n && m < A.n_cand) {
        b = (int)(d / S.n_neg); j = (int)(d - (long long)b * S.n_neg);
        u = S.u_ids[b];
        found = draw_negative(S, (unsigned long long)d * (unsigned long long)A.n_cand + (unsigned long long)m, call, u, S.i_ids[b], c);
        if (!found) c = S.replace;                  // nothing is acceptable for (u, i+): so says every candidate of the draw
        const size_t ur = (unsigned long long)u < (unsigned long long)A.U ? (size_t)u : 0;      // an id outside the table: row 0
        const float ub = (MODE == RBR_SCORE_FM && A.ub) ? A.ub[ur] : 0.f, ib = (MODE == RBR_SCORE_FM && A.ib) ? A.ib[c] : 0.f;
        const float s = score_pair<MODE>(A.ul + ur * A.K, A.il + (size_t)c * A.K, A.h, A.K, ub, ib, MODE == RBR_SCORE_FM ? A.g[0] : 0.f);
        key = s != s ? 0ull : make_key(s, (int)c);
        const long long q = ((long long)j * S.B + b) * A.n_cand + m;
        if (A.cand_out) A.cand_out[q] = c;
        if (A.cand_score) A.cand_score[q] = s;
    }
    // every lane-dependent loop has closed: all 64 lanes of the wave take part in the butterfly over the draw's 1 << log_w lanes
    for (int o = (1 << A.log_w) >> 1; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, o), hi = __shfl_xor((unsigned)(key >> 32), o);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other > key ? other : key;
    }
    if (first) {                                    // candidate 0 stores; it stands in where no candidate has a key (all NaN)
        const long long r = (long long)(j + 1) * S.B + b;
        S.u_out[r] = u;
        S.i_out[r] = (found && key != 0ull) ? (long long)key_item(key) : c;
        S.valid[(long long)j * S.B + b] = found ? 1.f : 0.f;
        if (j == 0) {       // slab 0: the observed pairs themselves
            S.u_out[b] = u;
            S.i_out[b] = S.i_ids[b];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) rng_advance_call(state, call);
}

}  // namespace rbr

extern "C" int rbr_sample_negatives(int32_t B, int32_t n_neg, int32_t I, int32_t item_lo, const int64_t* u_ids, const int64_t* i_ids,
                                    const int64_t* seen_off, const int32_t* seen_item, int64_t seen_nnz, int32_t U, uint64_t seed,
                                    uint64_t* state, int32_t max_tries, int64_t replace_id, int64_t* u_out, int64_t* i_out,
                                    float* valid, void* stream) {
    using namespace rbr;
    if (B <= 0 || n_neg < 1 || I <= 0 || (long long)B * n_neg > (1LL << 30)) {
        set_error("rbr_sample_negatives: bad shape B=%d n_neg=%d I=%d", B, n_neg, I);
        return RBR_ERR_BAD_ARG;
    }
    if (item_lo < 0 || item_lo >= I) { set_error("rbr_sample_negatives: item_lo=%d leaves no item of [0, %d)", item_lo, I); return RBR_ERR_BAD_ARG; }
    if (!u_ids || !i_ids || !state || !u_out || !i_out || !valid) { set_error("rbr_sample_negatives: null pointer"); return RBR_ERR_BAD_ARG; }
    if (int e = item_csr_ok("rbr_sample_negatives", true, seen_off, seen_item, seen_nnz, nullptr, U)) return e;
    if (max_tries < 1 || max_tries > 64) { set_error("rbr_sample_negatives: max_tries=%d outside [1, 64]", max_tries); return RBR_ERR_BAD_ARG; }
    if (replace_id < 0 || replace_id >= I) {
        set_error("rbr_sample_negatives: replace_id %lld is not an item of [0, %d)", (long long)replace_id, I);
        return RBR_ERR_BAD_ARG;
    }
    NegSample S;
    S.u_ids = reinterpret_cast<const long long*>(u_ids); S.i_ids = reinterpret_cast<const long long*>(i_ids);
    S.seen = item_csr(seen_off, seen_item, nullptr, seen_nnz, U);
    S.u_out = reinterpret_cast<long long*>(u_out); S.i_out = reinterpret_cast<long long*>(i_out); S.valid = valid;
    S.seed = seed; S.replace = replace_id;
    S.B = B; S.n_neg = n_neg; S.I = I; S.item_lo = item_lo; S.max_tries = max_tries;
    const unsigned grid = (unsigned)(((long long)B * n_neg + 255) / 256);
    hipLaunchKernelGGL(sample_negatives_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, S,
                       reinterpret_cast<unsigned long long*>(state));
    RBR_CHECK_LAUNCH("sample_negatives launch");
    return 0;
}

extern "C" int rbr_sample_hard_negatives(int32_t B, int32_t n_neg, int32_t n_cand, int32_t I, int32_t item_lo, const int64_t* u_ids,
                                         const int64_t* i_ids, const int64_t* seen_off, const int32_t* seen_item, int64_t seen_nnz,
                                         int32_t U, int32_t mode, int32_t K, const float* ul, const float* il, const float* h,
                                         const float* g, const float* ub, const float* ib, uint64_t seed, uint64_t* state,
                                         int32_t max_tries, int64_t replace_id, int64_t* u_out, int64_t* i_out, float* valid,
                                         int64_t* cand_out, float* cand_score, void* stream) {
    using namespace rbr;
    if (n_cand < 1 || n_cand > 64) { set_error("rbr_sample_hard_negatives: n_cand=%d outside [1, 64]", n_cand); return RBR_ERR_BAD_ARG; }
    if (B <= 0 || n_neg < 1 || I <= 0 || U <= 0 || (long long)B * n_neg * n_cand > (1LL << 30)) {
        set_error("rbr_sample_hard_negatives: bad shape B=%d n_neg=%d n_cand=%d U=%d I=%d", B, n_neg, n_cand, U, I);
        return RBR_ERR_BAD_ARG;
    }
    if (mode != RBR_SCORE_FM && mode != RBR_SCORE_DOT) {
        set_error("rbr_sample_hard_negatives: mode %d is neither RBR_SCORE_FM nor RBR_SCORE_DOT", mode);
        return RBR_ERR_BAD_ARG;
    }
    if (K < 1) { set_error("rbr_sample_hard_negatives: bad latent dimension K=%d", K); return RBR_ERR_BAD_ARG; }
    if (item_lo < 0 || item_lo >= I) { set_error("rbr_sample_hard_negatives: item_lo=%d leaves no item of [0, %d)", item_lo, I); return RBR_ERR_BAD_ARG; }
    if (!u_ids || !i_ids || !state || !u_out || !i_out || !valid) { set_error("rbr_sample_hard_negatives: null pointer"); return RBR_ERR_BAD_ARG; }
    if (!ul || !il) { set_error("rbr_sample_hard_negatives: null latent table"); return RBR_ERR_BAD_ARG; }
    if (mode == RBR_SCORE_FM && (!h || !g)) { set_error("rbr_sample_hard_negatives: RBR_SCORE_FM needs h and g"); return RBR_ERR_BAD_ARG; }
    if (int e = item_csr_ok("rbr_sample_hard_negatives", true, seen_off, seen_item, seen_nnz, nullptr, U)) return e;
    if (max_tries < 1 || max_tries > 64) { set_error("rbr_sample_hard_negatives: max_tries=%d outside [1, 64]", max_tries); return RBR_ERR_BAD_ARG; }
    if (replace_id < 0 || replace_id >= I) {
        set_error("rbr_sample_hard_negatives: replace_id %lld is not an item of [0, %d)", (long long)replace_id, I);
        return RBR_ERR_BAD_ARG;
    }
    HardNeg A;
    NegSample& S = A.S;
    S.u_ids = reinterpret_cast<const long long*>(u_ids); S.i_ids = reinterpret_cast<const long long*>(i_ids);
    S.seen = item_csr(seen_off, seen_item, nullptr, seen_nnz, U);
    S.u_out = reinterpret_cast<long long*>(u_out); S.i_out = reinterpret_cast<long long*>(i_out); S.valid = valid;
    S.seed = seed; S.replace = replace_id;
    S.B = B; S.n_neg = n_neg; S.I = I; S.item_lo = item_lo; S.max_tries = max_tries;
    A.ul = ul; A.il = il; A.h = h; A.g = g; A.ub = ub; A.ib = ib;
    A.cand_out = reinterpret_cast<long long*>(cand_out); A.cand_score = cand_score;
    A.U = U; A.K = K; A.n_cand = n_cand;
    A.log_w = 0;
    while ((1 << A.log_w) < n_cand) ++A.log_w;
    const unsigned grid = (unsigned)(((((long long)B * n_neg) << A.log_w) + 255) / 256);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
    if (mode == RBR_SCORE_FM)
        hipLaunchKernelGGL(sample_hard_negatives_kernel<RBR_SCORE_FM>, dim3(grid), dim3(256), 0, (hipStream_t)stream, A, st);
    else
        hipLaunchKernelGGL(sample_hard_negatives_kernel<RBR_SCORE_DOT>, dim3(grid), dim3(256), 0, (hipStream_t)stream, A, st);
    RBR_CHECK_LAUNCH("sample_hard_negatives launch");
    return 0;
}
