// neg_sample.hip -- negatives for a pairwise (BPR) objective on top of the id feed: for every observed pair (u, i+) of a batch,
// n_neg items of [item_lo, I) the user has not rated, drawn on the device and rejected against the seen-items CSR that the ranking
// evaluation already uses (recommend.Recommender.seen_from, the exclusion form of rbr_pair_score_topk).  One launch, one lane per
// draw, no host synchronisation: it sits in front of the id feed's gather inside a recorded step and draws a new set on every
// replay (the call number lives in device memory, as in rbr_dropout_multiplier).  The reference has no ranking objective at all.
//
// The draw is fixed by include/rbr_hip.h (rbr_sample_negatives) so that a host restatement gives the same integers:
//   draw d = b * n_neg + j, attempt t: word (t & 3) of philox4x32_10(quad = d * 16 + (t >> 2), call = state[0], seed),
//   candidate = item_lo + ((uint64)word * (I - item_lo) >> 32); after max_tries rejections a cyclic walk from the last candidate.
#include "rbr_common.h"

namespace rbr {

struct NegSample {
    const long long* u_ids;
    const long long* i_ids;
    const long long* seen_off;     // [U + 1] or null
    const int* seen_item;          // sorted within a user
    long long seen_nnz;
    long long* u_out;              // [(1 + n_neg) * B]
    long long* i_out;
    float* valid;                  // [n_neg * B]
    unsigned long long seed;
    long long replace;
    int B, n_neg, I, item_lo, U, max_tries;
};

// [a, e) of seen_item that serves user u; an id outside [0, U) has no row, and a malformed CSR cannot send a reader outside
// seen_item (offsets clamped to [0, seen_nnz], as rbr_pair_score_topk clamps them)
__device__ __forceinline__ void seen_bounds(const NegSample& S, long long u, long long& a, long long& e) {
    a = e = 0;
    if (S.seen_off == nullptr || (unsigned long long)u >= (unsigned long long)S.U) return;
    a = S.seen_off[u]; e = S.seen_off[u + 1];
    a = a < 0 ? 0 : a;
    e = e > S.seen_nnz ? S.seen_nnz : e;
    if (e < a) e = a;
}

// a negative may be any item but the pair's own and those of the user's seen row [a, e)
__device__ __forceinline__ bool neg_acceptable(const int* __restrict__ seen_item, long long c, long long pos, long long a, long long e) {
    if (c == pos) return false;
    long long lo = a, hi = e;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)seen_item[mid] < c) lo = mid + 1; else hi = mid;
    }
    return !(lo < e && (long long)seen_item[lo] == c);
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(const NegSample S, unsigned long long* __restrict__ state) {
    const unsigned long long call = state[0];       // every lane, before anything else: the last workgroup advances it
    const long long n = (long long)S.B * S.n_neg;
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d < n) {
        const int b = (int)(d / S.n_neg), j = (int)(d - (long long)b * S.n_neg);
        const long long u = S.u_ids[b], pos = S.i_ids[b];
        long long a, e;
        seen_bounds(S, u, a, e);
        const unsigned long long range = (unsigned long long)(S.I - S.item_lo);
        long long c = S.item_lo;
        bool found = false;
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        for (int t = 0; t < S.max_tries && !found; ++t) {
            if ((t & 3) == 0) philox4x32_10((unsigned long long)d * 16ull + (unsigned long long)(t >> 2), call, S.seed, w0, w1, w2, w3);
            const unsigned word = (t & 3) == 0 ? w0 : (t & 3) == 1 ? w1 : (t & 3) == 2 ? w2 : w3;
            c = (long long)S.item_lo + (long long)(((unsigned long long)word * range) >> 32);
            found = neg_acceptable(S.seen_item, c, pos, a, e);
        }
        // crowded row: walk on from the last candidate, cyclically, to the first acceptable item (`range` steps visit every item)
        for (unsigned long long s = 0; s < range && !found; ++s) {
            c = (long long)S.item_lo + (long long)(((unsigned long long)(c - S.item_lo) + 1ull) % range);
            found = neg_acceptable(S.seen_item, c, pos, a, e);
        }
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
    if (threadIdx.x == 0) {       // (no fence needed: the call number was consumed before this atomic is issued)
        if (atomicAdd(state + 1, 1ull) == (unsigned long long)gridDim.x - 1) {      // every workgroup has read state[0]
            state[1] = 0;
            state[0] = call + 1;
        }
    }
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
    if ((seen_off != nullptr) != (seen_item != nullptr) || seen_nnz < 0 || (!seen_off && seen_nnz != 0) || (seen_off && U <= 0)) {
        set_error("rbr_sample_negatives: the seen list is seen_off [U + 1] AND seen_item [seen_nnz] with U >= 1, or neither");
        return RBR_ERR_BAD_ARG;
    }
    if (max_tries < 1 || max_tries > 64) { set_error("rbr_sample_negatives: max_tries=%d outside [1, 64]", max_tries); return RBR_ERR_BAD_ARG; }
    if (replace_id < 0 || replace_id >= I) {
        set_error("rbr_sample_negatives: replace_id %lld is not an item of [0, %d)", (long long)replace_id, I);
        return RBR_ERR_BAD_ARG;
    }
    NegSample S;
    S.u_ids = reinterpret_cast<const long long*>(u_ids); S.i_ids = reinterpret_cast<const long long*>(i_ids);
    S.seen_off = reinterpret_cast<const long long*>(seen_off); S.seen_item = seen_item; S.seen_nnz = seen_nnz;
    S.u_out = reinterpret_cast<long long*>(u_out); S.i_out = reinterpret_cast<long long*>(i_out); S.valid = valid;
    S.seed = seed; S.replace = replace_id;
    S.B = B; S.n_neg = n_neg; S.I = I; S.item_lo = item_lo; S.U = U; S.max_tries = max_tries;
    const unsigned grid = (unsigned)(((long long)B * n_neg + 255) / 256);
    hipLaunchKernelGGL(sample_negatives_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, S,
                       reinterpret_cast<unsigned long long*>(state));
    RBR_CHECK_LAUNCH("sample_negatives launch");
    return 0;
}
