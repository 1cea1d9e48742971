// review_feed.hip -- the id-fed batch of the review split (NARRE, SimpleSiamese).  A review-split example is a function of
// (u_id, i_id) and meta.pkl's per-id review lists: a TRAIN example is the id's list with the target pair's own review removed
// (preprocess/divide_and_create_example_word.py:263-285: index() of the counterpart in the id's rid list, pop(), truncate / pad to
// rv_num), a valid / test example is the list truncated / padded as it is (:306-323).  Removing one slot and keeping R slots reads
// only the first R + 1 entries of a list, so the tables resident on the device hold R + 1 slots per id:
//
//   own id a, counterpart c = the other side's id of the pair
//   d = first j in [0, R) with rids[a][j] == c   (leave_one_out and 0 < c < rows of the other side; else no match: d = R)
//   out slot q <- table slot q + (q >= d)        (reviews and rids alike)
//   word_masks = revs != pad_token (utils.py:30-42);  rev_masks = any token of the review is not pad
// Stacked outputs, user rows first, and the id convention of doc_feed.hip (feed_ids.h).  One launch, nothing synchronises.
#include "rbr_common.h"
#include "feed_ids.h"

namespace rbr {

struct ReviewGather {
    FeedIds F;
    const int* revs[2];          // [N, R + 1, T]
    const int* rids[2];          // [N, R + 1]
    long long* revs_out;         // [2B, R, T]
    unsigned char* wmask;        // [2B, R, T]
    unsigned char* rmask;        // [2B, R] or null
    long long* rids_out;         // [2B, R] or null
    long long pad;
    int R, T, loo;
    int G, units, iters;         // lanes per review (a power of two <= 64), units per review (4-token chunks or tokens), ceil(units / G)
};

// G lanes share one output review (row r, slot q): each of them finds the row's dropped slot d by the same short scan of the
// row's R rids, so they agree on the source slot; the review mask is the group's bits of one ballot.
// VEC (T % 4 == 0, aligned pointers): a 16-byte load of int32 tokens, two 16-byte int64 stores and one 4-byte mask store per
// unit; otherwise one token per unit.
template <bool VEC>
__global__ __launch_bounds__(256) void review_gather_kernel(const ReviewGather P, long long* __restrict__ err) {
    const int lane_g = threadIdx.x & (P.G - 1);
    const int per_block = 256 / P.G;
    const long long n = 2LL * P.F.B * P.R;
    // the trip count depends on the block alone: whole waves reach the ballot
    for (long long v0 = (long long)blockIdx.x * per_block; v0 < n; v0 += (long long)gridDim.x * per_block) {
        const long long v = v0 + threadIdx.x / P.G;
        const bool valid = v < n;
        bool any = false;
        if (valid) {
            const int r = (int)(v / P.R), q = (int)(v - (long long)r * P.R);
            int side;
            const long long a = feed_row_id(P.F, r, side, q == 0 && lane_g == 0, err);
            const int* rid_row = P.rids[side] + a * (P.R + 1);
            const int d = feed_dropped_slot(P.F, rid_row, r, side, P.R, P.loo);
            const int src = q + (q >= d ? 1 : 0);
            const int* s = P.revs[side] + (a * (P.R + 1) + src) * P.T;
            long long* o = P.revs_out + v * P.T;
            unsigned char* wm = P.wmask + v * P.T;
            for (int it = 0; it < P.iters; ++it) {
                const int k = it * P.G + lane_g;
                if (k >= P.units) break;
                if (VEC) {
                    const int4 t = *reinterpret_cast<const int4*>(s + 4 * k);
                    longlong2* o2 = reinterpret_cast<longlong2*>(o + 4 * k);
                    o2[0] = make_longlong2(t.x, t.y);
                    o2[1] = make_longlong2(t.z, t.w);
                    const unsigned m = (unsigned)((long long)t.x != P.pad) | ((unsigned)((long long)t.y != P.pad) << 8) |
                                       ((unsigned)((long long)t.z != P.pad) << 16) | ((unsigned)((long long)t.w != P.pad) << 24);
                    reinterpret_cast<unsigned*>(wm)[k] = m;
                    any |= m != 0;
                } else {
                    const long long t = s[k];
                    o[k] = t;
                    wm[k] = t != P.pad;
                    any |= t != P.pad;
                }
            }
            if (lane_g == 0 && P.rids_out) P.rids_out[v] = rid_row[src];
        }
        const unsigned long long b = __ballot(any);
        if (valid && lane_g == 0 && P.rmask) {
            const unsigned long long grp = P.G == 64 ? ~0ull : ((1ull << P.G) - 1) << (threadIdx.x & 63);
            P.rmask[v] = (b & grp) != 0;
        }
    }
}

}  // namespace rbr

extern "C" int rbr_review_gather(int32_t B, int32_t R, int32_t T, const int64_t* u_ids, const int64_t* i_ids, const int32_t* user_revs,
                                 const int32_t* user_rids, int32_t U, const int32_t* item_revs, const int32_t* item_rids, int32_t I,
                                 int32_t leave_one_out, int64_t pad_token, int64_t replace_id, int64_t* revs_out,
                                 uint8_t* word_masks_out, uint8_t* rev_masks_out, int64_t* rids_out, int64_t* ids_out, int64_t* err,
                                 void* stream) {
    using namespace rbr;
    if (B <= 0 || R <= 0 || T <= 0 || U <= 0 || I <= 0 || (leave_one_out != 0 && leave_one_out != 1)) {
        set_error("rbr_review_gather: bad shape B=%d R=%d T=%d U=%d I=%d leave_one_out=%d", B, R, T, U, I, leave_one_out);
        return RBR_ERR_BAD_ARG;
    }
    if (!u_ids || !i_ids || !user_revs || !user_rids || !item_revs || !item_rids || !revs_out || !word_masks_out || !err) {
        set_error("rbr_review_gather: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    if (replace_id < 0 || replace_id >= U || replace_id >= I) {
        set_error("rbr_review_gather: replace_id %lld is not a row of both tables (U=%d, I=%d)", (long long)replace_id, U, I);
        return RBR_ERR_BAD_ARG;
    }
    ReviewGather P;
    P.F.ids[0] = reinterpret_cast<const long long*>(u_ids); P.F.ids[1] = reinterpret_cast<const long long*>(i_ids);
    P.F.rows[0] = U; P.F.rows[1] = I;
    P.F.ids_out = reinterpret_cast<long long*>(ids_out);
    P.F.replace = replace_id;
    P.F.B = B;
    P.revs[0] = user_revs; P.revs[1] = item_revs;
    P.rids[0] = user_rids; P.rids[1] = item_rids;
    P.revs_out = reinterpret_cast<long long*>(revs_out);
    P.wmask = word_masks_out;
    P.rmask = rev_masks_out;
    P.rids_out = reinterpret_cast<long long*>(rids_out);
    P.pad = pad_token;
    P.R = R; P.T = T; P.loo = leave_one_out;
    const auto aligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    const bool vec = T % 4 == 0 && aligned(user_revs, 16) && aligned(item_revs, 16) && aligned(revs_out, 16) && aligned(word_masks_out, 4);
    P.units = vec ? T / 4 : T;
    P.G = 1;
    while (P.G < P.units && P.G < 64) P.G <<= 1;
    P.iters = (P.units + P.G - 1) / P.G;
    const long long per_block = 256 / P.G, n = 2LL * B * R;
    const unsigned grid = (unsigned)std::min<long long>((n + per_block - 1) / per_block, 1LL << 20);      // block-stride beyond that
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(review_gather_kernel<true>, dim3(grid), dim3(256), 0, st, P, reinterpret_cast<long long*>(err));
    else
        hipLaunchKernelGGL(review_gather_kernel<false>, dim3(grid), dim3(256), 0, st, P, reinterpret_cast<long long*>(err));
    RBR_CHECK_LAUNCH("review_gather launch");
    return 0;
}
