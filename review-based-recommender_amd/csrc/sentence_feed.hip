// sentence_feed.hip -- the id-fed batch of the sentence split (AHN).  A sentence-split example follows the review split's rule
// (preprocess/divide_and_create_example_sent.py:262-300 is divide_and_create_example_word.py's copy / index() / pop() / truncate-pad
// with a review of sent_num x word_num tokens), so the tables hold R + 1 slots per id for the reason given at the top of
// review_feed.hip, and the dropped slot is feed_ids.h's feed_dropped_slot:
//
//   out slot q <- table slot q + (q >= d)                      (reviews [S, W] and rids alike)
//   sent_len  = number of tokens != pad_token in the sentence  (train_ahn.py:160-170 counts; it does not look for a prefix)
//   sent_mask = sent_len > 0                                   (:149-157: token sum != 0, the same thing for non-negative ids)
//   rev_mask  = any sentence of the review is non-empty        (:173-184)
// Stacked outputs, user rows first, and the id convention of feed_ids.h.  One launch, nothing synchronises, integers only.
//
// Work split: a power-of-two group of G lanes owns one output sentence; a workgroup owns whole reviews -- `rpb` of them per tile,
// their rpb * S sentences on its 256 / G groups (in `passes` rounds when one review has more sentences than the workgroup has
// groups; then rpb = 1).  The sentence length is a butterfly sum inside the group; the review mask is the OR of the groups'
// flags of one review, which may sit in different waves: each group leaves its flag in LDS, ONE barrier, and the first rpb
// threads of the workgroup combine theirs.  The flags are double-buffered by tile parity, so the barrier of the next tile is
// the only thing between a reader of this tile and a writer of the one after next.
#include "rbr_common.h"
#include "feed_ids.h"

namespace rbr {

struct SentenceGather {
    FeedIds F;
    const int* revs[2];          // [N, R + 1, S, W]
    const int* rids[2];          // [N, R + 1]
    long long* revs_out;         // [2B, R, S, W]
    long long* len_out;          // [2B, R, S]
    unsigned char* smask;        // [2B, R, S]
    unsigned char* rmask;        // [2B, R]
    long long* rids_out;         // [2B, R] or null
    long long pad;
    int R, S, W, loo;
    int G, units, iters;         // lanes per sentence (a power of two <= 64), units per sentence (4-token chunks or tokens), ceil(units / G)
    int per_block, rpb, passes;  // groups per workgroup (256 / G), reviews per tile, ceil(rpb * S / per_block)
};

// VEC (W % 4 == 0, aligned pointers): a 16-byte load of int32 tokens and two 16-byte int64 stores per unit; otherwise one token
// per unit.
template <bool VEC>
__global__ __launch_bounds__(256) void sentence_gather_kernel(const SentenceGather P, long long* __restrict__ err) {
    __shared__ int s_flag[2][256];
    const int lane_g = threadIdx.x & (P.G - 1);
    const int g = threadIdx.x / P.G;
    const long long n_rev = 2LL * P.F.B * P.R;
    const int tile_sents = P.rpb * P.S;
    int buf = 0;
    // the trip counts depend on the block alone: whole waves reach the shuffles and whole workgroups the barrier
    for (long long rev0 = (long long)blockIdx.x * P.rpb; rev0 < n_rev; rev0 += (long long)gridDim.x * P.rpb, buf ^= 1) {
        bool any = false;
        for (int p = 0; p < P.passes; ++p) {
            const int ts = p * P.per_block + g;          // sentence of the tile
            const int t = ts / P.S, s = ts - t * P.S;    // its review of the tile, its place in the review
            const long long rev = rev0 + t;
            const bool valid = ts < tile_sents && rev < n_rev;
            const long long v = rev * P.S + s;
            int cnt = 0;
            if (valid) {
                const int r = (int)(rev / P.R), q = (int)(rev - (long long)r * P.R);
                int side;
                const long long a = feed_row_id(P.F, r, side, q == 0 && s == 0 && lane_g == 0, err);
                const int* rid_row = P.rids[side] + a * (P.R + 1);
                const int d = feed_dropped_slot(P.F, rid_row, r, side, P.R, P.loo);
                const int src = q + (q >= d ? 1 : 0);
                const int* sp = P.revs[side] + ((a * (P.R + 1) + src) * P.S + s) * P.W;
                long long* o = P.revs_out + v * P.W;
                for (int it = 0; it < P.iters; ++it) {
                    const int k = it * P.G + lane_g;
                    if (k >= P.units) break;
                    if (VEC) {
                        const int4 x = *reinterpret_cast<const int4*>(sp + 4 * k);
                        longlong2* o2 = reinterpret_cast<longlong2*>(o + 4 * k);
                        o2[0] = make_longlong2(x.x, x.y);
                        o2[1] = make_longlong2(x.z, x.w);
                        cnt += (int)((long long)x.x != P.pad) + (int)((long long)x.y != P.pad) + (int)((long long)x.z != P.pad) +
                               (int)((long long)x.w != P.pad);
                    } else {
                        const long long x = sp[k];
                        o[k] = x;
                        cnt += (int)(x != P.pad);
                    }
                }
                if (s == 0 && lane_g == 0 && P.rids_out) P.rids_out[rev] = rid_row[src];
            }
            cnt = wave_sum_n(cnt, P.G);                  // 0 in a group without a sentence
            if (valid && lane_g == 0) {
                P.len_out[v] = cnt;
                P.smask[v] = cnt > 0;
            }
            any |= cnt > 0;
        }
        if (lane_g == 0) s_flag[buf][g] = any ? 1 : 0;
        __syncthreads();
        if ((int)threadIdx.x < P.rpb && rev0 + threadIdx.x < n_rev) {
            // review t of the tile: group slots [t * S, (t + 1) * S); with several passes the one review had every slot
            const int lo = threadIdx.x * P.S, hi = min(lo + P.S, P.per_block);
            int f = 0;
            for (int k = lo; k < hi; ++k) f |= s_flag[buf][k];
            P.rmask[rev0 + threadIdx.x] = f != 0;
        }
    }
}

}  // namespace rbr

extern "C" int rbr_sentence_gather(int32_t B, int32_t R, int32_t S, int32_t W, const int64_t* u_ids, const int64_t* i_ids,
                                   const int32_t* user_revs, const int32_t* user_rids, int32_t U, const int32_t* item_revs,
                                   const int32_t* item_rids, int32_t I, int32_t leave_one_out, int64_t pad_token, int64_t replace_id,
                                   int64_t* revs_out, int64_t* sent_len_out, uint8_t* sent_mask_out, uint8_t* rev_mask_out,
                                   int64_t* rids_out, int64_t* ids_out, int64_t* err, void* stream) {
    using namespace rbr;
    if (B <= 0 || R <= 0 || S <= 0 || W <= 0 || U <= 0 || I <= 0 || (leave_one_out != 0 && leave_one_out != 1)) {
        set_error("rbr_sentence_gather: bad shape B=%d R=%d S=%d W=%d U=%d I=%d leave_one_out=%d", B, R, S, W, U, I, leave_one_out);
        return RBR_ERR_BAD_ARG;
    }
    if (!u_ids || !i_ids || !user_revs || !user_rids || !item_revs || !item_rids || !revs_out || !sent_len_out || !sent_mask_out ||
        !rev_mask_out || !err) {
        set_error("rbr_sentence_gather: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    if (replace_id < 0 || replace_id >= U || replace_id >= I) {
        set_error("rbr_sentence_gather: replace_id %lld is not a row of both tables (U=%d, I=%d)", (long long)replace_id, U, I);
        return RBR_ERR_BAD_ARG;
    }
    SentenceGather P;
    P.F.ids[0] = reinterpret_cast<const long long*>(u_ids); P.F.ids[1] = reinterpret_cast<const long long*>(i_ids);
    P.F.rows[0] = U; P.F.rows[1] = I;
    P.F.ids_out = reinterpret_cast<long long*>(ids_out);
    P.F.replace = replace_id;
    P.F.B = B;
    P.revs[0] = user_revs; P.revs[1] = item_revs;
    P.rids[0] = user_rids; P.rids[1] = item_rids;
    P.revs_out = reinterpret_cast<long long*>(revs_out);
    P.len_out = reinterpret_cast<long long*>(sent_len_out);
    P.smask = sent_mask_out;
    P.rmask = rev_mask_out;
    P.rids_out = reinterpret_cast<long long*>(rids_out);
    P.pad = pad_token;
    P.R = R; P.S = S; P.W = W; P.loo = leave_one_out;
    const auto aligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    const bool vec = W % 4 == 0 && aligned(user_revs, 16) && aligned(item_revs, 16) && aligned(revs_out, 16);
    P.units = vec ? W / 4 : W;
    P.G = 1;
    while (P.G < P.units && P.G < 64) P.G <<= 1;
    P.iters = (P.units + P.G - 1) / P.G;
    P.per_block = 256 / P.G;
    P.rpb = std::max(1, P.per_block / S);
    P.passes = (P.rpb * S + P.per_block - 1) / P.per_block;
    const long long n_rev = 2LL * B * R;
    const unsigned grid = (unsigned)std::min<long long>((n_rev + P.rpb - 1) / P.rpb, 1LL << 20);      // block-stride beyond that
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(sentence_gather_kernel<true>, dim3(grid), dim3(256), 0, st, P, reinterpret_cast<long long*>(err));
    else
        hipLaunchKernelGGL(sentence_gather_kernel<false>, dim3(grid), dim3(256), 0, st, P, reinterpret_cast<long long*>(err));
    RBR_CHECK_LAUNCH("sentence_gather launch");
    return 0;
}
