// review_sample.hip -- the id-fed TRAIN batch of the review split with review sampling: the reference's sample_train_review
// (trainer/train_simple_siamese.py:346-368: every time a training example is fetched, a fresh uniform random subset of
// u_rv_num / i_rv_num of its non-empty reviews, in shuffled order, padded with empty reviews) inside the gather launch of
// review_feed.hip.  The tables hold P + 1 slots per id, P >= R the pool to draw from: the leave-one-out rule of review_feed.hip
// with P in place of R names the P candidates of a row, the live ones (a token that is not pad) are ordered by a Philox key,
// and the first n of them fill the leading output slots; the rest of the R slots are empty reviews.
//
// The draw is fixed by include/rbr_hip.h (rbr_review_sample_gather) so that a host restatement gives the same integers:
//   row r, candidate q in [0, P): src(q) = q + (q >= d), key(q) = word (e & 3) of philox4x32_10(e >> 2, call = state[0], seed),
//   e = r * 64 + q; live candidates ordered by (key, q); output slot k < min(n_side, live) <- the k-th of them.
//
// One wave per output row, lane j owns table slot j (P + 1 <= 64).  Liveness is read from the tokens at launch: the row's
// (P + 1) * T tokens are one contiguous run, read once, coalesced, each lane ORs a bit per slot it saw a token of and a butterfly
// merges the 64 masks.  No LDS, no atomics but the ticket of rbr_rng.h and the id record of feed_ids.h.
#include "rbr_common.h"
#include "feed_ids.h"
#include "rbr_rng.h"

namespace rbr {

struct ReviewSample {
    FeedIds F;
    const int* revs[2];          // [N, P + 1, T]
    const int* rids[2];          // [N, P + 1]
    long long* revs_out;         // [2B, R, T]
    unsigned char* wmask;        // [2B, R, T]
    unsigned char* rmask;        // [2B, R] or null
    long long* rids_out;         // [2B, R] or null
    int* slots_out;              // [2B, R] or null
    long long pad;
    unsigned long long seed;
    int R, T, P, loo;
    int n[2];                    // reviews kept per side
    int units;                   // units per review: 4-token chunks (VEC) or tokens
    int step_q, step_r;          // 64 = step_q * units + step_r: how (slot, unit) moves when a lane steps 64 units on
};

__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= __shfl_xor(lo, o);
        hi |= __shfl_xor(hi, o);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// Wave w of the block owns output row 4 * block + w of a round; everything row-dependent is wave-uniform, so whole waves reach
// every ballot and shuffle (the trip count of the round loop depends on the block alone, for the barrier in front of the ticket).
template <bool VEC>
__global__ __launch_bounds__(256) void review_sample_gather_kernel(const ReviewSample S, unsigned long long* __restrict__ state,
                                                                   long long* __restrict__ err) {
    const unsigned long long call = state[0];       // every lane, before anything else: the last workgroup advances it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = 2LL * S.F.B;
    const int P = S.P, R = S.R, U = S.units;
    for (long long r0 = (long long)blockIdx.x * 4; r0 < rows; r0 += (long long)gridDim.x * 4) {
        const long long r = r0 + wave;
        if (r >= rows) continue;                    // wave-uniform
        int side;
        const long long a = feed_row_id(S.F, (int)r, side, lane == 0, err);
        const long long c = S.F.ids[side ^ 1][r - (long long)side * S.F.B];
        const int* __restrict__ rid_row = S.rids[side] + a * (P + 1);
        const int* __restrict__ rev_row = S.revs[side] + a * (long long)(P + 1) * S.T;
        const int rid = lane <= P ? rid_row[lane] : 0;

        // d: the first of the P leading slots written for the counterpart (rid 0 is the pad, id 0 the padding id: never a match)
        const bool may = S.loo && c > 0 && c < S.F.rows[side ^ 1];
        const unsigned long long hit = __ballot(may && lane < P && (long long)rid == c);
        const int d = hit ? __ffsll((long long)hit) - 1 : P;

        // live table slots: one coalesced pass over the row's (P + 1) * units units
        unsigned long long seen = 0ull;
        {
            int slot = lane / U, u = lane - slot * U;
            while (slot <= P) {
                bool any;
                if (VEC) {
                    const int4 t = reinterpret_cast<const int4*>(rev_row)[(long long)slot * U + u];
                    any = (long long)t.x != S.pad || (long long)t.y != S.pad || (long long)t.z != S.pad || (long long)t.w != S.pad;
                } else {
                    any = (long long)rev_row[(long long)slot * U + u] != S.pad;
                }
                seen |= (unsigned long long)any << slot;
                slot += S.step_q; u += S.step_r;
                if (u >= U) { u -= U; ++slot; }
            }
        }
        const unsigned long long live_slots = wave_or64(seen);

        // candidate q = lane: its table slot, whether it is live, its key, and its rank among the live ones by (key, q)
        const int q = lane;
        const int src = q + (q >= d ? 1 : 0);
        const bool live = q < P && ((live_slots >> src) & 1ull);
        unsigned w[4];
        philox4x32_10((unsigned long long)r * 16ull + (unsigned long long)(q >> 2), call, S.seed, w[0], w[1], w[2], w[3]);
        const unsigned key = (q & 3) == 0 ? w[0] : (q & 3) == 1 ? w[1] : (q & 3) == 2 ? w[2] : w[3];
        const unsigned long long live_q = __ballot(live);
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const unsigned kj = (unsigned)__builtin_amdgcn_readlane((int)key, j);      // j is wave-uniform
            rank += ((live_q >> j) & 1ull) && (kj < key || (kj == key && j < q)) ? 1 : 0;
        }
        const int m = __popcll(live_q);
        const int keep = S.n[side] < m ? S.n[side] : m;
        const bool chosen = live && rank < keep;

        // lane k < R learns the table slot of output slot k (-1: an empty review)
        int mine = -1;
        for (int k = 0; k < R; ++k) {
            const unsigned long long b = __ballot(chosen && rank == k);
            const int qk = b ? __ffsll((long long)b) - 1 : -1;
            const int sk = qk < 0 ? -1 : qk + (qk >= d ? 1 : 0);
            mine = lane == k ? sk : mine;
        }
        const int my_rid = __shfl(rid, mine < 0 ? 0 : mine);
        if (lane < R) {
            const long long v = r * R + lane;
            if (S.rmask) S.rmask[v] = mine >= 0;
            if (S.rids_out) S.rids_out[v] = mine >= 0 ? (long long)my_rid : 0;
            if (S.slots_out) S.slots_out[v] = mine;
        }

        // the copy: the row's R * units output units, flat over the wave
        long long* __restrict__ o = S.revs_out + r * (long long)R * S.T;
        unsigned char* __restrict__ wm = S.wmask + r * (long long)R * S.T;
        int k = lane / U, u = lane - k * U;
        const int rounds = (R * U + 63) >> 6;       // wave-uniform: whole waves reach the shuffle
        for (int it = 0; it < rounds; ++it) {
            const int sk = __shfl(mine, k < R ? k : 0);
            if (k < R) {
                if (VEC) {
                    int4 t = make_int4(0, 0, 0, 0);
                    if (sk >= 0) t = reinterpret_cast<const int4*>(rev_row)[(long long)sk * U + u];
                    long long x = t.x, y = t.y, z = t.z, ww = t.w;
                    if (sk < 0) x = y = z = ww = S.pad;
                    longlong2* o2 = reinterpret_cast<longlong2*>(o + ((long long)k * U + u) * 4);
                    o2[0] = make_longlong2(x, y);
                    o2[1] = make_longlong2(z, ww);
                    const unsigned mk = (unsigned)(x != S.pad) | ((unsigned)(y != S.pad) << 8) | ((unsigned)(z != S.pad) << 16) |
                                        ((unsigned)(ww != S.pad) << 24);
                    reinterpret_cast<unsigned*>(wm)[(long long)k * U + u] = mk;
                } else {
                    const long long t = sk >= 0 ? (long long)rev_row[(long long)sk * U + u] : S.pad;
                    o[(long long)k * U + u] = t;
                    wm[(long long)k * U + u] = t != S.pad;
                }
            }
            k += S.step_q; u += S.step_r;
            if (u >= U) { u -= U; ++k; }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) rng_advance_call(state, call);
}

}  // namespace rbr

extern "C" int rbr_review_sample_gather(int32_t B, int32_t R, int32_t T, int32_t P, const int64_t* u_ids, const int64_t* i_ids,
                                        const int32_t* user_revs, const int32_t* user_rids, int32_t U, const int32_t* item_revs,
                                        const int32_t* item_rids, int32_t I, int32_t leave_one_out, int32_t n_user, int32_t n_item,
                                        int64_t pad_token, int64_t replace_id, uint64_t seed, uint64_t* state, int64_t* revs_out,
                                        uint8_t* word_masks_out, uint8_t* rev_masks_out, int64_t* rids_out, int64_t* ids_out,
                                        int32_t* slots_out, int64_t* err, void* stream) {
    using namespace rbr;
    if (B <= 0 || B > (1 << 30) || R <= 0 || T <= 0 || U <= 0 || I <= 0 || (leave_one_out != 0 && leave_one_out != 1)) {
        set_error("rbr_review_sample_gather: bad shape B=%d R=%d T=%d U=%d I=%d leave_one_out=%d", B, R, T, U, I, leave_one_out);
        return RBR_ERR_BAD_ARG;
    }
    if (P < R || P > 63) {
        set_error("rbr_review_sample_gather: pool P=%d outside [R=%d, 63]", P, R);
        return RBR_ERR_BAD_ARG;
    }
    if (n_user < 1 || n_user > R || n_item < 1 || n_item > R) {
        set_error("rbr_review_sample_gather: keep counts n_user=%d n_item=%d outside [1, R=%d]", n_user, n_item, R);
        return RBR_ERR_BAD_ARG;
    }
    if (replace_id < 0 || replace_id >= U || replace_id >= I) {
        set_error("rbr_review_sample_gather: replace_id %lld is not a row of both tables (U=%d, I=%d)", (long long)replace_id, U, I);
        return RBR_ERR_BAD_ARG;
    }
    if (!u_ids || !i_ids || !user_revs || !user_rids || !item_revs || !item_rids || !state || !revs_out || !word_masks_out || !err) {
        set_error("rbr_review_sample_gather: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    ReviewSample S;
    S.F.ids[0] = reinterpret_cast<const long long*>(u_ids); S.F.ids[1] = reinterpret_cast<const long long*>(i_ids);
    S.F.rows[0] = U; S.F.rows[1] = I;
    S.F.ids_out = reinterpret_cast<long long*>(ids_out);
    S.F.replace = replace_id;
    S.F.B = B;
    S.revs[0] = user_revs; S.revs[1] = item_revs;
    S.rids[0] = user_rids; S.rids[1] = item_rids;
    S.revs_out = reinterpret_cast<long long*>(revs_out);
    S.wmask = word_masks_out;
    S.rmask = rev_masks_out;
    S.rids_out = reinterpret_cast<long long*>(rids_out);
    S.slots_out = slots_out;
    S.pad = pad_token;
    S.seed = seed;
    S.R = R; S.T = T; S.P = P; S.loo = leave_one_out;
    S.n[0] = n_user; S.n[1] = n_item;
    const auto aligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; };
    const bool vec = T % 4 == 0 && aligned(user_revs, 16) && aligned(item_revs, 16) && aligned(revs_out, 16) && aligned(word_masks_out, 4);
    S.units = vec ? T / 4 : T;
    S.step_q = 64 / S.units; S.step_r = 64 % S.units;
    const long long blocks = (2LL * B + 3) / 4;
    const unsigned grid = (unsigned)std::min<long long>(blocks, 1024);      // block-stride beyond that
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sp = reinterpret_cast<unsigned long long*>(state);
    if (vec)
        hipLaunchKernelGGL(review_sample_gather_kernel<true>, dim3(grid), dim3(256), 0, st, S, sp, reinterpret_cast<long long*>(err));
    else
        hipLaunchKernelGGL(review_sample_gather_kernel<false>, dim3(grid), dim3(256), 0, st, S, sp, reinterpret_cast<long long*>(err));
    RBR_CHECK_LAUNCH("review_sample_gather launch");
    return 0;
}
