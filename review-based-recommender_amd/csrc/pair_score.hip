// pair_score.hip -- scoring from cached tower latents: every tower of the four models depends on its own side only, so a
// catalogue is encoded ONCE into latent tables ul [U, K] / il [I, K] and a (user, item) score is the pair-dependent tail alone:
//   RBR_SCORE_FM : relu(ul[u,:] * il[i,:]) . h + ub[u] + ib[i] + g     FM.forward in eval mode (deepconn/layers.py:189-209;
//                                                                      ub / ib NULL = FMWithoutUIBias)
//   RBR_SCORE_DOT: sum_k ul[u,k] * il[i,k]                             D-ATT (dual_att/dual_att.py:58)
// The FM score is not a GEMM (the ReLU sits between the product and the sum over k).  Four entries share ONE arithmetic,
// score_step / score_finish of pair_score_math.h -- explicit fmaf / __fmul_rn, k ascending -- so they agree bit for bit on the same pair:
//   rbr_pair_score_ids  : B pairs gathered by id (validation from the tables instead of two document encodes per pair)
//   rbr_pair_score_dense: the [Nu, Ni] matrix (tests, small catalogues)
//   rbr_pair_score_topk : the k best items of every user row WITHOUT the [Nu, Ni] matrix, two launches:
//     1. topk_slice_kernel, one wave per (tile of kTU user rows, slice of the items).  A lane owns one item of a 64-item step and
//        keeps its latents in VGPRs (32 at a time: one 128-byte line of the row); the user latents and h are wave-uniform (scalar
//        loads), so a (pair, k) term is 3 VALU instructions (mul, max, fma) with no LDS traffic.  Each user of the tile has a
//        sorted list of its k best (score, item) keys of this slice in LDS and the score of its k-th entry as a threshold; one
//        compare + ballot per (user, step) finds the rare lanes that beat it, and only those build a key, binary-search the
//        user's exclusion list and are inserted (all 64 lanes shift the list together).
//     2. topk_merge_kernel, one wave per user row: the per-slice lists through the same insertion, then items / scores out.
//   A key is (order-preserving bits of the score) << 32 | (2^32 - 1 - item): keys are distinct, "larger" is "score descending,
//   then item ascending", so the k largest keys are one well-defined set whatever order candidates arrive in -- no float
//   atomics, no order-dependent merge, the same bytes on every run.  NaN scores are never candidates.
//   rbr_pair_score_rank : where a held-out item lands -- for B (user row, target item) pairs the number of candidates whose key
//   beats the target's, the position the target has in that user's topk list of any k, without the [B, Ni] matrix, two launches:
//     1. rank_slice_kernel, the topk tile (score_chunk) with kTU integer counters per lane in place of the sorted lists: every
//        non-NaN item of the slice whose key beats the tile's wave-uniform target keys is counted, excluded or not, and so is
//        every NaN item; a wave reduction writes (beats, NaNs) per (pair, slice).
//     2. rank_finish_kernel, one wave per pair: the slices summed, then the pair's exclusion list walked (some 20 entries
//        against the Ni items of the sweep) and every entry that was counted taken off again -- exclusion is a subtraction
//        after the sweep, not a binary search per (pair, item) inside it.
//   All counts are integers: the same bytes on every run.
#include "rbr_common.h"
#include "item_csr.h"
#include "pair_score_math.h"

#include <cmath>
#include <cstdint>

namespace rbr {

constexpr int kTopKMax = 128;        // k of rbr_pair_score_topk
constexpr int kScoreDimMax = 4096;   // latent dimension K
constexpr int kTU = 8;               // user rows per wave of the slice kernel (8 accumulators beside 32 item latents)
constexpr int kMaxSplits = 64;       // item slices
constexpr int kTargetWaves = 2048;   // slice-kernel waves aimed at: 8 per CU.  Fewer, longer slices keep the insertions (about
                                     // k * ln(slice / k) per user and slice) small beside the 3 * K * slice instructions of scoring

// ---- the one arithmetic of all entries (score_step / score_finish / score_pair) and the key: pair_score_math.h

struct ScoreParams {
    const float* ul; const float* il;     // [U, K] / [I, K]
    const float* h; const float* g;       // [K], [1] (FM)
    const float* ub; const float* ib;     // [U], [I] or null (FM)
    int K;
};

// ---- B pairs by id.  An id outside its table is never dereferenced: row 0 stands in and err is updated as rbr::sanitize_id does
__device__ __forceinline__ long long checked_id(const long long* ids, int b, int rows, int set, long long* __restrict__ err) {
    long long v = ids[b];
    if ((unsigned long long)v >= (unsigned long long)rows) {
        if (err) {
            err[1] = v; err[2] = set;                 // any one offender (benign race)
            atomicAdd(reinterpret_cast<unsigned long long*>(err), 1ull);
        }
        v = 0;
    }
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void pair_score_ids_kernel(const ScoreParams P, int B, int U, int I, const long long* __restrict__ u_id,
                                                             const long long* __restrict__ i_id, float* __restrict__ out,
                                                             long long* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long u = checked_id(u_id, b, U, 0, err), i = checked_id(i_id, b, I, 1, err);
    const float ub = (MODE == RBR_SCORE_FM && P.ub) ? P.ub[u] : 0.f, ib = (MODE == RBR_SCORE_FM && P.ib) ? P.ib[i] : 0.f;
    const float g = MODE == RBR_SCORE_FM ? P.g[0] : 0.f;
    out[b] = score_pair<MODE>(P.ul + u * P.K, P.il + i * P.K, P.h, P.K, ub, ib, g);
}

// ---- [Nu, Ni]: a lane per item, blockIdx.y = user row (its latents are wave-uniform)
template <int MODE>
__global__ __launch_bounds__(256) void pair_score_dense_kernel(const ScoreParams P, int Nu, int Ni, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (i >= Ni) return;
    const float ub = (MODE == RBR_SCORE_FM && P.ub) ? P.ub[u] : 0.f, ib = (MODE == RBR_SCORE_FM && P.ib) ? P.ib[i] : 0.f;
    const float g = MODE == RBR_SCORE_FM ? P.g[0] : 0.f;
    out[(size_t)u * Ni + i] = score_pair<MODE>(P.ul + (size_t)u * P.K, P.il + (size_t)i * P.K, P.h, P.K, ub, ib, g);
}

// ---------------------------------------------------------------------------------------------------------------- top-k
// (make_key / key_score / key_item: pair_score_math.h)

// Lst[0 .. k): keys descending, 0 = empty slot.  All 64 lanes of the (single-wave) workgroup insert the same key x, which is
// in no slot yet: slot p keeps its key when that is larger, takes x when its predecessor is larger, else its predecessor's key.
__device__ __forceinline__ void list_insert(unsigned long long* Lst, int k, unsigned long long x, int lane) {
    const int p0 = lane, p1 = lane + 64;
    const unsigned long long a0 = p0 < k ? Lst[p0] : ~0ull, b0 = (p0 > 0 && p0 < k) ? Lst[p0 - 1] : ~0ull;
    unsigned long long a1 = ~0ull, b1 = ~0ull;
    if (k > 64 && p1 < k) { a1 = Lst[p1]; b1 = Lst[p1 - 1]; }
    __syncthreads();
    if (a0 < x) Lst[p0] = b0 > x ? x : b0;
    if (a1 < x) Lst[p1] = b1 > x ? x : b1;
    __syncthreads();
}

// The lanes with `c` offer their key; tk = Lst[k - 1] on entry and on return (0 while the list has room)
__device__ __forceinline__ unsigned long long list_offer(unsigned long long* Lst, int k, unsigned long long key, bool c,
                                                         unsigned long long tk, int lane) {
    unsigned long long m = __ballot(c);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned lo = __shfl((unsigned)key, src), hi = __shfl((unsigned)(key >> 32), src);
        const unsigned long long x = ((unsigned long long)hi << 32) | lo;
        if (x > tk) {                       // the threshold may have risen since the ballot
            list_insert(Lst, k, x, lane);
            tk = Lst[k - 1];
        }
    }
    return tk;
}

struct TopKArgs {
    ScoreParams P;
    ItemCsr excl;                  // user row r: the items it must never get (item_csr.h)
    unsigned long long* ws;        // [Nu, S, k] keys
    long long per;                 // items per slice (a multiple of 64)
    int Nu, Ni, k, item_lo, S, vec;
};

// KC latents of the lane's item against the kTU user rows of the tile: k0 .. k0 + KC of every accumulator, k ascending
template <int MODE, int KC>
__device__ __forceinline__ void score_chunk(float (&acc)[kTU], const float* __restrict__ ip, bool vec, const float* __restrict__ ul,
                                            const float* __restrict__ h, int u0, int Nu, int K, int k0) {
    float v[KC];
    if (vec) {
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(ip + k0)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < KC; ++j) v[j] = ip[k0 + j];
    }
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
        const float* __restrict__ up = ul + (size_t)min(u0 + u, Nu - 1) * K + k0;      // wave-uniform: scalar loads
#pragma unroll
        for (int j = 0; j < KC; ++j) acc[u] = score_step<MODE>(acc[u], up[j], v[j], MODE == RBR_SCORE_FM ? h[k0 + j] : 0.f);
    }
}

template <int MODE>
__global__ __launch_bounds__(64) void topk_slice_kernel(const TopKArgs A) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* Lst = reinterpret_cast<unsigned long long*>(smem);      // [kTU][k]
    float* thr = reinterpret_cast<float*>(Lst + kTU * A.k);                     // [kTU] score of the k-th entry, -inf while there is room
    const int lane = threadIdx.x, u0 = blockIdx.x * kTU, s = blockIdx.y;
    const int K = A.P.K, k = A.k, Nu = A.Nu;
    const float* __restrict__ ul = A.P.ul;
    const float* __restrict__ il = A.P.il;
    const float* __restrict__ h = A.P.h;
    for (int e = lane; e < kTU * k; e += 64) Lst[e] = 0ull;
    if (lane < kTU) thr[lane] = -INFINITY;
    __syncthreads();
    const long long lo = (long long)A.item_lo + (long long)s * A.per;
    const long long hi = min(lo + A.per, (long long)A.Ni);
    const float g = MODE == RBR_SCORE_FM ? A.P.g[0] : 0.f;
    for (long long base = lo; base < hi; base += 64) {
        const bool valid = base + lane < hi;
        const int item = (int)(valid ? base + lane : hi - 1);
        const float* __restrict__ ip = il + (size_t)item * K;
        float acc[kTU];
#pragma unroll
        for (int u = 0; u < kTU; ++u) acc[u] = 0.f;
        int k0 = 0;
        for (; k0 + 32 <= K; k0 += 32) score_chunk<MODE, 32>(acc, ip, A.vec != 0, ul, h, u0, Nu, K, k0);
        for (; k0 + 8 <= K; k0 += 8) score_chunk<MODE, 8>(acc, ip, A.vec != 0, ul, h, u0, Nu, K, k0);
        for (; k0 < K; ++k0) {
            const float v = ip[k0], hk = MODE == RBR_SCORE_FM ? h[k0] : 0.f;
#pragma unroll
            for (int u = 0; u < kTU; ++u) acc[u] = score_step<MODE>(acc[u], ul[(size_t)min(u0 + u, Nu - 1) * K + k0], v, hk);
        }
        const float ib = (MODE == RBR_SCORE_FM && A.P.ib) ? A.P.ib[item] : 0.f;
        unsigned um = 0;
#pragma unroll
        for (int u = 0; u < kTU; ++u) {
            const float ub = (MODE == RBR_SCORE_FM && A.P.ub) ? A.P.ub[min(u0 + u, Nu - 1)] : 0.f;
            acc[u] = score_finish<MODE>(acc[u], ub, ib, g);
            if (__ballot(valid && acc[u] >= thr[u]) != 0ull) um |= 1u << u;
        }
        // the rare path: users of the tile for which some lane reaches the threshold
        while (um) {
            const int u = __ffs((int)um) - 1;
            um &= um - 1;
            if (u0 + u >= Nu) continue;
            float sc = acc[0];
#pragma unroll
            for (int j = 1; j < kTU; ++j) sc = (j == u) ? acc[j] : sc;
            unsigned long long* Lu = Lst + u * k;
            unsigned long long tk = Lu[k - 1];
            const unsigned long long key = make_key(sc, item);
            bool c = valid && sc >= thr[u] && key > tk;
            long long xa, xe;
            if (c && csr_row(A.excl, u0 + u, xa, xe)) c = !csr_has(A.excl.item, xa, xe, item);
            const unsigned long long tk1 = list_offer(Lu, k, key, c, tk, lane);
            if (tk1 != tk) {
                if (lane == 0) thr[u] = key_score(tk1);
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int e = lane; e < kTU * k; e += 64) {
        const int u = e / k, j = e - u * k;
        if (u0 + u < Nu) A.ws[((size_t)(u0 + u) * A.S + s) * k + j] = Lst[e];
    }
}

__global__ __launch_bounds__(64) void topk_merge_kernel(const unsigned long long* __restrict__ ws, int S, int k,
                                                        long long* __restrict__ out_item, float* __restrict__ out_score) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* Lst = reinterpret_cast<unsigned long long*>(smem);      // [k]
    const int lane = threadIdx.x;
    const size_t user = blockIdx.x;
    const int n = S * k;
    const unsigned long long* __restrict__ src = ws + user * n;
    for (int e = lane; e < k; e += 64) Lst[e] = S == 1 ? src[e] : 0ull;         // one slice: its list is the answer
    __syncthreads();
    if (S > 1) {
        unsigned long long tk = 0ull;
        for (int base = 0; base < n; base += 64) {
            const int e = base + lane;
            const unsigned long long key = e < n ? src[e] : 0ull;
            tk = list_offer(Lst, k, key, key > tk, tk, lane);
        }
    }
    for (int j = lane; j < k; j += 64) {
        const unsigned long long key = Lst[j];
        out_item[user * k + j] = key ? (long long)key_item(key) : -1ll;
        out_score[user * k + j] = key ? key_score(key) : -INFINITY;
    }
}

// ----------------------------------------------------------------------------------------------------------------- rank
struct RankArgs {
    ScoreParams P;                 // P.ul [B, K] / P.ub [B]: the user rows gathered per pair
    const long long* tgt;          // [B] target item ids
    ItemCsr excl;                  // as in TopKArgs, a row per pair
    int2* ws;                      // [B, S] (items of the slice that beat the target, NaN items of the slice)
    int* rank; int* n_cand;        // [B]
    long long* err;                // the int64[4] record of rbr_sanitize_ids, or null
    long long per;                 // items per slice (a multiple of 64)
    int B, Ni, item_lo, S, vec;
};

// Key of pair b's target from score_pair (the bits every other entry gives that pair).  A target outside [0, Ni) is never
// dereferenced: row 0 stands in (the pair is unranked whatever its key).  false: the target's score is NaN.
template <int MODE>
__device__ __forceinline__ bool target_key(const RankArgs& A, int b, unsigned long long& key) {
    long long t = A.tgt[b];
    if ((unsigned long long)t >= (unsigned long long)A.Ni) t = 0;
    const int K = A.P.K;
    const float ub = (MODE == RBR_SCORE_FM && A.P.ub) ? A.P.ub[b] : 0.f, ib = (MODE == RBR_SCORE_FM && A.P.ib) ? A.P.ib[t] : 0.f;
    const float s = score_pair<MODE>(A.P.ul + (size_t)b * K, A.P.il + (size_t)t * K, A.P.h, K, ub, ib, MODE == RBR_SCORE_FM ? A.P.g[0] : 0.f);
    key = make_key(s, (int)t);
    return s == s;
}

template <int MODE>
__global__ __launch_bounds__(64) void rank_slice_kernel(const RankArgs A) {
    const int lane = threadIdx.x, u0 = blockIdx.x * kTU, s = blockIdx.y;
    const int K = A.P.K, B = A.B;
    const float* __restrict__ ul = A.P.ul;
    const float* __restrict__ il = A.P.il;
    const float* __restrict__ h = A.P.h;
    unsigned long long tk[kTU];       // wave-uniform
    int beats[kTU], nans[kTU];
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
        target_key<MODE>(A, min(u0 + u, B - 1), tk[u]);
        beats[u] = nans[u] = 0;
    }
    const long long lo = (long long)A.item_lo + (long long)s * A.per;
    const long long hi = min(lo + A.per, (long long)A.Ni);
    const float g = MODE == RBR_SCORE_FM ? A.P.g[0] : 0.f;
    for (long long base = lo; base < hi; base += 64) {
        const bool valid = base + lane < hi;
        const int item = (int)(valid ? base + lane : hi - 1);
        const float* __restrict__ ip = il + (size_t)item * K;
        float acc[kTU];
#pragma unroll
        for (int u = 0; u < kTU; ++u) acc[u] = 0.f;
        int k0 = 0;
        for (; k0 + 32 <= K; k0 += 32) score_chunk<MODE, 32>(acc, ip, A.vec != 0, ul, h, u0, B, K, k0);
        for (; k0 + 8 <= K; k0 += 8) score_chunk<MODE, 8>(acc, ip, A.vec != 0, ul, h, u0, B, K, k0);
        for (; k0 < K; ++k0) {
            const float v = ip[k0], hk = MODE == RBR_SCORE_FM ? h[k0] : 0.f;
#pragma unroll
            for (int u = 0; u < kTU; ++u) acc[u] = score_step<MODE>(acc[u], ul[(size_t)min(u0 + u, B - 1) * K + k0], v, hk);
        }
        const float ib = (MODE == RBR_SCORE_FM && A.P.ib) ? A.P.ib[item] : 0.f;
#pragma unroll
        for (int u = 0; u < kTU; ++u) {
            const float ub = (MODE == RBR_SCORE_FM && A.P.ub) ? A.P.ub[min(u0 + u, B - 1)] : 0.f;
            const float sc = score_finish<MODE>(acc[u], ub, ib, g);
            const bool nan = sc != sc;
            nans[u] += (valid && nan) ? 1 : 0;
            beats[u] += (valid && !nan && make_key(sc, item) > tk[u]) ? 1 : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
        const int nb = wave_sum(beats[u]), nn = wave_sum(nans[u]);
        if (lane == 0 && u0 + u < B) A.ws[(size_t)(u0 + u) * A.S + s] = make_int2(nb, nn);
    }
}

template <int MODE>
__global__ __launch_bounds__(64) void rank_finish_kernel(const RankArgs A) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int K = A.P.K;
    const long long t = A.tgt[b];
    const bool in_table = (unsigned long long)t < (unsigned long long)A.Ni;
    if (!in_table && lane == 0 && A.err) {            // recorded once per pair, as checked_id records an item id
        A.err[1] = t; A.err[2] = 1;
        atomicAdd(reinterpret_cast<unsigned long long*>(A.err), 1ull);
    }
    unsigned long long tk;
    const bool ranked = target_key<MODE>(A, b, tk) && in_table && t >= A.item_lo;
    int beats = 0, gone = 0;                          // `gone`: items of [item_lo, Ni) that are no candidates
    for (int s = lane; s < A.S; s += 64) {
        const int2 p = A.ws[(size_t)b * A.S + s];
        beats += p.x; gone += p.y;
    }
    long long a, e;
    if (csr_row(A.excl, b, a, e)) {
        const float ub = (MODE == RBR_SCORE_FM && A.P.ub) ? A.P.ub[b] : 0.f, g = MODE == RBR_SCORE_FM ? A.P.g[0] : 0.f;
        for (long long q = a + lane; q < e; q += 64) {
            const int j = A.excl.item[q];
            // outside the sweep, the target itself (never excluded), or the entry before it again
            if (j < A.item_lo || j >= A.Ni || (in_table && j == t) || (q > a && A.excl.item[q - 1] == j)) continue;
            const float ib = (MODE == RBR_SCORE_FM && A.P.ib) ? A.P.ib[j] : 0.f;
            const float sc = score_pair<MODE>(A.P.ul + (size_t)b * K, A.P.il + (size_t)j * K, A.P.h, K, ub, ib, g);
            if (sc != sc) continue;                   // the sweep has it among the NaNs already
            gone += 1;
            beats -= make_key(sc, j) > tk ? 1 : 0;
        }
    }
    beats = wave_sum(beats);
    gone = wave_sum(gone);
    if (lane == 0) {
        A.rank[b] = ranked ? beats : -1;
        A.n_cand[b] = A.Ni - A.item_lo - gone;
    }
}

// item slices of a call: a function of (Nu, Ni) only, so the workspace query and the call agree
static int topk_splits(int Nu, int Ni) {
    const long long tiles = ((long long)Nu + kTU - 1) / kTU;
    long long S = (kTargetWaves + tiles - 1) / tiles;
    S = std::min<long long>(S, ((long long)Ni + 63) / 64);
    return (int)std::max<long long>(1, std::min<long long>(S, kMaxSplits));
}

static int score_args_ok(const char* what, int mode, int K, const float* ul, const float* il, const float* h, const float* g) {
    if (mode != RBR_SCORE_FM && mode != RBR_SCORE_DOT) { set_error("%s: mode %d is neither RBR_SCORE_FM nor RBR_SCORE_DOT", what, mode); return RBR_ERR_BAD_ARG; }
    if (K <= 0) { set_error("%s: bad latent dimension K=%d", what, K); return RBR_ERR_BAD_ARG; }
    if (K > kScoreDimMax) { set_error("%s: K=%d above the supported %d", what, K, kScoreDimMax); return RBR_ERR_UNSUPPORTED; }
    if (!ul || !il) { set_error("%s: null latent table", what); return RBR_ERR_BAD_ARG; }
    if (mode == RBR_SCORE_FM && (!h || !g)) { set_error("%s: RBR_SCORE_FM needs h and g", what); return RBR_ERR_BAD_ARG; }
    return 0;
}

static int topk_shape_ok(const char* what, int Nu, int Ni, int K, int k) {
    if (Nu <= 0 || Ni <= 0 || K <= 0) { set_error("%s: bad shape Nu=%d Ni=%d K=%d", what, Nu, Ni, K); return RBR_ERR_BAD_ARG; }
    if (k < 1) { set_error("%s: k=%d must be at least 1", what, k); return RBR_ERR_BAD_ARG; }
    if (k > kTopKMax) { set_error("%s: k=%d above the supported %d", what, k, kTopKMax); return RBR_ERR_UNSUPPORTED; }
    if (K > kScoreDimMax) { set_error("%s: K=%d above the supported %d", what, K, kScoreDimMax); return RBR_ERR_UNSUPPORTED; }
    return 0;
}

static int rank_shape_ok(const char* what, int B, int Ni, int K) {
    if (B <= 0 || Ni <= 0 || K <= 0) { set_error("%s: bad shape B=%d Ni=%d K=%d", what, B, Ni, K); return RBR_ERR_BAD_ARG; }
    if (K > kScoreDimMax) { set_error("%s: K=%d above the supported %d", what, K, kScoreDimMax); return RBR_ERR_UNSUPPORTED; }
    return 0;
}

}  // namespace rbr

extern "C" int rbr_pair_score_ids(int32_t mode, int32_t B, int32_t K, const float* ul, int32_t U, const float* il, int32_t I,
                                  const int64_t* u_id, const int64_t* i_id, const float* h, const float* g, const float* ub,
                                  const float* ib, float* out, int64_t* err, void* stream) {
    using namespace rbr;
    if (B <= 0 || U <= 0 || I <= 0) { set_error("rbr_pair_score_ids: bad shape B=%d U=%d I=%d", B, U, I); return RBR_ERR_BAD_ARG; }
    if (int e = score_args_ok("rbr_pair_score_ids", mode, K, ul, il, h, g)) return e;
    if (!u_id || !i_id || !out) { set_error("rbr_pair_score_ids: null pointer"); return RBR_ERR_BAD_ARG; }
    const ScoreParams P{ul, il, h, g, ub, ib, K};
    const dim3 grid((B + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    const long long* u = reinterpret_cast<const long long*>(u_id);
    const long long* i = reinterpret_cast<const long long*>(i_id);
    if (mode == RBR_SCORE_FM)
        hipLaunchKernelGGL(pair_score_ids_kernel<RBR_SCORE_FM>, grid, dim3(256), 0, st, P, B, U, I, u, i, out, reinterpret_cast<long long*>(err));
    else
        hipLaunchKernelGGL(pair_score_ids_kernel<RBR_SCORE_DOT>, grid, dim3(256), 0, st, P, B, U, I, u, i, out, reinterpret_cast<long long*>(err));
    RBR_CHECK_LAUNCH("pair_score_ids launch");
    return 0;
}

extern "C" int rbr_pair_score_dense(int32_t mode, int32_t Nu, int32_t Ni, int32_t K, const float* ul, const float* il, const float* h,
                                    const float* g, const float* ub, const float* ib, float* out, void* stream) {
    using namespace rbr;
    if (Nu <= 0 || Ni <= 0) { set_error("rbr_pair_score_dense: bad shape Nu=%d Ni=%d", Nu, Ni); return RBR_ERR_BAD_ARG; }
    if (int e = score_args_ok("rbr_pair_score_dense", mode, K, ul, il, h, g)) return e;
    if (!out) { set_error("rbr_pair_score_dense: null output"); return RBR_ERR_BAD_ARG; }
    hipStream_t st = (hipStream_t)stream;
    for (int r0 = 0; r0 < Nu; r0 += 65535) {            // gridDim.y carries the user row
        const int rows = std::min(Nu - r0, 65535);
        const ScoreParams P{ul + (size_t)r0 * K, il, h, g, ub ? ub + r0 : nullptr, ib, K};
        const dim3 grid((Ni + 255) / 256, rows);
        float* o = out + (size_t)r0 * Ni;
        if (mode == RBR_SCORE_FM)
            hipLaunchKernelGGL(pair_score_dense_kernel<RBR_SCORE_FM>, grid, dim3(256), 0, st, P, rows, Ni, o);
        else
            hipLaunchKernelGGL(pair_score_dense_kernel<RBR_SCORE_DOT>, grid, dim3(256), 0, st, P, rows, Ni, o);
        RBR_CHECK_LAUNCH("pair_score_dense launch");
    }
    return 0;
}

extern "C" size_t rbr_pair_score_topk_ws_bytes(int32_t Nu, int32_t Ni, int32_t K, int32_t k) {
    using namespace rbr;
    if (topk_shape_ok("rbr_pair_score_topk_ws_bytes", Nu, Ni, K, k)) return 0;
    return (size_t)Nu * (size_t)topk_splits(Nu, Ni) * (size_t)k * sizeof(unsigned long long);
}

extern "C" int rbr_pair_score_topk(int32_t mode, int32_t Nu, int32_t Ni, int32_t K, int32_t k, int32_t item_lo, const float* ul,
                                   const float* il, const float* h, const float* g, const float* ub, const float* ib,
                                   const int64_t* excl_off, const int32_t* excl_item, int64_t excl_nnz, const int64_t* excl_row,
                                   int32_t excl_rows, int64_t* out_item, float* out_score, void* ws, void* stream) {
    using namespace rbr;
    if (int e = topk_shape_ok("rbr_pair_score_topk", Nu, Ni, K, k)) return e;
    if (int e = score_args_ok("rbr_pair_score_topk", mode, K, ul, il, h, g)) return e;
    if (item_lo < 0 || item_lo >= Ni) { set_error("rbr_pair_score_topk: item_lo=%d outside [0, %d)", item_lo, Ni); return RBR_ERR_BAD_ARG; }
    if (!out_item || !out_score || !ws) { set_error("rbr_pair_score_topk: null output or workspace"); return RBR_ERR_BAD_ARG; }
    if (int e = item_csr_ok("rbr_pair_score_topk", false, excl_off, excl_item, excl_nnz, excl_row, excl_rows)) return e;
    TopKArgs A;
    A.P = ScoreParams{ul, il, h, g, ub, ib, K};
    A.excl = item_csr(excl_off, excl_item, excl_row, excl_nnz, excl_row ? excl_rows : Nu);
    A.ws = static_cast<unsigned long long*>(ws);
    A.Nu = Nu; A.Ni = Ni; A.k = k; A.item_lo = item_lo;
    A.S = topk_splits(Nu, Ni);
    const long long n = (long long)Ni - item_lo;
    A.per = (((n + A.S - 1) / A.S) + 63) / 64 * 64;
    A.vec = (K % 4 == 0 && (reinterpret_cast<uintptr_t>(il) % 16) == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((Nu + kTU - 1) / kTU, A.S);
    const size_t lds = (size_t)kTU * k * sizeof(unsigned long long) + kTU * sizeof(float);
    if (mode == RBR_SCORE_FM)
        hipLaunchKernelGGL(topk_slice_kernel<RBR_SCORE_FM>, grid, dim3(64), lds, st, A);
    else
        hipLaunchKernelGGL(topk_slice_kernel<RBR_SCORE_DOT>, grid, dim3(64), lds, st, A);
    RBR_CHECK_LAUNCH("pair_score_topk slice launch");
    hipLaunchKernelGGL(topk_merge_kernel, dim3(Nu), dim3(64), (size_t)k * sizeof(unsigned long long), st, A.ws, A.S, k,
                       reinterpret_cast<long long*>(out_item), out_score);
    RBR_CHECK_LAUNCH("pair_score_topk merge launch");
    return 0;
}

extern "C" size_t rbr_pair_score_rank_ws_bytes(int32_t B, int32_t Ni, int32_t K) {
    using namespace rbr;
    if (rank_shape_ok("rbr_pair_score_rank_ws_bytes", B, Ni, K)) return 0;
    return (size_t)B * (size_t)topk_splits(B, Ni) * sizeof(int2);
}

extern "C" int rbr_pair_score_rank(int32_t mode, int32_t B, int32_t Ni, int32_t K, int32_t item_lo, const float* ul, const float* il,
                                   const float* h, const float* g, const float* ub, const float* ib, const int64_t* tgt,
                                   const int64_t* excl_off, const int32_t* excl_item, int64_t excl_nnz, const int64_t* excl_row,
                                   int32_t excl_rows, int32_t* rank, int32_t* n_cand, int64_t* err, void* ws, void* stream) {
    using namespace rbr;
    if (int e = rank_shape_ok("rbr_pair_score_rank", B, Ni, K)) return e;
    if (int e = score_args_ok("rbr_pair_score_rank", mode, K, ul, il, h, g)) return e;
    if (item_lo < 0 || item_lo >= Ni) { set_error("rbr_pair_score_rank: item_lo=%d outside [0, %d)", item_lo, Ni); return RBR_ERR_BAD_ARG; }
    if (!tgt || !rank || !n_cand || !ws) { set_error("rbr_pair_score_rank: null targets, output or workspace"); return RBR_ERR_BAD_ARG; }
    if (int e = item_csr_ok("rbr_pair_score_rank", false, excl_off, excl_item, excl_nnz, excl_row, excl_rows)) return e;
    RankArgs A;
    A.P = ScoreParams{ul, il, h, g, ub, ib, K};
    A.tgt = reinterpret_cast<const long long*>(tgt);
    A.excl = item_csr(excl_off, excl_item, excl_row, excl_nnz, excl_row ? excl_rows : B);
    A.ws = static_cast<int2*>(ws);
    A.rank = rank; A.n_cand = n_cand;
    A.err = reinterpret_cast<long long*>(err);
    A.B = B; A.Ni = Ni; A.item_lo = item_lo;
    A.S = topk_splits(B, Ni);
    const long long n = (long long)Ni - item_lo;
    A.per = (((n + A.S - 1) / A.S) + 63) / 64 * 64;
    A.vec = (K % 4 == 0 && (reinterpret_cast<uintptr_t>(il) % 16) == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((B + kTU - 1) / kTU, A.S);
    if (mode == RBR_SCORE_FM)
        hipLaunchKernelGGL(rank_slice_kernel<RBR_SCORE_FM>, grid, dim3(64), 0, st, A);
    else
        hipLaunchKernelGGL(rank_slice_kernel<RBR_SCORE_DOT>, grid, dim3(64), 0, st, A);
    RBR_CHECK_LAUNCH("pair_score_rank slice launch");
    if (mode == RBR_SCORE_FM)
        hipLaunchKernelGGL(rank_finish_kernel<RBR_SCORE_FM>, dim3(B), dim3(64), 0, st, A);
    else
        hipLaunchKernelGGL(rank_finish_kernel<RBR_SCORE_DOT>, dim3(B), dim3(64), 0, st, A);
    RBR_CHECK_LAUNCH("pair_score_rank finish launch");
    return 0;
}
