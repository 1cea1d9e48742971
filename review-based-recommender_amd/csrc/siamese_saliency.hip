// siamese_saliency.hip -- per-token and per-review contributions (gradient x input) of a SimpleSiamese tower: rbr_siamese_saliency.
//
// The tower is a masked average of word rows, an optional Linear + Tanh, AddictiveAttention over the reviews and LastFeat
// (review_bag.hip has the forward).  There is no max-pool, so nothing is held fixed: for a gradient g on the pooled feature the
// chain rule runs through the attention softmax as well, and splits into the part with the attention weights held constant
// (`fixed`) and the part that moves the weights (`through`); rbr_hip.h has the formula.
//
// One workgroup per side row (a user or an item), as addatt_fwd_kernel has, two parts:
//   1. the small part, in LDS: c_r = <g, x_r>, d logit_r, the attention's tanh projection recomputed from x, and per review the
//      two gradients on the averaged row -- gm_fixed_r and gm_thru_r [E] -- through the transform when there is one;
//   2. the row gather, the hot part.  A row is shared by G lanes (G = 1 .. 64 by the row width: one round over a row of up to 64
//      columns), so a wave holds 64 / G tokens side by side and, with kSsFlight rows in flight per group, takes a TILE of
//      min(64, 64 / G * kSsFlight) tokens of one review at a time; the waves take the (review, tile) pairs in turn.  The row
//      indices of a tile are fetched one per lane and broadcast (bag_fwd_kernel's scheme), ONE TILE AHEAD of the row reads, so a
//      tile waits for one load latency, not for the chain mask -> id -> row.  Every token row is read ONCE and dotted with both gm
//      vectors while it is in registers.  A wave's first tile depends on nothing part 1 computes: it is fetched BEFORE part 1.
// A side row is a few hundred rows of a few hundred bytes behind a chain of small loops: latency, not bandwidth, is what there is
// to hide, so the workgroup is 16 waves -- every serial loop of part 1 is one or two rounds, and part 2 has as many tiles in flight
// as a CU can hold (DESIGN.md 4.24 and profiles/r24_* have the measurements).
// Every output element is written once with a plain store, by one lane, after a butterfly of fixed order: no atomics, and a side
// row depends on nothing but itself -- the same bits on every run and in every batch.  Nothing of shape [n, R, T, E] is written.
#include "rbr_common.h"

namespace rbr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSsMaxR = 64;         // reviews per side row: kAttMaxR of review_bag.hip
constexpr int kSsThreads = 1024, kSsWaves = kSsThreads / kWave;
constexpr int kSsStretch = 64;      // the widest tile: one row index per lane
constexpr int kSsFlight = 8;        // token rows a lane group has in flight
constexpr size_t kSsLdsBytes = 64 * 1024;

struct SsArgs {
    int n, R, T, E, F, K;
    int G;                          // lanes per token: the power of two >= min(columns of a row, 64)
    int V;
    const float* table; const long long* ids; const unsigned char* word_mask; const unsigned char* rev_mask;
    const float* y; const float* a; const float* g; const float* Wt; const float* Wp; const float* bp; const float* wi;
    float* fixed; float* through; float* reviews;
};

__host__ __device__ inline int ss_pad4(int x) { return (x + 3) & ~3; }

// LDS floats: gy_fixed | gy_thru [R, F] | u [R, K] | g [F] | c, d logit, a, inv [kSsMaxR each] | with Wt: gm_fixed | gm_thru [R, E]
static size_t ss_lds_floats(int R, int E, int F, int K, bool has_wt) {
    return 2 * (size_t)ss_pad4(R * F) + ss_pad4(R * K) + ss_pad4(F) + 4 * kSsMaxR + (has_wt ? 2 * (size_t)ss_pad4(R * E) : 0);
}

// W columns of a row at p: four as one 16-byte load, or one (the other three count as 0.0f, which adds nothing)
template <bool VEC4>
__device__ __forceinline__ f32x4 ss_cols(const float* p) {
    if (VEC4) return *reinterpret_cast<const f32x4*>(p);
    return f32x4{p[0], 0.f, 0.f, 0.f};
}

__device__ __forceinline__ float ss_dot(f32x4 v, f32x4 m, float acc) {
    return fmaf(v.x, m.x, fmaf(v.y, m.y, fmaf(v.z, m.z, fmaf(v.w, m.w, acc))));
}

// One tile of the row gather: kSsFlight rows per lane group, fetched (ss_fetch) and later reduced against the review's gm vectors.
struct SsTile {
    int r, nt;                      // review and tokens of the tile
    long tok0;                      // first token of the tile in ids / word_mask / fixed / through
    int row[kSsFlight];             // table row of the group's token u (-1: none)
    f32x4 v[kSsFlight];             // its first-round columns
};

// Every lane fetches ONE row index of tile `it` (-1: masked, past the end, or an id outside the table, whose row counts as zero and
// is never used as an index).  The id and the mask byte are two independent loads.
__device__ __forceinline__ int ss_index(const SsArgs& A, int it, int tile, int ntile, long rev0, int lane) {
    const int r = it / ntile, t0 = (it - r * ntile) * tile;
    const long tok0 = (rev0 + r) * A.T + t0;
    int my_row = -1;
    if (lane < min(tile, A.T - t0)) {
        const long long id = A.ids[tok0 + lane];
        const bool live = A.word_mask == nullptr || A.word_mask[tok0 + lane];
        if (live && (unsigned long long)id < (unsigned long long)(unsigned)A.V) my_row = (int)id;
    }
    return my_row;
}

// The indices of tile `it` (my_row, from ss_index) are broadcast to the groups and the rows' first-round columns are read.  Neither
// function depends on anything part 1 computes.  Every lane of the wave makes the call.
template <bool VEC4>
__device__ __forceinline__ void ss_fetch(const SsArgs& A, int it, int my_row, int tile, int ntile, long rev0, int ngrp, int gi, int sl,
                                         bool col_ok, SsTile& t) {
    constexpr int W = VEC4 ? 4 : 1;
    t.r = it / ntile;
    const int t0 = (it - t.r * ntile) * tile;
    t.tok0 = (rev0 + t.r) * A.T + t0;
    t.nt = min(tile, A.T - t0);
#pragma unroll
    for (int u = 0; u < kSsFlight; ++u) {
        const int l = u * ngrp + gi;
        t.row[u] = __shfl(my_row, l & 63);
        if (l >= t.nt) t.row[u] = -1;
        t.v[u] = (col_ok && t.row[u] >= 0) ? ss_cols<VEC4>(A.table + (long)t.row[u] * A.E + W * sl) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <bool VEC4>
__global__ __launch_bounds__(kSsThreads) void siamese_saliency_kernel(const SsArgs A) {
    extern __shared__ __align__(16) float sm[];
    const int R = A.R, T = A.T, E = A.E, F = A.F, K = A.K;
    float* s_x = sm;                                  // [R][F] x = y[b], then gy_fixed in place
    float* s_t = s_x + ss_pad4(R * F);                // [R][F] gy_thru
    float* s_u = s_t + ss_pad4(R * F);                // [R][K] wi * (1 - tp^2)
    float* s_g = s_u + ss_pad4(R * K);                // [F]
    float* s_c = s_g + ss_pad4(F);                    // [R] c_r
    float* s_dl = s_c + kSsMaxR;                      // [R] d logit_r
    float* s_a = s_dl + kSsMaxR;                      // [R] attention weights
    float* s_inv = s_a + kSsMaxR;                     // [R] 1 / (unmasked tokens + 1e-8)
    const bool has_wt = A.Wt != nullptr;
    float* s_mf = has_wt ? s_inv + kSsMaxR : s_x;     // [R][E] gm_fixed (without the transform gm = gy, F == E)
    float* s_mt = has_wt ? s_mf + ss_pad4(R * E) : s_t;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long rev0 = (long)b * R;                    // first review of the side row in a / rev_mask / reviews
    const float* __restrict__ Wp = A.Wp;

    // the gather's geometry, and the wave's FIRST tile: its rows are on their way while part 1 runs
    constexpr int W = VEC4 ? 4 : 1;
    const int ncol = E / W, G = A.G, ngrp = 64 / G, gi = lane / G, sl = lane % G;
    const int tile = min(kSsStretch, ngrp * kSsFlight), ntile = (T + tile - 1) / tile, n_items = R * ntile;
    const bool col_ok = sl < ncol;
    SsTile tl;
    int it = wave, next_row = -1;                     // next_row: the lane's row index of the wave's NEXT tile, one tile ahead
    if (it < n_items) {
        ss_fetch<VEC4>(A, it, ss_index(A, it, tile, ntile, rev0, lane), tile, ntile, rev0, ngrp, gi, sl, col_ok, tl);
        if (it + kSsWaves < n_items) next_row = ss_index(A, it + kSsWaves, tile, ntile, rev0, lane);
    }

    // ---- the small part
    for (int e = tid; e < R * F; e += kSsThreads) s_x[e] = A.y[rev0 * F + e];
    for (int f = tid; f < F; f += kSsThreads) s_g[f] = A.g[(long)b * F + f];
    if (tid < R) s_a[tid] = A.a[rev0 + tid];
    __syncthreads();
    for (int r = wave; r < R; r += kSsWaves) {        // c_r and the review's token count: one wave per review
        float acc = 0.f;
        for (int f = lane; f < F; f += 64) acc = fmaf(s_g[f], s_x[r * F + f], acc);
        acc = wave_sum(acc);
        int cnt = 0;
        if (A.word_mask != nullptr) {
            const unsigned char* wm = A.word_mask + (rev0 + r) * T;
            for (int l = lane; l < T; l += 64) cnt += wm[l] ? 1 : 0;
            cnt = wave_sum(cnt);
        } else {
            cnt = T;
        }
        if (lane == 0) { s_c[r] = acc; s_inv[r] = 1.f / ((float)cnt + 1e-8f); }
    }
    // tp = tanh(Wp x + bp), kept as wi * tanh'.  The reviews run fastest over the threads: a wave reads a few rows of Wp, each
    // address shared by the R threads of one k, instead of 64 rows at once
    for (int e = tid; e < R * K; e += kSsThreads) {
        const int k = e / R, r = e - k * R;
        float acc = A.bp[k];
        const float* wrow = Wp + (long)k * F;
        for (int f = 0; f < F; ++f) acc = fmaf(s_x[r * F + f], wrow[f], acc);
        const float tv = tanhf(acc);
        s_u[r * K + k] = A.wi[k] * (1.f - tv * tv);
    }
    __syncthreads();
    if (tid < R) {
        float cbar = 0.f;
        for (int r = 0; r < R; ++r) cbar = fmaf(s_a[r], s_c[r], cbar);
        const float s = s_a[tid];
        // masked_fill blocks the gradient of masked logits (also when every review is masked and s is uniform)
        s_dl[tid] = (A.rev_mask == nullptr || A.rev_mask[rev0 + tid]) ? s * (s_c[tid] - cbar) : 0.f;
        A.reviews[rev0 + tid] = s * s_c[tid];
    }
    __syncthreads();
    for (int e = tid; e < R * F; e += kSsThreads) {   // gy_fixed = s g, gy_thru = d logit * Wp^T u, both times tanh'(x) under Wt
        const int r = e / F, f = e - r * F;
        float q = 0.f;
        for (int k = 0; k < K; ++k) q = fmaf(s_u[r * K + k], Wp[(long)k * F + f], q);
        const float x = s_x[e];
        const float d = 1.f - x * x;
        float gf = s_a[r] * s_g[f], gt = s_dl[r] * q;
        if (has_wt) { gf *= d; gt *= d; }
        s_x[e] = gf;
        s_t[e] = gt;
    }
    __syncthreads();
    if (has_wt) {                                     // gm = Wt^T gy
        for (int e = tid; e < R * E; e += kSsThreads) {
            const int r = e / E, d = e - r * E;
            float mf = 0.f, mt = 0.f;
            for (int f = 0; f < F; ++f) {
                const float w = A.Wt[(long)f * E + d];
                mf = fmaf(s_x[r * F + f], w, mf);
                mt = fmaf(s_t[r * F + f], w, mt);
            }
            s_mf[e] = mf;
            s_mt[e] = mt;
        }
        __syncthreads();
    }

    // ---- the row gather
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ table = A.table;
    while (it < n_items) {
        const float inv = s_inv[tl.r];
        const float* mf = s_mf + tl.r * E;
        const float* mt = s_mt + tl.r * E;
        const f32x4 mf0 = col_ok ? ss_cols<VEC4>(mf + W * sl) : zero;      // the first round's gm columns stay in registers
        const f32x4 mt0 = col_ok ? ss_cols<VEC4>(mt + W * sl) : zero;
        float p[2 * kSsFlight];                       // the tile's partial dots: fixed of token u, through of token u
#pragma unroll
        for (int u = 0; u < kSsFlight; ++u) {
            float pf = ss_dot(tl.v[u], mf0, 0.f), pt = ss_dot(tl.v[u], mt0, 0.f);
            if (tl.row[u] >= 0)                       // rows wider than one round (G == 64): the gm columns come from LDS
                for (int q = sl + G; q < ncol; q += G) {
                    const f32x4 w = ss_cols<VEC4>(table + (long)tl.row[u] * E + W * q);
                    pf = ss_dot(w, ss_cols<VEC4>(mf + W * q), pf);
                    pt = ss_dot(w, ss_cols<VEC4>(mt + W * q), pt);
                }
            p[2 * u] = pf;
            p[2 * u + 1] = pt;
        }
        wave_sum_n(p, G);                             // the 16 butterflies step by step together: a step waits for ONE shuffle, not 16
#pragma unroll
        for (int u = 0; u < kSsFlight; ++u) {
            const int l = u * ngrp + gi;
            if (sl == 0 && l < tl.nt) {               // a token without a row gets exactly 0 (inv is 1e8 where a review has none)
                A.fixed[tl.tok0 + l] = tl.row[u] >= 0 ? inv * p[2 * u] : 0.f;
                A.through[tl.tok0 + l] = tl.row[u] >= 0 ? inv * p[2 * u + 1] : 0.f;
            }
        }
        it += kSsWaves;
        if (it < n_items) {
            ss_fetch<VEC4>(A, it, next_row, tile, ntile, rev0, ngrp, gi, sl, col_ok, tl);
            if (it + kSsWaves < n_items) next_row = ss_index(A, it + kSsWaves, tile, ntile, rev0, lane);
        }
    }
}

}  // namespace rbr

using namespace rbr;

extern "C" int rbr_siamese_saliency(int32_t n, int32_t R, int32_t T, int32_t V, int32_t E, int32_t F, int32_t K, const float* table,
                                    const int64_t* ids, const uint8_t* word_mask, const uint8_t* rev_mask, const float* y,
                                    const float* a, const float* g, const float* Wt, const float* Wp, const float* bp,
                                    const float* wi, float* fixed, float* through, float* reviews, void* stream) {
    static_assert(kSsStretch == kWave, "one row offset per lane");
    if (n < 0 || R <= 0 || T <= 0 || V <= 0 || E <= 0 || F <= 0 || K <= 0 || E > kMaxDim || F > kMaxDim || K > kMaxDim) {
        set_error("rbr_siamese_saliency: bad shape n=%d R=%d T=%d V=%d E=%d F=%d K=%d", n, R, T, V, E, F, K);
        return RBR_ERR_BAD_ARG;
    }
    if (n == 0) return 0;
    if (R > kSsMaxR) { set_error("rbr_siamese_saliency: R=%d reviews (<= %d)", R, kSsMaxR); return RBR_ERR_BAD_ARG; }
    if (!table || !ids || !y || !a || !g || !Wp || !bp || !wi || !fixed || !through || !reviews) {
        set_error("rbr_siamese_saliency: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    if (!Wt && F != E) { set_error("rbr_siamese_saliency: F=%d != E=%d needs the transform's weight Wt", F, E); return RBR_ERR_BAD_ARG; }
    const size_t lds = ss_lds_floats(R, E, F, K, Wt != nullptr) * sizeof(float);
    if (lds > kSsLdsBytes) {
        set_error("rbr_siamese_saliency: R=%d E=%d F=%d K=%d needs more LDS than the %zu bytes a workgroup may have", R, E, F, K,
                  kSsLdsBytes);
        return RBR_ERR_UNSUPPORTED;
    }
    const bool vec4 = (E % 4 == 0) && ((((uintptr_t)table) & 15) == 0);      // as bag_fwd_kernel decides it
    const int ncol = vec4 ? E / 4 : E;
    int G = 1;
    while (G < ncol && G < kWave) G <<= 1;
    const SsArgs A{n, R, T, E, F, K, G, V, table, reinterpret_cast<const long long*>(ids), word_mask, rev_mask, y, a, g, Wt,
                   Wp, bp, wi, fixed, through, reviews};
    if (vec4)
        hipLaunchKernelGGL(siamese_saliency_kernel<true>, dim3((unsigned)n), dim3(kSsThreads), lds, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(siamese_saliency_kernel<false>, dim3((unsigned)n), dim3(kSsThreads), lds, (hipStream_t)stream, A);
    RBR_CHECK_LAUNCH("siamese saliency launch");
    return 0;
}
