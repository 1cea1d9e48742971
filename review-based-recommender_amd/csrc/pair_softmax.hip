// pair_softmax.hip -- in-batch softmax ranking loss over ALL B x B pairs of a batch's user and item latents, with its backward
// (rbr_pair_softmax_* of include/rbr_hip.h).  Every tower depends on its own side only, so the B item latents of a batch are
// B - 1 candidate negatives for every user of the batch at no encoder cost; what is pair-dependent -- the FM / dot score of
// (u_a, i_b), the head's dropout draw for (a, b, k), the false-negative test against the seen-items CSR, the row softmax and
// the chain rule back to the latents -- is these two launches.  The reference trains for rating regression only.
//
//   launch 1, row-owned (one workgroup per user row a): scores z[a, :] into LDS (8 groups of 32 lanes: a group takes a column,
//     its lanes the K products; xor-shuffle sum), the mask (ids compared, a binary search of the user's seen row), the
//     max-subtracted row softmax, ds[a, :] = d loss / d s[a, :] into the workspace, the row's loss term, and -- the row still in
//     LDS -- d_ul[a, :] and the row's partial of d_h.
//   launch 2, column-owned: a workgroup takes a strip of 64 columns (a wave's loads of ds are 256 contiguous bytes) and one
//     latent dimension; its four waves split the rows and meet in LDS in a fixed order: d_il[b, k], d_col_bias[b].  The
//     workgroups behind the strips sum the row losses and the d_h partials in index order; the last workgroup to finish
//     advances the dropout call number (both launches have read it by then).
//
// No float atomics; every output element has one owner that adds its terms in a fixed order: the same bits on every run.
#include "rbr_common.h"
#include "item_csr.h"

#include <cmath>

namespace rbr {

constexpr int kPsMaxB = 4096;
constexpr int kPsMaxK = 256;

struct PairSoftmax {
    const float *ul, *il, *h, *row_bias, *col_bias, *drop, *logq, *d_loss;
    const long long *u_id, *i_id;
    ItemCsr seen;                       // row u: the items user u has rated (item_csr.h)
    long long item_lo;
    const unsigned long long* call;     // call number of the in-kernel draw (rng_state, or the forward's saved one); NULL: none
    unsigned long long* rng_state;      // non-NULL: launch 2 advances the call number
    unsigned long long* call_out;       // the call number this call drew with (for rbr_pair_softmax_bwd)
    unsigned long long seed;
    float p_drop, inv_temp;
    float *loss, *pos, *d_ul, *d_il, *d_h, *d_col_bias, *d_row_bias;
    float *ds, *row_loss, *dh_part;     // workspace: [B, B], [B], [B, K]
    int mode, B, K, grads, col_blocks;
};

// the head's dropout multiplier of element e = (a * B + b) * K + k: the explicit one, or the draw rbr_dropout_multiplier makes
// for element e of call `call` (rbr_rng.h)
__device__ __forceinline__ float ps_mult(const PairSoftmax& S, unsigned long long call, long long e) {
    if (S.drop != nullptr) return S.drop[e];
    return S.p_drop > 0.f ? dropout_draw((unsigned long long)e, call, S.seed, S.p_drop) : 1.f;
}

// sum / max over the 256 threads in a fixed order (xor-shuffle tree over 64 lanes, then the four wave results in order);
// every thread gets the result.  s_w: 4 floats of LDS, free to be reused after the call returns.
__device__ __forceinline__ float ps_block_sum(float v, float* s_w) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
__device__ __forceinline__ float ps_block_max(float v, float* s_w) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_w[0], s_w[1]), fmaxf(s_w[2], s_w[3]));
}

__global__ __launch_bounds__(256) void pair_softmax_rows_kernel(const PairSoftmax S) {
    __shared__ float s_z[kPsMaxB];          // z[a, :], later ds[a, :]
    __shared__ float s_u[kPsMaxK];          // ul[a, :]
    __shared__ float s_red[2][8][32];
    __shared__ float s_w[4];
    const int a = blockIdx.x, t = threadIdx.x, g = t >> 5, kk = t & 31, B = S.B, K = S.K;
    const bool fm = S.mode == RBR_SCORE_FM;
    const unsigned long long call = S.call != nullptr ? S.call[0] : 0ull;
    for (int k = t; k < K; k += 256) s_u[k] = S.ul[(long)a * K + k];
    const long long ia = S.i_id[a];
    long long sa, se;                       // the user's seen row
    csr_row(S.seen, S.u_id[a], sa, se);
    const float rb = S.row_bias != nullptr ? S.row_bias[a] : 0.f;
    __syncthreads();

    for (int b = g; b < B; b += 8) {
        const float* x = S.il + (long)b * K;
        const long long e0 = ((long long)a * B + b) * K;
        float acc = 0.f;
        for (int k = kk; k < K; k += 32) {
            const float u = s_u[k], v = x[k];
            if (fm) {
                const float pr = u * v;
                float zr = (pr < 0.f) ? 0.f : pr;       // not fmaxf: relu(NaN) stays NaN, as in the head
                zr *= ps_mult(S, call, e0 + k);
                acc = fmaf(zr, S.h[k], acc);
            } else {
                acc = fmaf(u, v, acc);
            }
        }
        acc = wave_sum<32>(acc);
        if (kk == 0) {
            float s = acc;
            if (S.row_bias != nullptr) s += rb;
            if (S.col_bias != nullptr) s += S.col_bias[b];
            if (b == a) S.pos[a] = s;
            float z = S.inv_temp * s;
            if (S.logq != nullptr) z -= S.logq[b];
            bool ok = b == a;
            if (!ok) {
                const long long ib = S.i_id[b];
                ok = ib >= S.item_lo && ib != ia && !csr_has(S.seen.item, sa, se, ib);
            }
            s_z[b] = ok ? z : -INFINITY;
        }
    }
    __syncthreads();

    float m = -INFINITY;
    for (int b = t; b < B; b += 256) m = fmaxf(m, s_z[b]);
    m = ps_block_max(m, s_w);
    float part = 0.f;
    for (int b = t; b < B; b += 256) {
        const float z = s_z[b];
        part += (z == -INFINITY) ? 0.f : expf(z - m);
    }
    const float zaa = s_z[a];
    const float sum = ps_block_sum(part, s_w);
    if (t == 0) {
        S.row_loss[a] = (m + logf(sum)) - zaa;       // a row alone with its own column: sum = 1, m = zaa: exactly 0
        if (S.d_row_bias != nullptr) S.d_row_bias[a] = 0.f;       // a per-user constant cancels in a softmax over items: DEFINED as 0
    }
    if (!S.grads) return;

    const float scale = S.inv_temp / (float)B * (S.d_loss != nullptr ? S.d_loss[0] : 1.f);
    for (int b = t; b < B; b += 256) {       // every thread rewrites the elements it read above
        const float z = s_z[b];
        const float P = (z == -INFINITY) ? 0.f : expf(z - m) / sum;
        const float d = (P - (b == a ? 1.f : 0.f)) * scale;
        s_z[b] = d;
        S.ds[(long)a * B + b] = d;
    }
    __syncthreads();

    for (int k0 = 0; k0 < K; k0 += 32) {
        const int k = k0 + kk;
        float au = 0.f, ah = 0.f;
        if (k < K) {
            const float u = s_u[k], hk = fm ? S.h[k] : 0.f;
            for (int b = g; b < B; b += 8) {
                const float d = s_z[b];
                const float v = S.il[(long)b * K + k];
                if (fm) {
                    const float pr = u * v;
                    if (pr > 0.f) {
                        const float mm = ps_mult(S, call, ((long long)a * B + b) * K + k);
                        au = fmaf(d, mm * hk * v, au);
                        ah = fmaf(d, pr * mm, ah);
                    }
                } else {
                    au = fmaf(d, v, au);
                }
            }
        }
        s_red[0][g][kk] = au;
        s_red[1][g][kk] = ah;
        __syncthreads();
        if (g < 2 && k < K) {
            const float (*r)[32] = s_red[g];
            const float tot = ((r[0][kk] + r[1][kk]) + (r[2][kk] + r[3][kk])) + ((r[4][kk] + r[5][kk]) + (r[6][kk] + r[7][kk]));
            if (g == 0) S.d_ul[(long)a * K + k] = tot;
            else if (fm) S.dh_part[(long)a * K + k] = tot;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pair_softmax_cols_kernel(const PairSoftmax S) {
    __shared__ float s_part[4][2][64];
    __shared__ float s_red[8][32];
    __shared__ float s_w[4];
    const int t = threadIdx.x, B = S.B, K = S.K;
    const bool fm = S.mode == RBR_SCORE_FM;
    const unsigned long long call = S.call != nullptr ? S.call[0] : 0ull;
    if ((int)blockIdx.x < S.col_blocks) {
        const int strip = blockIdx.x / K, k = blockIdx.x % K;
        const int lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), b = strip * 64 + lane;
        float acc = 0.f, accb = 0.f;
        if (b < B) {
            const float v = S.il[(long)b * K + k], hk = fm ? S.h[k] : 0.f;
            for (int a = w; a < B; a += 4) {
                const float d = S.ds[(long)a * B + b];
                const float u = S.ul[(long)a * K + k];
                accb += d;
                if (fm) {
                    const float pr = u * v;
                    if (pr > 0.f) {
                        const float mm = ps_mult(S, call, ((long long)a * B + b) * K + k);
                        acc = fmaf(d, mm * hk * u, acc);
                    }
                } else {
                    acc = fmaf(d, u, acc);
                }
            }
        }
        s_part[w][0][lane] = acc;
        s_part[w][1][lane] = accb;
        __syncthreads();
        if (w == 0 && b < B) {
            S.d_il[(long)b * K + k] = (s_part[0][0][lane] + s_part[1][0][lane]) + (s_part[2][0][lane] + s_part[3][0][lane]);
            if (k == 0 && S.d_col_bias != nullptr)
                S.d_col_bias[b] = (s_part[0][1][lane] + s_part[1][1][lane]) + (s_part[2][1][lane] + s_part[3][1][lane]);
        }
    } else {
        const int x = (int)blockIdx.x - S.col_blocks;       // behind the strips: x == 0 sums the loss, each x a 32-wide chunk of d_h
        if (x == 0) {
            if (S.loss != nullptr) {
                float acc = 0.f;
                for (int a = t; a < B; a += 256) acc += S.row_loss[a];
                const float tot = ps_block_sum(acc, s_w);
                if (t == 0) S.loss[0] = tot / (float)B;
            }
            if (t == 0 && S.call_out != nullptr) S.call_out[0] = call;
        }
        if (S.grads && fm) {
            const int g = t >> 5, kk = t & 31, k = x * 32 + kk;
            float acc = 0.f;
            if (k < K)
                for (int a = g; a < B; a += 8) acc += S.dh_part[(long)a * K + k];
            s_red[g][kk] = acc;
            __syncthreads();
            if (g == 0 && k < K)
                S.d_h[k] = ((s_red[0][kk] + s_red[1][kk]) + (s_red[2][kk] + s_red[3][kk])) +
                           ((s_red[4][kk] + s_red[5][kk]) + (s_red[6][kk] + s_red[7][kk]));
        }
    }
    if (S.rng_state != nullptr) {       // the last workgroup to finish advances the call number: every one has read it
        __syncthreads();
        if (t == 0) rng_advance_call(S.rng_state, call);
    }
}

static size_t ps_align(size_t n) { return (n + 255) & ~(size_t)255; }

static bool ps_supported(int B, int K) { return B >= 1 && B <= kPsMaxB && K >= 1 && K <= kPsMaxK; }

// argument checks shared by the two entries; 0 or an error code, before any launch
static int ps_check(const char* who, int mode, int B, int K, const float* ul, const float* il, const float* h, const float* drop,
                    float p_drop, const void* rng, const long long* u_id, const long long* i_id, const long long* seen_off,
                    const int* seen_item, long long seen_nnz, int U, float inv_temp, const void* ws) {
    if (mode != RBR_SCORE_FM && mode != RBR_SCORE_DOT) { set_error("%s: unknown score mode %d", who, mode); return RBR_ERR_BAD_ARG; }
    if (B <= 0 || K <= 0) { set_error("%s: bad shape B=%d K=%d", who, B, K); return RBR_ERR_BAD_ARG; }
    if (!ps_supported(B, K)) {
        set_error("%s: B=%d K=%d outside the supported range 1 <= B <= %d, 1 <= K <= %d (there is no fallback)", who, B, K, kPsMaxB, kPsMaxK);
        return RBR_ERR_UNSUPPORTED;
    }
    if (!ul || !il || !u_id || !i_id || !ws) { set_error("%s: null pointer", who); return RBR_ERR_BAD_ARG; }
    if (mode == RBR_SCORE_FM && !h) { set_error("%s: the fm score needs h [K]", who); return RBR_ERR_BAD_ARG; }
    if (!(inv_temp > 0.f) || !std::isfinite(inv_temp)) { set_error("%s: inv_temp=%f must be positive and finite", who, (double)inv_temp); return RBR_ERR_BAD_ARG; }
    if (!(p_drop >= 0.f && p_drop < 1.f)) { set_error("%s: p_drop=%f outside [0,1)", who, (double)p_drop); return RBR_ERR_BAD_ARG; }
    if (drop && p_drop > 0.f) { set_error("%s: an explicit drop multiplier AND p_drop > 0: one of them", who); return RBR_ERR_BAD_ARG; }
    if (mode == RBR_SCORE_DOT && (drop || p_drop > 0.f)) { set_error("%s: the dot score has no dropout", who); return RBR_ERR_BAD_ARG; }
    if (p_drop > 0.f && !rng) { set_error("%s: p_drop > 0 needs the call number in device memory", who); return RBR_ERR_BAD_ARG; }
    return item_csr_ok(who, true, seen_off, seen_item, seen_nnz, nullptr, U);
}

static int ps_run(PairSoftmax& S, void* ws, hipStream_t st, const char* who) {
    const int B = S.B, K = S.K;
    char* p = static_cast<char*>(ws);
    S.ds = reinterpret_cast<float*>(p); p += ps_align(sizeof(float) * (size_t)B * B);
    S.row_loss = reinterpret_cast<float*>(p); p += ps_align(sizeof(float) * (size_t)B);
    S.dh_part = reinterpret_cast<float*>(p);
    S.col_blocks = S.grads ? ((B + 63) / 64) * K : 0;       // (strip of 64 columns, latent dimension) per workgroup: <= 64 * 256
    const int extra = (S.grads && S.mode == RBR_SCORE_FM) ? (K + 31) / 32 : 1;
    hipLaunchKernelGGL(pair_softmax_rows_kernel, dim3(B), dim3(256), 0, st, S);
    if (int e = check_hip(hipGetLastError(), who)) return e;
    hipLaunchKernelGGL(pair_softmax_cols_kernel, dim3(S.col_blocks + extra), dim3(256), 0, st, S);
    RBR_CHECK_LAUNCH(who);
    return 0;
}

}  // namespace rbr

extern "C" size_t rbr_pair_softmax_ws_bytes(int32_t B, int32_t K) {
    using namespace rbr;
    if (!ps_supported(B, K)) return 0;
    return ps_align(sizeof(float) * (size_t)B * B) + ps_align(sizeof(float) * (size_t)B) + ps_align(sizeof(float) * (size_t)B * K);
}

extern "C" int rbr_pair_softmax_fwd(int32_t mode, int32_t B, int32_t K, const float* ul, const float* il, const float* h,
                                    const float* row_bias, const float* col_bias, const float* drop, float p_drop, uint64_t seed,
                                    uint64_t* rng_state, const int64_t* u_id, const int64_t* i_id, const int64_t* seen_off,
                                    const int32_t* seen_item, int64_t seen_nnz, int32_t U, int64_t item_lo, const float* logq,
                                    float inv_temp, float* loss, float* pos, float* d_ul, float* d_il, float* d_h, float* d_col_bias,
                                    float* d_row_bias, uint64_t* call_out, void* ws, void* stream) {
    using namespace rbr;
    const char* who = "rbr_pair_softmax_fwd";
    if (int e = ps_check(who, mode, B, K, ul, il, h, drop, p_drop, rng_state, reinterpret_cast<const long long*>(u_id),
                         reinterpret_cast<const long long*>(i_id), reinterpret_cast<const long long*>(seen_off), seen_item, seen_nnz, U,
                         inv_temp, ws))
        return e;
    if (!loss || !pos) { set_error("%s: null pointer (loss, pos)", who); return RBR_ERR_BAD_ARG; }
    const bool grads = d_ul != nullptr || d_il != nullptr || d_h != nullptr || d_col_bias != nullptr;
    if (grads && (!d_ul || !d_il || (mode == RBR_SCORE_FM && !d_h) || ((col_bias != nullptr) != (d_col_bias != nullptr)))) {
        set_error("%s: the unit-root gradients come together: d_ul, d_il, d_h (fm) and d_col_bias exactly when col_bias is given", who);
        return RBR_ERR_BAD_ARG;
    }
    PairSoftmax S{};
    S.ul = ul; S.il = il; S.h = h; S.row_bias = row_bias; S.col_bias = col_bias; S.drop = drop; S.logq = logq; S.d_loss = nullptr;
    S.u_id = reinterpret_cast<const long long*>(u_id); S.i_id = reinterpret_cast<const long long*>(i_id);
    S.seen = item_csr(seen_off, seen_item, nullptr, seen_nnz, U); S.item_lo = item_lo;
    S.rng_state = p_drop > 0.f ? reinterpret_cast<unsigned long long*>(rng_state) : nullptr;
    S.call = S.rng_state;
    S.call_out = reinterpret_cast<unsigned long long*>(call_out);
    S.seed = seed; S.p_drop = p_drop; S.inv_temp = inv_temp;
    S.loss = loss; S.pos = pos; S.d_ul = d_ul; S.d_il = d_il; S.d_h = d_h; S.d_col_bias = d_col_bias; S.d_row_bias = d_row_bias;
    S.mode = mode; S.B = B; S.K = K; S.grads = grads ? 1 : 0;
    return ps_run(S, ws, (hipStream_t)stream, who);
}

extern "C" int rbr_pair_softmax_bwd(int32_t mode, int32_t B, int32_t K, const float* ul, const float* il, const float* h,
                                    const float* row_bias, const float* col_bias, const float* drop, float p_drop, uint64_t seed,
                                    const uint64_t* call, const int64_t* u_id, const int64_t* i_id, const int64_t* seen_off,
                                    const int32_t* seen_item, int64_t seen_nnz, int32_t U, int64_t item_lo, const float* logq,
                                    float inv_temp, const float* d_loss, float* pos_scratch, float* d_ul, float* d_il, float* d_h,
                                    float* d_col_bias, float* d_row_bias, void* ws, void* stream) {
    using namespace rbr;
    const char* who = "rbr_pair_softmax_bwd";
    if (int e = ps_check(who, mode, B, K, ul, il, h, drop, p_drop, call, reinterpret_cast<const long long*>(u_id),
                         reinterpret_cast<const long long*>(i_id), reinterpret_cast<const long long*>(seen_off), seen_item, seen_nnz, U,
                         inv_temp, ws))
        return e;
    if (!d_loss || !pos_scratch || !d_ul || !d_il || (mode == RBR_SCORE_FM && !d_h) || ((col_bias != nullptr) != (d_col_bias != nullptr))) {
        set_error("%s: null pointer (d_loss, pos_scratch, d_ul, d_il, d_h for fm; d_col_bias exactly when col_bias is given)", who);
        return RBR_ERR_BAD_ARG;
    }
    PairSoftmax S{};
    S.ul = ul; S.il = il; S.h = h; S.row_bias = row_bias; S.col_bias = col_bias; S.drop = drop; S.logq = logq; S.d_loss = d_loss;
    S.u_id = reinterpret_cast<const long long*>(u_id); S.i_id = reinterpret_cast<const long long*>(i_id);
    S.seen = item_csr(seen_off, seen_item, nullptr, seen_nnz, U); S.item_lo = item_lo;
    S.rng_state = nullptr;       // the forward advanced the call number; this launch re-draws the forward's set from the saved one
    S.call = p_drop > 0.f ? reinterpret_cast<const unsigned long long*>(call) : nullptr;
    S.call_out = nullptr;
    S.seed = seed; S.p_drop = p_drop; S.inv_temp = inv_temp;
    S.loss = nullptr; S.pos = pos_scratch; S.d_ul = d_ul; S.d_il = d_il; S.d_h = d_h; S.d_col_bias = d_col_bias; S.d_row_bias = d_row_bias;
    S.mode = mode; S.B = B; S.K = K; S.grads = 1;
    return ps_run(S, ws, (hipStream_t)stream, who);
}
