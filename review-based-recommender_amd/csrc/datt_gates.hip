// datt_gates.hip -- D-ATT attention gates (forward and backward).
//
// Replaces the `attn` branches of models/dual_att/layers.py:
//   LocalAttention  (layers.py:34-36,50): gate[b,l] = sigmoid(conv1d(E -> 1, win, pad (win-1)/2)(x)[b,l])
//   GlobalAttention (layers.py:65-67,84): gate[b,:] = sigmoid(conv1d(E -> 1, kernel = doc_len)(x)[b])
// with x = table[ids] (D-ATT has no masks: pad tokens read the table's pad row).  The products
// `score * x` (layers.py:51,85) are never materialised: the gate vector is handed to the fused conv
// kernel, which scales the token rows while gathering them (csrc/textcnn_fwd.hip, `gate`).
// One output channel => no GEMM shape; these are HBM/L2-bound row dot products on the VALU.
#include "rbr_common.h"
#include "lds_bucket.h"

#include <algorithm>

namespace rbr {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
typedef float f32x4g __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------- local gate
// One workgroup per (document, tile of 64 tokens): the 64 + win - 1 token rows are staged ONCE in LDS (each row is
// needed by `win` neighbouring tokens), then every wave reduces 16 tokens: lanes stride the embedding dim, win taps
// per lane, shuffle reduction.  w is the Conv1d weight [1, E, win].
constexpr int kGTile = 64;

__global__ __launch_bounds__(256) void local_gate_fwd_kernel(int B, int L, int E, int win, int ntile,
                                                             const long long* __restrict__ ids,
                                                             const float* __restrict__ table, const float* __restrict__ w,
                                                             const float* __restrict__ b0, float* __restrict__ gate) {
    extern __shared__ float s_rows[];                  // [kGTile + win - 1][E]
    __shared__ long s_off[kGTile + 2 * kMaxKF + 2];
    const int b = blockIdx.x / ntile, l0 = (blockIdx.x % ntile) * kGTile;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int pad = (win - 1) / 2, R = kGTile + win - 1;
    for (int r = tid; r < R; r += 256) {
        const int p = l0 - pad + r;
        s_off[r] = (p >= 0 && p < L) ? ids[(long)b * L + p] * (long)E : -1;     // zero padding outside the document
    }
    __syncthreads();
    for (int idx = tid; idx < R * E; idx += 256) {
        const int r = idx / E, e = idx - r * E;
        const long o = s_off[r];
        s_rows[idx] = (o >= 0) ? table[o + e] : 0.f;
    }
    __syncthreads();
    const float bias = b0[0];
    for (int t = wave; t < kGTile; t += 4) {
        if (l0 + t >= L) break;
        float s = 0.f;
        for (int e = lane; e < E; e += 64)
            for (int j = 0; j < win; ++j) s = fmaf(s_rows[(t + j) * E + e], w[(long)e * win + j], s);
        s = wave_sum(s);
        if (lane == 0) gate[(long)b * L + l0 + t] = sigmoidf_(s + bias);
    }
}

// ---- token-folded embedding gradient of a gate -----------------------------------------------------------
// dtable[id, :] += sum over the positions p of the window that carry token `id` of  row_p[:], with
//   local : row_p[e] = sum_j dpre[b, p - j + pad] * w[e, j]   ==>  sum_p row_p[e] = sum_j c_j * w[e, j],
//           c_j = sum_p dpre[b, p - j + pad]                        (win scalars per token)
//   global: row_p[e] = dpre[b] * w[e, p]                        ==>  dpre[b] * sum_p wT[p, e]
// One workgroup per (document, window of <= 256 positions): positions are bucketed by token through an LDS
// hash table, one wave per distinct token builds the folded row and issues ONE row of contiguous f32 atomics
// (a per-token atomic row for each of the 1 M tokens of cfg4 ran 1.3 ms: Zipf-hot rows serialise).
constexpr int kGWin = 256, kGHash = 1024;
constexpr int kGateWP = 8;       // floats per token row of the tap tables S / c of the token-product local gate (win <= 8)
constexpr int kGateCopies = 16;  // private copies of the tap-sum table c (summed by gp_csum_kernel)

__device__ __forceinline__ void gate_bwd_dx_kernel(int B, int L, int E, int win, int is_global, int nwin,
                                                          const long long* __restrict__ ids, const float* __restrict__ w,
                                                          const float* __restrict__ wT, const float* __restrict__ gate,
                                                          const float* __restrict__ dgate, const float* __restrict__ dpre_g,
                                                          int pad_idx, float* __restrict__ dtable,
                                                          const int* __restrict__ row_of_token, float* __restrict__ c_out,
                                                          long c_stride) {
    __shared__ int s_tok[kGWin];
    __shared__ short s_leader[kGWin], s_cnt[kGWin], s_start[kGWin], s_sorted[kGWin];
    __shared__ int s_fill[kGWin];                    // positions per leader (counted with LDS atomics: integers, any order)
    __shared__ int s_hkey[kGHash], s_hval[kGHash];
    __shared__ float s_dpre[kGWin + 2 * kMaxKF];     // local: dpre of the window plus a halo of `pad` each side
    __shared__ short s_keys[kGWin];                  // the leaders (first position of each distinct token), dense
    __shared__ int s_nkeys;
    extern __shared__ float s_cj[];                  // dense local mode: [kGWin][win] tap sums per distinct token
    const int b = blockIdx.x / nwin, p0 = (blockIdx.x % nwin) * kGWin;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int pad = (win - 1) / 2;
    const int nrow = min(kGWin, L - p0);

    bucket_hash_clear<kGHash>(s_hkey, s_hval);
    for (int r = tid; r < kGWin; r += 256) {
        int t = -1;
        // c_out mode keeps the pad token: its row feeds the weight gradient (only its TABLE row gets no gradient)
        if (r < nrow) { t = (int)ids[(long)b * L + p0 + r]; if (t == pad_idx && c_out == nullptr) t = -1; }
        s_tok[r] = t;
        s_fill[r] = 0;
    }
    if (!is_global) {
        for (int k = tid; k < kGWin + 2 * pad; k += 256) {
            const int l = p0 - pad + k;
            float v = 0.f;
            if (l >= 0 && l < L) { const float gv = gate[(long)b * L + l]; v = dgate[(long)b * L + l] * gv * (1.f - gv); }
            s_dpre[k] = v;
        }
    }
    __syncthreads();
    // positions by token (lds_bucket.h): per-token counts and the dense key list
    bucket_leaders<kGHash, false, true>(s_tok, kGWin, s_hkey, s_hval, s_leader, s_fill);
    __syncthreads();
    if (wave == 0) bucket_scan<true, false>(lane, s_fill, kGWin, s_start, s_cnt, s_keys, &s_nkeys);
    __syncthreads();
    // a token's positions in ASCENDING order (an atomic fill left them in arrival order: the tap sums below rounded differently
    // from run to run).  Up to 255 LDS reads for the last position of a window that holds one token, where the atomic fill took
    // one.  Not measured in isolation; the whole backward of the token-product gate at the cfg4 tower shape (512 x 1024 Zipf ids,
    // V = 50 k) went from 96 to 101 us with it, the row maps (rbr_datt_token_rows) from 21.6 to 15.8 us without the contended counter
    bucket_place_ordered(s_leader, kGWin, s_start, s_sorted);
    __syncthreads();
    // The folded rows leave the workgroup thread-parallel: a wave per token walked <= 64 tokens one after the other, each
    // with a dependent L2 read in front of its atomics (latency-bound: 88 us for the tap sums alone at cfg4).
    const int nkeys = s_nkeys;
    if (c_out != nullptr) {
        // token-product backward of the local gate: only the win tap sums c_j of the token leave the workgroup.  8 lanes
        // per token (one per tap), so that a token's row is ONE 32-byte atomic request; the workgroup adds into copy
        // blockIdx % kGateCopies of the tap-sum table: requests to the same line are served one after the other, and the row
        // of a Zipf-hot token would otherwise receive one from every window of every document.
        float* mine = c_out + (long)(blockIdx.x % kGateCopies) * c_stride;
        const int j = tid & (kGateWP - 1);
        for (int k = tid / kGateWP; k < nkeys; k += 256 / kGateWP) {
            const int key = s_keys[k], cnt = s_cnt[key], base = s_start[key];
            const int row = row_of_token[s_tok[key]];
            if (row < 0 || j >= win) continue;
            float cj = 0.f;
            for (int q = 0; q < cnt; ++q) cj += s_dpre[s_sorted[base + q] - j + 2 * pad];
            atomicAdd(mine + (long)row * kGateWP + j, cj);
        }
        return;
    }
    if (!is_global) {
        // the win tap sums of every token of the window, once, into LDS
        for (int k = tid; k < nkeys; k += 256) {
            const int key = s_keys[k], cnt = s_cnt[key], base = s_start[key];
            for (int j = 0; j < win; ++j) {
                float c = 0.f;
                for (int q = 0; q < cnt; ++q) c += s_dpre[s_sorted[base + q] - j + 2 * pad];
                s_cj[k * win + j] = c;
            }
        }
        __syncthreads();
    }
    const float dp = is_global ? dpre_g[b] : 0.f;
    const int total = nkeys * E;
    constexpr int kU = 4;                            // rows in flight per thread: the reads of 4 items before the first atomic
    for (int it = tid; it < total; it += 256 * kU) {
        float s[kU];
        float* dst[kU];
        int cnt[kU], base[kU], ee[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int item = it + u * 256;
            const bool ok = item < total;
            const int k = ok ? item / E : 0, e = ok ? item - k * E : 0;
            const int key = s_keys[k];
            cnt[u] = ok ? s_cnt[key] : 0;
            base[u] = s_start[key];
            ee[u] = e;
            dst[u] = dtable + (long)s_tok[key] * E + e;
            if (is_global) {
                s[u] = ok ? wT[(long)(p0 + s_sorted[base[u]]) * E + e] : 0.f;
            } else {
                float a = 0.f;
                for (int j = 0; j < win; ++j) a = fmaf(s_cj[k * win + j], w[(long)e * win + j], a);
                s[u] = a;
            }
        }
        if (is_global) {
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                for (int q = 1; q < cnt[u]; ++q) s[u] += wT[(long)(p0 + s_sorted[base[u] + q]) * E + ee[u]];
                s[u] *= dp;
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (cnt[u] > 0) atomicAdd(dst[u], s[u]);
    }
}

// wT[l, e] = w[e, l]   (global gate: coalesced reads of the per-position weight columns)
__device__ __forceinline__ void transpose_w_kernel(int E, int L, const float* __restrict__ w, float* __restrict__ wT) {
    const long n = (long)E * L;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const int l = (int)(k / E), e = (int)(k % E);
        wT[k] = w[(long)e * L + l];
    }
}

// per-document partial of dw[e, j] = sum_p x[b,p,e] * dpre[b, p - j + pad] and of db0.  The document is walked in
// tiles of 64 tokens staged in LDS; thread (e, half) owns column e for 32 tokens of each tile and keeps the win
// partial sums in registers; the two halves meet in LDS at the end.
__global__ __launch_bounds__(256) void local_gate_bwd_dw_kernel(int B, int L, int E, int win,
                                                                const long long* __restrict__ ids, const float* __restrict__ table,
                                                                const float* __restrict__ gate, const float* __restrict__ dgate,
                                                                float* __restrict__ ws /* [B][win*E + 1] */) {
    extern __shared__ float sm[];                      // dpre [L + 2*pad] | rows [kGTile][E]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pad = (win - 1) / 2;
    float* s_dpre = sm;                                // index l + pad; zero halo
    float* s_rows = sm + L + 2 * pad;
    __shared__ long s_off[kGTile];
    __shared__ float s_red[256];
    float part = 0.f;
    for (int k = tid; k < L + 2 * pad; k += 256) {
        const int l = k - pad;
        float v = 0.f;
        if (l >= 0 && l < L) {
            const float gv = gate[(long)b * L + l];
            v = dgate[(long)b * L + l] * gv * (1.f - gv);
            part += v;
        }
        s_dpre[k] = v;
    }
    s_red[tid] = part;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int k = 0; k < 256; ++k) t += s_red[k];
        ws[(long)b * (win * E + 1) + win * E] = t;
    }
    const int half = tid >> 7, e0 = tid & 127;          // two halves x 128 column lanes
    for (int ebase = 0; ebase < E; ebase += 128) {
        const int e = ebase + e0;
        for (int j0 = 0; j0 < win; j0 += kMaxKF) {
            float acc[kMaxKF];
#pragma unroll
            for (int j = 0; j < kMaxKF; ++j) acc[j] = 0.f;
            for (int l0 = 0; l0 < L; l0 += kGTile) {
                __syncthreads();
                if (tid < kGTile) s_off[tid] = (l0 + tid < L) ? ids[(long)b * L + l0 + tid] * (long)E : -1;
                __syncthreads();
                for (int idx = tid; idx < kGTile * E; idx += 256) {
                    const int r = idx / E, ee = idx - r * E;
                    const long o = s_off[r];
                    s_rows[idx] = (o >= 0) ? table[o + ee] : 0.f;
                }
                __syncthreads();
                if (e < E) {
                    for (int t = half * 32; t < half * 32 + 32; ++t) {
                        const float x = s_rows[t * E + e];
                        const int p = l0 + t;
#pragma unroll
                        for (int j = 0; j < kMaxKF; ++j)
                            if (j0 + j < win) acc[j] = fmaf(x, s_dpre[p - (j0 + j) + 2 * pad], acc[j]);
                    }
                }
            }
            // combine the two halves (fixed order) and store
            __syncthreads();
            float* s_acc = s_rows;                                // reuse: [2][kMaxKF][128]
#pragma unroll
            for (int j = 0; j < kMaxKF; ++j) s_acc[(half * kMaxKF + j) * 128 + e0] = acc[j];
            __syncthreads();
            if (half == 0 && e < E) {
#pragma unroll
                for (int j = 0; j < kMaxKF; ++j)
                    if (j0 + j < win)
                        ws[(long)b * (win * E + 1) + (long)(j0 + j) * E + e] = s_acc[j * 128 + e0] + s_acc[(kMaxKF + j) * 128 + e0];
            }
        }
    }
}

// dw[e*win + j] = sum_b ws[b][j*E + e];  db0 = sum_b ws[b][win*E]   (fixed partition and order).
// One workgroup per 32 outputs: 8 thread groups stride the documents.
__global__ __launch_bounds__(256) void local_gate_bwd_reduce_kernel(int B, int E, int win, const float* __restrict__ ws,
                                                                    float* __restrict__ dw, float* __restrict__ db0) {
    __shared__ float red[8][32];
    const int n = win * E + 1;
    const int kk = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int idx = blockIdx.x * 32 + kk;
    float s = 0.f;
    if (idx < n)
        for (int b = grp; b < B; b += 8) s += ws[(long)b * n + idx];
    red[grp][kk] = s;
    __syncthreads();
    if (grp == 0 && idx < n) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[q][kk];
        if (idx == win * E) db0[0] = t;
        else { const int j = idx / E, e = idx - j * E; dw[(long)e * win + j] = t; }
    }
}

// ---------------------------------------------------------------------------------- global gate
// one workgroup per document: thread l walks its token's row; w is the Conv1d weight [1, E, L]
__device__ __forceinline__ void global_gate_fwd_kernel(int B, int L, int E, const long long* __restrict__ ids,
                                                              const float* __restrict__ table, const float* __restrict__ w,
                                                              const float* __restrict__ b0, float* __restrict__ gate) {
    __shared__ float s_red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool vec = (E % 4 == 0) && ((((uintptr_t)table) & 15) == 0);
    float part = 0.f;
    for (int l = tid; l < L; l += 256) {
        const float* row = table + ids[(long)b * L + l] * (long)E;
        float s = 0.f;
        if (vec) {      // the thread's own row in 16-byte pieces (a quarter of the cache-line touches); w coalesced across threads
            int e = 0;
            for (; e + 16 <= E; e += 16) {      // 4 row quads and their 16 weight scalars requested before the first use
                f32x4g x[4];
                float wv[16];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4g*>(row + e + 4 * u);
#pragma unroll
                for (int u = 0; u < 16; ++u) wv[u] = w[(long)(e + u) * L + l];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s = fmaf(x[u].x, wv[4 * u], s); s = fmaf(x[u].y, wv[4 * u + 1], s);
                    s = fmaf(x[u].z, wv[4 * u + 2], s); s = fmaf(x[u].w, wv[4 * u + 3], s);
                }
            }
            for (; e < E; e += 4) {
                const f32x4g x = *reinterpret_cast<const f32x4g*>(row + e);
                s = fmaf(x.x, w[(long)e * L + l], s);
                s = fmaf(x.y, w[(long)(e + 1) * L + l], s);
                s = fmaf(x.z, w[(long)(e + 2) * L + l], s);
                s = fmaf(x.w, w[(long)(e + 3) * L + l], s);
            }
        } else {
            for (int e = 0; e < E; ++e) s = fmaf(row[e], w[(long)e * L + l], s);   // w reads coalesced across threads
        }
        part += s;
    }
    s_red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    const float g = sigmoidf_(s_red[0] + b0[0]);
    for (int l = tid; l < L; l += 256) gate[(long)b * L + l] = g;   // broadcast: the conv kernel takes a per-token gate
}

// dpre[b] = (sum_l dgate[b,l]) * g (1-g)
__device__ __forceinline__ void global_gate_bwd_dpre_kernel(int B, int L, const float* __restrict__ gate,
                                                                   const float* __restrict__ dgate, float* __restrict__ dpre) {
    __shared__ float s_red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float part = 0.f;
    for (int l = tid; l < L; l += 256) part += dgate[(long)b * L + l];
    s_red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) { const float g = gate[(long)b * L]; dpre[b] = s_red[0] * g * (1.f - g); }
}

// dw[e, l] = sum_b dpre[b] * x[b,l,e]  (one workgroup per position l);  block L computes db0.  The 256 threads split
// into document classes x embedding columns (E = 100: two classes), 8 independent row reads in flight per thread; the
// classes meet in LDS in fixed order.
__device__ __forceinline__ void global_gate_bwd_dw_kernel(int B, int L, int E, const long long* __restrict__ ids,
                                                                 const float* __restrict__ table, const float* __restrict__ dpre,
                                                                 float* __restrict__ dw, float* __restrict__ db0) {
    __shared__ float s_part[256];
    constexpr int kStage = 2048;                      // documents whose row offsets and dpre are staged per pass
    __shared__ long s_off[kStage];
    __shared__ float s_dp[kStage];
    const int l = blockIdx.x, tid = threadIdx.x;
    if (l == L) {
        if (tid == 0) { float s = 0.f; for (int b = 0; b < B; ++b) s += dpre[b]; db0[0] = s; }
        return;
    }
    const int ncls = max(1, 256 / E);                 // document classes that fit beside E columns
    for (int e0 = 0; e0 < E; e0 += 256) {
        const int cls = (E >= 256) ? 0 : tid / E, e = e0 + ((E >= 256) ? tid : tid - cls * E);
        const bool live = cls < ncls && e < E;
        float s = 0.f;
        // the token ids of this position (one per document, a strided column of `ids`) are fetched once per pass into LDS, all
        // at the same time: the row reads below then depend on nothing but LDS (they were a chain id -> row, 8 at a time)
        for (int bs = 0; bs < B; bs += kStage) {
            const int nb = min(kStage, B - bs);
            __syncthreads();
            for (int k = tid; k < nb; k += 256) {
                s_off[k] = ids[(long)(bs + k) * L + l] * (long)E;
                s_dp[k] = dpre[bs + k];
            }
            __syncthreads();
            if (live) {
                for (int b0i = cls; b0i < nb; b0i += 8 * ncls) {
                    float x[8], dp[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int b = b0i + u * ncls;
                        const bool ok = b < nb;
                        dp[u] = ok ? s_dp[b] : 0.f;
                        x[u] = ok ? table[s_off[b] + e] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) s = fmaf(dp[u], x[u], s);
                }
            }
        }
        __syncthreads();
        s_part[tid] = live ? s : 0.f;
        __syncthreads();
        if (live && cls == 0) {
            float t = s_part[tid];
            for (int c2 = 1; c2 < ncls; ++c2) t += s_part[tid + c2 * E];
            dw[(long)e * L + l] = t;
        }
    }
}


// ---------------------------------------------------------------------------------- local gate, token-product form
// The gate's input is an embedding LOOKUP too: pre[b,l] = b0 + sum_j S[ids[b, l+j-pad]][j] with S[t][j] = <table[t,:], w[:,j]>,
// so S is needed once per DISTINCT token of the batch (21 k of 1 M positions at cfg4) and the gate itself is a gather of
// `win` scalars per position from a table that lives in L2.  Backward: c[t][j] = sum of dpre over the positions whose tap j
// lands on token t (LDS-bucketed per 256-position window, gate_bwd_dx_kernel's c_out mode), then
//   dtable[t,:] = sum_j c[t][j] w[:,j]   (every row written once),   dw[:,j] = sum_t c[t][j] table[t,:],   db0 = sum_t c[t][pad].
__device__ __forceinline__ void gp_mark_kernel(long n, const long long* __restrict__ ids, int* __restrict__ used) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) used[ids[k]] = 1;
}

// Row numbers in vocabulary order: the number of used tokens below v.  (They came from an atomic counter, one add per wave in
// arrival order: the same batch got another permutation of rows from run to run, and everything summed in row order -- dw and
// db0 of the token-product gate -- rounded differently each time, and differently between a tower's shared maps and private ones.)
// gp_count_kernel leaves the used tokens of every 256 vocabulary entries, gp_compact_kernel's workgroup adds up those before it:
// nblk^2 / 2 reads of L2-resident ints over the grid (nblk = V / 256: 20 k reads at the 50 k vocabularies of the configs, 8 M at
// V = 1 M -- a vocabulary of that size wants a scan of the block counts first).  The last workgroup writes the row counter.
// The ranking inside a block is block_rank_256 (rbr_wave.h), shared with the conv's compact_block (textcnn_prod.hip).
__device__ __forceinline__ void gp_count_kernel(int V, const int* __restrict__ used, int* __restrict__ blk_count) {
    __shared__ int s_n[4];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const BlockRank r = block_rank_256((v < V) ? used[v] : 0, s_n);
    if (threadIdx.x == 0) blk_count[blockIdx.x] = r.total;
}

__device__ __forceinline__ void gp_compact_kernel(int V, int cap, const int* __restrict__ used, const int* __restrict__ blk_count,
                                                         int* __restrict__ row_of_token, int* __restrict__ tok_of_row,
                                                         int* __restrict__ counter) {
    __shared__ int s_red[256];
    __shared__ int s_n[4];
    const int tid = threadIdx.x;
    const int v = blockIdx.x * 256 + tid;
    const int u = (v < V) ? used[v] : 0;
    int part = 0;
    for (int k = tid; k < (int)blockIdx.x; k += 256) part += blk_count[k];
    s_red[tid] = part;
    const BlockRank r = block_rank_256(u, s_n);      // its barrier publishes s_red too
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    const int base = s_red[0];                                          // used tokens below the block
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *counter = base + r.total;
    if (v < V) {
        int row = -1;
        if (r.rank >= 0) {
            row = base + r.rank;
            if (row < cap) tok_of_row[row] = v; else row = -1;
        }
        row_of_token[v] = row;
    }
}

// S[row][j] = <table[tok_of_row[row], :], w[:, j]>; 16 lanes per row (four rows per wave): a wave per row spent its time in
// the 48 shuffles that fold eight accumulators over 64 lanes (22 us for 21 k rows of 400 bytes)
__device__ __forceinline__ void gp_taps_kernel(int E, int win, int cap, const int* __restrict__ counter,
                                                      const int* __restrict__ tok_of_row, const float* __restrict__ table,
                                                      const float* __restrict__ w, float* __restrict__ S) {
    const int n = min(*counter, cap);
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;                  // 16 row slots per workgroup
    for (int row0 = blockIdx.x * 16; row0 < n; row0 += gridDim.x * 16) {
        const int row = row0 + sub;
        const bool live = row < n;
        const float* trow = table + (long)(live ? tok_of_row[row] : 0) * E;
        float acc[kGateWP];
#pragma unroll
        for (int j = 0; j < kGateWP; ++j) acc[j] = 0.f;
        if (live)
            for (int e = l; e < E; e += 16) {
                const float x = trow[e];
#pragma unroll
                for (int j = 0; j < kGateWP; ++j)
                    if (j < win) acc[j] = fmaf(x, w[(long)e * win + j], acc[j]);
            }
#pragma unroll
        for (int j = 0; j < kGateWP; ++j)
            if (j < win) acc[j] = wave_sum<16>(acc[j]);
        if (live && l < kGateWP) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < kGateWP; ++j) if (j == l) v = acc[j];
            S[(long)row * kGateWP + l] = v;
        }
    }
}

__device__ __forceinline__ void gp_gate_kernel(int B, int L, int win, const long long* __restrict__ ids,
                                                      const int* __restrict__ row_of_token, const float* __restrict__ S,
                                                      const float* __restrict__ b0, float* __restrict__ gate) {
    const long n = (long)B * L;
    const int pad = (win - 1) / 2;
    const float bias = b0[0];
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const int l = (int)(k % L);
        float s = 0.f;
        for (int j = 0; j < win; ++j) {
            const int p = l + j - pad;
            if (p < 0 || p >= L) continue;                    // zero padding outside the document
            const int row = row_of_token[ids[k + j - pad]];
            s += S[(long)row * kGateWP + j];
        }
        gate[k] = sigmoidf_(s + bias);
    }
}

// c[0][k] += c[1..copies-1][k]   (fixed order)
__device__ __forceinline__ void gp_csum_kernel(int cap, const int* __restrict__ counter, float* __restrict__ c) {
    const long n = (long)min(*counter, cap) * kGateWP, stride = (long)cap * kGateWP;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        float s = c[k];
#pragma unroll
        for (int g = 1; g < kGateCopies; ++g) s += c[g * stride + k];
        c[k] = s;
    }
}

// ---- global gate, table gradient through the occurrence matrix ------------------------------------------------------
// dtable[t, :] = sum_p A[t, p] * wT[p, :]  with  A[t, p] = sum over the documents b that carry token t at position p of dpre[b].
// A is kept per distinct-token ROW ([n_rows, L] f32): building it costs ONE scalar atomic per position instead of a row of E
// (the f32 atomics are priced per 64-byte request, ~25 G/s chip-wide: the per-window rows of gate_bwd_dx_kernel are 2.9 M
// requests at cfg4, the scalars 0.5 M), and every table row is then written once, from its non-zeros.
__device__ __forceinline__ void gg_zero_kernel(int cap, int L, const int* __restrict__ counter, f32x4g* __restrict__ A,
                                                      int* __restrict__ dense_count) {
    const long n = (long)min(*counter, cap) * L / 4;                    // L % 4 == 0 (checked by the caller)
    const f32x4g z = {0.f, 0.f, 0.f, 0.f};
    if (blockIdx.x == 0 && threadIdx.x == 0) *dense_count = 0;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) A[k] = z;
}

__device__ __forceinline__ void gg_scatter_kernel(int B, int L, int pad_idx, const long long* __restrict__ ids,
                                                         const int* __restrict__ row_of_token, const float* __restrict__ dpre,
                                                         float* __restrict__ A) {
    const long n = (long)B * L;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const int t = (int)ids[k];
        if (t == pad_idx) continue;
        const int b = (int)(k / L), p = (int)(k - (long)b * L);
        atomicAdd(A + (long)row_of_token[t] * L + p, dpre[b]);
    }
}

// acc[c] += sum over the non-zeros of the 64-position stretch at p0 (lane j holds a = A[row, p0 + j]) of a * wT[p0 + j, c*64 + lane]:
// the non-zeros are visited kGgU at a time, their weight rows requested before the first use.
constexpr int kGgChunks = 4;                         // embedding columns per lane: E <= 256
constexpr int kGgU = 8;
__device__ __forceinline__ void gg_stretch(float a, int p0, int E, int lane, const float* __restrict__ wT, float (&acc)[kGgChunks]) {
    unsigned long long m = __ballot(a != 0.f);
    while (m) {
        int j[kGgU];
        float av[kGgU];
#pragma unroll
        for (int u = 0; u < kGgU; ++u) {
            j[u] = m ? __builtin_ctzll(m) : -1;
            if (m) m &= m - 1;
            av[u] = (j[u] >= 0) ? __shfl(a, j[u]) : 0.f;
        }
#pragma unroll
        for (int c = 0; c < kGgChunks; ++c) {
            const int e = c * 64 + lane;
            if (c * 64 >= E) break;                  // wave-uniform
            float x[kGgU];
#pragma unroll
            for (int u = 0; u < kGgU; ++u) x[u] = (j[u] >= 0 && e < E) ? wT[(long)(p0 + j[u]) * E + e] : 0.f;
#pragma unroll
            for (int u = 0; u < kGgU; ++u) acc[c] = fmaf(av[u], x[u], acc[c]);
        }
    }
}

// One WAVE per vocabulary entry (absent tokens and the pad row: zeros).  The wave reads its row of A (all stretches requested
// at once), counts the non-zeros, and either builds the table row from them or -- a row with more than kGgDense of them, a
// Zipf-hot token -- leaves it on the dense list for gg_dense_rows_kernel (a workgroup of 16 waves per row): a workgroup per
// entry spent its time on the fixed latencies of 50 k mostly near-empty rows, a wave per entry would walk the hot rows' 1024
// non-zeros one after the other.
constexpr int kGgDense = 96, kGgStretch = 16;        // stretches (of 64 positions) of a row held in registers at a time
__device__ __forceinline__ void gg_rows_kernel(int V, int L, int E, int pad_idx, const int* __restrict__ row_of_token,
                                                      const float* __restrict__ A, const float* __restrict__ wT,
                                                      float* __restrict__ dtable, int* __restrict__ dense_count,
                                                      int* __restrict__ dense_list, int accumulate) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= V) return;
    const int row = row_of_token[v];
    if (row < 0 || v == pad_idx) {
        if (!accumulate)
            for (int e = lane; e < E; e += 64) dtable[(long)v * E + e] = 0.f;
        return;
    }
    const float* arow = A + (long)row * L;
    int nnz = 0;
    float acc[kGgChunks];
#pragma unroll
    for (int c = 0; c < kGgChunks; ++c) acc[c] = 0.f;
    for (int pb = 0; pb < L; pb += 64 * kGgStretch) {
        float a[kGgStretch];
#pragma unroll
        for (int q = 0; q < kGgStretch; ++q) { const int p = pb + q * 64 + lane; a[q] = (p < L) ? arow[p] : 0.f; }   // one latency
#pragma unroll
        for (int q = 0; q < kGgStretch; ++q) nnz += __popcll(__ballot(a[q] != 0.f));
        if (nnz > kGgDense) {                        // wave-uniform; what was summed so far is dropped
            if (lane == 0) dense_list[atomicAdd(dense_count, 1)] = v;
            return;
        }
#pragma unroll
        for (int q = 0; q < kGgStretch; ++q) gg_stretch(a[q], pb + q * 64, E, lane, wT, acc);
    }
#pragma unroll
    for (int c = 0; c < kGgChunks; ++c) {
        const int e = c * 64 + lane;
        if (e < E) dtable[(long)v * E + e] = accumulate ? dtable[(long)v * E + e] + acc[c] : acc[c];
    }
}

// dense rows: one workgroup of 16 waves per listed token, wave w walks the stretches w, w + 16, ...; partial rows meet in LDS
__device__ __forceinline__ void gg_dense_rows_kernel(int L, int E, const int* __restrict__ row_of_token,
                                                             const float* __restrict__ A, const float* __restrict__ wT,
                                                             float* __restrict__ dtable, const int* __restrict__ dense_count,
                                                             const int* __restrict__ dense_list, int accumulate) {
    __shared__ float s_part[16][kGgChunks * 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = *dense_count;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int v = dense_list[i];
        const float* arow = A + (long)row_of_token[v] * L;
        float acc[kGgChunks];
#pragma unroll
        for (int c = 0; c < kGgChunks; ++c) acc[c] = 0.f;
        for (int p0 = wave * 64; p0 < L; p0 += 16 * 64) gg_stretch(p0 + lane < L ? arow[p0 + lane] : 0.f, p0, E, lane, wT, acc);
#pragma unroll
        for (int c = 0; c < kGgChunks; ++c) s_part[wave][c * 64 + lane] = acc[c];
        __syncthreads();
        for (int e = tid; e < E; e += 1024) {
            float t = 0.f;
#pragma unroll
            for (int w2 = 0; w2 < 16; ++w2) t += s_part[w2][e];
            dtable[(long)v * E + e] = accumulate ? dtable[(long)v * E + e] + t : t;
        }
        __syncthreads();
    }
}

// dtable[v, :] = sum_j c[row(v)][j] w[:, j]  (0 for absent tokens and the pad row): the whole [V, E] gradient is overwritten
__device__ __forceinline__ void gp_dtable_kernel(int V, int E, int win, int pad_idx, const int* __restrict__ row_of_token,
                                                        const float* __restrict__ c, const float* __restrict__ w,
                                                        float* __restrict__ dtable, int accumulate) {
    const long n = (long)V * E;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const int v = (int)(k / E), e = (int)(k - (long)v * E);
        const int row = row_of_token[v];
        float s = 0.f;
        const bool live = row >= 0 && v != pad_idx;
        if (live)
            for (int j = 0; j < win; ++j) s = fmaf(c[(long)row * kGateWP + j], w[(long)e * win + j], s);
        if (!accumulate) dtable[k] = s;
        else if (live) dtable[k] += s;                  // shared gradient buffer (functional.table_fanout): rows of the batch only
    }
}

// accumulate form: dtable[tok_of_row[row], :] += sum_j c[row][j] w[:, j] over the batch's rows only (the shared gradient buffer of
// functional.table_fanout): 2.1 M elements at cfg4 instead of the vocabulary's 5 M
__device__ __forceinline__ void gp_dtable_rows_kernel(int E, int win, int cap, int pad_idx, const int* __restrict__ counter,
                                                             const int* __restrict__ tok_of_row, const float* __restrict__ c,
                                                             const float* __restrict__ w, float* __restrict__ dtable) {
    const long n = (long)min(*counter, cap) * E;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const int row = (int)(k / E), e = (int)(k - (long)row * E);
        const int v = tok_of_row[row];
        if (v == pad_idx) continue;
        float* dst = dtable + (long)v * E + e;
        const float old = *dst;
        float s = 0.f;
        for (int j = 0; j < win; ++j) s = fmaf(c[(long)row * kGateWP + j], w[(long)e * win + j], s);
        *dst = old + s;
    }
}

// per-chunk partial of dw[e, j] = sum_rows c[row][j] * table[tok][e]  and  db0 = sum_rows c[row][pad]; 128 rows per workgroup
constexpr int kGpRows = 128;
__device__ __forceinline__ void gp_dw_partial_kernel(int E, int win, int cap, const int* __restrict__ counter,
                                                            const int* __restrict__ tok_of_row, const float* __restrict__ table,
                                                            const float* __restrict__ c, float* __restrict__ part) {
    __shared__ float s_c[kGpRows * kGateWP];
    __shared__ long s_off[kGpRows];
    const int n = min(*counter, cap);
    const int r0 = blockIdx.x * kGpRows, rows = max(0, min(kGpRows, n - r0));
    const int n_out = win * E + 1;
    float* my = part + (long)blockIdx.x * n_out;
    for (int e = threadIdx.x; e < rows * kGateWP; e += 256) s_c[e] = c[(long)r0 * kGateWP + e];
    for (int r = threadIdx.x; r < rows; r += 256) s_off[r] = (long)tok_of_row[r0 + r] * E;
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += 256) {
        float acc[kGateWP];
#pragma unroll
        for (int j = 0; j < kGateWP; ++j) acc[j] = 0.f;
        for (int r = 0; r < rows; ++r) {
            const float x = table[s_off[r] + e];
#pragma unroll
            for (int j = 0; j < kGateWP; ++j) acc[j] = fmaf(s_c[r * kGateWP + j], x, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kGateWP; ++j)
            if (j < win) my[(long)e * win + j] = acc[j];
    }
    if (threadIdx.x == 0) {
        float sb = 0.f;
        const int pad = (win - 1) / 2;
        for (int r = 0; r < rows; ++r) sb += s_c[r * kGateWP + pad];
        my[n_out - 1] = sb;
    }
}

// one wave per output: lanes stride the chunks that hold rows (ceil(n / 128) of them), shuffle reduction, fixed order
__device__ __forceinline__ void gp_dw_final_kernel(int cap, int n_out, const int* __restrict__ counter,
                                                          const float* __restrict__ part, float* __restrict__ dw,
                                                          float* __restrict__ db0) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= n_out) return;
    const int n_chunks = (min(*counter, cap) + kGpRows - 1) / kGpRows;
    float t = 0.f;
    for (int k = lane; k < n_chunks; k += 64) t += part[(long)k * n_out + o];
    t = wave_sum(t);
    if (lane == 0) { if (o < n_out - 1) dw[o] = t; else db0[0] = t; }
}

}  // namespace rbr

using namespace rbr;

// ---------------------------------------------------------------------------------- host side
// The openings the entry points share -- shape check, null check, window limit -- and the launch geometry, stated once.
namespace {

bool gate_args_ok(int B, int L, int E, int win) {
    if (B <= 0 || L <= 0 || E <= 0 || win <= 0) { set_error("bad gate shape B=%d L=%d E=%d win=%d", B, L, E, win); return false; }
    return true;
}
template <class... P> int refuse_null(const P*... p) {
    if (((p != nullptr) && ...)) return 0;
    set_error("null pointer");
    return RBR_ERR_BAD_ARG;
}
int refuse_wide_window(int win) {      // the dense local gate keeps kMaxKF taps in registers per pass and a halo of kMaxKF in LDS
    if (win <= 2 * kMaxKF + 1) return 0;
    set_error("local attention window %d exceeds the supported %d", win, 2 * kMaxKF + 1);
    return RBR_ERR_UNSUPPORTED;
}
const long long* ids64(const int64_t* ids) { return reinterpret_cast<const long long*>(ids); }
// grid of a grid-stride kernel over n items: ceil(n / 256) workgroups, at most `most`
dim3 grid256(long n, long most) { return dim3((unsigned)std::min<long>((n + 255) / 256, most)); }
int n_windows(int L) { return (L + kGWin - 1) / kGWin; }      // windows per document of gate_bwd_dx_kernel

}  // namespace

extern "C" int rbr_datt_local_gate_fwd(int32_t B, int32_t L, int32_t E, int32_t win, const int64_t* ids, const float* table,
                                       const float* w, const float* b0, float* gate, void* stream) {
    if (!gate_args_ok(B, L, E, win)) return RBR_ERR_BAD_ARG;
    if (win % 2 == 0) { set_error("local attention window must be odd, got %d", win); return RBR_ERR_BAD_ARG; }
    if (int e = refuse_null(ids, table, w, b0, gate)) return e;
    if (int e = refuse_wide_window(win)) return e;
    const size_t smem = (size_t)(kGTile + win - 1) * E * sizeof(float);
    if (smem > 120 * 1024) { set_error("embedding dim %d too large for the local-gate LDS tile", E); return RBR_ERR_UNSUPPORTED; }
    const int ntile = (L + kGTile - 1) / kGTile;
    hipLaunchKernelGGL(local_gate_fwd_kernel, dim3((unsigned)(B * ntile)), dim3(256), smem, (hipStream_t)stream, B, L, E, win,
                       ntile, ids64(ids), table, w, b0, gate);
    RBR_CHECK_LAUNCH("datt local gate fwd launch");
    return 0;
}

extern "C" int rbr_datt_global_gate_fwd(int32_t B, int32_t L, int32_t E, const int64_t* ids, const float* table,
                                        const float* w, const float* b0, float* gate, void* stream) {
    if (!gate_args_ok(B, L, E, 1)) return RBR_ERR_BAD_ARG;
    if (int e = refuse_null(ids, table, w, b0, gate)) return e;
    return launch<global_gate_fwd_kernel, 256>(dim3(B), dim3(256), 0, (hipStream_t)stream, "datt global gate fwd launch",
                                               B, L, E, ids64(ids), table, w, b0, gate);
}

extern "C" size_t rbr_datt_gate_bwd_ws_floats(int32_t B, int32_t L, int32_t E, int32_t win, int32_t is_global) {
    if (B <= 0 || L <= 0 || E <= 0 || win <= 0) return 0;
    return is_global ? (size_t)B + (size_t)E * L : (size_t)B * ((size_t)win * E + 1);
}

extern "C" int rbr_datt_local_gate_bwd(int32_t B, int32_t L, int32_t E, int32_t win, const int64_t* ids, const float* table,
                                       const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                                       float* db0, float* dtable, float* ws, void* stream) {
    if (!gate_args_ok(B, L, E, win)) return RBR_ERR_BAD_ARG;
    if (int e = refuse_null(ids, table, w, gate, dgate, dw, db0, ws)) return e;
    if ((size_t)L * sizeof(float) > 60 * 1024) { set_error("doc_len %d too large for the LDS strip", L); return RBR_ERR_UNSUPPORTED; }
    if (int e = refuse_wide_window(win)) return e;
    hipStream_t st = (hipStream_t)stream;
    const size_t smem_dw = (size_t)(L + 2 * ((win - 1) / 2) + std::max(kGTile * E, 2 * kMaxKF * 128)) * sizeof(float);
    if (smem_dw > 140 * 1024) { set_error("doc_len %d x emb %d too large for the local-gate LDS tiles", L, E); return RBR_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(local_gate_bwd_dw_kernel, dim3(B), dim3(256), smem_dw, st, B, L, E, win, ids64(ids), table, gate, dgate, ws);
    RBR_CHECK_LAUNCH("datt local gate bwd dw launch");
    hipLaunchKernelGGL(local_gate_bwd_reduce_kernel, dim3((unsigned)((win * E + 1 + 31) / 32)), dim3(256), 0, st, B, E, win,
                       ws, dw, db0);
    RBR_CHECK_LAUNCH("datt local gate bwd reduce launch");
    if (dtable == nullptr) return 0;
    const int nwin = n_windows(L);
    return launch<gate_bwd_dx_kernel, 256>(dim3((unsigned)(B * nwin)), dim3(256), (size_t)kGWin * win * sizeof(float), st,
                                           "datt local gate bwd dx launch", B, L, E, win, 0, nwin, ids64(ids), w, nullptr, gate, dgate,
                                           nullptr, pad_idx, dtable, nullptr, nullptr, 0L);
}

// ---- global gate backward: the two phases both forms share (dpre at the front of `ws`, wT behind it)
namespace {
int global_gate_bwd_weights(int B, int L, int E, const long long* ids, const float* table, const float* gate, const float* dgate,
                            float* dpre, float* dw, float* db0, hipStream_t st) {
    if (int e = launch<global_gate_bwd_dpre_kernel, 256>(dim3(B), dim3(256), 0, st, "datt global gate bwd dpre launch",
                                                         B, L, gate, dgate, dpre)) return e;
    return launch<global_gate_bwd_dw_kernel, 256>(dim3(L + 1), dim3(256), 0, st, "datt global gate bwd dw launch",
                                                  B, L, E, ids, table, dpre, dw, db0);
}
int global_gate_transpose(int E, int L, const float* w, float* wT, hipStream_t st) {
    return launch<transpose_w_kernel, 256>(grid256((long)E * L, 2048), dim3(256), 0, st, "datt global gate transpose launch", E, L, w, wT);
}
}  // namespace

extern "C" int rbr_datt_global_gate_bwd(int32_t B, int32_t L, int32_t E, const int64_t* ids, const float* table,
                                        const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                                        float* db0, float* dtable, float* ws, void* stream) {
    if (!gate_args_ok(B, L, E, 1)) return RBR_ERR_BAD_ARG;
    if (int e = refuse_null(ids, table, w, gate, dgate, dw, db0, ws)) return e;
    hipStream_t st = (hipStream_t)stream;
    float *dpre = ws, *wT = ws + B;
    if (int e = global_gate_bwd_weights(B, L, E, ids64(ids), table, gate, dgate, dpre, dw, db0, st)) return e;
    if (dtable == nullptr) return 0;
    if (int e = global_gate_transpose(E, L, w, wT, st)) return e;
    const int nwin = n_windows(L);
    return launch<gate_bwd_dx_kernel, 256>(dim3((unsigned)(B * nwin)), dim3(256), 0, st, "datt global gate bwd dx launch",
                                           B, L, E, 1, 1, nwin, ids64(ids), w, wT, gate, dgate, dpre, pad_idx, dtable,
                                           nullptr, nullptr, 0L);
}

// ---- distinct-token row maps of a document batch: row_of_token [V] (dense row or -1), tok_of_row [cap],
// the row counter; rows numbered in vocabulary order.  One layout and one build for the tower's shared maps (rbr_datt_token_rows:
// the whole `rows` buffer) and for a token-product gate's private ones (the same block at the front of its `ws`).
namespace {

struct TokenRowsLayout { size_t counter, used, row_of_token, tok_of_row, blk, total; int cap; };      // byte offsets
bool token_rows_layout(int B, int L, int V, TokenRowsLayout& T) {
    if (B <= 0 || L <= 0 || V <= 0) return false;
    T.cap = (int)std::min<long>(V, (long)B * L);
    size_t o = 0;
    T.counter = o;      o += 256;
    T.used = o;         o += align256((size_t)V * sizeof(int));      // contiguous with the counter: zeroed together
    T.row_of_token = o; o += align256((size_t)V * sizeof(int));
    T.tok_of_row = o;   o += align256((size_t)T.cap * sizeof(int));
    T.blk = o;          o += align256((((size_t)V + 255) / 256) * sizeof(int));        // used tokens per 256 vocabulary entries
    T.total = o;
    return true;
}

// The maps as typed pointers: the one place that casts the layout's offsets.  `base` is const for the consumers, which only read.
struct TokenRows { int *counter, *used, *row_of_token, *tok_of_row, *blk; int cap; };
bool token_rows(int B, int L, int V, const void* base, TokenRows& R) {
    TokenRowsLayout T;
    if (!token_rows_layout(B, L, V, T)) return false;
    char* p = static_cast<char*>(const_cast<void*>(base));
    auto at = [p](size_t o) { return reinterpret_cast<int*>(p + o); };
    R = TokenRows{at(T.counter), at(T.used), at(T.row_of_token), at(T.tok_of_row), at(T.blk), T.cap};
    return true;
}

// zero (counter | used) -> mark -> count per 256 vocabulary entries -> compact
int build_token_rows(const TokenRows& R, const long long* ids, long n_pos, int V, hipStream_t st) {
    const dim3 vocab_blocks((V + 255) / 256);
    if (int e = zero_words(R.counter, (size_t)(R.row_of_token - R.counter) * sizeof(int), st)) return e;
    if (int e = launch<gp_mark_kernel, 256>(grid256(n_pos, 2048), dim3(256), 0, st, "token rows mark launch", n_pos, ids, R.used)) return e;
    if (int e = launch<gp_count_kernel, 256>(vocab_blocks, dim3(256), 0, st, "token rows count launch", V, R.used, R.blk)) return e;
    return launch<gp_compact_kernel, 256>(vocab_blocks, dim3(256), 0, st, "token rows compact launch",
                                          V, R.cap, R.used, R.blk, R.row_of_token, R.tok_of_row, R.counter);
}

}  // namespace

extern "C" size_t rbr_datt_token_rows_ws_bytes(int32_t B, int32_t L, int32_t V) {
    TokenRowsLayout T;
    return token_rows_layout(B, L, V, T) ? T.total : 0;
}

extern "C" int rbr_datt_token_rows(int32_t B, int32_t L, int32_t V, const int64_t* ids, void* rows, void* stream) {
    TokenRows R;
    if (!rbr_datt_token_rows_ws_bytes(B, L, V)) { set_error("bad token-rows shape B=%d L=%d V=%d", B, L, V); return RBR_ERR_BAD_ARG; }
    if (int e = refuse_null(ids, rows)) return e;
    token_rows(B, L, V, rows, R);
    return build_token_rows(R, ids64(ids), (long)B * L, V, (hipStream_t)stream);
}

// Where rbr_datt_token_rows left the maps inside `rows` (the layout is private): the twin of rbr_textcnn_token_list
extern "C" int rbr_datt_token_rows_maps(int32_t B, int32_t L, int32_t V, const void* rows, const int32_t** row_of_token,
                                        const int32_t** n_rows, const int32_t** tok_of_row, int32_t* cap) {
    TokenRows R;
    if (!rows || !token_rows(B, L, V, rows, R)) { set_error("no token rows for B=%d L=%d V=%d", B, L, V); return RBR_ERR_BAD_ARG; }
    if (row_of_token) *row_of_token = R.row_of_token;
    if (n_rows) *n_rows = R.counter;
    if (tok_of_row) *tok_of_row = R.tok_of_row;
    if (cap) *cap = R.cap;
    return 0;
}

// ---- token-product local gate (same results as rbr_datt_local_gate_fwd / _bwd; `ws` must survive from forward to backward)
// ws = a token-rows block (the private maps; unused when the tower's shared ones are handed in) | S | c | part
namespace {

struct GateProdLayout { TokenRowsLayout rows; size_t S, c, part, total; int cap, n_chunks; };
bool gate_prod_layout(int B, int L, int E, int win, int V, GateProdLayout& G) {
    if (E <= 0 || win <= 0 || win > kGateWP || win % 2 == 0 || !token_rows_layout(B, L, V, G.rows)) return false;
    G.cap = G.rows.cap;
    G.n_chunks = (G.cap + kGpRows - 1) / kGpRows;
    size_t o = G.rows.total;
    G.S = o;            o += align256((size_t)G.cap * kGateWP * sizeof(float));
    G.c = o;            o += align256((size_t)G.cap * kGateWP * sizeof(float) * kGateCopies);
    G.part = o;         o += align256((size_t)G.n_chunks * ((size_t)win * E + 1) * sizeof(float));
    G.total = o;
    return true;
}

// What a token-product gate call works on: its row maps -- the tower's shared ones (`rows`) or the private ones at the front of
// `ws` -- and its own regions, typed.
struct GateProd {
    TokenRows R;
    float *S, *c, *part;      // tap products [cap][kGateWP], tap sums [kGateCopies][cap][kGateWP], dw partials [n_chunks][win * E + 1]
    int cap, n_chunks;
};
int gate_prod(int B, int L, int E, int win, int V, void* ws, const void* rows, GateProd& P) {
    GateProdLayout G;
    if (!gate_prod_layout(B, L, E, win, V, G)) {
        set_error("bad local gate shape B=%d L=%d E=%d win=%d V=%d", B, L, E, win, V);
        return RBR_ERR_BAD_ARG;
    }
    if (int e = refuse_null(ws)) return e;
    token_rows(B, L, V, rows ? rows : ws, P.R);
    char* p = static_cast<char*>(ws);
    auto at = [p](size_t o) { return reinterpret_cast<float*>(p + o); };
    P.S = at(G.S); P.c = at(G.c); P.part = at(G.part);
    P.cap = G.cap; P.n_chunks = G.n_chunks;
    return 0;
}

}  // namespace

extern "C" size_t rbr_datt_local_gate_prod_ws_bytes(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V) {
    GateProdLayout G;
    if (!gate_prod_layout(B, L, E, win, V, G)) return 0;
    const int mode = forced_conv_mode();
    if (mode == 1 || (mode != 2 && !token_rows_pay(V, (long)B * L))) return 0;
    return G.total;
}

extern "C" int rbr_datt_local_gate_fwd_prod(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V, const int64_t* ids,
                                            const float* table, const float* w, const float* b0, float* gate, void* ws,
                                            const void* rows, void* stream) {
    GateProd P;
    if (int e = gate_prod(B, L, E, win, V, ws, rows, P)) return e;
    if (int e = refuse_null(ids, table, w, b0, gate)) return e;
    hipStream_t st = (hipStream_t)stream;
    const long n_pos = (long)B * L;
    // the tower's shared maps (rbr_datt_token_rows) were not handed in: build private ones
    if (rows == nullptr)
        if (int e = build_token_rows(P.R, ids64(ids), n_pos, V, st)) return e;
    if (int e = launch<gp_taps_kernel, 256>(dim3((unsigned)std::min((P.cap + 15) / 16, 4096)), dim3(256), 0, st, "datt gate taps launch",
                                            E, win, P.cap, P.R.counter, P.R.tok_of_row, table, w, P.S)) return e;
    return launch<gp_gate_kernel, 256>(grid256(n_pos, 8192), dim3(256), 0, st, "datt gate gather launch",
                                       B, L, win, ids64(ids), P.R.row_of_token, P.S, b0, gate);
}

extern "C" int rbr_datt_local_gate_bwd_prod(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V, const int64_t* ids,
                                            const float* table, const float* w, const float* gate, const float* dgate,
                                            int32_t pad_idx, float* dw, float* db0, float* dtable, void* ws, const void* rows,
                                            int32_t accumulate, void* stream) {
    GateProd P;
    if (int e = gate_prod(B, L, E, win, V, ws, rows, P)) return e;
    if (int e = refuse_null(ids, table, w, gate, dgate, dw, db0)) return e;
    hipStream_t st = (hipStream_t)stream;
    const TokenRows& R = P.R;
    const long c_stride = (long)P.cap * kGateWP;       // one copy of the tap-sum table
    if (int e = zero_words(P.c, (size_t)c_stride * sizeof(float) * kGateCopies, st)) return e;
    const int nwin = n_windows(L);
    if (int e = launch<gate_bwd_dx_kernel, 256>(dim3((unsigned)(B * nwin)), dim3(256), 0, st, "datt gate tap-sum launch",
                                                B, L, E, win, 0, nwin, ids64(ids), w, nullptr, gate, dgate, nullptr, pad_idx,
                                                nullptr, R.row_of_token, P.c, c_stride)) return e;
    if (int e = launch<gp_csum_kernel, 256>(grid256(c_stride, 2048), dim3(256), 0, st, "datt gate tap-sum fold launch",
                                            P.cap, R.counter, P.c)) return e;
    const int n_out = win * E + 1;
    if (int e = launch<gp_dw_partial_kernel, 256>(dim3(P.n_chunks), dim3(256), 0, st, "datt gate dw partial launch",
                                                  E, win, P.cap, R.counter, R.tok_of_row, table, P.c, P.part)) return e;
    if (int e = launch<gp_dw_final_kernel, 256>(dim3((n_out + 3) / 4), dim3(256), 0, st, "datt gate dw final launch",
                                                P.cap, n_out, R.counter, P.part, dw, db0)) return e;
    if (dtable == nullptr) return 0;
    if (accumulate)
        return launch<gp_dtable_rows_kernel, 256>(grid256((long)P.cap * E, 8192), dim3(256), 0, st, "gp_dtable_rows_kernel launch",
                                                  E, win, P.cap, pad_idx, R.counter, R.tok_of_row, P.c, w, dtable);
    return launch<gp_dtable_kernel, 256>(grid256((long)V * E, 8192), dim3(256), 0, st, "datt gate dtable launch",
                                         V, E, win, pad_idx, R.row_of_token, P.c, w, dtable, 0);
}

// ---- global gate backward over the tower's row maps
// ws = dpre [B] | wT [E * L] | A [cap * L] (16-byte aligned) | dense count (4 ints) | dense list [V]
namespace {
struct GlobalRowsWs { float *dpre, *wT, *A; f32x4g* A4; int *dense_count, *dense_list; };
GlobalRowsWs global_rows_ws(int B, int L, int E, int cap, float* ws) {
    GlobalRowsWs W;
    W.dpre = ws;
    W.wT = ws + B;
    W.A = W.wT + (((size_t)E * L + 3) & ~(size_t)3);             // 16-byte aligned behind wT when ws is
    if ((reinterpret_cast<uintptr_t>(W.A) & 15) != 0) W.A += 4 - ((reinterpret_cast<uintptr_t>(W.A) & 15) >> 2);
    W.A4 = reinterpret_cast<f32x4g*>(W.A);
    W.dense_count = reinterpret_cast<int*>(W.A + (size_t)cap * L);
    W.dense_list = W.dense_count + 4;
    return W;
}
}  // namespace

extern "C" size_t rbr_datt_global_gate_bwd_rows_ws_floats(int32_t B, int32_t L, int32_t E, int32_t V) {
    TokenRowsLayout T;
    if (!token_rows_layout(B, L, V, T) || E <= 0 || E > kGgChunks * 64 || L % 4 != 0) return 0;   // 0: use rbr_datt_global_gate_bwd
    return (size_t)B + (size_t)E * L + 8 + (size_t)T.cap * L + 4 + (size_t)V;
}

extern "C" int rbr_datt_global_gate_bwd_rows(int32_t B, int32_t L, int32_t E, int32_t V, const int64_t* ids, const float* table,
                                             const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                                             float* db0, float* dtable, float* ws, const void* rows, int32_t accumulate, void* stream) {
    if (!gate_args_ok(B, L, E, 1) || !rbr_datt_token_rows_ws_bytes(B, L, V)) return RBR_ERR_BAD_ARG;
    if (E > kGgChunks * 64 || L % 4 != 0) {
        set_error("global gate over token rows needs E <= %d and L %% 4 == 0 (E=%d L=%d)", kGgChunks * 64, E, L);
        return RBR_ERR_UNSUPPORTED;
    }
    // accumulate & 2: the table-gradient phase alone -- dpre is in `ws` already (an earlier call with dtable == NULL on the same
    // workspace did the weight phase); a caller that puts the two phases of its towers on different streams (functional._DattTowers)
    const bool rows_only = (accumulate & 2) != 0;
    accumulate &= 1;
    if (int e = refuse_null(ids, w, ws, rows)) return e;
    if (int e = rows_only ? refuse_null(dtable) : refuse_null(table, gate, dgate, dw, db0)) return e;
    hipStream_t st = (hipStream_t)stream;
    TokenRows R;
    token_rows(B, L, V, rows, R);
    const GlobalRowsWs W = global_rows_ws(B, L, E, R.cap, ws);
    if (!rows_only)
        if (int e = global_gate_bwd_weights(B, L, E, ids64(ids), table, gate, dgate, W.dpre, dw, db0, st)) return e;
    if (dtable == nullptr) return 0;
    if (int e = global_gate_transpose(E, L, w, W.wT, st)) return e;
    PairSolo solo;        // zero A -> scatter into A -> rows from A: a chain over the 160 MB occurrence matrix (rbr_launch.h)
    if (int e = launch<gg_zero_kernel, 256>(grid256((long)R.cap * L / 4, 8192), dim3(256), 0, st, "datt global gate occurrence zero launch",
                                            R.cap, L, R.counter, W.A4, W.dense_count)) return e;
    if (int e = launch<gg_scatter_kernel, 256>(grid256((long)B * L, 8192), dim3(256), 0, st, "datt global gate occurrence scatter launch",
                                               B, L, pad_idx, ids64(ids), R.row_of_token, W.dpre, W.A)) return e;
    if (int e = launch<gg_rows_kernel, 256>(dim3((unsigned)((V + 3) / 4)), dim3(256), 0, st, "datt global gate rows launch",
                                            V, L, E, pad_idx, R.row_of_token, W.A, W.wT, dtable, W.dense_count, W.dense_list, accumulate)) return e;
    return launch<gg_dense_rows_kernel, 1024>(dim3((unsigned)std::min(V, 512)), dim3(1024), 0, st, "datt global gate dense rows launch",
                                              L, E, R.row_of_token, W.A, W.wT, dtable, W.dense_count, W.dense_list, accumulate);
}
