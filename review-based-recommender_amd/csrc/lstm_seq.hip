// lstm_seq.hip -- one-layer bidirectional LSTM over N padded sequences of at most T steps, forward and backward:
// rbr_lstm_seq_fwd / rbr_lstm_seq_bwd (AHN's shared sentence encoder, models/ahn/ahn_layers.py:249-312, and the max over
// the words that follows it, ahn_model.py:62-67), and rbr_lstm_seq_saliency: gradient x input of every step through the
// backward's loop, without d_xproj (lstm_saliency_kernel, below the backward).
//
// The input projection xproj = x W_ih^T + b_ih + b_hh of BOTH directions is a plain GEMM over [N * T, E] and is done by
// rbr_linear_* in front of this file; what is left is the recurrence  gates_t = xproj_t + h_{t-1} W_hh^T  (gate order i, f, g, o),
// c_t = f c_{t-1} + i g,  h_t = o tanh(c_t), which cannot be batched over time.
//
// Tiling.  One workgroup owns a tile of TS sentences and ONE direction and loops over time.  Thread (j, sg) owns hidden unit j
// of the RS sentences of sentence group sg (TS = RS * nsg): the four gate pre-activations of unit j for RS sentences are
// 4 * RS accumulators in registers, c stays in registers, h of the tile lives in LDS (two buffers, one barrier per step).  A
// step streams W_hh once per workgroup -- from the k-major copy `wt` the forward makes first, so that the lanes of a wave read
// consecutive addresses -- and multiplies it with RS broadcast reads of h per four k: 4 * RS FMAs per weight load.  W_hh
// (2 x 4Hh x Hh floats: 720 KB at Hh = 150) stays in L2 for the whole launch; it does not fit in LDS.  Plain f32 FMAs in a
// fixed order: a sentence's result depends on nothing but the sentence, and two runs give the same bits.
//
// Sentences of a tile have different lengths.  Every workgroup loops to the LONGEST length of its tile -- a uniform trip count,
// so every __syncthreads() is reached by every thread -- and a sentence that has ended merely stops writing.  So that this
// costs little, the tiles are filled in the order of a counting sort by length that one small launch builds on the device
// (longest first: the long tiles start first); a sentence's result does not depend on the tile it lands in.  Step s of a
// sentence of length len is position t = s (forward direction) or t = len - 1 - s (reverse direction): what a packed sequence
// does.  No cooperative launch, no grid-wide synchronisation, no spin wait.
//
// The forward keeps, for the backward, the gate activations and c of every valid position and h_{t-1} (zeros at a sentence's
// first step and at every position behind its end).  The backward is the same loop in the opposite order: d_gates of the tile
// go through LDS, d h_{t-1} = d_gates W_hh uses the torch layout as it is (lanes along k), and
// d W_hh = sum over all positions of d_gates^T h_{t-1} is ONE product per direction on the MFMA GEMM of dense_misc.hip with its
// K (the positions) split in a fixed way and added in slice order: no float atomics anywhere.
#include "rbr_common.h"

namespace rbr {

constexpr int kLstmMaxT = 1000;       // the reference clamps sentence lengths there (ahn_layers.py:300)
constexpr int kLstmMaxH = 256;

struct LstmArgs {
    int N, T, Hh;
    int HP;          // Hh rounded up to 4: row pitch of h in LDS and row count of the k-major weight copy
    int JW;          // lanes along the hidden units: Hh rounded up to 64
    int nsg;         // sentence groups per workgroup
    int TS;          // sentences per workgroup = RS * nsg
    int tout_per_seq;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// wt[dir][k][r] = w_dir[r][k] for k < Hh, 0 for Hh <= k < HP
__global__ __launch_bounds__(256) void lstm_wt_kernel(int Hh, int HP, const float* __restrict__ w0, const float* __restrict__ w1,
                                                      float* __restrict__ wt) {
    const long per = (long)HP * 4 * Hh;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < 2 * per; e += (long)gridDim.x * 256) {
        const int dir = e >= per;
        const long q = e - dir * per;
        const int k = (int)(q / (4 * Hh)), r = (int)(q % (4 * Hh));
        const float* w = dir ? w1 : w0;
        wt[e] = (k < Hh) ? w[(long)r * Hh + k] : 0.f;
    }
}

__device__ __forceinline__ int clamped_len(long long l, int T) { return (int)(l < 0 ? 0 : (l > T ? T : l)); }

// perm[slot] = sentence, the sentences in the order of their (clamped) length, longest first; slots N .. npad-1 hold -1.
// One workgroup: a counting sort over the T + 1 <= 1001 lengths in LDS.  Which of two sentences of EQUAL length comes first is
// left to the arrival order of the integer atomics: it decides only which tile slot a sentence takes, never a result.
__global__ __launch_bounds__(1024) void lstm_perm_kernel(int N, int T, int npad, const long long* __restrict__ lengths,
                                                         int* __restrict__ perm) {
    __shared__ int cnt[kLstmMaxT + 1];
    const int tid = threadIdx.x;
    for (int l = tid; l <= T; l += 1024) cnt[l] = 0;
    __syncthreads();
    for (int n = tid; n < N; n += 1024) atomicAdd(&cnt[clamped_len(lengths[n], T)], 1);
    __syncthreads();
    if (tid == 0) {                                   // counts -> first slot of each length, longest first
        int o = 0;
        for (int l = T; l >= 0; --l) { const int c = cnt[l]; cnt[l] = o; o += c; }
    }
    __syncthreads();
    for (int n = tid; n < N; n += 1024) perm[atomicAdd(&cnt[clamped_len(lengths[n], T)], 1)] = n;
    for (int p = N + tid; p < npad; p += 1024) perm[p] = -1;
}

// sentences (s_n; -1: none) and lengths (clamped to [0, T]; 0 for an empty slot) of the tile into LDS; returns the longest
__device__ __forceinline__ int tile_lengths(const LstmArgs& A, const long long* __restrict__ lengths, const int* __restrict__ perm,
                                            int tile, int* s_len, int* s_n) {
    if ((int)threadIdx.x < A.TS) {
        const int n = perm[(long)tile * A.TS + threadIdx.x];
        s_n[threadIdx.x] = n;
        s_len[threadIdx.x] = (n >= 0) ? clamped_len(lengths[n], A.T) : 0;
    }
    __syncthreads();
    int lmax = 0;
    for (int r = 0; r < A.TS; ++r) lmax = max(lmax, s_len[r]);
    return lmax;
}

template <int RS>
__global__ __launch_bounds__(256) void lstm_fwd_kernel(const LstmArgs A, const float* __restrict__ xproj, const float* __restrict__ wt,
                                                       const long long* __restrict__ lengths, const int* __restrict__ perm,
                                                       const int* __restrict__ t_out, float* __restrict__ out, float* __restrict__ pooled, int* __restrict__ argmax,
                                                       float* __restrict__ gates, float* __restrict__ cs, float* __restrict__ hprev) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* hbuf = reinterpret_cast<float*>(smem);                                   // [2][TS][HP]
    int* s_len = reinterpret_cast<int*>(smem + (size_t)2 * A.TS * A.HP * sizeof(float));
    int* s_n = s_len + A.TS;
    const int tid = threadIdx.x, dir = blockIdx.y, tile = blockIdx.x;
    const int Hh = A.Hh, HP = A.HP, T = A.T;
    const int j = tid % A.JW, sg = tid / A.JW;
    const bool jv = j < Hh;
    for (int e = tid; e < 2 * A.TS * HP; e += blockDim.x) hbuf[e] = 0.f;
    const int lmax = tile_lengths(A, lengths, perm, tile, s_len, s_n);       // (its barrier also covers the zero fill)
    const int* my_n = s_n + sg * RS;              // the RS sentences of this thread
    const float* __restrict__ w = wt + (long)dir * HP * 4 * Hh;
    float c[RS], best[RS];
    int bt[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) { c[r] = 0.f; best[r] = -INFINITY; bt[r] = -1; }

    for (int s = 0; s < lmax; ++s) {
        const float* hp = hbuf + ((s & 1) * A.TS + sg * RS) * HP;
        float* hn = hbuf + (((s & 1) ^ 1) * A.TS + sg * RS) * HP;
        if (jv) {
            float acc[4][RS];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int len = s_len[sg * RS + r];
                const bool on = s < len;
                const int t = dir ? len - 1 - s : s;
                const long at = on ? ((long)my_n[r] * T + t) * 8L * Hh + (long)dir * 4 * Hh + j : 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g][r] = on ? xproj[at + (long)g * Hh] : 0.f;
            }
            for (int k4 = 0; k4 < HP; k4 += 4) {
                float wv[4][4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int g = 0; g < 4; ++g) wv[kk][g] = w[(long)(k4 + kk) * 4 * Hh + g * Hh + j];
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const float4 hv = *reinterpret_cast<const float4*>(hp + r * HP + k4);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float a = acc[g][r];
                        a = fmaf(hv.x, wv[0][g], a);
                        a = fmaf(hv.y, wv[1][g], a);
                        a = fmaf(hv.z, wv[2][g], a);
                        a = fmaf(hv.w, wv[3][g], a);
                        acc[g][r] = a;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int len = s_len[sg * RS + r];
                if (s < len) {
                    const int t = dir ? len - 1 - s : s;
                    const long pos = (long)my_n[r] * T + t;
                    const float gi = sigmoidf_(acc[0][r]), gf = sigmoidf_(acc[1][r]), gg = tanhf(acc[2][r]), go = sigmoidf_(acc[3][r]);
                    const float cn = fmaf(gf, c[r], gi * gg);
                    const float h = go * tanhf(cn);
                    c[r] = cn;
                    if (gates != nullptr) {
                        float* gp = gates + pos * 8L * Hh + (long)dir * 4 * Hh + j;
                        gp[0] = gi; gp[Hh] = gf; gp[2 * Hh] = gg; gp[3 * Hh] = go;
                        cs[pos * 2L * Hh + dir * Hh + j] = cn;
                        hprev[pos * 2L * Hh + dir * Hh + j] = hp[r * HP + j];
                    }
                    if (out != nullptr) out[pos * 2L * Hh + dir * Hh + j] = h;
                    // the first maximum in t, in either direction of travel
                    if (dir ? h >= best[r] : h > best[r]) { best[r] = h; bt[r] = t; }
                    hn[r * HP + j] = h;
                }
            }
        }
        __syncthreads();
    }
    if (!jv) return;
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        const long n = my_n[r];
        if (n < 0) continue;
        const int len = s_len[sg * RS + r];
        for (int t = len; t < T; ++t) {                                   // behind the sentence's end: zeros
            const long at = (n * T + t) * 2L * Hh + dir * Hh + j;
            if (out != nullptr) out[at] = 0.f;
            if (gates != nullptr) hprev[at] = 0.f;
        }
        if (pooled != nullptr) {
            // the reference takes the max over the batch-trimmed, zero-padded output: a sentence shorter than the batch's
            // output length competes with one zero
            const int to = t_out[A.tout_per_seq ? n : 0];
            float m = best[r];
            int a = bt[r];
            if (len < to && !(m > 0.f)) { m = 0.f; a = -1; }
            if (len == 0) { m = 0.f; a = -1; }
            pooled[n * 2L * Hh + dir * Hh + j] = m;
            argmax[n * 2L * Hh + dir * Hh + j] = a;
        }
    }
}

// d pre-activations of one unit at one step from the saved gate activations, c_t (ct), c_{t-1} (cp; 0 at the sentence's first
// step) and dh = d h_t; dc_rec, the d c carried from the later step, becomes this step's.  The ONE statement of this arithmetic:
// the backward and the word saliency both inline it, so the two see the same d pre-activations bit for bit.
struct LstmDpre { float ai, af, ag, ao; };
__device__ __forceinline__ LstmDpre lstm_dpre(float gi, float gf, float gg, float go, float ct, float cp, float dh, float& dc_rec) {
    const float tc = tanhf(ct);
    const float dc = fmaf(dh * go, 1.f - tc * tc, dc_rec);
    LstmDpre d;
    d.ai = dc * gg * gi * (1.f - gi);
    d.af = dc * cp * gf * (1.f - gf);
    d.ag = dc * gi * (1.f - gg * gg);
    d.ao = dh * tc * go * (1.f - go);
    dc_rec = dc * gf;
    return d;
}

// d h_{t-1}[j] of the RS sentences of a thread = sum over the 4 Hh gate rows of d_gates[row] * W_hh[row][j], d_gates of the
// thread's sentence group (tile rows row0 .. row0 + RS - 1 of dg) read from LDS, W_hh in the torch layout (lanes along k).
template <int RS>
__device__ __forceinline__ void lstm_dh_prev(int Hh, int G4, int j, const float* __restrict__ w, const float* dg, int row0,
                                             float (&dh_rec)[RS]) {
    float acc[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) acc[r] = 0.f;
    for (int q4 = 0; q4 < G4; q4 += 4) {
        float wv[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) wv[qq] = w[(long)(q4 + qq) * Hh + j];
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            const float4 d = *reinterpret_cast<const float4*>(dg + (row0 + r) * G4 + q4);
            float a = acc[r];
            a = fmaf(d.x, wv[0], a);
            a = fmaf(d.y, wv[1], a);
            a = fmaf(d.z, wv[2], a);
            a = fmaf(d.w, wv[3], a);
            acc[r] = a;
        }
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) dh_rec[r] = acc[r];
}

template <int RS>
__global__ __launch_bounds__(256) void lstm_bwd_kernel(const LstmArgs A, const float* __restrict__ w0, const float* __restrict__ w1,
                                                       const long long* __restrict__ lengths, const int* __restrict__ perm,
                                                       const float* __restrict__ gates,
                                                       const float* __restrict__ cs, const float* __restrict__ d_out,
                                                       const float* __restrict__ d_pooled, const int* __restrict__ argmax,
                                                       float* __restrict__ d_xproj) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dg = reinterpret_cast<float*>(smem);                                     // [TS][4 Hh] d pre-activations of the step
    int* s_len = reinterpret_cast<int*>(smem + (size_t)A.TS * 4 * A.Hh * sizeof(float));
    int* s_n = s_len + A.TS;
    const int tid = threadIdx.x, dir = blockIdx.y, tile = blockIdx.x;
    const int Hh = A.Hh, T = A.T, G4 = 4 * A.Hh;
    const int j = tid % A.JW, sg = tid / A.JW;
    const bool jv = j < Hh;
    const int lmax = tile_lengths(A, lengths, perm, tile, s_len, s_n);
    const int* my_n = s_n + sg * RS;
    const float* __restrict__ w = dir ? w1 : w0;                                    // [4 Hh][Hh]
    float dh_rec[RS], dc_rec[RS], dpl[RS];
    int amx[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        dh_rec[r] = 0.f; dc_rec[r] = 0.f; dpl[r] = 0.f; amx[r] = -1;
        const long n = my_n[r];
        if (jv && n >= 0 && d_pooled != nullptr) {
            amx[r] = argmax[n * 2L * Hh + dir * Hh + j];
            dpl[r] = d_pooled[n * 2L * Hh + dir * Hh + j];
        }
    }

    for (int s = lmax - 1; s >= 0; --s) {
        if (jv) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int len = s_len[sg * RS + r];
                float* dgr = dg + (sg * RS + r) * G4 + j;
                if (s < len) {
                    const int t = dir ? len - 1 - s : s;
                    const long pos = (long)my_n[r] * T + t;
                    const float* gp = gates + pos * 8L * Hh + (long)dir * 4 * Hh + j;
                    const float gi = gp[0], gf = gp[Hh], gg = gp[2 * Hh], go = gp[3 * Hh];
                    const float ct = cs[pos * 2L * Hh + dir * Hh + j];
                    const float cp = (s > 0) ? cs[(pos + (dir ? 1 : -1)) * 2L * Hh + dir * Hh + j] : 0.f;
                    float dh = dh_rec[r];
                    if (d_out != nullptr) dh += d_out[pos * 2L * Hh + dir * Hh + j];
                    if (amx[r] == t) dh += dpl[r];
                    const LstmDpre d = lstm_dpre(gi, gf, gg, go, ct, cp, dh, dc_rec[r]);
                    float* dx = d_xproj + pos * 8L * Hh + (long)dir * 4 * Hh + j;
                    dx[0] = d.ai; dx[Hh] = d.af; dx[2 * Hh] = d.ag; dx[3 * Hh] = d.ao;
                    dgr[0] = d.ai; dgr[Hh] = d.af; dgr[2 * Hh] = d.ag; dgr[3 * Hh] = d.ao;
                } else {
                    dgr[0] = 0.f; dgr[Hh] = 0.f; dgr[2 * Hh] = 0.f; dgr[3 * Hh] = 0.f;
                }
            }
        }
        __syncthreads();
        if (jv && s > 0) lstm_dh_prev<RS>(Hh, G4, j, w, dg, sg * RS, dh_rec);
        __syncthreads();
    }
    if (!jv) return;
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        const long n = my_n[r];
        if (n < 0) continue;
        const int len = s_len[sg * RS + r];
        for (int t = len; t < T; ++t) {                                   // behind the sentence's end (and empty rows): zeros
            float* dx = d_xproj + (n * T + t) * 8L * Hh + (long)dir * 4 * Hh + j;
            dx[0] = 0.f; dx[Hh] = 0.f; dx[2 * Hh] = 0.f; dx[3 * Hh] = 0.f;
        }
    }
}

// Word saliency: lstm_bwd_kernel's loop -- the same tiling, tile_lengths, trip count and d h_{t-1} through LDS -- that stores no
// d_xproj.  The input projection is linear, so gradient x input of a word needs no dx:
//     <d score / d x_t, x_t> = <W_ih^T dpre_t, x_t> = <dpre_t, W_ih x_t> = <dpre_t, xw_t>       (xw: the BIAS-FREE projection)
// and each step reduces a thread's four products dpre * xw over the hidden-unit lanes: the xor butterfly of rbr_wave.h inside a
// wave (lanes j >= Hh and ended sentences add 0.0f), lane 0 of each wave leaves the sums of its RS sentences in LDS in front of the
// step's first barrier, and behind it thread `slot` adds the JW / 64 wave sums of its sentence in wave order and stores
// words_out[n, t, dir].  `red` is written again only behind the step's second barrier.  The order of every addition depends on
// Hh alone: a word's bits depend on its sentence, not on the tile slot, the batch or the run.  No atomics, no workspace.
template <int RS>
__global__ __launch_bounds__(256) void lstm_saliency_kernel(const LstmArgs A, const float* __restrict__ w0, const float* __restrict__ w1,
                                                            const long long* __restrict__ lengths, const int* __restrict__ perm,
                                                            const float* __restrict__ gates, const float* __restrict__ cs,
                                                            const float* __restrict__ xw, const float* __restrict__ d_pooled,
                                                            const int* __restrict__ argmax, float* __restrict__ words_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dg = reinterpret_cast<float*>(smem);                                     // [TS][4 Hh] d pre-activations of the step
    int* s_len = reinterpret_cast<int*>(smem + (size_t)A.TS * 4 * A.Hh * sizeof(float));
    int* s_n = s_len + A.TS;
    float* red = reinterpret_cast<float*>(s_n + A.TS);                              // [waves][RS] wave sums of the step
    const int tid = threadIdx.x, dir = blockIdx.y, tile = blockIdx.x;
    const int Hh = A.Hh, T = A.T, G4 = 4 * A.Hh;
    const int j = tid % A.JW, sg = tid / A.JW;
    const int lane = tid & 63, wave = tid >> 6, wpg = A.JW >> 6;                    // wpg: waves per sentence group
    const bool jv = j < Hh;
    const int lmax = tile_lengths(A, lengths, perm, tile, s_len, s_n);
    const int* my_n = s_n + sg * RS;
    const float* __restrict__ w = dir ? w1 : w0;                                    // [4 Hh][Hh]
    float dh_rec[RS], dc_rec[RS], dpl[RS];
    int amx[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        dh_rec[r] = 0.f; dc_rec[r] = 0.f; dpl[r] = 0.f; amx[r] = -1;
        const long n = my_n[r];
        if (jv && n >= 0) {
            amx[r] = argmax[n * 2L * Hh + dir * Hh + j];
            dpl[r] = d_pooled[n * 2L * Hh + dir * Hh + j];
        }
    }

    for (int s = lmax - 1; s >= 0; --s) {
        float p[RS];
#pragma unroll
        for (int r = 0; r < RS; ++r) p[r] = 0.f;
        if (jv) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int len = s_len[sg * RS + r];
                float* dgr = dg + (sg * RS + r) * G4 + j;
                if (s < len) {
                    const int t = dir ? len - 1 - s : s;
                    const long pos = (long)my_n[r] * T + t;
                    const float* gp = gates + pos * 8L * Hh + (long)dir * 4 * Hh + j;
                    const float gi = gp[0], gf = gp[Hh], gg = gp[2 * Hh], go = gp[3 * Hh];
                    const float ct = cs[pos * 2L * Hh + dir * Hh + j];
                    const float cp = (s > 0) ? cs[(pos + (dir ? 1 : -1)) * 2L * Hh + dir * Hh + j] : 0.f;
                    float dh = dh_rec[r];
                    if (amx[r] == t) dh += dpl[r];
                    const LstmDpre d = lstm_dpre(gi, gf, gg, go, ct, cp, dh, dc_rec[r]);
                    const float* xp = xw + pos * 8L * Hh + (long)dir * 4 * Hh + j;
                    p[r] = fmaf(d.ao, xp[3 * Hh], fmaf(d.ag, xp[2 * Hh], fmaf(d.af, xp[Hh], d.ai * xp[0])));
                    dgr[0] = d.ai; dgr[Hh] = d.af; dgr[2 * Hh] = d.ag; dgr[3 * Hh] = d.ao;
                } else {
                    dgr[0] = 0.f; dgr[Hh] = 0.f; dgr[2 * Hh] = 0.f; dgr[3 * Hh] = 0.f;
                }
            }
        }
        wave_sum_n(p, 64);                      // every lane of every wave is here: lmax is the workgroup's
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < RS; ++r) red[wave * RS + r] = p[r];
        }
        __syncthreads();
        if (tid < A.TS && s < s_len[tid]) {     // sentence slot tid = group tid / RS, row tid % RS: its waves in wave order
            const float* rp = red + (tid / RS) * wpg * RS + tid % RS;
            float v = rp[0];
            for (int k = 1; k < wpg; ++k) v += rp[k * RS];
            const int len = s_len[tid];
            words_out[((long)s_n[tid] * T + (dir ? len - 1 - s : s)) * 2 + dir] = v;
        }
        if (jv && s > 0) lstm_dh_prev<RS>(Hh, G4, j, w, dg, sg * RS, dh_rec);
        __syncthreads();
    }
    for (int e = tid; e < A.TS * T; e += blockDim.x) {                    // behind the sentence's end (and empty rows): zeros
        const int slot = e / T, t = e % T;
        const long n = s_n[slot];
        if (n >= 0 && t >= s_len[slot]) words_out[(n * T + t) * 2 + dir] = 0.f;
    }
}

// the workgroup shape for Hh: lanes along the hidden units in whole waves, the rest of the 256 threads along the sentences
static bool lstm_args(const char* what, int32_t N, int32_t T, int32_t Hh, LstmArgs& A, int& rs) {
    if (N < 0 || T < 1 || Hh < 1) { set_error("%s: bad sizes N=%d T=%d Hh=%d", what, N, T, Hh); return false; }
    A.N = N; A.T = T; A.Hh = Hh;
    A.HP = (Hh + 3) & ~3;
    A.JW = (Hh + 63) & ~63;
    A.nsg = std::max(1, 256 / A.JW);
    rs = (16L * A.nsg * 4 * Hh * 4 <= 49152) ? 16 : 8;      // 16 sentences per thread while the backward's LDS tile stays within 48 KB
    A.TS = rs * A.nsg;
    A.tout_per_seq = 0;
    return true;
}
static int lstm_refuse(const char* what, int32_t T, int32_t Hh) {
    if (T > kLstmMaxT) { set_error("%s: T=%d > %d (the reference clamps sentence lengths there)", what, T, kLstmMaxT); return RBR_ERR_UNSUPPORTED; }
    if (Hh > kLstmMaxH) { set_error("%s: Hh=%d > %d hidden units per direction", what, Hh, kLstmMaxH); return RBR_ERR_UNSUPPORTED; }
    return 0;
}
// saved state: gates [N,T,8Hh] | c [N,T,2Hh] | h_{t-1} [N,T,2Hh] | wt [2,HP,4Hh] | perm [N rounded up to 64]
struct LstmSaved { float *gates, *cs, *hprev, *wt; int* perm; size_t bytes; };
static LstmSaved lstm_saved(void* base, long N, long T, long Hh) {
    const long HP = (Hh + 3) & ~3L;
    char* p = static_cast<char*>(base);
    LstmSaved S;
    size_t o = 0;
    S.gates = reinterpret_cast<float*>(p + o); o += align256((size_t)N * T * 8 * Hh * 4);
    S.cs = reinterpret_cast<float*>(p + o); o += align256((size_t)N * T * 2 * Hh * 4);
    S.hprev = reinterpret_cast<float*>(p + o); o += align256((size_t)N * T * 2 * Hh * 4);
    S.wt = reinterpret_cast<float*>(p + o); o += align256((size_t)2 * HP * 4 * Hh * 4);
    S.perm = reinterpret_cast<int*>(p + o); o += align256((size_t)((N + 63) & ~63L) * 4);      // every tile size divides 64
    S.bytes = o;
    return S;
}

}  // namespace rbr

using namespace rbr;

extern "C" size_t rbr_lstm_seq_ws_bytes(int32_t N, int32_t T, int32_t Hh) {
    if (N < 0 || T < 1 || Hh < 1) return 0;
    return lstm_saved(nullptr, N, T, Hh).bytes;
}

extern "C" size_t rbr_lstm_seq_bwd_ws_bytes(int32_t N, int32_t T, int32_t Hh) {
    if (N < 1 || T < 1 || Hh < 1) return 0;
    return align256(gemm_strided_ws_floats(4 * Hh, Hh, (int)std::min<long>((long)N * T, 0x7fffffff)) * sizeof(float)) + 256;
}

extern "C" int rbr_lstm_seq_fwd(int32_t N, int32_t T, int32_t Hh, const float* xproj, const float* w_hh_fwd, const float* w_hh_rev,
                                const int64_t* lengths, const int32_t* t_out, int32_t t_out_per_seq, float* out, float* pooled,
                                int32_t* argmax, void* saved, void* stream) {
    LstmArgs A;
    int rs;
    if (!lstm_args("rbr_lstm_seq_fwd", N, T, Hh, A, rs)) return RBR_ERR_BAD_ARG;
    if (int e = lstm_refuse("rbr_lstm_seq_fwd", T, Hh)) return e;
    if (N == 0) return 0;
    if (!xproj || !w_hh_fwd || !w_hh_rev || !lengths || !saved) { set_error("rbr_lstm_seq_fwd: null pointer"); return RBR_ERR_BAD_ARG; }
    if (!out && !pooled) { set_error("rbr_lstm_seq_fwd: neither out nor pooled is asked for"); return RBR_ERR_BAD_ARG; }
    if (pooled && (!argmax || !t_out)) { set_error("rbr_lstm_seq_fwd: pooled needs argmax and the device scalar t_out"); return RBR_ERR_BAD_ARG; }
    if ((long)N * T > 0x7fffffffL / (8L * Hh)) { set_error("rbr_lstm_seq_fwd: N * T * 8 Hh exceeds 2^31 elements"); return RBR_ERR_UNSUPPORTED; }
    A.tout_per_seq = t_out_per_seq ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    LstmSaved S = lstm_saved(saved, N, T, Hh);
    float* wt = S.wt;
    const long nwt = 2L * A.HP * 4 * Hh;
    hipLaunchKernelGGL(lstm_wt_kernel, dim3((unsigned)std::min<long>((nwt + 255) / 256, 1024)), dim3(256), 0, st, Hh, A.HP, w_hh_fwd,
                       w_hh_rev, wt);
    RBR_CHECK_LAUNCH("lstm weight transpose launch");
    const dim3 grid((unsigned)((N + A.TS - 1) / A.TS), 2), block((unsigned)(A.JW * A.nsg));
    hipLaunchKernelGGL(lstm_perm_kernel, dim3(1), dim3(1024), 0, st, (int)N, (int)T, (int)(grid.x * A.TS), reinterpret_cast<const long long*>(lengths),
                       S.perm);
    RBR_CHECK_LAUNCH("lstm length sort launch");
    const size_t lds = (size_t)2 * A.TS * A.HP * sizeof(float) + (size_t)2 * A.TS * sizeof(int);
    const long long* len64 = reinterpret_cast<const long long*>(lengths);
    if (rs == 16)
        hipLaunchKernelGGL(lstm_fwd_kernel<16>, grid, block, lds, st, A, xproj, wt, len64, S.perm, t_out, out, pooled, argmax, S.gates, S.cs, S.hprev);
    else
        hipLaunchKernelGGL(lstm_fwd_kernel<8>, grid, block, lds, st, A, xproj, wt, len64, S.perm, t_out, out, pooled, argmax, S.gates, S.cs, S.hprev);
    RBR_CHECK_LAUNCH("lstm forward launch");
    return 0;
}

extern "C" int rbr_lstm_seq_bwd(int32_t N, int32_t T, int32_t Hh, const float* w_hh_fwd, const float* w_hh_rev, const int64_t* lengths,
                                const void* saved, const float* d_out, const float* d_pooled, const int32_t* argmax, float* d_xproj,
                                float* d_w_hh_fwd, float* d_w_hh_rev, void* ws, void* stream) {
    LstmArgs A;
    int rs;
    if (!lstm_args("rbr_lstm_seq_bwd", N, T, Hh, A, rs)) return RBR_ERR_BAD_ARG;
    if (int e = lstm_refuse("rbr_lstm_seq_bwd", T, Hh)) return e;
    if (!d_w_hh_fwd || !d_w_hh_rev) { set_error("rbr_lstm_seq_bwd: null weight gradient"); return RBR_ERR_BAD_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                              // nothing was summed: the weight gradients are zero
        if (int e = zero_words(d_w_hh_fwd, (size_t)4 * Hh * Hh * 4, st)) return e;
        return zero_words(d_w_hh_rev, (size_t)4 * Hh * Hh * 4, st);
    }
    if (!w_hh_fwd || !w_hh_rev || !lengths || !saved || !d_xproj || !ws) { set_error("rbr_lstm_seq_bwd: null pointer"); return RBR_ERR_BAD_ARG; }
    if (!d_out && !d_pooled) { set_error("rbr_lstm_seq_bwd: neither d_out nor d_pooled is given"); return RBR_ERR_BAD_ARG; }
    if (d_pooled && !argmax) { set_error("rbr_lstm_seq_bwd: d_pooled needs the forward's argmax"); return RBR_ERR_BAD_ARG; }
    if ((long)N * T > 0x7fffffffL / (8L * Hh)) { set_error("rbr_lstm_seq_bwd: N * T * 8 Hh exceeds 2^31 elements"); return RBR_ERR_UNSUPPORTED; }
    LstmSaved S = lstm_saved(const_cast<void*>(saved), N, T, Hh);
    const dim3 grid((unsigned)((N + A.TS - 1) / A.TS), 2), block((unsigned)(A.JW * A.nsg));
    const size_t lds = (size_t)A.TS * 4 * Hh * sizeof(float) + (size_t)2 * A.TS * sizeof(int);
    const long long* len64 = reinterpret_cast<const long long*>(lengths);
    if (rs == 16)
        hipLaunchKernelGGL(lstm_bwd_kernel<16>, grid, block, lds, st, A, w_hh_fwd, w_hh_rev, len64, S.perm, S.gates, S.cs, d_out, d_pooled, argmax, d_xproj);
    else
        hipLaunchKernelGGL(lstm_bwd_kernel<8>, grid, block, lds, st, A, w_hh_fwd, w_hh_rev, len64, S.perm, S.gates, S.cs, d_out, d_pooled, argmax, d_xproj);
    RBR_CHECK_LAUNCH("lstm backward launch");
    // d W_hh[row][k] = sum over the positions p of d_xproj[p][dir * 4Hh + row] * h_{t-1}[p][dir * Hh + k]
    const int K = N * T;
    float* part = gemm_strided_ws_floats(4 * Hh, Hh, K) ? static_cast<float*>(ws) : nullptr;
    for (int dir = 0; dir < 2; ++dir) {
        if (int e = gemm_strided(4 * Hh, Hh, K, d_xproj + (long)dir * 4 * Hh, 1, 8L * Hh, S.hprev + (long)dir * Hh, 1, 2L * Hh,
                                 dir ? d_w_hh_rev : d_w_hh_fwd, Hh, part, st))
            return e;
    }
    return 0;
}

extern "C" int rbr_lstm_seq_saliency(int32_t N, int32_t T, int32_t Hh, const float* w_hh_fwd, const float* w_hh_rev, const int64_t* lengths,
                                     const void* saved, const float* xw, const float* d_pooled, const int32_t* argmax, float* words_out,
                                     void* stream) {
    LstmArgs A;
    int rs;
    if (!lstm_args("rbr_lstm_seq_saliency", N, T, Hh, A, rs)) return RBR_ERR_BAD_ARG;
    if (int e = lstm_refuse("rbr_lstm_seq_saliency", T, Hh)) return e;
    if (N == 0) return 0;
    if (!w_hh_fwd || !w_hh_rev || !lengths || !saved || !xw || !d_pooled || !argmax || !words_out) {
        set_error("rbr_lstm_seq_saliency: null pointer");
        return RBR_ERR_BAD_ARG;
    }
    if ((long)N * T > 0x7fffffffL / (8L * Hh)) { set_error("rbr_lstm_seq_saliency: N * T * 8 Hh exceeds 2^31 elements"); return RBR_ERR_UNSUPPORTED; }
    LstmSaved S = lstm_saved(const_cast<void*>(saved), N, T, Hh);
    const dim3 grid((unsigned)((N + A.TS - 1) / A.TS), 2), block((unsigned)(A.JW * A.nsg));
    // the backward's tile and tile lists, and one wave sum per wave and sentence row behind them
    const size_t lds = (size_t)A.TS * 4 * Hh * sizeof(float) + (size_t)2 * A.TS * sizeof(int) + (size_t)(block.x / 64) * rs * sizeof(float);
    const long long* len64 = reinterpret_cast<const long long*>(lengths);
    if (rs == 16)
        hipLaunchKernelGGL(lstm_saliency_kernel<16>, grid, block, lds, (hipStream_t)stream, A, w_hh_fwd, w_hh_rev, len64, S.perm, S.gates, S.cs, xw, d_pooled, argmax, words_out);
    else
        hipLaunchKernelGGL(lstm_saliency_kernel<8>, grid, block, lds, (hipStream_t)stream, A, w_hh_fwd, w_hh_rev, len64, S.perm, S.gates, S.cs, xw, d_pooled, argmax, words_out);
    RBR_CHECK_LAUNCH("lstm word saliency launch");
    return 0;
}
