// rbr_rng.h -- the device-side random numbers of librbr_hip.so, stated once: Philox4x32-10, THE dropout draw of one element, and
// the protocol of the call number that lives in device memory.
//   draw    : element e of call number `call` under `seed` is word (e & 3) of the Philox block with counter (e >> 2, call); kept
//             iff dropout_keep, multiplier 1 / (1 - p).  rbr_dropout_multiplier writes it for every element of a tensor; the head
//             forward and the in-batch softmax draw single elements of the same tensor in their kernels (dropout_draw): one
//             function, so "exactly what rbr_dropout_multiplier writes" (include/rbr_hip.h) holds by construction.
//   protocol: state[0] is the call number, state[1] a ticket that is zero between launches.  Every workgroup of a launch reads
//             state[0] first; the last one to take a ticket advances it (rng_advance_call), so a launch recorded into a hipGraph
//             draws a new set on every replay.  (The tickets that PUBLISH data -- the MSE loss of pair_head.hip, the lists of
//             textcnn_prod.hip -- carry fences and are a different protocol.)
#pragma once

#include <hip/hip_runtime.h>

namespace rbr {

__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__device__ __forceinline__ void philox4x32_10(unsigned long long quad, unsigned long long call, unsigned long long seed,
                                              unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3) {
    c0 = (unsigned)quad; c1 = (unsigned)(quad >> 32); c2 = (unsigned)call; c3 = (unsigned)(call >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ bool dropout_keep(unsigned word, float p) {      // u in [0,1) from the top 24 bits; keep iff u >= p
    return (float)(word >> 8) * (1.f / 16777216.f) >= p;
}
// a drawn word's multiplier (dropout_mult_kernel: one Philox block serves four elements)
__device__ __forceinline__ float dropout_word_mult(unsigned word, float p) { return dropout_keep(word, p) ? 1.f / (1.f - p) : 0.f; }

// THE draw of element e
__device__ __forceinline__ float dropout_draw(unsigned long long e, unsigned long long call, unsigned long long seed, float p) {
    unsigned w[4];
    philox4x32_10(e >> 2, call, seed, w[0], w[1], w[2], w[3]);
    return dropout_word_mult(w[e & 3], p);
}

// The ticket, called by ONE thread of every workgroup of the launch.  Contract: every thread of the workgroup has consumed `call`
// (= state[0], read by this launch) and a workgroup barrier lies between those reads and this call, so the workgroup that takes
// the last ticket knows every read of state[0] done.  Nothing else is published through the ticket: no fence.
__device__ __forceinline__ void rng_advance_call(unsigned long long* state, unsigned long long call) {
    if (atomicAdd(state + 1, 1ull) == (unsigned long long)gridDim.x - 1) {
        state[1] = 0;
        state[0] = call + 1;
    }
}

}  // namespace rbr
