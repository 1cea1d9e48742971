// lds_bucket.h -- group the rows of a workgroup's window by token in LDS, so that what the rows of one token add to the
// embedding table can be summed in the workgroup and leave it as ONE row of atomics per distinct token.
//
// Users: gate_bwd_dx_kernel (datt_gates.hip), bag_bwd_bucket_kernel (review_bag.hip), dx_window_kernel (textcnn_bwd.hip).
// Workgroups of kBucketThreads threads.  The arrays are the caller's own __shared__ arrays (each kernel keeps its LDS layout).
//
// Contract -- what each array holds after each step, n = rows of the window, s_tok[r] < 0 = absent row (masked, padding, outside):
//   bucket_hash_clear   s_hkey[0..HASH) = -1 (empty), s_hval[0..HASH) = kBucketNoRow.            Barrier: the caller's, before
//                       bucket_leaders (it is the one behind the caller's own fill of s_tok and zeroing of s_fill).
//   bucket_leaders      s_hkey[slot] = token that owns the slot (open addressing, linear probe that wraps at HASH),
//                       s_hval[slot] = FIRST row of the window with that token,
//                       s_leader[r]  = that first row for the token of row r: rows with equal tokens share a leader, and a
//                                      leader leads itself.  An absent row gets -1, or r itself with SELF_LEADS.
//                       COUNT: s_fill[lead] += 1 per present row (s_fill zeroed by the caller beforehand).
//                       One barrier inside (between insert and resolve); NONE behind: the caller's next barrier covers it.
//   bucket_scan         (one wave; s_fill[key] = members of the group led by row `key`, 0 for a row that leads nothing)
//                       s_cnt[key] = s_fill[key], s_start[key] = exclusive prefix of the counts: group `key` owns
//                       s_sorted[s_start[key] .. + s_cnt[key]).  KEYS: s_keys[0..*s_nkeys) = the leaders with a non-empty
//                       group, ascending.  RESET_FILL: s_fill[0..n) = 0 again (the cursor of bucket_place_arrival).
//   bucket_place_*      s_sorted = the member indices, group by group.
//                       _ordered: members are the rows themselves and come out ASCENDING within a group (rank = number of earlier
//                       rows with the same leader; up to n LDS reads per row): sums over a group round the same on every run.
//                       _arrival: members (rows, or items that name a row) take the next free place of their group with an LDS
//                       atomicAdd on s_fill: O(1), but the order within a group differs from run to run, and so does the
//                       rounding of a float sum over it.
//   Each site keeps the placement it was written with: gate_bwd_dx_kernel is ordered (its row maps and tap sums are tested
//   for reproducibility), the bag and the conv window kernels are arrival-order.  Switching one of them changes results and
//   time; that is a decision of its own, not a clean-up.
//
// Assumptions: HASH is a power of two and n <= HASH / 2 (load factor <= 1/2: the probe ends, and stays short);
// n <= 32767 and member indices <= 32767 (short indices); tokens are non-negative ints.
#pragma once

#include "rbr_wave.h"

namespace rbr {

constexpr int kBucketThreads = 256;
constexpr int kBucketNoRow = 32767;      // above every row index

template <int HASH>
__device__ __forceinline__ void bucket_hash_clear(int* s_hkey, int* s_hval) {
    for (int k = threadIdx.x; k < HASH; k += kBucketThreads) { s_hkey[k] = -1; s_hval[k] = kBucketNoRow; }
}

template <int HASH, bool SELF_LEADS, bool COUNT>
__device__ __forceinline__ void bucket_leaders(const int* s_tok, int n, int* s_hkey, int* s_hval, short* s_leader, int* s_fill) {
    static_assert(HASH > 1 && (HASH & (HASH - 1)) == 0, "HASH must be a power of two");
    const int tid = threadIdx.x;
    for (int r = tid; r < n; r += kBucketThreads) {
        const int t = s_tok[r];
        int slot = -1;
        if (t >= 0) {
            unsigned hh = ((unsigned)t * 2654435761u) >> (32 - __builtin_ctz(HASH));      // the top log2(HASH) bits
            for (;;) {
                const int old = atomicCAS(&s_hkey[hh], -1, t);
                if (old == -1 || old == t) break;
                hh = (hh + 1) & (HASH - 1);
            }
            atomicMin(&s_hval[hh], r);
            slot = (int)hh;
        }
        s_leader[r] = (short)slot;       // temporarily the hash slot
    }
    __syncthreads();
    for (int r = tid; r < n; r += kBucketThreads) {
        const int slot = s_leader[r];
        const int lead = slot >= 0 ? s_hval[slot] : (SELF_LEADS ? r : -1);
        s_leader[r] = (short)lead;
        if (COUNT && lead >= 0) atomicAdd(&s_fill[lead], 1);
    }
}

// run by ONE wave (lane = its lane index); s_keys / s_nkeys are not touched without KEYS
template <bool KEYS, bool RESET_FILL>
__device__ __forceinline__ void bucket_scan(int lane, int* s_fill, int n, short* s_start, short* s_cnt, short* s_keys, int* s_nkeys) {
    int run = 0, krun = 0;
    for (int r0 = 0; r0 < n; r0 += 64) {
        const int r = r0 + lane;
        const int c = (r < n) ? s_fill[r] : 0;
        const int inc = wave_incl_scan(c, lane);
        const int kinc = KEYS ? wave_incl_scan(c > 0 ? 1 : 0, lane) : 0;
        if (r < n) {
            s_start[r] = (short)(run + inc - c);
            s_cnt[r] = (short)c;
            if (RESET_FILL) s_fill[r] = 0;
            if (KEYS && c > 0) s_keys[krun + kinc - 1] = (short)r;
        }
        run += __shfl(inc, 63);
        if (KEYS) krun += __shfl(kinc, 63);
    }
    if (KEYS && lane == 0) *s_nkeys = krun;
}

__device__ __forceinline__ void bucket_place_ordered(const short* s_leader, int n, const short* s_start, short* s_sorted) {
    for (int r = threadIdx.x; r < n; r += kBucketThreads) {
        const int lead = s_leader[r];
        if (lead >= 0) {
            int rank = 0;
            for (int q = lead; q < r; ++q) rank += (s_leader[q] == lead);      // lead is the group's first row: the walk starts there
            s_sorted[s_start[lead] + rank] = (short)r;
        }
    }
}

// key_of(m): leader of member m of [0, n_members), or < 0 for a member that belongs to no group
template <class KeyOf>
__device__ __forceinline__ void bucket_place_arrival(int n_members, KeyOf key_of, const short* s_start, int* s_fill, short* s_sorted) {
    for (int m = threadIdx.x; m < n_members; m += kBucketThreads) {
        const int key = key_of(m);
        if (key >= 0) s_sorted[s_start[key] + atomicAdd(&s_fill[key], 1)] = (short)m;
    }
}

}  // namespace rbr
