// item_csr.h -- "which items does this row list?", stated once: the CSR of items a user has seen / a row must not be offered, as
// rbr_pair_score_topk / rbr_pair_score_rank (exclusion list), rbr_sample_negatives / rbr_sample_hard_negatives and
// rbr_pair_softmax_* (seen list) take it.  THE RULE for a malformed list: no offset can send a reader outside item[0 .. nnz) --
// a row's [a, e) is clamped to [0, nnz] and e raised to a -- and a row outside [0, rows) lists nothing.
//
// Every caller gets the same answers from csr_row / csr_has as from the code it had of its own:
//   * topk (`excluded`): lower-bound search of [a, e); it had no "e raised to a", which its loop did not need (empty for
//     e <= a), and compared 32-bit items -- an int item id sign-extends to the 64-bit compare used here.
//   * rank_finish_kernel: bounds only, then a lane-strided walk of [a, e), empty for e <= a as well.
//   * the two samplers and the softmax: this text, with rows = U, no row[] indirection and a raw int64 id to look up.
#pragma once

#include "rbr_common.h"

namespace rbr {

struct ItemCsr {                 // by value inside a kernel's argument struct
    const long long* off;        // [rows + 1], or null: no list at all
    const int* item;             // [nnz], ascending within a row
    const long long* row;        // the caller's row r reads row row[r] of `off`, or null (= r)
    long long nnz;
    int rows;
};

// [a, e) of C.item that serves the caller's row r.  false and a = e = 0: there is no list, or the row lies outside [0, rows).
__device__ __forceinline__ bool csr_row(const ItemCsr& C, long long r, long long& a, long long& e) {
    a = e = 0;
    if (C.off == nullptr) return false;
    if (C.row != nullptr) r = C.row[r];
    if ((unsigned long long)r >= (unsigned long long)C.rows) return false;
    a = C.off[r]; e = C.off[r + 1];
    a = a < 0 ? 0 : a;
    e = e > C.nnz ? C.nnz : e;
    if (e < a) e = a;            // (a > nnz only ever with e == a: nothing is read)
    return true;
}

// whether item[a .. e) (ascending) holds x: lower bound, 64-bit compare (the softmax looks up a raw int64 id)
__device__ __forceinline__ bool csr_has(const int* __restrict__ item, long long a, long long e, long long x) {
    long long lo = a, hi = e;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)item[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < e && (long long)item[lo] == x;
}

// The one argument check of the five entries, before any launch; 0 or RBR_ERR_BAD_ARG with the error text set.  seen: the list
// of the samplers and the softmax (no row[]; a list needs rows >= 1); else the exclusion list of topk / rank (row[] with its
// own row count).
inline int item_csr_ok(const char* who, bool seen, const void* off, const void* item, long long nnz, const void* row, int rows) {
    if ((off != nullptr) != (item != nullptr) || nnz < 0 || (!off && (nnz != 0 || row)) || (seen && off && rows <= 0)) {
        set_error(seen ? "%s: the seen list is seen_off [U + 1] AND seen_item [seen_nnz] with U >= 1, or neither"
                       : "%s: the exclusion list is excl_off [rows + 1] AND excl_item [excl_nnz], or neither", who);
        return RBR_ERR_BAD_ARG;
    }
    if (row && rows <= 0) { set_error("%s: excl_row with excl_rows=%d", who, rows); return RBR_ERR_BAD_ARG; }
    return 0;
}

inline ItemCsr item_csr(const int64_t* off, const int32_t* item, const int64_t* row, int64_t nnz, int rows) {
    return ItemCsr{reinterpret_cast<const long long*>(off), item, reinterpret_cast<const long long*>(row), nnz, rows};
}

}  // namespace rbr
