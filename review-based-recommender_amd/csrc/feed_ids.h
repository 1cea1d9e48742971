// feed_ids.h -- the id convention of the id-fed batches (doc_feed.hip, review_feed.hip): the stacked output has 2B rows, user
// rows first; row r reads the id of its side, an id outside its table is never dereferenced -- row `replace` stands in for it,
// ids_out gets `replace`, and err is updated as rbr::sanitize_id does (err[0] count, err[1] one offending value, err[2] its set:
// 0 = u_ids, 1 = i_ids).
// The leave-one-out slot of the review gathers (review_feed.hip, sentence_feed.hip) is stated here too: feed_dropped_slot.
#pragma once

#include "rbr_common.h"

namespace rbr {

struct FeedIds {
    const long long* ids[2];
    long long rows[2];
    long long* ids_out;
    long long replace;
    int B;
};

// row r of the stacked output -> its side, its checked id; the lane that owns the row's first token records a bad id
__device__ __forceinline__ long long feed_row_id(const FeedIds& F, int r, int& side, bool first_lane, long long* __restrict__ err) {
    side = r >= F.B ? 1 : 0;
    long long v = F.ids[side][r - side * F.B];
    if ((unsigned long long)v >= (unsigned long long)F.rows[side]) {
        if (first_lane) {
            err[1] = v; err[2] = side;                // any one offender (benign race)
            atomicAdd(reinterpret_cast<unsigned long long*>(err), 1ull);
        }
        v = F.replace;
    }
    if (first_lane && F.ids_out) F.ids_out[r] = v;
    return v;
}

// the slot that row r's example leaves out of its id's list: d = the first j in [0, R) with rid_row[j] == c, c the other side's id
// of the pair, when `loo` and 0 < c < rows of the other side (rid 0 is the pad, id 0 the padding id: neither ever matches); else
// d = R.  Output slot q then reads table slot q + (q >= d).  rid_row: the R + 1 counterpart ids of the row's own (checked) id.
__device__ __forceinline__ int feed_dropped_slot(const FeedIds& F, const int* __restrict__ rid_row, int r, int side, int R, int loo) {
    int d = R;
    if (loo) {
        const long long c = F.ids[side ^ 1][r - side * F.B];
        if (c > 0 && c < F.rows[side ^ 1]) {
            for (int j = R - 1; j >= 0; --j)          // no early exit: the R loads are independent of each other
                d = (long long)rid_row[j] == c ? j : d;
        }
    }
    return d;
}

}  // namespace rbr
