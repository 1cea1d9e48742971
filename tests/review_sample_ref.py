"""Integer restatement of rbr_review_sample_gather's draw (include/rbr_hip.h) in numpy, shared by the review sampler's host and
GPU tests.  Written from the header's six steps, on bpr_ref's Philox; it shares no code with data.py's cpu path."""
import numpy as np

from bpr_ref import philox4x32_10


def keys(rows, P, call, seed):
    """key(q) of step 4 for every row of `rows` (ints) and q in [0, P): uint64 [len(rows), P], each below 2^32."""
    e = np.asarray(rows, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(P, dtype=np.uint64)[None, :]
    words = philox4x32_10(e >> np.uint64(2), call, seed)
    out = np.zeros_like(e)
    for w in range(4):
        out = np.where((e & np.uint64(3)) == np.uint64(w), words[w], out)
    return out


def chosen(live, n, rows, call, seed):
    """Step 5 for a matrix of live flags [len(rows), P]: the candidates q that land in output slots 0 .. n - 1 of every row, in
    order, -1 where the row has fewer live candidates: int64 [len(rows), n]."""
    live = np.asarray(live, dtype=bool)
    P = live.shape[1]
    key = keys(rows, P, call, seed)
    qs = np.broadcast_to(np.arange(P), live.shape)
    # (key ascending, q ascending) among the live; the dead sort behind every 32-bit key
    order = np.lexsort((qs, np.where(live, key, np.uint64(1) << np.uint64(32))), axis=1)
    out = np.full((live.shape[0], n), -1, dtype=np.int64)
    w = min(n, P)
    out[:, :w] = np.where(np.arange(w)[None, :] < live.sum(1)[:, None], order[:, :w], -1)
    return out


def gather_ref(u_ids, i_ids, user_revs, user_rids, item_revs, item_rids, R, n_user, n_item, seed, call, leave_one_out=True,
               pad=0, replace_id=0):
    """All outputs of one launch with call number `call`, as numpy arrays: revs int64 [2B, R, T], word_masks / rev_masks bool,
    rids int64 [2B, R], ids int64 [2B], slots int32 [2B, R]; and `bad`, the number of own ids outside their table."""
    u_ids, i_ids = np.asarray(u_ids, dtype=np.int64), np.asarray(i_ids, dtype=np.int64)
    tabs = ((np.asarray(user_revs), np.asarray(user_rids)), (np.asarray(item_revs), np.asarray(item_rids)))
    B, P, T = len(u_ids), tabs[0][0].shape[1] - 1, tabs[0][0].shape[2]
    revs = np.full((2 * B, R, T), pad, dtype=np.int64)
    rids = np.zeros((2 * B, R), dtype=np.int64)
    slots = np.full((2 * B, R), -1, dtype=np.int32)
    ids = np.zeros(2 * B, dtype=np.int64)
    live = np.zeros((2 * B, P), dtype=bool)
    src = np.zeros((2 * B, P), dtype=np.int64)
    own_of = np.zeros(2 * B, dtype=np.int64)
    bad = 0
    for r in range(2 * B):
        s = 0 if r < B else 1
        b = r - s * B
        a, c = ((u_ids[b], i_ids[b]), (i_ids[b], u_ids[b]))[s]
        tab, rid = tabs[s]
        if not 0 <= a < tab.shape[0]:
            a, bad = replace_id, bad + 1
        ids[r] = own_of[r] = a
        d = P                                                                    # step 1
        if leave_one_out and 0 < c < tabs[s ^ 1][0].shape[0]:
            for j in range(P):
                if rid[a, j] == c:
                    d = j
                    break
        for q in range(P):                                                       # steps 2, 3
            src[r, q] = q + (q >= d)
            live[r, q] = bool((tab[a, src[r, q]] != pad).any())
    n_of = np.where(np.arange(2 * B) < B, n_user, n_item)
    pick = chosen(live, R, np.arange(2 * B), call, seed)                         # steps 4, 5
    for r in range(2 * B):
        s = 0 if r < B else 1
        tab, rid = tabs[s]
        for k in range(R):
            q = pick[r, k]
            if q >= 0 and k < n_of[r]:
                slots[r, k] = src[r, q]
                revs[r, k] = tab[own_of[r], src[r, q]]
                rids[r, k] = rid[own_of[r], src[r, q]]
    wm = revs != pad                                                             # step 6: the rest stays empty
    return dict(revs=revs, word_masks=wm, rev_masks=slots >= 0, rids=rids, ids=ids, slots=slots, bad=bad)


def random_tables(rng, N, P, T, V=40):
    """Random pool tables of one side, int32: ragged lists (0 .. P + 1 reviews), some reviews empty, row 0 all pad."""
    revs = np.zeros((N, P + 1, T), dtype=np.int32)
    rids = np.zeros((N, P + 1), dtype=np.int32)
    for a in range(1, N):
        k = int(rng.integers(0, P + 2))
        rids[a, :k] = rng.integers(1, N, size=k)
        revs[a, :k] = rng.integers(1, V, size=(k, T))
        revs[a, :k][rng.random(k) < 0.25] = 0                   # an empty review keeps its rid
    return revs, rids
