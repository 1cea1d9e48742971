"""Integer restatement of rbr_sample_negatives' draw (include/rbr_hip.h) in numpy, shared by the sampler's host and GPU tests:
Philox4x32-10 as csrc/rbr_rng.h states it, the candidate mapping, the accept rule and the cyclic walk."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
K0, K1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(quad, call, seed):
    """The four 32-bit words of the block with counter (quad, call) under key `seed`: quad a uint64 array, call / seed ints."""
    quad = np.asarray(quad, dtype=np.uint64)
    c0, c1 = quad & LO, quad >> S32
    c2 = np.full_like(quad, call & 0xFFFFFFFF)
    c3 = np.full_like(quad, (call >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + K0) & 0xFFFFFFFF, (k1 + K1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def seen_sets(seen, n_users):
    """user id -> set of seen items from a CSR (off [U + 1], items); {} for None."""
    if seen is None:
        return {}
    off, items = (np.asarray(t) for t in seen)
    return {u: set(int(x) for x in items[off[u]:off[u + 1]]) for u in range(min(n_users, len(off) - 1))}


def sample_negatives_ref(u_ids, i_ids, n_neg, n_items, seen, seed, call, item_lo=1, max_tries=16, replace_id=0, stats=None):
    """(u_out, i_out int64 [(1 + n_neg) * B], valid f32 [n_neg * B]) of call number `call`.  `stats` (a dict) receives
    "attempts" (the most attempts any draw made) and "walks" (the draws that took the walk)."""
    u_ids, i_ids = np.asarray(u_ids, dtype=np.int64), np.asarray(i_ids, dtype=np.int64)
    B = len(u_ids)
    n_users = 0 if seen is None else len(seen[0]) - 1
    rows = seen_sets(seen, n_users)
    span = n_items - item_lo
    n = B * n_neg
    d = np.arange(n, dtype=np.uint64)
    b_of = (np.arange(n) // n_neg)
    pos = i_ids[b_of]
    row_of = [rows.get(int(u), set()) if 0 <= int(u) < n_users else set() for u in u_ids]

    def ok(k, c):
        return c != int(pos[k]) and c not in row_of[int(b_of[k])]

    cand = np.full(n, item_lo, dtype=np.int64)
    found = np.zeros(n, dtype=bool)
    words = None
    attempts = 0
    for t in range(max_tries):
        act = np.flatnonzero(~found)
        if act.size == 0:
            break
        attempts = t + 1
        if t % 4 == 0:
            words = np.stack(philox4x32_10(d * np.uint64(16) + np.uint64(t >> 2), call, seed))
        c = item_lo + ((words[t & 3][act] * np.uint64(span)) >> S32).astype(np.int64)
        cand[act] = c
        found[act] = [ok(int(k), int(x)) for k, x in zip(act, c)]
    walks = np.flatnonzero(~found)
    for k in walks:
        c = int(cand[k])
        for _ in range(span):
            c = item_lo + (c - item_lo + 1) % span
            if ok(int(k), c):
                cand[k], found[k] = c, True
                break
    if stats is not None:
        stats["attempts"], stats["walks"] = attempts, int(walks.size)
    j_of = np.arange(n) % n_neg
    u_out = np.empty((1 + n_neg) * B, dtype=np.int64)
    i_out = np.empty((1 + n_neg) * B, dtype=np.int64)
    valid = np.empty(n_neg * B, dtype=np.float32)
    u_out[:B], i_out[:B] = u_ids, i_ids
    r = (j_of + 1) * B + b_of
    u_out[r] = u_ids[b_of]
    i_out[r] = np.where(found, cand, replace_id)
    valid[j_of * B + b_of] = found.astype(np.float32)
    return u_out, i_out, valid
