"""Writes a tiny sentence split shaped like the reference's preprocess output (preprocess/divide_and_create_example_sent.py), for
the id-fed AHN tests.  The sentence-split counterpart of make_review_dataset:

  * a review in meta is RECTANGULAR: sent_num sentences of word_num word ids, zero-padded (create_meta, :203-245);
  * meta's per-id lists are RAGGED defaultdict-style dicts built from the train interactions in row order: an id has as many
    reviews as it wrote, and there is no key 0;
  * a TRAIN example is built by the reference's own list operations (:262-300): copy(), index() of the counterpart, pop(),
    truncate / pad to rv_num -- and carries the popped review as its 8th field;
  * a VALID example is the lists truncated / padded as they are (:301-340).

write_sentence_split lays the interactions out as make_review_dataset.write_review_split does (users with 1, R, R + 1 and R + 3
reviews; dropped indices 0, R - 1, R and > R; a user who reviewed one item twice; a valid pair whose user reviewed that item in the
train split) and plants, in the first reviews of the user with R + 1 of them: a review with an empty sentence between two non-empty
ones, a review whose sentences are all empty (its rid is a real item), and sentences of length 1 and of length word_num.  Every
call asserts that the layout holds all of that."""
import numpy as np

from make_review_dataset import _truncate_pad, dump_split


def _sentence(rng, vocab, W, n):
    """n word ids followed by W - n pads."""
    return [int(x) for x in rng.integers(2, vocab, size=n)] + [0] * (W - n)


def random_review(rng, vocab, S, W, holes=False):
    """An S x W review: a random number of non-empty sentences at random places (so empty sentences stand between live ones),
    each 1..W words long; with `holes`, a pad word may also stand INSIDE a sentence (a length is a count, not a prefix)."""
    rv = [[0] * W for _ in range(S)]
    for s in rng.choice(S, size=int(rng.integers(0, S + 1)), replace=False):
        sent = _sentence(rng, vocab, W, int(rng.integers(1, W + 1)))
        if holes and W > 2 and rng.random() < 0.3:
            sent[int(rng.integers(0, W - 1))] = 0
            sent[W - 1] = int(rng.integers(2, vocab))
        rv[int(s)] = sent
    return rv


def train_example(meta, uid, iid, rating, R, S, W):
    u_revs, u_rids = meta["user_reviews"][uid].copy(), meta["user_rids"][uid].copy()
    del_idx = meta["user_rids"][uid].index(iid)
    ui_rev = u_revs[del_idx]
    u_revs.pop(del_idx)
    u_rids.pop(del_idx)
    i_revs, i_rids = meta["item_reviews"][iid].copy(), meta["item_rids"][iid].copy()
    del_idx = meta["item_rids"][iid].index(uid)
    i_revs.pop(del_idx)
    i_rids.pop(del_idx)
    pad = [[0] * W] * S
    return [uid, iid, rating, _truncate_pad(u_revs, R, pad), _truncate_pad(i_revs, R, pad), _truncate_pad(u_rids, R, 0),
            _truncate_pad(i_rids, R, 0), ui_rev]


def valid_example(meta, uid, iid, rating, R, S, W):
    pad = [[0] * W] * S
    return [uid, iid, rating, _truncate_pad(meta["user_reviews"][uid].copy(), R, pad),
            _truncate_pad(meta["item_reviews"][iid].copy(), R, pad), _truncate_pad(meta["user_rids"][uid].copy(), R, 0),
            _truncate_pad(meta["item_rids"][iid].copy(), R, 0)]


def meta_from_rows(rows, reviews):
    """meta's four per-id dicts from the train interactions `rows` = [(u, i), ...] in row order, review k belonging to row k."""
    meta = {"user_reviews": {}, "item_reviews": {}, "user_rids": {}, "item_rids": {}}
    for (u, i), rv in zip(rows, reviews):
        meta["user_reviews"].setdefault(u, []).append(rv)
        meta["item_reviews"].setdefault(i, []).append(rv)
        meta["user_rids"].setdefault(u, []).append(i)
        meta["item_rids"].setdefault(i, []).append(u)
    return meta


def random_split(n_users, n_items, vocab, R, S, W, n_train, n_valid, seed=0):
    """An in-memory split of any shape: (meta dict with the sizes, train examples, valid examples) from n_train random
    interactions (repeated pairs included), reviews with holes."""
    rng = np.random.default_rng(seed)
    rows = [(int(rng.integers(1, n_users)), int(rng.integers(1, n_items))) for _ in range(n_train)]
    meta = meta_from_rows(rows, [random_review(rng, vocab, S, W, holes=True) for _ in rows])
    train = [train_example(meta, u, i, float(rng.integers(1, 6)), R, S, W) for u, i in rows]
    users, items = sorted(meta["user_reviews"]), sorted(meta["item_reviews"])
    valid = [valid_example(meta, int(rng.choice(users)), int(rng.choice(items)), float(rng.integers(1, 6)), R, S, W)
             for _ in range(n_valid)]
    return (dict(meta, user_num=n_users, item_num=n_items, rv_num=R, sent_num=S, word_num=W, vocab_size=vocab), train, valid)


def write_sentence_split(data_dir, n_users=12, n_items=10, vocab=60, rv_num=4, sent_num=3, word_num=5, n_valid=20, seed=0):
    """43 train interactions (= examples) and n_valid valid examples.  Returns the sizes, `pairs` and `dropped`: per train example
    the (user-side, item-side) index that index() found."""
    R, S, W = rv_num, sent_num, word_num
    assert n_users >= 12 and n_items >= R + 4 and R >= 3 and S >= 3 and W >= 2
    rng = np.random.default_rng(seed)
    per_user = {1: [1], 2: list(range(1, R + 1)), 3: list(range(1, R + 2)), 4: list(range(1, R + 4)), 5: [2, 2, 3]}
    for u, k in zip(range(6, 12), (2, 3, 6, 4, 5, 3)):
        per_user[u] = [int(x) for x in rng.choice(np.arange(1, n_items), size=k, replace=False)]
    cursor = {u: 0 for u in per_user}
    rows = []
    while len(rows) < sum(len(v) for v in per_user.values()):
        u = int(rng.choice([u for u in per_user if cursor[u] < len(per_user[u])]))
        rows.append((u, per_user[u][cursor[u]]))
        cursor[u] += 1

    reviews = [random_review(rng, vocab, S, W) for _ in rows]
    third = [k for k, (u, _) in enumerate(rows) if u == 3][:3]       # user 3's first three reviews: in every other example of its
    gap = [[0] * W for _ in range(S)]
    gap[0], gap[2] = _sentence(rng, vocab, W, 2), _sentence(rng, vocab, W, W - 1)
    ends = [[0] * W for _ in range(S)]
    ends[0], ends[1] = _sentence(rng, vocab, W, 1), _sentence(rng, vocab, W, W)
    reviews[third[0]], reviews[third[1]], reviews[third[2]] = gap, [[0] * W for _ in range(S)], ends

    meta = meta_from_rows(rows, reviews)
    train = [train_example(meta, u, i, float(rng.integers(1, 6)), R, S, W) for u, i in rows]
    items = sorted(meta["item_reviews"])
    valid_pairs = [(4, 1)] + [(int(rng.integers(1, 12)), int(rng.choice(items))) for _ in range(n_valid - 1)]
    valid = [valid_example(meta, u, i, float(rng.integers(1, 6)), R, S, W) for u, i in valid_pairs]

    dropped = [(meta["user_rids"][u].index(i), meta["item_rids"][i].index(u)) for u, i in rows]
    counts = {len(v) for v in meta["user_reviews"].values()}
    assert {1, R, R + 1, R + 3} <= counts and 0 not in meta["user_reviews"] and 0 not in meta["item_reviews"]
    du = {d for d, _ in dropped}
    assert {0, R - 1, R} <= du and max(du) > R
    assert rows.count((5, 2)) == 2 and 1 in meta["user_rids"][4]
    everything = [rv for v in meta["user_reviews"].values() for rv in v]
    assert all(len(rv) == S and all(len(s) == W for s in rv) for rv in everything)                      # rectangular
    live = lambda s: any(s)                                                                               # noqa: E731
    assert any(live(rv[a]) and not live(rv[a + 1]) and live(rv[a + 2]) for rv in everything for a in range(S - 2))
    mine = list(zip(meta["user_reviews"][3], meta["user_rids"][3]))
    assert any(not any(map(live, rv)) and rid != 0 for rv, rid in mine[:R])
    lengths = {sum(x != 0 for x in s) for rv in everything for s in rv}
    assert {1, W} <= lengths
    # ... and the examples show it: some train example holds the all-empty review, rid and all, in its R slots
    assert any(not any(map(live, rv)) and rid != 0 for e in train for rv, rid in zip(e[3], e[5]))

    dump_split(data_dir, dict(meta, user_num=n_users, item_num=n_items, rv_num=R, sent_num=S, word_num=W), vocab, train, valid)
    return dict(user_num=n_users, item_num=n_items, vocab=vocab, rv_num=R, sent_num=S, word_num=W, n_train=len(train),
                n_valid=len(valid), dropped=dropped, pairs=rows)
