"""Writes a tiny review split shaped like the reference's preprocess output (preprocess/divide_and_create_example_word.py), for
the id-fed review tests.  Unlike make_dataset.write_review_split, whose meta is rectangular and whose examples are meta's rows:

  * meta's per-id lists are RAGGED defaultdict-style dicts built from the train interactions in row order (create_meta, :216-229):
    an id has as many reviews as it wrote, and there is no key 0;
  * a TRAIN example is built by the reference's own list operations (:263-287): copy(), index() of the counterpart, pop(),
    truncate / pad to rv_num -- and carries the popped review as its 8th field;
  * a VALID example is the lists truncated / padded as they are (:306-325).

The interactions are laid out so that the split contains, for rv_num = R: users with 1, R, R + 1 and R + 3 reviews; train pairs
whose dropped index is 0, R - 1, R and > R; a user who reviewed one item twice (index() finds the first); and a valid pair whose
user also reviewed that item in the train split (nothing is dropped from a valid example)."""
import os
import pickle

import numpy as np

from make_dataset import _fake_module


def _truncate_pad(xs, n, pad):
    xs = xs[:n]
    return xs + [pad] * (n - len(xs))


def train_example(meta, uid, iid, rating, rv_num, rv_len):
    u_revs, u_rids = meta["user_reviews"][uid].copy(), meta["user_rids"][uid].copy()
    del_idx = meta["user_rids"][uid].index(iid)
    ui_rev = u_revs[del_idx]
    u_revs.pop(del_idx)
    u_rids.pop(del_idx)
    i_revs, i_rids = meta["item_reviews"][iid].copy(), meta["item_rids"][iid].copy()
    del_idx = meta["item_rids"][iid].index(uid)
    i_revs.pop(del_idx)
    i_rids.pop(del_idx)
    pad = [0] * rv_len
    return [uid, iid, rating, _truncate_pad(u_revs, rv_num, pad), _truncate_pad(i_revs, rv_num, pad),
            _truncate_pad(u_rids, rv_num, 0), _truncate_pad(i_rids, rv_num, 0), ui_rev]


def valid_example(meta, uid, iid, rating, rv_num, rv_len):
    pad = [0] * rv_len
    return [uid, iid, rating, _truncate_pad(meta["user_reviews"][uid].copy(), rv_num, pad),
            _truncate_pad(meta["item_reviews"][iid].copy(), rv_num, pad), _truncate_pad(meta["user_rids"][uid].copy(), rv_num, 0),
            _truncate_pad(meta["item_rids"][iid].copy(), rv_num, 0)]


def meta_from_rows(rows, vocab, rv_len, rng):
    """meta's four per-id dicts from the train interactions `rows` = [(u, i), ...] in row order (create_meta, :216-229), one
    random right-padded review per row; also a rating per row."""
    meta = {"user_reviews": {}, "item_reviews": {}, "user_rids": {}, "item_rids": {}}
    ratings = []
    for u, i in rows:
        r = rng.integers(2, vocab, size=rv_len)
        r[int(rng.integers(min(2, rv_len), rv_len + 1)):] = 0
        rv = [int(x) for x in r]
        meta["user_reviews"].setdefault(u, []).append(rv)
        meta["item_reviews"].setdefault(i, []).append(rv)
        meta["user_rids"].setdefault(u, []).append(i)
        meta["item_rids"].setdefault(i, []).append(u)
        ratings.append(float(rng.integers(1, 6)))
    return meta, ratings


def random_split(n_users, n_items, vocab, rv_num, rv_len, n_train, n_valid, seed=0):
    """An in-memory split of any size: (meta dict with the sizes, train examples, valid examples) from n_train random
    interactions (repeated pairs included) -- for shapes the fixed layout of write_review_split does not fit."""
    rng = np.random.default_rng(seed)
    rows = [(int(rng.integers(1, n_users)), int(rng.integers(1, n_items))) for _ in range(n_train)]
    meta, ratings = meta_from_rows(rows, vocab, rv_len, rng)
    train = [train_example(meta, u, i, r, rv_num, rv_len) for (u, i), r in zip(rows, ratings)]
    users, items = sorted(meta["user_reviews"]), sorted(meta["item_reviews"])
    valid = [valid_example(meta, int(rng.choice(users)), int(rng.choice(items)), float(rng.integers(1, 6)), rv_num, rv_len)
             for _ in range(n_valid)]
    return dict(meta, user_num=n_users, item_num=n_items, rv_num=rv_num, rv_len=rv_len, vocab_size=vocab), train, valid


def dump_split(data_dir, meta, vocab, train, valid):
    """meta.pkl (with an indexlizer of `vocab` tokens from a module that no longer exists afterwards, as make_dataset writes it)
    and the two example files."""
    os.makedirs(data_dir, exist_ok=True)
    with _fake_module(data_dir, vocab) as indexlizer:
        full = dict({k: v for k, v in meta.items() if k != "vocab_size"}, indexlizer=indexlizer)
        with open(os.path.join(data_dir, "meta.pkl"), "wb") as f:
            pickle.dump(full, f)
    for name, ex in (("train", train), ("valid", valid)):
        with open(os.path.join(data_dir, f"{name}_exmaples.pkl"), "wb") as f:
            pickle.dump(ex, f)


def write_review_split(data_dir, n_users=12, n_items=10, vocab=60, rv_num=4, rv_len=8, n_valid=20, seed=0):
    """43 train interactions (= examples) and n_valid valid examples.  Returns the sizes and `dropped`: per train example the
    (user-side, item-side) index that index() found."""
    R = rv_num
    assert n_users >= 12 and n_items >= R + 4
    rng = np.random.default_rng(seed)
    per_user = {1: [1], 2: list(range(1, R + 1)), 3: list(range(1, R + 2)), 4: list(range(1, R + 4)), 5: [2, 2, 3]}
    for u, k in zip(range(6, 12), (2, 3, 6, 4, 5, 3)):
        per_user[u] = [int(x) for x in rng.choice(np.arange(1, n_items), size=k, replace=False)]
    # rows in an order that interleaves the users (each user's own order is kept: it is the order of its list in meta)
    cursor = {u: 0 for u in per_user}
    rows = []
    while len(rows) < sum(len(v) for v in per_user.values()):
        u = int(rng.choice([u for u in per_user if cursor[u] < len(per_user[u])]))
        rows.append((u, per_user[u][cursor[u]]))
        cursor[u] += 1

    meta, ratings = meta_from_rows(rows, vocab, rv_len, rng)
    train = [train_example(meta, u, i, r, R, rv_len) for (u, i), r in zip(rows, ratings)]
    items = sorted(meta["item_reviews"])
    valid_pairs = [(4, 1)] + [(int(rng.integers(1, 12)), int(rng.choice(items))) for _ in range(n_valid - 1)]
    valid = [valid_example(meta, u, i, float(rng.integers(1, 6)), R, rv_len) for u, i in valid_pairs]

    dropped = [(meta["user_rids"][u].index(i), meta["item_rids"][i].index(u)) for u, i in rows]
    counts = {len(v) for v in meta["user_reviews"].values()}
    assert {1, R, R + 1, R + 3} <= counts and 0 not in meta["user_reviews"] and 0 not in meta["item_reviews"]
    du = {d for d, _ in dropped}
    assert {0, R - 1, R} <= du and max(du) > R
    assert rows.count((5, 2)) == 2 and 1 in meta["user_rids"][4]

    dump_split(data_dir, dict(meta, user_num=n_users, item_num=n_items, rv_num=R, rv_len=rv_len), vocab, train, valid)
    return dict(user_num=n_users, item_num=n_items, vocab=vocab, rv_num=R, rv_len=rv_len, n_train=len(train), n_valid=len(valid),
                dropped=dropped, pairs=rows)
