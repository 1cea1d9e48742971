"""The sentence split (AHN) on the host: the reader on both feeds, ragged examples padded to [B, R, S, W], the load-time refusals,
the cache's torch restatement against the examples' own collate with the lengths and masks of the reference's three static methods,
the C ABI entry and its argument checks, and the trainer's refusals for --model ahn (CPU only)."""
import ctypes as C
import os
import pickle

import pytest
import torch

import make_sentence_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a non-NULL pointer value: every call below is refused before anything would read it


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("sentence_split")
    info = make_sentence_dataset.write_sentence_split(str(d))
    return str(d), info


def _load(d, name):
    with open(os.path.join(d, f"{name}_exmaples.pkl"), "rb") as f:
        return pickle.load(f)


def _store(d, name, ex):
    with open(os.path.join(d, f"{name}_exmaples.pkl"), "wb") as f:
        pickle.dump(ex, f)


# trainer/train_ahn.py:149-184, restated: the masks are SUM-based there, the lengths a count of the non-zero words
def ref_sent_mask(batch_reviews):
    return batch_reviews.sum(dim=-1) != 0


def ref_sent_lengths(batch_reviews):
    sent_lengths = torch.ones(size=list(batch_reviews.size()), dtype=torch.int64)
    sent_lengths[batch_reviews == 0] = 0
    return sent_lengths.sum(dim=-1)


def ref_review_mask(batch_reviews):
    bz, rn = batch_reviews.size(0), batch_reviews.size(1)
    review_mask = torch.ones(size=(bz, rn), dtype=torch.bool)
    review_mask[batch_reviews.sum(dim=-1).sum(dim=-1) == 0] = False
    return review_mask


def test_the_helper_split_is_reference_shaped(split):
    d, info = split
    train, valid = _load(d, "train"), _load(d, "valid")
    R, S, W = info["rv_num"], info["sent_num"], info["word_num"]
    assert all(len(e) == 8 and len(e[7]) == S and all(len(s) == W for s in e[7]) for e in train)
    assert all(len(e) == 7 for e in valid)
    assert all(len(e[3]) == len(e[4]) == len(e[5]) == len(e[6]) == R for e in train + valid)
    assert all(len(rv) == S and all(len(s) == W for s in rv) for e in train + valid for rv in e[3] + e[4])
    # the valid pair (4, 1): user 4 reviewed item 1 in the train split, and the valid example still holds that review's rid
    assert valid[0][:2] == [4, 1] and valid[0][5][0] == 1
    k = info["pairs"].index((4, 1))
    assert info["dropped"][k][0] == 0 and train[k][5][0] != 1
    with open(os.path.join(d, "meta.pkl"), "rb") as f:
        assert b"fake_tokenizer_mod" in f.read()              # the indexlizer names a module that is gone: the tolerant unpickler's job


def test_reader_on_both_feeds(split):
    from review_based_recommender_amd import data as D
    d, info = split
    R, S, W = info["rv_num"], info["sent_num"], info["word_num"]
    assert D.SentenceDataset.FEEDS == ("examples", "ids")
    ds = D.SentenceDataset(d, "train")
    assert ds.feed == "examples" and len(ds) == info["n_train"] and len(ds[0]) == 7
    assert (ds.rv_num, ds.sent_num, ds.word_num, ds.vocab_size) == (R, S, W, info["vocab"])
    assert (ds.user_num, ds.item_num) == (info["user_num"], info["item_num"]) and 0 not in ds.user_reviews
    b = ds.collate_fn([ds[k] for k in range(5)])
    assert len(b) == 7
    assert b[0].shape == b[1].shape == (5, R, S, W) and b[4].shape == b[5].shape == (5, R) and b[2].shape == b[3].shape == b[6].shape == (5,)
    assert all(t.dtype == torch.int64 for t in b[:6]) and b[6].dtype == torch.float32
    train = _load(d, "train")
    for k in range(5):                                          # the examples are rectangular here: the batch is the lists
        assert b[0][k].tolist() == train[k][3] and b[1][k].tolist() == train[k][4]
        assert b[4][k].tolist() == train[k][5] and b[5][k].tolist() == train[k][6]
        assert (int(b[2][k]), int(b[3][k]), float(b[6][k])) == tuple(train[k][:3])
    ids = D.SentenceDataset(d, "train", feed="ids")
    assert len(ids[0]) == 3
    u, i, r = ids.collate_fn([ids[k] for k in range(5)])
    assert torch.equal(u, b[2]) and torch.equal(i, b[3]) and torch.equal(r, b[6]) and u.dtype == torch.int64 and r.dtype == torch.float32
    D.SentenceDataset(d, "valid", feed="ids")
    with pytest.raises(ValueError):
        D.SentenceDataset(d, "train", feed="tokens")


def _strip(x):
    """A padded nested list as the ragged one it pads: trailing zeros / empty tails dropped on every level."""
    if not isinstance(x, list):
        return x
    x = [_strip(y) for y in x]
    while x and (x[-1] == 0 or x[-1] == []):
        x.pop()
    return x


def test_ragged_examples_pad_to_the_right_shapes(tmp_path):
    """Fewer than R reviews, fewer than S sentences, sentences shorter than W (train_ahn.py:381-419 fills zeros around them)."""
    from review_based_recommender_amd import data as D
    d = str(tmp_path / "sent")
    info = make_sentence_dataset.write_sentence_split(d)
    full = D.SentenceDataset(d, "valid")
    want = full.collate_fn([full[k] for k in range(len(full))])
    ex = _load(d, "valid")
    ragged = [e[:3] + [_strip(f) for f in e[3:7]] for e in ex]
    flat = [rv for e in ragged for rv in e[3] + e[4]]
    assert any(len(e[3]) < info["rv_num"] for e in ragged) and any(len(rv) < info["sent_num"] for rv in flat)
    assert any(len(s) < info["word_num"] for rv in flat for s in rv) and any(s == [] for rv in flat for s in rv)
    _store(d, "valid", ragged)
    ds = D.SentenceDataset(d, "valid")
    got = ds.collate_fn([ds[k] for k in range(len(ds))])
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    D.SentenceDataset(d, "valid", feed="ids")                    # compared after padding: the ragged split passes the id feed's check


@pytest.mark.parametrize("what,text", [("reviews", "rv_num"), ("sentences", "sent_num"), ("words", "word_num"), ("rids", "rv_num")])
@pytest.mark.parametrize("feed", ["examples", "ids"])
def test_over_long_examples_are_refused_at_load_time(tmp_path, what, text, feed):
    from review_based_recommender_amd import data as D
    d = str(tmp_path / "sent")
    info = make_sentence_dataset.write_sentence_split(d)
    ex = _load(d, "valid")
    e, W = ex[6], info["word_num"]
    if what == "reviews":
        e[4] = e[4] + [e[4][0]]
    elif what == "sentences":
        e[3] = [e[3][0] + [[0] * W]] + e[3][1:]
    elif what == "words":
        e[3] = e[3][:1] + [[e[3][1][0] + [3]] + e[3][1][1:]] + e[3][2:]
    else:
        e[5] = e[5] + [1]
    _store(d, "valid", ex)
    with pytest.raises(ValueError, match=rf"valid example 6\b.*{text}"):
        D.SentenceDataset(d, "valid", feed=feed)


@pytest.mark.parametrize("set_name,k,field", [("train", 7, 3), ("train", 11, 6), ("valid", 3, 4), ("valid", 0, 5)])
def test_id_feed_refuses_examples_that_differ_from_meta(tmp_path, set_name, k, field):
    from review_based_recommender_amd import data as D
    d = str(tmp_path / "sent")
    make_sentence_dataset.write_sentence_split(d)
    D.SentenceDataset(d, set_name, feed="ids")                  # the helper's split passes the check
    ex = _load(d, set_name)
    e = ex[k]
    if field in (3, 4):                                         # one word of the last sentence, still inside the vocabulary
        rv = [list(s) for s in e[field][0]]
        rv[-1][-1] = 3 if rv[-1][-1] != 3 else 4
        e[field] = [rv] + list(e[field][1:])
    else:                                                       # one rid, still a valid id
        rids = list(e[field])
        rids[0] = 2 if rids[0] != 2 else 3
        e[field] = rids
    _store(d, set_name, ex)
    D.SentenceDataset(d, set_name)                              # the example feed trains on the example's own copy
    name = {3: "u_revs", 4: "i_revs", 5: "u_rids", 6: "i_rids"}[field]
    with pytest.raises(ValueError, match=rf"{set_name} example {k}\b.*{name}"):
        D.SentenceDataset(d, set_name, feed="ids")


def test_range_checks_cover_the_ragged_tokens(tmp_path):
    from review_based_recommender_amd import data as D
    d = str(tmp_path / "sent")
    info = make_sentence_dataset.write_sentence_split(d)
    ex = _load(d, "valid")
    ex[2][4] = [[list(s) for s in rv] for rv in ex[2][4]]
    ex[2][4][1][0][0] = info["vocab"]
    _store(d, "valid", ex)
    with pytest.raises(IndexError, match="item review tokens"):
        D.SentenceDataset(d, "valid")
    ds = D.SentenceDataset(d, "train")
    ds.user_rids[2][1] = info["item_num"]                       # a counterpart id past the item table, in meta
    with pytest.raises(IndexError, match="user_rids"):
        D.DeviceSentenceCache(ds, "cpu")


@pytest.mark.parametrize("set_name", ["train", "valid"])
def test_cpu_cache_gather_equals_the_examples_collate(split, set_name):
    """Every batch of the split: the train split under leave-one-out, the valid split without; lengths and masks against the
    reference's own rules applied to the collated tokens."""
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.SentenceDataset(d, set_name)
    cache = D.DeviceSentenceCache(ds, "cpu")
    R, S, W = info["rv_num"], info["sent_num"], info["word_num"]
    assert cache.user_table.dtype == cache.item_rid_table.dtype == torch.int32
    assert cache.user_table.shape == (info["user_num"], R + 1, S, W) and cache.item_rid_table.shape == (info["item_num"], R + 1)
    assert not cache.user_table[0].any() and not cache.item_table[0].any() and not cache.item_rid_table[0].any()
    loo = set_name == "train"
    feed = cache.feed(loo)
    differs = False
    for s in range(0, len(ds), 8):
        b = ds.collate_fn([ds[k] for k in range(s, min(s + 8, len(ds)))])
        B = b[2].shape[0]
        revs = torch.cat([b[0], b[1]])
        want = dict(revs=revs, sent_lens=ref_sent_lengths(revs), sent_masks=ref_sent_mask(revs), rev_masks=ref_review_mask(revs),
                    rids=torch.cat([b[4], b[5]]), ids=torch.cat([b[2], b[3]]))
        got = dict(zip(cache.NAMES, cache.gather(b[2], b[3], loo)))
        for name in cache.NAMES:
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            assert torch.equal(got[name], want[name]), (set_name, s, name)
        args = feed.inputs(b[2], b[3])
        assert len(args) == 10
        for k, name in enumerate(("revs", "sent_masks", "sent_lens", "rev_masks", "ids")):
            assert torch.equal(args[2 * k], want[name][:B]) and torch.equal(args[2 * k + 1], want[name][B:]), name
        for a, z in zip(args, feed.empty_inputs(B)):
            assert a.shape == z.shape and a.dtype == z.dtype and not z.any()
        differs |= not torch.equal(cache.gather(b[2], b[3], not loo)[0], revs)
    assert differs                       # the other rule gives other batches on this split: the test can tell the two apart
    assert cache.gather(b[2], b[3], loo, rids=False, ids=None)[4:] == (None, None)
    with pytest.raises(IndexError):
        cache.gather(torch.tensor([info["user_num"]]), torch.tensor([1]), loo)
    with pytest.raises(IndexError):
        cache.gather(torch.tensor([1]), torch.tensor([-1]), loo)


@pytest.mark.parametrize("set_name", ["train", "valid"])
def test_cpu_feed_gathers_into_the_views_of_an_input_block(split, set_name):
    """SentenceFeed.gather(out=...): the ten views of a block laid out by empty_inputs(B) receive what inputs() returns, the bytes
    of the block outside the views keep their 0xA5, rids are not made."""
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.train_step import _flat_layout, _flat_views
    d, _ = split
    ds = D.SentenceDataset(d, set_name)
    feed = D.DeviceSentenceCache(ds, "cpu").feed(set_name == "train")
    b = ds.collate_fn([ds[k] for k in range(5)])
    like = list(feed.empty_inputs(5))
    layout = _flat_layout(like)
    flat = torch.full((layout[-1],), 0xA5, dtype=torch.uint8)
    views = _flat_views(flat, layout, like)
    got = feed.gather(b[2], b[3], out=views)
    assert got["rids"] is None and got["revs"].data_ptr() == views[0].data_ptr()
    args = feed.inputs(b[2], b[3])
    assert len(views) == len(args) == 10 and torch.equal(args[0], b[0]) and torch.equal(args[1], b[1])
    for k, (v, a) in enumerate(zip(views, args)):
        assert v.dtype == a.dtype and v.shape == a.shape and torch.equal(v, a), k
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for o, t in zip(layout, like):
        covered[o:o + t.numel() * t.element_size()] = True
    assert not bool(covered.all()) and bool((flat[~covered] == 0xA5).all())


def test_sentence_masks_count_words_wherever_they_stand():
    from review_based_recommender_amd import data as D
    revs = torch.tensor([[[[0, 5, 0, 7], [0, 0, 0, 0], [9, 0, 0, 0]], [[0, 0, 0, 0]] * 3]])
    lens, sm, rm = D.sentence_masks(revs)
    assert lens.tolist() == [[[2, 0, 1], [0, 0, 0]]] and sm.tolist() == [[[True, False, True], [False] * 3]] and rm.tolist() == [[True, False]]
    assert torch.equal(lens, ref_sent_lengths(revs)) and torch.equal(sm, ref_sent_mask(revs)) and torch.equal(rm, ref_review_mask(revs))


def test_the_review_split_rule_is_the_sentence_splits_rule():
    """review_example_from_meta over a review of S x W tokens is, flattened, review_example_from_meta over S * W tokens."""
    import types

    from review_based_recommender_amd import data as D
    meta, train, _ = make_sentence_dataset.random_split(7, 7, 40, 3, 2, 4, 30, 4, seed=2)
    sent = types.SimpleNamespace(**meta)
    flat = {k: {i: [sum(rv, []) for rv in v] for i, v in meta[k].items()} for k in ("user_reviews", "item_reviews")}
    rev = types.SimpleNamespace(**dict(meta, **flat, rv_len=8))
    del rev.sent_num, rev.word_num
    for e in train:
        for loo in (True, False):
            a = D.review_example_from_meta(sent, e[0], e[1], loo)
            b = D.review_example_from_meta(rev, e[0], e[1], loo)
            assert [sum(rv, []) for rv in a[0]] == b[0] and [sum(rv, []) for rv in a[1]] == b[1] and a[2:] == b[2:]
        assert list(D.review_example_from_meta(sent, e[0], e[1], True)) == e[3:7]


def test_header_and_binding_declare_sentence_gather():
    from review_based_recommender_amd import _lib
    with open(os.path.join(ROOT, "include", "rbr_hip.h")) as f:
        assert "int rbr_sentence_gather(" in f.read()
    res, args = _lib.SIGNATURES["rbr_sentence_gather"]
    assert res is C.c_int and len(args) == 23
    assert hasattr(C.CDLL(_lib.LIB_PATH), "rbr_sentence_gather")
    assert hasattr(_lib.lib(), "rbr_sentence_gather")


def _gather(L, B=4, R=3, S=2, W=8, u=P, i=P, ur=P, ud=P, U=9, ir=P, idd=P, I=7, loo=1, pad=0, replace=0, revs=P, lens=P, sm=P, rm=P,
            rids=None, ids=None, err=P):
    return L.rbr_sentence_gather(B, R, S, W, u, i, ur, ud, U, ir, idd, I, loo, pad, replace, revs, lens, sm, rm, rids, ids, err, None)


@pytest.mark.parametrize("kw,text", [
    (dict(B=0), b"bad shape"), (dict(B=-2), b"bad shape"), (dict(R=0), b"bad shape"), (dict(S=0), b"bad shape"), (dict(S=-1), b"bad shape"),
    (dict(W=0), b"bad shape"), (dict(U=0), b"bad shape"), (dict(I=0), b"bad shape"), (dict(loo=2), b"bad shape"), (dict(loo=-1), b"bad shape"),
    (dict(u=None), b"null"), (dict(i=None), b"null"), (dict(ur=None), b"null"), (dict(ud=None), b"null"), (dict(ir=None), b"null"),
    (dict(idd=None), b"null"), (dict(revs=None), b"null"), (dict(lens=None), b"null"), (dict(sm=None), b"null"), (dict(rm=None), b"null"),
    (dict(err=None), b"null"),
    (dict(replace=-1), b"replace_id"), (dict(replace=7), b"replace_id"), (dict(replace=8), b"replace_id"), (dict(replace=9), b"replace_id"),
])
def test_sentence_gather_refuses_bad_arguments(kw, text):
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    assert _gather(L, **kw) == -1          # RBR_ERR_BAD_ARG
    msg = L.rbr_last_error()
    assert b"rbr_sentence_gather" in msg and text in msg, msg


@pytest.mark.parametrize("key,cfg", [
    ("device_cache", {"device_cache": True}),
    ("eval_from_towers", {"device_reviews": True, "eval_from_towers": True}),
    ("rank_metrics", {"device_reviews": True, "rank_metrics": [10]}),
    ("loss", {"device_reviews": True, "loss": "bpr"}),
    ("loss", {"device_reviews": True, "loss": "softmax"}),
    ("sample_train_review", {"device_reviews": True, "sample_train_review": True}),
    ("parallel", {"parallel": True}),
])
def test_trainer_refuses_for_ahn(tmp_path, key, cfg):
    """Each config switches on one refused key; the data directory is empty, so the refusal came before anything was read."""
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    assert "ahn" in ReviewExperiment.KINDS
    with pytest.raises(ValueError, match=rf"^{key} is not available with --model ahn: \w"):
        ReviewExperiment("ahn", Args(dict(cfg, data_dir=str(tmp_path))))
