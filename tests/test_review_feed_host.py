"""The id-fed review split on the host: the id collate, the load-time check that the examples are what the leave-one-out rule
gives from meta, the cache's torch restatement against the examples' own collate, ragged meta through DeviceDocCache, the range
checks, the C ABI entry and the trainer's config errors (CPU only)."""
import os
import pickle

import pytest
import torch

import make_review_dataset


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("review_split")
    info = make_review_dataset.write_review_split(str(d))
    return str(d), info


def test_the_helper_split_is_reference_shaped(split):
    d, info = split
    with open(os.path.join(d, "train_exmaples.pkl"), "rb") as f:
        train = pickle.load(f)
    with open(os.path.join(d, "valid_exmaples.pkl"), "rb") as f:
        valid = pickle.load(f)
    R, T = info["rv_num"], info["rv_len"]
    assert all(len(e) == 8 and len(e[7]) == T for e in train) and all(len(e) == 7 for e in valid)
    assert all(len(e[3]) == len(e[4]) == len(e[5]) == len(e[6]) == R for e in train + valid)
    # the valid pair (4, 1): user 4 reviewed item 1 in the train split, and the valid example still holds that review's rid
    assert valid[0][:2] == [4, 1] and valid[0][5][0] == 1
    k = info["pairs"].index((4, 1))
    assert info["dropped"][k][0] == 0 and train[k][5][0] != 1


def test_id_collate_shapes_and_dtypes(split):
    from review_based_recommender_amd import data as D
    d, _ = split
    ds = D.ReviewDataset(d, "train", feed="ids")
    assert D.ReviewDataset.FEEDS == ("examples", "ids")
    assert len(ds[0]) == 3
    u, i, r = ds.collate_fn([ds[k] for k in range(5)])
    assert u.shape == i.shape == r.shape == (5,)
    assert u.dtype == i.dtype == torch.int64 and r.dtype == torch.float32
    ref_ds = D.ReviewDataset(d, "train")
    assert ref_ds.feed == "examples" and len(ref_ds[0]) == 7
    ref = ref_ds.collate_fn([ref_ds[k] for k in range(5)])
    assert len(ref) == 9 and torch.equal(u, ref[4]) and torch.equal(i, ref[5]) and torch.equal(r, ref[8])
    with pytest.raises(ValueError):
        D.ReviewDataset(d, "train", feed="tokens")


@pytest.mark.parametrize("set_name,k,field,slot", [("train", 7, 3, None), ("train", 11, 6, None), ("valid", 3, 4, None),
                                                   ("valid", 0, 5, 0)])
def test_id_feed_refuses_examples_that_differ_from_meta(tmp_path, set_name, k, field, slot):
    from review_based_recommender_amd import data as D
    d = tmp_path / "rev"
    make_review_dataset.write_review_split(str(d))
    D.ReviewDataset(str(d), set_name, feed="ids")               # the helper's split passes the check
    path = d / f"{set_name}_exmaples.pkl"
    with open(path, "rb") as f:
        ex = pickle.load(f)
    e = ex[k]
    if field in (3, 4):                                         # one token, still inside the vocabulary
        rev = list(e[field][0])
        rev[0] = 3 if rev[0] != 3 else 4
        e[field] = [rev] + list(e[field][1:])
    else:                                                       # one rid, still a valid id
        rids = list(e[field])
        rids[slot or 0] = 2 if rids[slot or 0] != 2 else 3
        e[field] = rids
    with open(path, "wb") as f:
        pickle.dump(ex, f)
    D.ReviewDataset(str(d), set_name)                           # the example feed trains on the example's own copy
    name = {3: "u_revs", 4: "i_revs", 5: "u_rids", 6: "i_rids"}[field]
    with pytest.raises(ValueError, match=rf"{set_name} example {k}\b.*{name}"):
        D.ReviewDataset(str(d), set_name, feed="ids")


def test_a_train_pair_absent_from_the_list_is_compared_under_the_no_drop_rule(tmp_path):
    from review_based_recommender_amd import data as D
    d = tmp_path / "rev"
    info = make_review_dataset.write_review_split(str(d))
    meta = D.load_pickle(str(d / "meta.pkl"))
    ds = D.ReviewDataset(str(d), "train")
    u = 1
    i = next(x for x in range(1, info["item_num"]) if x not in meta["user_rids"][u] and x in meta["item_rids"])
    plain = make_review_dataset.valid_example(meta, u, i, 3.0, info["rv_num"], info["rv_len"])
    assert list(D.review_example_from_meta(ds, u, i, True)) == plain[3:7]


@pytest.mark.parametrize("set_name", ["train", "valid"])
def test_cpu_cache_inputs_equal_the_examples_collate(split, set_name):
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.ReviewDataset(d, set_name)
    cache = D.DeviceReviewCache(ds, "cpu")
    R, T = info["rv_num"], info["rv_len"]
    assert cache.user_table.dtype == cache.user_rid_table.dtype == torch.int32
    assert cache.user_table.shape == (info["user_num"], R + 1, T) and cache.item_rid_table.shape == (info["item_num"], R + 1)
    assert cache.user.shape == (info["user_num"], R, T) and cache.item_rids.shape == (info["item_num"], R)
    assert not cache.user_table[0].any() and not cache.item_rid_table[0].any()
    ref = ds.collate_fn([ds[k] for k in range(len(ds))])
    u_ids, i_ids = ref[4], ref[5]
    loo = set_name == "train"
    got = cache.feed("narre", loo).inputs(u_ids, i_ids)
    assert len(got) == 8
    for k, (a, b) in enumerate(zip(got, ref[:8])):
        assert a.dtype == b.dtype and torch.equal(a, b), (set_name, k)
    got = cache.feed("simple_siamese", loo).inputs(u_ids, i_ids)
    want = (*ref[:4], ref[2].any(-1), ref[3].any(-1), ref[4], ref[5])
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(a, b), (set_name, k)
    if loo:          # the other rule gives another batch on this split: the test can tell them apart
        other = cache.feed("narre", False).inputs(u_ids, i_ids)
        assert not torch.equal(other[0], ref[0]) and not torch.equal(other[7], ref[7])
    with pytest.raises(ValueError):
        cache.feed("deepconn", True)
    with pytest.raises(IndexError):
        cache.feed("narre", loo).inputs(torch.tensor([info["user_num"]]), torch.tensor([1]))


def test_ragged_meta_through_device_doc_cache_is_truncated_and_padded(split):
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.ReviewDataset(d, "valid")
    cache = D.DeviceDocCache(ds, "cpu")
    R, T = info["rv_num"], info["rv_len"]
    assert cache.user.dtype == cache.user_rids.dtype == torch.int64
    assert cache.user.shape == (info["user_num"], R, T) and cache.item_rids.shape == (info["item_num"], R)
    for tab, rid, revs, rids, n in ((cache.user, cache.user_rids, ds.user_reviews, ds.user_rids, info["user_num"]),
                                    (cache.item, cache.item_rids, ds.item_reviews, ds.item_rids, info["item_num"])):
        for i in range(n):
            rv = list(revs.get(i, []))[:R]
            rd = list(rids.get(i, []))[:R]
            assert tab[i].tolist() == rv + [[0] * T] * (R - len(rv)), i
            assert rid[i].tolist() == rd + [0] * (R - len(rd)), i
    rc = D.DeviceReviewCache(ds, "cpu")
    assert torch.equal(rc.user.long(), cache.user) and torch.equal(rc.item_rids, cache.item_rids)


def test_rectangular_meta_through_device_doc_cache_is_unchanged(tmp_path):
    import make_dataset
    from review_based_recommender_amd import data as D
    make_dataset.write_review_split(str(tmp_path / "rect"))
    ds = D.ReviewDataset(str(tmp_path / "rect"), "train")
    cache = D.DeviceDocCache(ds, "cpu")
    assert torch.equal(cache.user, torch.tensor([ds.user_reviews[i] for i in range(ds.user_num)]))
    assert torch.equal(cache.item_rids, torch.tensor([ds.item_rids[i] for i in range(ds.item_num)]))


def test_cache_range_checks_name_the_table(split):
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.ReviewDataset(d, "train")
    ds.item_reviews[3][0] = list(ds.item_reviews[3][0])
    ds.item_reviews[3][0][1] = info["vocab"]                    # one token past the vocabulary, in meta
    with pytest.raises(IndexError, match="item_reviews"):
        D.DeviceReviewCache(ds, "cpu")
    ds = D.ReviewDataset(d, "train")
    ds.user_rids[2][1] = info["item_num"]                       # a counterpart id past the item table
    with pytest.raises(IndexError, match="user_rids"):
        D.DeviceReviewCache(ds, "cpu")


def test_header_and_binding_declare_review_gather():
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rbr_hip.h")) as f:
        assert "int rbr_review_gather(" in f.read()
    res, args = _lib.SIGNATURES["rbr_review_gather"]
    assert len(args) == 21
    assert hasattr(_lib.lib(), "rbr_review_gather")


def test_trainer_config_errors_name_the_other_key(tmp_path):
    from review_based_recommender_amd.trainer import DEFAULTS, Args, ReviewExperiment
    assert DEFAULTS["device_reviews"] is False
    for kind in ("deepconn", "dual_att"):
        with pytest.raises(ValueError, match="device_cache"):
            ReviewExperiment(kind, Args({"data_dir": str(tmp_path), "device_reviews": True}))
    for kind in ("narre", "simple_siamese"):
        with pytest.raises(ValueError, match="device_reviews"):
            ReviewExperiment(kind, Args({"data_dir": str(tmp_path), "device_cache": True}))
