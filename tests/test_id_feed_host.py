"""The id-fed doc split on the host: the id collate, the load-time check that the examples' documents are
meta's, the cache's token range check, the C ABI entry and the trainer's refusal for the review split (CPU only)."""
import os
import pickle

import pytest
import torch

import make_dataset


def test_id_collate_shapes_and_dtypes(tmp_path):
    from review_based_recommender_amd import data as D
    make_dataset.write_doc_split(str(tmp_path / "doc"))
    for with_ids in (True, False):              # D-ATT's split carries the ids too: only its doc collate drops them
        ds = D.DocDataset(str(tmp_path / "doc"), "train", with_ids=with_ids, feed="ids")
        u, i, r = ds.collate_fn([ds[k] for k in range(5)])
        assert u.shape == i.shape == r.shape == (5,)
        assert u.dtype == i.dtype == torch.int64 and r.dtype == torch.float32
        ref = D.DocDataset(str(tmp_path / "doc"), "train").collate_fn([ds.examples[k] for k in range(5)])
        assert torch.equal(u, ref[4]) and torch.equal(i, ref[5]) and torch.equal(r, ref[6])
        assert D.DocDataset.id_collate_fn([ds.examples[k] for k in range(5)])[0].tolist() == u.tolist()
    with pytest.raises(ValueError):
        D.DocDataset(str(tmp_path / "doc"), "train", feed="tokens")


def test_id_feed_refuses_examples_that_differ_from_meta(tmp_path):
    from review_based_recommender_amd import data as D
    d = tmp_path / "doc"
    make_dataset.write_doc_split(str(d))
    path = d / "train_exmaples.pkl"
    with open(path, "rb") as f:
        ex = pickle.load(f)
    doc = list(ex[7][3])
    doc[0] = 3 if doc[0] != 3 else 4          # still a valid token: only the match with meta fails
    ex[7][3] = doc
    with open(path, "wb") as f:
        pickle.dump(ex, f)
    D.DocDataset(str(d), "train")              # the doc feed trains on the example's own copy, as the reference does
    with pytest.raises(ValueError, match=r"example 7\b.*u_doc"):
        D.DocDataset(str(d), "train", feed="ids")


def test_cache_checks_the_tokens_of_meta_once(tmp_path):
    from review_based_recommender_amd import data as D
    d = tmp_path / "doc"
    info = make_dataset.write_doc_split(str(d))
    ds = D.DocDataset(str(d), "train")
    cache = D.DeviceDocCache(ds, "cpu")
    assert cache.user.dtype == torch.int32 and cache.user.shape == (info["user_num"], info["doc_len"])
    ds.item_docs[3] = list(ds.item_docs[3])
    ds.item_docs[3][5] = info["vocab"]          # one token past the vocabulary, in meta (not in any example)
    with pytest.raises(IndexError, match="item_docs"):
        D.DeviceDocCache(ds, "cpu")


def test_header_and_binding_declare_doc_gather():
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rbr_hip.h")) as f:
        assert "int rbr_doc_gather(" in f.read()
    res, args = _lib.SIGNATURES["rbr_doc_gather"]
    assert len(args) == 15


def test_trainer_refuses_device_cache_for_the_review_split(tmp_path):
    from review_based_recommender_amd.trainer import ReviewExperiment, Args
    for kind in ("narre", "simple_siamese"):
        with pytest.raises(ValueError, match="device_cache"):
            ReviewExperiment(kind, Args({"data_dir": str(tmp_path), "device_cache": True}))
