"""Host-side checks of dynamic negative sampling (rbr_sample_hard_negatives, data.NegativeFeed(n_cand=...), the trainer's
neg_candidates / neg_refresh_steps): the symbol is declared, bound and exported; the C entry, the feed and the trainer refuse what
they cannot serve before any launch; the integer restatement (tests/hard_neg_ref.py) equals the uniform sampler's at n_cand = 1
and its key orders by score descending, then item ascending.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from bpr_ref import sample_negatives_ref
from hard_neg_ref import choose, expected_outputs, sample_hard_negatives_ref, score_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a non-NULL pointer value: every call below is refused before anything would read it


def test_symbol_is_declared_bound_and_exported():
    from review_based_recommender_amd import _lib
    with open(os.path.join(ROOT, "include", "rbr_hip.h")) as f:
        assert "int rbr_sample_hard_negatives(" in f.read()
    res, args = _lib.SIGNATURES["rbr_sample_hard_negatives"]
    assert res is C.c_int and len(args) == 29
    assert hasattr(C.CDLL(_lib.LIB_PATH), "rbr_sample_hard_negatives")
    assert hasattr(_lib.lib(), "rbr_sample_hard_negatives")


def _hard(L, B=4, n_neg=1, n_cand=4, I=9, item_lo=1, u=P, i=P, off=None, items=None, nnz=0, U=3, mode=0, K=4, ul=P, il=P, h=P, g=P,
          ub=None, ib=None, state=P, tries=16, replace=0, uo=P, io=P, valid=P):
    return L.rbr_sample_hard_negatives(B, n_neg, n_cand, I, item_lo, u, i, off, items, nnz, U, mode, K, ul, il, h, g, ub, ib, 1, state,
                                       tries, replace, uo, io, valid, None, None, None)


@pytest.mark.parametrize("kw,text", [
    (dict(n_cand=0), b"n_cand"), (dict(n_cand=65), b"n_cand"), (dict(K=0), b"K=0"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
    (dict(h=None), b"needs h and g"), (dict(g=None), b"needs h and g"),
    (dict(ul=None), b"latent table"), (dict(il=None), b"latent table"), (dict(mode=1, ul=None, h=None, g=None), b"latent table"),
    # ... and what rbr_sample_negatives refuses
    (dict(B=0), b"bad shape"), (dict(n_neg=0), b"bad shape"), (dict(I=0), b"bad shape"), (dict(U=0), b"bad shape"),
    (dict(B=1 << 20, n_neg=1 << 5, n_cand=64), b"bad shape"),
    (dict(item_lo=9), b"item_lo"), (dict(item_lo=-1), b"item_lo"),
    (dict(u=None), b"null"), (dict(i=None), b"null"), (dict(state=None), b"null"), (dict(uo=None), b"null"), (dict(io=None), b"null"),
    (dict(valid=None), b"null"),
    (dict(off=P), b"seen list"), (dict(items=P), b"seen list"), (dict(nnz=3), b"seen list"), (dict(off=P, items=P, nnz=-1), b"seen list"),
    (dict(tries=0), b"max_tries"), (dict(tries=65), b"max_tries"), (dict(replace=-1), b"replace_id"), (dict(replace=9), b"replace_id"),
])
def test_hard_sampler_refuses_bad_arguments(kw, text):
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    assert _hard(L, **kw) == -1          # RBR_ERR_BAD_ARG
    msg = L.rbr_last_error()
    assert b"rbr_sample_hard_negatives" in msg and text in msg, msg


def test_dot_mode_needs_neither_h_nor_g():
    """... so the refusal it ends in is a later one: the NULL state."""
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    assert _hard(L, mode=1, h=None, g=None, state=None) == -1 and b"null pointer" in L.rbr_last_error()


def test_functional_entry_checks_the_shared_arguments_like_sample_negatives():
    from review_based_recommender_amd import functional as RF
    ids = torch.zeros(4, dtype=torch.int64)
    t = torch.zeros(3, 2)
    kw = dict(n_cand=2, mode="dot", ul=t, il=t)
    with pytest.raises(RuntimeError, match="state must be"):
        RF.sample_hard_negatives(ids, ids, 1, 3, None, state=torch.zeros(2), **kw)
    with pytest.raises(RuntimeError, match="one row per user id"):
        RF.sample_hard_negatives(ids, ids, 1, 3, (ids, ids, ids), state=torch.zeros(2, dtype=torch.int64), **kw)
    with pytest.raises(RuntimeError, match=r"u_ids / i_ids must be \[B\] each"):
        RF.sample_hard_negatives(ids, ids[:3], 1, 3, None, state=torch.zeros(2, dtype=torch.int64), **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.sample_hard_negatives(ids, ids, 1, 3, None, state=torch.zeros(2, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="unknown score mode"):
        RF.sample_hard_negatives(ids, ids, 1, 3, None, state=torch.zeros(2, dtype=torch.int64), **dict(kw, mode="cosine"))


# ------------------------------------------------------------------------------------------------ the feed
class _Inner:
    device = torch.device("cpu")


@pytest.mark.parametrize("n_cand", [0, 65, -1, True, 2.0, "4", None])
def test_negative_feed_refuses_bad_n_cand(n_cand):
    from review_based_recommender_amd.data import NegativeFeed
    with pytest.raises(ValueError, match="n_cand"):
        NegativeFeed(_Inner(), None, 9, n_cand=n_cand)


def test_negative_feed_keeps_todays_buffers_at_n_cand_1_and_above():
    from review_based_recommender_amd.data import NegativeFeed
    for n_cand in (1, 4):
        f = NegativeFeed(_Inner(), None, 9, n_neg=3, **({} if n_cand == 1 else {"n_cand": n_cand}))
        assert f.n_cand == n_cand and f.tables is None
        u, i, v = f.buffers(5)
        assert u.shape == i.shape == (20,) and v.shape == (15,) and u.dtype == torch.int64 and v.dtype == torch.float32
        assert f.buffers(5)[0] is u and f.buffers(4)[0] is not u
        f.reseed(11, call=6)
        assert f.seed == 11 and f.state.tolist() == [6, 0]


def test_negative_feed_needs_tables_before_it_samples_hard_negatives():
    from review_based_recommender_amd.data import NegativeFeed
    f = NegativeFeed(_Inner(), None, 9, n_cand=2)
    ids = torch.ones(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="set_tables"):
        f.sample(ids, ids)
    with pytest.raises(RuntimeError, match="set_tables"):
        f.inputs(ids, ids)


def test_set_tables_copies_once_and_then_copies_into_the_same_storage():
    from review_based_recommender_amd.data import NegativeFeed
    f = NegativeFeed(_Inner(), None, 9, n_cand=2)
    ul, il, h = torch.randn(5, 3), torch.randn(9, 3), torch.randn(3, 1)
    f.set_tables("fm", ul, il, h, None, None, None)
    own_ul, own_il = f.tables
    assert own_ul is not ul and own_ul.data_ptr() != ul.data_ptr() and torch.equal(own_ul, ul) and torch.equal(own_il, il)
    assert f._tables[3] is h                                  # the head's parameters are the caller's, not copies
    ptrs = (own_ul.data_ptr(), own_il.data_ptr())
    f.set_tables("fm", ul + 1, il * 2, h, None, None, None)
    assert (f.tables[0].data_ptr(), f.tables[1].data_ptr()) == ptrs
    assert torch.equal(f.tables[0], ul + 1) and torch.equal(f.tables[1], il * 2)
    with pytest.raises(ValueError, match="changed shape"):
        f.set_tables("fm", torch.randn(6, 3), il, h, None, None, None)
    with pytest.raises(ValueError, match="latent tables must be"):
        f.set_tables("fm", ul, torch.randn(8, 3), h, None, None, None)


# ------------------------------------------------------------------------------------------------ the trainer
BPR = dict(loss="bpr", device_cache=True, eval_from_towers=True, rank_metrics=[5], select_by="ndcg@5")


@pytest.mark.parametrize("kind,cfg,text", [
    ("deepconn", dict(BPR, neg_candidates=0), "neg_candidates must be"),
    ("deepconn", dict(BPR, neg_candidates=65), "neg_candidates must be"),
    ("deepconn", dict(BPR, neg_candidates=4.0), "neg_candidates must be"),
    ("deepconn", dict(BPR, neg_candidates=True), "neg_candidates must be"),
    ("deepconn", dict(neg_candidates=0), "neg_candidates must be"),
    ("deepconn", dict(neg_candidates=4), "neg_candidates 4 needs loss \"bpr\""),
    ("narre", dict(BPR, loss="softmax", device_cache=False, device_reviews=True, neg_candidates=2), "neg_candidates 2 needs loss \"bpr\""),
    ("deepconn", dict(BPR, neg_candidates=4, neg_refresh_steps=-1), "neg_refresh_steps must be"),
    ("deepconn", dict(BPR, neg_candidates=4, neg_refresh_steps=2.5), "neg_refresh_steps must be"),
    ("deepconn", dict(BPR, neg_candidates=4, neg_refresh_steps=False), "neg_refresh_steps must be"),
    ("deepconn", dict(BPR, neg_refresh_steps=3), "neg_refresh_steps 3 needs neg_candidates > 1"),
    ("deepconn", dict(BPR, neg_candidates=1, neg_refresh_steps=3), "neg_refresh_steps 3 needs neg_candidates > 1"),
    # neg_candidates > 1 is the BPR path: what that path needs is still asked for
    ("deepconn", dict(BPR, neg_candidates=4, select_by="rmse"), "needs a rank metric in select_by"),
    ("deepconn", dict(BPR, neg_candidates=4, device_cache=False, eval_from_towers=False, rank_metrics=[], select_by="rmse"), "needs device_cache"),
])
def test_trainer_refuses_what_the_hard_negative_path_cannot_serve(kind, cfg, text):
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises(ValueError, match=text):
        ReviewExperiment(kind, Args(dict(cfg, data_dir="/nonexistent", model_name=kind)))


def test_trainer_defaults_to_the_uniform_sampler():
    from review_based_recommender_amd import trainer
    assert trainer.DEFAULTS["neg_candidates"] == 1 and trainer.DEFAULTS["neg_refresh_steps"] == 0


# ------------------------------------------------------------------------------------------------ the restatement
def _seen(I):
    every = list(range(1, I))
    rows = [[], every[::2], every[1:], every, every[:-1], every[:1]]
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int64), np.array([x for r in rows for x in r], dtype=np.int32)


@pytest.mark.parametrize("I,max_tries", [(2, 16), (9, 1), (9, 16), (300, 16)])
def test_restatement_at_one_candidate_is_the_uniform_sampler(I, max_tries):
    rng = np.random.default_rng(I)
    B, n_neg = 23, 3
    u, i = rng.integers(0, 6, size=B), rng.integers(1, I, size=B)
    for seen in (None, _seen(I)):
        ref = sample_negatives_ref(u, i, n_neg, I, seen, 77, 4, max_tries=max_tries, replace_id=1)
        cand, found = sample_hard_negatives_ref(u, i, n_neg, 1, I, seen, 77, 4, max_tries=max_tries, replace_id=1)
        assert cand.shape == (n_neg, B, 1) and found.shape == (n_neg, B)
        got = expected_outputs(u, i, cand, found, np.zeros(cand.shape, dtype=np.float32))
        for g, r in zip(got, ref):
            assert g.dtype == r.dtype and np.array_equal(g, r)


def test_restated_candidates_are_the_uniform_draws_of_index_d_times_n_cand_plus_m():
    """Candidate m of draw d of a B-pair batch is what the uniform sampler draws for the SINGLE pair b as its negative
    j * n_cand + m ... restated without the reshape: one pair at a time, n_neg = 1, so d = b."""
    I, n_cand, seed, call = 9, 5, 3, 2
    u, i = np.array([1, 4, 0, 5]), np.array([2, 8, 3, 1])
    cand, found = sample_hard_negatives_ref(u, i, 1, n_cand, I, _seen(I), seed, call, replace_id=1)
    assert found[0].tolist() == [True, False, True, True]          # user 4 has seen all but item 8, its positive
    assert cand[0, 1].tolist() == [1] * n_cand
    flat = sample_negatives_ref(np.repeat(u, n_cand), np.repeat(i, n_cand), 1, I, _seen(I), seed, call, replace_id=1)[1]
    assert np.array_equal(cand[0].reshape(-1), flat[len(u) * n_cand:])


def test_key_orders_by_score_descending_then_item_ascending():
    nan, inf = float("nan"), float("inf")
    order = [(inf, 3), (inf, 7), (3.5, 0), (1e-45, 2), (0.0, 1), (0.0, 9), (-0.0, 1), (-0.0, 4), (-1e-45, 5), (-2.0, 6), (-2.0, 8), (-inf, 0),
             (-inf, 2 ** 31 - 1)]
    keys = score_key(np.array([s for s, _ in order], dtype=np.float32), np.array([c for _, c in order]))
    assert keys.dtype == np.uint64 and all(int(a) > int(b) > 0 for a, b in zip(keys[:-1], keys[1:])), keys
    neg_nan = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    assert score_key(np.array([nan, neg_nan], dtype=np.float32), np.array([0, 5])).tolist() == [0, 0]
    # +0.0 and -0.0 are different keys (the bit pattern orders them), as on the device
    assert int(score_key(np.float32([0.0]), np.array([9]))[0]) > int(score_key(np.float32([-0.0]), np.array([1]))[0])
    # the choice: NaN never wins while a number exists; all NaN -> candidate 0; ties -> the lower item id
    cand = np.array([[[4, 2, 7, 2]], [[5, 6, 7, 8]], [[9, 3, 3, 6]]])
    scores = np.array([[[nan, -inf, nan, -inf]], [[nan, nan, nan, nan]], [[1.0, 2.0, 2.0, 2.0]]], dtype=np.float32)
    assert choose(cand, scores).tolist() == [[2], [5], [3]]
