"""Host-side checks of the BPR training path: the draw of rbr_sample_negatives as the header states it (restated in integers,
tests/bpr_ref.py) is uniform over the eligible items and behaves in a crowded row as measured when the draw was fixed; the new
C entries refuse bad arguments before any launch; the trainer and the feed refuse the configurations they cannot serve.  No
kernel is launched."""
import numpy as np
import pytest
import torch

from bpr_ref import sample_negatives_ref


# ------------------------------------------------------------------------------------------------ the draw, on the CPU
@pytest.mark.parametrize("seed,call", [(0, 0), (1234, 0), (1234, 7)])
def test_draw_is_uniform_over_the_eligible_items(seed, call):
    """I = 9, item_lo = 1, positive 3, no seen list: 7 eligible items, B * n_neg = 28672 draws, expected 4096 each, sigma =
    sqrt(28672 * (1/7) * (6/7)) = 59.3.  Every count within 4 sigma; measured when the draw was fixed: at most 2.2 sigma, and
    no draw of these three (seed, call) pairs is rejected more than 6 times (7 attempts)."""
    B, n_neg = 4096, 7
    st = {}
    u, i, valid = sample_negatives_ref(np.ones(B), np.full(B, 3), n_neg, 9, None, seed, call, item_lo=1, stats=st)
    neg = i[B:]
    assert valid.min() == 1.0 and set(neg.tolist()) == {1, 2, 4, 5, 6, 7, 8}
    counts = np.bincount(neg, minlength=9)
    dev = np.abs(counts[[1, 2, 4, 5, 6, 7, 8]] - B * n_neg / 7) / 59.3
    print(f"seed {seed} call {call}: worst deviation {dev.max():.2f} sigma, attempts {st['attempts']}, walks {st['walks']}")
    assert dev.max() <= 4.0
    assert dev.max() <= 2.2 + 0.05 and st["attempts"] <= 7 and st["walks"] == 0      # the recorded figures of this very draw


def test_crowded_row_takes_the_walk_and_returns_only_unseen_items():
    """seen {1, 3, 4, 6, 8}, positive 2, I = 9: only 5 and 7 are left (3 in 4 attempts are rejected; 0.75^16 = 1 %).  B = 256,
    n_neg = 4, seed 5, call 3: the walk runs in 9 of the 1024 draws."""
    off = np.array([0, 0, 5], dtype=np.int64)
    items = np.array([1, 3, 4, 6, 8], dtype=np.int32)
    st = {}
    u, i, valid = sample_negatives_ref(np.ones(256), np.full(256, 2), 4, 9, (off, items), 5, 3, item_lo=1, max_tries=16, stats=st)
    assert set(i[256:].tolist()) == {5, 7} and valid.min() == 1.0
    assert st["walks"] == 9
    assert np.array_equal(u, np.ones(5 * 256, dtype=np.int64)) and np.array_equal(i[:256], np.full(256, 2))


def test_restated_walk_wraps_and_gives_up():
    # max_tries = 1 and all but item 1 seen: whatever the first candidate, the walk must arrive at 1 -- past I - 1 when it starts above
    off = np.array([0, 7], dtype=np.int64)
    items = np.arange(2, 9, dtype=np.int32)
    u, i, valid = sample_negatives_ref(np.zeros(64), np.full(64, 4), 2, 9, (off, items), 7, 0, item_lo=1, max_tries=1)
    assert set(i[64:].tolist()) == {1} and valid.min() == 1.0
    # one item, and it is the positive: nothing to draw
    u, i, valid = sample_negatives_ref(np.zeros(3), np.full(3, 1), 2, 2, None, 7, 0, item_lo=1, replace_id=1)
    assert set(i[3:].tolist()) == {1} and valid.max() == 0.0


# ------------------------------------------------------------------------------------------------ C entries refuse before launching
def _lib():
    from review_based_recommender_amd import _lib
    return _lib.lib()


P = 4096          # a non-NULL pointer value: every call below is refused before anything would read it


def _sample(L, B=4, n_neg=1, I=9, item_lo=1, u=P, i=P, off=None, items=None, nnz=0, U=0, state=P, tries=16, replace=0, uo=P, io=P,
            valid=P):
    return L.rbr_sample_negatives(B, n_neg, I, item_lo, u, i, off, items, nnz, U, 1, state, tries, replace, uo, io, valid, None)


@pytest.mark.parametrize("kw,text", [
    (dict(B=0), b"bad shape"), (dict(n_neg=0), b"bad shape"), (dict(I=0), b"bad shape"),
    (dict(item_lo=9), b"item_lo"), (dict(item_lo=-1), b"item_lo"),
    (dict(u=None), b"null"), (dict(i=None), b"null"), (dict(state=None), b"null"), (dict(uo=None), b"null"),
    (dict(io=None), b"null"), (dict(valid=None), b"null"),
    (dict(off=P), b"seen list"), (dict(items=P), b"seen list"), (dict(nnz=3), b"seen list"), (dict(off=P, items=P, nnz=-1, U=3), b"seen list"),
    (dict(off=P, items=P, nnz=2, U=0), b"seen list"),
    (dict(tries=0), b"max_tries"), (dict(tries=65), b"max_tries"),
    (dict(replace=-1), b"replace_id"), (dict(replace=9), b"replace_id"),
])
def test_sample_negatives_refuses_bad_arguments(kw, text):
    L = _lib()
    assert _sample(L, **kw) == -1          # RBR_ERR_BAD_ARG
    assert text in L.rbr_last_error(), L.rbr_last_error()


def test_bpr_loss_entries_refuse_bad_arguments():
    L = _lib()
    for args in ((0, 1, P, None, P, P), (4, 0, P, None, P, P), (4, 1, None, None, P, P), (4, 1, P, None, None, P),
                 (1 << 29, 2, P, None, P, P)):
        assert L.rbr_bpr_loss_fwd(*args, None) == -1
        assert b"bpr_loss_fwd" in L.rbr_last_error()
    for args in ((0, 1, P, None, P, P), (4, 0, P, None, P, P), (4, 1, None, None, P, P), (4, 1, P, None, None, P),
                 (4, 1, P, None, P, None)):
        assert L.rbr_bpr_loss_bwd(*args, None) == -1
        assert b"bpr_loss_bwd" in L.rbr_last_error()


def test_functional_entries_refuse_cpu_tensors_and_bad_shapes():
    from review_based_recommender_amd import functional as RF
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.bpr_loss(torch.zeros(4, requires_grad=True), 1)
    with pytest.raises(RuntimeError, match=r"\(1 \+ n_neg\) \* B"):
        RF.bpr_loss(torch.zeros(5), 1)
    with pytest.raises(RuntimeError, match="valid must be"):
        RF.bpr_loss(torch.zeros(6), 2, torch.zeros(3))
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="state must be"):
        RF.sample_negatives(ids, ids, 1, 9, None, state=torch.zeros(2))
    with pytest.raises(RuntimeError, match="one row per user id"):
        RF.sample_negatives(ids, ids, 1, 9, (ids, ids, ids), state=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.sample_negatives(ids, ids, 1, 9, None, state=torch.zeros(2, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ feed and trainer refusals
class _Inner:
    device = torch.device("cpu")


@pytest.mark.parametrize("kw,text", [(dict(n_neg=0), "n_neg"), (dict(n_neg=True), "n_neg"), (dict(n_neg=1.5), "n_neg"),
                                     (dict(item_lo=9), "item_lo"), (dict(item_lo=-1), "item_lo"),
                                     (dict(max_tries=0), "max_tries"), (dict(max_tries=65), "max_tries")])
def test_negative_feed_refuses_bad_settings(kw, text):
    from review_based_recommender_amd.data import NegativeFeed
    with pytest.raises(ValueError, match=text):
        NegativeFeed(_Inner(), None, 9, **kw)


def test_negative_feed_keeps_one_buffer_set_per_batch_size():
    from review_based_recommender_amd.data import NegativeFeed
    f = NegativeFeed(_Inner(), None, 9, n_neg=3)
    u, i, v = f.buffers(5)
    assert u.shape == i.shape == (20,) and v.shape == (15,) and u.dtype == torch.int64 and v.dtype == torch.float32
    assert f.buffers(5)[0] is u and f.buffers(4)[0] is not u
    f.reseed(11, call=6)
    assert f.seed == 11 and f.state.tolist() == [6, 0]


BPR = dict(loss="bpr", device_cache=True, eval_from_towers=True, rank_metrics=[5], select_by="ndcg@5")


@pytest.mark.parametrize("kind,cfg,text", [
    ("deepconn", dict(loss="hinge"), "loss must be one of"),
    ("deepconn", dict(select_by="auc"), "select_by must be"),
    ("deepconn", dict(select_by="ndcg@0"), "select_by must be"),
    ("deepconn", dict(select_by="hr@x"), "select_by must be"),
    ("deepconn", dict(select_by="ndcg@5"), "needs rank_metrics to contain 5"),
    ("deepconn", dict(select_by="hr@10", device_cache=True, eval_from_towers=True, rank_metrics=[5]), "needs rank_metrics to contain 10"),
    ("deepconn", dict(select_by="mrr"), "needs rank_metrics to contain a cut-off"),
    ("deepconn", dict(BPR, device_cache=False, eval_from_towers=False, rank_metrics=[], select_by="rmse"), "needs device_cache"),
    ("narre", dict(BPR, device_cache=False, eval_from_towers=False, rank_metrics=[], select_by="rmse"), "needs device_cache"),
    ("deepconn", dict(BPR, select_by="rmse"), "needs a rank metric in select_by"),
    ("deepconn", dict(BPR, n_neg=0), "n_neg must be"),
    ("deepconn", dict(BPR, n_neg=2.0), "n_neg must be"),
    ("deepconn", dict(loss="bpr", device_cache=True, parallel=True), "not available with parallel"),
])
def test_trainer_refuses_what_the_bpr_path_cannot_serve(kind, cfg, text):
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises(ValueError, match=text):
        ReviewExperiment(kind, Args(dict(cfg, data_dir="/nonexistent", model_name=kind)))
