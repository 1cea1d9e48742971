"""Host-side checks of the in-batch softmax path: the float64 restatement the GPU tests compare the kernels with
(tests/softmax_ref.py) agrees with torch autograd of the same loss; the mask fixture has the rows it claims; the C entries refuse
bad arguments before any launch; the trainer, the feed and the objective refuse what they cannot serve.  No kernel is launched."""
import ctypes as C

import pytest
import torch

import softmax_ref as SR


# ------------------------------------------------------------------------------------------------ the restatement, on the CPU
@pytest.mark.parametrize("fm", [True, False])
@pytest.mark.parametrize("B,K", [(1, 3), (2, 1), (9, 5), (33, 7)])
def test_restated_gradients_equal_float64_autograd(fm, B, K):
    c = SR.random_case(B, K, fm, 100 + B + K, with_rb=True, with_cb=True, with_logq=True, with_drop=True)
    inv_temp, d_loss = 1.0 / 0.25, 2.5
    ref = SR.pair_softmax_ref(c["ul"], c["il"], c["u_ids"], c["i_ids"], fm, c["h"], c["row_bias"], c["col_bias"], c["drop"], c["seen"],
                              1, c["logq"], inv_temp, d_loss)
    leaves = {k: c[k].double().requires_grad_(True) for k in ("ul", "il", "h", "row_bias", "col_bias") if c[k] is not None}
    drop = None if c["drop"] is None else c["drop"].double()
    loss, s = SR.loss_f64(leaves["ul"], leaves["il"], leaves.get("h"), leaves["row_bias"], leaves["col_bias"], drop, c["logq"].double(),
                          ref["allowed"][0], inv_temp, fm)
    (loss * d_loss).backward()
    assert abs(float(loss.detach()) - float(ref["loss"][0])) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert torch.allclose(s.diagonal().detach(), ref["pos"][0], rtol=0, atol=1e-12)
    for name, leaf in (("d_ul", "ul"), ("d_il", "il"), ("d_h", "h"), ("d_col_bias", "col_bias")):
        if name in ref:
            got = leaves[leaf].grad
            assert torch.allclose(got, ref[name][0].reshape(got.shape), rtol=0, atol=1e-12), name
            assert bool((ref[name][1] >= 0).all())


@pytest.mark.parametrize("fm", [True, False])
@pytest.mark.parametrize("B,K", [(1, 3), (2, 1), (9, 5), (33, 7), (65, 33)])
def test_row_bias_gradient_sums_are_zero_to_1e_15(fm, B, K):
    """The gradient of a per-user constant, as a sum over the row (unit root, temperature 1: |ds| <= 1 / B): autograd's and the
    restated row sums are float64 rounding noise around the DEFINED 0."""
    c = SR.random_case(B, K, fm, 200 + B + K, with_rb=True, with_cb=True, with_logq=True, with_drop=True)
    ref = SR.pair_softmax_ref(c["ul"], c["il"], c["u_ids"], c["i_ids"], fm, c["h"], c["row_bias"], c["col_bias"], c["drop"], c["seen"],
                              1, c["logq"])
    assert float(ref["row_sums"][0].abs().max()) <= 1e-15
    rb = c["row_bias"].double().requires_grad_(True)
    loss, _ = SR.loss_f64(c["ul"].double(), c["il"].double(), None if c["h"] is None else c["h"].double(), rb, c["col_bias"].double(),
                          None if c["drop"] is None else c["drop"].double(), c["logq"].double(), ref["allowed"][0], 1.0, fm)
    loss.backward()
    assert float(rb.grad.abs().max()) <= 1e-15


def test_a_row_alone_with_its_own_column_is_exactly_zero():
    u_ids, i_ids, seen, item_lo, _ = SR.mask_fixture()
    c = SR.random_case(8, 5, True, 3, with_rb=True, with_cb=True, with_logq=True, with_drop=False)
    ref = SR.pair_softmax_ref(c["ul"], c["il"], u_ids, i_ids, True, c["h"], c["row_bias"], c["col_bias"], None, seen, item_lo, c["logq"])
    assert float(ref["d_ul"][0][0].abs().max()) == 0.0 and float(ref["d_ul"][1][0].abs().max()) == 0.0
    assert float(ref["P"][0][0, 0]) == 1.0
    # column 4 (the pad id) is masked in every row other than its own: d_il[4] is row 4's term alone
    P, allowed = ref["P"][0], ref["allowed"][0]
    assert not bool(allowed[[0, 1, 2, 3, 5, 6, 7], 4].any()) and float(P[[0, 1, 2, 3, 5, 6, 7], 4].abs().max()) == 0.0


def test_mask_fixture_has_the_rows_it_claims():
    u_ids, i_ids, seen, item_lo, allowed = SR.mask_fixture()
    got = SR.allowed_mask(u_ids, i_ids, seen, item_lo)
    assert torch.equal(got, allowed)
    assert got[0].tolist() == [True] + [False] * 7                       # every negative masked
    assert not got[3, 1] and not got[1, 3] and i_ids[1] == i_ids[3]      # a duplicate item
    assert not got[1, 6] and 7 in seen[1][6:9].tolist()                  # the seen CSR
    assert not bool(got[[0, 1, 2, 3, 5, 6, 7], 4].any()) and int(i_ids[4]) < item_lo      # the pad id
    assert u_ids[1] == u_ids[2] and not got[1, 2] and not got[2, 1]      # two rows of one user: each has rated the other's item
    assert int(u_ids[5]) >= seen[0].shape[0] - 1 and got[5].tolist() == [True] * 4 + [False] + [True] * 3      # outside the CSR
    assert int(seen[0][5]) > seen[1].shape[0] and not got[6, 5]          # an out-of-range offset, clamped: item 6 still masked
    assert bool(got.diagonal().all())


# ------------------------------------------------------------------------------------------------ C entries refuse before launching
def _lib():
    from review_based_recommender_amd import _lib
    return _lib.lib()


P = 4096          # a non-NULL pointer value: every call below is refused before anything would read it
FM, DOT = 0, 1


def _args(**kw):
    a = dict(mode=FM, B=4, K=3, ul=P, il=P, h=P, row_bias=None, col_bias=None, drop=None, p_drop=0.0, seed=1, rng=None, u=P, i=P,
             off=None, items=None, nnz=0, U=0, item_lo=1, logq=None, inv_temp=1.0)
    a.update(kw)
    return a


def _fwd(L, loss=P, pos=P, d_ul=None, d_il=None, d_h=None, d_cb=None, ws=P, **kw):
    a = _args(**kw)
    return L.rbr_pair_softmax_fwd(a["mode"], a["B"], a["K"], a["ul"], a["il"], a["h"], a["row_bias"], a["col_bias"], a["drop"], a["p_drop"],
                                  a["seed"], a["rng"], a["u"], a["i"], a["off"], a["items"], a["nnz"], a["U"], a["item_lo"], a["logq"],
                                  a["inv_temp"], loss, pos, d_ul, d_il, d_h, d_cb, None, None, ws, None)


def _bwd(L, d_loss=P, pos=P, d_ul=P, d_il=P, d_h=P, d_cb=None, ws=P, **kw):
    a = _args(**kw)
    return L.rbr_pair_softmax_bwd(a["mode"], a["B"], a["K"], a["ul"], a["il"], a["h"], a["row_bias"], a["col_bias"], a["drop"], a["p_drop"],
                                  a["seed"], a["rng"], a["u"], a["i"], a["off"], a["items"], a["nnz"], a["U"], a["item_lo"], a["logq"],
                                  a["inv_temp"], d_loss, pos, d_ul, d_il, d_h, d_cb, None, ws, None)


BAD = [
    (dict(ul=None), b"null"), (dict(il=None), b"null"), (dict(u=None), b"null"), (dict(i=None), b"null"), (dict(ws=None), b"null"),
    (dict(h=None), b"needs h"), (dict(mode=2), b"score mode"), (dict(B=0), b"bad shape"), (dict(K=0), b"bad shape"),
    (dict(inv_temp=0.0), b"inv_temp"), (dict(inv_temp=-1.0), b"inv_temp"), (dict(inv_temp=float("inf")), b"inv_temp"),
    (dict(inv_temp=float("nan")), b"inv_temp"),
    (dict(drop=P, p_drop=0.5, rng=P), b"one of them"),
    (dict(mode=DOT, drop=P), b"no dropout"), (dict(mode=DOT, p_drop=0.5, rng=P), b"no dropout"),
    (dict(p_drop=1.0, rng=P), b"p_drop"), (dict(p_drop=-0.1, rng=P), b"p_drop"), (dict(p_drop=float("nan"), rng=P), b"p_drop"),
    (dict(p_drop=0.5), b"call number"),
    (dict(off=P), b"seen list"), (dict(items=P), b"seen list"), (dict(nnz=3), b"seen list"), (dict(off=P, items=P, nnz=2, U=0), b"seen list"),
]


@pytest.mark.parametrize("kw,text", BAD)
def test_pair_softmax_entries_refuse_bad_arguments(kw, text):
    L = _lib()
    for entry in (_fwd, _bwd):
        assert entry(L, **kw) == -1, entry.__name__          # RBR_ERR_BAD_ARG
        assert text in L.rbr_last_error(), L.rbr_last_error()


def test_pair_softmax_entries_refuse_missing_outputs():
    L = _lib()
    for kw in (dict(loss=None), dict(pos=None), dict(d_ul=P), dict(d_ul=P, d_il=P), dict(d_ul=P, d_il=P, d_h=P, d_cb=P),
               dict(d_ul=P, d_il=P, d_h=P, col_bias=P)):
        assert _fwd(L, **kw) == -1 and b"rbr_pair_softmax_fwd" in L.rbr_last_error()
    for kw in (dict(d_loss=None), dict(pos=None), dict(d_ul=None), dict(d_il=None), dict(d_h=None), dict(d_cb=P), dict(col_bias=P)):
        assert _bwd(L, **kw) == -1 and b"rbr_pair_softmax_bwd" in L.rbr_last_error()


@pytest.mark.parametrize("B,K", [(4097, 32), (256, 257), (1 << 20, 8)])
def test_pair_softmax_refuses_unsupported_shapes_and_sizes_them_zero(B, K):
    L = _lib()
    assert L.rbr_pair_softmax_ws_bytes(B, K) == 0
    for entry in (_fwd, _bwd):
        assert entry(L, B=B, K=K) == -2          # RBR_ERR_UNSUPPORTED
        assert b"no fallback" in L.rbr_last_error()
    assert L.rbr_pair_softmax_ws_bytes(0, 8) == 0 and L.rbr_pair_softmax_ws_bytes(8, 0) == 0
    assert L.rbr_pair_softmax_ws_bytes(4096, 256) >= 4 * (4096 * 4096 + 4096 + 4096 * 256)
    assert L.rbr_pair_softmax_ws_bytes(1, 1) > 0


def test_functional_entry_refuses_cpu_tensors_and_bad_shapes():
    from review_based_recommender_amd import functional as RF
    ids = torch.zeros(4, dtype=torch.int64)
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="unknown score mode"):
        RF.pair_softmax_loss(x, x, ids, ids, "cosine")
    with pytest.raises(RuntimeError, match=r"\[B, K\]"):
        RF.pair_softmax_loss(x, torch.zeros(5, 3), ids, ids, "dot")
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.pair_softmax_loss(x, x, ids, ids, "dot")


# ------------------------------------------------------------------------------------------------ feed, objective, trainer refusals
class _Inner:
    device = torch.device("cpu")

    def empty_inputs(self, B, with_ids=True):
        return (torch.zeros(B, 2, dtype=torch.int64),) * 2

    def gather(self, u, i, out=None):
        return "gathered", u, i

    def inputs(self, u, i, with_ids=True):
        return "inputs", u, i


def test_in_batch_feed_refuses_what_it_cannot_serve():
    from review_based_recommender_amd.data import InBatchFeed
    off, items = torch.tensor([0, 1, 2]), torch.tensor([3, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="wraps an id feed"):
        InBatchFeed(object(), None)
    for lo in (-1, True, 1.5):
        with pytest.raises(ValueError, match="item_lo"):
            InBatchFeed(_Inner(), None, item_lo=lo)
    with pytest.raises(ValueError, match="one row per user id"):
        InBatchFeed(_Inner(), (off, items, off))
    with pytest.raises(ValueError, match="seen must be"):
        InBatchFeed(_Inner(), (off, items.to(torch.int64)))
    with pytest.raises(ValueError, match="seen must be"):
        InBatchFeed(_Inner(), (off.to(torch.int32), items))
    f = InBatchFeed(_Inner(), (off, items), item_lo=2)
    with pytest.raises(RuntimeError, match=r"\[B\] each"):
        f.gather(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))


def test_in_batch_feed_keeps_references_to_the_last_gathers_ids():
    from review_based_recommender_amd.data import InBatchFeed
    f = InBatchFeed(_Inner(), None)
    assert f.item_lo == 1 and f.seen is None and f._last is None
    u, i = torch.arange(4), torch.arange(4) + 1
    assert f.gather(u, i)[0] == "gathered" and f.u_ids is u and f.i_ids is i          # references: a slot's own static tensors
    u2, i2 = torch.arange(4) + 2, torch.arange(4) + 3
    assert f.inputs(u2, i2)[0] == "inputs" and f.u_ids is u2 and f.i_ids is i2
    assert len(f.empty_inputs(5)) == 2 and f.empty_inputs(5)[0].shape == (5, 2)


def test_objective_refuses_what_it_cannot_serve():
    from review_based_recommender_amd.data import InBatchFeed
    from review_based_recommender_amd.train_step import InBatchSoftmaxObjective

    class _Model:
        def pair_latents(self, *b):
            return None

        def score_mode_and_params(self):
            return "dot", None, None, None, None

    feed = InBatchFeed(_Inner(), None)
    with pytest.raises(ValueError, match="two-tower model"):
        InBatchSoftmaxObjective(object(), feed)
    with pytest.raises(ValueError, match="InBatchFeed"):
        InBatchSoftmaxObjective(_Model(), _Inner())
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            InBatchSoftmaxObjective(_Model(), feed, temperature=t)
    with pytest.raises(RuntimeError, match="gathered no batch"):
        InBatchSoftmaxObjective(_Model(), feed).forward_loss(_Model(), ())


SOFTMAX = dict(loss="softmax", device_cache=True, eval_from_towers=True, rank_metrics=[5], select_by="ndcg@5")


@pytest.mark.parametrize("kind,cfg,text", [
    ("deepconn", dict(SOFTMAX, device_cache=False, eval_from_towers=False, rank_metrics=[], select_by="rmse"), "needs device_cache"),
    ("narre", dict(SOFTMAX, device_cache=False, eval_from_towers=False, rank_metrics=[], select_by="rmse"), "needs device_cache"),
    ("deepconn", dict(SOFTMAX, select_by="rmse"), "needs a rank metric in select_by"),
    ("dual_att", dict(SOFTMAX, select_by="rmse"), "needs a rank metric in select_by"),
    ("deepconn", dict(loss="softmax", device_cache=True, parallel=True), "not available with parallel"),
    ("deepconn", dict(SOFTMAX, softmax_temperature=0), "softmax_temperature"),
    ("deepconn", dict(SOFTMAX, softmax_temperature="1"), "softmax_temperature"),
    ("deepconn", dict(SOFTMAX, softmax_temperature=True), "softmax_temperature"),
])
def test_trainer_refuses_what_the_softmax_path_cannot_serve(kind, cfg, text):
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises(ValueError, match=text):
        ReviewExperiment(kind, Args(dict(cfg, data_dir="/nonexistent", model_name=kind)))


def test_softmax_is_a_loss_of_the_trainer_with_its_defaults():
    from review_based_recommender_amd import trainer
    assert "softmax" in trainer.LOSSES and trainer.LOSSES[:2] == ("mse", "bpr")
    assert trainer.DEFAULTS["softmax_temperature"] == 1.0 and trainer.DEFAULTS["logq_correction"] is False
