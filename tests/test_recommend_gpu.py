"""Scores and top-K recommendation from cached tower latents on the GPU (csrc/pair_score.hip through functional.pair_score*,
the models' encode_users / encode_items, recommend.Recommender, the trainer's eval_from_towers).

Yardsticks: the reference's eval predictions of the committed fixtures (1e-4, the project's FWD_TOL); the score formula
recomputed in float64 from the same fp32 tables with the fp32 rounding bound (K + 3) * 2^-23 * (sum_k |t_k| + |ub| + |ib| + |g|)
(K products and K + 2 additions, a factor 2 of slack); torch.sort(stable) of the dense scores for the ranking, compared exactly."""
import json
import math

import numpy as np
import pytest
import torch

import make_dataset
import synth
from helpers import golden, max_err, quiet

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-4          # BASELINE.json north_star: outputs within 1e-4 (fp32) of the reference CPU forward
DEV = "cuda:0"
NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ parity with the reference
def _deepconn(cfgname):
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    c = synth.DEEPCONN_CFGS[cfgname]
    m = quiet(DeepCoNNpp, c["U"], c["I"], c["V"], c["kz"], c["D"], c["H"], c["K"], c["L"], None, 0.5)
    m.load_state_dict(synth.deepconn_params(c, 0))
    b = synth.deepconn_batch(c, 1, edge_cases=cfgname != "cfg1")
    return m, (b["u_docs"], b["u_masks"], b["u_ids"]), (b["i_docs"], b["i_masks"], b["i_ids"]), b["u_ids"], b["i_ids"]


def _narre(cfgname):
    from review_based_recommender_amd.models.narre.narre import NARRE
    c = synth.NARRE_CFGS[cfgname]
    m = quiet(NARRE, c["U"], c["I"], c["V"], c["kz"], c["H"], c["D"], c["A"], c["K"], c["R"], c["T"], 0.5, 0, 0, 0, None, "CNN")
    m.load_state_dict(synth.narre_params(c, 0))
    b = synth.narre_batch(c, 1, edge_cases=True)
    return (m, (b["u_text"], b["u_masks"], b["u_id"], b["reuid"]), (b["i_text"], b["i_masks"], b["i_id"], b["reiid"]), b["u_id"],
            b["i_id"])


def _datt(cfgname):
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    c = synth.DATT_CFGS[cfgname]
    m = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    m.load_state_dict(synth.datt_params(c, 0))
    b = synth.datt_batch(c, 1, edge_cases=True)
    return m, (b["u_docs"],), (b["i_docs"],), None, None


def _siamese(cfgname):
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    c = synth.SIAMESE_CFGS[cfgname]
    m = quiet(SimpleSiamese, c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.5, 0.2, 0.1, c["UB"], c["LT"])
    m.load_state_dict(synth.siamese_params(c, 0))
    b = synth.siamese_batch(c, 1, edge_cases=True)
    return (m, (b["u_revs"], b["u_word_masks"], b["u_rev_masks"], b["u_ids"]),
            (b["i_revs"], b["i_word_masks"], b["i_rev_masks"], b["i_ids"]), b["u_ids"], b["i_ids"])


@pytest.mark.parametrize("name,build,cfgname", [
    ("deepconn_tiny", _deepconn, "tiny"), ("deepconn_small", _deepconn, "small"), ("deepconn_cfg1", _deepconn, "cfg1"),
    ("narre_tiny", _narre, "tiny"), ("narre_small", _narre, "small"),
    ("datt_tiny", _datt, "tiny"), ("datt_small", _datt, "small"),
    ("siamese_tiny", _siamese, "tiny"), ("siamese_small", _siamese, "small")])
def test_tower_latents_reproduce_the_reference_predictions(golden_dir, name, build, cfgname):
    """The batch's B user rows and B item rows encoded side by side; the diagonal of the dense [B, B] scores, and the id-paired
    scores, against the fixture's eval predictions.  The model is left in train mode with dropout 0.5 everywhere: the encode
    methods have eval semantics whatever the mode, and restore it."""
    from review_based_recommender_amd import functional as RF
    g = golden(golden_dir, name)
    model, u_args, i_args, u_ids, i_ids = build(cfgname)
    model.to(DEV).train()
    ul = model.encode_users(*[t.to(DEV) for t in u_args])
    il = model.encode_items(*[t.to(DEV) for t in i_args])
    assert model.training and not ul.requires_grad
    B = u_args[0].shape[0]
    assert ul.shape == il.shape and ul.shape[0] == B
    mode, h, gb, ub, ib = model.score_mode_and_params()
    # latent rows are per batch row here; the id-keyed biases are gathered to rows the same way
    ub_rows = ub.detach()[u_ids.to(DEV)] if ub is not None else None
    ib_rows = ib.detach()[i_ids.to(DEV)] if ib is not None else None
    dense = RF.pair_score_dense(mode, ul, il, h, gb, ub_rows, ib_rows)
    assert dense.shape == (B, B)
    err = max_err(dense.diagonal().cpu().numpy(), g["pred_eval"])
    print(f"{name}: max |dense diagonal - pred_eval| = {err:.3e}")
    assert err <= FWD_TOL
    rows = torch.arange(B, device=DEV)
    paired = RF.pair_score(mode, ul, il, rows, rows, h, gb, ub_rows, ib_rows)
    err = max_err(paired.cpu().numpy(), g["pred_eval"])
    print(f"{name}: max |paired - pred_eval| = {err:.3e}")
    assert err <= FWD_TOL
    assert torch.equal(paired.view(torch.int32), dense.diagonal().contiguous().view(torch.int32))
    RF.check_id_errors(DEV)


def test_single_side_encodes_take_unequal_row_counts():
    """encode_users / encode_items are one-sided: 3 users and 7 items give the rows the full batch gave."""
    model, u_args, i_args, _, _ = _deepconn("small")
    model.to(DEV).eval()
    ul = model.encode_users(*[t.to(DEV) for t in u_args])
    il = model.encode_items(*[t.to(DEV) for t in i_args])
    ul3 = model.encode_users(*[t[:3].to(DEV) for t in u_args])
    il7 = model.encode_items(*[t[:7].to(DEV) for t in i_args])
    assert ul3.shape == (3, ul.shape[1]) and il7.shape == (7, il.shape[1])
    # both encodes restate the same reference rows, each within FWD_TOL (the conv formulation may differ with the row count)
    assert max_err(ul3.cpu().numpy(), ul[:3].cpu().numpy()) <= FWD_TOL and max_err(il7.cpu().numpy(), il[:7].cpu().numpy()) <= FWD_TOL


# ------------------------------------------------------------------------------------------------ arithmetic
def _tables(Nu, Ni, K, seed, biases=True):
    gen = torch.Generator().manual_seed(seed)
    ul, il = torch.randn(Nu, K, generator=gen), torch.randn(Ni, K, generator=gen)
    h, g = torch.randn(K, 1, generator=gen), torch.randn(1, generator=gen)
    ub, ib = (torch.randn(Nu, 1, generator=gen), torch.randn(Ni, 1, generator=gen)) if biases else (None, None)
    return ul, il, h, g, ub, ib


def _to_dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _float64_scores(mode, ul, il, h, g, ub, ib):
    """(score, bound) in float64 from the fp32 tables: bound = (K + 3) 2^-23 (sum_k |t_k| + |ub| + |ib| + |g|)."""
    K = ul.shape[1]
    t = ul.double()[:, None, :] * il.double()[None, :, :]
    extra = torch.zeros(ul.shape[0], il.shape[0], dtype=torch.float64)
    if mode == "fm":
        t = torch.relu(t) * h.double().view(1, 1, K)
        score = t.sum(-1) + g.double()
        extra = extra + g.double().abs()
        if ub is not None:
            score = score + ub.double().view(-1, 1) + ib.double().view(1, -1)
            extra = extra + ub.double().abs().view(-1, 1) + ib.double().abs().view(1, -1)
    else:
        score = t.sum(-1)
    return score, (K + 3) * 2.0 ** -23 * (t.abs().sum(-1) + extra)


@pytest.mark.parametrize("biases", [True, False])
@pytest.mark.parametrize("mode", ["fm", "dot"])
@pytest.mark.parametrize("Ni", [2, 1003])
@pytest.mark.parametrize("Nu", [1, 257])
@pytest.mark.parametrize("K", [4, 8, 32, 50])
def test_scores_against_float64_and_bit_identity_of_the_three_entries(K, Nu, Ni, mode, biases):
    from review_based_recommender_amd import functional as RF
    ul, il, h, g, ub, ib = _tables(Nu, Ni, K, seed=K * 7 + Nu + Ni, biases=biases)
    d_ul, d_il, d_h, d_g, d_ub, d_ib = _to_dev(ul, il, h, g, ub, ib)
    dense = RF.pair_score_dense(mode, d_ul, d_il, d_h, d_g, d_ub, d_ib)
    ref, bound = _float64_scores(mode, ul, il, h, g, ub, ib)
    ratio = ((dense.cpu().double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"K={K} Nu={Nu} Ni={Ni} {mode} biases={biases}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the id entry: random pairs, plus every corner of the tables
    gen = torch.Generator().manual_seed(1)
    u_ids = torch.cat([torch.randint(0, Nu, (300,), generator=gen), torch.tensor([0, Nu - 1, 0, Nu - 1])])
    i_ids = torch.cat([torch.randint(0, Ni, (300,), generator=gen), torch.tensor([0, 0, Ni - 1, Ni - 1])])
    paired = RF.pair_score(mode, d_ul, d_il, u_ids.to(DEV), i_ids.to(DEV), d_h, d_g, d_ub, d_ib)
    assert torch.equal(paired.cpu().view(torch.int32), dense.cpu()[u_ids, i_ids].view(torch.int32))
    # the top-K entry: the scores it reports are the dense entries of the items it reports
    k = min(10, Ni)
    items, scores = RF.pair_score_topk(mode, d_ul, d_il, k, d_h, d_g, d_ub, d_ib)
    assert int(items.min()) >= 0
    assert torch.equal(scores.cpu().view(torch.int32), torch.gather(dense.cpu(), 1, items.cpu()).view(torch.int32))
    RF.check_id_errors(DEV)


def test_out_of_range_ids_score_as_row_zero_and_are_reported():
    from review_based_recommender_amd import functional as RF
    ul, il, h, g, ub, ib = _to_dev(*_tables(5, 6, 8, seed=3))
    RF.check_id_errors(DEV)
    got = RF.pair_score("fm", ul, il, torch.tensor([2, 5, -1, 3], device=DEV), torch.tensor([1, 2, 3, 6], device=DEV), h, g, ub, ib)
    want = RF.pair_score("fm", ul, il, torch.tensor([2, 0, 0, 3], device=DEV), torch.tensor([1, 2, 3, 0], device=DEV), h, g, ub, ib)
    assert torch.equal(got, want)
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)        # the record is cleared


# ------------------------------------------------------------------------------------------------ ranking
def _yardstick(dense, k, item_lo, exclude=None):
    """torch.sort(stable, descending) of the dense scores with the excluded and < item_lo columns at -inf; slots that hold a
    masked column are the fill: item -1, score -inf."""
    d = dense.clone()
    Nu, Ni = d.shape
    d[:, :item_lo] = NEG_INF
    if exclude is not None:
        off, items = exclude[0].cpu(), exclude[1].cpu().long()
        rows = torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])
        if len(exclude) > 2:                       # CSR over ids, user row r takes row exclude[2][r]
            ids = exclude[2].cpu()
            for r in range(Nu):
                d[r, items[int(off[ids[r]]):int(off[ids[r] + 1])].to(d.device)] = NEG_INF
        else:
            d[rows.to(d.device), items.to(d.device)] = NEG_INF
    s, idx = torch.sort(d, dim=1, descending=True, stable=True)
    s, idx = s[:, :k], idx[:, :k]
    if k > Ni:
        s = torch.cat([s, torch.full((Nu, k - Ni), NEG_INF, device=s.device)], 1)
        idx = torch.cat([idx, torch.full((Nu, k - Ni), -1, dtype=idx.dtype, device=idx.device)], 1)
    return torch.where(s == NEG_INF, torch.full_like(idx, -1), idx).contiguous(), s.contiguous()


def _assert_same_ranking(got, want, what):
    (gi, gs), (wi, ws) = got, want
    assert gi.dtype == torch.int64 and gs.dtype == torch.float32 and gi.shape == wi.shape
    bad = (gi != wi).any(1) | (gs.view(torch.int32) != ws.view(torch.int32)).any(1)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {gi.shape[0]} rows differ, first row {int(bad.nonzero()[0])}"


def _random_csr(Nu, Ni, gen, max_per_row, full_rows=()):
    off, items = [0], []
    for r in range(Nu):
        n = Ni if r in full_rows else int(torch.randint(0, max_per_row + 1, (1,), generator=gen))
        row = torch.randperm(Ni, generator=gen)[:n].sort().values
        items.append(row)
        off.append(off[-1] + n)
    return torch.tensor(off, dtype=torch.int64), torch.cat(items).to(torch.int32)


@pytest.mark.parametrize("mode", ["fm", "dot"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_topk_matches_a_stable_sort_257_by_1003(k, mode):
    """No exclusions, per-user exclusion lists (empty rows, rows that cover every item), item_lo 0 and 1, duplicated item rows
    (exact ties, broken by the lower id), and the same bytes from two calls in a row."""
    from review_based_recommender_amd import functional as RF
    Nu, Ni, K = 257, 1003, 32
    ul, il, h, g, ub, ib = _tables(Nu, Ni, K, seed=11 + k)
    gen = torch.Generator().manual_seed(5)
    dup = torch.randint(0, Ni, (200,), generator=gen)              # 200 items become copies of other items: exact ties
    src = torch.randint(0, Ni, (200,), generator=gen)
    il[dup], ib[dup] = il[src].clone(), ib[src].clone()
    ul, il, h, g, ub, ib = _to_dev(ul, il, h, g, ub, ib)
    dense = RF.pair_score_dense(mode, ul, il, h, g, ub, ib)
    assert int((dense[:, :, None] == dense[:, None, :64]).sum()) > Nu * 64          # ties exist beyond the diagonal
    for item_lo in (0, 1):
        got = RF.pair_score_topk(mode, ul, il, k, h, g, ub, ib, item_lo=item_lo)
        _assert_same_ranking(got, _yardstick(dense, k, item_lo), f"item_lo={item_lo}")
    again = RF.pair_score_topk(mode, ul, il, k, h, g, ub, ib, item_lo=1)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))
    off, items = _random_csr(Nu, Ni, torch.Generator().manual_seed(6), max_per_row=40, full_rows=(0, 100, Nu - 1))
    assert bool((off[1:] == off[:-1]).any())                                          # some rows exclude nothing
    excl = (off.to(DEV), items.to(DEV))
    got = RF.pair_score_topk(mode, ul, il, k, h, g, ub, ib, item_lo=1, exclude=excl)
    _assert_same_ranking(got, _yardstick(dense, k, 1, excl), "per-user exclusion")
    assert bool((got[0][0] == -1).all()) and bool((got[1][100] == NEG_INF).all())    # rows whose list covers every item
    empty = (torch.zeros(Nu + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    _assert_same_ranking(RF.pair_score_topk(mode, ul, il, k, h, g, ub, ib, item_lo=1, exclude=empty), _yardstick(dense, k, 1),
                         "empty exclusion")
    # a CSR over ids serving a block of user rows through a row map
    ids = torch.randint(0, Nu, (Nu,), generator=gen)
    mapped = (off.to(DEV), items.to(DEV), ids.to(DEV))
    _assert_same_ranking(RF.pair_score_topk(mode, ul, il, k, h, g, ub, ib, item_lo=1, exclude=mapped), _yardstick(dense, k, 1, mapped),
                         "mapped exclusion")


@pytest.mark.parametrize("k", [1, 10, 128])
def test_topk_matches_a_stable_sort_512_by_100003(k):
    from review_based_recommender_amd import functional as RF
    Nu, Ni, K = 512, 100003, 32
    ul, il, h, g, ub, ib = _tables(Nu, Ni, K, seed=23)
    gen = torch.Generator().manual_seed(7)
    dup, src = torch.randint(0, Ni, (5000,), generator=gen), torch.randint(0, Ni, (5000,), generator=gen)
    il[dup], ib[dup] = il[src].clone(), ib[src].clone()
    ul, il, h, g, ub, ib = _to_dev(ul, il, h, g, ub, ib)
    dense = RF.pair_score_dense("fm", ul, il, h, g, ub, ib)
    got = RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1)
    _assert_same_ranking(got, _yardstick(dense, k, 1), "no exclusion")
    again = RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))
    # every user excludes its own current top 50 and a random handful: the ranking moves down exactly
    top50 = torch.sort(dense, dim=1, descending=True, stable=True).indices[:, :50].cpu()
    rows = [torch.unique(torch.cat([top50[r], torch.randint(0, Ni, (int(torch.randint(0, 30, (1,), generator=gen)),), generator=gen)]))
            for r in range(Nu)]
    off = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    excl = (off.to(DEV), torch.cat(rows).to(torch.int32).to(DEV))
    _assert_same_ranking(RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1, exclude=excl), _yardstick(dense, k, 1, excl),
                         "per-user exclusion")
    del dense


@pytest.mark.parametrize("Ni,item_lo,k", [(2, 1, 10), (2, 0, 128), (7, 1, 7), (65, 1, 128), (130, 3, 128)])
def test_fewer_candidates_than_k_end_in_the_fill(Ni, item_lo, k):
    from review_based_recommender_amd import functional as RF
    ul, il, h, g, ub, ib = _to_dev(*_tables(19, Ni, 8, seed=Ni))
    dense = RF.pair_score_dense("fm", ul, il, h, g, ub, ib)
    items, scores = RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=item_lo)
    _assert_same_ranking((items, scores), _yardstick(dense, k, item_lo), "fill")
    n = Ni - item_lo
    assert bool((items[:, :n] >= item_lo).all()) and bool((items[:, n:] == -1).all()) and bool((scores[:, n:] == NEG_INF).all())


def test_unsupported_k_is_an_error_not_a_fallback():
    from review_based_recommender_amd import functional as RF
    ul, il, h, g, ub, ib = _to_dev(*_tables(4, 300, 8, seed=1))
    for k in (0, 129):
        with pytest.raises(RuntimeError, match="rbr_pair_score_topk failed"):
            RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib)


def test_topk_records_into_a_graph_and_replays_with_new_latents():
    """One capture of topk on a single stream (the conventions of train_step.GraphedForward: warm-up on a side stream, the
    library's capture guard around the recording), one replay after the latent VALUES changed in place."""
    from review_based_recommender_amd import _lib, functional as RF
    from review_based_recommender_amd.train_step import _capture_stream
    Nu, Ni, K, k = 64, 5000, 32, 10
    ul, il, h, g, ub, ib = _to_dev(*_tables(Nu, Ni, K, seed=31))
    off, items = _random_csr(Nu, Ni, torch.Generator().manual_seed(2), max_per_row=20)
    excl = (off.to(DEV), items.to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1, exclude=excl)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cs = _capture_stream(torch.device(DEV))
    with _lib.capture_guard(cs), torch.cuda.graph(graph, stream=cs, capture_error_mode="global"):
        out = RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1, exclude=excl)
    ul2, il2, _, _, ub2, ib2 = _to_dev(*_tables(Nu, Ni, K, seed=32))
    for dst, new in ((ul, ul2), (il, il2), (ub, ub2), (ib, ib2)):
        dst.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    dense = RF.pair_score_dense("fm", ul, il, h, g, ub, ib)
    _assert_same_ranking((out[0].clone(), out[1].clone()), _yardstick(dense, k, 1, excl), "graph replay")


# ------------------------------------------------------------------------------------------------ end to end
def _doc_experiment_model(tmp_path):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)
    ds = D.DocDataset(data_dir, "train")
    torch.manual_seed(0)
    m = quiet(DeepCoNNpp, ds.user_num, ds.item_num, ds.vocab_size, [3, 5], 12, 8, 4, ds.doc_len, None, 0.5).to(DEV)
    return data_dir, ds, m


def test_recommender_scores_like_the_model_and_never_recommends_seen_items(tmp_path):
    from review_based_recommender_amd import data as D, functional as RF
    from review_based_recommender_amd.recommend import Recommender
    _, ds, m = _doc_experiment_model(tmp_path)
    cache = D.DeviceDocCache(ds, DEV)
    m.train()
    rec = Recommender(m, cache)
    assert rec.stale
    rec.refresh(chunk=5)                     # ragged chunks: 12 users and 10 items in blocks of 5
    assert not rec.stale and m.training
    assert rec.user_latents.shape == (ds.user_num, 4) and rec.item_latents.shape == (ds.item_num, 4)
    u = torch.tensor([e[0] for e in ds.examples], device=DEV)
    i = torch.tensor([e[1] for e in ds.examples], device=DEV)
    m.eval()
    with torch.no_grad():
        want = m(*cache.inputs(u, i))
    got = rec.score(u, i)
    err = float((got - want).abs().max())
    print(f"max |Recommender.score - model forward| = {err:.3e}")
    assert err <= 2e-4                       # each path is held to 1e-4 against the reference
    users = torch.arange(1, ds.user_num, device=DEV)
    full = rec.score_all(users)
    assert full.shape == (ds.user_num - 1, ds.item_num)
    assert torch.equal(full[u - 1, i].view(torch.int32), got.view(torch.int32))
    seen = Recommender.seen_from(ds.examples, ds.user_num, DEV)
    items, scores = rec.topk(users, 5, exclude=seen)
    rated = {(int(e[0]), int(e[1])) for e in ds.examples}
    for r, uid in enumerate(users.tolist()):
        row = [x for x in items[r].tolist() if x >= 0]
        assert 0 not in row and not any((uid, x) in rated for x in row)
        assert len(row) == min(5, ds.item_num - 1 - len({x for (a, x) in rated if a == uid}))
    _assert_same_ranking((items, scores), _yardstick(full, 5, 1, (seen.off, seen.items, users)), "Recommender.topk")
    with torch.no_grad():                    # a torch-side in-place update is seen by `stale`
        m.fm.g_bias.add_(1.0)
    assert rec.stale
    assert float((rec.refresh().score(u, i) - want - 1.0).abs().max()) <= 2e-4
    RF.check_id_errors(DEV)


def test_cli_writes_one_line_per_user(tmp_path):
    from review_based_recommender_amd import recommend
    data_dir, ds, m = _doc_experiment_model(tmp_path)
    cfg = {"data_dir": data_dir, "model_name": "deepconn", "kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12,
           "latent_dim": 4, "dropout": 0.5}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    torch.save({"model": m.state_dict(), "optimizer": {}, "updates": 0, "args": cfg}, tmp_path / "best_model.pt")
    out = tmp_path / "recs.jsonl"
    rc = recommend.main(["--model", "deepconn", "--config", str(tmp_path / "cfg.json"), "--checkpoint", str(tmp_path / "best_model.pt"),
                         "--k", "4", "--exclude-train", "--out", str(out), "--chunk", "5"])
    assert rc == 0
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == ds.user_num - 1 and [l["user"] for l in lines] == list(range(1, ds.user_num))
    rated = {(int(e[0]), int(e[1])) for e in ds.examples}
    for l in lines:
        assert len(l["items"]) == len(l["scores"]) <= 4 and 0 not in l["items"]
        assert l["scores"] == sorted(l["scores"], reverse=True)
        assert not any((l["user"], x) in rated for x in l["items"])


@pytest.mark.parametrize("kind", ["deepconn", "dual_att"])
def test_trainer_validates_from_towers_like_the_default_path(tmp_path, kind):
    """eval_from_towers: the validation RMSE from latent tables against the default id-fed forward, same parameters.  RMSE is
    1-Lipschitz in the largest prediction difference, so 2e-4 is the bound of the predictions themselves."""
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": kind, "kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12, "latent_dim": 4, "dropout": 0.5,
           "epochs": 1, "batch_size": 16, "l_window_size": 5, "l_out_size": 8, "g_out_size": 4, "emb_size": 12, "hidden_size_1": 10,
           "hidden_size_2": 5, "device_cache": True, "patience": 100}
    rmse = {}
    state = None
    for towers in (False, True):
        path = tmp_path / f"{kind}_{int(towers)}.json"
        path.write_text(json.dumps(dict(cfg, eval_from_towers=towers)))
        exp = ReviewExperiment(kind, parse_args(str(path)), uid=f"v{int(towers)}")
        if state is None:
            exp.train_one_epoch(0)
            state = {k: v.clone() for k, v in exp.model.state_dict().items()}
        else:
            exp.model.load_state_dict(state)
        exp.valid_one_epoch()
        assert exp.valid_count == len(exp.valid_set)
        rmse[towers] = exp.last_valid_rmse
    print(f"{kind}: validation rmse default {rmse[False]:.7f}, from towers {rmse[True]:.7f}")
    assert math.isfinite(rmse[False]) and abs(rmse[True] - rmse[False]) <= 2e-4
    with pytest.raises(ValueError, match="eval_from_towers"):
        bad = tmp_path / "bad.json"
        bad.write_text(json.dumps(dict(cfg, eval_from_towers=True, device_cache=False)))
        ReviewExperiment(kind, parse_args(str(bad)), uid="bad")
