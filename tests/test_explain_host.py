"""CPU checks behind the explanation feature: the closed form of rbr_textcnn_saliency (tests/explain_ref.py) against float64
autograd, its completeness, top_tokens' order, the CLI rules of --explain, and the models that are not covered.  No kernel runs."""
import numpy as np
import pytest
import torch

import explain_ref as X
import synth
from helpers import quiet


def _case(seed, n_docs, L, D, V, kzs, chans, valid, tanh, with_mask, with_gate):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, D, generator=g, dtype=torch.float64)
    ids = torch.randint(0, V, (n_docs, L), generator=g)
    mask = (torch.rand(n_docs, L, generator=g) > 0.25) if with_mask else None
    gate = (torch.rand(n_docs, L, generator=g, dtype=torch.float64) * 1.6 - 0.8) if with_gate else None
    ws = [torch.randn(c, D, k, generator=g, dtype=torch.float64) / np.sqrt(D * k) for k, c in zip(kzs, chans)]
    bs = [torch.randn(c, generator=g, dtype=torch.float64) * 0.1 for c in chans]
    d_feat = torch.randn(n_docs, sum(chans), generator=g, dtype=torch.float64)
    return table, ids, mask, gate, ws, bs, d_feat


@pytest.mark.parametrize("with_gate", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("tanh", [False, True])
@pytest.mark.parametrize("valid,kzs", [(False, [1, 3, 7]), (True, [2, 3, 4])])
def test_closed_form_is_autograd_gradient_times_input(valid, kzs, tanh, with_mask, with_gate):
    table, ids, mask, gate, ws, bs, d_feat = _case(11 + 2 * valid + tanh, 5, 23, 12, 40, kzs, [4, 5, 3], valid, tanh, with_mask,
                                                   with_gate)
    feat, argmax, want = X.autograd_saliency(table, ids, mask, gate, ws, bs, d_feat, valid, tanh)
    got, ab, cnt = X.saliency(table, ids, mask, gate, ws, feat, argmax, d_feat, valid, tanh, counts=True)
    scale = float(want.abs().max())
    assert scale > 0
    assert float((got - want).abs().max()) <= 1e-12 * scale
    assert bool((ab >= got.abs() - 1e-12 * scale).all()) and bool(((cnt == 0) == (ab == 0)).all())
    if with_mask:
        assert bool((got[~mask] == 0).all())
    if not tanh:                                                                   # completeness (ReLU)
        want_sum = X.relu_completeness(feat, d_feat, bs)
        assert float((got.sum(1) - want_sum).abs().max()) <= 1e-12 * (1 + float(want_sum.abs().max()))


def test_a_window_wider_than_the_document_and_out_of_range_argmax():
    table, ids, mask, gate, ws, bs, d_feat = _case(3, 4, 1, 8, 10, [3], [6], False, False, False, False)
    feat, argmax, want = X.autograd_saliency(table, ids, None, None, ws, bs, d_feat)
    got, _ = X.saliency(table, ids, None, None, ws, feat, argmax, d_feat)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    bad = argmax.clone()
    bad[0, :] = -1
    bad[1, :] = 6
    got2, ab2 = X.saliency(table, ids, None, None, ws, feat, bad, d_feat)
    assert bool((got2[:2] == 0).all()) and bool((ab2[:2] == 0).all()) and torch.equal(got2[2:], got[2:])


def test_pair_references_explain_their_own_score():
    """deepconn_pair / narre_pair: text = what the tower's features add through LastFeat, tokens sum to it up to the conv bias."""
    c = synth.DEEPCONN_CFGS["tiny"]
    sd, b = synth.deepconn_params(c, 0), synth.deepconn_batch(c, 1)
    ids = torch.arange(1, c["B"] + 1)
    r = X.deepconn_pair(sd, b["u_docs"], b["u_masks"], b["i_docs"], b["i_masks"], ids, ids)
    assert r["user_tokens"].shape == (c["B"], c["L"]) and bool((r["user_tokens"][~b["u_masks"]] == 0).all())
    assert bool(torch.isfinite(r["score"]).all()) and r["bad_margins"] >= 0
    c = synth.NARRE_CFGS["tiny"]
    sd, b = synth.narre_params(c, 0), synth.narre_batch(c, 1)
    ids = torch.arange(1, c["B"] + 1)
    r = X.narre_pair(sd, b["u_text"], b["u_masks"], b["i_text"], b["i_masks"], ids, ids, b["reuid"], b["reiid"])
    assert r["item_tokens"].shape == (c["B"], c["R"], c["T"])
    assert float((r["user_reviews"].sum(1) - r["user_text"]).abs().max()) <= 1e-12
    assert float((r["user_review_weights"].sum(1) - 1).abs().max()) <= 1e-6       # the softmax's + 1e-8


def test_top_tokens_order_and_tie_rule():
    from review_based_recommender_amd.recommend import top_tokens
    w = torch.tensor([[0.5, -2.0, 2.0, 0.0, -0.5, 2.0], [0.0, 0.0, 0.0, 1.0, -1.0, 0.0]])
    docs = torch.arange(12).view(2, 6) + 100
    pos, tok, wt = top_tokens(w, docs, 4)
    assert pos.tolist() == [[1, 2, 5, 0], [3, 4, 0, 1]]
    assert tok.tolist() == [[101, 102, 105, 100], [109, 110, 106, 107]]
    assert wt.tolist() == [[-2.0, 2.0, 2.0, 0.5], [1.0, -1.0, 0.0, 0.0]]
    pos3, _, _ = top_tokens(w.view(2, 2, 3), docs.view(2, 2, 3), 99)                # trailing dims flattened, n capped
    assert pos3.shape == (2, 6) and pos3[0].tolist() == [1, 2, 5, 0, 4, 3]
    with pytest.raises(ValueError):
        top_tokens(w, docs, 0)


def test_parse_cli_rules_for_explain():
    from review_based_recommender_amd.recommend import parse_cli
    base = ["--model", "deepconn", "--config", "c.json", "--checkpoint", "m.pt"]
    a = parse_cli(base + ["--out", "o.jsonl", "--explain", "3"])
    assert a.explain == 3
    assert parse_cli(base + ["--out", "o.jsonl"]).explain is None
    for bad in (["--eval-split", "test", "--explain", "3"],                        # --explain without --out
                ["--out", "o.jsonl", "--explain", "0"], ["--out", "o.jsonl", "--explain", "-2"]):
        with pytest.raises(SystemExit):
            quiet(parse_cli, base + bad)
    with pytest.raises(SystemExit):
        quiet(parse_cli, ["--model", "dual_att", "--config", "c.json", "--checkpoint", "m.pt", "--out", "o", "--explain", "2"])


def test_saliency_is_declared_in_header_binding_and_library():
    import ctypes as C
    import os
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int rbr_textcnn_saliency(" in open(os.path.join(root, "include", "rbr_hip.h")).read()
    assert "rbr_textcnn_saliency" in _lib.SIGNATURES and len(_lib.SIGNATURES["rbr_textcnn_saliency"][1]) == 11
    L = _lib.lib()
    # host-side refusals need no GPU: null descriptor, a bad descriptor, a split gate, null pointers; n_docs == 0 is a no-op
    assert L.rbr_textcnn_saliency(None, *([None] * 10)) == -1
    d = _lib.make_desc(2, 8, 4, 10, [3], [2], _lib.PAD_SAME, _lib.ACT_RELU, None)
    assert L.rbr_textcnn_saliency(C.byref(d), *([None] * 10)) == -1 and b"null pointer" in L.rbr_last_error()
    even = _lib.make_desc(2, 8, 4, 10, [4], [2], _lib.PAD_SAME, _lib.ACT_RELU, None)
    assert L.rbr_textcnn_saliency(C.byref(even), *([None] * 10)) == -1 and b"odd" in L.rbr_last_error()
    split = _lib.make_desc(2, 8, 4, 10, [1, 3], [2, 2], _lib.PAD_SAME, _lib.ACT_RELU, None, _lib.conv_gate_split(1))
    assert L.rbr_textcnn_saliency(C.byref(split), *([None] * 10)) == -2 and b"GATE_SPLIT" in L.rbr_last_error()
    empty = _lib.make_desc(0, 8, 4, 10, [3], [2], _lib.PAD_SAME, _lib.ACT_RELU, None)
    assert L.rbr_textcnn_saliency(C.byref(empty), *([None] * 10)) == 0


def test_models_outside_the_coverage_raise_value_errors():
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    from review_based_recommender_amd.recommend import Recommender
    c = synth.DATT_CFGS["tiny"]
    datt = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    c = synth.SIAMESE_CFGS["tiny"]
    siam = quiet(SimpleSiamese, c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.5, 0.2, 0.1, c["UB"], c["LT"])
    c = synth.DEEPCONN_CFGS["tiny"]
    hier = quiet(DeepCoNNpp, c["U"], c["I"], c["V"], [3], c["D"], c["H"], c["K"], c["L"], None, 0.5, arch="HierPooling")
    docs = torch.zeros(2, c["L"], dtype=torch.int64)
    for m, args in ((datt, (docs,)), (siam, (docs,)), (hier, (docs, docs != 0, torch.zeros(2, dtype=torch.int64), torch.zeros(2, c["K"])))):
        with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):
            m.explain_users(*args)
        with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):
            m.explain_items(*args)
    rec = Recommender(datt, user=torch.zeros(3, 16, dtype=torch.int64), item=torch.zeros(3, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):
        rec.explain(torch.tensor([1]), torch.tensor([1]))
