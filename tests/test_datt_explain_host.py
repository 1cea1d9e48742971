"""CPU checks behind D-ATT's explanation: the closed form of rbr_datt_saliency (tests/datt_explain_ref.py) against float64
autograd of the whole pair score, the entry's declaration and host-side refusals, the CLI rules of --attention, and the models
that are not covered.  No kernel runs."""
import pytest
import torch

import datt_explain_ref as X
import synth
from helpers import quiet


@pytest.mark.parametrize("cfgname,seed", [("tiny", 1), ("tiny", 2), ("small", 1), ("small", 3)])
def test_closed_form_is_autograd_through_both_gates(cfgname, seed):
    cfg = synth.DATT_CFGS[cfgname]
    sd, b = synth.datt_params(cfg, seed=seed), synth.datt_batch(cfg, seed=seed + 10)
    r = X.datt_pair(sd, b["u_docs"], b["i_docs"])
    table = sd["word_embeddings.embedding.weight"]
    for side, docs in (("user", b["u_docs"]), ("item", b["i_docs"])):
        got = X.saliency(table, docs, r[f"{side}_local_gate"], r[f"{side}_global_gate"], r[f"{side}_ws"], 1, r[f"{side}_feat"],
                         r[f"{side}_argmax"], r[f"{side}_d_feat"], r[f"{side}_w_l"], r[f"{side}_w_g"])
        tokens = got["fixed"][0] + got["through"][0]
        scale = float(r[f"{side}_tokens"].abs().max())
        assert scale > 0
        assert float((tokens - r[f"{side}_tokens"]).abs().max()) <= 1e-12 * scale
        assert float((got["fixed"][0] - r[f"{side}_tokens_fixed"]).abs().max()) <= 1e-12 * scale
        for name in ("d_gate_l", "d_gate_g"):
            want = r[f"{side}_{name}"]
            assert float(want.abs().max()) > 0
            assert float((got[name][0] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        # the gate path is no rounding term: the closed form without it misses the gradient
        assert float(got["through"][0].abs().sum()) > 1e-3 * float(tokens.abs().sum())
        for name, (val, ab, n) in got.items():
            assert bool((ab >= val.abs() * (1 - 1e-12)).all()) and bool((n >= 0).all()), name


def test_reference_margins_of_the_seeds_the_gpu_test_uses():
    """bad_margins of the (parameter seed s, batch seed s + 10) pairs: the GPU comparison runs on the clean ones only."""
    for cfgname, clean, unclean in (("tiny", (1, 2, 3, 4, 5, 6), ()), ("small", (1, 3, 5, 6), (2, 4))):
        cfg = synth.DATT_CFGS[cfgname]
        for s in clean + unclean:
            r = X.datt_pair(synth.datt_params(cfg, seed=s), *(synth.datt_batch(cfg, seed=s + 10)[k] for k in ("u_docs", "i_docs")))
            assert (r["bad_margins"] == 0) == (s in clean), (cfgname, s, r["bad_margins"])


def test_datt_saliency_is_declared_in_header_binding_and_library():
    import ctypes as C
    import os
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int rbr_datt_saliency(" in open(os.path.join(root, "include", "rbr_hip.h")).read()
    assert "rbr_datt_saliency" in _lib.SIGNATURES and len(_lib.SIGNATURES["rbr_datt_saliency"][1]) == 16
    L = _lib.lib()

    def call(desc, win=5, ptr=None):
        return L.rbr_datt_saliency(None if desc is None else C.byref(desc), *([ptr] * 7), win, *([ptr] * 6), None)

    def desc(kzs=(1, 2, 3, 4), split=1, n_docs=2):
        flags = _lib.conv_gate_split(split) if split else 0
        return _lib.make_desc(n_docs, 8, 4, 10, list(kzs), [2] * len(kzs), _lib.PAD_VALID, _lib.ACT_TANH, None, flags)

    # host-side refusals need no GPU; every one names its cause, and nothing is launched
    assert call(None) == -1 and b"null descriptor" in L.rbr_last_error()
    assert call(desc()) == -1 and b"null pointer" in L.rbr_last_error()
    assert call(desc(split=0)) == -1 and b"GATE_SPLIT" in L.rbr_last_error()
    for win in (0, -1, 2, 4):
        assert call(desc(), win) == -1 and b"odd" in L.rbr_last_error()
    assert call(desc(), 11) == -2 and b"win = 11" in L.rbr_last_error()
    wide = desc()
    wide.kz[3] = 10
    assert call(wide) == -2 and b"width 10" in L.rbr_last_error()
    for win in (1, 3, 5, 7, 9):                                          # accepted windows get as far as the pointer check
        assert call(desc(), win) == -1 and b"null pointer" in L.rbr_last_error()
    assert call(desc(split=3)) == -1 and b"null pointer" in L.rbr_last_error()
    assert call(desc(n_docs=0)) == 0                                     # an empty batch is a no-op
    # the un-gated entry keeps refusing a split gate
    assert L.rbr_textcnn_saliency(C.byref(desc()), *([None] * 10)) == -2 and b"GATE_SPLIT" in L.rbr_last_error()


def test_parse_cli_rules_for_attention():
    from review_based_recommender_amd.recommend import parse_cli
    base = ["--model", "dual_att", "--config", "c.json", "--checkpoint", "m.pt"]
    a = parse_cli(base + ["--out", "o.jsonl", "--attention", "3"])
    assert a.attention == 3 and a.explain is None
    assert parse_cli(base + ["--out", "o.jsonl"]).attention is None
    for bad in (["--eval-split", "test", "--attention", "3"],                      # --attention without --out
                ["--out", "o.jsonl", "--attention", "0"], ["--out", "o.jsonl", "--attention", "-2"]):
        with pytest.raises(SystemExit):
            quiet(parse_cli, base + bad)
    for model in ("deepconn", "narre", "simple_siamese", "ahn"):
        with pytest.raises(SystemExit):
            quiet(parse_cli, ["--model", model, "--config", "c.json", "--checkpoint", "m.pt", "--out", "o", "--attention", "2"])


def test_explain_with_dual_att_still_exits():
    from review_based_recommender_amd.recommend import parse_cli
    with pytest.raises(SystemExit):
        quiet(parse_cli, ["--model", "dual_att", "--config", "c.json", "--checkpoint", "m.pt", "--out", "o", "--explain", "2"])


def test_attention_covers_datt_only():
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    from review_based_recommender_amd.recommend import Recommender
    c = synth.SIAMESE_CFGS["tiny"]
    siam = quiet(SimpleSiamese, c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.5, 0.2, 0.1, c["UB"], c["LT"])
    rec = Recommender(siam, user=torch.zeros(3, 2, 4, dtype=torch.int64), item=torch.zeros(3, 2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="covers D-ATT"):
        rec.attention(torch.tensor([1]), torch.tensor([1]))
    c = synth.DATT_CFGS["tiny"]
    datt = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    rec = Recommender(datt, user=torch.zeros(3, 16, dtype=torch.int64), item=torch.zeros(3, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):                # explain keeps refusing D-ATT
        rec.explain(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError, match="B >= 1"):
        rec.attention(torch.tensor([[1]]), torch.tensor([[1]]))
    with pytest.raises(RuntimeError, match="refresh"):                               # covered, but there are no tables yet
        rec.attention(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):
        datt.explain_users(torch.zeros(2, 16, dtype=torch.int64))
