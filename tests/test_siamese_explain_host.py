"""CPU checks behind SimpleSiamese's explanation: the closed form of rbr_siamese_saliency (tests/siamese_explain_ref.py) against
float64 autograd, completeness, the f32 evaluation that licenses the GPU test's bound, the entry's declaration and host-side
refusals, the CLI rules of --contributions, and the models that are not covered.  No kernel runs."""
import pytest
import torch

import edge_refs as E
import siamese_explain_ref as X
import synth
from helpers import quiet

CASES = X.edge_cases()


def _from_model(cfgname, seed):
    """The op's inputs as the float64 tower of a synth model leaves them: (closed-form arguments, autograd results)."""
    cfg = synth.SIAMESE_CFGS[cfgname]
    sd, b = synth.siamese_params(cfg, seed=seed), synth.siamese_batch(cfg, seed=seed + 10, edge_cases=True)
    gen = torch.Generator().manual_seed(seed)
    F = cfg["K"] if cfg["LT"] else cfg["D"]
    g = torch.randn(cfg["B"], F, generator=gen, dtype=torch.float64)
    Wt, bt = sd.get("latent_transform_layer.0.weight"), sd.get("latent_transform_layer.0.bias")
    Wp, bp = sd["review_att_layer.proj_layer.0.weight"], sd["review_att_layer.proj_layer.0.bias"]
    wi = sd["review_att_layer.inner_product.weight"]
    table = sd["word_embedding.embedding.weight"]
    args = (table, b["u_revs"], b["u_word_masks"], b["u_rev_masks"])
    y, a, tokens, tokens_fixed = X.autograd_saliency(*args, g, Wt, bt, Wp, bp, wi)
    return args + (y, a, g, Wt, Wp, bp, wi), (tokens, tokens_fixed), b


@pytest.mark.parametrize("cfgname,seed", [("tiny", 1), ("tiny", 2), ("small", 1), ("small", 3)])
def test_closed_form_is_autograd_through_the_attention(cfgname, seed):
    args, (tokens, tokens_fixed), b = _from_model(cfgname, seed)
    got = X.saliency(*args)
    scale = float(tokens.abs().max())
    assert scale > 0
    assert float((got["fixed"][0] + got["through"][0] - tokens).abs().max()) <= 1e-12 * scale
    assert float((got["fixed"][0] - tokens_fixed).abs().max()) <= 1e-12 * scale
    # the softmax path is no rounding term: the closed form without it misses the gradient
    assert float(got["through"][0].abs().sum()) > 1e-3 * float(tokens.abs().sum())
    # row 0 has no review at all (uniform attention over empty bags): nothing to attribute, and nothing flows through
    assert not bool(b["u_rev_masks"][0].any()) and bool((got["through"][0][0] == 0).all()) and bool((got["fixed"][0][0] == 0).all())
    for name in ("fixed", "through", "reviews"):
        val, ab, n = got[name]
        assert bool((ab >= val.abs() * (1 - 1e-12)).all()) and n > 0, name


@pytest.mark.parametrize("cfgname,seed", [("tiny", 1), ("tiny", 2)])
def test_fixed_is_complete_without_the_transform(cfgname, seed):
    assert not synth.SIAMESE_CFGS[cfgname]["LT"]
    got = X.saliency(*_from_model(cfgname, seed)[0])
    reviews = got["reviews"][0]
    assert float(reviews.abs().max()) > 0
    assert float((got["fixed"][0].sum(-1) - reviews).abs().max()) <= 1e-7 * float(reviews.abs().max())      # the 1e-8 of inv_r


@pytest.mark.parametrize("name", sorted(CASES))
def test_f32_evaluation_in_another_order_lies_inside_the_bound(name):
    """What licenses the bound of tests/test_siamese_saliency_edges_gpu.py: an f32 evaluation that sums in another order than
    the kernel is held to the same per-element bound, at every edge case."""
    c = X.make_case(seed=sorted(CASES).index(name) + 1, **CASES[name])
    args = [c[k] for k in X.OP_ARGS]
    ref, got = X.saliency(*args), X.saliency_f32(*args)
    assert ref["pre_abs"] <= 1.0, "the through count assumes pre-activations of magnitude sum <= 1"
    for k in ("fixed", "through", "reviews"):
        val, ab, n = ref[k]
        E.check("siamese-saliency-f32-host", f"{name}.{k}", got[k], val, E.bound_of(n, ab))
    if CASES[name].get("masks") == "edges":
        assert bool((ref["through"][1][-1] == 0).all())                      # the row that keeps no review: no terms at all
        if c["word_mask"] is not None:
            assert bool((ref["fixed"][1][~c["word_mask"]] == 0).all())


def test_parse_cli_rules_for_contributions():
    from review_based_recommender_amd.recommend import parse_cli
    base = ["--model", "simple_siamese", "--config", "c.json", "--checkpoint", "m.pt"]
    a = parse_cli(base + ["--out", "o.jsonl", "--contributions", "3"])
    assert a.contributions == 3 and a.explain is None and a.attention is None
    assert parse_cli(base + ["--out", "o.jsonl"]).contributions is None
    for bad in (["--eval-split", "test", "--contributions", "3"],                  # --contributions without --out
                ["--out", "o.jsonl", "--contributions", "0"], ["--out", "o.jsonl", "--contributions", "-2"]):
        with pytest.raises(SystemExit):
            quiet(parse_cli, base + bad)
    for model in ("deepconn", "narre", "dual_att", "ahn"):
        with pytest.raises(SystemExit):
            quiet(parse_cli, ["--model", model, "--config", "c.json", "--checkpoint", "m.pt", "--out", "o", "--contributions", "2"])
    for flag in ("--explain", "--attention"):                                      # both keep refusing the model
        with pytest.raises(SystemExit):
            quiet(parse_cli, base + ["--out", "o", flag, "2"])


def test_siamese_saliency_is_declared_in_header_binding_and_library():
    import os
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int rbr_siamese_saliency(" in open(os.path.join(root, "include", "rbr_hip.h")).read()
    assert "rbr_siamese_saliency" in _lib.SIGNATURES and len(_lib.SIGNATURES["rbr_siamese_saliency"][1]) == 22
    L = _lib.lib()

    def call(n=2, R=3, T=4, V=10, E=8, F=8, K=2, ptr=1 << 20, Wt=None, **null):
        """Pointers are never dereferenced on the host: a refusal comes before any launch, and these calls are all refusals."""
        names = ("table", "ids", "word_mask", "rev_mask", "y", "a", "g", "Wt", "Wp", "bp", "wi", "fixed", "through", "reviews")
        ptrs = {k: ptr for k in names}
        ptrs.update(word_mask=None, rev_mask=None, Wt=Wt)
        ptrs.update(null)
        return L.rbr_siamese_saliency(n, R, T, V, E, F, K, *(ptrs[k] for k in names), None)

    # host-side refusals need no GPU; every one names its cause, and nothing is launched
    for k in ("table", "ids", "y", "a", "g", "Wp", "bp", "wi", "fixed", "through", "reviews"):
        assert call(**{k: None}) == -1 and b"null pointer" in L.rbr_last_error(), k
    assert call(ptr=None) == -1 and b"null pointer" in L.rbr_last_error()
    assert call(R=65) == -1 and b"R=65" in L.rbr_last_error()
    assert call(F=5) == -1 and b"Wt" in L.rbr_last_error()                   # F != E without the transform
    assert call(R=64, E=300, F=300) == -2 and b"LDS" in L.rbr_last_error()   # 2 * 64 * 300 floats alone are 150 KiB
    assert call(R=64, E=300, F=16, Wt=1 << 20) == -2 and b"LDS" in L.rbr_last_error()
    for bad in (dict(R=0), dict(T=0), dict(E=0), dict(K=0), dict(n=-1), dict(K=16385), dict(E=16388, F=16388), dict(F=16385)):
        assert call(**bad) == -1 and b"bad shape" in L.rbr_last_error(), bad
    assert call(n=0) == 0 and call(n=0, ptr=None) == 0                       # an empty batch is a no-op


def test_contributions_covers_simple_siamese_only():
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    from review_based_recommender_amd.recommend import Contributions, Recommender
    assert Contributions._fields == ("score", "user_tokens", "item_tokens", "user_tokens_fixed", "item_tokens_fixed", "user_text",
                                     "item_text", "user_review_weights", "user_reviews", "item_review_weights", "item_reviews")
    c = synth.DATT_CFGS["tiny"]
    datt = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    rec = Recommender(datt, user=torch.zeros(3, 16, dtype=torch.int64), item=torch.zeros(3, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="explain.*attention"):
        rec.contributions(torch.tensor([1]), torch.tensor([1]))
    c = synth.SIAMESE_CFGS["tiny"]
    siam = quiet(SimpleSiamese, c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.5, 0.2, 0.1, c["UB"], c["LT"])
    rec = Recommender(siam, user=torch.zeros(3, 2, 4, dtype=torch.int64), item=torch.zeros(3, 2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="B >= 1"):
        rec.contributions(torch.tensor([[1]]), torch.tensor([[1]]))
    with pytest.raises(RuntimeError, match="refresh"):                               # covered, but there are no tables yet
        rec.contributions(torch.tensor([1]), torch.tensor([1]))
    # the explanations of the other models keep refusing this one, in their own words
    with pytest.raises(ValueError, match="DeepCoNN\\+\\+ and NARRE"):
        rec.explain(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError, match="covers D-ATT"):
        rec.attention(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError, match="SimpleSiamese is not covered"):
        siam.explain_users()
