"""Seeded AHN configurations, parameters (the reference's state_dict keys and shapes) and batches for tests/golden/ahn_*.npz
(generator: make_golden_ahn.py).  The fixtures themselves carry the parameters and inputs; this module is how they were drawn."""
from collections import OrderedDict

import torch

# B examples, R reviews, S sentences per review, W words per sentence (both sides), E = H (the reference views the word rows with
# hidden_dim, ahn_model.py:58), K FM factors, U / I / V table sizes; seed: chosen so that every routing max of the float64
# reference leads its runner-up by the margin make_golden_ahn.py asserts
AHN_CFGS = {
    "tiny": dict(B=2, R=3, S=4, W=6, E=12, H=12, K=4, U=7, I=8, V=40, seed=0),
    "small": dict(B=3, R=4, S=4, W=8, E=20, H=20, K=6, U=9, I=10, V=60, seed=3),
}


def ahn_shapes(c):
    E, H, Hh, K = c["E"], c["H"], c["H"] // 2, c["K"]
    s = OrderedDict()
    s["word_embeddings.embedding.weight"] = (c["V"], E)
    for sfx in ("", "_reverse"):
        s[f"word_encoder._encoder.weight_ih_l0{sfx}"] = (4 * Hh, E)
        s[f"word_encoder._encoder.weight_hh_l0{sfx}"] = (4 * Hh, Hh)
        s[f"word_encoder._encoder.bias_ih_l0{sfx}"] = (4 * Hh,)
        s[f"word_encoder._encoder.bias_hh_l0{sfx}"] = (4 * Hh,)
    for agg in ("unbalanced_sentence_aggregator", "unbalanced_review_aggregator"):
        if agg == "unbalanced_review_aggregator":
            for side in ("user", "item"):
                s[f"{side}_review_trans_layer.0.weight"] = (H, H)
                s[f"{side}_review_trans_layer.0.bias"] = (H,)
        s[f"{agg}.item_aggregator.trans_layer.0.weight"] = (H, H)
        s[f"{agg}.item_aggregator.gate_layer.0.weight"] = (H, H)
        s[f"{agg}.item_aggregator.proj_layer.weight"] = (1, H)
        s[f"{agg}.bilinear.weight"] = (H, H)
    s["user_embeddings.embedding.weight"] = (c["U"], H)
    s["item_embeddigns.embedding.weight"] = (c["I"], H)
    s["fm.V"] = (4 * H, K)
    s["fm.lin.weight"] = (1, 4 * H)
    s["fm.lin.bias"] = (1,)
    return s


def ahn_params(c, seed=None):
    g = torch.Generator().manual_seed(1000 + (c["seed"] if seed is None else seed))
    sd = OrderedDict()
    for k, shape in ahn_shapes(c).items():
        scale = 0.6 if k.startswith("word_embeddings") else 0.2 if k.startswith("fm.") else 0.4
        sd[k] = torch.randn(*shape, generator=g) * scale
    sd["word_embeddings.embedding.weight"][0] = 0.0          # the padding row
    return sd


def ahn_batch(c, seed=None):
    """Inputs of AHN.forward plus ratings.  Edge cases: empty sentences, an empty review on each side (its mask is off), one-word
    sentences, sentences of full width on the item side only (the sides' longest sentences differ)."""
    g = torch.Generator().manual_seed(2000 + (c["seed"] if seed is None else seed))
    B, R, S, W = c["B"], c["R"], c["S"], c["W"]

    def side(longest):
        lens = torch.randint(0, longest + 1, (B, R, S), generator=g)
        lens[0, 0, 0], lens[0, 0, 1], lens[B - 1, 1, 0] = longest, 1, 0
        lens[B - 1, R - 1] = 0                               # an empty review
        lens[0, 1, S - 1] = 0                                # an empty sentence inside a live review
        lens[:, 0, 0] = torch.maximum(lens[:, 0, 0], torch.ones(B, dtype=torch.int64))      # every example keeps a live review
        ids = torch.randint(1, c["V"], (B, R, S, W), generator=g)
        ids = ids * (torch.arange(W).view(1, 1, 1, W) < lens.unsqueeze(-1))
        return ids, lens, lens > 0, (lens > 0).any(dim=2)

    u_ids_w, u_len, u_sm, u_rm = side(W - 2)
    i_ids_w, i_len, i_sm, i_rm = side(W)
    return OrderedDict(
        user_reviews=u_ids_w, item_reviews=i_ids_w, user_sent_masks=u_sm, item_sent_masks=i_sm, user_sent_lengths=u_len,
        item_sent_lenghts=i_len, user_review_masks=u_rm, item_review_masks=i_rm,
        user_ids=torch.randint(1, c["U"], (B,), generator=g), item_ids=torch.randint(1, c["I"], (B,), generator=g),
        ratings=torch.randint(1, 6, (B,), generator=g).float())


FORWARD_KEYS = ("user_reviews", "item_reviews", "user_sent_masks", "item_sent_masks", "user_sent_lengths", "item_sent_lenghts",
                "user_review_masks", "item_review_masks", "user_ids", "item_ids")
