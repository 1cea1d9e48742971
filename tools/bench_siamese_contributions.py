"""Recommender.contributions and its op (csrc/siamese_saliency.hip) against the torch composition a user could write without it,
as one JSON line.

    timeout -k 10 600 python tools/bench_siamese_contributions.py [--repeats 5] [--iters 20] [--warmup 3] [--limit 540]

SimpleSiamese at the `toys` shape (tests/golden/synth.py parameters, Zipf reviews keyed by id, 1001 users / items): 256 pairs, 11
reviews of 50 tokens per side, E = 108, no latent transform.  Device events, medians over --repeats blocks of --iters calls after
--warmup calls:
  contributions_ms   one Recommender.contributions(u_ids, i_ids) call (both towers: the review bag, the attention, one linear,
                     the op, a few elementwise ops and row gathers)
  op_ms              functional.siamese_saliency alone on the user side's reviews (y / a / g precomputed): one launch
  composed_ms        the same numbers through torch autograd on the same GPU, reviews and d_latent: rows [n, R, T, E]
                     materialised with requires_grad, masked mean, the attention, LastFeat's W, backward, (x.grad * x).sum(-1)
  max_abs_diff       largest difference between the op's fixed + through and the composition's (and the largest |value|)
What the op has to move, from the shapes, and the floor that sets:
  gather_mb          the token rows the op reads, one per position: n * R * T * E * 4 bytes
  floor_us           gather_mb at 8.6 TB/s, the measured rate of uniformly random rows of a table the Infinity Cache holds (the
                     21.6 MB word table fits it); op_over_floor = op_ms over that
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import numpy as np
import torch

from benchlib import arm, parser, quiet, timed_ms

import synth  # noqa: E402  (benchlib set the path)

DEV = "cuda:0"
N_IDS, PAIRS = 1001, 256
GATHER_TBPS = 8.6          # random rows out of the Infinity Cache, chip-wide


def recommender():
    """SimpleSiamese `toys` on synthetic per-id reviews, its refreshed Recommender and 256 pairs."""
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    from review_based_recommender_amd.recommend import Recommender
    rng = np.random.default_rng(5)
    c = synth.SIAMESE_CFGS["toys"]
    m = quiet(SimpleSiamese, c["D"], c["K"], c["V"], N_IDS, N_IDS, None, False, 0.5, 0.2, 0.1, c["UB"], c["LT"])
    m.load_state_dict(synth.siamese_params(dict(c, U=N_IDS, I=N_IDS), 0))
    sides = []
    for _ in range(2):
        revs = synth._docs(rng, N_IDS * c["R"], c["T"], c["V"]).reshape(N_IDS, c["R"], c["T"])
        dead = np.arange(c["R"])[None, :] >= rng.integers(1, c["R"] + 1, size=N_IDS)[:, None]      # trailing reviews: all pad
        revs[dead] = 0
        revs[0] = 0                                         # id 0: the padding id has no text
        sides.append(torch.from_numpy(revs))
    m.validate_ids = False
    m.to(DEV).eval()
    rec = Recommender(m, user=sides[0].to(DEV), item=sides[1].to(DEV)).refresh(chunk=256)
    u_ids = torch.from_numpy(rng.integers(1, N_IDS, size=PAIRS)).to(DEV)
    i_ids = torch.from_numpy(rng.integers(1, N_IDS, size=PAIRS)).to(DEV)
    return m, rec, u_ids, i_ids, c


def composed_tokens(m, revs, d_latent):
    """The user tower's tokens by torch autograd over materialised rows (eval semantics: no dropout)."""
    wm = revs != 0
    rm = wm.any(-1)
    x = (m.word_embedding.weight.detach()[revs] * wm.unsqueeze(-1)).requires_grad_(True)          # [n, R, T, E]
    y = x.sum(2) / (wm.sum(-1, keepdim=True) + 1e-8)
    if m.latent_transform:
        lin = m.latent_transform_layer[0]
        y = torch.tanh(torch.nn.functional.linear(y, lin.weight.detach(), lin.bias.detach()))
    att = m.review_att_layer
    t = torch.tanh(torch.nn.functional.linear(y, att.proj_layer[0].weight.detach(), att.proj_layer[0].bias.detach()))
    logit = (t @ att.inner_product.weight.detach().view(-1)).masked_fill(~rm, -1e8)
    pooled = (torch.softmax(logit, dim=1).unsqueeze(-1) * y).sum(1)
    ((pooled @ m.user_last_feat_layer.W.detach()) * d_latent).sum().backward()
    return (x.grad * x.detach()).sum(-1)


def main():
    ap = parser(__doc__, repeats=5, iters=20, warmup=3, limit=540)
    a = ap.parse_args()
    arm("bench_siamese_contributions.py", a.limit)
    from review_based_recommender_amd import functional as RF
    m, rec, u_ids, i_ids, c = recommender()
    co = rec.contributions(u_ids, i_ids)
    torch.cuda.synchronize()
    c_ms = timed_ms(lambda: rec.contributions(u_ids, i_ids), a.iters, a.warmup, a.repeats)
    # the user side's problem, with the gradient contributions() puts on its pooled feature
    table = m.word_embedding.weight.detach()
    revs = rec.cache.user.index_select(0, u_ids).contiguous()
    n, R, T = revs.shape
    wm = revs != 0
    rm = wm.any(-1)
    zu, zi = rec.user_latents[u_ids], rec.item_latents[i_ids]
    d_latent = (m.fm.h.detach().view(1, -1) * (zu * zi > 0) * zi).contiguous()
    att = m.review_att_layer
    Wp, bp, wi = att.proj_layer[0].weight.detach(), att.proj_layer[0].bias.detach(), att.inner_product.weight.detach()
    Wt = None
    with torch.no_grad():
        y = RF.review_bag(table, revs.reshape(n * R, T), wm.reshape(n * R, T))
        if m.latent_transform:
            lin = m.latent_transform_layer[0]
            y, Wt = RF.linear(y, lin.weight.detach(), lin.bias.detach(), tanh=True), lin.weight.detach()
        y = y.view(n, R, -1)
        _, s = att(y, rm)
        g = RF.linear(d_latent, m.user_last_feat_layer.W.detach())
    s = s.view(n, R).contiguous()
    op = lambda: RF.siamese_saliency(table, revs, wm, rm, y, s, g, Wt, Wp, bp, wi)          # noqa: E731
    composed = lambda: composed_tokens(m, revs, d_latent)                                   # noqa: E731
    o, t_out = op(), composed()
    torch.cuda.synchronize()
    o_ms = timed_ms(op, a.iters, a.warmup, a.repeats)
    t_ms = timed_ms(composed, max(1, a.iters // 4), 1, a.repeats)
    E = c["D"]
    gather_b = 4.0 * E * n * R * T
    floor_us = gather_b / (GATHER_TBPS * 1e12) * 1e6
    tokens = o.fixed + o.through
    res = {
        "bench": "siamese_contributions", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
        "shape": {"pairs": PAIRS, "R": R, "T": T, "E": E, "K": c["K"], "latent_transform": bool(c["LT"]), "ids_per_side": N_IDS},
        "contributions_ms": round(c_ms[0], 4), "contributions_ms_min_max": [round(c_ms[1], 4), round(c_ms[2], 4)],
        "op_ms": round(o_ms[0], 4), "op_ms_min_max": [round(o_ms[1], 4), round(o_ms[2], 4)],
        "composed_ms": round(t_ms[0], 4), "composed_ms_min_max": [round(t_ms[1], 4), round(t_ms[2], 4)],
        "composed_over_op": round(t_ms[0] / o_ms[0], 2), "composed_over_contributions_side": round(t_ms[0] / (c_ms[0] / 2), 2),
        "op_vs_contributions_max_abs_diff": float((tokens - co.user_tokens).abs().max()),
        "max_abs_diff": float((tokens - t_out).abs().max()), "max_abs_value": float(tokens.abs().max()),
        "through_share": round(float(o.through.abs().sum() / tokens.abs().sum()), 4),
        "gather_mb": round(gather_b / 1e6, 2), "floor_us": round(floor_us, 2), "op_over_floor": round(o_ms[0] * 1e3 / floor_us, 1),
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
