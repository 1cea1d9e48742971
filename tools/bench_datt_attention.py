"""Recommender.attention and its op (csrc/datt_saliency.hip) against the torch composition a user could write without it, as one
JSON line.

    timeout -k 10 600 python tools/bench_datt_attention.py [--repeats 5] [--iters 20] [--warmup 3] [--limit 540]

D-ATT cfg4 (tests/golden/synth.py parameters, Zipf documents keyed by id, 1001 users / items): 256 pairs, a 1024-token document
per side, E = 100.  Device events, medians over --repeats blocks of --iters calls after --warmup calls:
  attention_ms    one Recommender.attention(u_ids, i_ids) call (both towers: both gates, the merged conv with argmax, three
                  linears, the op, a few elementwise ops)
  op_ms           functional.datt_saliency alone on the user side's documents (gates / feat / argmax / d_feat precomputed):
                  both launches
  composed_ms     the same numbers through torch autograd on the same GPU, documents and d_latent: rows materialised with
                  requires_grad, F.conv1d gates and convs, max_pool1d, the fc, backward, (x.grad * x).sum(-1)
  max_abs_diff    largest difference between attention's user_tokens and the composition's (and the largest |value|, for scale)
What the op has to move and compute, from the shapes (code below), and the floor that sets:
  launch1_mflop   2 * E * taps of the channels with a gradient (the dot products of launch 1's first phase)
  launch2_mflop   2 * E * (win + 1) per position
  gather_mb       the embedded rows launch 2 reads, one per position (E floats each; launch 1 reads one row per tap besides)
  floor_us        gather_mb at 8.6 TB/s, the measured rate of random rows served by the Infinity Cache (the 20 MB word table
                  fits it); op_over_floor = op_ms over that
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import numpy as np
import torch
import torch.nn.functional as F

from benchlib import arm, parser, quiet, timed_ms

import synth  # noqa: E402  (benchlib set the path)

DEV = "cuda:0"
N_IDS, PAIRS = 1001, 256
GATHER_TBPS = 8.6          # random rows out of the Infinity Cache, chip-wide


def recommender():
    """D-ATT cfg4 on synthetic per-id documents, its refreshed Recommender and 256 pairs."""
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    from review_based_recommender_amd.recommend import Recommender
    rng = np.random.default_rng(5)
    c = synth.DATT_CFGS["cfg4"]
    m = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    m.load_state_dict(synth.datt_params(c, 0))
    docs = [torch.from_numpy(synth._docs(rng, N_IDS, c["L"], c["V"])) for _ in range(2)]
    for d in docs:
        d[0] = 0                                            # id 0: the padding id has no text
    m.validate_ids = False
    m.to(DEV).eval()
    rec = Recommender(m, user=docs[0].to(DEV), item=docs[1].to(DEV)).refresh(chunk=256)
    u_ids = torch.from_numpy(rng.integers(1, N_IDS, size=PAIRS)).to(DEV)
    i_ids = torch.from_numpy(rng.integers(1, N_IDS, size=PAIRS)).to(DEV)
    return m, rec, u_ids, i_ids, c


def composed_tokens(m, docs, d_latent):
    """The user tower's tokens by torch autograd over materialised rows (eval semantics: no dropout)."""
    lo, gl = m.u_local_atten, m.u_global_atten
    x = m.word_embeddings.weight.detach()[docs].requires_grad_(True)                 # [n, L, E]
    xt = x.transpose(1, 2)
    gate_l = torch.sigmoid(F.conv1d(xt, lo.attn[0].weight.detach(), lo.attn[0].bias.detach(), padding=lo.padding_size))
    gate_g = torch.sigmoid(F.conv1d(xt, gl.attn[0].weight.detach(), gl.attn[0].bias.detach()))
    feats = []
    for conv, gate in ((lo.conv[0], gate_l), (gl.conv1[0], gate_g), (gl.conv2[0], gate_g), (gl.conv3[0], gate_g)):
        y = torch.tanh(F.conv1d(xt * gate, conv.weight.detach(), conv.bias.detach()))
        feats.append(F.max_pool1d(y, y.shape[-1]).squeeze(-1))
    hid = F.relu(F.linear(torch.cat(feats, 1), m.fc[0].weight.detach(), m.fc[0].bias.detach()))
    lat = F.linear(hid, m.fc[3].weight.detach(), m.fc[3].bias.detach())
    (lat * d_latent).sum().backward()
    return (x.grad * x.detach()).sum(-1)


def main():
    ap = parser(__doc__, repeats=5, iters=20, warmup=3, limit=540)
    a = ap.parse_args()
    arm("bench_datt_attention.py", a.limit)
    from review_based_recommender_amd import functional as RF
    m, rec, u_ids, i_ids, c = recommender()
    at = rec.attention(u_ids, i_ids)
    torch.cuda.synchronize()
    a_ms = timed_ms(lambda: rec.attention(u_ids, i_ids), a.iters, a.warmup, a.repeats)
    # the user side's problem, with the gradient attention() puts on its pooled features
    lo, gl = m.u_local_atten, m.u_global_atten
    table = m.word_embeddings.weight.detach()
    docs = rec.cache.user.index_select(0, u_ids).contiguous()
    d_latent = rec.item_latents[i_ids].contiguous()
    convs = [lo.conv[0], gl.conv1[0], gl.conv2[0], gl.conv3[0]]
    ws, bs = [cv.weight.detach() for cv in convs], [cv.bias.detach() for cv in convs]
    aw = (lo.attn[0].weight.detach(), gl.attn[0].weight.detach())
    with torch.no_grad():
        gate_l = RF.datt_gate(table, aw[0], lo.attn[0].bias.detach(), docs, is_global=False)
        gate_g = RF.datt_gate(table, aw[1], gl.attn[0].bias.detach(), docs, is_global=True)
        feat, argmax = RF.textcnn(table, docs, None, ws, bs, gate=(gate_l, gate_g), gate_split=1, pad_mode=RF.PAD_VALID,
                                  act=RF.ACT_TANH, padding_idx=0, return_argmax=True)
        hid = RF.linear(feat, m.fc[0].weight.detach(), m.fc[0].bias.detach(), relu=True)
        d_feat = RF.linear(RF.linear(d_latent, m.fc[3].weight.detach().t().contiguous()) * (hid > 0),
                           m.fc[0].weight.detach().t().contiguous()).contiguous()
    gates = torch.stack([gate_l, gate_g])
    op = lambda: RF.datt_saliency(table, docs, gates, ws, feat, argmax, d_feat, aw)         # noqa: E731
    composed = lambda: composed_tokens(m, docs, d_latent)                                   # noqa: E731
    o, c_out = op(), composed()
    torch.cuda.synchronize()
    o_ms = timed_ms(op, a.iters, a.warmup, a.repeats)
    c_ms = timed_ms(composed, max(1, a.iters // 4), 1, a.repeats)
    # counts from the shapes: taps of launch 1 (channels with a gradient; every tap of a 'valid' window is in range)
    E, L, win = c["E"], c["L"], c["win"]
    live = ((d_feat != 0) & (feat.abs() < 1)).cpu()
    taps, c0 = 0, 0
    for w in ws:
        taps += int(live[:, c0:c0 + w.shape[0]].sum()) * w.shape[2]
        c0 += w.shape[0]
    flop1, flop2 = 2.0 * E * taps, 2.0 * E * (win + 1) * PAIRS * L
    gather_b = 4.0 * E * PAIRS * L
    floor_us = gather_b / (GATHER_TBPS * 1e12) * 1e6
    res = {
        "bench": "datt_attention", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
        "shape": {"pairs": PAIRS, "L": L, "E": E, "win": win, "l_out": c["l_out"], "g_out": c["g_out"], "ids_per_side": N_IDS},
        "attention_ms": round(a_ms[0], 4), "attention_ms_min_max": [round(a_ms[1], 4), round(a_ms[2], 4)],
        "op_ms": round(o_ms[0], 4), "op_ms_min_max": [round(o_ms[1], 4), round(o_ms[2], 4)],
        "composed_ms": round(c_ms[0], 4), "composed_ms_min_max": [round(c_ms[1], 4), round(c_ms[2], 4)],
        "composed_over_op": round(c_ms[0] / o_ms[0], 2), "composed_over_attention_side": round(c_ms[0] / (a_ms[0] / 2), 2),
        "op_vs_attention_max_abs_diff": float((o.fixed + o.through - at.user_tokens).abs().max()),
        "max_abs_diff": float((at.user_tokens - c_out).abs().max()), "max_abs_value": float(at.user_tokens.abs().max()),
        "through_share": round(float(o.through.abs().sum() / (o.fixed + o.through).abs().sum()), 4),
        "launch1_taps": taps, "launch1_mflop": round(flop1 / 1e6, 3), "launch2_mflop": round(flop2 / 1e6, 3),
        "gather_mb": round(gather_b / 1e6, 2), "floor_us": round(floor_us, 2), "op_over_floor": round(o_ms[0] * 1e3 / floor_us, 1),
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
