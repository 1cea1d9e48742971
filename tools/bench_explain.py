"""Recommender.explain and its kernel (csrc/textcnn_saliency.hip) against the composition the package offered before it, as one
JSON line.

    timeout -k 10 600 python tools/bench_explain.py [--repeats 5] [--iters 20] [--warmup 3] [--limit 540]

  cfg2   DeepCoNN++ cfg2 (tests/golden/synth.py parameters, Zipf documents keyed by id, 1001 users / items): 256 pairs, a
         512-token document per side
  cfg3   NARRE cfg3: 256 pairs, 10 reviews of 50 tokens per side
Per shape, device events, medians over --repeats blocks of --iters calls after --warmup calls:
  explain_ms      one Recommender.explain(u_ids, i_ids) call (both towers: forward with argmax, linear, the kernel, a few
                  elementwise ops; NARRE also its attention pool)
  kernel_ms       functional.textcnn_saliency alone on the user side's documents (feat / argmax / d_feat precomputed)
  composed_ms     the same numbers through autograd, on the same documents and d_feat: rows materialised with
                  functional.embedding, NgramFeat.forward on them, backward from d_feat, (x.grad * x).sum(-1)
  max_abs_diff    largest difference between the two results (and the largest |value|, for scale)
  phase1_mflop    2 * D * sum(ch * kz) per document the kernel actually computes (channels with a gradient, unmasked in-range
                  taps) -- the dot products of its first phase -- and phase1_gflops = that over kernel_ms
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import numpy as np
import torch

from benchlib import arm, parser, quiet, timed_ms

import synth  # noqa: E402  (benchlib set the path)

DEV = "cuda:0"


def recommender(kind):
    """A model of the shape on synthetic per-id text, its refreshed Recommender and 256 pairs."""
    from review_based_recommender_amd.recommend import Recommender
    rng = np.random.default_rng(5)
    if kind == "cfg2":
        from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
        c = synth.DEEPCONN_CFGS["cfg2"]
        m = quiet(DeepCoNNpp, c["U"], c["I"], c["V"], c["kz"], c["D"], c["H"], c["K"], c["L"], None, 0.5)
        m.load_state_dict(synth.deepconn_params(c, 0))
        docs = [torch.from_numpy(synth._docs(rng, n, c["L"], c["V"])) for n in (c["U"], c["I"])]
        extra = {}
    else:
        from review_based_recommender_amd.models.narre.narre import NARRE
        c = synth.NARRE_CFGS["cfg3"]
        m = quiet(NARRE, c["U"], c["I"], c["V"], c["kz"], c["H"], c["D"], c["A"], c["K"], c["R"], c["T"], 0.5, 0, 0, 0, None, "CNN")
        m.load_state_dict(synth.narre_params(c, 0))
        docs = [torch.from_numpy(synth._docs(rng, n * c["R"], c["T"], c["V"])).view(n, c["R"], c["T"]) for n in (c["U"], c["I"])]
        rids = [torch.from_numpy(rng.integers(1, n, size=(k, c["R"])).astype(np.int64)) for k, n in ((c["U"], c["I"]), (c["I"], c["U"]))]
        for r in rids:
            r[0] = 0
        extra = dict(user_rids=rids[0].to(DEV), item_rids=rids[1].to(DEV))
    for d in docs:
        d[0] = 0                                            # id 0: the padding id has no text
    m.validate_ids = False
    m.to(DEV).eval()
    rec = Recommender(m, user=docs[0].to(DEV), item=docs[1].to(DEV), **extra).refresh(chunk=256)
    u_ids = torch.from_numpy(rng.integers(1, c["U"], size=256)).to(DEV)
    i_ids = torch.from_numpy(rng.integers(1, c["I"], size=256)).to(DEV)
    return m, rec, u_ids, i_ids, c


def bench_shape(kind, a):
    from review_based_recommender_amd import functional as RF
    m, rec, u_ids, i_ids, c = recommender(kind)
    ex = rec.explain(u_ids, i_ids)
    torch.cuda.synchronize()
    e_ms = timed_ms(lambda: rec.explain(u_ids, i_ids), a.iters, a.warmup, a.repeats)
    # the user side's conv problem, with the gradient explain() puts on its pooled features
    conv, table = m.ngram.feature_layer[0], m.word_embeddings.weight.detach()
    docs = rec.cache.user.index_select(0, u_ids)
    flat = docs.reshape(-1, docs.shape[-1]).contiguous()
    mask = flat != 0
    ws = [w.detach() for w in conv.weights()]
    with torch.no_grad():
        feat, argmax = RF.textcnn(table, flat, mask, ws, [b.detach() for b in conv.biases()], padding_idx=0, return_argmax=True)
        zu, zi = rec.user_latents[u_ids], rec.item_latents[i_ids]
        g = RF.linear(m.fm.h.detach().view(1, -1) * (zu * zi > 0) * zi, m.user_feat.W.detach())
        if kind == "cfg3":
            g = (ex.user_review_weights.unsqueeze(-1) * g.unsqueeze(1)).reshape(flat.shape[0], -1)
    g = g.contiguous()
    kernel = lambda: RF.textcnn_saliency(table, flat, mask, ws, feat, argmax, g)           # noqa: E731

    def composed():
        x = RF.embedding(table, flat, None).detach().requires_grad_(True)                   # [n_docs, L, D] rows
        out = m.ngram(x, mask).squeeze(-1)
        out.backward(g)
        return (x.grad * x.detach()).sum(-1)

    k_out, c_out = kernel(), composed()
    torch.cuda.synchronize()
    k_ms = timed_ms(kernel, a.iters, a.warmup, a.repeats)
    c_ms = timed_ms(composed, max(1, a.iters // 4), 1, a.repeats)
    # dot products of the kernel's first phase: live channels x taps that land on an unmasked token of the document
    D, L = table.shape[1], flat.shape[1]
    live = ((feat > 0) & (g != 0)).cpu()
    taps, c0 = 0, 0
    am, mk = argmax.cpu().long(), mask.cpu()
    for w in ws:
        ch, kz = w.shape[0], w.shape[2]
        for j in range(kz):
            t = am[:, c0:c0 + ch] + j - (kz - 1) // 2
            ok = (t >= 0) & (t < L) & mk.gather(1, t.clamp(0, L - 1)) & live[:, c0:c0 + ch]
            taps += int(ok.sum())
        c0 += ch
    flop = 2.0 * D * taps
    return {
        f"{kind}_shape": {"pairs": 256, "docs_per_side": int(flat.shape[0]), "L": L, "D": D, "kz": list(c["kz"]), "H": c["H"]},
        f"{kind}_explain_ms": round(e_ms[0], 4), f"{kind}_explain_ms_min_max": [round(e_ms[1], 4), round(e_ms[2], 4)],
        f"{kind}_kernel_ms": round(k_ms[0], 4), f"{kind}_kernel_ms_min_max": [round(k_ms[1], 4), round(k_ms[2], 4)],
        f"{kind}_composed_ms": round(c_ms[0], 4), f"{kind}_composed_ms_min_max": [round(c_ms[1], 4), round(c_ms[2], 4)],
        f"{kind}_composed_over_kernel": round(c_ms[0] / k_ms[0], 2),
        f"{kind}_max_abs_diff": float((k_out - c_out).abs().max()), f"{kind}_max_abs_value": float(k_out.abs().max()),
        f"{kind}_phase1_taps": taps, f"{kind}_phase1_mflop": round(flop / 1e6, 3),
        f"{kind}_phase1_gflops": round(flop / (k_ms[0] * 1e-3) / 1e9, 1),
    }


def main():
    ap = parser(__doc__, repeats=5, iters=20, warmup=3, limit=540)
    a = ap.parse_args()
    arm("bench_explain.py", a.limit)
    res = {"bench": "explain", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters}
    for kind in ("cfg2", "cfg3"):
        res.update(bench_shape(kind, a))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
