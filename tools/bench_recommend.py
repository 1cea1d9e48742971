"""Catalogue encode and fused top-K (csrc/pair_score.hip) against the torch composition a user without it would write, as one
JSON line.

    timeout -k 10 900 python tools/bench_recommend.py [--repeats 5] [--iters 20] [--warmup 3] [--limit 840] [--only topk]

  S1  U = I = 1001, K = 32, k = 10: DeepCoNN++ cfg2 (tests/golden/synth.py parameters, synth-style Zipf documents keyed by id);
      encode_ms = Recommender.refresh() over both sides, then topk for all users against the encoded tables
  S2  Nu = 4096 user rows x Ni = 100 003 items, K = 32, k = 10, random latent tables (no model has such a catalogue here)
Per shape: fused_ms (functional.pair_score_topk, item_lo = 1), torch_ms -- chunked relu(ul[:, None] * il[None]) @ h + biases
followed by torch.topk, the chunk sized to ~1 GiB of [chunk, Ni, K] intermediates -- and their ratio, both timed in this run with
device events: medians over --repeats blocks of --iters calls after --warmup calls.  same_items says whether both paths chose
the same items (their scores differ in the last bits: the composition sums in another order, so near-ties may swap).
valu_floor_ms is 3 lane-operations per (pair, k) at 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz (39.3 T unpacked lane-ops/s, the
157.3 TF vector peak); fused_floor_fraction = valu_floor_ms / fused_ms (the merge launch included in fused_ms).
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above.  Kernel times of their own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_recommend.py --only topk --repeats 1 --iters 5
"""
from __future__ import annotations

import json

import numpy as np
import torch

from benchlib import arm, parser, quiet, timed_ms

import synth  # noqa: E402  (benchlib set the path)

LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9        # 39.3e12 unpacked fp32 lane-operations per second (an fma counts 2 FLOP and is issued
                                             # for 64 lanes over 4 cycles on a 16-lane pipe: 157.3 TFLOP/s)


def torch_topk(ul, il, h, g, ub, ib, k, item_lo, budget_bytes=1 << 30):
    """What a user of the package without pair_score_topk writes: scores in chunks of user rows, then torch.topk."""
    Nu, K = ul.shape
    Ni = il.shape[0]
    chunk = max(1, min(Nu, budget_bytes // (Ni * K * 4)))
    items, scores = [], []
    for a in range(0, Nu, chunk):
        s = torch.relu(ul[a:a + chunk, None, :] * il[None, :, :]) @ h.view(-1) + ub[a:a + chunk].view(-1, 1) + ib.view(1, -1) + g
        s[:, :item_lo] = float("-inf")
        v, i = torch.topk(s, k, dim=1)
        items.append(i)
        scores.append(v)
    return torch.cat(items), torch.cat(scores)


def bench_shape(name, ul, il, h, g, ub, ib, k, a):
    from review_based_recommender_amd import _lib, functional as RF
    Nu, K = ul.shape
    Ni = il.shape[0]
    fused = lambda: RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1)      # noqa: E731
    torch_ = lambda: torch_topk(ul, il, h, g, ub, ib, k, 1)                             # noqa: E731
    fi, fs = fused()
    ti, ts = torch_()
    torch.cuda.synchronize()
    f_ms = timed_ms(fused, a.iters, a.warmup, a.repeats)
    t_ms = timed_ms(torch_, max(1, a.iters // 4), 1, a.repeats)
    floor_ms = 3.0 * Nu * (Ni - 1) * K / LANE_OPS_PER_S * 1e3
    return {
        f"{name}_shape": {"Nu": Nu, "Ni": Ni, "K": K, "k": k},
        f"{name}_fused_ms": round(f_ms[0], 4), f"{name}_fused_ms_min_max": [round(f_ms[1], 4), round(f_ms[2], 4)],
        f"{name}_torch_ms": round(t_ms[0], 4), f"{name}_torch_ms_min_max": [round(t_ms[1], 4), round(t_ms[2], 4)],
        f"{name}_torch_over_fused": round(t_ms[0] / f_ms[0], 2),
        f"{name}_same_items": float((fi == ti).float().mean()),
        f"{name}_max_score_diff": float((fs - ts).abs().max()),
        f"{name}_valu_floor_ms": round(floor_ms, 4),
        f"{name}_fused_floor_fraction": round(floor_ms / f_ms[0], 4),
        f"{name}_ws_bytes": int(_lib.lib().rbr_pair_score_topk_ws_bytes(Nu, Ni, K, k)),
    }


def s1_tables(a, res):
    """DeepCoNN++ cfg2 over a synthetic catalogue of 1001 users / 1001 items: the latent tables of a real model."""
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    from review_based_recommender_amd.recommend import Recommender
    cfg = synth.DEEPCONN_CFGS["cfg2"]
    m = quiet(DeepCoNNpp, cfg["U"], cfg["I"], cfg["V"], cfg["kz"], cfg["D"], cfg["H"], cfg["K"], cfg["L"], None, 0.5)
    m.load_state_dict(synth.deepconn_params(cfg, 0))
    m.validate_ids = False
    m.to("cuda:0").eval()
    rng = np.random.default_rng(5)
    docs = [torch.from_numpy(synth._docs(rng, n, cfg["L"], cfg["V"])).to(torch.int32) for n in (cfg["U"], cfg["I"])]
    for d in docs:
        d[0] = 0                                            # id 0: the all-pad document
    rec = Recommender(m, user=docs[0].to("cuda:0"), item=docs[1].to("cuda:0"))
    if a.only != "topk":
        e_ms = timed_ms(lambda: rec.refresh(chunk=256), 1, 1, a.repeats)
        res["S1_encode_ms"] = round(e_ms[0], 3)
        res["S1_encode_ms_min_max"] = [round(e_ms[1], 3), round(e_ms[2], 3)]
        res["S1_encode_docs"] = cfg["U"] + cfg["I"]
    else:
        rec.refresh(chunk=256)
    _, h, g, ub, ib = m.score_mode_and_params()
    return rec.user_latents, rec.item_latents, h.detach(), g.detach(), ub.detach(), ib.detach()


def main():
    ap = parser(__doc__, repeats=5, iters=20, warmup=3, limit=840)
    ap.add_argument("--only", choices=["all", "topk"], default="all", help="topk: skip the encode timing (profiler runs)")
    a = ap.parse_args()
    arm("bench_recommend.py", a.limit)
    res = {"bench": "recommend", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters}
    res.update(bench_shape("S1", *s1_tables(a, res), 10, a))
    gen = torch.Generator().manual_seed(0)
    Nu, Ni, K = 4096, 100003, 32
    tabs = [torch.randn(Nu, K, generator=gen), torch.randn(Ni, K, generator=gen), torch.randn(K, 1, generator=gen),
            torch.randn(1, generator=gen), torch.randn(Nu, 1, generator=gen), torch.randn(Ni, 1, generator=gen)]
    res.update(bench_shape("S2", *[t.to("cuda:0") for t in tabs], 10, a))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
