"""Review sampling inside the id-fed gather against the plain id-fed gather, as one JSON line: NARRE at the cfg3 shape and
SimpleSiamese at the `toys` shape, on the split of tools/bench_review_feed.py made deeper (40 interactions per user on average, so
that a pool of 32 reviews is mostly full).

    python tools/bench_review_sample.py [--steps 200] [--warmup 20] [--repeats 5]

Four id feeds over the same meta: `plain` (rbr_review_gather, leave-one-out); `sample_pR_all` (rbr_review_sample_gather, pool P =
R, n = R kept: the plain batch's reviews in random order, so the same encoder work as `plain`); `sample_pR` (P = R) and
`sample_p32` (P = 32), which keep n = R // 2 reviews per side.  All in one run, per model:
  gather_us      the feed's launch alone at the step's shape: 20 gathers recorded into one hipGraph, per gather; the timed blocks
                 of the feeds alternate, gather_us_min_max is the spread of the blocks
  step_ms        replay of the recorded id-fed step (gather + step; 4 resident slots, rotated; dropout 0.5, HipClipAdam,
                 validate_ids = False, as the trainer runs it), the same pairs on every feed, blocks alternating; step_ms_min_max
  launches       kernel nodes of the recorded steps (kernel_launches(), keep_graph=True)
  bytes_read     table bytes one launch asks for: plain 2B * (R * T + R) * 4; sampler 2B * ((P + 1) * (T + 1) + n * T) * 4 -- the
                 liveness pass over the row's P + 1 reviews, the rids, and the kept reviews a second time (cache hits)
  bytes_written  2B * (R * T * 9 + ...) -- the same for all feeds: the outputs keep R slots
Medians over --repeats timed blocks of --steps steps."""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_review_dataset  # noqa: E402
import synth  # noqa: E402
from bench_review_feed import DEV, GATHERS_PER_GRAPH, SLOTS, alternating_ms, build_model  # noqa: E402

POOL = 32
PER_USER = 40


def bench_model(kind, c, a):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    B, R, T = c["B"], c["R"], c["T"]
    n = max(R // 2, 1)
    meta, train, _ = make_review_dataset.random_split(c["U"], c["I"], c["V"], R, T, PER_USER * c["U"], B, seed=0)
    ds = types.SimpleNamespace(**meta)
    pool = max(POOL, R)
    narrow, wide = D.DeviceReviewCache(ds, DEV), D.DeviceReviewCache(ds, DEV, pool=pool)
    feeds = {"plain": narrow.feed(kind, True), "sample_pR_all": narrow.sampled_feed(kind, R, R, seed=0),
             "sample_pR": narrow.sampled_feed(kind, n, n, seed=0), f"sample_p{pool}": wide.sampled_feed(kind, n, n, seed=0)}
    pools = {"plain": (None, R), "sample_pR_all": (R, R), "sample_pR": (R, n), f"sample_p{pool}": (pool, n)}
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(SLOTS):
        ex = [train[int(k)] for k in rng.choice(len(train), size=B, replace=False)]
        batches.append((torch.tensor([e[0] for e in ex]), torch.tensor([e[1] for e in ex]),
                        torch.tensor([e[2] for e in ex], dtype=torch.float32)))
    live = (wide.user_pool_table[:, :pool] != 0).any(-1).sum(1).float()
    res = {"B": B, "R": R, "T": T, "kept_per_side": n, "pool": pool,
           "mean_live_reviews_per_user_in_pool": round(float(live[1:].mean()), 2)}

    sts = {}
    for k, feed in feeds.items():
        m = build_model(kind, c)
        u, i, r = [t.to(DEV) for t in batches[0]]
        sts[k] = GraphedTrainStep.from_ids(m, make_optimizer(m, capturable=True, hip_clip_adam=True), feed, u, i, r, slots=SLOTS,
                                           keep_graph=True)
        for s in range(SLOTS):
            sts[k].stage(s, tuple(batches[s][:-1]), batches[s][-1])
    res["launches"] = {k: st.kernel_launches() for k, st in sts.items()}
    timed = alternating_ms({k: (lambda j, st=st: st(slot=j % SLOTS)) for k, st in sts.items()}, a.steps, a.warmup, a.repeats)
    res["step_ms"] = {k: round(v[0], 4) for k, v in timed.items()}
    res["step_ms_min_max"] = {k: [round(v[1], 4), round(v[2], 4)] for k, v in timed.items()}

    # each feed's launch alone, at the step's shape, into its own step's input views
    graphs = {}
    for k, feed in feeds.items():
        st = sts[k]
        (u, i), _, _ = st.slot_inputs(0)
        views = st.slot_batch(0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            feed.gather(u, i, out=views)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GATHERS_PER_GRAPH):
                feed.gather(u, i, out=views)
        graphs[k] = g
    timed = alternating_ms({k: (lambda j, g=g: g.replay()) for k, g in graphs.items()}, a.steps, a.warmup, a.repeats)
    res["gather_us"] = {k: round(v[0] * 1e3 / GATHERS_PER_GRAPH, 3) for k, v in timed.items()}
    res["gather_us_min_max"] = {k: [round(v[1] * 1e3 / GATHERS_PER_GRAPH, 3), round(v[2] * 1e3 / GATHERS_PER_GRAPH, 3)]
                                for k, v in timed.items()}
    res["bytes_read"] = {k: 2 * B * ((R * T + R) * 4 if p is None else ((p + 1) * (T + 1) + kept * T) * 4)
                         for k, (p, kept) in pools.items()}
    res["bytes_written"] = 2 * B * (R * T * 9 + R * 9 + 8)
    for k, feed in feeds.items():
        if hasattr(feed, "state") and int(feed.state[1]) != 0:
            raise SystemExit(f"{kind} {k}: the sampler's ticket is not back at zero")
    del sts, graphs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_review_sample needs an MI355X")
    from review_based_recommender_amd import functional as RF
    torch.manual_seed(0)
    res = {"tool": "bench_review_sample", "optimizer": "HipClipAdam", "graph": f"hipGraph, {SLOTS} resident slots",
           "precision": RF.get_prod_precision(), "dropout": 0.5, "validate_ids": False, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "gathers_per_graph": GATHERS_PER_GRAPH}
    res["narre_cfg3"] = bench_model("narre", synth.NARRE_CFGS["cfg3"], a)
    res["simple_siamese_toys"] = bench_model("simple_siamese", synth.SIAMESE_CFGS["toys"], a)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
