"""Dynamic negative sampling (rbr_sample_hard_negatives, data.NegativeFeed(n_cand=...)) against the uniform sampler, as one JSON
line: the sampler alone at the cfg2 catalogue, and the recorded BPR step of DeepCoNN++ (cfg2) and NARRE (cfg3) with
neg_candidates = 4 against the uniform step in the same run.

    timeout -k 10 900 python tools/bench_hard_negatives.py [--steps 200] [--warmup 20] [--repeats 5] [--limit 840]

  sampler           U = I = 1001, K = 32, B = 256, n_neg = 1, FM head with biases, about 20 seen items per user: ms per launch
                    of rbr_sample_negatives ("uniform") and of rbr_sample_hard_negatives at n_cand 1, 4, 16, 64, each from 20
                    launches recorded into one hipGraph; `parity_n_cand_1`: the three outputs of n_cand = 1 equal the uniform
                    sampler's from the same (seed, call)
  <model>           per model (tools/bench_bpr_step.py's setup: dropout 0.5, HipClipAdam, GraphedTrainStep with 2 resident slots,
                    validate_ids = False), both steps recorded from the same parameters on the same staged batches:
    uniform_step_ms / hard_step_ms   the recorded BPR step with NegativeFeed(n_cand=1) / (n_cand=4, tables of one
                    Recommender.refresh() before the first step: the trainer's snapshot), and hard_minus_uniform_ms; timed
                    with lr 0 (the same launches, the parameters stay put over the thousand replays of two resident batches)
    launches        kernel nodes of the two recorded steps
    refresh_ms      one Recommender.refresh() + set_tables (what an epoch, or neg_refresh_steps updates, pay once)
    share_close     the share of (pair, negative) tuples with pred_neg - pred_pos > -1 -- the tuples whose softplus still has a
                    gradient worth the encode -- over --share-steps replays per variant, the models training as they go (each
                    on its own negatives: a model trained on harder negatives also separates them faster), with mean_loss;
                    share_close_first_step: the first replay alone, the one both variants run from identical parameters
The timed blocks alternate between the variants; device events around each block of --steps calls, medians over --repeats
blocks with min / max.  The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_review_dataset  # noqa: E402
import synth  # noqa: E402
from bench_bpr_step import DEV, PER_GRAPH, SLOTS, build_model, random_seen  # noqa: E402

N_NEG = 1
N_CAND = 4


def alternating_ms(fns, steps, warmup, repeats):
    """Timed blocks of the functions in turn (a, b, a, b, ...), device events around each block: {name: (median, min, max) ms
    per call}."""
    for fn in fns.values():
        for i in range(warmup):
            fn(i)
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for i in range(steps):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            out[k].append(t0.elapsed_time(t1) / steps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def graph_of(fn):
    """PER_GRAPH calls of `fn` recorded into one hipGraph (one eager call first, on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            fn()
    return g


def bench_sampler(a):
    from review_based_recommender_amd import functional as RF
    c = synth.DEEPCONN_CFGS["cfg2"]
    U, I, K, B = c["U"], c["I"], c["K"], 256
    gen = torch.Generator(device=DEV).manual_seed(0)
    ul, il = torch.randn(U, K, generator=gen, device=DEV), torch.randn(I, K, generator=gen, device=DEV)
    head = dict(mode="fm", ul=ul, il=il, h=torch.randn(K, generator=gen, device=DEV), g=torch.randn(1, generator=gen, device=DEV),
                ub=torch.randn(U, generator=gen, device=DEV), ib=torch.randn(I, generator=gen, device=DEV))
    seen = random_seen(U, I, 20, seed=0)
    rng = np.random.default_rng(1)
    u, i = (torch.from_numpy(rng.integers(1, n, B)).to(DEV) for n in (U, I))

    def buffers():
        return (torch.zeros(2 * B, dtype=torch.int64, device=DEV), torch.zeros(2 * B, dtype=torch.int64, device=DEV),
                torch.zeros(B, dtype=torch.float32, device=DEV))

    def state(call=0):
        return torch.tensor([call, 0], dtype=torch.int64, device=DEV)

    uniform = RF.sample_negatives(u, i, N_NEG, I, seen, state=state(3), seed=5)
    one = RF.sample_hard_negatives(u, i, N_NEG, I, seen, n_cand=1, state=state(3), seed=5, **head)
    res = {"B": B, "n_neg": N_NEG, "U": U, "I": I, "K": K, "mode": "fm", "launches_per_graph": PER_GRAPH,
           "parity_n_cand_1": all(torch.equal(x, y) for x, y in zip(uniform, one))}
    graphs, keep = {}, []
    st, out = state(), buffers()
    keep.append((st, out))
    graphs["uniform"] = graph_of(lambda: RF.sample_negatives(u, i, N_NEG, I, seen, state=st, seed=0, out=out))
    for n_cand in (1, 4, 16, 64):
        st, out = state(), buffers()
        keep.append((st, out))
        graphs[f"n_cand_{n_cand}"] = graph_of(lambda n_cand=n_cand, st=st, out=out: RF.sample_hard_negatives(
            u, i, N_NEG, I, seen, n_cand=n_cand, state=st, seed=0, out=out, **head))
    timed = alternating_ms({k: (lambda n, g=g: g.replay()) for k, g in graphs.items()}, a.steps, a.warmup, a.repeats)
    res["ms_per_launch"] = {k: round(v[0] / PER_GRAPH, 5) for k, v in timed.items()}
    res["ms_per_launch_min_max"] = {k: [round(v[1] / PER_GRAPH, 5), round(v[2] / PER_GRAPH, 5)] for k, v in timed.items()}
    return res


def bench_model(kind, c, a):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.train_step import BprObjective, GraphedTrainStep, make_optimizer
    B, U, I = c["B"], c["U"], c["I"]
    rng = np.random.default_rng(0)
    if kind == "deepconn":
        docs = types.SimpleNamespace(user_docs=synth._docs(rng, U, c["L"], c["V"]).tolist(),
                                     item_docs=synth._docs(rng, I, c["L"], c["V"]).tolist(), user_num=U, item_num=I, vocab_size=c["V"])
        cache = inner = D.DeviceDocCache(docs, DEV)
        seen = random_seen(U, I, 20, seed=0)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            meta, train, valid = make_review_dataset.random_split(U, I, c["V"], c["R"], c["T"], 10 * U, B, seed=0)
            make_review_dataset.dump_split(tmp, meta, c["V"], train, valid)
            ds = D.ReviewDataset(tmp, "train")
        cache = D.DeviceReviewCache(ds, DEV)
        inner = cache.feed("narre", True)
        seen = Recommender.seen_from(ds.examples, U, DEV)
    rng = np.random.default_rng(1)
    pairs = [tuple(torch.from_numpy(x).to(DEV) for x in (rng.integers(1, U, B), rng.integers(1, I, B),
                                                          rng.integers(1, 6, B).astype(np.float32))) for _ in range(SLOTS)]
    res = {"B": B, "n_neg": N_NEG, "n_cand": N_CAND, "U": U, "I": I}

    def stepper(n_cand, **opt):
        m = build_model(kind, c)
        nf = D.NegativeFeed(inner, seen, I, n_neg=N_NEG, seed=0, n_cand=n_cand)
        if n_cand > 1:
            rec = Recommender(m, cache)

            def refresh():
                rec.refresh()
                nf.set_tables(m.score_mode_and_params()[0], rec.user_latents, rec.item_latents, *m.score_mode_and_params()[1:])

            refresh()
            if "refresh_ms" not in res:
                res["refresh_ms"] = round(alternating_ms({"r": lambda n: refresh()}, 3, 1, 3)["r"][0], 3)
        u, i, r = pairs[0]
        st = GraphedTrainStep.from_ids(m, make_optimizer(m, capturable=True, hip_clip_adam=True, **opt), nf, u, i, r, slots=SLOTS,
                                       keep_graph=True, objective=BprObjective(nf))
        for s, (u, i, r) in enumerate(pairs):
            st.stage(s, (u, i), r)
        nf.reseed(0, call=0)
        return st, nf

    (uni, nf_u), (hard, nf_h) = stepper(1), stepper(N_CAND)
    res["launches"] = {"uniform": uni.kernel_launches(), "hard": hard.kernel_launches()}

    # the shares first, from the same parameters and the same call numbers: what the extra launch buys
    close = {"uniform": torch.zeros((), device=DEV), "hard": torch.zeros((), device=DEV)}
    loss = {"uniform": torch.zeros((), device=DEV), "hard": torch.zeros((), device=DEV)}
    res["share_close_first_step"] = {}
    for n in range(a.share_steps):
        for name, st in (("uniform", uni), ("hard", hard)):
            step_loss, _, pred = st(slot=n % SLOTS)
            share = ((pred[B:].view(N_NEG, B) - pred[:B]) > -1.0).float().mean()
            if n == 0:          # the one replay both variants run from identical parameters
                res["share_close_first_step"][name] = round(float(share), 4)
            close[name] += share
            loss[name] += step_loss
    res["share_close"] = {k: round(float(v) / a.share_steps, 4) for k, v in close.items()}
    res["mean_loss"] = {k: round(float(v) / a.share_steps, 4) for k, v in loss.items()}
    res["share_steps"] = a.share_steps
    for name, st in (("uniform", uni), ("hard", hard)):
        if not np.isfinite(float(st.loss)):
            raise SystemExit(f"{kind}: non-finite BPR loss in the {name} step")
    del uni, hard
    torch.cuda.empty_cache()

    # the timing on steps that leave the parameters where they are (lr 0: the same launches doing the same work): a thousand
    # replays of two resident batches at the default lr memorise them, scores reach 1e3 and the loss of either variant can overflow
    (uni, nf_u), (hard, nf_h) = stepper(1, lr=0.0), stepper(N_CAND, lr=0.0)
    timed = alternating_ms({"uniform": lambda n: uni(slot=n % SLOTS), "hard": lambda n: hard(slot=n % SLOTS)}, a.steps, a.warmup, a.repeats)
    res["uniform_step_ms"], res["hard_step_ms"] = round(timed["uniform"][0], 4), round(timed["hard"][0], 4)
    res["step_ms_min_max"] = {k: [round(v[1], 4), round(v[2], 4)] for k, v in timed.items()}
    res["hard_minus_uniform_ms"] = round(timed["hard"][0] - timed["uniform"][0], 4)
    for name, st in (("uniform", uni), ("hard", hard)):
        if not np.isfinite(float(st.loss)):
            raise SystemExit(f"{kind}: non-finite BPR loss in the {name} step")
    res["valid_fraction"] = {"uniform": round(float(nf_u.valid.mean()), 4), "hard": round(float(nf_h.valid.mean()), 4)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share-steps", type=int, default=50, help="replays per variant behind share_close")
    ap.add_argument("--limit", type=int, default=840, help="seconds after which the process ends itself")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hard_negatives.py needs an MI355X: there is no CPU fallback and no CPU timing")
    signal.alarm(a.limit)
    from review_based_recommender_amd import functional as RF
    torch.manual_seed(0)
    res = {"bench": "hard_negatives", "device": torch.cuda.get_device_name(0), "optimizer": "HipClipAdam",
           "graph": f"hipGraph, {SLOTS} resident slots", "precision": RF.get_prod_precision(), "dropout": 0.5, "validate_ids": False,
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    res["sampler"] = bench_sampler(a)
    res["deepconn_cfg2"] = bench_model("deepconn", synth.DEEPCONN_CFGS["cfg2"], a)
    res["narre_cfg3"] = bench_model("narre", synth.NARRE_CFGS["cfg3"], a)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
