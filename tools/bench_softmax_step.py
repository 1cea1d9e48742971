"""The recorded in-batch softmax step (id-feed gather + towers + all-pairs loss) against the recorded MSE id-fed step on the same B
pairs and the recorded BPR step with n_neg = 1, as one JSON line: DeepCoNN++ at the cfg2 shape and NARRE at the cfg3 shape, B = 256.

    timeout -k 10 900 python tools/bench_softmax_step.py [--steps 200] [--warmup 20] [--repeats 5] [--limit 840]

Per model (dropout 0.5, HipClipAdam, GraphedTrainStep with 2 resident slots, validate_ids = False, as the trainer runs it), the
protocol of tools/bench_bpr_step.py:
  softmax_step_ms   (a) from_ids(InBatchFeed(feed), objective=InBatchSoftmaxObjective): B pairs, B - 1 in-batch negatives each
  mse_step_ms       (b) from_ids(feed) on the same B pairs: the step the package had before; (a) - (b) is the price of the
                    un-fused tail plus the two new launches
  bpr_step_ms       (c) from_ids(NegativeFeed(feed), objective=BprObjective), n_neg = 1: 2B documents per side
  launches          kernel nodes of the three recorded steps (kernel_launches(), keep_graph=True)
  loss_ms           functional.pair_softmax_loss forward + unit-root backward alone at the step's shape (in-kernel dropout, seen
                    CSR, biases), 20 per hipGraph, per call
  torch_loss_ms     the torch autograd composition of the same loss, eager (broadcast [B, B, K], searchsorted mask, logsumexp)
  max_diff          the largest difference between the two: loss and the gradients of ul, il, h (explicit dropout multiplier)
The timed blocks of (a), (b), (c) alternate; medians over --repeats blocks of --steps replays, with min / max.  Seen lists as
in bench_bpr_step.py.  The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import bench_bpr_step as BB  # noqa: E402  (puts the repository root and tests/ on sys.path)
import make_review_dataset  # noqa: E402
import synth  # noqa: E402

DEV = BB.DEV
SLOTS = BB.SLOTS
B = 256


def torch_loss(ul, il, h, row_bias, col_bias, drop, u, i, keys, n_items, temperature):
    """The loss as torch ops on the device: broadcast [B, B, K], the seen test as a searchsorted over the sorted (user, item) keys."""
    s = (torch.relu(ul[:, None, :] * il[None, :, :]) * drop * h).sum(-1) + row_bias[:, None] + col_bias[None, :]
    z = s / temperature
    key = (u[:, None] * n_items + i[None, :]).reshape(-1)
    at = torch.searchsorted(keys, key).clamp_max(keys.numel() - 1)
    in_seen = (keys[at] == key).view(z.shape)
    allowed = torch.eye(z.shape[0], dtype=torch.bool, device=z.device) | ((i[None, :] >= 1) & (i[None, :] != i[:, None]) & ~in_seen)
    lse = torch.logsumexp(torch.where(allowed, z, torch.full_like(z, float("-inf"))), dim=1)
    return (lse - z.diagonal()).mean()


def bench_model(kind, c, a):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.train_step import BprObjective, GraphedTrainStep, InBatchSoftmaxObjective, make_optimizer
    U, I, K = c["U"], c["I"], c["K"]
    rng = np.random.default_rng(0)
    if kind == "deepconn":
        docs = types.SimpleNamespace(user_docs=synth._docs(rng, U, c["L"], c["V"]).tolist(),
                                     item_docs=synth._docs(rng, I, c["L"], c["V"]).tolist(), user_num=U, item_num=I, vocab_size=c["V"])
        inner = D.DeviceDocCache(docs, DEV)
        seen = BB.random_seen(U, I, 20, seed=0)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            meta, train, valid = make_review_dataset.random_split(U, I, c["V"], c["R"], c["T"], 10 * U, B, seed=0)
            make_review_dataset.dump_split(tmp, meta, c["V"], train, valid)
            ds = D.ReviewDataset(tmp, "train")
        inner = D.DeviceReviewCache(ds, DEV).feed("narre", True)
        seen = Recommender.seen_from(ds.examples, U, DEV)
    rng = np.random.default_rng(1)
    pairs = [tuple(torch.from_numpy(x).to(DEV) for x in (rng.integers(1, U, B), rng.integers(1, I, B),
                                                          rng.integers(1, 6, B).astype(np.float32))) for _ in range(SLOTS)]

    def stepper(which):
        m = BB.build_model(kind, c)
        feed, obj = inner, None
        if which == "softmax":
            feed = D.InBatchFeed(inner, seen)
            obj = InBatchSoftmaxObjective(m, feed)
        elif which == "bpr":
            feed = D.NegativeFeed(inner, seen, I, n_neg=1, seed=0)
            obj = BprObjective(feed)
        u, i, r = pairs[0]
        st = GraphedTrainStep.from_ids(m, make_optimizer(m, capturable=True, hip_clip_adam=True), feed, u, i, r, slots=SLOTS,
                                       keep_graph=True, objective=obj)
        for s, (u, i, r) in enumerate(pairs):
            st.stage(s, (u, i), r)
        return st

    res = {"B": B, "K": K, "U": U, "I": I, "seen_per_user_mean": round(seen.items.numel() / max(U - 1, 1), 1)}
    steps = {k: stepper(k) for k in ("softmax", "mse", "bpr")}
    res["launches"] = {k: st.kernel_launches() for k, st in steps.items()}
    timed = BB.alternating_ms({k: (lambda n, st=st: st(slot=n % SLOTS)) for k, st in steps.items()}, a.steps, a.warmup, a.repeats)
    for k in steps:
        res[f"{k}_step_ms"] = round(timed[k][0], 4)
    res["step_ms_min_max"] = {k: [round(v[1], 4), round(v[2], 4)] for k, v in timed.items()}
    res["softmax_minus_mse_ms"] = round(timed["softmax"][0] - timed["mse"][0], 4)
    res["softmax_below_bpr_ranges_disjoint"] = bool(timed["softmax"][2] < timed["bpr"][1])
    for k, st in steps.items():
        if not np.isfinite(float(st.loss)):
            raise SystemExit(f"{kind}: non-finite {k} loss")
    res["softmax_loss"] = round(float(steps["softmax"].loss), 4)
    del steps
    torch.cuda.empty_cache()

    # the loss alone, at the step's shape
    u, i, _ = pairs[0]
    gen = torch.Generator(device=DEV).manual_seed(0)
    leaves = [(0.3 * torch.randn(B, K, device=DEV, generator=gen)).requires_grad_(True) for _ in range(2)]
    h = (0.1 * torch.randn(K, device=DEV, generator=gen)).requires_grad_(True)
    rb, cb = (0.1 * torch.randn(B, device=DEV, generator=gen) for _ in range(2))
    unit = RF.unit_scalar(DEV)

    def hip(drop=None, p_drop=0.5):
        for t in (*leaves, h):
            t.grad = None
        loss, _ = RF.pair_softmax_loss(leaves[0], leaves[1], u, i, "fm", h=h, row_bias=rb, col_bias=cb, drop=drop, seen=seen,
                                       item_lo=1, p_drop=p_drop)
        loss.backward(unit)
        return loss

    res["loss_ms"] = round(BB.graphed_ms(hip, a), 5)
    owner = torch.repeat_interleave(torch.arange(U, device=DEV), seen.off[1:] - seen.off[:-1])
    keys = owner * I + seen.items.long()
    drop = RF.dropout_multiplier((B, B, K), 0.5, True, DEV)

    def composed():
        for t in (*leaves, h):
            t.grad = None
        loss = torch_loss(leaves[0], leaves[1], h, rb, cb, drop, u, i, keys, I, 1.0)
        loss.backward()
        return loss

    l_hip = hip(drop, 0.0).detach().clone()
    g_hip = [t.grad.clone() for t in (*leaves, h)]
    l_t = composed().detach()
    res["max_diff"] = {"loss": float((l_hip - l_t).abs()),
                       **{n: float((g - t.grad).abs().max()) for n, g, t in zip(("d_ul", "d_il", "d_h"), g_hip, (*leaves, h))}}
    timed = BB.alternating_ms({"hip": lambda n: hip(), "torch": lambda n: composed()}, a.steps, a.warmup, a.repeats)
    res["loss_eager_ms"], res["torch_loss_ms"] = round(timed["hip"][0], 4), round(timed["torch"][0], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=840, help="seconds after which the process ends itself")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_softmax_step.py needs an MI355X: there is no CPU fallback and no CPU timing")
    signal.alarm(a.limit)
    from review_based_recommender_amd import functional as RF
    torch.manual_seed(0)
    res = {"bench": "softmax_step", "device": torch.cuda.get_device_name(0), "optimizer": "HipClipAdam",
           "graph": f"hipGraph, {SLOTS} resident slots", "precision": RF.get_prod_precision(), "dropout": 0.5, "validate_ids": False,
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    res["deepconn_cfg2"] = bench_model("deepconn", synth.DEEPCONN_CFGS["cfg2"], a)
    res["narre_cfg3"] = bench_model("narre", synth.NARRE_CFGS["cfg3"], a)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
