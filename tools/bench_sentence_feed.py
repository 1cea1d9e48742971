"""The id-fed sentence split (AHN) against the example-fed one, as one JSON line, at the reference's default config
(models/ahn/default_ahn.json: batch 32, 300-d words, hidden 300, k 10, dropout 0.5; 10 reviews of 10 sentences of 20 words).

    timeout -k 10 900 python tools/bench_sentence_feed.py [--steps 50] [--warmup 5] [--repeats 5] [--loader-batches 40]

Both feeds run the same EAGER step (train_step with HipClipAdam, validate_ids = False: what `trainer.py --model ahn` runs with
fast_step; AHN's step is not recorded as a hipGraph) on a reference-shaped sentence split in a temporary directory
(tests/make_sentence_dataset.random_split: 201 users / 201 items, V = 20000, ragged meta, leave-one-out train examples).  The
example-fed side is this project's SentenceDataset.collate_fn (numpy), not the reference's per-sentence collate.
  gather_ms            rbr_sentence_gather alone at the step's shape: 20 gathers recorded into one hipGraph, device events around
                       blocks of replays, per gather; gather_bytes = what one gather reads and writes
  step_ms              from a collated host batch to the end of the step, per step: host-to-device copies, the lengths and masks
                       (example-fed: data.sentence_masks on the device; id-fed: made by the gather), forward, backward, clip + Adam;
                       the same pairs on both feeds, the timed blocks of the two feeds alternate, step_ms_min_max is their spread
  loader_ms            host time of the dataset's collate per batch (no GPU work)
  trainer_pairs_per_s  DataLoader (num_workers=0, shuffled) -> to device -> step, over --loader-batches batches
Medians over --repeats timed blocks of --steps steps (loader figures: one block of --loader-batches batches each)."""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_sentence_dataset  # noqa: E402
from make_review_dataset import dump_split  # noqa: E402

DEV = torch.device("cuda", 0)
B, R, S, W, E, H, K, V, U, I = 32, 10, 10, 20, 300, 300, 10, 20000, 201, 201
GATHERS_PER_GRAPH = 20


def build_model():
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = AHN(E, H, K, U, I, V, None, rnn_dropout=0.0, dropout=0.5, item_review_num=R)
    m.validate_ids = False
    return m.to(DEV).train()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loader-batches", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sentence_feed needs an MI355X")
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import make_optimizer, train_step

    with tempfile.TemporaryDirectory() as tmp:
        meta, train, valid = make_sentence_dataset.random_split(U, I, V, R, S, W, max(2 * B * a.loader_batches, 10 * U), B, seed=0)
        dump_split(tmp, meta, V, train, valid)
        ds_ex = D.SentenceDataset(tmp, "train")
        ds_ids = D.SentenceDataset(tmp, "train", feed="ids")
    cache = D.DeviceSentenceCache(ds_ex, DEV)
    feed = cache.feed(True)
    rng = np.random.default_rng(1)
    picks = [[int(k) for k in rng.choice(len(ds_ex), size=B, replace=False)] for _ in range(4)]
    ex_batches = [ds_ex.collate_fn([ds_ex[k] for k in p]) for p in picks]
    id_batches = [ds_ids.collate_fn([ds_ids[k] for k in p]) for p in picks]

    def example_inputs(batch):
        """trainer._to_device for AHN."""
        batch = [t.to(DEV, non_blocking=True) for t in batch]
        u_revs, i_revs, u_ids, i_ids = batch[:4]
        (u_len, u_sm, u_rm), (i_len, i_sm, i_rm) = D.sentence_masks(u_revs), D.sentence_masks(i_revs)
        return (u_revs, i_revs, u_sm, i_sm, u_len, i_len, u_rm, i_rm, u_ids, i_ids), batch[-1]

    def id_inputs(batch):
        u_ids, i_ids, ratings = [t.to(DEV, non_blocking=True) for t in batch]
        return feed.inputs(u_ids, i_ids), ratings

    # the two feeds hand the model the same bits
    for x, y in zip(example_inputs(ex_batches[0])[0], id_inputs(id_batches[0])[0]):
        if x.dtype != y.dtype or not torch.equal(x, y):
            raise SystemExit("the id-fed batch differs from the example-fed one")

    res = {"tool": "bench_sentence_feed", "device": torch.cuda.get_device_name(0), "optimizer": "HipClipAdam", "graph": "none (eager step)",
           "dropout": 0.5, "validate_ids": False, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "loader_batches": a.loader_batches, "shape": {"B": B, "R": R, "S": S, "W": W, "E": E, "H": H, "K": K, "V": V, "U": U, "I": I},
           "train_examples": len(ds_ex)}

    # ---- the gather alone
    u, i = id_batches[0][0].to(DEV), id_batches[0][1].to(DEV)
    out = dict(zip(cache.NAMES, cache.gather(u, i, True)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cache.gather(u, i, True, **out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GATHERS_PER_GRAPH):
            cache.gather(u, i, True, **out)
    for _ in range(a.warmup):
        g.replay()
    blocks = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            g.replay()
        e1.record()
        e1.synchronize()
        blocks.append(e0.elapsed_time(e1) / (a.steps * GATHERS_PER_GRAPH))
    res["gather_ms"] = round(statistics.median(blocks), 5)
    res["gather_ms_min_max"] = [round(min(blocks), 5), round(max(blocks), 5)]
    # per row: int32 tokens read and int64 tokens written, int64 lengths and 1-byte masks written, R + 1 int32 rids read and R int64
    # rids written, the id read and written
    res["gather_bytes"] = 2 * B * (R * S * W * 12 + R * S * 9 + R + (R + 1) * 4 + R * 8 + 16)
    del g

    # ---- the eager step from a host batch
    steppers = {}
    for k, make, batches in (("example_fed", example_inputs, ex_batches), ("id_fed", id_inputs, id_batches)):
        m = build_model()
        opt = make_optimizer(m, hip_clip_adam=True)

        def step(n, m=m, opt=opt, make=make, batches=batches):
            inputs, ratings = make(batches[n % len(batches)])
            return train_step(m, opt, inputs, ratings)[0]
        steppers[k] = step
    for fn in steppers.values():
        for n in range(a.warmup):
            fn(n)
    timed = {k: [] for k in steppers}
    for _ in range(a.repeats):
        for k, fn in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(a.steps):
                fn(n)
            torch.cuda.synchronize()
            timed[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res["step_ms"] = {k: round(statistics.median(v), 4) for k, v in timed.items()}
    res["step_ms_min_max"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in timed.items()}

    # ---- the loader's host time, and the loader + step loop
    res["loader_ms"], res["trainer_pairs_per_s"] = {}, {}
    for k, ds, make in (("example_fed", ds_ex, example_inputs), ("id_fed", ds_ids, id_inputs)):
        order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).tolist()
        idx = [order[j * B:(j + 1) * B] for j in range(a.loader_batches)]
        t0 = time.perf_counter()
        for j in range(a.loader_batches):
            ds.collate_fn([ds[x] for x in idx[j]])
        res["loader_ms"][k] = round((time.perf_counter() - t0) * 1e3 / a.loader_batches, 4)
        sub = torch.utils.data.Subset(ds, order[:B * a.loader_batches])
        loader = torch.utils.data.DataLoader(sub, batch_size=B, shuffle=True, collate_fn=ds.collate_fn, num_workers=0,
                                             drop_last=True, generator=torch.Generator().manual_seed(0))
        m = build_model()
        opt = make_optimizer(m, hip_clip_adam=True)
        train_step(m, opt, *make(next(iter(loader))))            # first-use set-up outside the timed loop
        acc = torch.zeros((), device=DEV)
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in loader:
            inputs, ratings = make(batch)
            acc += train_step(m, opt, inputs, ratings)[0]
            n += ratings.shape[0]
        torch.cuda.synchronize()
        res["trainer_pairs_per_s"][k] = round(n / (time.perf_counter() - t0), 1)
        if not torch.isfinite(acc):
            raise SystemExit(f"{k}: non-finite loss in the trainer loop")
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
