"""The id-fed review split against the example-fed one, as one JSON line: NARRE at the cfg3 shape and SimpleSiamese at the `toys`
shape (defalut_simple_train.json).

    python tools/bench_review_feed.py [--steps 200] [--warmup 20] [--repeats 5] [--loader-batches 40]

Both feeds run the same recorded step (dropout 0.5, HipClipAdam, GraphedTrainStep, validate_ids = False, as the trainer runs it) on
a reference-shaped review split in a temporary directory (tests/make_review_dataset.random_split: 1001 users / 1001 items, ragged
meta, leave-one-out train examples; tokens uniform over the vocabulary).  The id-fed step records rbr_review_gather into each slot
in front of the step.  Per model:
  step_ms              replay of a resident slot (4 slots, rotated), per step; the same pairs on both feeds; the timed blocks of
                       the two feeds alternate, step_ms_min_max is the spread of the blocks
  gather_ms            rbr_review_gather alone at the step's shape: 20 gathers recorded into one hipGraph, per gather -- the bound
                       on how far the id-fed step_ms may lie above the example-fed one
  loader_ms            per batch: the dataset's collate + staging into the step's input slot + synchronise, the way the trainer
                       stages (SimpleSiamese's example feed goes through device tensors and derives its review masks there)
  trainer_pairs_per_s  DataLoader (num_workers=0, shuffled) -> stage -> replay of a one-slot step over --loader-batches steps
  launches             kernel nodes of the recorded steps (kernel_launches(), keep_graph=True)
Medians over --repeats timed blocks of --steps steps (loader figures: one block of --loader-batches batches each).
"""
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
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_review_dataset  # noqa: E402
import synth  # noqa: E402

DEV = torch.device("cuda", 0)
SLOTS = 4
GATHERS_PER_GRAPH = 20


def build_model(kind, c):
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "narre":
            from review_based_recommender_amd.models.narre.narre import NARRE
            m = NARRE(c["U"], c["I"], c["V"], c["kz"], c["H"], c["D"], c["A"], c["K"], c["R"], c["T"], 0.5, 0, 0, 0, None, "CNN")
            m.load_state_dict(synth.narre_params(c, 0))
        else:
            from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
            m = SimpleSiamese(c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.5, 0.2, 0.0, c["UB"], c["LT"])
            m.load_state_dict(synth.siamese_params(c, 0))
    m.validate_ids = False
    return m.to(DEV).train()


def median_ms(fn, steps, warmup, repeats):
    for i in range(warmup):
        fn(i)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return statistics.median(out)


def alternating_ms(fns, steps, warmup, repeats):
    """Timed blocks of the functions in turn (a, b, a, b, ...), so that drift of the box lands on all of them alike: {name:
    (median, min, max) ms per step}."""
    for fn in fns.values():
        for i in range(warmup):
            fn(i)
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                fn(i)
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def model_args(kind, batch):
    """A collate batch on the device as (the model's arguments, ratings): trainer._to_device."""
    batch = [t.to(DEV, non_blocking=True) for t in batch]
    if kind == "simple_siamese":
        u_revs, i_revs, u_wm, i_wm, u_ids, i_ids = batch[:6]
        return (u_revs, i_revs, u_wm, i_wm, u_wm.any(-1), i_wm.any(-1), u_ids, i_ids), batch[-1]
    return tuple(batch[:-1]), batch[-1]


def bench_model(kind, c, a):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    B = c["B"]
    with tempfile.TemporaryDirectory() as tmp:
        n_train = max(B * a.loader_batches, 10 * c["U"])
        meta, train, valid = make_review_dataset.random_split(c["U"], c["I"], c["V"], c["R"], c["T"], n_train, B, seed=0)
        make_review_dataset.dump_split(tmp, meta, c["V"], train, valid)
        ds_ex = D.ReviewDataset(tmp, "train")
        ds_ids = D.ReviewDataset(tmp, "train", feed="ids")
    cache = D.DeviceReviewCache(ds_ex, DEV)
    feed = cache.feed(kind, True)
    rng = np.random.default_rng(1)
    picks = [[int(k) for k in rng.choice(len(ds_ex), size=B, replace=False)] for _ in range(SLOTS)]
    ex_batches = [ds_ex.collate_fn([ds_ex[k] for k in p]) for p in picks]
    id_batches = [ds_ids.collate_fn([ds_ids[k] for k in p]) for p in picks]

    def steppers(slots):
        out = {}
        inputs, ratings = model_args(kind, ex_batches[0])
        m = build_model(kind, c)
        out["example_fed"] = GraphedTrainStep(m, make_optimizer(m, capturable=True, hip_clip_adam=True), inputs, ratings, slots=slots,
                                              keep_graph=True)
        u, i, r = [t.to(DEV) for t in id_batches[0]]
        m = build_model(kind, c)
        out["id_fed"] = GraphedTrainStep.from_ids(m, make_optimizer(m, capturable=True, hip_clip_adam=True), feed, u, i, r,
                                                  slots=slots, keep_graph=True)
        return out

    def stage(k, st, s, ex_batch, id_batch):
        if k == "id_fed":
            st.stage(s, tuple(id_batch[:-1]), id_batch[-1])
        elif kind == "simple_siamese":                  # its review masks are derived on the device: no direct host staging
            st.stage(s, *model_args(kind, ex_batch))
        else:
            st.stage(s, tuple(ex_batch[:-1]), ex_batch[-1])

    res = {"B": B, "R": c["R"], "T": c["T"]}
    sts = steppers(SLOTS)
    res["launches"] = {k: st.kernel_launches() for k, st in sts.items()}
    for k, st in sts.items():
        for s in range(SLOTS):
            stage(k, st, s, ex_batches[s], id_batches[s])
    timed = alternating_ms({k: (lambda n, st=st: st(slot=n % SLOTS)) for k, st in sts.items()}, a.steps, a.warmup, a.repeats)
    res["step_ms"] = {k: round(v[0], 4) for k, v in timed.items()}
    res["step_ms_min_max"] = {k: [round(v[1], 4), round(v[2], 4)] for k, v in timed.items()}

    # the gather alone, at the step's shape, into the id-fed step's own input views
    st = sts["id_fed"]
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
    res["gather_ms"] = round(median_ms(lambda n: g.replay(), a.steps, a.warmup, a.repeats) / GATHERS_PER_GRAPH, 5)
    res["gather_bytes"] = 2 * B * c["R"] * c["T"] * 13
    del sts, st, g, views
    torch.cuda.empty_cache()

    res["loader_ms"], res["trainer_pairs_per_s"] = {}, {}
    sts = steppers(1)
    for k, ds in (("example_fed", ds_ex), ("id_fed", ds_ids)):
        st = sts[k]
        order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).tolist()
        idx = [order[j * B:(j + 1) * B] for j in range(a.loader_batches)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(a.loader_batches):
            batch = ds.collate_fn([ds[x] for x in idx[j]])
            stage(k, st, 0, batch, batch)
            torch.cuda.synchronize()
        res["loader_ms"][k] = round((time.perf_counter() - t0) * 1e3 / a.loader_batches, 4)
        sub = torch.utils.data.Subset(ds, order[:B * a.loader_batches])
        loader = torch.utils.data.DataLoader(sub, batch_size=B, shuffle=True, collate_fn=ds.collate_fn, num_workers=0,
                                             drop_last=True, generator=torch.Generator().manual_seed(0))
        acc = torch.zeros((), device=DEV)
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in loader:
            stage(k, st, 0, batch, batch)
            loss, gnorm, _ = st(slot=0)
            acc += loss.clone()
            n += batch[-1].shape[0]
        torch.cuda.synchronize()
        res["trainer_pairs_per_s"][k] = round(n / (time.perf_counter() - t0), 1)
        if not torch.isfinite(acc):
            raise SystemExit(f"{kind} {k}: non-finite loss in the trainer loop")
    del sts
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loader-batches", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_review_feed needs an MI355X")
    from review_based_recommender_amd import functional as RF
    torch.manual_seed(0)
    res = {"tool": "bench_review_feed", "optimizer": "HipClipAdam", "graph": f"hipGraph, {SLOTS} resident slots",
           "precision": RF.get_prod_precision(), "dropout": 0.5, "validate_ids": False, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "loader_batches": a.loader_batches}
    res["narre_cfg3"] = bench_model("narre", synth.NARRE_CFGS["cfg3"], a)
    res["simple_siamese_toys"] = bench_model("simple_siamese", synth.SIAMESE_CFGS["toys"], a)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
