"""The id-fed doc split against the doc-fed one at the cfg2 shape, as one JSON line.

    python tools/bench_id_feed.py [--steps 200] [--warmup 20] [--repeats 5] [--loader-batches 40]

Both feeds run the headline's step (bench.py: DeepCoNN++ cfg2, dropout 0.5, HipClipAdam, GraphedTrainStep, the f32 class) with
validate_ids = False, as the trainer runs it.  The id-fed step records rbr_doc_gather into each slot in front of the same step.
  step_ms              replay of a resident slot (4 slots, rotated), per step; the same pairs on both feeds, with the headline's
                       synth-style Zipf documents (keyed by id) and ids uniform over [1, 1001)
  loader_ms            per batch: DocDataset collate + staging into the step's input slot + synchronise (a make_dataset-style
                       doc split of 1001 users / 1001 items / L = 512 / V = 50002 in a temporary directory; its tokens are
                       uniform over the vocabulary, which makes its step slower than the Zipf documents' step)
  trainer_pairs_per_s  DataLoader (num_workers=0, shuffled) -> stage -> replay of a one-slot step over --loader-batches steps on
                       that split: the trainer's loop
  repeat_ids           ids Zipf(1.07) over 1001, Zipf documents keyed by id: the distinct-document fraction of a batch and the
                       id-fed step with dedup_by_id off / on
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
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_dataset  # noqa: E402
import synth  # noqa: E402

DEV = torch.device("cuda", 0)
SLOTS = 4


def build_model(cfg, dedup=False):
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    with contextlib.redirect_stdout(io.StringIO()):
        m = DeepCoNNpp(cfg["U"], cfg["I"], cfg["V"], cfg["kz"], cfg["D"], cfg["H"], cfg["K"], cfg["L"], None, 0.5)
    m.load_state_dict(synth.deepconn_params(cfg, 0))
    m.validate_ids = False
    m.dedup_by_id = dedup
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


def zipf_ids(rng, n, rows, s=1.07):
    p = np.arange(1, rows + 1, dtype=np.float64) ** -s
    return torch.from_numpy(rng.choice(rows, size=n, p=p / p.sum()).astype(np.int64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loader-batches", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_id_feed needs an MI355X")
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    torch.manual_seed(0)
    cfg = synth.DEEPCONN_CFGS["cfg2"]
    B, L, V, U, I = cfg["B"], cfg["L"], cfg["V"], cfg["U"], cfg["I"]

    with tempfile.TemporaryDirectory() as tmp:
        n_train = B * a.loader_batches
        make_dataset.write_doc_split(tmp, n_users=U, n_items=I, vocab=V, doc_len=L, n_train=n_train, n_valid=B, seed=0)
        ds_doc = D.DocDataset(tmp, "train")
        ds_ids = D.DocDataset(tmp, "train", feed="ids")
    ds_cache = D.DeviceDocCache(ds_doc, DEV)
    rng = np.random.default_rng(0)
    zipf_docs = types.SimpleNamespace(user_docs=synth._docs(rng, U, L, V).tolist(), item_docs=synth._docs(rng, I, L, V).tolist(),
                                      user_num=U, item_num=I, vocab_size=V)
    zcache = D.DeviceDocCache(zipf_docs, DEV)

    def doc_fed(cache, u, i):
        ud, idc = cache.user.cpu()[u].long(), cache.item.cpu()[i].long()
        return ud, idc, ud != 0, idc != 0, u.clone(), i.clone()

    rng = np.random.default_rng(1)
    pairs = [(torch.from_numpy(rng.integers(1, U, B)), torch.from_numpy(rng.integers(1, I, B)),
              torch.from_numpy(rng.integers(1, 6, B).astype(np.float32))) for _ in range(SLOTS)]

    def steppers(cache, dedup=False, with_doc=True, slots=SLOTS):
        out = {}
        u0, i0, r0 = pairs[0]
        if with_doc:
            m = build_model(cfg, dedup)
            o = make_optimizer(m, capturable=True, hip_clip_adam=True)
            out["doc_fed"] = GraphedTrainStep(m, o, [t.to(DEV) for t in doc_fed(cache, u0, i0)], r0.to(DEV), slots=slots,
                                              keep_graph=True)
        m = build_model(cfg, dedup)
        o = make_optimizer(m, capturable=True, hip_clip_adam=True)
        out["id_fed"] = GraphedTrainStep.from_ids(m, o, cache, u0.to(DEV), i0.to(DEV), r0.to(DEV), slots=slots, keep_graph=True)
        return out

    def stage_doc(st, s, u, i, r):
        st.stage(s, doc_fed(zcache, u, i), r)

    def stage_ids(st, s, u, i, r):
        st.stage(s, (u, i), r)

    stage = {"doc_fed": stage_doc, "id_fed": stage_ids}
    res = {"tool": "bench_id_feed", "workload": "DeepCoNN++ cfg2", "B": B, "L": L, "optimizer": "HipClipAdam",
           "graph": f"hipGraph, {SLOTS} resident slots", "precision": RF.get_prod_precision(), "dropout": 0.5,
           "validate_ids": False, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}

    sts = steppers(zcache)
    res["launches"] = {k: st.kernel_launches() for k, st in sts.items()}
    res["step_ms"] = {}
    for k, st in sts.items():
        for s, (u, i, r) in enumerate(pairs):
            stage[k](st, s, u, i, r)
        res["step_ms"][k] = round(median_ms(lambda n, st=st: st(slot=n % SLOTS), a.steps, a.warmup, a.repeats), 4)

    del sts
    torch.cuda.empty_cache()

    # loader: collate + stage into slot 0 + synchronise, per batch; then the trainer's loop DataLoader -> stage -> replay
    res["loader_ms"], res["trainer_pairs_per_s"] = {}, {}
    sts = steppers(ds_cache, slots=1)
    for k, ds in (("doc_fed", ds_doc), ("id_fed", ds_ids)):
        st = sts[k]
        order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).tolist()
        idx = [order[j * B:(j + 1) * B] for j in range(a.loader_batches)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(a.loader_batches):
            batch = ds.collate_fn([ds[x] for x in idx[j]])
            st.stage(0, tuple(batch[:-1]), batch[-1])
            torch.cuda.synchronize()
        res["loader_ms"][k] = round((time.perf_counter() - t0) * 1e3 / a.loader_batches, 4)
        loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, collate_fn=ds.collate_fn, num_workers=0,
                                             drop_last=True, generator=torch.Generator().manual_seed(0))
        acc = torch.zeros((), device=DEV)
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in loader:
            st.stage(0, tuple(batch[:-1]), batch[-1])
            loss, gnorm, _ = st(slot=0)
            acc += loss.clone()
            n += batch[-1].shape[0]
        torch.cuda.synchronize()
        res["trainer_pairs_per_s"][k] = round(n / (time.perf_counter() - t0), 1)
        if not torch.isfinite(acc):
            raise SystemExit(f"{k}: non-finite loss in the trainer loop")
    del sts
    torch.cuda.empty_cache()

    # repeated ids: Zipf(1.07) over 1001, documents keyed by id; id-fed step with dedup_by_id off / on
    rng = np.random.default_rng(2)
    pairs = [(zipf_ids(rng, B, U), zipf_ids(rng, B, I), torch.from_numpy(rng.integers(1, 6, B).astype(np.float32)))
             for _ in range(SLOTS)]
    frac = statistics.mean((len(set(u.tolist())) + len(set(i.tolist()))) / (2 * B) for u, i, _ in pairs)
    rep = {"distinct_doc_fraction": round(frac, 4), "id_fed_step_ms": {}}
    for dedup in (False, True):
        st = steppers(zcache, dedup, with_doc=False)["id_fed"]
        for s, (u, i, r) in enumerate(pairs):
            st.stage(s, (u, i), r)
        rep["id_fed_step_ms"]["dedup_on" if dedup else "dedup_off"] = round(
            median_ms(lambda n, st=st: st(slot=n % SLOTS), a.steps, a.warmup, a.repeats), 4)
        del st
        torch.cuda.empty_cache()
    res["repeat_ids"] = rep
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
