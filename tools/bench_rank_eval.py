"""Held-out rank evaluation (rbr_pair_score_rank, csrc/pair_score.hip) against the composition the package offered before it, as one
JSON line.

    timeout -k 10 600 python tools/bench_rank_eval.py [--repeats 5] [--iters 20] [--warmup 3] [--limit 540]

Shape: synthetic latent tables U = I = 50 001, K = 50, fm mode with biases; B = 4096 held-out (user, item) pairs; a training-like
exclusion list of about 20 items per user (CSR over all user ids, served to the pairs through their user ids, as
Recommender.rank serves a SeenItems).  Timed, all on the same gathered user rows:
  fused_ms     functional.pair_score_rank (item_lo = 1): two launches, a [B, slices] workspace of int pairs
  composed_ms  what could be written without it: functional.pair_score_dense over chunks of user rows (--budget bytes of
               scores per chunk), then torch: the excluded cells and column 0 set to NaN (their index tensors are built outside the
               timed region), the target's score put back, compare against it with the tie rule, two sums
  dense_ms     the pair_score_dense calls of that composition alone (the same chunks, nothing done with the scores)
  topk128_ms   functional.pair_score_topk(k = 128) over the same rows and lists, for scale: the deepest list topk can give
The ranks and candidate counts of both paths are asserted equal before anything is timed.  Device events around blocks of --iters
calls after --warmup calls of every path; the paths alternate block by block and the medians over --repeats blocks are
reported (with min / max).  valu_floor_ms is 3 lane-operations per (pair, item, k) at 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9        # unpacked fp32 lane-operations per second (tools/bench_recommend.py)
DEV = "cuda:0"


def timed_blocks(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}: per repeat one block of `iters` calls of each path in turn, device events around
    each block."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def make_problem(U, I, K, B, per_user, seed):
    gen = torch.Generator().manual_seed(seed)
    ul, il = torch.randn(U, K, generator=gen), torch.randn(I, K, generator=gen)
    h, g = torch.randn(K, 1, generator=gen), torch.randn(1, generator=gen)
    ub, ib = torch.randn(U, 1, generator=gen), torch.randn(I, 1, generator=gen)
    u_ids = torch.randint(1, U, (B,), generator=gen)
    i_ids = torch.randint(1, I, (B,), generator=gen)
    # per user a sorted, duplicate-free list of 0 .. 2 * per_user rated items
    counts = torch.randint(0, 2 * per_user + 1, (U,), generator=gen)
    counts[0] = 0
    owner = torch.repeat_interleave(torch.arange(U), counts)
    cells = torch.unique(owner * I + torch.randint(1, I, (int(counts.sum()),), generator=gen))      # sorted by (user, item)
    off = torch.zeros(U + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(cells // I, minlength=U), 0)
    return ul, il, h, g, ub, ib, u_ids, i_ids, off, (cells % I).to(torch.int32)


def composed_rank(RF, rows, il, h, g, ub_rows, ib, tgt, item_lo, chunks):
    """Ranks from the dense scores, `chunks` = [(a, b, excluded cell rows, excluded cell items)]."""
    Ni = il.shape[0]
    ids = torch.arange(Ni, device=rows.device)[None, :]
    rank, n_cand = [], []
    for a, b, er, ei in chunks:
        s = RF.pair_score_dense("fm", rows[a:b], il, h, g, ub_rows[a:b], ib)
        t = tgt[a:b, None]
        ts = s.gather(1, t)
        s[er, ei] = float("nan")
        s[:, :item_lo] = float("nan")
        s.scatter_(1, t, ts)                                   # the target is never excluded
        rank.append(((s > ts) | ((s == ts) & (ids < t))).sum(1))      # a NaN compares false: no candidate
        n_cand.append((s == s).sum(1))
    return torch.cat(rank).to(torch.int32), torch.cat(n_cand).to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--budget", type=int, default=1 << 28, help="bytes of dense scores per chunk of the composition")
    ap.add_argument("--limit", type=int, default=540, help="seconds after which the process ends itself")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_eval.py needs an MI355X: there is no CPU fallback and no CPU timing")
    signal.alarm(a.limit)
    from review_based_recommender_amd import _lib, functional as RF
    U, I, K, B, item_lo = 50001, 50001, 50, 4096, 1
    ul, il, h, g, ub, ib, u_ids, i_ids, off, items = [t.to(DEV) for t in make_problem(U, I, K, B, 20, seed=0)]
    rows, ub_rows = RF.embedding(ul, u_ids, None), RF.embedding(ub, u_ids, None)
    excl = (off, items, u_ids)
    step = max(1, min(B, a.budget // (I * 4)))
    chunks = []
    for lo in range(0, B, step):
        u = u_ids[lo:lo + step]
        n = off[u + 1] - off[u]
        er = torch.repeat_interleave(torch.arange(u.numel(), device=DEV), n)
        start = torch.repeat_interleave(off[u] - (torch.cumsum(n, 0) - n), n)
        chunks.append((lo, min(lo + step, B), er, items[start + torch.arange(er.numel(), device=DEV)].long()))

    fused = lambda: RF.pair_score_rank("fm", rows, il, i_ids, h, g, ub_rows, ib, item_lo=item_lo, exclude=excl)       # noqa: E731
    composed = lambda: composed_rank(RF, rows, il, h, g, ub_rows, ib, i_ids, item_lo, chunks)                         # noqa: E731
    dense = lambda: [RF.pair_score_dense("fm", rows[lo:hi], il, h, g, ub_rows[lo:hi], ib) for lo, hi, _, _ in chunks]      # noqa: E731
    topk = lambda: RF.pair_score_topk("fm", rows, il, 128, h, g, ub_rows, ib, item_lo=item_lo, exclude=excl)          # noqa: E731
    (fr, fc), (cr, cc) = fused(), composed()
    torch.cuda.synchronize()
    RF.check_id_errors(DEV)
    assert torch.equal(fr, cr) and torch.equal(fc, cc), (
        f"fused and composed ranks differ in {int((fr != cr).sum())} pairs, candidate counts in {int((fc != cc).sum())}")
    ms = timed_blocks({"fused": fused, "composed": composed, "dense": dense, "topk128": topk}, a.iters, a.warmup, a.repeats)
    floor_ms = 3.0 * B * (I - item_lo) * K / LANE_OPS_PER_S * 1e3
    res = {"bench": "rank_eval", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"U": U, "I": I, "K": K, "B": B, "mode": "fm", "excluded_per_pair_mean": round(sum(c[2].numel() for c in chunks) / B, 2),
                     "composition_chunks": len(chunks)},
           "ranks_equal": True, "mean_rank": round(float(fr.double().mean()), 1)}
    for name, (med, lo, hi) in ms.items():
        res[f"{name}_ms"] = round(med, 4)
        res[f"{name}_ms_min_max"] = [round(lo, 4), round(hi, 4)]
    res["composed_over_fused"] = round(ms["composed"][0] / ms["fused"][0], 2)
    res["topk128_over_fused"] = round(ms["topk128"][0] / ms["fused"][0], 2)
    res["valu_floor_ms"] = round(floor_ms, 4)
    res["fused_floor_fraction"] = round(floor_ms / ms["fused"][0], 4)
    res["fused_ws_bytes"] = int(_lib.lib().rbr_pair_score_rank_ws_bytes(B, I, K))
    res["composed_score_bytes"] = B * I * 4
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
