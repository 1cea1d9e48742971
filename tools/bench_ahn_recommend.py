"""AHN's query surface over cached sentence tables (recommend.AhnRecommender, csrc/ahn_pair.hip) against what scoring an AHN pair
costs without it, on the same GPU and the same synthetic catalogue, as one JSON line.

    timeout -k 10 900 python tools/bench_ahn_recommend.py [--repeats 5] [--iters 5] [--warmup 2] [--limit 840] [--out FILE]

Shape: the reference's default config (models/ahn/default_ahn.json: 10 reviews x 10 sentences x 20 words per side, E = H = 300,
k = 10), a 1001 x 1001 catalogue (id 0 = padding) of seeded random reviews, V = 20000; about one sentence in 21 is empty.
Device events, medians over --repeats blocks of --iters calls after --warmup calls (refresh: --repeats single calls):
  refresh_ms            AhnRecommender.refresh(): the encoder over all 2002 ids and the state tables
  score_256_ms          score() of 256 random pairs
  score_all_32_ms       score_all() of 32 users: 32 x 1001 scores
  topk_32_k10_ms        topk(k = 10) of 32 users (score_all + the torch selection)
  kernel_*_ms, *_tflops the C-ABI call alone (event pairs around it), with 2 * P * RuSu * RiSi * F over the time and its share of
                        the f32 matrix peak (157.3 TFLOP/s)
  aggregate_256_ms      (a) AHN.aggregate in torch on sentence vectors gathered from the SAME cached tables, the same 256 pairs
  forward_256_ms        (b) AHN.forward on plain-gathered batches of 32 pairs, 8 of them: what anyone runs today
  table_mb              bytes of the state tables
  max_abs_diff_*        score() against (a) and against (b) on those pairs
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json
import os

import torch

from benchlib import arm, parser, quiet, rounded_ms as timed_ms

DEV = "cuda:0"
RV, SN, WN, E, K = 10, 10, 20, 300, 10
N_IDS, V = 1001, 20000
F32_MATRIX_PEAK_TFLOPS = 157.3


def main():
    ap = parser(__doc__, repeats=5, iters=5, warmup=2, limit=840)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    arm("bench_ahn_recommend.py", a.limit)
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.recommend import AhnRecommender

    g = torch.Generator().manual_seed(23)

    def table():
        lens = torch.randint(0, WN + 1, (N_IDS, RV, SN), generator=g)
        lens[1, 0, 0] = WN                                                   # the table's longest sentence is a full one
        t = torch.randint(1, V, (N_IDS, RV, SN, WN), generator=g) * (torch.arange(WN) < lens.unsqueeze(-1))
        t[0] = 0
        return t.to(torch.int32).to(DEV)

    user, item = table(), table()
    model = quiet(AHN, E, E, K, N_IDS, N_IDS, V, None, rnn_dropout=0.0, dropout=0.5, item_review_num=RV).to(DEV).eval()
    rec = AhnRecommender(model, user=user, item=item)
    res = {"bench": "ahn_recommend", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"users": N_IDS, "items": N_IDS, "reviews": RV, "sentences": SN, "words": WN, "F": E, "K": K}}
    res["refresh_ms"], res["refresh_ms_min"], res["refresh_ms_max"] = timed_ms(lambda: rec.refresh(), 1, 1, a.repeats)
    res["table_mb"] = round(sum(t.numel() * t.element_size() for st in (rec.user_state, rec.item_state) for t in st) / 2 ** 20, 1)

    pu = torch.randint(1, N_IDS, (256,), generator=g).to(DEV)
    pi = torch.randint(1, N_IDS, (256,), generator=g).to(DEV)
    pu[0], pi[0] = 1, 1                                                      # every plain-gathered batch of 32 holds a full sentence
    for b in range(1, 8):
        pu[32 * b], pi[32 * b] = 1, 1
    u32 = torch.arange(1, 33, device=DEV)
    queries = (("score_256_ms", lambda: rec.score(pu, pi)), ("score_all_32_ms", lambda: rec.score_all(u32)),
               ("topk_32_k10_ms", lambda: rec.topk(u32, 10)))
    for name, fn in queries:
        res[name], res[name + "_min"], res[name + "_max"] = timed_ms(fn, a.iters, a.warmup, a.repeats)

    # the kernel alone
    for key, fn, pairs in (("ahn_pair_score_ids", queries[0][1], 256), ("ahn_pair_score_dense", queries[1][1], 32 * N_IDS)):
        _lib.TIMER.start()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        _lib.TIMER.stop()
        ms = _lib.TIMER.summary()[key][1]
        tflops = 2.0 * pairs * (RV * SN) * (RV * SN) * E / (ms * 1e-3) / 1e12
        short = "kernel_ids_256" if pairs == 256 else "kernel_dense_32"
        res[short + "_ms"], res[short + "_tflops"] = round(ms, 4), round(tflops, 2)
        res[short + "_share_of_f32_matrix_peak"] = round(tflops / F32_MATRIX_PEAK_TFLOPS, 4)

    # (a) the torch composition on sentence vectors from the same tables
    us, its = rec.user_state, rec.item_state
    usm, urm = us.sent_masks, us.rev_masks
    ilen, ism, irm = D.sentence_masks(item, 0)

    def aggregate():
        with RF.eval_mode(model):
            return model.aggregate(us.X.index_select(0, pu).view(256, RV, SN, E), ys.index_select(0, pi), usm.index_select(0, pu),
                                   ism.index_select(0, pi), urm.index_select(0, pu), irm.index_select(0, pi), pu, pi)[0]

    with RF.eval_mode(model):            # the item side's sentence vectors are not part of the state: encode them once for (a)
        t_out = RF.lstm_t_out(ilen.reshape(-1), WN)
        ys = torch.cat([model._encode_side(item[a0:a0 + 32].to(torch.int64), ilen[a0:a0 + 32], t_out) for a0 in range(0, N_IDS, 32)])
    res["aggregate_256_ms"], res["aggregate_256_ms_min"], res["aggregate_256_ms_max"] = timed_ms(aggregate, a.iters, a.warmup, a.repeats)

    # (b) the whole forward on plain-gathered batches
    def batch(lo):
        u, i = pu[lo:lo + 32], pi[lo:lo + 32]
        ur, ir = user.index_select(0, u).to(torch.int64), item.index_select(0, i).to(torch.int64)
        ul, um, uM = D.sentence_masks(ur, 0)
        il, im, iM = D.sentence_masks(ir, 0)
        return ur, ir, um, im, ul, il, uM, iM, u, i

    def forward():
        with RF.eval_mode(model):
            return torch.cat([model(*batch(lo))[0] for lo in range(0, 256, 32)])

    res["forward_256_ms"], res["forward_256_ms_min"], res["forward_256_ms_max"] = timed_ms(forward, a.iters, a.warmup, a.repeats)
    score = rec.score(pu, pi)
    res["max_abs_diff_aggregate"] = float((score - aggregate()).abs().max())
    res["max_abs_diff_forward"] = float((score - forward()).abs().max())
    res["aggregate_over_score"] = round(res["aggregate_256_ms"] / res["score_256_ms"], 3)
    res["forward_over_score"] = round(res["forward_256_ms"] / res["score_256_ms"], 3)
    RF.check_id_errors(DEV)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
