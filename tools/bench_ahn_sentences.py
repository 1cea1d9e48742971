"""AhnRecommender.sentences and its op (csrc/ahn_explain.hip) against the score launch on the same pairs and against the
composition a user could write without the op, on the same GPU and the same synthetic catalogue, as one JSON line.

    timeout -k 10 600 python tools/bench_ahn_sentences.py [--repeats 5] [--iters 10] [--warmup 3] [--limit 540] [--out FILE]

Shape: the reference's default config (models/ahn/default_ahn.json: 10 reviews x 10 sentences x 20 words per side, E = H = 300,
k = 10), a 1001 x 1001 catalogue (id 0 = padding) of seeded random reviews, V = 20000 -- tools/bench_ahn_recommend.py's -- and 256
random pairs.  Device events, medians over --repeats blocks of --iters calls after --warmup calls:
  sentences_ms       one AhnRecommender.sentences(u_ids, i_ids) call (the id check, the op, two row gathers, two casts)
  op_ms              functional.ahn_pair_explain alone: one launch
  score_ms           functional.ahn_pair_score on the same pairs in the same run: one launch
  composed_ms        the same numbers without the op: functional.ahn_pair_attend on the pairs' gathered rows, a torch FM over the
                     hoisted rows, autograd.grad down to dX, dXt [P, Ru*Su, F], dKs [P, Ri*Si, F], dKr [P, Ri, F], and row dots
                     (tests/ahn_explain_ref.explain_torch with the HIP op in place of the torch attention)
  op_over_score, composed_over_op   the two ratios of that one run
  max_abs_diff       the op against the composition over the eight contribution tensors, beside the largest |value|
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import torch

from benchlib import arm, parser, quiet, rounded_ms as timed_ms

import ahn_explain_ref as E_REF  # noqa: E402  (benchlib set the path)

DEV = "cuda:0"
RV, SN, WN, E, K = 10, 10, 20, 300, 10
N_IDS, V, PAIRS = 1001, 20000, 256


def main():
    ap = parser(__doc__, repeats=5, iters=10, warmup=3, limit=540)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    arm("bench_ahn_sentences.py", a.limit)
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
    rec = AhnRecommender(model, user=user, item=item).refresh()
    pu = torch.randint(1, N_IDS, (PAIRS,), generator=g).to(DEV)
    pi = torch.randint(1, N_IDS, (PAIRS,), generator=g).to(DEV)
    us, its, head = rec.user_state, rec.item_state, rec.head
    extra = RF.AhnExplainRows(rec.item_rows, *rec.explain_head)

    sentences = lambda: rec.sentences(pu, pi)                                            # noqa: E731
    op = lambda: RF.ahn_pair_explain(us, its, head, extra, pu, pi)                       # noqa: E731
    score = lambda: RF.ahn_pair_score(us, its, head, pu, pi)                             # noqa: E731

    # the composition: the pairs' rows gathered once (not timed), then attend + FM + autograd.grad + dots per call
    t = dict(X=us.X.index_select(0, pu), Xt=us.Xt.index_select(0, pu), sent_mask=us.sent_masks.index_select(0, pu),
             rev_mask=us.rev_masks.index_select(0, pu), Ks=its.Ks.index_select(0, pi), Kr=its.Kr.index_select(0, pi), bt=head.bt)
    h = dict(ufm=us.fm.index_select(0, pu), ifm=its.fm.index_select(0, pi), VzT=head.VzT, vz2=head.vz2, lz=head.lz, lin_b=head.lin_b,
             Rp=extra.Rp.index_select(0, pi), beta=its.item_review_weights.index_select(0, pi), VqT=extra.VqT, vq2=extra.vq2, lq=extra.lq)
    attend = lambda X, Xt, m, M, Ks, Kr, bt, G: RF.ahn_pair_attend(X, Xt, m, M, Ks, Kr, bt, groups=G)       # noqa: E731
    composed = lambda: E_REF.explain_torch(t, h, 1, attend=attend)                       # noqa: E731

    got, want = op(), composed()
    torch.cuda.synchronize()
    diff = max(float((getattr(got, k) - want[k].view_as(getattr(got, k))).abs().max()) for k in E_REF.FIELDS)
    big = max(float(getattr(got, k).abs().max()) for k in E_REF.FIELDS)
    res = {"bench": "ahn_sentences", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"pairs": PAIRS, "users": N_IDS, "items": N_IDS, "reviews": RV, "sentences": SN, "words": WN, "F": E, "K": K}}
    for name, fn, iters in (("sentences_ms", sentences, a.iters), ("op_ms", op, a.iters), ("score_ms", score, a.iters),
                            ("composed_ms", composed, max(1, a.iters // 2))):
        res[name], res[name + "_min"], res[name + "_max"] = timed_ms(fn, iters, a.warmup, a.repeats)
    res["op_over_score"] = round(res["op_ms"] / res["score_ms"], 3)
    res["composed_over_op"] = round(res["composed_ms"] / res["op_ms"], 2)
    res["score_bits_equal"] = bool(torch.equal(got.score, score()))
    res["max_abs_diff"], res["max_abs_value"] = diff, big
    res["item_rows_mb"] = round(rec.item_rows.numel() * 4 / 2 ** 20, 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
