"""CPU-only checks of the held-out rank evaluation (rbr_pair_score_rank, functional.pair_score_rank, recommend.rank_metrics, the
CLI's --eval-split, the trainer's rank_metrics key): the metric formulas against hand-written values, argument validation before
any device call, the command line and the HIP-device gate.  No kernel is launched."""
import json
import math

import pytest
import torch

import make_dataset

BAD_ARG, UNSUPPORTED = -1, -2
P = 0x1000        # a non-NULL pointer that is never dereferenced: every check below fails before the first device call
TOL = 1e-12       # float64 sums of a handful of terms


def _close(got, want):
    return got is not None and abs(got - want) <= TOL


def test_rank_metrics_against_hand_written_values():
    from review_based_recommender_amd.recommend import rank_metrics
    rank = torch.tensor([0, 1, 9, 10, -1], dtype=torch.int32)
    n_cand = torch.tensor([11, 11, 11, 11, 11], dtype=torch.int32)
    m = rank_metrics(rank, n_cand, (1, 10))
    assert list(m) == ["hr@1", "ndcg@1", "hr@10", "ndcg@10", "mrr", "auc", "mean_rank", "n", "unranked"]
    assert _close(m["hr@1"], 1 / 5) and _close(m["ndcg@1"], 1 / 5)
    assert _close(m["hr@10"], 3 / 5)                                       # rank 10 is the 11th place: outside the first 10
    assert _close(m["ndcg@10"], (1 + 1 / math.log2(3) + 1 / math.log2(11)) / 5)
    assert _close(m["mrr"], (1 + 1 / 2 + 1 / 10 + 1 / 11 + 0) / 5)         # the unranked pair counts as 0
    assert _close(m["auc"], (1 + 0.9 + 0.1 + 0) / 4)                       # over the four ranked pairs
    assert _close(m["mean_rank"], 20 / 4)
    assert (m["n"], m["unranked"]) == (5, 1)
    # int64 input and a [B, 1] shape are the same pairs
    assert rank_metrics(rank.long().view(-1, 1), n_cand.long().view(-1, 1), [1, 10]) == m


def test_rank_metrics_leaves_single_candidate_pairs_out_of_auc_and_takes_empty_input():
    from review_based_recommender_amd.recommend import rank_metrics
    # the second pair's item is its only candidate: rank 0, a hit everywhere, but no other candidate to be ahead of
    m = rank_metrics(torch.tensor([2, 0]), torch.tensor([5, 1]), (1,))
    assert _close(m["auc"], 1 - 2 / 4) and _close(m["hr@1"], 1 / 2) and _close(m["mrr"], (1 / 3 + 1) / 2)
    assert _close(m["mean_rank"], 1.0) and (m["n"], m["unranked"]) == (2, 0)
    only = rank_metrics(torch.tensor([0]), torch.tensor([1]), (3,))
    assert only["auc"] is None and _close(only["hr@3"], 1.0)
    unranked = rank_metrics(torch.tensor([-1, -1]), torch.tensor([7, 7]), (3,))
    assert unranked["hr@3"] == 0.0 and unranked["mrr"] == 0.0 and unranked["auc"] is None and unranked["mean_rank"] is None
    assert unranked["unranked"] == 2
    empty = rank_metrics(torch.empty(0, dtype=torch.int32), torch.empty(0, dtype=torch.int32), (5, 10))
    assert (empty["n"], empty["unranked"]) == (0, 0)
    assert all(empty[k] is None for k in ("hr@5", "ndcg@5", "hr@10", "ndcg@10", "mrr", "auc", "mean_rank"))
    json.dumps(empty)                                                      # None, not NaN: the CLI's line stays JSON
    with pytest.raises(ValueError):
        rank_metrics(torch.tensor([0]), torch.tensor([3]), (0,))
    with pytest.raises(ValueError):
        rank_metrics(torch.tensor([0, 1]), torch.tensor([3]), (1,))


def test_rank_workspace_query():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    for B, Ni in ((1, 2), (4096, 50001), (257, 1003), (1, 1 << 30), (1 << 20, 3)):
        ws = L.rbr_pair_score_rank_ws_bytes(B, Ni, 50)
        assert 0 < ws <= B * 8 * 64 and ws % (B * 8) == 0, (B, Ni)
    assert L.rbr_pair_score_rank_ws_bytes(4096, 50001, 50) <= 4096 * 50001 * 4 // 1024        # nothing like the [B, Ni] matrix
    for shape in ((0, 10, 8), (-1, 10, 8), (4, 0, 8), (4, 10, 0)):
        assert L.rbr_pair_score_rank_ws_bytes(*shape) == 0, shape
        assert b"bad shape" in L.rbr_last_error()
    assert L.rbr_pair_score_rank_ws_bytes(4, 10, 4097) == 0
    assert b"4097" in L.rbr_last_error()


def _rank(L, mode=0, B=4, Ni=10, K=8, item_lo=1, ul=P, il=P, h=P, g=P, ub=P, ib=P, tgt=P, off=None, items=None, nnz=0, rows=None,
          n_rows=0, rank=P, n_cand=P, err=None, ws=P):
    return L.rbr_pair_score_rank(mode, B, Ni, K, item_lo, ul, il, h, g, ub, ib, tgt, off, items, nnz, rows, n_rows, rank, n_cand, err,
                                 ws, None)


@pytest.mark.parametrize("kw,code", [
    (dict(ul=None), BAD_ARG), (dict(il=None), BAD_ARG), (dict(h=None), BAD_ARG), (dict(g=None), BAD_ARG), (dict(tgt=None), BAD_ARG),
    (dict(B=0), BAD_ARG), (dict(B=-3), BAD_ARG), (dict(Ni=0), BAD_ARG), (dict(K=0), BAD_ARG), (dict(K=4097), UNSUPPORTED),
    (dict(item_lo=10), BAD_ARG), (dict(item_lo=-1), BAD_ARG),
    (dict(off=P), BAD_ARG), (dict(items=P), BAD_ARG), (dict(nnz=4), BAD_ARG), (dict(off=P, items=P, nnz=-1), BAD_ARG),
    (dict(rows=P, n_rows=4), BAD_ARG), (dict(off=P, items=P, rows=P, n_rows=0), BAD_ARG),
    (dict(rank=None), BAD_ARG), (dict(n_cand=None), BAD_ARG), (dict(ws=None), BAD_ARG), (dict(mode=2), BAD_ARG),
    (dict(mode=1, h=None, g=None, ub=None, ib=None, item_lo=10), BAD_ARG),        # the dot mode needs no head, and still validates
])
def test_rank_refuses_bad_arguments_before_touching_a_device(kw, code):
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    assert _rank(L, **kw) == code, kw
    assert len(L.rbr_last_error()) > 0


def test_rank_refuses_cpu_tensors():
    from review_based_recommender_amd import functional as RF
    ul, il = torch.zeros(3, 4), torch.zeros(5, 4)
    h, g = torch.zeros(4, 1), torch.zeros(1)
    tgt = torch.tensor([1, 2, 3])
    for call in (lambda: RF.pair_score_rank("fm", ul, il, tgt, h, g),
                 lambda: RF.pair_score_rank("dot", ul, il, tgt),
                 lambda: RF.pair_score_rank("dot", ul[:0], il, tgt[:0])):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(ValueError):
        RF.pair_score_rank("cosine", ul, il, tgt)


BASE = ["--model", "deepconn", "--config", "c", "--checkpoint", "m"]


def test_cli_eval_arguments():
    from review_based_recommender_amd.recommend import parse_cli
    a = parse_cli(BASE + ["--eval-split", "valid", "--ks", "5,10", "--exclude-train", "--metrics-out", "m.json"])
    assert (a.eval_split, a.ks, a.metrics_out, a.out, a.exclude_train) == ("valid", (5, 10), "m.json", None, True)
    b = parse_cli(BASE + ["--eval-split", "test"])
    assert (b.eval_split, b.ks, b.metrics_out, b.out) == ("test", (5, 10, 20), None, None)
    c = parse_cli(BASE + ["--eval-split", "test", "--out", "recs.jsonl", "--ks", "1"])        # lists and metrics in one run
    assert (c.out, c.ks) == ("recs.jsonl", (1,))
    d = parse_cli(BASE + ["--out", "recs.jsonl"])                                               # today's command line
    assert d.eval_split is None and d.out == "recs.jsonl"
    for bad in (BASE,                                                   # --out stays required without --eval-split
                BASE + ["--ks", "5", "--out", "o"], BASE + ["--metrics-out", "m.json", "--out", "o"],
                BASE + ["--eval-split", "train"], BASE + ["--eval-split", "valid", "--ks", "0"],
                BASE + ["--eval-split", "valid", "--ks", "5,-1"], BASE + ["--eval-split", "valid", "--ks", "5,x"],
                BASE + ["--eval-split", "valid", "--ks", ""], BASE + ["--eval-split", "valid", "--ks", "5,,10"],
                BASE + ["--eval-split", "valid", "--ks", str(2 ** 31)]):
        with pytest.raises(SystemExit):
            parse_cli(bad)


def test_trainer_refuses_rank_metrics_without_towers_or_with_parallel(tmp_path):
    """Both refusals come with the eval_from_towers check: before the dataset is read and before a device is asked for."""
    from review_based_recommender_amd import trainer
    assert trainer.DEFAULTS["rank_metrics"] == []
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)
    cfg = {"data_dir": data_dir, "model_name": "deepconn", "device_cache": True, "eval_from_towers": True, "rank_metrics": [5]}
    for change, text in ((dict(eval_from_towers=False), "rank_metrics needs eval_from_towers"), (dict(parallel=True), "parallel"),
                         (dict(rank_metrics=[0]), "cut-offs"), (dict(rank_metrics="5,10"), "cut-offs")):
        with pytest.raises(ValueError, match=text):
            trainer.ReviewExperiment("deepconn", trainer.Args(dict(cfg, **change)), uid="bad")
