"""Trainer-equivalent entry point: the behaviour of the reference's
trainer/train_{deepconn_pp,narre,dual_att}.py on top of the HIP modules (plus `--model simple_siamese` on the review
split: plain Adam, none of train_simple_siamese.py's SparseAdam / scheduler; its review sampling is `sample_train_review`).

    python -m review_based_recommender_amd.trainer --model deepconn --config cfg.json
    python -m torch.distributed.run --nproc-per-node 8 -m review_based_recommender_amd.trainer --model deepconn --config cfg.json

Kept from the reference: the flat JSON config keys (models/*/default_*.json), output directory
`./{log_dir}/{dataset}/{model_name}/{uid}` with `log.txt` (experiment.py:64-83), the args / parameter
tables (experiment.py:101-123), the step (train_deepconn_pp.py:161-168), the log line
`epoch: e/E, step: s/S, loss: ..., rmse: ..., lr: ..., gnorm: ..., time: ...` every `log_idx` steps
(:176-184), validation RMSE with best-model checkpoint `{"model","optimizer","updates","args"}`
(experiment.py:127-139, train_deepconn_pp.py:214-217) and patience early stop by raising `EarlyStop`
(:226-232).  Deliberate differences: `kernel_sizes` / `hidden_dim` come from the config unless
`--reference-quirks` restores the trainers' hard-coded `[3]` / 150 (train_deepconn_pp.py:125,
train_narre.py:124-125); `parallel: true` means one process per GPU with an RCCL gradient all-reduce
(launch with torch.distributed.run) instead of nn.DataParallel -- with nn.DataParallel's semantics: `batch_size` is the
GLOBAL batch, split evenly over the ranks (train_deepconn_pp.py:130 scatters each batch over the GPUs), every epoch
draws a new permutation (sampler.set_epoch), and validation shards the examples without padding so each one counts
once in the all-reduced RMSE; running loss / gnorm are accumulated on
the device and read back only at log lines (the reference calls loss.item() twice per step); the config key
`fast_step: true` switches to HipClipAdam and hipGraph replay of the step (train_step.py); `device_cache: true` (DeepCoNN++ and
D-ATT) keeps meta.pkl's documents on the GPU and feeds the step (u_id, i_id, rating) batches whose documents are gathered
there (data.DeviceDocCache; the loaders check once that every example's documents are meta's for its ids); `eval_from_towers:
true` (with device_cache) validates from latent tables: every user / item document is encoded once per validation pass and a
pair is scored from two table rows (recommend.Recommender), instead of both documents being encoded for every pair;
`rank_metrics: [10]` (with eval_from_towers, one process) also ranks every validation pair's item among all items the user has
not rated in the training split and logs `valid hr@10: ..., ndcg@10: ..., mrr: ...` after the RMSE line, which, like best-model
selection and early stopping, is unchanged;
`device_reviews: true` (NARRE and SimpleSiamese) is the review split's counterpart of device_cache: meta.pkl's reviews stay on the
GPU (data.DeviceReviewCache), the loaders ship (u_id, i_id, rating) and one launch rebuilds the batch -- training examples with
the pair's own review left out, validation examples plain (the loaders check once that every example is what that rule gives
for its ids); eval_from_towers works on top of it;
`sample_train_review: true` (with device_reviews, one process; `u_rv_num` / `i_rv_num` default rv_num, `review_pool` default rv_num,
`review_sample_seed` default `seed`) is train_simple_siamese.py:346-368 inside that launch: every training batch keeps a fresh
uniform random subset of u_rv_num / i_rv_num of each example's non-empty reviews, in random order, in rv_num slots with an empty
tail (data.SampledReviewFeed); the subset is drawn from the id's first review_pool (<= 63) reviews less the pair's own, so a pool
above rv_num lets reviews that truncation drops reach training.  Validation batches stay plain.  The draw is counter-based --
fixed by (review_sample_seed, step, row) -- where the reference uses numpy's global generator;
`loss: "bpr"` (with device_cache or device_reviews, one process; `n_neg: 1`, `neg_seed` = `seed`) trains for ranking instead of
rating regression: every batch pair is joined by n_neg items its user has not rated in the training split, drawn on the device
(data.NegativeFeed), and the step minimises -log sigmoid(score(u, i+) - score(u, i-)) (train_step.BprObjective); the step log line
keeps its format with the BPR loss under `loss` (its `rmse` field is sqrt of the mean loss then, not an RMSE);
`select_by: "hr@K" | "ndcg@K" | "mrr"` (default "rmse"; K must be in rank_metrics; required with loss "bpr") makes best_model.pt
and `patience` follow that validation metric, higher is better, and the rank line ends in `best <metric>: ...`;
`loss: "softmax"` (same preconditions as "bpr"; `softmax_temperature: 1.0`, `logq_correction: false`; n_neg / neg_seed are
ignored) trains for ranking with the in-batch softmax: the batch stays the B observed pairs and every user's negatives are the other
items of the batch -- less the pad id, the pair's own item and the items the user has rated in the training split -- scored from
the towers' latent rows over all B x B pairs (data.InBatchFeed, train_step.InBatchSoftmaxObjective); logq_correction subtracts
log((count_i + 1) / (N + I)) of the training examples from item i's logit; the step log line keeps its format with the loss under
`loss`;
`neg_candidates: M` (1..64, default 1 = the uniform sampler, call for call; above 1 needs loss "bpr") is dynamic negative sampling:
every negative is the best-scoring of M uniform draws, scored on the device from the latent tables of the validation's
recommend.Recommender under the model's live head parameters (functional.sample_hard_negatives), and only the winner is encoded.
The tables are a snapshot: encoded once before the first training step and taken over from every validation pass's refresh for the
next epoch, and with `neg_refresh_steps: N` (default 0 = never) also re-encoded every N updates within an epoch; the feed keeps its
own copies (data.NegativeFeed.set_tables), so a recorded step stays valid across refreshes.  A small M is advised: the arg-max of
many candidates is often an item the user would rate well but has not rated in the training split.  The log format is unchanged.
`--model ahn` trains AHN (trainer/train_ahn.py) on the sentence split (data.SentenceDataset): the loader's 7-tuple goes to the device,
where the sentence lengths and the sentence / review masks of train_ahn.py:149-184 are derived from the tokens (data.sentence_masks);
`device_reviews: true` keeps meta.pkl's reviews on the GPU (data.DeviceSentenceCache) and one launch rebuilds a batch -- reviews,
lengths and masks -- from (u_id, i_id), leave-one-out for training, plain for validation; `fast_step` selects HipClipAdam but AHN's step
and eval forward run eagerly (no hipGraph is recorded, and one log line says so); device_cache, eval_from_towers, rank_metrics, a
`loss` other than "mse", sample_train_review and parallel are refused: AHN's sides attend to each other, so it has no per-id towers.
`ahn_tables: true` (--model ahn with device_reviews) opts into what AHN's asymmetry does allow -- the item side never looks at the
user, so every id has SENTENCE tables (recommend.AhnRecommender; about 240 KB per user and 120 KB per item in f32 at the default
shape: a deliberate memory opt-in, the bytes are logged once after the first refresh).  With it eval_from_towers validates from
those tables (refresh once per pass, then one launch of the fused pair tail per batch), rank_metrics / select_by rank every
validation pair's item from them (rank_metrics alone switches eval_from_towers on: AHN has no other way to rank), and `loss: "bpr"`
trains through AHN.forward_groups (train_step.AhnBprObjective over data.NegativeFeed): a step encodes B users and (1 + n_neg) * B
items instead of (1 + n_neg) * B of each, the user side's co-attention is one differentiable HIP op (functional.ahn_pair_attend),
and a user is represented by the observed pair's leave-one-out reviews for its negatives too (the AHN BPR rule, stated at
forward_groups).  Table scores follow the fixed-t_out rule of DESIGN.md 4.20: they can differ from the loader-fed validation where
a batch's longest sentence is shorter than the table's.  `fused_pair_tail: true` (with ahn_tables) runs the MSE step's user-side
co-attention on the same op (AHN.fused_tail).  Still refused for AHN, each with its reason: loss "softmax", neg_candidates > 1,
sample_train_review, parallel, device_cache; the step stays eager.
"""
from __future__ import annotations

import argparse
import datetime
import json
import math
import os
import time

import torch
import torch.nn as nn

from . import data as D
from . import functional as RF
from .train_step import GraphedForward, GraphedTrainStep, make_optimizer, train_step


class Args:
    """experiment.py:30-37 -- flat JSON -> attribute bag."""

    def __init__(self, cfg: dict):
        self.__dict__.update(cfg)


def parse_args(config_file: str) -> Args:
    with open(config_file) as f:
        return Args(json.load(f))


class EarlyStop(Exception):
    pass


DEFAULTS = dict(log_dir="logs", dataset="dataset", log=True, log_idx=500, verbose=False, parallel=False, epochs=64,
                batch_size=50, lr=0.002, max_grad_norm=5.0, patience=5, dropout=0.5, arch="CNN", use_pretrain=False,
                num_workers=0, fast_step=False, shuffle=True, seed=0, record_steps=False, device_cache=False, eval_from_towers=False,
                device_reviews=False, rank_metrics=[], loss="mse", n_neg=1, neg_seed=None, select_by="rmse",
                softmax_temperature=1.0, logq_correction=False, neg_candidates=1, neg_refresh_steps=0, sample_train_review=False,
                u_rv_num=None, i_rv_num=None, review_pool=None, review_sample_seed=None, ahn_tables=False, fused_pair_tail=False)

LOSSES = ("mse", "bpr", "softmax")


def _rank_metric_of(select_by):
    """("hr" | "ndcg", K) or ("mrr", None) for a rank-metric `select_by`, None for "rmse"; anything else is refused."""
    if select_by == "rmse":
        return None
    if select_by == "mrr":
        return "mrr", None
    name, _, k = str(select_by).partition("@")
    if name in ("hr", "ndcg") and k.isdigit() and int(k) >= 1 and str(int(k)) == k:
        return name, int(k)
    raise ValueError(f"select_by must be \"rmse\", \"hr@K\", \"ndcg@K\" or \"mrr\", got {select_by!r}")


def _feed_states(feed):
    """The device-resident call numbers (`state`) of an id feed and of the feeds it wraps (`.feed`), outermost first."""
    states = []
    while feed is not None:
        if hasattr(feed, "state"):
            states.append(feed.state)
        feed = getattr(feed, "feed", None)
    return states


class _ShardSampler(torch.utils.data.Sampler):
    """Validation shard of one rank: examples rank, rank + world, ... in order -- no padding, so every example is seen by
    exactly one rank (DistributedSampler(drop_last=False) repeats examples to even the shards out, which would count them
    twice in the all-reduced squared error)."""

    def __init__(self, n: int, rank: int, world: int):
        self.idx = list(range(rank, n, world))

    def __iter__(self):
        return iter(self.idx)

    def __len__(self):
        return len(self.idx)


def make_loaders(train_set, valid_set, args, rank: int, world: int):
    """(train_loader, valid_loader, train_sampler, valid_sampler, per-rank batch) with nn.DataParallel's semantics on
    `world` ranks: `args.batch_size` is the global batch (train_deepconn_pp.py:130 scatters it over the GPUs), the training
    sampler reshuffles every epoch once the caller runs set_epoch(epoch), validation is sharded without padding."""
    parallel = world > 1
    if parallel and args.batch_size % world:
        raise ValueError(f"batch_size {args.batch_size} does not split evenly over {world} ranks")
    rank_batch = args.batch_size // world if parallel else args.batch_size
    train_sampler = valid_sampler = None
    if parallel:
        train_sampler = torch.utils.data.distributed.DistributedSampler(
            train_set, num_replicas=world, rank=rank, shuffle=bool(args.shuffle), seed=int(args.seed), drop_last=True)
        valid_sampler = _ShardSampler(len(valid_set), rank, world)
    gen = torch.Generator().manual_seed(int(args.seed))
    train_loader = torch.utils.data.DataLoader(
        train_set, batch_size=rank_batch, shuffle=bool(args.shuffle) and train_sampler is None, sampler=train_sampler,
        collate_fn=train_set.collate_fn, num_workers=args.num_workers, drop_last=train_sampler is not None, generator=gen)
    valid_loader = torch.utils.data.DataLoader(
        valid_set, batch_size=rank_batch, shuffle=False, sampler=valid_sampler, collate_fn=valid_set.collate_fn,
        num_workers=args.num_workers)
    return train_loader, valid_loader, train_sampler, valid_sampler, rank_batch


def make_model(kind: str, a: Args, ds, quirks: bool = False):
    """The model of `kind` for the config `a` and the dataset `ds` (train_*.py build_model), on the CPU; also what
    recommend.py rebuilds before it loads a checkpoint."""
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "deepconn":
            from .models.deepconn.deepconn import DeepCoNNpp
            ks = [3] if quirks else a.kernel_sizes
            return DeepCoNNpp(user_size=ds.user_num, item_size=ds.item_num, vocab_size=ds.vocab_size, kernel_sizes=ks,
                              hidden_dim=a.hidden_dim, embedding_dim=a.embedding_dim, dropout=a.dropout,
                              latent_dim=a.latent_dim, doc_len=ds.doc_len, pretrained_embeddings=None, arch=a.arch)
        if kind == "narre":
            from .models.narre.narre import NARRE
            ks = [3] if quirks else a.kernel_sizes
            hd = 150 if quirks else a.hidden_dim
            return NARRE(user_size=ds.user_num, item_size=ds.item_num, vocab_size=ds.vocab_size, kernel_sizes=ks,
                         hidden_dim=hd, embedding_dim=a.embedding_dim, att_dim=a.att_dim, latent_dim=a.latent_dim,
                         max_doc_num=ds.rv_num, max_doc_len=ds.rv_len, dropout=a.dropout, word_padding_idx=0,
                         user_padding_idx=0, item_padding_idx=0, pretrained_embeddings=None, arch=a.arch)
        if kind == "simple_siamese":
            # trainer/train_simple_siamese.py:161-167 (keys of models/simple_siamese/defalut_simple_train.json)
            from .models.simple_siamese.simple_siamese import SimpleSiamese
            return SimpleSiamese(embedding_dim=a.embedding_dim, latent_dim=a.latent_dim, vocab_size=ds.vocab_size,
                                 user_size=ds.user_num, item_size=ds.item_num, pretrained_embeddings=None,
                                 freeze_embeddings=getattr(a, "freeze_embeddings", False), dropout=a.dropout,
                                 word_dropout=getattr(a, "word_dropout", 0.2),
                                 review_dropout=getattr(a, "review_dropout", 0.0),
                                 use_ui_bias=getattr(a, "use_ui_bias", True),
                                 latent_transform=getattr(a, "latent_transform", False))
        if kind == "ahn":
            # trainer/train_ahn.py:129-134 (keys of models/ahn/default_ahn.json)
            from .models.ahn.ahn_model import AHN
            return AHN(a.embedding_dim, a.hidden_dim, a.k_factor, user_size=ds.user_num, item_size=ds.item_num,
                       word_vocab_size=ds.vocab_size, pretrained_word_embeddings=None, rnn_dropout=a.rnn_dropout,
                       dropout=a.dropout, item_review_num=ds.rv_num)
        from .models.dual_att.dual_att import DualAtt
        return DualAtt(vocab_size=ds.vocab_size, doc_len=ds.doc_len, l_window_size=a.l_window_size,
                       l_out_size=a.l_out_size, g_out_size=a.g_out_size, emb_size=a.emb_size,
                       hidden_size_1=a.hidden_size_1, hidden_size_2=a.hidden_size_2, dropout=a.dropout,
                       pretrained_embeddings=None)


class ReviewExperiment:
    KINDS = ("deepconn", "narre", "dual_att", "simple_siamese", "ahn")

    def __init__(self, kind: str, args: Args, reference_quirks: bool = False, uid: str | None = None):
        if kind not in self.KINDS:
            raise ValueError(f"{kind} is not one of {self.KINDS}")
        for k, v in DEFAULTS.items():
            if not hasattr(args, k):
                setattr(args, k, v)
        if getattr(args, "use_pretrain", False):
            raise RuntimeError("use_pretrain needs gensim + a word2vec file (train_deepconn_pp.py:105-119): pass "
                               "pretrained rows through the model's `pretrained_embeddings` argument instead")
        if kind == "ahn":
            # AHN's two sides attend to each other from the sentences up: there is no per-id tower whose
            # latent row could be cached, ranked from or scored against a sampled negative
            # `ahn_tables` opts into what the asymmetry does allow: only the user side looks at the pair,
            # so per-id SENTENCE tables (recommend.AhnRecommender) validate and rank, and a BPR step encodes every user once
            no_towers = "AHN's sides attend to each other, so it has no per-id towers"
            tables = bool(args.ahn_tables)
            opt_in = "; \"ahn_tables\": true (with device_reviews) uses per-id sentence tables instead"
            refused = (("device_cache", bool(args.device_cache), "the sentence split's id feed is device_reviews"),
                       ("eval_from_towers", bool(args.eval_from_towers) and not tables, no_towers + " to validate from" + opt_in),
                       ("rank_metrics", bool(args.rank_metrics) and not tables, no_towers + " to rank a catalogue from" + opt_in),
                       ("loss", args.loss != "mse" and not tables, f"only \"mse\" is, got {args.loss!r}; the ranking losses score "
                        "their negatives from per-id towers, and " + no_towers + "; \"ahn_tables\": true (with device_reviews) "
                        "trains \"bpr\" with every user encoded once"),
                       ("loss", args.loss == "softmax" and tables, "the in-batch softmax scores all B x B pairs from latent rows, "
                        "and " + no_towers + " (\"bpr\" is available with ahn_tables)"),
                       ("neg_candidates", args.neg_candidates != 1 and tables, "the hard-negative sampler scores its candidates "
                        "from latent tables, and " + no_towers),
                       ("sample_train_review", bool(args.sample_train_review), "review sampling is not built for the sentence split"),
                       ("parallel", bool(args.parallel), "data-parallel AHN is not built"))
            for key, on, why in refused:
                if on:
                    raise ValueError(f"{key} is not available with --model ahn: {why}")
            if tables and not bool(args.device_reviews):
                raise ValueError("ahn_tables needs device_reviews: the per-id sentence tables are encoded from the reviews resident "
                                 "on the GPU (data.DeviceSentenceCache)")
            if bool(args.fused_pair_tail) and not tables:
                raise ValueError("fused_pair_tail needs ahn_tables: both opt into the HIP pair tail of csrc/ahn_attend.hip")
            if tables and args.rank_metrics:
                # AHN ranks from the sentence tables only, so asking for ranks IS asking for the table validation: the RMSE line
                # and the ranks then come from the same scores (the args table prints the key as it ends up)
                args.eval_from_towers = True
        elif bool(args.ahn_tables) or bool(args.fused_pair_tail):
            raise ValueError(f"ahn_tables / fused_pair_tail are valid for --model ahn, not {kind}: the other models have per-id "
                             "towers (eval_from_towers)")
        if bool(args.device_cache) and kind not in ("deepconn", "dual_att"):
            # the review split's training examples are not per-id data: the reference drops the target pair's own review from
            # the user's and the item's lists before truncating (preprocess/divide_and_create_example_word.py:263-285)
            raise ValueError(f"device_cache is valid for --model deepconn and dual_att, not {kind}: the review split's examples "
                             "are not per-id documents (its id feed is device_reviews)")
        if bool(args.device_reviews) and kind not in ("narre", "simple_siamese", "ahn"):
            raise ValueError(f"device_reviews is valid for --model narre, simple_siamese and ahn, not {kind}: the doc split's id "
                             "feed is device_cache")
        if bool(args.eval_from_towers) and not (bool(args.device_cache) or bool(args.device_reviews)):
            raise ValueError("eval_from_towers needs device_cache (--model deepconn or dual_att) or device_reviews (narre or "
                             "simple_siamese): validation then scores each pair from latent tables encoded once per epoch from "
                             "the per-id documents")
        if args.rank_metrics:
            ks = args.rank_metrics
            if not isinstance(ks, (list, tuple)) or any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in ks):
                raise ValueError(f"rank_metrics must be a list of cut-offs K >= 1, got {ks!r}")
            if not bool(args.eval_from_towers):
                raise ValueError("rank_metrics needs eval_from_towers: the validation pairs are ranked from the latent tables")
            if bool(args.parallel):
                raise ValueError("rank_metrics is not available with parallel: the ranks of the shards are not reduced over the "
                                 "processes")
        if args.loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {args.loss!r}")
        metric = _rank_metric_of(args.select_by)
        if metric is not None and (not args.rank_metrics or (metric[1] is not None and metric[1] not in args.rank_metrics)):
            raise ValueError(f"select_by {args.select_by!r} needs rank_metrics to contain "
                             f"{'a cut-off' if metric[1] is None else metric[1]}: the model is selected by a metric the "
                             "validation pass computes")
        if args.loss == "bpr":
            if isinstance(args.n_neg, bool) or not isinstance(args.n_neg, int) or args.n_neg < 1:
                raise ValueError(f"n_neg must be an integer >= 1, got {args.n_neg!r}")
            if not (bool(args.device_cache) or bool(args.device_reviews)):
                raise ValueError("loss \"bpr\" needs device_cache (--model deepconn or dual_att) or device_reviews (narre or "
                                 "simple_siamese): a negative's documents are gathered on the device by its id")
            if bool(args.parallel):
                raise ValueError("loss \"bpr\" is not available with parallel: the negative sampler and the pairwise step "
                                 "run in one process")
            if metric is None:
                raise ValueError("loss \"bpr\" needs a rank metric in select_by (\"hr@K\", \"ndcg@K\" or \"mrr\"): a "
                                 "pairwise loss does not fit ratings, so the validation RMSE cannot select the model")
        nc, nr = args.neg_candidates, args.neg_refresh_steps
        if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
            raise ValueError(f"neg_candidates must be an integer in [1, 64], got {nc!r}")
        if nc > 1 and args.loss != "bpr":
            raise ValueError(f"neg_candidates {nc} needs loss \"bpr\": the candidates are negatives of the pairwise step, and loss "
                             f"{args.loss!r} draws none")
        if isinstance(nr, bool) or not isinstance(nr, int) or nr < 0:
            raise ValueError(f"neg_refresh_steps must be an integer >= 0, got {nr!r}")
        if nr > 0 and nc == 1:
            raise ValueError(f"neg_refresh_steps {nr} needs neg_candidates > 1: the uniform sampler reads no latent tables")
        if args.loss == "softmax":
            t = args.softmax_temperature
            if isinstance(t, bool) or not isinstance(t, (int, float)) or not (0.0 < float(t) < math.inf):
                raise ValueError(f"softmax_temperature must be a positive number, got {t!r}")
            if not (bool(args.device_cache) or bool(args.device_reviews)):
                raise ValueError("loss \"softmax\" needs device_cache (--model deepconn or dual_att) or device_reviews (narre or "
                                 "simple_siamese): the all-pairs loss reads the batch's ids from the id feed")
            if bool(args.parallel):
                raise ValueError("loss \"softmax\" is not available with parallel: the item latents of the other processes' "
                                 "batches are not gathered")
            if metric is None:
                raise ValueError("loss \"softmax\" needs a rank metric in select_by (\"hr@K\", \"ndcg@K\" or \"mrr\"): a "
                                 "ranking loss does not fit ratings, so the validation RMSE cannot select the model")
        if bool(args.sample_train_review):
            if not bool(args.device_reviews):
                raise ValueError("sample_train_review needs device_reviews (--model narre or simple_siamese): the reviews are "
                                 "drawn inside the launch that rebuilds a batch from its ids")
            if bool(args.parallel):
                raise ValueError("sample_train_review is not available with parallel: every process would draw the same keys "
                                 "for its local rows")
            for name in ("u_rv_num", "i_rv_num", "review_pool"):
                v = getattr(args, name)
                if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
                    raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
            if args.review_pool is not None and args.review_pool > D.DeviceReviewCache.MAX_POOL:
                raise ValueError(f"review_pool must be at most {D.DeviceReviewCache.MAX_POOL}, got {args.review_pool}")
        self.select_metric = None if metric is None else args.select_by
        self.best_score = -math.inf          # the best select_by metric so far (higher is better); unused with "rmse"
        self.kind, self.args, self.quirks = kind, args, reference_quirks
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if not torch.cuda.is_available():
            raise RuntimeError("the HIP path needs an MI355X: there is no CPU fallback")
        torch.cuda.set_device(local_rank)
        self.device = torch.device("cuda", local_rank)
        self.uid = uid or datetime.datetime.now().strftime("%y%m%d_%H%M%S")
        self.updates = 0
        self.best_rmse = 1e3
        self.patience = 0
        self.grad_sync = None
        self._graphed_eval = None            # the recorded eval forward; False once the runtime has refused its capture
        self._towers = None                  # the one Recommender (_negative_towers)
        self._seen = None                    # the training split's seen-items CSR
        self._table_bytes_logged = False
        self.last_rank_metrics = None

        review_split = kind in ("narre", "simple_siamese", "ahn")
        cls = D.SentenceDataset if kind == "ahn" else D.ReviewDataset if review_split else D.DocDataset
        form = () if review_split else (kind == "deepconn",)      # DocDataset: do the loader's batches carry the ids (D-ATT's do not)
        kw = {"feed": "ids"} if args.device_cache or args.device_reviews else {}
        self.train_set = cls(args.data_dir, "train", *form, **kw)
        self.valid_set = cls(args.data_dir, "valid", *form, **kw)
        # device_cache: meta.pkl's documents resident on this GPU (train and valid share meta.pkl, so one cache serves both)
        self.cache = self.train_feed = self.eval_feed = None
        if args.device_cache:
            self.cache = D.DeviceDocCache(self.train_set, self.device)
            # what rebuilds a batch from its ids, in the model's form: D-ATT takes the documents only
            self.train_feed = self.eval_feed = self.cache.feed(kind != "dual_att")
        elif args.device_reviews and kind == "ahn":
            # the sentence split's reviews resident on this GPU: the same two rules, lengths and masks made by the same launch
            self.cache = D.DeviceSentenceCache(self.train_set, self.device)
            self.train_feed, self.eval_feed = self.cache.feed(True), self.cache.feed(False)
        elif args.device_reviews:
            # meta.pkl's reviews resident on this GPU; a train batch leaves each pair's own review out, a valid batch does not
            R = int(self.train_set.rv_num)
            sampling = bool(args.sample_train_review)
            if sampling:
                # counts and pool against the split's rv_num, before anything goes to the GPU
                for name in ("u_rv_num", "i_rv_num"):
                    if getattr(args, name) is not None and getattr(args, name) > R:
                        raise ValueError(f"{name} must be in [1, rv_num = {R}], got {getattr(args, name)}")
                if args.review_pool is not None and args.review_pool < R:
                    raise ValueError(f"review_pool must be in [rv_num = {R}, {D.DeviceReviewCache.MAX_POOL}], got {args.review_pool}")
            self.cache = D.DeviceReviewCache(self.train_set, self.device, pool=args.review_pool if sampling else None)
            self.train_feed, self.eval_feed = self.cache.feed(kind, True), self.cache.feed(kind, False)
            if sampling:
                seed = args.seed if args.review_sample_seed is None else args.review_sample_seed
                self.train_feed = self.cache.sampled_feed(kind, args.u_rv_num, args.i_rv_num, seed=int(seed))
        self.objective = None
        if args.loss == "bpr":
            # negatives are items the user has not rated in the training split: the same CSR the validation ranks against
            from .recommend import Recommender
            from .train_step import AhnBprObjective, BprObjective
            self._seen = Recommender.seen_from(self.train_set.examples, self.train_set.user_num, self.device)
            seed = args.seed if args.neg_seed is None else args.neg_seed
            n_items = (self.cache.item_table if kind == "ahn" else self.cache.item).shape[0]
            self.train_feed = D.NegativeFeed(self.train_feed, self._seen, n_items, n_neg=args.n_neg, seed=int(seed),
                                             n_cand=args.neg_candidates)
            # AHN: every user encoded once for its 1 + n_neg items (AHN.forward_groups), not once per expanded pair
            self.objective = AhnBprObjective(self.train_feed) if kind == "ahn" else BprObjective(self.train_feed)
        self._make_dir()
        self.build_model()
        if kind == "ahn" and bool(args.fused_pair_tail):
            self.model.fused_tail = True         # the MSE step's user-side co-attention on csrc/ahn_attend.hip
        if args.loss == "softmax":
            # false negatives are the items the user has rated in the training split: the CSR the validation ranks against
            from .recommend import Recommender
            from .train_step import InBatchSoftmaxObjective
            self._seen = Recommender.seen_from(self.train_set.examples, self.train_set.user_num, self.device)
            self.train_feed = D.InBatchFeed(self.train_feed, self._seen)
            logq = None
            if bool(args.logq_correction):      # log sampling probability of an item as a batch column, add-one smoothed; once, on the host
                n_items = self.cache.item.shape[0]
                counts = torch.bincount(torch.tensor([int(e[1]) for e in self.train_set.examples], dtype=torch.int64),
                                        minlength=n_items)[:n_items].double()
                logq = torch.log((counts + 1.0) / (counts.sum() + n_items)).float().to(self.device)
            self.objective = InBatchSoftmaxObjective(self.model, self.train_feed, temperature=float(args.softmax_temperature), logq=logq)
        # both splits were range-checked against their tables when they were loaded (data.validate_ranges): the per-forward
        # device-side check (one launch) is not needed on top
        self.model.validate_ids = False
        self.step_losses = [] if args.record_steps else None      # per-step training loss (device scalars), for tests
        self.step_gnorms = [] if args.record_steps else None      # and the gradient norm in front of the clip
        self.parallel = self.world > 1 and bool(args.parallel)
        (self.train_loader, self.valid_loader, self.train_sampler, self.valid_sampler,
         self.rank_batch) = make_loaders(self.train_set, self.valid_set, args, self.rank, self.world if self.parallel else 1)
        # fast_step: clip + Adam as two HIP launches and the whole step replayed as a hipGraph for full-size batches
        # (same update rule; see train_step.HipClipAdam / GraphedTrainStep)
        self.optimizer = make_optimizer(self.model, lr=args.lr, hip_clip_adam=bool(args.fast_step))
        self._graphed = None
        self._graphed_key = None
        # fast_step records the step and the eval forward as hipGraphs -- not for AHN, whose recorded step is not built: it keeps
        # HipClipAdam and runs eagerly
        self._record = bool(args.fast_step) and kind != "ahn"
        self.loss_func = nn.MSELoss()
        if self.parallel:
            from .distributed import GradAllReduce, broadcast_parameters, init_process_group_from_env
            init_process_group_from_env(os.environ.get("RBR_TRAINER_BACKEND", "nccl"))
            broadcast_parameters(self.model)
            self.grad_sync = GradAllReduce(self.model)
        self.print_args()
        self.print_model_stats()
        if bool(args.fast_step) and not self._record:
            self.print_write_to_log("fast_step: HipClipAdam only; the AHN step and eval forward are not recorded as hipGraphs "
                                    "(they run eagerly)")

    # ------------------------------------------------------------------ bookkeeping (experiment.py:64-123)
    def _make_dir(self):
        a = self.args
        self.out_dir = "./{}/{}/{}/{}".format(a.log_dir, a.dataset, a.model_name, self.uid)
        os.makedirs(self.out_dir, exist_ok=True)
        self.log_path = os.path.join(self.out_dir, "log.txt")

    def print_write_to_log(self, text: str):
        if self.rank != 0:
            return
        if self.args.log:
            try:
                with open(self.log_path, "a") as f:
                    f.write(text + "\n")
            except IOError:
                print("Cannot write a line into {}".format(self.log_path))
        print(text, flush=True)

    def print_args(self):
        for name, val in self.args.__dict__.items():
            self.print_write_to_log("{}: {}".format(name, val))
        self.print_write_to_log("=" * 50)

    def print_model_stats(self):
        self.print_write_to_log("List of all Trainable Variables")
        for i, (name, p) in enumerate(self.model.named_parameters()):
            if p.requires_grad:
                self.print_write_to_log("param {:3}: {:15} {}".format(i, str(tuple(p.shape)), name))
        n = sum(p.numel() for p in self.model.parameters())
        self.print_write_to_log("The total number of trainable parameters: {:,d}".format(n))
        self.print_write_to_log("=" * 50)

    def save(self, name: str):
        if self.rank != 0:
            return
        if not name.endswith(".pt"):
            name += ".pt"
        torch.save({"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(), "updates": self.updates,
                    "args": dict(self.args.__dict__)}, os.path.join(self.out_dir, name))

    # ------------------------------------------------------------------ model (train_*.py build_model)
    def build_model(self):
        self.model = make_model(self.kind, self.args, self.train_set, self.quirks)
        self.model.to(self.device)

    # ------------------------------------------------------------------ data
    def _to_device(self, batch):
        batch = [t.to(self.device, non_blocking=True) for t in batch]
        if self.kind == "simple_siamese":
            # review-split batch (u_revs, i_revs, word masks x2, ids x2, review ids x2, ratings) -> the model's arguments:
            # review masks mark the reviews that hold any token (simple_siamese/utils.py:94-106)
            u_revs, i_revs, u_wm, i_wm, u_ids, i_ids = batch[:6]
            return (u_revs, i_revs, u_wm, i_wm, u_wm.any(-1), i_wm.any(-1), u_ids, i_ids), batch[-1]
        if self.kind == "ahn":
            # sentence-split batch (u_revs, i_revs, ids x2, review ids x2, ratings) -> AHN's ten arguments: the sentence lengths
            # and the masks are derived here, on the device, from the tokens (train_ahn.py:197-202 does it on the host)
            u_revs, i_revs, u_ids, i_ids = batch[:4]
            (u_len, u_sm, u_rm), (i_len, i_sm, i_rm) = D.sentence_masks(u_revs), D.sentence_masks(i_revs)
            return (u_revs, i_revs, u_sm, i_sm, u_len, i_len, u_rm, i_rm, u_ids, i_ids), batch[-1]
        return tuple(batch[:-1]), batch[-1]

    # ------------------------------------------------------------------ loops (train_deepconn_pp.py:143-232)
    def train_one_epoch(self, epoch: int):
        a = self.args
        loader = self.train_loader
        if self.train_sampler is not None:
            self.train_sampler.set_epoch(epoch)          # a new permutation every epoch, the same one on every rank
        loss_sum = torch.zeros((), device=self.device)
        sq_err = torch.zeros((), device=self.device)
        gnorm = torch.zeros((), device=self.device)
        steps = count = 0
        start = time.time()
        self.model.train()
        hard = a.neg_candidates > 1
        if hard and self.train_feed.tables is None:
            self._refresh_negative_tables()              # before the first training step; later epochs use the validation's tables
        for i, batch in enumerate(loader):
            if hard and a.neg_refresh_steps > 0 and i > 0 and i % a.neg_refresh_steps == 0:
                self._refresh_negative_tables()
            staged = self._step_from_host(batch)
            if staged is not None:
                loss, gnorm, ratings = staged
            elif self.cache is not None:
                loss, gnorm, ratings = self._id_step(batch)
            else:
                inputs, ratings = self._to_device(batch)
                loss, gnorm = self._step(inputs, ratings)
            self.updates += 1
            if self.step_losses is not None:
                self.step_losses.append(loss.detach().clone())
                self.step_gnorms.append(gnorm.detach().clone())
            loss_sum += loss
            sq_err += loss * ratings.size(0)
            steps += 1
            count += ratings.size(0)
            if (i + 1) % a.log_idx == 0 and a.log:
                elapsed = (time.time() - start) / a.log_idx
                rmse = math.sqrt(float(sq_err) / count)       # the step's synchronisation point (the reference syncs every step)
                RF.check_id_errors(self.device)               # an id outside its table -> IndexError, as nn.Embedding raises
                self.print_write_to_log(
                    "epoch: {}/{}, step: {}/{}, loss: {:.3f}, rmse: {:.3f}, lr: {}, gnorm: {:3f}, time: {:.3f}".format(
                        epoch, a.epochs, i + 1, len(loader), float(loss_sum) / steps, rmse,
                        self.optimizer.param_groups[0]["lr"], float(gnorm), elapsed))
                loss_sum.zero_()
                sq_err.zero_()
                steps = count = 0
                start = time.time()

    def _step_from_host(self, batch):
        """`fast_step` with the recorded step in hand: a loader batch of the recorded shape goes host-to-device straight into
        the step's input block (GraphedTrainStep.stage) and the step is replayed -- no intermediate device tensors, no
        device-to-device copies.  None: not applicable (first batch, ragged batch, a model whose inputs are derived on the
        device), the caller takes the _to_device + _step route."""
        if not self._record or self._graphed is None or (self.kind == "simple_siamese" and self.cache is None):
            return None
        key = tuple((t.shape, t.dtype) for t in batch)
        if key != self._graphed_key:
            return None
        self._graphed.stage(0, tuple(batch[:-1]), batch[-1])
        loss, gnorm, _ = self._graphed(slot=0)
        return loss.clone(), gnorm.clone(), self._graphed.ratings

    def _replay(self, key, record, *batch):
        """`fast_step`: the step recorded for the batch shape `key` replayed on `batch` -- record() makes it at first use --, as
        (loss, gnorm) copies (the graph's outputs are overwritten by the next replay); None: a batch of another shape (the
        ragged last one), or graphs are off, and the caller steps eagerly."""
        if not self._record:
            return None
        if self._graphed is None:
            self._graphed, self._graphed_key = record(), key
        if key != self._graphed_key:
            return None
        loss, gnorm, _ = self._graphed(*batch)
        return loss.clone(), gnorm.clone()

    def _step(self, inputs, ratings):
        """One optimisation step; with `fast_step` the step recorded for this batch shape is replayed (a ragged last
        batch, or a batch of another shape, runs eagerly)."""
        a = self.args
        key = tuple((t.shape, t.dtype) for t in inputs) + ((ratings.shape, ratings.dtype),)
        done = self._replay(key, lambda: GraphedTrainStep(self.model, self.optimizer, inputs, ratings, a.max_grad_norm,
                                                          self.grad_sync), inputs, ratings)
        return done or train_step(self.model, self.optimizer, inputs, ratings, a.max_grad_norm, self.grad_sync)[:2]

    def _id_step(self, batch):
        """device_cache / device_reviews: one step on a (u_ids, i_ids, ratings) batch.  With `fast_step` the id-fed step recorded
        for this batch shape (gather + step) is replayed; otherwise, and for a ragged last batch, the documents are gathered
        eagerly and train_step runs on them."""
        a = self.args
        u_ids, i_ids, ratings = [t.to(self.device, non_blocking=True) for t in batch]

        def record():
            # recording runs warm-up steps: they must not use up the draws of the negative sampler or the review sampler
            states = _feed_states(self.train_feed)
            calls = [t.clone() for t in states]
            graphed = GraphedTrainStep.from_ids(self.model, self.optimizer, self.train_feed, u_ids, i_ids, ratings,
                                                a.max_grad_norm, self.grad_sync, objective=self.objective)
            for t, c in zip(states, calls):
                t.copy_(c)
            return graphed

        done = self._replay(tuple((t.shape, t.dtype) for t in batch), record, (u_ids, i_ids), ratings)
        if done is None:
            done = train_step(self.model, self.optimizer, self.train_feed.inputs(u_ids, i_ids), ratings, a.max_grad_norm,
                              self.grad_sync, objective=self.objective)[:2]
        return (*done, ratings)

    def _eval_forward(self, inputs, feed=None):
        """The eval forward of `inputs` -- the model's arguments, or with `feed` (device_cache / device_reviews) the batch's
        (u_ids, i_ids), gathered in front of it: replayed from a hipGraph for the loader's regular batch shape (recorded at first
        use; the parameters are read in place, so training steps in between need no re-recording), eager for any other shape
        (the ragged last batch) and when graphs are off."""
        if self._record and inputs and inputs[0].is_cuda:
            g = self._graphed_eval
            if g is None:
                try:
                    g = self._graphed_eval = GraphedForward(self.model, inputs, feed=feed)
                except Exception as e:          # a capture the runtime refuses costs the speed-up, not the validation
                    self.print_write_to_log(f"eval forward not graphed ({type(e).__name__}: {str(e)[:100]})")
                    g = self._graphed_eval = False
            if g and g.matches(inputs):
                return g(inputs)
        out = self.model(*(inputs if feed is None else feed.inputs(*inputs)))
        return out[0] if isinstance(out, tuple) else out

    def _negative_towers(self):
        """The one Recommender of this experiment: the validation's latent tables, and with neg_candidates > 1 the sampler's."""
        if self._towers is None:
            from .recommend import AhnRecommender, Recommender
            # AHN (ahn_tables): per-id sentence tables and the fused pair tail speak the same protocol
            self._towers = (AhnRecommender if self.kind == "ahn" else Recommender)(self.model, self.cache)
        return self._towers

    def _hand_tables_to_feed(self, towers):
        """neg_candidates > 1: the feed copies the tables (a recorded step keeps its pointers); the head's parameters stay live."""
        mode, h, g, ub, ib = self.model.score_mode_and_params()
        self.train_feed.set_tables(mode, towers.user_latents, towers.item_latents, h, g, ub, ib)

    def _refresh_negative_tables(self):
        """Encodes the catalogue with the parameters as they are now and hands the tables to the negative sampler (the model's
        train / eval mode is as before afterwards: Recommender.refresh restores it)."""
        self._hand_tables_to_feed(self._negative_towers().refresh())

    def valid_one_epoch(self):
        loader = self.valid_loader
        sq_err = torch.zeros((), device=self.device, dtype=torch.float64)
        loss_sum = torch.zeros((), device=self.device, dtype=torch.float64)
        count = torch.zeros((), device=self.device, dtype=torch.float64)
        steps = 0
        self.model.eval()
        towers = None
        if self.args.eval_from_towers:
            # every user / item document encoded ONCE into latent tables (the parameters changed since the last epoch), then a
            # pair is two row gathers and the head's arithmetic instead of two document encodes (recommend.Recommender)
            towers = self._negative_towers()
            towers.refresh()
            if self.kind == "ahn" and not self._table_bytes_logged:
                self._table_bytes_logged = True      # ahn_tables is a memory opt-in: say once what it costs
                nbytes = sum(t.numel() * t.element_size() for st in (towers.user_state, towers.item_state) for t in st)
                self.print_write_to_log("ahn_tables: {:,d} bytes of per-id sentence tables ({} users, {} items)".format(
                    nbytes, towers.n_users, towers.n_items))
            if self.args.neg_candidates > 1:
                self._hand_tables_to_feed(towers)          # the next epoch's candidates are scored from this pass's tables
        ranks = []
        if self.args.rank_metrics and self._seen is None:
            # what a validation item competes against: every item its user has not rated in the training split
            self._seen = towers.seen_from(self.train_set.examples, towers.n_users, self.device)
        with torch.no_grad():
            for batch in loader:
                if towers is not None:
                    u_ids, i_ids, ratings = [t.to(self.device, non_blocking=True) for t in batch]
                    pred = towers.score(u_ids, i_ids)
                    if self.args.rank_metrics:
                        ranks.append(towers.rank(u_ids, i_ids, exclude=self._seen))
                elif self.cache is not None:
                    u_ids, i_ids, ratings = [t.to(self.device, non_blocking=True) for t in batch]
                    pred = self._eval_forward((u_ids, i_ids), self.eval_feed)
                else:
                    inputs, ratings = self._to_device(batch)
                    pred = self._eval_forward(inputs)
                loss = self.loss_func(pred, ratings)
                sq_err += loss.double() * ratings.size(0)
                loss_sum += loss.double()
                count += ratings.size(0)
                steps += 1
        if self.parallel:
            import torch.distributed as dist
            for t in (sq_err, count):
                dist.all_reduce(t)
        self.valid_count = int(count)                     # examples that entered the RMSE: len(valid_set), each once
        rmse = math.sqrt(float(sq_err) / max(float(count), 1.0))
        self.last_valid_rmse = rmse
        RF.check_id_errors(self.device)
        if self.select_metric is not None:
            self.best_rmse = min(self.best_rmse, rmse)        # reported; the model is selected below, by its rank metric
        else:
            self.best_rmse = -self._selected(-rmse, -self.best_rmse)      # lower is better: selected by its negative
        self.print_write_to_log("valid loss: {:.3f}, valid rmse: {:.3f}, best rmse: {:.3f}".format(
            float(loss_sum) / max(steps, 1), rmse, self.best_rmse))
        if ranks:
            from .recommend import rank_metrics
            m = self.last_rank_metrics = rank_metrics(torch.cat([r for r, _ in ranks]), torch.cat([c for _, c in ranks]),
                                                      self.args.rank_metrics)
            keys = [f"{name}@{k}" for k in self.args.rank_metrics for name in ("hr", "ndcg")] + ["mrr"]
            line = "valid " + ", ".join("{}: {:.3f}".format(k, m[k]) for k in keys)
            if self.select_metric is not None:
                self.best_score = self._selected(m[self.select_metric], self.best_score)
                line += ", best {}: {:.3f}".format(self.select_metric, self.best_score)
            self.print_write_to_log(line)
        if self.patience >= self.args.patience:
            raise EarlyStop("early stop")

    def _selected(self, score, best):
        """Model selection by a score where higher is better: a `score` above `best` saves best_model.pt and resets the patience;
        anything else (None: the metric had no pair to rank) uses one up.  Returns the best score so far."""
        if score is not None and score > best:
            self.save("best_model.pt")
            self.patience = 0
            return score
        self.patience += 1
        return best

    def train(self):
        self.print_write_to_log("start training ...")
        for epoch in range(self.args.epochs):
            self.train_one_epoch(epoch)
            self.valid_one_epoch()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, choices=ReviewExperiment.KINDS)
    ap.add_argument("--config", required=True, help="flat JSON config with the reference's keys")
    ap.add_argument("--reference-quirks", action="store_true", help="hard-code kernel_sizes=[3] (and NARRE hidden_dim=150)")
    a = ap.parse_args(argv)
    exp = ReviewExperiment(a.model, parse_args(a.config), reference_quirks=a.reference_quirks)
    try:
        exp.train()
    except EarlyStop:
        exp.print_write_to_log("early stop (patience {})".format(exp.args.patience))


if __name__ == "__main__":
    main()
