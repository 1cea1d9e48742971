"""Catalogue scoring and top-K recommendation from cached tower latents.

    python -m review_based_recommender_amd.recommend --model deepconn --config cfg.json --checkpoint best_model.pt \\
        --k 10 [--exclude-train] --out recs.jsonl
    python -m review_based_recommender_amd.recommend --model deepconn --config cfg.json --checkpoint best_model.pt \\
        --eval-split test [--ks 5,10,20] [--exclude-train] [--metrics-out metrics.json]

Every tower of the four models depends on its own side only (DeepCoNN++ / SimpleSiamese: LastFeat(encoder(doc), id); NARRE: the
same over an attention pool keyed by the reviews' own counterpart ids; D-ATT: the shared fc over cat(local, global)), and the
pair-dependent rest is the FM head or an inner product.  `Recommender.refresh()` therefore encodes every user and every item
ONCE into latent tables [U, K] / [I, K]; `score`, `score_all` and `topk` then run on the tables alone (csrc/pair_score.hip) --
`topk` without ever building the U x I score matrix, and `rank` / `evaluate` say where the held-out item of a (user, item) pair
lands in that user's ranking (HR@K, NDCG@K, MRR, AUC), without it too.  The reference can only score a pair by encoding both of
its documents (models/deepconn/deepconn.py:43-53) and has no ranking entry at all.

The output file holds one JSON line per user id 1 .. U-1 (id 0 is the padding id of both sides: never a user, never recommended):
    {"user": u, "items": [...], "scores": [...]}
With --explain N every line also carries "why", one entry per recommended item (DeepCoNN++ and NARRE, CNN arch): the N tokens of
the user's and of the item's text that moved the score most, as [position, token, weight] (words where meta.pkl's vocabulary is
readable, else token ids; NARRE: position = review slot * rv_len + position in the review), and for NARRE the item's N
weightiest reviews as [slot, id of the review's author, attention weight, contribution] (Recommender.explain).
With --attention N (dual_att) every line carries "why" too, one entry per recommended item: the N entries of largest |weight| of
the user's and of the item's document as [position, token, weight, local_gate], the weight followed through both attention gates
(Recommender.attention).
With --contributions N (simple_siamese) every line carries "why" too, one entry per recommended item: per side the N tokens of
largest |weight| as [review slot * rv_len + position, token, weight], the weight followed through the review attention, and the N
reviews of largest |contribution| as [slot, id of the review's counterpart (-1 where unknown), attention weight, contribution]
(Recommender.contributions).
With --eval-split the (user, item) pairs of that split are ranked instead (as well, when --out is given too) and one JSON line of
rank_metrics goes to --metrics-out, or to stdout.

--model ahn: AHN's towers attend to each other, so it has no latent tables -- but only the user side depends on the pair, and the
encoder on the id alone.  `AhnRecommender` keeps per-id SENTENCE tables and scores a pair by the co-attention tail in one HIP launch
per block (csrc/ahn_pair.hip); same flags and JSON lines, sentence split instead of the doc / review split, --explain refused.
With --sentences N (ahn) every line carries "why", one entry per recommended item: "user_sentences", the N sentences of the user
of largest |contribution| as [review slot, sentence slot, attention weight, contribution, matched item review slot, matched item
sentence slot] -- the contribution followed through both softmaxes and both max-similarities, the match being the item sentence
the co-attention paired it with -- plus, where meta.pkl's vocabulary is readable, the sentence's words and the matched item
sentence's words; "item_sentences", the N matched item sentences of largest |match contribution| as [review slot, sentence slot,
item_sent_weight, match contribution]; "user_reviews" and "item_reviews" as [slot, attention weight, contribution]
(AhnRecommender.sentences, csrc/ahn_explain.hip: one launch per block of pairs).
With --words N beside --sentences every entry of "user_sentences" and "item_sentences" ends with the sentence's N words of largest
|contribution| as [position, word, contribution], the contribution followed through the BiLSTM and everything behind it, the
item's through its own attention path as well as its matches (AhnRecommender.words, csrc/lstm_seq.hip: the encoder runs again).
"""
from __future__ import annotations

import argparse
import json
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import functional as RF

KINDS = {"DeepCoNNpp": "deepconn", "NARRE": "narre", "DualAtt": "dual_att", "SimpleSiamese": "simple_siamese"}
PAD = 0                 # padding token and padding user / item id of the reference's data (utils.py:30-42, meta.pkl row 0)


class SeenItems(NamedTuple):
    """Items every USER ID has already rated, CSR over all user ids: off int64 [U + 1], items int32 sorted within a user."""
    off: torch.Tensor
    items: torch.Tensor


class Explanation(NamedTuple):
    """Recommender.explain: why the pairs (u_ids[b], i_ids[b]) scored as they did.  tokens: DeepCoNN++ [B, doc_len], NARRE
    [B, rv_num, rv_len]; the four review fields are None for DeepCoNN++ (its towers read one document each)."""
    score: torch.Tensor                                   # [B] = Recommender.score
    user_tokens: torch.Tensor                             # contribution of every token position of the user's text
    item_tokens: torch.Tensor
    user_text: torch.Tensor                               # [B] what the user's text as a whole adds to the score
    item_text: torch.Tensor
    user_review_weights: Optional[torch.Tensor] = None    # [B, rv_num] NARRE's attention weights
    user_reviews: Optional[torch.Tensor] = None           # [B, rv_num] contribution of every review; sums to user_text
    item_review_weights: Optional[torch.Tensor] = None
    item_reviews: Optional[torch.Tensor] = None


class Attention(NamedTuple):
    """Recommender.attention (D-ATT): the two attention gates of each side of the pairs (u_ids[b], i_ids[b]) and what every token
    adds to the score, followed through the fc, the convs AND both gates (DualAtt.attend_users has the fields' definitions)."""
    score: torch.Tensor                   # [B] = Recommender.score
    user_local_gate: torch.Tensor         # [B, doc_len] the local gate of every position
    user_global_gate: torch.Tensor        # [B] the document's global gate
    user_tokens: torch.Tensor             # [B, doc_len] gradient x input of every token, through the gates
    user_tokens_fixed: torch.Tensor       # [B, doc_len] the part with the gates held constant
    user_local_text: torch.Tensor         # [B] what the local half of the features adds to the score
    user_global_text: torch.Tensor        # [B] the global half
    item_local_gate: torch.Tensor
    item_global_gate: torch.Tensor
    item_tokens: torch.Tensor
    item_tokens_fixed: torch.Tensor
    item_local_text: torch.Tensor
    item_global_text: torch.Tensor


class Contributions(NamedTuple):
    """Recommender.contributions (SimpleSiamese): what every token and every review of each side of the pairs (u_ids[b],
    i_ids[b]) adds to the score (SimpleSiamese.contribute_users has the fields' definitions)."""
    score: torch.Tensor                   # [B] = Recommender.score
    user_tokens: torch.Tensor             # [B, rv_num, rv_len] gradient x input of every token, through the attention softmax
    item_tokens: torch.Tensor
    user_tokens_fixed: torch.Tensor       # [B, rv_num, rv_len] the part with the attention weights held constant
    item_tokens_fixed: torch.Tensor
    user_text: torch.Tensor               # [B] what the user's text as a whole adds to the score
    item_text: torch.Tensor
    user_review_weights: torch.Tensor     # [B, rv_num] the forward attention weights
    user_reviews: torch.Tensor            # [B, rv_num] contribution of every review under those weights; sums to user_text
    item_review_weights: torch.Tensor
    item_reviews: torch.Tensor


class SentenceContributions(NamedTuple):
    """AhnRecommender.sentences: what every sentence and review of the pairs (u_ids[b], i_ids[b]) adds to AHN's score, and which
    item sentence each user sentence matched (functional.ahn_pair_explain and include/rbr_hip.h have the definitions)."""
    score: torch.Tensor                   # [B] = AhnRecommender.score
    user_sent_weights: torch.Tensor       # [B, Ru, Su] the four weight arrays of AhnRecommender.attention
    item_sent_weights: torch.Tensor       # [B, Ri, Si]
    user_review_weights: torch.Tensor     # [B, Ru]
    item_review_weights: torch.Tensor     # [B, Ri]
    user_sentences: torch.Tensor          # [B, Ru, Su] gradient x input of every sentence vector, through both softmaxes and maxima
    user_sentences_fixed: torch.Tensor    # [B, Ru, Su] the part with both attention weightings held constant
    user_reviews: torch.Tensor            # [B, Ru] contribution of every user review; sums to user_text
    user_text: torch.Tensor               # [B] what the user's text as a whole adds to the score
    user_match: torch.Tensor              # int64 [B, Ru, Su] the flat item sentence ri * Si + si each user sentence matched
    review_match: torch.Tensor            # int64 [B, Ru] the item review each user review matched
    item_sentence_match: torch.Tensor     # [B, Ri, Si] what an item sentence adds as the match of user sentences; 0 where unmatched
    item_review_match: torch.Tensor       # [B, Ri] the same for the item's reviews
    item_reviews: torch.Tensor            # [B, Ri] the item's own path, its attention weights held constant; sums to item_text
    item_text: torch.Tensor               # [B]


class WordContributions(NamedTuple):
    """AhnRecommender.words: what every WORD of the pairs (u_ids[b], i_ids[b]) adds to AHN's score -- gradient x input of the
    word's embedding, followed through the BiLSTM, the max over the words and everything behind it (AHN.word_contributions)."""
    score: torch.Tensor                   # [B] = AhnRecommender.score
    user_words: torch.Tensor              # [B, Ru, Su, W] = user_words_dir.sum(-1)
    item_words: torch.Tensor              # [B, Ri, Si, W] through the item's FULL path: as the match of user sentences and its own
    user_sentences: torch.Tensor          # [B, Ru, Su] <d score / d sentence vector, sentence vector> = sentences().user_sentences
    item_sentences: torch.Tensor          # [B, Ri, Si] the same for the item's sentences, full path
    user_words_dir: torch.Tensor          # [B, Ru, Su, W, 2] the split by BiLSTM direction (forward, reverse)
    item_words_dir: torch.Tensor          # [B, Ri, Si, W, 2]


def top_tokens(tokens: torch.Tensor, docs: torch.Tensor, n: int):
    """(position int64 [rows, n'], token id [rows, n'], weight [rows, n']) of the n' = min(n, positions) entries of largest
    |weight| in every row of tokens [rows, ...] (trailing dimensions are flattened: a NARRE position is slot * rv_len + t),
    |weight| descending, ties by the lower position; docs holds the token ids, same shape."""
    if n < 1:
        raise ValueError("top_tokens needs n >= 1")
    if tokens.shape != docs.shape:
        raise ValueError(f"tokens and docs must have one shape, got {tuple(tokens.shape)} / {tuple(docs.shape)}")
    w, d = tokens.reshape(tokens.shape[0], -1), docs.reshape(docs.shape[0], -1)
    pos = torch.sort(w.abs(), dim=1, descending=True, stable=True).indices[:, :min(int(n), w.shape[1])]
    return pos, torch.gather(d, 1, pos), torch.gather(w, 1, pos)


def rank_metrics(rank: torch.Tensor, n_cand: torch.Tensor, ks) -> dict:
    """Ranking metrics of held-out pairs from their exact ranks (Recommender.rank; any integer tensors, CPU or GPU), summed in
    float64.  rank < 0 is an unranked pair: a miss in the first three.
        hr@K      mean(0 <= rank < K)
        ndcg@K    mean(1 / log2(rank + 2) where 0 <= rank < K, else 0)         one relevant item per pair: the ideal DCG is 1
        mrr       mean(1 / (rank + 1), 0 where unranked)
        auc       mean(1 - rank / (n_cand - 1)) over the ranked pairs with n_cand > 1: the share of the other candidates below
        mean_rank mean(rank) over the ranked pairs
        n, unranked   pairs, and pairs with rank < 0
    A mean over no pair at all is None."""
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError(f"every K of rank_metrics must be at least 1, got {ks}")
    r, c = rank.reshape(-1).to(torch.int64), n_cand.reshape(-1).to(torch.int64)
    if r.shape != c.shape:
        raise ValueError(f"rank and n_cand must hold one value per pair each, got {tuple(rank.shape)} / {tuple(n_cand.shape)}")
    ranked = r >= 0
    rd = r.clamp_min(0).double()
    in_auc = ranked & (c > 1)
    sums = [ranked.sum().double(), in_auc.sum().double(), (ranked.double() / (rd + 1)).sum(),
            (in_auc.double() * (1 - rd / (c - 1).clamp_min(1).double())).sum(), (ranked.double() * rd).sum()]
    for k in ks:
        hit = (ranked & (r < k)).double()
        sums += [hit.sum(), (hit / torch.log2(rd + 2)).sum()]
    n = r.numel()
    n_ranked, n_auc, mrr, auc, rank_sum, *per_k = torch.stack(sums).tolist()       # one read-back
    mean = lambda total, count: total / count if count else None                   # noqa: E731
    out = {}
    for j, k in enumerate(ks):
        out[f"hr@{k}"], out[f"ndcg@{k}"] = mean(per_k[2 * j], n), mean(per_k[2 * j + 1], n)
    out.update({"mrr": mean(mrr, n), "auc": mean(auc, n_auc), "mean_rank": mean(rank_sum, n_ranked), "n": n,
                "unranked": n - int(n_ranked)})
    return out


def _check_pairs(u_ids, i_ids, chunk, tables=None):
    """The pair arguments of explain / attention / contributions / sentences / words: chunk >= 1 and two id vectors [B], B >= 1.
    `tables` (AhnRecommender._tables) runs between the two checks: AHN's entry points report missing tables before a bad shape."""
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    if tables is not None:
        tables()
    if u_ids.dim() != 1 or u_ids.shape != i_ids.shape or u_ids.shape[0] == 0:
        raise ValueError(f"u_ids / i_ids must be [B] each with B >= 1, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")


def _cat_chunks(parts, empty=None):
    """The columns of the per-chunk result tuples `parts`, each concatenated over the chunks; a single chunk's columns are
    returned as they are (no launch), and no chunk at all gives `empty`."""
    if not parts:
        return empty
    return [torch.cat(col) if len(parts) > 1 else col[0] for col in zip(*parts)]


def _evaluate(rec, pairs, ks, exclude, chunk) -> dict:
    """Recommender.evaluate and AhnRecommender.evaluate: rec.rank over `chunk` pairs at a time, one rank_metrics call."""
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    dev = rec._device()
    if len(pairs) == 2 and all(torch.is_tensor(t) for t in pairs):
        u_ids, i_ids = (t.to(dev, torch.int64) for t in pairs)
    else:
        u_ids = torch.tensor([int(e[0]) for e in pairs], dtype=torch.int64, device=dev)
        i_ids = torch.tensor([int(e[1]) for e in pairs], dtype=torch.int64, device=dev)
    parts = [rec.rank(u_ids[a:a + chunk], i_ids[a:a + chunk], exclude) for a in range(0, u_ids.shape[0], chunk)]
    rank, n_cand = _cat_chunks(parts, empty=[torch.empty(0, dtype=torch.int32, device=dev)] * 2)
    return rank_metrics(rank, n_cand, ks)


# what each tower's explain_* / attend_* / contribute_* returns per side: the result's field names less user_ / item_
_SIDE_FIELDS = {"deepconn": ("tokens", "text"), "narre": ("tokens", "text", "review_weights", "reviews"),
                "dual_att": ("local_gate", "global_gate", "tokens", "tokens_fixed", "local_text", "global_text"),
                "simple_siamese": ("tokens", "tokens_fixed", "text", "review_weights", "reviews")}


class Recommender:
    """Latent tables of a trained model over a whole catalogue, and the queries on them.

    `cache`: a data.DeviceDocCache (doc split for DeepCoNN++ / D-ATT) or data.DeviceReviewCache (review split for NARRE /
    SimpleSiamese; a DeviceDocCache of the review split serves too); or pass the
    per-id document tensors yourself: `user` / `item` = [U, L] (doc split) or [U, R, T] (review split) integer tensors on the
    model's device, plus `user_rids` / `item_rids` [U, R] int64 for NARRE.  Row 0 of each side is the padding id.

    The tables are a snapshot: call refresh() again after the parameters change.  `stale` compares the parameters' torch
    version counters with those seen by the last refresh -- it catches torch-side in-place updates (optimizer.step(),
    load_state_dict), NOT the updates train_step.HipClipAdam or a replayed hipGraph write through raw pointers."""

    def __init__(self, model, cache=None, *, user=None, item=None, user_rids=None, item_rids=None):
        kind = KINDS.get(type(model).__name__)
        if kind is None:
            raise ValueError(f"{type(model).__name__} is not one of {sorted(KINDS)}")
        if cache is None:
            if user is None or item is None:
                raise ValueError("Recommender needs a DeviceDocCache or the per-id `user` / `item` document tensors")
            cache = SimpleNamespace(user=user, item=item, user_rids=user_rids, item_rids=item_rids)
        want_dim = 3 if kind in ("narre", "simple_siamese") else 2
        if cache.user.dim() != want_dim or cache.item.dim() != want_dim:
            raise ValueError(f"{kind} reads {'[U, R, T] reviews' if want_dim == 3 else '[U, L] documents'} per id, got "
                             f"{tuple(cache.user.shape)} / {tuple(cache.item.shape)}")
        if kind == "narre" and (cache.user_rids is None or cache.item_rids is None):
            raise ValueError("NARRE's attention pools need the reviews' counterpart ids (user_rids / item_rids)")
        self.model, self.kind, self.cache = model, kind, cache
        self.n_users, self.n_items = cache.user.shape[0], cache.item.shape[0]
        self.item_lo = 1                     # the padding id 0 is never recommended
        self.user_latents: Optional[torch.Tensor] = None
        self.item_latents: Optional[torch.Tensor] = None
        self._versions = None

    # ------------------------------------------------------------------ the tables
    def _tower_args(self, side: str, ids: torch.Tensor, take):
        """The positional arguments this kind's towers read for the ids `ids` of a side; `take` selects those ids' rows from a
        cache table (refresh: a slice, the pair driver: a gather)."""
        c = self.cache
        docs = take(getattr(c, side)).to(torch.int64).contiguous()
        if self.kind == "dual_att":
            return (docs,)
        word_masks = docs != PAD
        if self.kind == "deepconn":
            return docs, word_masks, ids
        if self.kind == "narre":
            return docs, word_masks, ids, take(getattr(c, f"{side}_rids"))
        return docs, word_masks, word_masks.any(-1), ids           # review masks: the reviews that hold any token

    def _encode(self, side: str, a: int, b: int) -> torch.Tensor:
        ids = torch.arange(a, b, dtype=torch.int64, device=getattr(self.cache, side).device)
        return getattr(self.model, f"encode_{side}s")(*self._tower_args(side, ids, lambda t: t[a:b]))

    def refresh(self, chunk: int = 256) -> "Recommender":
        """Encodes all users and all items, `chunk` ids at a time, into the latent tables (eval semantics, no autograd; the
        model's train / eval mode is restored afterwards).  Call it again after the parameters change."""
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        with RF.eval_mode(self.model):
            tables = []
            for side, n in (("user", self.n_users), ("item", self.n_items)):
                table = None
                for a in range(0, n, chunk):
                    rows = self._encode(side, a, min(a + chunk, n))
                    if table is None:
                        table = torch.empty(n, rows.shape[1], dtype=torch.float32, device=rows.device)
                    table[a:a + rows.shape[0]] = rows
                tables.append(table)
            self.user_latents, self.item_latents = tables
        self._versions = [p._version for p in self.model.parameters()]
        return self

    @property
    def stale(self) -> bool:
        """True before the first refresh() and when a parameter's torch version counter moved since the last one (see the class
        docstring for what that does not see)."""
        return self._versions is None or self._versions != [p._version for p in self.model.parameters()]

    def _tables(self):
        if self.user_latents is None:
            raise RuntimeError("Recommender.refresh() has not been called: there are no latent tables yet")
        return self.user_latents, self.item_latents

    def _user_rows(self, u_ids):
        """The latent rows and bias rows of u_ids (HIP row gathers), the checked ids, and the rest of the head's parameters."""
        ul, il = self._tables()
        mode, h, g, ub, ib = self.model.score_mode_and_params()
        (u_ids,) = RF.sanitize_ids([(u_ids, self.n_users, PAD)])
        with torch.no_grad():
            rows = RF.embedding(ul, u_ids, None)
            ub_rows = RF.embedding(ub.detach(), u_ids, None) if ub is not None else None
        return mode, rows, il, h, g, ub_rows, ib, u_ids

    # ------------------------------------------------------------------ the queries
    def score(self, u_ids: torch.Tensor, i_ids: torch.Tensor) -> torch.Tensor:
        """Predicted ratings [B] of the pairs (u_ids[b], i_ids[b]): two row gathers and the head's arithmetic per pair."""
        ul, il = self._tables()
        mode, h, g, ub, ib = self.model.score_mode_and_params()
        return RF.pair_score(mode, ul, il, u_ids, i_ids, h, g, ub, ib)

    def score_all(self, u_ids: torch.Tensor) -> torch.Tensor:
        """Predicted ratings [len(u_ids), I] of the given users against every item id (column 0 is the padding id)."""
        mode, rows, il, h, g, ub_rows, ib, _ = self._user_rows(u_ids)
        return RF.pair_score_dense(mode, rows, il, h, g, ub_rows, ib)

    def topk(self, u_ids: torch.Tensor, k: int, exclude=None):
        """(items int64 [len(u_ids), k], scores [len(u_ids), k]): each user's k best items, score descending, ties by the lower
        item id; item 0 never appears.  `exclude`: a SeenItems (Recommender.seen_from: CSR over all user ids), or a CSR pair
        (off int64 [len(u_ids) + 1], items int32 sorted within a row) aligned with u_ids.  Rows with fewer than k candidates
        end in item -1, score -inf."""
        mode, rows, il, h, g, ub_rows, ib, u_ids = self._user_rows(u_ids)
        if isinstance(exclude, SeenItems):
            exclude = (exclude.off, exclude.items, u_ids)
        return RF.pair_score_topk(mode, rows, il, k, h, g, ub_rows, ib, item_lo=self.item_lo, exclude=exclude)

    def rank(self, u_ids: torch.Tensor, i_ids: torch.Tensor, exclude=None):
        """(rank int32 [B], n_cand int32 [B]) of the held-out pairs (u_ids[b], i_ids[b]): rank[b] is the position of item
        i_ids[b] in the list topk(u_ids[b], k, exclude) of any k -- the number of candidates that come before it -- and n_cand[b]
        the number of candidates it competes in; exact, without the score matrix, for ranks beyond every k.  `exclude` as in
        topk, a row per pair; the held-out item itself is never excluded.  rank -1: the padding item 0, an id outside the
        table, or a NaN score."""
        mode, rows, il, h, g, ub_rows, ib, u_ids = self._user_rows(u_ids)
        if isinstance(exclude, SeenItems):
            exclude = (exclude.off, exclude.items, u_ids)
        return RF.pair_score_rank(mode, rows, il, i_ids, h, g, ub_rows, ib, item_lo=self.item_lo, exclude=exclude)

    def _explain_pairs(self, result, verb: str, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int):
        """The driver of explain / attention / contributions: the score, the head's gradient on both latent rows, and per chunk
        of pairs the towers' `verb`_users / `verb`_items on the pairs' cache rows, read as _encode reads them; `result` is
        built by field name from the towers' _SIDE_FIELDS."""
        _check_pairs(u_ids, i_ids, chunk)
        ul, il = self._tables()
        mode, h, _, _, _ = self.model.score_mode_and_params()
        score = self.score(u_ids, i_ids)
        u_ids, i_ids = RF.sanitize_ids([(u_ids, self.n_users, PAD), (i_ids, self.n_items, PAD)])
        with torch.no_grad():
            zu, zi = RF.embedding(ul, u_ids, None), RF.embedding(il, i_ids, None)
            if mode == "fm":                 # score = relu(zu * zi) . h + biases
                live = h.detach().view(1, -1) * (zu * zi > 0)
                d_u, d_i = live * zi, live * zu
            else:                            # the inner product: each side's gradient is the other side's row
                d_u, d_i = zi, zu

        def tower(side, ids, d_latent):
            return getattr(self.model, f"{verb}_{side}s")(*self._tower_args(side, ids, lambda t: t.index_select(0, ids)), d_latent)

        cols = _cat_chunks([tower("user", u_ids[a:a + chunk], d_u[a:a + chunk]) + tower("item", i_ids[a:a + chunk], d_i[a:a + chunk])
                            for a in range(0, u_ids.shape[0], chunk)])
        names = [f"{side}_{field}" for side in ("user", "item") for field in _SIDE_FIELDS[self.kind]]
        return result(score=score, **dict(zip(names, cols)))

    def explain(self, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int = 256) -> Explanation:
        """Why the pairs (u_ids[b], i_ids[b]) scored as they did (DeepCoNN++ and NARRE, CNN arch), `chunk` pairs at a time, from
        the latent tables and the cache rows; eval semantics, no autograd, the model's mode is restored.
        With zu, zi the pair's latent rows the FM head is score = relu(zu * zi) . h + biases, so d score / d zu =
        h * [zu * zi > 0] * zi (and zu for the item side); each tower turns that gradient into gradient x input of its own text
        (the models' explain_users / explain_items): *_tokens per token position, *_text per side, and for NARRE *_reviews per
        review under the attention weights *_review_weights, which are held constant.  The id embeddings and the biases are the
        part of the score no text explains."""
        if self.kind not in ("deepconn", "narre"):
            raise ValueError(f"Recommender.explain covers DeepCoNN++ and NARRE with arch='CNN'; {type(self.model).__name__} is not covered")
        return self._explain_pairs(Explanation, "explain", u_ids, i_ids, chunk)

    def attention(self, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int = 256) -> Attention:
        """D-ATT's answer to "why": both attention gates of each side of the pairs (u_ids[b], i_ids[b]) and the per-token
        contributions followed through them, `chunk` pairs at a time, from the latent tables and the cache rows; eval semantics, no
        autograd, the model's mode is restored.  The score is the plain inner product of the latent rows, so d score / d (the
        user's latent row) is the item's row and the reverse; each tower turns that gradient into its six fields
        (DualAtt.attend_users / attend_items)."""
        if self.kind != "dual_att":
            raise ValueError(f"Recommender.attention covers D-ATT (DualAtt); {type(self.model).__name__} is not covered "
                             "(DeepCoNN++ and NARRE: Recommender.explain)")
        return self._explain_pairs(Attention, "attend", u_ids, i_ids, chunk)

    def contributions(self, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int = 256) -> Contributions:
        """SimpleSiamese's answer to "why": per-token and per-review contributions of each side of the pairs (u_ids[b],
        i_ids[b]), `chunk` pairs at a time, from the latent tables and the cache rows; eval semantics, no autograd, the model's
        mode is restored.  The head is explain's -- d score / d zu = h * [zu * zi > 0] * zi, and zu for the item side -- and each
        tower turns that gradient into its five fields (SimpleSiamese.contribute_users / contribute_items): the tower has no
        max-pool, so *_tokens follow the attention softmax too, and *_tokens_fixed hold the weights constant."""
        if self.kind != "simple_siamese":
            raise ValueError(f"Recommender.contributions covers SimpleSiamese; {type(self.model).__name__} is not covered "
                             "(DeepCoNN++ and NARRE: Recommender.explain, D-ATT: Recommender.attention)")
        return self._explain_pairs(Contributions, "contribute", u_ids, i_ids, chunk)

    def _device(self):
        return self._tables()[0].device

    def evaluate(self, pairs, ks=(5, 10, 20), exclude=None, chunk: int = 4096) -> dict:
        """rank_metrics of held-out pairs: `pairs` is a dataset's examples (sequences starting (u_id, i_id, ...)) or the id
        tensors (u_ids, i_ids) themselves.  Ranked `chunk` pairs at a time, one rank_metrics call over all of them; `exclude`: a
        SeenItems (the CLI's --exclude-train: the training split's seen_from) or None."""
        return _evaluate(self, pairs, ks, exclude, chunk)

    @staticmethod
    def seen_from(examples, n_users: int, device=None) -> SeenItems:
        """The items each user id has rated in `examples` (a dataset's examples: sequences starting (u_id, i_id, ...)) as a
        SeenItems over user ids 0 .. n_users-1: duplicates dropped, items ascending within a user."""
        pairs = sorted({(int(e[0]), int(e[1])) for e in examples})
        if pairs and not (0 <= pairs[0][0] and pairs[-1][0] < n_users):
            raise IndexError(f"user ids span [{pairs[0][0]}, {pairs[-1][0]}] but there are {n_users} users")
        counts = torch.zeros(n_users + 1, dtype=torch.int64)
        if pairs:
            counts[1:] = torch.bincount(torch.tensor([u for u, _ in pairs], dtype=torch.int64), minlength=n_users)
        off = torch.cumsum(counts, 0)
        items = torch.tensor([i for _, i in pairs], dtype=torch.int32)
        return SeenItems(off.to(device), items.to(device)) if device is not None else SeenItems(off, items)


# ---------------------------------------------------------------------------------------------------------------- AHN
def exclusion_mask(exclude, u_ids: torch.Tensor, n_items: int) -> Optional[torch.Tensor]:
    """bool [len(u_ids), n_items] of the items each row must never get, from the `exclude` argument of topk / rank: None, a
    SeenItems (CSR over all user ids; row b takes user u_ids[b]) or a CSR pair (off int64 [len(u_ids) + 1], items int32)
    aligned with u_ids.  Torch composition, any device, no host synchronisation; items outside [0, n_items) list nothing."""
    if exclude is None:
        return None
    n, dev = u_ids.shape[0], u_ids.device
    off, items = exclude[0].to(dev), exclude[1].to(dev, torch.int64)
    entry_row = torch.searchsorted(off[1:].contiguous(), torch.arange(items.shape[0], device=dev), right=True)
    if isinstance(exclude, SeenItems):
        # several rows may name one user: one of them collects the user's entries, every row then copies its user's collector
        n_users = off.shape[0] - 1
        collector = torch.full((n_users + 1,), n, dtype=torch.int64, device=dev)
        inside = (u_ids >= 0) & (u_ids < n_users)
        slot = torch.where(inside, u_ids, torch.full_like(u_ids, n_users))
        collector[slot] = torch.where(inside, torch.arange(n, device=dev), torch.full_like(u_ids, n))
        entry_row = collector[entry_row.clamp_max(n_users)]
        row_of = collector[slot]
    else:
        if off.shape[0] != n + 1:
            raise ValueError(f"exclude offsets must be [{n + 1}] for {n} rows, got {tuple(off.shape)}")
        row_of = torch.arange(n, device=dev)
    ok = (items >= 0) & (items < n_items) & (entry_row < n)
    mask = torch.zeros(n + 1, n_items, dtype=torch.bool, device=dev)          # row n: the sink of everything that lists nothing
    mask[torch.where(ok, entry_row, torch.full_like(entry_row, n)), torch.where(ok, items, torch.zeros_like(items))] = True
    mask[n] = False
    return mask[row_of]


def select_topk(scores: torch.Tensor, k: int, excluded: Optional[torch.Tensor] = None, item_lo: int = 1):
    """Recommender.topk's rule over a dense score block [n, I]: (items int64 [n, k], scores [n, k]) -- the candidates are the
    items >= item_lo that are not `excluded` (bool [n, I]) and whose score is not NaN; score descending, ties by the lower item
    id; rows with fewer than k candidates end in item -1, score -inf.  Two stable sorts (torch composition)."""
    if k < 1:
        raise ValueError("k must be at least 1")
    n, n_items = scores.shape
    cols = torch.arange(n_items, device=scores.device).view(1, n_items)
    cand = (cols >= item_lo) & ~torch.isnan(scores)
    if excluded is not None:
        cand = cand & ~excluded
    order = torch.sort(torch.where(cand, scores, torch.full_like(scores, float("-inf"))), dim=1, descending=True, stable=True).indices
    first = torch.sort((~torch.gather(cand, 1, order)).to(torch.int8), dim=1, stable=True).indices      # candidates first, order kept
    order = torch.gather(order, 1, first)
    got = torch.gather(cand, 1, order)
    if k > n_items:                             # more asked than there are items: the rest is fill
        order = torch.cat([order, order.new_zeros(n, k - n_items)], dim=1)
        got = torch.cat([got, got.new_zeros(n, k - n_items)], dim=1)
    order, got = order[:, :k], got[:, :k]
    vals = torch.gather(scores, 1, order)
    return (torch.where(got, order, torch.full_like(order, -1)),
            torch.where(got, vals, torch.full_like(vals, float("-inf"))))


def rank_in_block(scores: torch.Tensor, targets: torch.Tensor, excluded: Optional[torch.Tensor] = None, item_lo: int = 1):
    """Recommender.rank's rule over a dense score block [B, I], row b for the pair (b, targets[b]): (rank int32 [B], n_cand int32
    [B]).  Candidates as in select_topk, except that the target is never excluded; rank = candidates with a higher score, or the
    same score and a lower id; rank -1: a target outside [item_lo, I) or a NaN score.  Compare and count (torch composition)."""
    B, n_items = scores.shape
    cols = torch.arange(n_items, device=scores.device).view(1, n_items)
    tgt = targets.to(torch.int64).view(B, 1)
    ranked = (tgt >= item_lo) & (tgt < n_items)
    t_safe = torch.where(ranked, tgt, torch.zeros_like(tgt))
    s_t = torch.gather(scores, 1, t_safe)
    ranked = ranked & ~torch.isnan(s_t)
    cand = (cols >= item_lo) & ~torch.isnan(scores)
    if excluded is not None:
        cand = cand & (~excluded | (cols == tgt))
    beats = cand & ((scores > s_t) | ((scores == s_t) & (cols < tgt)))
    rank = torch.where(ranked.view(B), beats.sum(1), torch.full((B,), -1, dtype=torch.int64, device=scores.device))
    return rank.to(torch.int32), cand.sum(1).to(torch.int32)


class AhnRecommender:
    """Recommender's queries for AHN, over per-id SENTENCE tables instead of latent tables.

    AHN's towers attend to each other, but not symmetrically (models/ahn/ahn_layers.py): the item side is pooled by
    GatedAttention alone and only the user side depends on the pair -- through two bilinear max-similarities, two masked
    softmaxes, one Linear + ReLU and the FM.  The BiLSTM encoder, nine tenths of the arithmetic, depends on the id only.
    refresh() therefore runs the encoder ONCE per id (AHN.encode_users / encode_items) and keeps, per user, the sentence
    vectors X and X @ Wt^T with the masks, and per item the pre-multiplied keys Ks, Kr and its own attention weights; a score
    is then the pair tail alone, one HIP launch per block (functional.ahn_pair_score*, csrc/ahn_pair.hip).  In f32 that is
    2 * Ru * Su * F * 4 bytes per user and (Ri * Si + Ri) * F * 4 per item: about 240 KB and 120 KB at the default shape.
    refresh() also keeps the items' transformed reviews r' (`item_rows` [I, Ri, F], from the same sentence vectors: the encoder
    still runs once per id) for sentences(): Ri * F * 4 bytes more per item, about 12 KB on top of the 120 KB.

    `cache`: a data.DeviceSentenceCache of the sentence split, or pass `user` / `item` = per-id word-id tensors [N, R, S, W] on
    the model's device (row 0 = the padding id).  The tables are read by the PLAIN rule: the first rv_num slots of an id's row, as
    a valid or test example reads them (DeviceSentenceCache.gather(..., leave_one_out=False)); masks are data.sentence_masks.

    The t_out rule: the reference's max over the words has a zero candidate that depends on the BATCH's longest sentence per
    side, so a cached sentence vector needs one fixed output length.  refresh() takes, per side, the longest clamped sentence of
    the whole table (functional.lstm_t_out, on the device).  A table score then equals AHN.forward on a plain-gathered batch
    whenever that batch's longest sentence per side equals the table's.

    topk / rank / evaluate have Recommender's semantics (score descending, ties by the lower item id, item 0 never recommended,
    -1 / -inf fill, the target never excluded, rank -1 for the padding item, an id outside the table or a NaN score).  They
    select over the dense block of score_all with a torch composition (select_topk: stable sorts; rank_in_block: compare and
    count): the top-K and rank kernels of csrc/pair_score.hip score from latent rows internally and take no score block.

    `stale` is Recommender's: torch version counters, blind to raw-pointer updates."""

    def __init__(self, model, cache=None, *, user=None, item=None):
        if type(model).__name__ != "AHN":
            raise ValueError(f"AhnRecommender serves AHN, not {type(model).__name__} (Recommender serves {sorted(KINDS)})")
        if cache is not None:
            R = int(cache.rv_num)
            user, item = cache.user_table[:, :R], cache.item_table[:, :R]
        if user is None or item is None:
            raise ValueError("AhnRecommender needs a DeviceSentenceCache or the per-id `user` / `item` word-id tensors [N, R, S, W]")
        if user.dim() != 4 or item.dim() != 4:
            raise ValueError(f"AHN reads [N, R, S, W] sentences per id, got {tuple(user.shape)} / {tuple(item.shape)}")
        self.model, self.user, self.item = model, user, item
        self.n_users, self.n_items = user.shape[0], item.shape[0]
        self.item_lo = 1                     # the padding id 0 is never recommended
        self.user_state = self.item_state = self.head = None
        self.item_rows = self.explain_head = None      # r' [I, Ri, F] and the FM's q block: what sentences() reads beyond the score's
        self.t_out = None                    # (user, item): each side's fixed output length, device int32 [1] (words() re-encodes with it)
        self._versions = None

    # ------------------------------------------------------------------ the tables
    def refresh(self, chunk: int = 32) -> "AhnRecommender":
        """Encodes all users and all items, `chunk` ids (chunk * R * S sentences) at a time, into the state tables; eval
        semantics, no autograd, the model's mode is restored.  Call it again after the parameters change."""
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        from . import data as D
        m = self.model
        states, t_outs = [], []
        with RF.eval_mode(m):
            for docs, n, state_of in ((self.user, self.n_users, m.user_state), (self.item, self.n_items, m.item_state)):
                if not docs.is_cuda:
                    raise RuntimeError(f"the per-id sentence tables must live on a HIP device (got {docs.device}); there is no CPU path")
                t_out = RF.lstm_t_out(D.sentence_masks(docs, PAD)[0].reshape(-1), docs.shape[-1])
                t_outs.append(t_out)
                fields = None
                for a in range(0, n, chunk):
                    revs = docs[a:a + chunk].to(torch.int64).contiguous()
                    lens, sent_masks, rev_masks = D.sentence_masks(revs, PAD)
                    ids = torch.arange(a, a + revs.shape[0], dtype=torch.int64, device=revs.device)
                    sents = m._encode_side(revs, lens, t_out)      # the encoder runs once per id: the state and r' both come from it
                    rows = state_of(sents, sent_masks, rev_masks, ids)
                    extra = [m.item_reviews(sents, sent_masks)] if state_of == m.item_state else []
                    if fields is None:
                        fields = [torch.empty(n, *t.shape[1:], dtype=t.dtype, device=t.device) for t in (*rows, *extra)]
                    for dst, t in zip(fields, (*rows, *extra)):
                        dst[a:a + t.shape[0]] = t
                states.append(type(rows)(*fields[:len(rows)]))
            self.user_state, self.item_state = states
            self.item_rows = fields[-1]
            self.head, self.explain_head = m.pair_head(), m.explain_head()
            self.t_out = tuple(t_outs)
        self._versions = [p._version for p in m.parameters()]
        return self

    stale = Recommender.stale
    seen_from = staticmethod(Recommender.seen_from)

    def _tables(self):
        if self.user_state is None:
            raise RuntimeError("AhnRecommender.refresh() has not been called: there are no sentence tables yet")
        return self.user_state, self.item_state, self.head

    def _device(self):
        return self._tables()[0].X.device

    # ------------------------------------------------------------------ the queries
    def score(self, u_ids: torch.Tensor, i_ids: torch.Tensor) -> torch.Tensor:
        """Predicted ratings [B] of the pairs (u_ids[b], i_ids[b]): the pair tail over the tables, one launch."""
        us, its, head = self._tables()
        return RF.ahn_pair_score(us, its, head, u_ids, i_ids)

    def score_all(self, u_ids: torch.Tensor) -> torch.Tensor:
        """Predicted ratings [len(u_ids), I] of the given users against every item id (column 0 is the padding id), bit for bit
        what score() gives for each pair."""
        us, its, head = self._tables()
        (u_ids,) = RF.sanitize_ids([(u_ids, self.n_users, PAD)])
        return RF.ahn_pair_score_dense(us, its, head, u_ids)

    def attention(self, u_ids: torch.Tensor, i_ids: torch.Tensor):
        """The model's four weight arrays for the pairs, without the encoder: (user_sent_weights [B, Ru, Su], item_sent_weights
        [B, Ri, Si], user_review_weights [B, Ru], item_review_weights [B, Ri]) -- AHN.forward's outputs 1..4."""
        us, its, head = self._tables()
        u_ids, i_ids = RF.sanitize_ids([(u_ids, self.n_users, PAD), (i_ids, self.n_items, PAD)])
        _, w, v = RF.ahn_pair_score(us, its, head, u_ids, i_ids, weights=True)
        return w, its.item_sent_weights.index_select(0, i_ids), v, its.item_review_weights.index_select(0, i_ids)

    def sentences(self, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int = 256) -> SentenceContributions:
        """AHN's answer to "why": for the pairs (u_ids[b], i_ids[b]), `chunk` pairs per launch, from the tables alone
        (functional.ahn_pair_explain, csrc/ahn_explain.hip) -- the score and the four weight arrays, what every user sentence and
        review adds to the score (gradient x input of the sentence vector, followed through both softmaxes and both
        max-similarities; *_fixed holds the attention weightings constant), WHICH item sentence each user sentence matched and
        which item review each user review, what the matched item sentences / reviews add through that match, and the item's own
        reviews under its own weights (held constant, as NARRE's are in Recommender.explain).  The id embeddings and the biases
        are the part of the score no text explains; no encoder runs and no autograd."""
        _check_pairs(u_ids, i_ids, chunk, self._tables)
        us, its, head = self._tables()
        u_ids, i_ids = RF.sanitize_ids([(u_ids, self.n_users, PAD), (i_ids, self.n_items, PAD)])
        extra = RF.AhnExplainRows(self.item_rows, *self.explain_head)
        ex = RF.AhnPairExplanation(*_cat_chunks([RF.ahn_pair_explain(us, its, head, extra, u_ids[a:a + chunk], i_ids[a:a + chunk])
                                                 for a in range(0, u_ids.shape[0], chunk)]))
        return SentenceContributions(ex.score, ex.user_sent_weights, its.item_sent_weights.index_select(0, i_ids), ex.user_review_weights,
                                     its.item_review_weights.index_select(0, i_ids), ex.user_sentences, ex.user_sentences_fixed,
                                     ex.user_reviews, ex.user_text, ex.user_match.to(torch.int64), ex.review_match.to(torch.int64),
                                     ex.item_sentence_match, ex.item_review_match, ex.item_reviews, ex.item_text)

    def words(self, u_ids: torch.Tensor, i_ids: torch.Tensor, chunk: int = 8) -> WordContributions:
        """sentences() one level down: what every word of both sides' text adds to the score of the pairs (u_ids[b], i_ids[b]).
        Unlike sentences() this runs the encoder again: per chunk of pairs the pairs' word ids are gathered from the per-id
        tables, both sides are re-encoded with the TABLES' own t_out per side (so the sentence vectors are the tables' X), the
        tail runs under autograd on the detached sentence vectors, and the two sentence gradients go through the recurrence's
        word-saliency kernel (AHN.word_contributions, functional.lstm_seq_word_saliency; csrc/lstm_seq.hip) -- one launch for
        both sides when their word widths agree.  The item's words are explained through its full path: as the match of user
        sentences and through its own attention pooling.  Padding words, masked sentences and masked reviews hold exactly 0.

        NOT attributed: the biases (the LSTM's b_ih + b_hh are no part of x W_ih^T, and the linear layers' and the FM's are no
        part of any word), the id embeddings, and the dependence of the attention on routing ties -- each max (over the words,
        and both max-similarities) passes its gradient to the one candidate the forward picked, so where two candidates tie a
        word's share depends on which was picked, and the zero candidate of the max over the words takes no gradient.

        `chunk` pairs are encoded at a time.  The encoder's state, the bias-free projection and the projection the recurrence
        reads come to 28 * Hh * W * 4 bytes per sentence ((8 + 2 + 2) Hh floats of state and twice 8 Hh per word): about
        336 KB per sentence and 67 MB per pair of 200 sentences at the default shape (Hh 150, W 20).  The default of 8 pairs
        keeps a chunk near half of the 1 GiB that the input projection's operands may span (15 would still fit; the
        embedded words and the autograd tail need room too)."""
        _check_pairs(u_ids, i_ids, chunk, self._tables)
        from . import data as D
        u_ids, i_ids = RF.sanitize_ids([(u_ids, self.n_users, PAD), (i_ids, self.n_items, PAD)])
        parts = []
        for a in range(0, u_ids.shape[0], chunk):
            pu, pi = u_ids[a:a + chunk], i_ids[a:a + chunk]
            ur, ir = self.user.index_select(0, pu).to(torch.int64), self.item.index_select(0, pi).to(torch.int64)
            (ul, usm, urm), (il, ism, irm) = D.sentence_masks(ur, PAD), D.sentence_masks(ir, PAD)
            parts.append(self.model.word_contributions(ur, ir, usm, ism, ul, il, urm, irm, pu, pi, *self.t_out)[:5])
        score, uw, iw, us_, is_ = _cat_chunks(parts)
        return WordContributions(score, uw.sum(-1), iw.sum(-1), us_, is_, uw, iw)

    def topk(self, u_ids: torch.Tensor, k: int, exclude=None):
        """Recommender.topk over score_all's block (select_topk)."""
        scores = self.score_all(u_ids)
        (u_ids,) = RF.sanitize_ids([(u_ids, self.n_users, PAD)])
        return select_topk(scores, k, exclusion_mask(exclude, u_ids, self.n_items), self.item_lo)

    def rank(self, u_ids: torch.Tensor, i_ids: torch.Tensor, exclude=None):
        """Recommender.rank over score_all's block (rank_in_block): one row of I scores per pair."""
        scores = self.score_all(u_ids)
        (u_ids,) = RF.sanitize_ids([(u_ids, self.n_users, PAD)])
        return rank_in_block(scores, i_ids.to(scores.device), exclusion_mask(exclude, u_ids, self.n_items), self.item_lo)

    def evaluate(self, pairs, ks=(5, 10, 20), exclude=None, chunk: int = 256) -> dict:
        """Recommender.evaluate: rank_metrics of held-out pairs, ranked `chunk` pairs (chunk x I scores) at a time."""
        return _evaluate(self, pairs, ks, exclude, chunk)


# ---------------------------------------------------------------------------------------------------------------- the "why" lists
def _vocabulary(data_dir):
    """token id -> word from meta.pkl's indexlizer (_vocab._token2id), or None where it cannot be read."""
    from . import data as D
    try:
        ix = D.load_pickle(os.path.join(data_dir, "meta.pkl"))["indexlizer"]
        t2i = getattr(getattr(ix, "_vocab", ix), "_token2id", None)
        return {int(i): str(t) for t, i in t2i.items()} if isinstance(t2i, dict) else None
    except Exception:
        return None


def _kept_pairs(u_ids, items):
    """For the users u_ids [n_u] and their recommended items [n_u, k] (CPU, -1 = fill): the kept pairs (pu, pi) on u_ids' device,
    each pair's place (row, slot) in the output, and the empty "why" skeleton -- per user one None per kept item."""
    keep = items >= 0
    rows, cols = keep.nonzero(as_tuple=True)
    why = [[None] * int(keep[r].sum()) for r in range(items.shape[0])]
    places = list(zip(rows.tolist(), (keep.cumsum(1) - 1)[rows, cols].tolist()))
    return u_ids[rows.to(u_ids.device)], items[rows, cols].to(u_ids.device), places, why


def _fill(why, places, **cols):
    """Writes one entry per pair, {name: cols[name][p]}, to the pair's place in the skeleton."""
    for p, (r, slot) in enumerate(places):
        why[r][slot] = {name: col[p] for name, col in cols.items()}
    return why


def _entries(top, word=None, mid=(), tail=(), width=None):
    """The JSON entries of every pair from top_tokens' (position, id, weight) [P, n']: per kept position
    [position] + [id] + mid + [weight] + tail, entries of weight 0.0 dropped.  width: the position splits into [position //
    width, position % width]; word: id -> what stands for it; mid / tail: further columns [P, n'], tensors or nested lists."""
    pos, ids, weight = (t.cpu().tolist() for t in top)
    mid, tail = ([c.cpu().tolist() if torch.is_tensor(c) else c for c in cols] for cols in (mid, tail))
    place = (lambda q: [q]) if width is None else (lambda q: [q // width, q % width])
    return [[place(q) + [word(t) if word else t] + [c[p][k] for c in mid] + [x] + [c[p][k] for c in tail]
             for k, (q, t, x) in enumerate(zip(pos[p], ids[p], weight[p])) if x != 0.0] for p in range(len(pos))]


def _word_of(words):
    return (lambda t: words.get(t, t)) if words else None


def _token_entries(tokens, table, ids, n, words, gate=None):
    """Per pair the n tokens of largest |weight| as [position, word, weight] (+ [gate at the position])."""
    top = top_tokens(tokens, table.index_select(0, ids).to(torch.int64), n)
    return _entries(top, _word_of(words), tail=() if gate is None else [torch.gather(gate, 1, top[0])])


def _review_entries(contrib, att, rids, ids, n):
    """Per pair the n reviews of largest |contribution| as [slot, counterpart id (-1 where the cache has none), attention,
    contribution]."""
    rid = rids.index_select(0, ids).to(torch.int64) if rids is not None else torch.full_like(contrib, -1, dtype=torch.int64)
    top = top_tokens(contrib, rid, n)
    return _entries(top, mid=[torch.gather(att, 1, top[0])])


def _why(rec, u_ids, items, n, words):
    """The "why" lists of --explain for the users u_ids [n_u] and their recommended items [n_u, k] (CPU, -1 = fill)."""
    pu, pi, places, why = _kept_pairs(u_ids, items)
    if not places:
        return why
    ex, c = rec.explain(pu, pi), rec.cache
    cols = {"user_tokens": _token_entries(ex.user_tokens, c.user, pu, n, words),
            "item_tokens": _token_entries(ex.item_tokens, c.item, pi, n, words)}
    if ex.item_reviews is not None:
        cols["item_reviews"] = _review_entries(ex.item_reviews, ex.item_review_weights, c.item_rids, pi, n)
    return _fill(why, places, **cols)


def _why_attention(rec, u_ids, items, n, words):
    """The "why" lists of --attention for the users u_ids [n_u] and their recommended items [n_u, k] (CPU, -1 = fill): per item
    the n entries of largest |tokens| on each side as [position, word, weight, local_gate]."""
    pu, pi, places, why = _kept_pairs(u_ids, items)
    if not places:
        return why
    at, c = rec.attention(pu, pi), rec.cache
    return _fill(why, places, user_tokens=_token_entries(at.user_tokens, c.user, pu, n, words, at.user_local_gate),
                 item_tokens=_token_entries(at.item_tokens, c.item, pi, n, words, at.item_local_gate),
                 user_global_gate=at.user_global_gate.cpu().tolist(), item_global_gate=at.item_global_gate.cpu().tolist())


def _why_contributions(rec, u_ids, items, n, words):
    """The "why" lists of --contributions for the users u_ids [n_u] and their recommended items [n_u, k] (CPU, -1 = fill): per
    item and side the n tokens of largest |weight| as [slot-major position, word, weight] and the n reviews of largest
    |contribution| as [slot, counterpart id (-1 where the cache has none), attention, contribution]."""
    pu, pi, places, why = _kept_pairs(u_ids, items)
    if not places:
        return why
    co, c = rec.contributions(pu, pi), rec.cache
    return _fill(why, places, user_tokens=_token_entries(co.user_tokens, c.user, pu, n, words),
                 item_tokens=_token_entries(co.item_tokens, c.item, pi, n, words),
                 user_reviews=_review_entries(co.user_reviews, co.user_review_weights, getattr(c, "user_rids", None), pu, n),
                 item_reviews=_review_entries(co.item_reviews, co.item_review_weights, getattr(c, "item_rids", None), pi, n))


def _why_sentences(rec, u_ids, items, n, words, n_words=None):
    """The "why" lists of --sentences for the users u_ids [n_u] and their recommended items [n_u, k] (CPU, -1 = fill): per item
    the n user sentences of largest |contribution| as [review slot, sentence slot, weight, contribution, matched item review
    slot, matched item sentence slot] (with a vocabulary: + the sentence's words and the matched item sentence's words, token 0
    dropped), the n matched item sentences of largest |match contribution| as [review slot, sentence slot, item_sent_weight,
    match contribution], and both sides' n reviews of largest |contribution| as [slot, weight, contribution].  With n_words
    (--words) every user and item sentence entry ends with its n_words words of largest |contribution| as [position, word,
    contribution] (AhnRecommender.words; the item's through its full path), zeros dropped."""
    pu, pi, places, why = _kept_pairs(u_ids, items)
    if not places:
        return why
    sc = rec.sentences(pu, pi)
    wc = rec.words(pu, pi) if n_words is not None else None
    Su, Si = sc.user_sentences.shape[2], sc.item_sentence_match.shape[2]

    def picked(t, pos):
        """the rows [P, n', width] of the flat sentence slots pos [P, n'] out of t [P, R, S, width]"""
        return torch.gather(t.reshape(t.shape[0], -1, t.shape[-1]), 1, pos.view(*pos.shape, 1).expand(-1, -1, t.shape[-1]))

    def sent_words(table, ids, pos):
        """per pair and picked sentence its words, token 0 dropped"""
        sents = picked(table.index_select(0, ids).to(torch.int64), pos).cpu().tolist()
        return [[[words.get(t, t) for t in s if t != PAD] for s in row] for row in sents]

    def top_words(contrib, table, ids, pos):
        """per pair and picked sentence its n_words weightiest words as [position, word, contribution]"""
        c, toks = picked(contrib, pos), picked(table.index_select(0, ids).to(torch.int64), pos)
        t = c.abs().topk(min(n_words, c.shape[-1]), dim=-1).indices
        flat = _entries([x.flatten(0, 1) for x in (t, torch.gather(toks, 2, t), torch.gather(c, 2, t))], _word_of(words))
        return [flat[p * pos.shape[1]:(p + 1) * pos.shape[1]] for p in range(pos.shape[0])]

    top = top_tokens(sc.user_sentences, sc.user_sent_weights, n)
    hit = torch.gather(sc.user_match.reshape(top[0].shape[0], -1), 1, top[0])                 # the matched flat item sentence
    tail = [hit.cpu() // Si, hit.cpu() % Si]
    if words:
        tail += [sent_words(rec.user, pu, top[0]), sent_words(rec.item, pi, hit)]
    if wc is not None:
        tail.append(top_words(wc.user_words, rec.user, pu, top[0]))
    user_sentences = _entries(top, width=Su, tail=tail)
    top = top_tokens(sc.item_sentence_match, sc.item_sent_weights, n)
    item_sentences = _entries(top, width=Si, tail=[top_words(wc.item_words, rec.item, pi, top[0])] if wc is not None else ())
    return _fill(why, places, user_sentences=user_sentences,
                 user_reviews=_entries(top_tokens(sc.user_reviews, sc.user_review_weights, n)), item_sentences=item_sentences,
                 item_reviews=_entries(top_tokens(sc.item_reviews, sc.item_review_weights, n)))


# ---------------------------------------------------------------------------------------------------------------- CLI
# the flags that add "why" to every line of --out: the models each covers, and the function of its lists
_WHY_FLAGS = {"explain": (("deepconn", "narre"), _why), "attention": (("dual_att",), _why_attention),
              "contributions": (("simple_siamese",), _why_contributions), "sentences": (("ahn",), _why_sentences)}


def parse_cli(argv=None):
    ap = argparse.ArgumentParser(prog="python -m review_based_recommender_amd.recommend",
                                 description="top-K recommendations of a trained model for every user of its dataset")
    ap.add_argument("--model", required=True, choices=sorted(KINDS.values()) + ["ahn"])
    ap.add_argument("--config", required=True, help="the flat JSON config the model was trained with (trainer.py)")
    ap.add_argument("--checkpoint", required=True, help="best_model.pt written by the trainer")
    ap.add_argument("--k", type=int, default=10, help="items per user (1..128)")
    ap.add_argument("--exclude-train", action="store_true", help="never recommend an item the user rated in the training split")
    ap.add_argument("--out", help="output file, one JSON line per user (required unless --eval-split is given)")
    ap.add_argument("--eval-split", choices=["valid", "test"], help="rank this split's held-out (user, item) pairs: HR / NDCG / MRR / AUC")
    ap.add_argument("--ks", help="cut-offs K of hr@K / ndcg@K with --eval-split, comma-separated (default 5,10,20)")
    ap.add_argument("--metrics-out", help="file for the one JSON line of metrics of --eval-split (default: stdout)")
    ap.add_argument("--explain", type=int, metavar="N", help="with --out: add \"why\" to every line, the N weightiest tokens (and, "
                    "for NARRE, reviews) behind each recommended item; deepconn and narre only")
    ap.add_argument("--attention", type=int, metavar="N", help="with --out: add \"why\" to every line, the N weightiest tokens of each "
                    "side behind each recommended item with their local gates, followed through both attention gates; dual_att only")
    ap.add_argument("--contributions", type=int, metavar="N", help="with --out: add \"why\" to every line, the N weightiest tokens and "
                    "reviews of each side behind each recommended item, followed through the review attention; simple_siamese only")
    ap.add_argument("--sentences", type=int, metavar="N", help="with --out: add \"why\" to every line, the N weightiest user sentences "
                    "behind each recommended item with the item sentence each matched, the matched item sentences and both sides' "
                    "reviews; ahn only")
    ap.add_argument("--words", type=int, metavar="N", help="with --sentences: every user and item sentence of \"why\" also carries "
                    "its N weightiest words with their contributions, followed through the BiLSTM; ahn only")
    ap.add_argument("--chunk", type=int, default=256, help="ids encoded / users ranked per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reference-quirks", action="store_true", help="as for the trainer: kernel_sizes=[3] (NARRE hidden_dim=150)")
    a = ap.parse_args(argv)
    if not 1 <= a.k <= 128:
        ap.error("--k must be in 1..128")
    if a.chunk < 1:
        ap.error("--chunk must be at least 1")
    for flag, (models, _) in _WHY_FLAGS.items():
        if getattr(a, flag) is None:
            continue
        if getattr(a, flag) < 1:
            ap.error(f"--{flag} must be at least 1")
        if a.out is None:
            ap.error(f"--{flag} adds to the lines of --out: give --out")
        if a.model not in models:
            ap.error(f"--{flag} covers {' and '.join(models)} ({a.model}: --{next(f for f, (m, _) in _WHY_FLAGS.items() if a.model in m)})")
    if a.words is not None:
        if a.words < 1:
            ap.error("--words must be at least 1")
        if a.model != "ahn":
            ap.error("--words covers ahn (it adds to --sentences)")
        if a.sentences is None:
            ap.error("--words adds to the sentences of --sentences: give --sentences")
    if a.eval_split is None:
        if a.out is None:
            ap.error("--out is required unless --eval-split is given")
        if a.ks is not None or a.metrics_out is not None:
            ap.error("--ks and --metrics-out belong to --eval-split")
    try:
        a.ks = tuple(int(k) for k in ("5,10,20" if a.ks is None else a.ks).split(","))
    except ValueError:
        ap.error(f"--ks must be comma-separated integers, got {a.ks!r}")
    if any(not 1 <= k < 2 ** 31 for k in a.ks):
        ap.error("every K of --ks must be in 1..2^31-1")
    return a


def main(argv=None) -> int:
    a = parse_cli(argv)
    from . import data as D
    from .trainer import DEFAULTS, make_model, parse_args
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP path needs an MI355X: there is no CPU fallback")
    cfg = parse_args(a.config)
    for key, v in DEFAULTS.items():
        if not hasattr(cfg, key):
            setattr(cfg, key, v)
    dev = torch.device(a.device)
    review_split = a.model in ("narre", "simple_siamese")
    if a.model == "ahn":
        ds = D.SentenceDataset(cfg.data_dir, "train")
    else:
        ds = D.ReviewDataset(cfg.data_dir, "train") if review_split else D.DocDataset(cfg.data_dir, "train", with_ids=a.model == "deepconn")
    # the review split's meta holds as many reviews per id as the id wrote: DeviceReviewCache's first rv_num slots are what a
    # valid / test example reads
    if a.model == "ahn":
        cache = D.DeviceSentenceCache(ds, dev)
    else:
        cache = D.DeviceReviewCache(ds, dev) if review_split else D.DeviceDocCache(ds, dev)
    model = make_model(a.model, cfg, ds, a.reference_quirks)
    ck = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    model.load_state_dict(ck["model"] if "model" in ck else ck)
    model.to(dev).eval()
    # AHN: sentence tables and the pair tail (AhnRecommender); a chunk of ids is chunk * R * S sentences through the encoder
    rec = AhnRecommender(model, cache).refresh(chunk=min(a.chunk, 32)) if a.model == "ahn" else Recommender(model, cache).refresh(chunk=a.chunk)
    seen = Recommender.seen_from(ds.examples, rec.n_users, dev) if a.exclude_train else None
    flag = next((f for f in _WHY_FLAGS if getattr(a, f) is not None), None)        # at most one: each covers other models
    words = _vocabulary(cfg.data_dir) if flag is not None else None
    if a.out is not None:
        with open(a.out, "w") as f:
            for lo in range(1, rec.n_users, a.chunk):
                u_ids = torch.arange(lo, min(lo + a.chunk, rec.n_users), dtype=torch.int64, device=dev)
                items, scores = rec.topk(u_ids, a.k, exclude=seen)
                items, scores = items.cpu(), scores.cpu()
                why = None
                if flag is not None:
                    why = _WHY_FLAGS[flag][1](rec, u_ids, items, getattr(a, flag), words, *([a.words] if a.words is not None else []))
                for r, u in enumerate(u_ids.tolist()):
                    keep = items[r] >= 0
                    line = {"user": u, "items": items[r][keep].tolist(), "scores": scores[r][keep].tolist()}
                    if why is not None:
                        line["why"] = why[r]
                    f.write(json.dumps(line) + "\n")
    if a.eval_split is not None:
        held_out = D.load_pickle(os.path.join(cfg.data_dir, f"{a.eval_split}_exmaples.pkl"))
        line = json.dumps(dict(rec.evaluate(held_out, a.ks, exclude=seen), split=a.eval_split, exclude_train=bool(a.exclude_train)))
        if a.metrics_out is not None:
            with open(a.metrics_out, "w") as f:
                f.write(line + "\n")
        else:
            print(line, flush=True)
    RF.check_id_errors(dev)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
