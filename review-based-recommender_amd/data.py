"""Readers for the reference's on-disk dataset format and a device-resident document cache.

Format (written by the reference's preprocess/divide_and_create_example_{doc,word}.py, read by its trainers):
  <data_dir>/meta.pkl             dict: user_num, item_num, indexlizer, and
      doc split  : user_docs, item_docs (id -> [doc_len] token ids), doc_len     (train_deepconn_pp.py:254-262)
      review split: rv_num, rv_len, user_reviews, item_reviews (id -> [rv_num][rv_len]),
                    user_rids, item_rids (id -> [rv_num] counterpart ids)          (train_narre.py:254-266)
      sentence split: rv_num, sent_num, word_num, user_reviews, item_reviews (id -> reviews, each [sent_num][word_num]),
                    user_rids, item_rids                                           (train_ahn.py:329-338)
  <data_dir>/{train,valid,test}_exmaples.pkl   (sic)  list of examples
      doc split  : [u_id, i_id, rating, u_doc, i_doc]                              (train_deepconn_pp.py:276)
      review split: 7-tuples (valid/test) or 8-tuples (train; the last field is dropped)  (train_narre.py:273-279)

`meta["indexlizer"]` is an instance of the reference's preprocess._tokenizer.Indexlizer holding function
references (nltk tokenizers, clean_str).  `load_pickle` resolves ONLY an allow-list of globals (plain containers of
builtins / collections and numpy's array reconstructors); every other class or function a pickle names -- importable or
not, `os.system` included -- becomes an inert placeholder: the object graph loads, nothing from it is executed, and only
`_vocab._token2id` (the vocabulary size) is read.

Parity status of the format: UNPINNED.  The reference holds no dataset fixture and its preprocess scripts need nltk, so
the layout above is restated from the trainers' read sites cited here; tests/make_dataset.py writes files of that layout.
The loader also validates every token / user / item id against its table once, at load time (`validate_ranges`).
"""
from __future__ import annotations

import importlib
import os
import pickle
from typing import Sequence

import torch


class _Placeholder:
    """Stands in for a class / function of a module that is not importable in this environment."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        else:
            self.__dict__["_state"] = state

    def __call__(self, *a, **k):
        raise RuntimeError("placeholder for an object of a module that is not importable here")


# globals a dataset pickle may legitimately reconstruct: containers and numpy arrays / scalars.  Nothing callable with a
# side effect is on the list; REDUCE on anything else calls a _Placeholder constructor, which does nothing.
_ALLOWED_GLOBALS = {
    "builtins": {"list", "dict", "tuple", "set", "frozenset", "int", "float", "complex", "str", "bytes", "bytearray",
                 "bool", "slice", "range", "object"},
    "collections": {"OrderedDict", "defaultdict", "Counter", "deque"},
    "numpy": {"ndarray", "dtype"},
    "numpy.core.multiarray": {"_reconstruct", "scalar"},
    "numpy._core.multiarray": {"_reconstruct", "scalar"},
    "numpy.core.numeric": {"_frombuffer"},
    "numpy._core.numeric": {"_frombuffer"},
}


class _TolerantUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if name in _ALLOWED_GLOBALS.get(module, ()):
            return getattr(importlib.import_module(module), name)
        return type(name, (_Placeholder,), {"__module__": module})


def load_pickle(path):
    with open(path, "rb") as f:
        return _TolerantUnpickler(f).load()


def vocab_size_of(indexlizer) -> int:
    """len(indexlizer._vocab)  (preprocess/_tokenizer.py:73-74: the size of _token2id)."""
    vocab = getattr(indexlizer, "_vocab", None)
    for holder in (vocab, indexlizer):
        t2i = getattr(holder, "_token2id", None) if holder is not None else None
        if t2i is not None:
            return len(t2i)
    if isinstance(indexlizer, int):
        return int(indexlizer)
    raise ValueError("cannot find the vocabulary (_vocab._token2id) in meta['indexlizer']")


def _check_range(values, limit: int, what: str) -> None:
    t = torch.as_tensor(values, dtype=torch.int64)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= limit):
        raise IndexError(f"{what}: ids span [{int(t.min())}, {int(t.max())}] but the table has {limit} rows "
                         "(vocabulary / meta.pkl mismatch?)")


def get_mask(tensor: torch.Tensor, padding_idx: int = 0) -> torch.Tensor:
    """utils.py:30-42 -- bool mask, False where the token equals padding_idx."""
    return tensor != padding_idx


def _rows(mapping, n, what):
    """id -> row table as a list of length n (dicts keyed by id or sequences indexed by id)."""
    if isinstance(mapping, dict):
        any_row = next(iter(mapping.values()))
        zero = [[0] * len(any_row[0]) for _ in any_row] if isinstance(any_row[0], (list, tuple)) else [0] * len(any_row)
        return [mapping.get(i, zero) for i in range(n)]
    if len(mapping) < n:
        raise ValueError(f"{what} has {len(mapping)} rows for {n} ids")
    return list(mapping[:n])


class DocDataset(torch.utils.data.Dataset):
    """doc split (DeepCoNN / D-ATT): examples are [u_id, i_id, rating, u_doc, i_doc].

    feed="docs" (the reference's): a batch carries its documents (collate_fn, train_deepconn_pp.py:281-292).
    feed="ids": a batch is (u_ids int64, i_ids int64, ratings f32) -- also for the D-ATT split (with_ids=False), whose
    documents are then gathered by id -- and the documents come from meta.pkl's per-id tables on the device
    (DeviceDocCache.gather).  That is only the same batch when every example's documents ARE meta's documents for its ids
    (preprocess/divide_and_create_example_doc.py:261-262 builds them so); the id feed checks it once, at load time, and
    refuses a split that differs (ValueError naming the first such example)."""

    FEEDS = ("docs", "ids")

    def __init__(self, data_dir: str, set_name: str, with_ids: bool = True, feed: str = "docs"):
        if feed not in self.FEEDS:
            raise ValueError(f"feed must be one of {self.FEEDS}, got {feed!r}")
        meta = load_pickle(os.path.join(data_dir, "meta.pkl"))
        self.user_num, self.item_num = meta["user_num"], meta["item_num"]
        self.doc_len = meta["doc_len"]
        self.vocab_size = vocab_size_of(meta["indexlizer"])
        self.user_docs, self.item_docs = meta["user_docs"], meta["item_docs"]
        self.examples = load_pickle(os.path.join(data_dir, f"{set_name}_exmaples.pkl"))
        self.set_name = set_name
        self.with_ids = with_ids
        self.feed = feed
        self.validate_ranges()
        if feed == "ids":
            self.check_documents_match_meta()

    def validate_ranges(self) -> None:
        """Every token / user / item id of the split against its table, once at load time: the IndexError nn.Embedding
        would raise on the first bad batch (models/deepconn/layers.py:23), up front.  A model fed from a validated dataset
        may run with validate_ids = False."""
        _check_range([e[0] for e in self.examples], self.user_num, "user ids")
        _check_range([e[1] for e in self.examples], self.item_num, "item ids")
        _check_range([e[3] for e in self.examples], self.vocab_size, "user document tokens")
        _check_range([e[4] for e in self.examples], self.vocab_size, "item document tokens")

    def check_documents_match_meta(self) -> None:
        """The id feed's precondition: example k's u_doc / i_doc equal meta's user_docs[u_id] / item_docs[i_id]."""
        urows = _rows(self.user_docs, self.user_num, "user_docs")
        irows = _rows(self.item_docs, self.item_num, "item_docs")
        for k, e in enumerate(self.examples):
            for side, rows, idx, doc in (("u_doc", urows, int(e[0]), e[3]), ("i_doc", irows, int(e[1]), e[4])):
                if list(doc) != list(rows[idx]):
                    which = "user_docs" if side == "u_doc" else "item_docs"
                    raise ValueError(f"{self.set_name} example {k}: its {side} is not meta.pkl's {which}[{idx}], so the id feed "
                                     "would train on other documents than the example's (use feed='docs')")

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i):
        return self.examples[i][:3] if self.feed == "ids" else self.examples[i][:5]

    def collate_fn(self, batch):
        """train_deepconn_pp.py:281-292 (with ids) / train_dual_att.py:273-280 (docs and ratings only); the id feed's batch
        is id_collate_fn's."""
        if self.feed == "ids":
            return self.id_collate_fn(batch)
        u_ids, i_ids, ratings, u_docs, i_docs = zip(*batch)
        u_docs, i_docs = torch.LongTensor(u_docs), torch.LongTensor(i_docs)
        ratings = torch.FloatTensor(ratings)
        if not self.with_ids:
            return u_docs, i_docs, ratings
        return (u_docs, i_docs, get_mask(u_docs), get_mask(i_docs), torch.LongTensor(u_ids), torch.LongTensor(i_ids), ratings)

    @staticmethod
    def id_collate_fn(batch):
        """(u_ids int64 [B], i_ids int64 [B], ratings f32 [B]) of examples (or their first three fields)."""
        u_ids, i_ids, ratings = zip(*[e[:3] for e in batch])
        return torch.LongTensor(u_ids), torch.LongTensor(i_ids), torch.FloatTensor(ratings)


def _first_slots(lists, idx: int, n: int, pad):
    """The first n entries of id idx's list in meta (absent id: none), padded with `pad`: truncate_pad_tokens of the reference's
    preprocess, which is all an example ever reads of a per-id list."""
    row = list((lists.get(idx, ()) if isinstance(lists, dict) else lists[idx])[:n])
    return row + [pad] * (n - len(row))


def _review_shape(ds):
    """The shape of one review of the split `ds` was read from: (rv_len,) tokens on the review split, (sent_num, word_num) -- sentences
    of words -- on the sentence split."""
    return (int(ds.sent_num), int(ds.word_num)) if hasattr(ds, "sent_num") else (int(ds.rv_len),)


def _fit(x, shape):
    """The nested list `x` truncated / zero-padded to `shape` on every axis (a list of lists)."""
    n = shape[0]
    if len(shape) == 1:
        x = list(x[:n])
        return x + [0] * (n - len(x))
    rows = [_fit(r, shape[1:]) for r in list(x)[:n]]
    return rows + [_fit((), shape[1:]) for _ in range(n - len(rows))]


def _fill(dst, x) -> None:
    """The ragged nested list `x` into the zeroed numpy array `dst`, left-aligned on every axis.  A rectangular (sub)list is one
    array assignment; only where the list is ragged does the copy descend a level."""
    import numpy as np
    try:
        a = np.asarray(x, dtype=np.int64)
    except (ValueError, TypeError):          # ragged below this level
        a = None
    if a is not None and a.ndim == dst.ndim:
        dst[tuple(slice(0, n) for n in a.shape)] = a
    elif a is None or a.size:
        for j, sub in enumerate(x):
            _fill(dst[j], sub)


def review_example_from_meta(ds, u_id: int, i_id: int, leave_one_out: bool):
    """Fields 3..6 (u_revs, i_revs, u_rids, i_rids) of the example of the pair, from meta's per-id lists alone -- on the review
    split and, with a review of sent_num x word_num tokens, on the sentence split (_review_shape).
    leave_one_out (the train split, preprocess/divide_and_create_example_word.py:263-285, ..._sent.py:262-300): the id's review of
    the pair's counterpart -- the first one in its rid list -- is removed before the list is truncated / padded to rv_num; removing
    one slot and keeping rv_num reads the first rv_num + 1 entries only, and a match at or beyond slot rv_num changes nothing.
    Without leave_one_out (valid / test, :306-323), or without such a review, the first rv_num slots as they are."""
    R, shape = ds.rv_num, _review_shape(ds)
    zero = _fit((), shape)
    out = []
    for revs, rids, own, other in ((ds.user_reviews, ds.user_rids, u_id, i_id), (ds.item_reviews, ds.item_rids, i_id, u_id)):
        rv = [_fit(r, shape) for r in _first_slots(revs, own, R + 1, zero)]
        rd = [int(x) for x in _first_slots(rids, own, R + 1, 0)]
        d = R
        if leave_one_out and other > 0 and other in rd[:R]:
            d = rd.index(other)
        out.append(([rv[q + (q >= d)] for q in range(R)], [rd[q + (q >= d)] for q in range(R)]))
    (u_revs, u_rids), (i_revs, i_rids) = out
    return u_revs, i_revs, u_rids, i_rids


class ReviewDataset(torch.utils.data.Dataset):
    """review split (NARRE, SimpleSiamese): examples are (u_id, i_id, rating, u_revs, i_revs, u_rids, i_rids[, extra]).

    feed="examples" (the reference's): a batch carries its reviews (collate_fn, train_narre.py:316-330).
    feed="ids": a batch is (u_ids int64, i_ids int64, ratings f32) and the reviews are rebuilt on the device from meta.pkl's
    per-id lists (DeviceReviewCache).  That is only the same batch when every example IS what review_example_from_meta gives
    for its ids (the reference's preprocess builds them so); the id feed checks it once, at load time, and refuses a split
    that differs (ValueError naming the first such example and field)."""

    FEEDS = ("examples", "ids")

    def __init__(self, data_dir: str, set_name: str, feed: str = "examples"):
        if feed not in self.FEEDS:
            raise ValueError(f"feed must be one of {self.FEEDS}, got {feed!r}")
        meta = load_pickle(os.path.join(data_dir, "meta.pkl"))
        self.user_num, self.item_num = meta["user_num"], meta["item_num"]
        self.rv_num, self.rv_len = meta["rv_num"], meta["rv_len"]
        self.vocab_size = vocab_size_of(meta["indexlizer"])
        self.user_reviews, self.item_reviews = meta["user_reviews"], meta["item_reviews"]
        self.user_rids, self.item_rids = meta["user_rids"], meta["item_rids"]
        self.examples = load_pickle(os.path.join(data_dir, f"{set_name}_exmaples.pkl"))
        self.set_name = set_name
        self.feed = feed
        self.validate_ranges()
        if feed == "ids":
            self.check_examples_match_meta()

    def validate_ranges(self) -> None:
        _check_range([e[0] for e in self.examples], self.user_num, "user ids")
        _check_range([e[1] for e in self.examples], self.item_num, "item ids")
        _check_range([e[3] for e in self.examples], self.vocab_size, "user review tokens")
        _check_range([e[4] for e in self.examples], self.vocab_size, "item review tokens")
        _check_range([e[5] for e in self.examples], self.item_num, "user-side counterpart (item) ids")
        _check_range([e[6] for e in self.examples], self.user_num, "item-side counterpart (user) ids")

    def check_examples_match_meta(self) -> None:
        """The id feed's precondition: fields 3..6 of example k are review_example_from_meta of its ids -- leave-one-out for the
        train split, plain otherwise."""
        loo = self.set_name == "train"
        names = ("u_revs", "i_revs", "u_rids", "i_rids")
        for k, e in enumerate(self.examples):
            want = review_example_from_meta(self, int(e[0]), int(e[1]), loo)
            for name, got, ref in zip(names, e[3:7], want):
                got = [list(r) for r in got] if name.endswith("revs") else [int(x) for x in got]
                if got != ref:
                    rule = "with the pair's own review left out" if loo else "truncated / padded to rv_num"
                    raise ValueError(f"{self.set_name} example {k}: its {name} is not meta.pkl's list of id "
                                     f"{int(e[0]) if name[0] == 'u' else int(e[1])} {rule}, so the id feed would train on other "
                                     "reviews than the example's (use feed='examples')")

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i):
        if self.feed == "ids":
            return self.examples[i][:3]
        return self.examples[i][:7]     # train examples carry an 8th field that the trainer drops

    def collate_fn(self, batch):
        """train_narre.py:316-330; the id feed's batch is DocDataset.id_collate_fn's."""
        if self.feed == "ids":
            return DocDataset.id_collate_fn(batch)
        u_ids, i_ids, ratings, u_revs, i_revs, u_rids, i_rids = zip(*[e[:7] for e in batch])
        u_revs, i_revs = torch.LongTensor(u_revs), torch.LongTensor(i_revs)
        return (u_revs, i_revs, get_mask(u_revs), get_mask(i_revs), torch.LongTensor(u_ids), torch.LongTensor(i_ids),
                torch.LongTensor(u_rids), torch.LongTensor(i_rids), torch.FloatTensor(ratings))


class SentenceDataset(torch.utils.data.Dataset):
    """sentence split (AHN; written by preprocess/divide_and_create_example_sent.py, read by trainer/train_ahn.py:319-358): meta.pkl
    holds rv_num, sent_num, word_num and the per-id lists user_reviews / item_reviews (id -> reviews, each a list of sentences of
    word ids) and user_rids / item_rids; examples are (u_id, i_id, rating, u_revs, i_revs, u_rids, i_rids[, extra]).

    feed="examples" (the reference's): a batch carries its reviews -- collate_fn returns train_ahn.py:381-419's 7-tuple, zero-padded
    to [B, rv_num, sent_num, word_num] from lists that may hold fewer reviews, fewer sentences or shorter sentences.  Anything
    LONGER than that shape is refused at load time (the reference's collate would fail on its first such batch).
    feed="ids": a batch is (u_ids int64, i_ids int64, ratings f32) and the reviews are rebuilt on the device from meta.pkl's per-id
    lists (DeviceSentenceCache) under ReviewDataset's precondition, checked once at load time: every example, padded, IS what
    review_example_from_meta gives for its ids."""

    FEEDS = ("examples", "ids")
    FIELDS = ("u_revs", "i_revs", "u_rids", "i_rids")

    def __init__(self, data_dir: str, set_name: str, feed: str = "examples"):
        if feed not in self.FEEDS:
            raise ValueError(f"feed must be one of {self.FEEDS}, got {feed!r}")
        meta = load_pickle(os.path.join(data_dir, "meta.pkl"))
        self.user_num, self.item_num = meta["user_num"], meta["item_num"]
        self.rv_num, self.sent_num, self.word_num = int(meta["rv_num"]), int(meta["sent_num"]), int(meta["word_num"])
        self.vocab_size = vocab_size_of(meta["indexlizer"])
        self.user_reviews, self.item_reviews = meta["user_reviews"], meta["item_reviews"]
        self.user_rids, self.item_rids = meta["user_rids"], meta["item_rids"]
        self.examples = load_pickle(os.path.join(data_dir, f"{set_name}_exmaples.pkl"))
        self.set_name = set_name
        self.feed = feed
        self.check_example_shapes()
        self.validate_ranges()
        if feed == "ids":
            self.check_examples_match_meta()

    def check_example_shapes(self) -> None:
        """No example holds more than rv_num reviews (or rids), a review more than sent_num sentences, a sentence more than
        word_num words: the padded batch has no room for them."""
        R, S, W = self.rv_num, self.sent_num, self.word_num
        for k, e in enumerate(self.examples):
            for name, field in zip(self.FIELDS, e[3:7]):
                if len(field) > R:
                    raise ValueError(f"{self.set_name} example {k}: its {name} holds {len(field)} entries, more than rv_num = {R}")
                if name.endswith("rids"):
                    continue
                for j, review in enumerate(field):
                    if len(review) > S:
                        raise ValueError(f"{self.set_name} example {k}: review {j} of its {name} has {len(review)} sentences, "
                                         f"more than sent_num = {S}")
                    longest = max(map(len, review), default=0)
                    if longest > W:
                        raise ValueError(f"{self.set_name} example {k}: review {j} of its {name} has a sentence of {longest} "
                                         f"words, more than word_num = {W}")

    def validate_ranges(self) -> None:
        """As ReviewDataset.validate_ranges; the ragged reviews are walked example by example."""
        import itertools

        import numpy as np
        flat = itertools.chain.from_iterable
        _check_range([e[0] for e in self.examples], self.user_num, "user ids")
        _check_range([e[1] for e in self.examples], self.item_num, "item ids")
        for f, limit, what in ((3, self.vocab_size, "user review tokens"), (4, self.vocab_size, "item review tokens")):
            lo, hi = 0, -1
            for e in self.examples:
                t = np.fromiter(flat(flat(e[f])), dtype=np.int64)
                if t.size:
                    lo, hi = min(lo, int(t.min())), max(hi, int(t.max()))
            _check_range([lo, max(hi, 0)], limit, what)
        _check_range([x for e in self.examples for x in e[5]], self.item_num, "user-side counterpart (item) ids")
        _check_range([x for e in self.examples for x in e[6]], self.user_num, "item-side counterpart (user) ids")

    def padded(self, e):
        """Fields 3..6 of example `e` as zero-padded numpy arrays: ([R, S, W], [R, S, W], [R], [R]) int64."""
        import numpy as np
        R, S, W = self.rv_num, self.sent_num, self.word_num
        out = (np.zeros((R, S, W), np.int64), np.zeros((R, S, W), np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64))
        for dst, x in zip(out, e[3:7]):
            _fill(dst, x)
        return out

    def check_examples_match_meta(self) -> None:
        """The id feed's precondition: fields 3..6 of example k, padded to [R][S][W], are review_example_from_meta of its ids --
        leave-one-out for the train split, plain otherwise."""
        import numpy as np
        loo = self.set_name == "train"
        for k, e in enumerate(self.examples):
            want = review_example_from_meta(self, int(e[0]), int(e[1]), loo)
            for name, got, ref in zip(self.FIELDS, self.padded(e), want):
                if not np.array_equal(got, np.asarray(ref, dtype=np.int64)):
                    rule = "with the pair's own review left out" if loo else "truncated / padded to rv_num"
                    raise ValueError(f"{self.set_name} example {k}: its {name} is not meta.pkl's list of id "
                                     f"{int(e[0]) if name[0] == 'u' else int(e[1])} {rule}, so the id feed would train on other "
                                     "reviews than the example's (use feed='examples')")

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i):
        if self.feed == "ids":
            return self.examples[i][:3]
        return self.examples[i][:7]     # train examples carry an 8th field (the popped review) that the trainer drops

    def collate_fn(self, batch):
        """train_ahn.py:381-419: (u_revs [B, R, S, W] int64, i_revs, u_ids, i_ids, u_rids [B, R], i_rids, ratings f32), filled with
        numpy -- one array assignment per rectangular block -- instead of one tensor per sentence; the id feed's batch is
        DocDataset.id_collate_fn's."""
        if self.feed == "ids":
            return DocDataset.id_collate_fn(batch)
        import numpy as np
        B, R, S, W = len(batch), self.rv_num, self.sent_num, self.word_num
        revs = np.zeros((2, B, R, S, W), np.int64)
        rids = np.zeros((2, B, R), np.int64)
        for b, e in enumerate(batch):
            _fill(revs[0, b], e[3])
            _fill(revs[1, b], e[4])
            _fill(rids[0, b], e[5])
            _fill(rids[1, b], e[6])
        revs, rids = torch.from_numpy(revs), torch.from_numpy(rids)
        return (revs[0], revs[1], torch.LongTensor([e[0] for e in batch]), torch.LongTensor([e[1] for e in batch]),
                rids[0], rids[1], torch.FloatTensor([e[2] for e in batch]))


def _review_tables(reviews, rids, n: int, slots: int, T):
    """meta's per-id review lists -- ragged: an id has as many reviews as it wrote, and absent ids have none -- as rectangular
    tables of `slots` reviews per id: (int64 [n, slots, *T], int64 [n, slots]) on the host, zero-padded (pad token / rid 0).
    T: the shape of one review -- its token count, or (sent_num, word_num) on the sentence split."""
    import numpy as np
    shape = (T,) if isinstance(T, int) else tuple(T)
    tab = np.zeros((n, slots) + shape, dtype=np.int64)
    rid = np.zeros((n, slots), dtype=np.int64)
    for i in range(n):
        rv = _first_slots(reviews, i, slots, None)
        rd = _first_slots(rids, i, slots, None)
        k = sum(r is not None for r in rv)
        if k != sum(r is not None for r in rd):
            raise ValueError(f"id {i} has {k} reviews but {sum(r is not None for r in rd)} counterpart ids in meta.pkl")
        if k:
            rid[i, :k] = rd[:k]
            try:
                block = np.asarray(rv[:k], dtype=np.int64)
            except (ValueError, TypeError):          # ragged reviews
                block = None
            if block is not None and block.shape == (k,) + shape:
                tab[i, :k] = block
            else:                                    # reviews of another shape: truncated / zero-padded one by one
                tab[i, :k] = [_fit(r, shape) for r in rv[:k]]
    return torch.from_numpy(tab), torch.from_numpy(rid)


def _resident_tables(ds, side: str, slots: int, T, pad: int, device):
    """One side's ("user" / "item") resident pair for an id feed: int32 (reviews [N, slots, *T], rids [N, slots]) on `device` from
    meta's ragged lists (_review_tables), tokens range-checked against the vocabulary and rids against the other side's id count,
    row 0 all pad."""
    n_other = ds.item_num if side == "user" else ds.user_num
    tab, rid = _review_tables(getattr(ds, f"{side}_reviews"), getattr(ds, f"{side}_rids"), getattr(ds, f"{side}_num"), slots, T)
    _check_range(tab, ds.vocab_size, f"meta.pkl {side}_reviews tokens")
    _check_range(rid, n_other, f"meta.pkl {side}_rids")
    tab[0] = pad                            # id 0 is the padding id: the row a bad id is replaced by
    rid[0] = 0
    return tab.to(torch.int32).to(device), rid.to(torch.int32).to(device)


def _deliver(got, given, required: int):
    """The cpu restatement's results `got` under the gathers' output convention, `given` being what the caller passed for each: a
    tensor is copied into; the first `required` are handed over on None; the others on True and left out on None / False."""
    return tuple(dst.copy_(val) if torch.is_tensor(dst) else (val if dst is True or (dst is None and n < required) else None)
                 for n, (dst, val) in enumerate(zip(given, got)))


def _slots_torch(own, other, tab, rid, n_other: int, leave_one_out: bool):
    """The id feeds' rule on the host, one side: for own ids [B] with counterparts `other`, over the tables tab [N, R+1, ...] /
    rid [N, R+1], d = the FIRST j < R with rid[own][j] == other (leave_one_out and 0 < other < n_other; else R) and output slot q
    reads table slot q + (q >= d).  Returns (reviews [B, R, ...] int64, rids [B, R] int64)."""
    R = rid.shape[1] - 1
    _check_range(own, tab.shape[0], "ids of a gathered batch")
    q = torch.arange(R)
    rr = rid.index_select(0, own).to(torch.int64)                                   # [B, R + 1]
    hit = (rr[:, :R] == other[:, None]) & ((other > 0) & (other < n_other))[:, None] & bool(leave_one_out)
    d = torch.where(hit.any(1), hit.to(torch.int64).argmax(1), torch.full_like(own, R))
    src = q[None, :] + (q[None, :] >= d[:, None]).to(torch.int64)
    rows = tab.index_select(0, own).to(torch.int64)
    idx = src.view(*src.shape, *([1] * (rows.dim() - 2))).expand(-1, -1, *rows.shape[2:])
    return rows.gather(1, idx), rr.gather(1, src)


def sentence_masks(revs: torch.Tensor, pad: int = 0):
    """trainer/train_ahn.py:149-184 for word ids revs [.., R, S, W], on the tensor's device: (sentence lengths [.., R, S] int64 --
    the number of tokens != pad, get_sent_lengths counts and does not look for a prefix --, sentence masks [.., R, S] bool,
    review masks [.., R] bool).  The reference's masks are `token sum != 0`; token ids are non-negative, so that is `length > 0`
    and `any sentence non-empty`."""
    lens = (revs != pad).sum(-1)
    sent_masks = lens > 0
    return lens, sent_masks, sent_masks.any(-1)


class _IdFeed:
    """The id-feed protocol -- what GraphedTrainStep.from_ids / GraphedForward.from_ids, the trainer, NegativeFeed and InBatchFeed
    take: empty_inputs / gather / inputs for a batch of (u_ids, i_ids).  A feed states `order` (the names of its model's arguments,
    each a (user, item) pair), `like` ({name: (shape behind the batch dimension, dtype)}), `optional` (the names its cache
    produces only when asked), `kind` (its model, for messages) and _gather(u_ids, i_ids, **outputs) -> {name: stacked [2B, ...] or
    None}, how its cache's one launch is called: `outputs` gives per name a stacked tensor to write into, True (an optional output to
    allocate) or None (an optional output to leave out)."""

    optional = ("rev_masks", "rids", "ids")

    def _order(self, with_ids: bool = True):
        """`order` for DeviceDocCache's parameter `with_ids`: a feed bound to its model ignores it."""
        return self.order

    def _outputs(self, out, order):
        """_gather's `outputs` for the arguments `order`: allocated, or the stacked views of `out`; nothing else is produced."""
        if out is None:
            asked = {k: True for k in order if k in self.optional}
        elif len(out) != 2 * len(order):
            raise RuntimeError(f"out must be the {2 * len(order)} arguments of {self.kind}")
        else:
            asked = {k: _adjacent(out[2 * n], out[2 * n + 1]) for n, k in enumerate(order)}
        return {**dict.fromkeys(self.optional), **asked}

    def _gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, **outputs):
        """A feed over a `cache` with NAMES and gather(u_ids, i_ids, leave_one_out, **outputs); every other feed states its own."""
        return dict(zip(self.cache.NAMES, self.cache.gather(u_ids, i_ids, self.leave_one_out, **outputs)))

    def empty_inputs(self, B: int, with_ids: bool = True):
        """Zeroed tensors of inputs()' shapes and dtypes for B pairs (what a recorded step lays its input block out by)."""
        return tuple(torch.zeros((B, *self.like[k][0]), dtype=self.like[k][1], device=self.device)
                     for k in self._order(with_ids) for _ in range(2))

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, out=None, **kw):
        """The pairs' batch, stacked ({name: [2B, ...]}, user rows first).  `out`: the model's arguments to write into instead, each
        (user, item) pair adjacent in one allocation -- the input views of a recorded step."""
        return self._gather(u_ids, i_ids, **self._outputs(out, self._order()), **kw)

    def inputs(self, u_ids: torch.Tensor, i_ids: torch.Tensor, with_ids: bool = True):
        """The model's arguments for the pairs, in its own order -- views of one gather."""
        B, order = u_ids.shape[0], self._order(with_ids)
        got = self._gather(u_ids, i_ids, **self._outputs(None, order))
        return tuple(half for k in order for half in (got[k][:B], got[k][B:]))


class DeviceDocCache(_IdFeed):
    """All user / item documents resident on the GPU, so a batch is a pair of id vectors gathered ON DEVICE
    instead of 2 x doc_len token ids per pair shipped from the DataLoader workers.

    doc split: user_docs [U, L], item_docs [I, L] int32 (half the bytes of int64; every token was range-checked against the
    vocabulary once, here, so a gathered batch needs no per-step token check); review split: reviews [U, R, T] plus
    counterpart ids [U, R], int64.
    The reference trains on the examples' own copies (train_deepconn_pp.py:276); for the doc split those are
    the same per-id documents (DocDataset.check_documents_match_meta), so gathering by id is equivalent.  (For the review split's train
    examples the reference removes the target pair's own review, divide_and_create_example_word.py:262-288: DeviceReviewCache
    rebuilds those from ids; this cache holds the first rv_num reviews per id, the valid / test rule.)"""

    PAD = 0          # get_mask's padding id (utils.py:30-42)
    optional = ("masks", "ids")
    kind = "the doc split"

    def __init__(self, ds, device):
        self.device = torch.device(device)
        if isinstance(ds, ReviewDataset):
            # meta's lists are ragged on a real split (an id has as many reviews as it wrote): the first rv_num, zero-padded
            user, urid = _review_tables(ds.user_reviews, ds.user_rids, ds.user_num, ds.rv_num, ds.rv_len)
            item, irid = _review_tables(ds.item_reviews, ds.item_rids, ds.item_num, ds.rv_num, ds.rv_len)
            self.user, self.item = user.to(self.device), item.to(self.device)
            self.user_rids, self.item_rids = urid.to(self.device), irid.to(self.device)
        else:
            user = torch.tensor(_rows(ds.user_docs, ds.user_num, "user_docs"), dtype=torch.int64)
            item = torch.tensor(_rows(ds.item_docs, ds.item_num, "item_docs"), dtype=torch.int64)
            _check_range(user, ds.vocab_size, "meta.pkl user_docs tokens")
            _check_range(item, ds.vocab_size, "meta.pkl item_docs tokens")
            self.user = user.to(torch.int32).to(self.device)
            self.item = item.to(torch.int32).to(self.device)
            self.user_rids = self.item_rids = None
            self.doc_len = L = self.user.shape[1]
            self.like = {"docs": ((L,), torch.int64), "masks": ((L,), torch.bool), "ids": ((), torch.int64)}

    def _order(self, with_ids: bool = True):
        """(u_docs, i_docs, u_masks, i_masks, u_ids, i_ids) for DeepCoNN++, (u_docs, i_docs) for D-ATT (with_ids=False)."""
        return ("docs", "masks", "ids") if with_ids else ("docs",)

    def _gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, **outputs):
        from . import functional as RF
        if self.user_rids is not None:
            raise RuntimeError("gather is the doc split's id feed (the review split's is DeviceReviewCache.feed)")
        u_ids = u_ids.to(self.device, non_blocking=True)
        i_ids = i_ids.to(self.device, non_blocking=True)
        return dict(zip(("docs", "masks", "ids"), RF.doc_gather(u_ids, i_ids, self.user, self.item, self.PAD, 0, **outputs)))

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, out=None, masks: bool = True, ids: bool = True):
        """The documents of the pairs (u_ids[b], i_ids[b]) on the device (functional.doc_gather, one launch): stacked
        (docs [2B, L] int64, masks [2B, L] bool or None, ids [2B] int64 or None), user rows first.  `out`: a doc-fed batch to
        write into instead -- (u_docs, i_docs) or (u_docs, i_docs, u_masks, i_masks, u_ids, i_ids), each pair adjacent in one
        allocation (the input views of a recorded step); its length decides masks / ids.  An id outside its table gets the
        all-pad row 0 and an IndexError at functional.check_id_errors()."""
        if out is not None and len(out) not in (2, 6):
            raise RuntimeError("out must be (u_docs, i_docs) or (u_docs, i_docs, u_masks, i_masks, u_ids, i_ids)")
        outputs = dict(masks=masks, ids=ids) if out is None else self._outputs(out, self._order(len(out) == 6))
        return tuple(self._gather(u_ids, i_ids, **outputs).values())

    def feed(self, with_ids: bool) -> "_DocFeed":
        """The cache bound to its model's form -- with_ids=True: DeepCoNN++'s six arguments, False: D-ATT's two -- as
        DeviceReviewCache.feed binds a review cache: the feed's methods ignore the with_ids they are passed."""
        return _DocFeed(self, with_ids)

    def doc_batch(self, u_ids: torch.Tensor, i_ids: torch.Tensor):
        if self.device.type != "cuda":
            u_ids, i_ids = u_ids.to(self.device), i_ids.to(self.device)
            u_docs, i_docs = self.user.index_select(0, u_ids).long(), self.item.index_select(0, i_ids).long()
            return u_docs, i_docs, get_mask(u_docs), get_mask(i_docs), u_ids, i_ids
        return self.inputs(u_ids, i_ids, with_ids=True)

    def review_batch(self, u_ids: torch.Tensor, i_ids: torch.Tensor):
        u_ids, i_ids = u_ids.to(self.device), i_ids.to(self.device)
        u, i = self.user.index_select(0, u_ids), self.item.index_select(0, i_ids)
        return (u, i, get_mask(u), get_mask(i), u_ids, i_ids, self.user_rids.index_select(0, u_ids),
                self.item_rids.index_select(0, i_ids))


class _DocFeed(_IdFeed):
    """A DeviceDocCache bound to with_ids (DeviceDocCache.feed): the cache's launch under one model's argument order."""

    optional = DeviceDocCache.optional

    def __init__(self, cache: DeviceDocCache, with_ids: bool):
        self.cache, self.with_ids, self.device = cache, bool(with_ids), cache.device
        self.kind = "deepconn" if with_ids else "dual_att"
        self.order, self.like, self._gather = cache._order(with_ids), cache.like, cache._gather


class DeviceReviewCache:
    """meta.pkl's reviews resident on the device, R + 1 = rv_num + 1 slots per id, so that a review-split batch -- train
    (leave-one-out) or valid -- is rebuilt from (u_ids, i_ids) by one launch (functional.review_gather; see
    review_example_from_meta for the rule and why R + 1 slots are enough).

    Tables: int32 reviews [N, R+1, T] and counterpart ids [N, R+1] per side, from meta's possibly ragged per-id lists; ids absent
    from meta, and id 0, are all-pad rows.  Tokens were range-checked against the vocabulary and rids against the other side's
    id count once, here, so a gathered batch needs no per-step check.  `.user` / `.item` / `.user_rids` / `.item_rids` are the
    first R slots -- the valid rule, what recommend.Recommender encodes.  With device "cpu" the same methods run a plain torch
    restatement of the kernel (host tests, cross-checks).

    pool = P (rv_num <= P <= 63; None: today's object, nothing more is resident): the review SAMPLER's tables
    (`user_pool_table` / `user_pool_rid_table` and the item side's) hold P + 1 slots per id, so sampled_feed() draws a train
    example's reviews from the id's first P reviews instead of its first rv_num.  Everything above keeps its meaning and its
    bytes: the plain tables, gather and feed read the first R + 1 slots only."""

    PAD = 0
    NAMES = ("revs", "word_masks", "rev_masks", "rids", "ids")                # gather's outputs; sample_gather adds "slots"
    ORDER = {"narre": ("revs", "word_masks", "ids", "rids"), "simple_siamese": ("revs", "word_masks", "rev_masks", "ids")}
    MAX_POOL = 63        # one lane of a wave per table slot (csrc/review_sample.hip)

    def __init__(self, ds, device, pool=None):
        self.device = torch.device(device)
        self.rv_num, self.rv_len = int(ds.rv_num), int(ds.rv_len)
        R = self.rv_num
        if pool is not None and (isinstance(pool, bool) or not isinstance(pool, int) or not R <= pool <= self.MAX_POOL):
            raise ValueError(f"pool must be an integer in [rv_num = {R}, {self.MAX_POOL}], got {pool!r}")
        self.pool = R if pool is None else pool
        tabs = {}
        for side in ("user", "item"):
            wide = _resident_tables(ds, side, self.pool + 1, self.rv_len, self.PAD, self.device)
            # the plain gather takes contiguous [N, R + 1, ..] tables: with a wider pool, its own copies of the leading slots
            tabs[side] = wide + (wide if self.pool == R else (wide[0][:, :R + 1].contiguous(), wide[1][:, :R + 1].contiguous()))
        (self.user_pool_table, self.user_pool_rid_table, self.user_table, self.user_rid_table) = tabs["user"]
        (self.item_pool_table, self.item_pool_rid_table, self.item_table, self.item_rid_table) = tabs["item"]
        self.user, self.item = self.user_table[:, :R], self.item_table[:, :R]
        self.user_rids = self.user_rid_table[:, :R].to(torch.int64)
        self.item_rids = self.item_rid_table[:, :R].to(torch.int64)

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, leave_one_out: bool, revs=None, word_masks=None, rev_masks=True,
               rids=True, ids=True):
        """functional.review_gather over the tables (stacked outputs, user rows first); on the cpu, its torch restatement,
        which raises the IndexError of an id outside its table at once."""
        u_ids, i_ids = u_ids.to(self.device, non_blocking=True), i_ids.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            from . import functional as RF
            return RF.review_gather(u_ids, i_ids, self.user_table, self.user_rid_table, self.item_table, self.item_rid_table,
                                    leave_one_out, self.PAD, 0, revs=revs, word_masks=word_masks, rev_masks=rev_masks, rids=rids,
                                    ids=ids)
        return _deliver(self._gather_torch(u_ids, i_ids, leave_one_out), (revs, word_masks, rev_masks, rids, ids), 2)

    def _gather_torch(self, u_ids, i_ids, leave_one_out: bool):
        u = _slots_torch(u_ids, i_ids, self.user_table, self.user_rid_table, self.item_table.shape[0], leave_one_out)
        i = _slots_torch(i_ids, u_ids, self.item_table, self.item_rid_table, self.user_table.shape[0], leave_one_out)
        revs2, rids2 = torch.cat([u[0], i[0]]), torch.cat([u[1], i[1]])
        wm = revs2 != self.PAD
        return revs2, wm, wm.any(-1), rids2, torch.cat([u_ids, i_ids])

    def feed(self, kind: str, leave_one_out: bool) -> "ReviewFeed":
        """The id feed of model `kind` ("narre" / "simple_siamese"): what GraphedTrainStep.from_ids / GraphedForward.from_ids and
        the trainer take for `cache`.  leave_one_out=True rebuilds train examples, False valid / test examples."""
        return ReviewFeed(self, kind, leave_one_out)

    def sampled_feed(self, kind: str, n_user=None, n_item=None, seed: int = 0) -> "SampledReviewFeed":
        """The TRAIN feed of model `kind` with review sampling (the reference's sample_train_review, u_rv_num = n_user, i_rv_num =
        n_item; None: rv_num): every gather keeps a fresh uniform random subset of each row's non-empty candidate reviews -- the
        id's first `pool` reviews less the pair's own -- in random order, in rv_num slots with an empty tail."""
        return SampledReviewFeed(self, kind, n_user, n_item, seed)

    def sample_gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, n_user: int, n_item: int, seed: int, state: torch.Tensor,
                      revs=None, word_masks=None, rev_masks=True, rids=True, ids=True, slots=None):
        """functional.review_sample_gather over the pool tables, leave-one-out (stacked outputs, user rows first, plus the slots);
        on the cpu, the host restatement of the draw, which advances state[0] itself."""
        u_ids, i_ids = u_ids.to(self.device, non_blocking=True), i_ids.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            from . import functional as RF
            return RF.review_sample_gather(u_ids, i_ids, self.user_pool_table, self.user_pool_rid_table, self.item_pool_table,
                                           self.item_pool_rid_table, self.rv_num, n_user, n_item, state=state, seed=seed,
                                           leave_one_out=True, pad_token=self.PAD, replace_id=0, revs=revs, word_masks=word_masks,
                                           rev_masks=rev_masks, rids=rids, ids=ids, slots=slots)
        got = self._sample_gather_host(u_ids, i_ids, n_user, n_item, seed, int(state[0]))
        state[0] += 1
        return _deliver(got, (revs, word_masks, rev_masks, rids, ids, slots), 2)

    def _sample_gather_host(self, u_ids, i_ids, n_user: int, n_item: int, seed: int, call: int):
        """THE DRAW of include/rbr_hip.h (rbr_review_sample_gather) in numpy, for call number `call`."""
        import numpy as np
        R, P, T, B = self.rv_num, self.pool, self.rv_len, u_ids.shape[0]
        u, i = u_ids.numpy().astype(np.int64), i_ids.numpy().astype(np.int64)
        q = np.arange(P, dtype=np.int64)
        k = np.arange(R, dtype=np.int64)
        outs = []
        for side, (own, other, tab, rid, n_other, keep) in enumerate(
                ((u, i, self.user_pool_table, self.user_pool_rid_table, self.item_pool_table.shape[0], n_user),
                 (i, u, self.item_pool_table, self.item_pool_rid_table, self.user_pool_table.shape[0], n_item))):
            _check_range(own, tab.shape[0], "ids of a gathered batch")
            rr = rid.numpy()[own].astype(np.int64)                                  # [B, P + 1]
            rv = tab.numpy()[own].astype(np.int64)                                  # [B, P + 1, T]
            hit = (rr[:, :P] == other[:, None]) & ((other > 0) & (other < n_other))[:, None]
            d = np.where(hit.any(1), hit.argmax(1), P)                              # the FIRST match, else P
            src = q[None, :] + (q[None, :] >= d[:, None])                           # [B, P]
            live = np.take_along_axis((rv != self.PAD).any(-1), src, 1)
            e = ((np.arange(B, dtype=np.uint64) + np.uint64(side * B))[:, None] * np.uint64(64) + q[None, :].astype(np.uint64))
            words = np.stack(_philox4x32_10(e >> np.uint64(2), call, seed))         # [4, B, P]
            key = np.take_along_axis(words, (e & np.uint64(3)).astype(np.int64)[None], 0)[0]
            # live candidates first, by (key, q): a dead one sorts behind every 32-bit key
            order = np.argsort(np.where(live, key, np.uint64(1) << np.uint64(32)) * np.uint64(64) + q[None, :].astype(np.uint64), 1)
            filled = k[None, :] < np.minimum(keep, live.sum(1))[:, None]            # [B, R]
            slot = np.where(filled, np.take_along_axis(src, order[:, :R], 1), -1)
            at = np.maximum(slot, 0)
            revs = np.where(filled[:, :, None], np.take_along_axis(rv, at[:, :, None], 1), self.PAD)
            rids = np.where(filled, np.take_along_axis(rr, at, 1), 0)
            outs.append((revs, rids, slot))
        revs2 = torch.from_numpy(np.concatenate([o[0] for o in outs]))
        rids2 = torch.from_numpy(np.concatenate([o[1] for o in outs]))
        slots2 = torch.from_numpy(np.concatenate([o[2] for o in outs]).astype(np.int32))
        wm = revs2 != self.PAD
        return revs2, wm, wm.any(-1), rids2, torch.cat([u_ids, i_ids]), slots2


def _philox4x32_10(quad, call: int, seed: int):
    """The four words of the Philox4x32-10 block with counter (quad, call) under key `seed` (csrc/rbr_rng.h): quad a uint64 numpy
    array, words as uint64 arrays below 2^32."""
    import numpy as np
    lo, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1 = quad & lo, quad >> s32
    c2 = np.full_like(quad, call & 0xFFFFFFFF)
    c3 = np.full_like(quad, (call >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


class _Reseed:
    """reseed() of a feed that draws: `seed` and `state` (int64 [2] on the feed's device, [call number, ticket])."""

    def reseed(self, seed: int, call: int = 0) -> None:
        """The next draw is call number `call` under `seed` (no host synchronisation: one small copy on the current stream).
        A recorded step holds the seed it was recorded with: reseed it with that seed, to move the call number only."""
        self.seed = int(seed)
        self.state.copy_(torch.tensor([int(call), 0], dtype=torch.int64), non_blocking=True)


class ReviewFeed(_IdFeed):
    """One model's view of a DeviceReviewCache under one rule: empty_inputs / gather / inputs with DeviceDocCache's meaning, in
    the model's own argument order --
      narre          (u_revs, i_revs, u_word_masks, i_word_masks, u_ids, i_ids, u_rids, i_rids)
      simple_siamese (u_revs, i_revs, u_word_masks, i_word_masks, u_rev_masks, i_rev_masks, u_ids, i_ids)"""

    def __init__(self, cache: DeviceReviewCache, kind: str, leave_one_out: bool):
        if kind not in cache.ORDER:
            raise ValueError(f"the review feed serves {sorted(cache.ORDER)}, not {kind}")
        self.cache, self.kind, self.leave_one_out = cache, kind, bool(leave_one_out)
        self.order = cache.ORDER[kind]
        self.device = cache.device
        R, T = cache.rv_num, cache.rv_len
        self.like = {"revs": ((R, T), torch.int64), "word_masks": ((R, T), torch.bool), "rev_masks": ((R,), torch.bool),
                     "rids": ((R,), torch.int64), "ids": ((), torch.int64)}


class SampledReviewFeed(_Reseed, ReviewFeed):
    """ReviewFeed under the train rule with the reference's review sampling (trainer/train_simple_siamese.py:346-368,
    sample_train_review): every gather keeps n_user / n_item (the reference's u_rv_num / i_rv_num; None: rv_num) of each row's
    non-empty candidate reviews, a fresh uniform random subset in random order, and pads to rv_num slots with empty reviews.  The
    candidates are the id's first cache.pool reviews less the pair's own, so with pool > rv_num reviews that truncation drops
    reach training.  Shapes, dtypes and protocol are ReviewFeed's: models, recorded input blocks and wrappers (NegativeFeed,
    InBatchFeed) take it unchanged, and a recorded gather draws anew on every replay.

    `state`: int64 [2] on the feed's device, [call number, ticket] (csrc/rbr_rng.h); the launch advances the call number, on the
    cpu the host restatement does.  reseed(seed, call) restarts the sequence: (seed, call) fixes a draw exactly
    (include/rbr_hip.h, rbr_review_sample_gather).  `slots` of the last gather's dict: None unless asked for (gather(slots=True))."""

    def __init__(self, cache: DeviceReviewCache, kind: str, n_user=None, n_item=None, seed: int = 0):
        super().__init__(cache, kind, True)
        R = cache.rv_num
        self.n_user, self.n_item = (R if n is None else n for n in (n_user, n_item))
        for name, n in (("n_user", self.n_user), ("n_item", self.n_item)):
            if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= R:
                raise ValueError(f"{name} must be an integer in [1, rv_num = {R}], got {n!r}")
        self.seed = int(seed)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)

    def _gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, slots=None, **outputs):
        """ReviewFeed's with the draw of the feed's next call number; `slots` (gather(slots=...)): True / an int32 [2B, R] tensor for
        the table slot behind every output slot (-1: empty)."""
        got = self.cache.sample_gather(u_ids, i_ids, self.n_user, self.n_item, self.seed, self.state, slots=slots, **outputs)
        return dict(zip(self.cache.NAMES + ("slots",), got))


class DeviceSentenceCache:
    """The sentence split's DeviceReviewCache (AHN): meta.pkl's reviews resident on the device as int32 tables [N, R+1, S, W] with
    their counterpart ids [N, R+1] per side, so that a batch -- train (leave-one-out) or valid -- is rebuilt from (u_ids, i_ids) by
    one launch (functional.sentence_gather), sentence lengths and masks included.  Ids absent from meta, and id 0, are all-pad rows;
    tokens were range-checked against the vocabulary and rids against the other side's id count once, here.  With device "cpu"
    the same methods run a plain torch restatement of the kernel (host tests, cross-checks)."""

    PAD = 0
    NAMES = ("revs", "sent_lens", "sent_masks", "rev_masks", "rids", "ids")

    def __init__(self, ds, device):
        self.device = torch.device(device)
        self.rv_num, self.sent_num, self.word_num = int(ds.rv_num), int(ds.sent_num), int(ds.word_num)
        (self.user_table, self.user_rid_table), (self.item_table, self.item_rid_table) = (
            _resident_tables(ds, side, self.rv_num + 1, (self.sent_num, self.word_num), self.PAD, self.device)
            for side in ("user", "item"))

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, leave_one_out: bool, rids=True, ids=True, **out):
        """functional.sentence_gather over the tables: (revs, sent_lens, sent_masks, rev_masks, rids, ids), stacked, user rows first
        (`out`: its output tensors by name); on the cpu, its torch restatement, which raises the IndexError of an id outside its
        table at once."""
        u_ids, i_ids = u_ids.to(self.device, non_blocking=True), i_ids.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            from . import functional as RF
            return RF.sentence_gather(u_ids, i_ids, self.user_table, self.user_rid_table, self.item_table, self.item_rid_table,
                                      leave_one_out, self.PAD, 0, rids=rids, ids=ids, **out)
        out.update(rids=rids, ids=ids)
        return _deliver(self._gather_torch(u_ids, i_ids, leave_one_out), [out.get(name) for name in self.NAMES], 4)

    def _gather_torch(self, u_ids, i_ids, leave_one_out: bool):
        u = _slots_torch(u_ids, i_ids, self.user_table, self.user_rid_table, self.item_table.shape[0], leave_one_out)
        i = _slots_torch(i_ids, u_ids, self.item_table, self.item_rid_table, self.user_table.shape[0], leave_one_out)
        revs2 = torch.cat([u[0], i[0]])
        return (revs2, *sentence_masks(revs2, self.PAD), torch.cat([u[1], i[1]]), torch.cat([u_ids, i_ids]))

    def feed(self, leave_one_out: bool) -> "SentenceFeed":
        """AHN's id feed under one rule: leave_one_out=True rebuilds train examples, False valid / test examples."""
        return SentenceFeed(self, leave_one_out)


class SentenceFeed(_IdFeed):
    """AHN's view of a DeviceSentenceCache under one rule: the model's ten forward arguments (models/ahn/ahn_model.py) --
    (u_revs, i_revs, u_sent_masks, i_sent_masks, u_sent_lens, i_sent_lens, u_rev_masks, i_rev_masks, u_ids, i_ids)."""

    ORDER = order = ("revs", "sent_masks", "sent_lens", "rev_masks", "ids")
    optional = ("rids", "ids")
    kind = "ahn"

    def __init__(self, cache: DeviceSentenceCache, leave_one_out: bool):
        self.cache, self.leave_one_out = cache, bool(leave_one_out)
        self.device = cache.device
        R, S, W = cache.rv_num, cache.sent_num, cache.word_num
        self.like = {"revs": ((R, S, W), torch.int64), "sent_masks": ((R, S), torch.bool), "sent_lens": ((R, S), torch.int64),
                     "rev_masks": ((R,), torch.bool), "ids": ((), torch.int64)}


class NegativeFeed(_Reseed):
    """An id feed (DeviceDocCache, ReviewFeed) behind a negative sampler, for a pairwise objective (train_step.BprObjective): a
    batch of B observed pairs becomes (1 + n_neg) * B pairs -- rows [0, B) the pairs themselves, rows [(j+1)B, (j+2)B) each
    pair's j-th negative, an item of [item_lo, n_items) its user has not rated (functional.sample_negatives; `seen`: the training
    split's recommend.Recommender.seen_from, or None) -- and the inner feed gathers those.  It speaks the inner feed's protocol
    (empty_inputs / gather / inputs), so GraphedTrainStep.from_ids records sampler + gather + step, and every replay draws new
    negatives.  A review feed applies its leave-one-out rule to every expanded pair as to any pair (a negative's pair has no
    review of its own to leave out).

    n_cand > 1 is dynamic negative sampling (functional.sample_hard_negatives): every negative is the best-scoring of n_cand such
    draws under latent tables handed over with set_tables(); only the winner is gathered and encoded.  The feed keeps its OWN
    static copies of the tables, so a recorded step holds valid pointers across refreshes; the head's parameters are the model's
    live ones.  n_cand = 1 (the default) is the uniform sampler, call for call.

    The expanded ids and the `valid` flags (f32 [n_neg * B]: 0 where a user has no unrated item) live in static buffers, one
    set per batch size B (`buffers(B)`; `u_out` / `i_out` / `valid` are those of the last gather); `state` is the sampler's
    [call number, ticket] on the device.  reseed(seed, call) restarts the sequence: (seed, call) fixes a draw exactly."""

    def __init__(self, feed, seen, n_items: int, n_neg: int = 1, seed: int = 0, item_lo: int = 1, max_tries: int = 16,
                 n_cand: int = 1):
        if isinstance(n_neg, bool) or not isinstance(n_neg, int) or n_neg < 1:
            raise ValueError(f"n_neg must be an integer >= 1, got {n_neg!r}")
        if not 0 <= int(item_lo) < int(n_items):
            raise ValueError(f"item_lo {item_lo} leaves no item of [0, {n_items})")
        if not 1 <= int(max_tries) <= 64:
            raise ValueError(f"max_tries must be in [1, 64], got {max_tries}")
        if isinstance(n_cand, bool) or not isinstance(n_cand, int) or not 1 <= n_cand <= 64:
            raise ValueError(f"n_cand must be an integer in [1, 64], got {n_cand!r}")
        self.feed, self.device = feed, torch.device(feed.device)
        self.seen = None if seen is None else (seen[0].to(self.device), seen[1].to(self.device))
        self.n_items, self.n_neg, self.item_lo, self.max_tries = int(n_items), n_neg, int(item_lo), int(max_tries)
        self.n_cand = n_cand
        self.seed = int(seed)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._buffers = {}
        self._last = None
        self._tables = None          # (mode, ul, il, h, g, ub, ib) of set_tables: ul / il the feed's own copies

    def set_tables(self, mode, ul, il, h=None, g=None, ub=None, ib=None) -> None:
        """The latent tables ul [U, K] / il [n_items, K] and the head (`mode`, h, g, ub, ib: model.score_mode_and_params()) that
        score the candidates of n_cand > 1.  The first call allocates the feed's own f32 copies of ul / il; later calls copy into
        them (same shapes), on the current stream: a step recorded in between keeps its pointers and draws from the new values.
        h, g, ub, ib are kept as given -- the model's live parameters, not copies."""
        if ul.dim() != 2 or il.dim() != 2 or ul.shape[1] != il.shape[1] or il.shape[0] != self.n_items:
            raise ValueError(f"latent tables must be [U, K] / [{self.n_items}, K], got {tuple(ul.shape)} / {tuple(il.shape)}")
        if self._tables is None:
            own_ul = ul.detach().to(self.device, torch.float32, copy=True).contiguous()
            own_il = il.detach().to(self.device, torch.float32, copy=True).contiguous()
        else:
            own_ul, own_il = self._tables[1], self._tables[2]
            if own_ul.shape != ul.shape or own_il.shape != il.shape:
                raise ValueError(f"latent tables changed shape: {tuple(own_ul.shape)} / {tuple(own_il.shape)} were set, got "
                                 f"{tuple(ul.shape)} / {tuple(il.shape)}")
            own_ul.copy_(ul.detach())
            own_il.copy_(il.detach())
        self._tables = (mode, own_ul, own_il, h, g, ub, ib)

    tables = property(lambda self: None if self._tables is None else self._tables[1:3], doc="the feed's own (ul, il), or None")

    def buffers(self, B: int):
        """(u_out, i_out, valid) of batch size B: the sampler's static outputs."""
        buf = self._buffers.get(B)
        if buf is None:
            rows = (1 + self.n_neg) * B
            buf = self._buffers[B] = (torch.zeros(rows, dtype=torch.int64, device=self.device),
                                      torch.zeros(rows, dtype=torch.int64, device=self.device),
                                      torch.zeros(self.n_neg * B, dtype=torch.float32, device=self.device))
        return buf

    u_out = property(lambda self: self._last[0])
    i_out = property(lambda self: self._last[1])
    valid = property(lambda self: self._last[2])

    def sample(self, u_ids: torch.Tensor, i_ids: torch.Tensor):
        """Draws the negatives of the pairs into buffers(B) and returns them."""
        from . import functional as RF
        if self.n_cand > 1 and self._tables is None:
            raise RuntimeError("NegativeFeed(n_cand > 1) scores its candidates from latent tables: call set_tables() first")
        u_ids, i_ids = u_ids.to(self.device, non_blocking=True), i_ids.to(self.device, non_blocking=True)
        if self.n_cand == 1:
            self._last = RF.sample_negatives(u_ids, i_ids, self.n_neg, self.n_items, self.seen, state=self.state, seed=self.seed,
                                             item_lo=self.item_lo, max_tries=self.max_tries, replace_id=self.item_lo,
                                             out=self.buffers(u_ids.shape[0]))
        else:
            mode, ul, il, h, g, ub, ib = self._tables
            self._last = RF.sample_hard_negatives(u_ids, i_ids, self.n_neg, self.n_items, self.seen, n_cand=self.n_cand, mode=mode,
                                                  ul=ul, il=il, h=h, g=g, ub=ub, ib=ib, state=self.state, seed=self.seed,
                                                  item_lo=self.item_lo, max_tries=self.max_tries, replace_id=self.item_lo,
                                                  out=self.buffers(u_ids.shape[0]))
        return self._last

    def empty_inputs(self, B: int, with_ids: bool = True):
        """The inner feed's empty_inputs for the (1 + n_neg) * B expanded pairs."""
        self.buffers(B)            # allocated here, outside any capture
        return self.feed.empty_inputs((1 + self.n_neg) * B, with_ids)

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, out=None, **kw):
        """Sampler, then the inner feed's gather of the expanded pairs (`out`: the model's arguments for (1 + n_neg) * B pairs)."""
        u_out, i_out, _ = self.sample(u_ids, i_ids)
        return self.feed.gather(u_out, i_out, out=out, **kw)

    def inputs(self, u_ids: torch.Tensor, i_ids: torch.Tensor, with_ids: bool = True):
        """The model's arguments for the expanded pairs."""
        u_out, i_out, _ = self.sample(u_ids, i_ids)
        return self.feed.inputs(u_out, i_out, with_ids=with_ids)


class InBatchFeed:
    """An id feed (DeviceDocCache, ReviewFeed) for the in-batch softmax objective (train_step.InBatchSoftmaxObjective): the batch
    stays the B observed pairs -- every user's negatives are the other B - 1 items of the same batch, at no encoder cost -- so
    the inner feed gathers exactly what it would for the MSE step.  What this class adds is what the all-pairs loss needs beside
    the latents: the (u_ids, i_ids) of the last gather (`u_ids` / `i_ids`: references, not copies, as NegativeFeed's buffers --
    a recorded slot's objective therefore reads that slot's own static id tensors), the seen-items CSR on the device (`seen`:
    the training split's recommend.Recommender.seen_from, or None: an item its user has rated is no negative) and item_lo (ids
    below it, the pad id, are nobody's negative).  It speaks the inner feed's protocol (empty_inputs / gather / inputs)."""

    def __init__(self, feed, seen, item_lo: int = 1):
        for name in ("empty_inputs", "gather", "inputs", "device"):
            if not hasattr(feed, name):
                raise ValueError(f"InBatchFeed wraps an id feed (empty_inputs / gather / inputs / device); {type(feed).__name__} has no {name}")
        if isinstance(item_lo, bool) or not isinstance(item_lo, int) or item_lo < 0:
            raise ValueError(f"item_lo must be an integer >= 0, got {item_lo!r}")
        if seen is not None:
            if len(seen) != 2:
                raise ValueError("seen must be (off [U + 1], items): one row per user id (recommend.Recommender.seen_from)")
            off, items = seen
            if off.dtype != torch.int64 or items.dtype != torch.int32 or off.dim() != 1 or items.dim() != 1 or off.shape[0] < 2:
                raise ValueError(f"seen must be (int64 [U + 1], int32 [nnz]), got {off.dtype} {tuple(off.shape)}, "
                                 f"{items.dtype} {tuple(items.shape)}")
        self.feed, self.device = feed, torch.device(feed.device)
        self.seen = None if seen is None else (seen[0].to(self.device), seen[1].to(self.device))
        self.item_lo = item_lo
        self._last = None

    u_ids = property(lambda self: self._last[0])
    i_ids = property(lambda self: self._last[1])

    def _note(self, u_ids: torch.Tensor, i_ids: torch.Tensor):
        if u_ids.dim() != 1 or u_ids.shape != i_ids.shape:
            raise RuntimeError(f"u_ids / i_ids must be [B] each, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")
        self._last = (u_ids.to(self.device, non_blocking=True), i_ids.to(self.device, non_blocking=True))
        return self._last

    def empty_inputs(self, B: int, with_ids: bool = True):
        return self.feed.empty_inputs(B, with_ids)

    def gather(self, u_ids: torch.Tensor, i_ids: torch.Tensor, out=None, **kw):
        """The inner feed's gather of the pairs; the ids are kept for the objective."""
        u, i = self._note(u_ids, i_ids)
        return self.feed.gather(u, i, out=out, **kw)

    def inputs(self, u_ids: torch.Tensor, i_ids: torch.Tensor, with_ids: bool = True):
        """The model's arguments for the pairs; the ids are kept for the objective."""
        u, i = self._note(u_ids, i_ids)
        return self.feed.inputs(u, i, with_ids=with_ids)


def _adjacent(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[a; b] as ONE view when b directly follows a in the same allocation (a write through it lands in a and b)."""
    if not (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel()):
        raise RuntimeError("the output pair must be adjacent halves of one allocation (see train_step._flat_layout)")
    return a.as_strided((2 * a.shape[0], *a.shape[1:]), a.stride(), a.storage_offset())
