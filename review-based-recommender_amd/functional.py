"""torch.autograd.Functions over the C ABI (include/rbr_hip.h).  HIP tensors only."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import ACT_RELU, ACT_TANH, PAD_SAME, PAD_VALID, TIMER, check, current_stream, dev_ptr, ptr_array

F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8


def _mask_u8(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    raise RuntimeError(f"mask must be bool or uint8, got {mask.dtype}")


def _call(key: Optional[str], fn, *args) -> None:
    """check(fn(*args)) for the C-ABI entry `fn`, bracketed by a pair of TIMER events recorded under `key` while bench.py's
    kernel-timing pass is on.  key None: never bracketed (inside a D-ATT pair region an event pair would be a stream operation
    ahead of the recorded launches)."""
    ev = TIMER.record(key) if key is not None else None
    check(fn(*args), fn.__name__)
    if ev is not None:
        ev.record()


@contextlib.contextmanager
def _timed(key: str):
    """The same bracket around a block of several calls."""
    ev = TIMER.record(key)
    yield
    if ev is not None:
        ev.record()


# Data-parallel tap exchange (distributed.TapExchange): when a sink is installed, the backward of an un-gated conv over the
# sink's word table emits its (token, value) taps instead of the dense table gradient; the sink rebuilds the averaged
# gradient of all ranks after an all-gather of the taps (rbr_textcnn_bwd_taps / rbr_textcnn_dtable_from_taps).
_TAP_SINKS: dict = {}       # word-table data_ptr -> sink: several models (an eval / EMA copy, a second trainer) can coexist


def set_prod_precision(name: Optional[str]) -> None:
    """Arithmetic of the token-product conv's GEMM (rbr_set_prod_precision): "f32" (f32 MFMA, an fma chain bit for bit),
    "bf16x3" (default: exact three-plane bf16 split, 6 plane products, f32 accumulation: f32-class accuracy), "bf16x2",
    "bf16" (operands rounded to bf16: the reduced-precision row of BASELINE configs 3 and 5); None restores the default.
    Set it between steps, never between a forward and its backward (the workspace layout depends on it)."""
    if name is not None and name not in _lib.PROD_PRECISIONS:
        raise ValueError(f"unknown product precision {name!r}; one of {sorted(_lib.PROD_PRECISIONS)}")
    _lib.lib().rbr_set_prod_precision(-1 if name is None else _lib.PROD_PRECISIONS[name])


_DTABLE_MODE: list = [None]


def set_dtable_mode(mode: Optional[str]) -> None:
    """How an un-gated conv's backward accumulates the word-table gradient: None (default; env RBR_DTABLE_MODE) = G built with
    f32 atomics, whose arrival order leaves rounding-level run-to-run noise in the result; "fixed" = every (token, tap, channel)
    cell summed in 64-bit fixed point (2^-40 units, integer adds: order-free) -- two runs over the same batch give the same
    bits, like the reference's CPU embedding backward (models/deepconn/layers.py:22-24).  It is the data-parallel tap rebuild run
    on this rank's taps alone (rbr_textcnn_bwd_taps + rbr_textcnn_dtable_from_taps, n_sets = 1): a sort per step, eager
    launches only (rocPRIM's sort cannot be recorded into a hipGraph here), D % 4 == 0."""
    if mode not in (None, "fixed"):
        raise ValueError(f"unknown dtable mode {mode!r}; None or 'fixed'")
    _DTABLE_MODE[0] = mode


def _dtable_fixed() -> bool:
    return (_DTABLE_MODE[0] or os.environ.get("RBR_DTABLE_MODE")) == "fixed"


def get_prod_precision() -> str:
    mode = _lib.lib().rbr_get_prod_precision()
    return {v: k for k, v in _lib.PROD_PRECISIONS.items()}[mode]


def set_prod_split(name: Optional[str]) -> None:
    """Realisation of the "bf16x3" class on the forward GEMM's rows-in-registers route (rbr_set_prod_split; six or more
    128-column groups, D >= 177): "f16x2s" (default: two scaled f16 planes, 3 plane products, the same f32-class accuracy) or
    "bf16x3" (the six-product bf16 kernel: the A/B switch); None restores the default (env RBR_PROD_SPLIT).  Every other kernel
    and class ignores it.  Set it between steps, like the precision."""
    if name is not None and name not in _lib.PROD_SPLITS:
        raise ValueError(f"unknown product split {name!r}; one of {sorted(_lib.PROD_SPLITS)}")
    _lib.lib().rbr_set_prod_split(-1 if name is None else _lib.PROD_SPLITS[name])


def get_prod_split() -> str:
    split = _lib.lib().rbr_get_prod_split()
    return {v: k for k, v in _lib.PROD_SPLITS.items()}[split]


# --------------------------------------------------------------------------- id range check
_ID_ERR: dict = {}       # per device: int64[4] error record of rbr_sanitize_ids (zero while clean)


def _id_err(dev) -> torch.Tensor:
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _ID_ERR.get(idx)
    if t is None:
        t = _ID_ERR[idx] = torch.zeros(4, dtype=torch.int64, device=dev)
    return t


def sanitize_ids(sets, stack_first_two: bool = False):
    """Range check in front of the embedding-style lookups: `sets` = [(ids int64 tensor, table rows, replacement row), ...]
    (at most 8).  Returns clean copies (one launch, one allocation): an id outside [0, rows) becomes `replacement` and is
    recorded on the device; check_id_errors() raises the IndexError nn.Embedding would have raised (reference
    models/deepconn/layers.py:23) at the caller's next synchronisation point.  With `stack_first_two` the first two
    outputs (equal shapes) are adjacent and the first return value is the stacked [2n, ...] tensor (user rows first)."""
    if not sets or len(sets) > _lib.MAX_ID_SETS:
        raise RuntimeError(f"sanitize_ids takes 1..{_lib.MAX_ID_SETS} id tensors")
    dev = sets[0][0].device
    tens = []
    for t, rows, rep in sets:
        if t.dtype != I64:
            raise RuntimeError(f"ids must be int64, got {t.dtype}")
        dev_ptr(t.contiguous(), I64, "ids")        # device gate
        tens.append(t.contiguous())
    flat = torch.empty(sum(t.numel() for t in tens), dtype=I64, device=dev)
    outs, o = [], 0
    arr = (_lib.IdSet * len(tens))()
    for k, (t, (_, rows, rep)) in enumerate(zip(tens, sets)):
        v = flat[o:o + t.numel()].view(t.shape)
        outs.append(v)
        o += t.numel()
        rep = 0 if rep is None or rep < 0 else int(rep)
        arr[k] = _lib.IdSet(t.data_ptr() if t.numel() else None, v.data_ptr() if t.numel() else None, t.numel(), int(rows), rep)
    _call(None, _lib.lib().rbr_sanitize_ids, len(tens), arr, _id_err(dev).data_ptr(), current_stream())
    if stack_first_two:
        a, b = tens[0], tens[1]
        if a.shape != b.shape:
            raise RuntimeError("stack_first_two needs equal shapes")
        outs = [flat[:2 * a.numel()].view(2 * a.shape[0], *a.shape[1:])] + outs[2:]
    return outs


def check_id_errors(device=None) -> None:
    """Raises IndexError when any id seen by sanitize_ids() since the last call was outside its table (and clears the
    record).  Synchronises with the device: call it where the trainer synchronises anyway (its loss.item() log points)."""
    devs = list(_ID_ERR) if device is None else [torch.device(device).index if torch.device(device).index is not None
                                                 else torch.cuda.current_device()]
    for idx in devs:
        t = _ID_ERR.get(idx)
        if t is None:
            continue
        rec = t.cpu()
        if int(rec[0]) > 0:
            t.zero_()
            raise IndexError(f"index out of range in self: {int(rec[0])} id(s) outside their table on cuda:{idx}, e.g. "
                             f"{int(rec[1])} in id tensor #{int(rec[2])} of its call; such ids were replaced by the padding row")


def dedup_rows(u_ids: torch.Tensor, i_ids: torch.Tensor, user_size: int, item_size: int, masks: Optional[torch.Tensor], L: int):
    """In-batch dedup of the documents by id (rbr_dedup_rows): returns (first [2B] int64, masks_out [2B, L] bool).  Rows
    [0, B) are the user side, [B, 2B) the item side; first[r] is the first row of the same side carrying the same id, and
    masks_out blanks every row that is not its own first occurrence, so the encoder skips the repeated documents.
    Everything has a static shape and nothing synchronises: the step stays graph-capturable."""
    B = u_ids.shape[0]
    dev = u_ids.device
    u_ids, i_ids = u_ids.contiguous(), i_ids.contiguous()
    mask8 = _mask_u8(masks)
    if mask8 is not None and mask8.shape != (2 * B, L):
        raise RuntimeError(f"masks must be [{2 * B}, {L}], got {tuple(mask8.shape)}")
    L_ = _lib.lib()
    ws = torch.empty(L_.rbr_dedup_ws_bytes(int(user_size), int(item_size)), dtype=torch.uint8, device=dev)
    first = torch.empty(2 * B, dtype=I64, device=dev)
    out = torch.empty(2 * B, L, dtype=torch.uint8, device=dev)
    _call(None, L_.rbr_dedup_rows, B, int(L), dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"), int(user_size),
          int(item_size), dev_ptr(mask8, U8, "mask"), ws.data_ptr(), dev_ptr(first, I64, "first"), dev_ptr(out, U8, "mask_out"),
          current_stream())
    return first, out.view(torch.bool)


def _pair_batch(u_ids: torch.Tensor, i_ids: torch.Tensor) -> int:
    """B of a gather's id vectors, which must be [B] each."""
    if u_ids.dim() != 1 or u_ids.shape != i_ids.shape:
        raise RuntimeError(f"u_ids / i_ids must be [B] each, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")
    return u_ids.shape[0]


def _check_review_tables(user_revs, user_rids, item_revs, item_rids, dims: str) -> None:
    """The resident (reviews, rids) pair of both sides: reviews [U, *dims] / [I, *dims] with equal `dims` (their names for the
    message: "R+1, T", "R+1, S, W") and at least two slots, rids [U, slots] / [I, slots]."""
    nd = 2 + dims.count(",")
    if user_revs.dim() != nd or item_revs.dim() != nd or user_revs.shape[1:] != item_revs.shape[1:] or user_revs.shape[1] < 2:
        raise RuntimeError(f"review tables must be [U, {dims}] / [I, {dims}], got {tuple(user_revs.shape)} / "
                           f"{tuple(item_revs.shape)}")
    n = user_revs.shape[1]
    if user_rids.shape != (user_revs.shape[0], n) or item_rids.shape != (item_revs.shape[0], n):
        raise RuntimeError(f"rid tables must be [U, {n}] / [I, {n}], got {tuple(user_rids.shape)} / {tuple(item_rids.shape)}")


def _gather_outputs(dev, rows: int, spec, given):
    """The stacked outputs of a gather.  spec: (name, trailing shape, dtype, optional) per output; `given`: what the caller passed
    for each.  A tensor is written into and must be contiguous, [rows, *trailing] and of that dtype; a required output is
    allocated on None; an optional one is allocated on True and left out (None) on None / False."""
    outs = []
    for (name, tail, dtype, optional), t in zip(spec, given):
        shape = (rows, *tail)
        if optional and (t is None or t is False):
            t = None
        elif t is (True if optional else None):
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {dtype} tensor of shape {list(shape)}, got {t.dtype} {list(t.shape)}")
        outs.append(t)
    return outs


def _review_outputs(R: int, T: int):
    """_gather_outputs' spec of the review split's five outputs."""
    return (("revs", (R, T), I64, False), ("word_masks", (R, T), torch.bool, False), ("rev_masks", (R,), torch.bool, True),
            ("rids", (R,), I64, True), ("ids", (), I64, True))


def doc_gather(u_ids: torch.Tensor, i_ids: torch.Tensor, user_docs: torch.Tensor, item_docs: torch.Tensor, pad_token: int = 0,
               replace_id: int = 0, docs: Optional[torch.Tensor] = None, masks=True, ids=True):
    """The id-fed doc-split batch (rbr_doc_gather, one launch): returns (docs2 [2B, L] int64, masks2 [2B, L] bool or None,
    ids2 [2B] int64 or None), user rows first -- docs2[:B] / docs2[B:] are the u_docs / i_docs that DocDataset.collate_fn builds
    for the same ids, masks2 = docs2 != pad_token, ids2 the checked ids.  user_docs / item_docs: [U, L] / [I, L] int32 tables.

    An id outside its table reads row `replace_id` instead (the all-pad row 0 of meta.pkl's tables) and is recorded like
    sanitize_ids() records it: check_id_errors() raises nn.Embedding's IndexError at the caller's next synchronisation point.
    (The doc-fed path keeps the document the caller sent for a bad id; here no document exists for it.)

    `docs` / `masks` / `ids`: stacked output tensors to write into (a recorded step's input views), True to allocate, or
    None / False to leave out (masks / ids; D-ATT takes the documents only).  No autograd, no sync: graph-capturable."""
    B = _pair_batch(u_ids, i_ids)
    if user_docs.dim() != 2 or item_docs.dim() != 2 or item_docs.shape[1] != user_docs.shape[1]:
        raise RuntimeError(f"tables must be [U, L] / [I, L], got {tuple(user_docs.shape)} / {tuple(item_docs.shape)}")
    L, dev = user_docs.shape[1], u_ids.device
    docs, masks, ids = _gather_outputs(dev, 2 * B, (("docs", (L,), I64, False), ("masks", (L,), torch.bool, True),
                                                    ("ids", (), I64, True)), (docs, masks, ids))
    if B == 0:
        return docs, masks, ids
    _call(None, _lib.lib().rbr_doc_gather, B, L, dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"),
          dev_ptr(user_docs, I32, "user_docs"), user_docs.shape[0], dev_ptr(item_docs, I32, "item_docs"), item_docs.shape[0],
          int(pad_token), int(replace_id), dev_ptr(docs, I64, "docs"),
          dev_ptr(None if masks is None else masks.view(U8), U8, "masks"), dev_ptr(ids, I64, "ids"), _id_err(dev).data_ptr(),
          current_stream())
    return docs, masks, ids


def review_gather(u_ids: torch.Tensor, i_ids: torch.Tensor, user_revs: torch.Tensor, user_rids: torch.Tensor,
                  item_revs: torch.Tensor, item_rids: torch.Tensor, leave_one_out: bool, pad_token: int = 0, replace_id: int = 0,
                  revs: Optional[torch.Tensor] = None, word_masks: Optional[torch.Tensor] = None, rev_masks=True, rids=True, ids=True):
    """The id-fed review-split batch (rbr_review_gather, one launch): returns (revs2 [2B, R, T] int64, word_masks2 [2B, R, T]
    bool, rev_masks2 [2B, R] bool or None, rids2 [2B, R] int64 or None, ids2 [2B] int64 or None), user rows first -- the halves
    are what ReviewDataset.collate_fn builds from the examples of the same pairs.  Tables: user_revs [U, R+1, T] / user_rids
    [U, R+1], item_revs [I, R+1, T] / item_rids [I, R+1], int32 (data.DeviceReviewCache).

    leave_one_out (a train example): the first of an id's R leading reviews that was written for the pair's counterpart is
    dropped and the following slots move up; without it, or without such a review, the first R slots are taken as they are.
    word_masks2 = revs2 != pad_token, rev_masks2 = word_masks2.any(-1).  An own id outside its table reads row `replace_id`
    and is recorded as doc_gather records it (check_id_errors()).

    `revs` / `word_masks`: stacked tensors to write into, or None to allocate; `rev_masks` / `rids` / `ids`: a stacked tensor,
    True to allocate, None / False to leave out.  No autograd, no sync: graph-capturable."""
    B = _pair_batch(u_ids, i_ids)
    _check_review_tables(user_revs, user_rids, item_revs, item_rids, "R+1, T")
    R, T, dev = user_revs.shape[1] - 1, user_revs.shape[2], u_ids.device
    revs, word_masks, rev_masks, rids, ids = _gather_outputs(dev, 2 * B, _review_outputs(R, T),
                                                             (revs, word_masks, rev_masks, rids, ids))
    if B == 0:
        return revs, word_masks, rev_masks, rids, ids
    _call(None, _lib.lib().rbr_review_gather, B, R, T, dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"),
          dev_ptr(user_revs, I32, "user_revs"), dev_ptr(user_rids, I32, "user_rids"), user_revs.shape[0],
          dev_ptr(item_revs, I32, "item_revs"), dev_ptr(item_rids, I32, "item_rids"), item_revs.shape[0],
          int(bool(leave_one_out)), int(pad_token), int(replace_id), dev_ptr(revs, I64, "revs"),
          dev_ptr(word_masks.view(U8), U8, "word_masks"), dev_ptr(None if rev_masks is None else rev_masks.view(U8), U8, "rev_masks"),
          dev_ptr(rids, I64, "rids"), dev_ptr(ids, I64, "ids"), _id_err(dev).data_ptr(), current_stream())
    return revs, word_masks, rev_masks, rids, ids


def sentence_gather(u_ids: torch.Tensor, i_ids: torch.Tensor, user_revs: torch.Tensor, user_rids: torch.Tensor,
                    item_revs: torch.Tensor, item_rids: torch.Tensor, leave_one_out: bool, pad_token: int = 0, replace_id: int = 0,
                    revs: Optional[torch.Tensor] = None, sent_lens: Optional[torch.Tensor] = None,
                    sent_masks: Optional[torch.Tensor] = None, rev_masks: Optional[torch.Tensor] = None, rids=True, ids=True):
    """The id-fed sentence-split batch (rbr_sentence_gather, one launch): returns (revs2 [2B, R, S, W] int64, sent_lens2 [2B, R, S]
    int64, sent_masks2 [2B, R, S] bool, rev_masks2 [2B, R] bool, rids2 [2B, R] int64 or None, ids2 [2B] int64 or None), user rows
    first -- the halves are what SentenceDataset.collate_fn builds from the examples of the same pairs, with the lengths and masks
    of data.sentence_masks.  Tables: user_revs [U, R+1, S, W] / user_rids [U, R+1], item_revs [I, R+1, S, W] / item_rids [I, R+1],
    int32 (data.DeviceSentenceCache).  leave_one_out, bad ids and replace_id: as in review_gather.

    `revs` / `sent_lens` / `sent_masks` / `rev_masks`: stacked tensors to write into, or None to allocate; `rids` / `ids`: a stacked
    tensor, True to allocate, None / False to leave out.  No autograd, no sync: graph-capturable."""
    B = _pair_batch(u_ids, i_ids)
    _check_review_tables(user_revs, user_rids, item_revs, item_rids, "R+1, S, W")
    R, S, W = user_revs.shape[1] - 1, user_revs.shape[2], user_revs.shape[3]
    dev = u_ids.device
    revs, sent_lens, sent_masks, rev_masks, rids, ids = _gather_outputs(
        dev, 2 * B, (("revs", (R, S, W), I64, False), ("sent_lens", (R, S), I64, False), ("sent_masks", (R, S), torch.bool, False),
                     ("rev_masks", (R,), torch.bool, False), ("rids", (R,), I64, True), ("ids", (), I64, True)),
        (revs, sent_lens, sent_masks, rev_masks, rids, ids))
    if B == 0:
        return revs, sent_lens, sent_masks, rev_masks, rids, ids
    _call(None, _lib.lib().rbr_sentence_gather, B, R, S, W, dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"),
          dev_ptr(user_revs, I32, "user_revs"), dev_ptr(user_rids, I32, "user_rids"), user_revs.shape[0],
          dev_ptr(item_revs, I32, "item_revs"), dev_ptr(item_rids, I32, "item_rids"), item_revs.shape[0],
          int(bool(leave_one_out)), int(pad_token), int(replace_id), dev_ptr(revs, I64, "revs"),
          dev_ptr(sent_lens, I64, "sent_lens"), dev_ptr(sent_masks.view(U8), U8, "sent_masks"),
          dev_ptr(rev_masks.view(U8), U8, "rev_masks"), dev_ptr(rids, I64, "rids"), dev_ptr(ids, I64, "ids"),
          _id_err(dev).data_ptr(), current_stream())
    return revs, sent_lens, sent_masks, rev_masks, rids, ids


def review_sample_gather(u_ids: torch.Tensor, i_ids: torch.Tensor, user_revs: torch.Tensor, user_rids: torch.Tensor,
                         item_revs: torch.Tensor, item_rids: torch.Tensor, R: int, n_user: int, n_item: int, *, state, seed: int = 0,
                         leave_one_out: bool = True, pad_token: int = 0, replace_id: int = 0, revs: Optional[torch.Tensor] = None,
                         word_masks: Optional[torch.Tensor] = None, rev_masks=True, rids=True, ids=True, slots=None):
    """The id-fed TRAIN batch of the review split with review sampling (rbr_review_sample_gather, one launch): review_gather's
    outputs with R slots per row, of which the leading min(n_side, live) hold a fresh uniform random subset of the row's live
    candidate reviews in random order and the rest are empty reviews -- the reference's sample_train_review
    (trainer/train_simple_siamese.py:346-368).  Tables: user_revs [U, P+1, T] / user_rids [U, P+1], item_revs [I, P+1, T] /
    item_rids [I, P+1], int32, R <= P <= 63: the candidates are the P slots that review_gather's rule with P in place of R gives;
    a candidate is live when its review holds a token != pad_token.  The draw is stated in include/rbr_hip.h.

    `state`: int64 [2] on the device, [call number, 0]; the launch advances the call number itself, so two calls (or two replays
    of a recorded call) draw different sets, and (seed, call number) fixes a set exactly.
    Returns (revs2, word_masks2, rev_masks2, rids2, ids2, slots2): the first five as review_gather's (`revs` / `word_masks`:
    tensors to write into or None to allocate; `rev_masks` / `rids` / `ids`: a tensor, True to allocate, None / False to leave out);
    slots2 int32 [2B, R] -- the table slot each output slot was copied from, -1 for an empty one -- under the same convention
    (default: left out).  No autograd, no sync: graph-capturable."""
    B = _pair_batch(u_ids, i_ids)
    _check_review_tables(user_revs, user_rids, item_revs, item_rids, "P+1, T")
    P, T, R = user_revs.shape[1] - 1, user_revs.shape[2], int(R)
    if state.shape != (2,) or state.dtype != I64:
        raise RuntimeError(f"state must be int64 [2], got {state.dtype} {tuple(state.shape)}")
    if R < 1:
        raise RuntimeError(f"R must be >= 1, got {R}")
    dev = u_ids.device
    revs, word_masks, rev_masks, rids, ids, slots = _gather_outputs(
        dev, 2 * B, _review_outputs(R, T) + (("slots", (R,), I32, True),), (revs, word_masks, rev_masks, rids, ids, slots))
    if B == 0:
        return revs, word_masks, rev_masks, rids, ids, slots
    _call(None, _lib.lib().rbr_review_sample_gather, B, R, T, P, dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"),
          dev_ptr(user_revs, I32, "user_revs"), dev_ptr(user_rids, I32, "user_rids"), user_revs.shape[0],
          dev_ptr(item_revs, I32, "item_revs"), dev_ptr(item_rids, I32, "item_rids"), item_revs.shape[0],
          int(bool(leave_one_out)), int(n_user), int(n_item), int(pad_token), int(replace_id), int(seed) & 0xFFFFFFFFFFFFFFFF,
          dev_ptr(state, I64, "state"), dev_ptr(revs, I64, "revs"), dev_ptr(word_masks.view(U8), U8, "word_masks"),
          dev_ptr(None if rev_masks is None else rev_masks.view(U8), U8, "rev_masks"), dev_ptr(rids, I64, "rids"),
          dev_ptr(ids, I64, "ids"), dev_ptr(slots, I32, "slots"), _id_err(dev).data_ptr(), current_stream())
    return revs, word_masks, rev_masks, rids, ids, slots


def set_tap_sink(sink, table: Optional[torch.Tensor] = None) -> None:
    """Installs `sink` for the word table it exchanges (sink.table); set_tap_sink(None, table) removes that table's sink,
    set_tap_sink(None) removes all of them."""
    if sink is None:
        if table is None:
            _TAP_SINKS.clear()
        else:
            _TAP_SINKS.pop(table.data_ptr(), None)
        return
    _TAP_SINKS[sink.table.data_ptr()] = sink


# ---- one gradient buffer for several producers of a table's gradient ------------------------------------------------------
def _fanout_acc(table: torch.Tensor):
    """Called in an op's forward: the (buffer, stream) of the table_fanout `table` is an alias of, or None.  The buffer hangs on
    the fan-out's own autograd node, so concurrent or interleaved forwards / backwards of several steps cannot meet in one."""
    node = table.grad_fn
    return getattr(node, "acc", None) if type(node).__name__ == "_TableFanoutBackward" else None


def _table_acc(acc, device):
    """In an op's backward: the shared buffer when this op may add its rows to it (same stream as the fan-out), else None."""
    if acc is None or acc[1] != torch.cuda.current_stream(device):
        return None
    return acc[0]


class _TableFanout(torch.autograd.Function):
    """n aliases of a table, one per consumer.  The consumers' backwards that support it add their rows into ONE zeroed buffer
    (kept on this node) and each hand that same buffer back; here the duplicates are dropped, so a step with 8 producers of
    table gradient (D-ATT: two gates and two convs per tower) pays one 20 MB fill instead of seven 60 MB autograd adds and eight
    dense [V, D] outputs.  A consumer that returns a tensor of its own is added the ordinary way."""

    @staticmethod
    def forward(ctx, table, n):
        ctx.set_materialize_grads(False)
        ctx.acc = (torch.zeros_like(table), torch.cuda.current_stream(table.device))
        return tuple(table.view(table.shape) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        total, seen = None, set()
        for g in grads:
            if g is None or g.data_ptr() in seen:
                continue
            seen.add(g.data_ptr())
            total = g if total is None else total + g
        return total, None


def table_fanout(table: torch.Tensor, n: int):
    """`n` aliases of `table` for `n` consumer ops of one step (hand each op its own alias).  With gradients on, the ops that
    can (token-product convs and gates) then add their table-gradient rows into one shared buffer instead of producing a
    dense gradient each: see _TableFanout.  Without gradients: the table itself, n times."""
    if not (torch.is_grad_enabled() and table.requires_grad and table.is_cuda):
        return (table,) * n
    return _TableFanout.apply(table, n)


class _ConvSaved:
    """What a conv forward allocates (_conv_fwd_buffers) and what it leaves for its backward (a plain record: the fused encoder +
    head function shares the backward, D-ATT keeps one per tower)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _conv_desc(table, n_docs, L, ws, pad_mode, act, padding_idx, flags: int = 0):
    """Descriptor of the conv with the weights `ws` ([C_w, D, kz_w] each) over [n_docs, L] ids into `table`."""
    V, D = table.shape
    return _lib.make_desc(n_docs, L, D, V, [int(w.shape[2]) for w in ws], [int(w.shape[0]) for w in ws], pad_mode, act, padding_idx,
                          flags)


def _conv_operands(table, ids, mask, weights, pad_mode, act, padding_idx, flags: int = 0):
    """What every conv entry starts with: contiguous operands, the device / dtype gate before anything touches HIP, the mask
    check and the descriptor.  Returns (table_c, ids, mask8, ws, desc)."""
    table_c = table.contiguous()
    dev_ptr(table_c, F32, "word table")
    if ids.dim() != 2:
        raise RuntimeError("ids must be [n_docs, L]")
    ids = ids.contiguous()
    mask8 = _mask_u8(mask)
    if mask8 is not None and mask8.shape != ids.shape:
        raise AssertionError("inputs.shape[:-1] == masks.shape")   # deepconn/utils.py:58
    ws = [w.contiguous() for w in weights]
    return table_c, ids, mask8, ws, _conv_desc(table_c, ids.shape[0], ids.shape[1], ws, pad_mode, act, padding_idx, flags)


# ---- forward workspaces that are KEPT from call to call: the two-launch prepare stage (rbr_textcnn_prod_prepare_ids_kept) -------
# That entry finds the workspace's list state zero and leaves it zero, so somebody has to own the workspace between calls.
# Eager calls: a free list per (device, stream) -- calls on one stream are ordered --; a workspace is out on loan for as long as
# anything holds the tensor a checkout returned (the forward's record, the row-form gradient that still reads its token list).
# Recorded steps: the graph keeps the workspace's ADDRESS, so the workspace must live as long as the graph and serve nobody else:
# the recording object opens kept_ws_owner(list) around its capture and the workspaces move into that list.  A capture without
# an owner, or without a free workspace on its stream (prepare_stream_state creates them ahead of a recording: a buffer made during
# a capture would sit in the graph's private pool, where a later tensor may be laid over it), gets None: the three-launch chain.
# RBR_PREP_TWO_LAUNCH=0 switches the whole thing off (the A/B of DESIGN.md section 4.14: 0.3442 / 0.3477 ms per cfg2 step with
# the switch off against 0.3374 - 0.3425 with it on; the prepare stage 21.0 -> 16.2 us).
_KEPT_WS: dict = {}          # (device index, stream handle) -> [_KeptWs]
_KEPT_OWNER: list = []       # innermost kept_ws_owner() list


def _kept_state(desc):
    """((offset, bytes) x 3) of a forward workspace's list state: marks, row mask, the two kept counter words."""
    off = (C.c_int64 * 6)()
    check(_lib.lib().rbr_textcnn_prod_list_state(C.byref(desc), off), "rbr_textcnn_prod_list_state")
    return tuple((int(off[k]), int(off[k + 1])) for k in (0, 2, 4))


class _KeptWs:
    def __init__(self, state, nbytes, dev):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.busy, self.state = False, state          # (workspaces of one size and one state layout are interchangeable)
        self.zero()

    def fits(self, state, nbytes) -> bool:
        return self.buf.numel() == nbytes and self.state == state

    def zero(self):
        for o, n in self.state:
            self.buf[o:o + n].zero_()
        self.dirty = False


class _KeptLease:
    def __init__(self, ws):
        self.ws = ws
        ws.busy = True

    def __del__(self):
        self.ws.busy = False


@contextlib.contextmanager
def kept_ws_owner(owned: list):
    """with kept_ws_owner(self._kept): <capture> -- forward workspaces a recording takes are appended to `owned`, which must
    live as long as the recorded graph (train_step.GraphedTrainStep / GraphedForward)."""
    _KEPT_OWNER.append(owned)
    try:
        yield owned
    finally:
        _KEPT_OWNER.pop()


def _kept_ws_checkout(desc, nbytes, dev):
    """A workspace of `nbytes` whose list state is zero, as a tensor that carries its loan, or None (see above)."""
    if os.environ.get("RBR_PREP_TWO_LAUNCH", "1") == "0":
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    free = _KEPT_WS.setdefault((idx, torch.cuda.current_stream(idx).cuda_stream), [])
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and not _KEPT_OWNER:
        return None
    state = _kept_state(desc)
    ws = next((w for w in free if not w.busy and w.fits(state, nbytes) and not (capturing and w.dirty)), None)
    if ws is None:
        if capturing:
            return None
        ws = _KeptWs(state, nbytes, dev)
        free.append(ws)
    elif ws.dirty:
        ws.zero()
    t = ws.buf[:]                    # a tensor object of this checkout's own: the loan lives and dies with it
    t._kept = ws
    if capturing:
        free.remove(ws)
        _KEPT_OWNER[-1].append(ws)
    else:
        t._kept_lease = _KeptLease(ws)
    return t


def _kept_ws_prepare_stream(dev, idx) -> None:
    """For every (size, descriptor) a stream of the device has used: a free workspace on the CURRENT stream."""
    cur = _KEPT_WS.setdefault((idx, torch.cuda.current_stream(idx).cuda_stream), [])
    seen = {(w.buf.numel(), w.state) for (d, _), lst in list(_KEPT_WS.items()) if d == idx for w in lst}
    for n, state in seen:
        if not any(c.fits(state, n) and not c.busy and not c.dirty for c in cur):
            cur.append(_KeptWs(state, n, dev))


def _conv_fwd_buffers(rec, desc, dev, feat=None, argmax=None, kept=False):
    """Plan queries and output buffers of a conv forward, left on the record `rec` -- allocations only, nothing launches: pval /
    pidx (the pool's per-slab partials), feat / argmax [n_docs, C] (or the caller's views) and prod_ws, the workspace of the
    token-product formulation (None: it does not apply to this shape, the dense formulation runs).  kept: prod_ws from the kept
    workspaces when one is to be had (its tensor then has `_kept`: _prod_forward takes the two-launch prepare stage)."""
    L_ = _lib.lib()
    n_part = L_.rbr_textcnn_partial_elems(C.byref(desc))
    if not n_part:
        check(-1, "rbr_textcnn plan")
    ws_bytes = L_.rbr_textcnn_fwd_ws_bytes(C.byref(desc))      # > 0: the token-product formulation will run
    Ctot = sum(desc.ch[:desc.n_widths])
    rec.pval = torch.empty(n_part, dtype=F32, device=dev)
    rec.pidx = torch.empty(n_part, dtype=I32, device=dev)
    rec.feat = feat if feat is not None else torch.empty(desc.n_docs, Ctot, dtype=F32, device=dev)
    rec.argmax = argmax if argmax is not None else torch.empty(desc.n_docs, Ctot, dtype=I32, device=dev)
    rec.prod_ws = (_kept_ws_checkout(desc, ws_bytes, dev) if kept else None) if ws_bytes else None
    if rec.prod_ws is None and ws_bytes:
        rec.prod_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    return rec


def _prod_forward(desc, rec, table, ids, mask8, gate, ws, st, *, id_sets=None, prepare_key="textcnn_prod_prepare"):
    """The token-product forward, stage by stage (each stage is what rbr_textcnn_conv_fwd would run): prepare -> table -> pool,
    into rec.pval / rec.pidx (_conv_fwd_buffers).  Library calls only, so that D-ATT can issue it inside a pair region (where its
    prepare stage has never been bracketed: prepare_key None).  id_sets = (n, IdSet array, error record): the range check of
    the raw id tensors rides in the prepare stage's first launch (rbr_textcnn_prod_prepare_ids)."""
    L_ = _lib.lib()
    d, wsp = C.byref(desc), rec.prod_ws.data_ptr()
    ids_p, mask_p, pidx_p = dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"), dev_ptr(rec.pidx, I32, "pidx")
    kept = getattr(rec.prod_ws, "_kept", None) if id_sets is not None else None
    if kept is not None:
        # two launches (check + mark + scan | list + weight images) on a workspace whose list state stays zero; after an error the
        # state is undefined: the owner clears it before the next use
        try:
            _call(prepare_key, L_.rbr_textcnn_prod_prepare_ids_kept, d, *id_sets, ids_p, mask_p, ptr_array(ws, F32, "conv weight"),
                  pidx_p, wsp, st)
        except Exception:
            kept.dirty = True
            raise
    elif id_sets is not None:
        _call(prepare_key, L_.rbr_textcnn_prod_prepare_ids, d, *id_sets, ids_p, mask_p, ptr_array(ws, F32, "conv weight"), pidx_p,
              wsp, st)
    else:
        _call(prepare_key, L_.rbr_textcnn_prod_prepare, d, ids_p, mask_p, ptr_array(ws, F32, "conv weight"), pidx_p, wsp, st)
    _call("textcnn_prod_table", L_.rbr_textcnn_prod_table, d, dev_ptr(table, F32, "word table"), wsp, st)
    _call("textcnn_prod_pool", L_.rbr_textcnn_prod_pool, d, ids_p, mask_p, dev_ptr(gate, F32, "gate"), dev_ptr(rec.pval, F32, "pval"),
          pidx_p, wsp, st)


def _pool_finalize(desc, rec, bs, st):
    """feat / argmax from the pool's partials (either formulation) and the conv biases."""
    _call(None, _lib.lib().rbr_textcnn_pool_finalize, C.byref(desc), dev_ptr(rec.pval, F32, "pval"), dev_ptr(rec.pidx, I32, "pidx"),
          ptr_array(bs, F32, "conv bias"), dev_ptr(rec.feat, F32, "feat"), dev_ptr(rec.argmax, I32, "argmax"), st)


class _TextCNN(torch.autograd.Function):
    """feat[n_docs, C] = pool(act(conv(mask * gate * table[ids])))  -- see rbr_textcnn_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, table, gate, ids, mask, kernel_sizes, pad_mode, act, padding_idx, conv_flags, *wb):
        ctx.fanout_acc = _fanout_acc(table)
        n = len(kernel_sizes)
        weights, biases = wb[:n], wb[n:]
        table_c, ids, mask8, ws, desc = _conv_operands(table, ids, mask, weights, pad_mode, act, padding_idx, conv_flags)
        for k, w, b in zip(kernel_sizes, weights, biases):
            assert w.shape[1] == table.shape[1] and w.shape[2] == k and b.shape[0] == w.shape[0]
        bs = [b.contiguous() for b in biases]
        if gate is not None:
            gate = gate.contiguous()
        L_ = _lib.lib()
        dev = table.device
        n_packed = L_.rbr_textcnn_packed_floats(C.byref(desc))
        if not n_packed:
            check(-1, "rbr_textcnn plan")
        buf = _conv_fwd_buffers(_ConvSaved(), desc, dev)
        st = current_stream()
        packed = None         # MFMA tile image of the conv weights: the dense forward and the scatter backward read it
        if buf.prod_ws is not None:
            _prod_forward(desc, buf, table_c, ids, mask8, gate, ws, st)
        else:
            packed = _TextCNN._pack(L_, desc, ws, n_packed, dev, st)
            _call("textcnn_conv_fwd", L_.rbr_textcnn_conv_fwd, C.byref(desc), dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
                  dev_ptr(gate, F32, "gate"), dev_ptr(table_c, F32, "word table"), ptr_array(ws, F32, "conv weight"),
                  dev_ptr(packed, F32, "packed"), dev_ptr(buf.pval, F32, "pval"), dev_ptr(buf.pidx, I32, "pidx"), None, st)
        _pool_finalize(desc, buf, bs, st)
        feat, argmax = buf.feat, buf.argmax
        ctx.desc = desc
        ctx.n = n
        ctx.has_gate = gate is not None
        ctx.has_mask = mask8 is not None
        ctx.prod_ws = buf.prod_ws      # distinct-token list of the batch, reused by the table-gradient GEMM
        ctx.save_for_backward(table_c, ids, packed, feat, argmax, *([mask8] if mask8 is not None else []),
                              *([gate] if gate is not None else []), *ws)
        ctx.mark_non_differentiable(argmax)
        ctx.set_materialize_grads(False)        # no zero-filled "gradient" tensor for argmax (a fill launch per step)
        return feat, argmax

    @staticmethod
    def _pack(L_, desc, ws, n_packed, dev, st):
        packed = torch.empty(n_packed, dtype=F32, device=dev)
        _call(None, L_.rbr_textcnn_pack, C.byref(desc), ptr_array(ws, F32, "conv weight"), dev_ptr(packed, F32, "packed"), st)
        return packed

    @staticmethod
    def backward(ctx, d_feat, _d_argmax):
        saved = list(ctx.saved_tensors)
        table, ids, packed, feat, argmax = saved[:5]
        k = 5
        mask8 = None
        gate = None
        if ctx.has_mask:
            mask8 = saved[k]; k += 1
        if ctx.has_gate:
            gate = saved[k]; k += 1
        S = _ConvSaved(table=table, ids=ids, packed=packed, feat=feat, argmax=argmax, mask8=mask8, gate=gate, ws=list(saved[k:]),
                       desc=ctx.desc, prod_ws=ctx.prod_ws, fanout_acc=ctx.fanout_acc)
        dtable, dgate, dWs, dbs = _textcnn_backward(S, d_feat, ctx.needs_input_grad[0], ctx.has_gate and ctx.needs_input_grad[1])
        return (dtable, dgate, None, None, None, None, None, None, None, *dWs, *dbs)


# ---- backward of the fused encoder: one dispatcher, one function per table-gradient strategy, the weight-gradient chain ------
class _Fork:
    """The second stream of `dev` (_side_stream), forked from the current stream HERE: the event is recorded at construction.
    `with fork:` -- now or after more work has been enqueued on the current stream -- runs its body on the second stream behind
    the fork point; fork.join() makes the current stream wait for that body.  Inside a captured graph the two become parallel
    branches.  on=False, or RBR_BWD_OVERLAP=0: the body runs inline on the current stream."""

    def __init__(self, dev, on: bool = True):
        self.side = _side_stream(dev) if on else None
        self.done = None
        if self.side is not None:
            self.forked = torch.cuda.Event()
            self.forked.record()

    def __enter__(self):
        if self.side is not None:
            self.side.wait_event(self.forked)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.side is not None:
            if exc[0] is None:
                self.done = torch.cuda.Event()
                self.done.record()
            self._ctx.__exit__(*exc)
        return False

    def join(self) -> None:
        _join(self.done)


def _g_chain(key, flags, st, desc, operands, fwd_ws, bws, dtable, dgate, sq):
    """rbr_textcnn_bwd_dtable_prod_ex on the raw stream `st`: the token-product table gradient over the forward's distinct-token
    list in `fwd_ws`.  flags: the phases -- G_BUILD (G in `bws`, and dgate, from operands = (ids, mask8, gate, feat, argmax,
    d_feat)), G_PRODUCT (dtable [, sq] = G @ Wprod^T) -- plus G_ACCUMULATE / G_ROWS for the product.  What a phase that is not
    asked for would read or write is passed as NULL.  key: the TIMER key of the call, or None."""
    build, product = flags & _lib.G_BUILD, flags & _lib.G_PRODUCT
    ids, mask8, gate, feat, argmax, d_feat = operands if build else (None,) * 6
    _call(key, _lib.lib().rbr_textcnn_bwd_dtable_prod_ex, C.byref(desc), dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
          dev_ptr(gate, F32, "gate"), dev_ptr(feat, F32, "feat"), dev_ptr(argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"),
          fwd_ws.data_ptr(), bws.data_ptr(), dev_ptr(dtable if product else None, F32, "dtable"),
          dev_ptr(dgate if build else None, F32, "dgate"), dev_ptr(sq if product else None, F32, "sq_part"), flags, st)


def _textcnn_backward(S, d_feat, need_table: bool, need_gate: bool, side_job=None):
    """Backward of the fused encoder from d_feat [n_docs, C]: returns (dtable, dgate, dWs, dbs).  dtable is None when the table
    gradient left through a side channel instead: the data-parallel tap sink, or -- compact row form -- the optimizer that
    registered for it (set_row_grad_sink).  Picks the table-gradient strategy; each one also runs the weight-gradient chain.
    Precedence: tap sink (one that accepts the call wins over fixed mode), fixed point, token product, token list, window scatter.
    side_job: a callable that enqueues work independent of this backward on the current stream; it runs on the weight-gradient
    branch, behind the weight-gradient kernels, inside the same fork and join (_EncodeHead: what is left of the head's backward)."""
    L_ = _lib.lib()
    table, gate, desc = S.table, S.gate, S.desc
    dev = table.device
    d_feat = (torch.zeros_like(S.feat) if d_feat is None else d_feat).contiguous()
    dWs = [torch.empty_like(w) for w in S.ws]
    dbs = [torch.empty(w.shape[0], dtype=F32, device=dev) for w in S.ws]
    plain = need_table and gate is None          # the tap and token-list forms of the table gradient serve un-gated convs only
    sink = _TAP_SINKS.get(table.data_ptr())          # only the sink installed for THIS table ever sees the call
    if plain and sink is not None and sink.accepts(table, desc, L_):
        dtable, dgate = _bwd_tap_sink(S, d_feat, sink, dWs, dbs, side_job)
    elif plain and _dtable_fixed() and (fixed_bytes := L_.rbr_textcnn_dtable_from_taps_ws_bytes(C.byref(desc), 1)):
        dtable, dgate = _bwd_fixed(S, d_feat, fixed_bytes, dWs, dbs, side_job)
    elif (need_table or need_gate) and S.prod_ws is not None and (bws_bytes := L_.rbr_textcnn_bwd_prod_ws_bytes(C.byref(desc))):
        dtable, dgate = _bwd_token_product(S, d_feat, need_table, need_gate, bws_bytes, dWs, dbs, side_job)
    elif plain and (list_bytes := L_.rbr_textcnn_bwd_dtable_list_ws_bytes(C.byref(desc))):
        dtable, dgate = _bwd_token_list(S, d_feat, list_bytes, dWs, dbs, side_job)
    else:
        dtable, dgate = _bwd_window_scatter(S, d_feat, need_table, need_gate, dWs, dbs, side_job)
    return dtable, dgate, dWs, dbs


def _bwd_dw(S, d_feat, dWs, dbs, fork, side_job=None) -> None:
    """The weight-gradient chain (rbr_textcnn_bwd_dw) on `fork`'s stream, joined before returning.  The weight-gradient kernels
    and the table-gradient kernels both start from d_feat and share nothing else: the former go to a second stream, so the two
    chains overlap -- also inside a captured graph, where the fork becomes two parallel branches.  A strategy forks BEFORE its
    table-gradient chain and calls this AFTER it: in a replayed graph the branch captured first keeps the queue of the nodes
    before and after the fork, and the join of the other branch into that queue costs ~10 us -- so the longer (table) branch goes
    first and the step's next kernel follows it without a gap."""
    L_ = _lib.lib()
    wsb = torch.empty(max(L_.rbr_textcnn_bwd_ws_floats(C.byref(S.desc)), 1), dtype=F32, device=S.table.device)
    with fork:
        _call("textcnn_bwd_dw", L_.rbr_textcnn_bwd_dw, C.byref(S.desc), dev_ptr(S.ids, I64, "ids"), dev_ptr(S.mask8, U8, "mask"),
              dev_ptr(S.gate, F32, "gate"), dev_ptr(S.table, F32, "table"), dev_ptr(S.feat, F32, "feat"),
              dev_ptr(S.argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"), ptr_array(dWs, F32, "dW"),
              ptr_array(dbs, F32, "dbias"), dev_ptr(wsb, F32, "ws"), current_stream())
        # side_job BEHIND the weight-gradient kernels.  (Measured and dropped, round 7: in front of them -- head_bwd then takes
        # 29 us beside the zero fill and the G build, dw_partial4 starts 35 us later and the join waits for this branch: the step
        # 0.377-0.379 ms against 0.348-0.351.)
        if side_job is not None:
            side_job()
    fork.join()


def _bwd_taps(key, S, d_feat, tok, val) -> None:
    """(token, value) taps of an un-gated conv's table gradient: rbr_textcnn_bwd_taps."""
    _call(key, _lib.lib().rbr_textcnn_bwd_taps, C.byref(S.desc), dev_ptr(S.ids, I64, "ids"), dev_ptr(S.mask8, U8, "mask"),
          dev_ptr(S.feat, F32, "feat"), dev_ptr(S.argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"),
          dev_ptr(tok, I32, "tap tokens"), dev_ptr(val, F32, "tap values"), current_stream())


def _bwd_tap_sink(S, d_feat, sink, dWs, dbs, side_job=None):
    """Data-parallel tap sink: the taps go to the exchange, which produces table.grad after the all-gather -- no dtable here."""
    dev = S.table.device
    fork = _Fork(dev)
    tok, val = sink.local_buffers(_lib.lib().rbr_textcnn_taps_count(C.byref(S.desc)), dev)
    _bwd_taps("textcnn_bwd_dtable", S, d_feat, tok, val)
    sink.record(S.desc, list(S.ws))
    _bwd_dw(S, d_feat, dWs, dbs, fork, side_job)
    return None, None


def _bwd_fixed(S, d_feat, fixed_bytes, dWs, dbs, side_job=None):
    """set_dtable_mode("fixed"): order-free fixed-point sums, the data-parallel tap rebuild run on this rank's taps alone.  The
    weight gradient follows on the same stream."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("RBR_DTABLE_MODE=fixed sorts with rocPRIM and cannot be recorded into a hipGraph: run the step eagerly")
    L_ = _lib.lib()
    dev = S.table.device
    n_taps = L_.rbr_textcnn_taps_count(C.byref(S.desc))
    tok = torch.empty(n_taps, dtype=I32, device=dev)
    val = torch.empty(n_taps, dtype=F32, device=dev)
    tws = torch.empty(fixed_bytes, dtype=torch.uint8, device=dev)
    dtable = torch.empty_like(S.table)
    _bwd_taps(None, S, d_feat, tok, val)
    _call(None, L_.rbr_textcnn_dtable_from_taps, C.byref(S.desc), 1, dev_ptr(tok, I32, "tap tokens"), dev_ptr(val, F32, "tap values"),
          ptr_array(S.ws, F32, "conv weight"), tws.data_ptr(), dev_ptr(dtable, F32, "dtable"), current_stream())
    _bwd_dw(S, d_feat, dWs, dbs, _Fork(dev, on=False), side_job)
    return dtable, None


def _bwd_token_product(S, d_feat, need_table, need_gate, bws_bytes, dWs, dbs, side_job=None):
    """Token-product backward: dtable = G @ Wprod^T over the forward's distinct-token list (no atomics on the table); d(gate) of
    gated convs (D-ATT) is read off the forward's product table.  Returns (dtable, dgate); dtable is None when the rows went to
    the optimizer's row sink."""
    L_ = _lib.lib()
    table, desc = S.table, S.desc
    dev = table.device
    st = current_stream()
    # many short documents (NARRE's reviews): dW = G^T @ table[distinct tokens] on the MFMA pipe, from the G the
    # table-gradient call builds anyway (0 floats of workspace = not this shape: the window-row kernels of _bwd_dw)
    dwg_floats = L_.rbr_textcnn_bwd_dw_from_g_ws_floats(C.byref(desc)) if need_table else 0
    acc = _table_acc(S.fanout_acc, dev) if need_table else None
    # compact row gradient: the optimizer that asked for it takes the rows of the batch's tokens, nobody writes (or later
    # reads) the zero rows of a dense [V, D] gradient
    row_sink = _row_grad_sink_for(table) if (need_table and S.gate is None and acc is None) else None
    flags, out, sq = 0, None, None
    if row_sink is not None:
        cap, rot = C.c_int32(0), C.c_void_p()
        _call(None, L_.rbr_textcnn_token_list, C.byref(desc), S.prod_ws.data_ptr(), C.byref(rot), None, None, C.byref(cap))
        out = torch.empty(cap.value, table.shape[1], dtype=F32, device=dev)
        sq = torch.empty(L_.rbr_textcnn_row_grad_partials(C.byref(desc)), dtype=F32, device=dev)   # one per workgroup
        flags = _lib.G_ROWS
    elif acc is not None and not dwg_floats:          # shared gradient buffer of the step (table_fanout): rows added, buffer handed back
        out, flags = acc, _lib.G_ACCUMULATE
    elif need_table:
        out = torch.empty_like(table)          # the token-list backwards overwrite the whole table gradient
    # the token-product backward zeroes dgate in the launch that zeroes its G rows
    dgate = torch.empty_like(S.gate) if need_gate else None
    bws = torch.empty(bws_bytes, dtype=torch.uint8, device=dev)

    def g(key, phases):
        _g_chain(key, phases, st, desc, (S.ids, S.mask8, S.gate, S.feat, S.argmax, d_feat), S.prod_ws, bws, out, dgate, sq)

    fork = None if dwg_floats else _Fork(dev)          # the weight chain of _bwd_dw, forked ahead of the table chain
    ev = TIMER.record("textcnn_bwd_dtable")
    if dwg_floats or (ev is not None and out is not None):
        g(None, _lib.G_BUILD)
        if dwg_floats:
            # G first; then its two consumers side by side: dtable = G @ Wprod^T on this stream, dW = G^T @ table rows on the
            # second one (fork after the build, join before returning; two parallel branches in a captured graph)
            dwg_ws = torch.empty(dwg_floats, dtype=F32, device=dev)
            fork = _Fork(dev)
            with fork:
                _call("textcnn_bwd_dw", L_.rbr_textcnn_bwd_dw_from_g, C.byref(desc), dev_ptr(table, F32, "table"),
                      dev_ptr(S.feat, F32, "feat"), dev_ptr(d_feat, F32, "d_feat"), S.prod_ws.data_ptr(), bws.data_ptr(),
                      ptr_array(dWs, F32, "dW"), ptr_array(dbs, F32, "dbias"), dev_ptr(dwg_ws, F32, "ws"), current_stream())
                if side_job is not None:
                    side_job()
        else:
            # timing pass (bench.py): the call's two phases as two calls, so that the sparse product (ONE launch,
            # g_times_w) gets HIP events of its own -- same kernels, same order, same arguments
            ev.record()
            ev = None
        g("textcnn_bwd_g_product", _lib.G_PRODUCT | flags)
    else:
        g(None, _lib.G_BUILD | _lib.G_PRODUCT | flags)
    if ev is not None:
        ev.record()
    if dwg_floats:
        fork.join()
    else:
        _bwd_dw(S, d_feat, dWs, dbs, fork, side_job)
    if row_sink is not None:
        row_sink.put_row_grad(table, RowGradient(table, out, sq, rot.value, S.prod_ws))
        return None, dgate
    return out, dgate


def _bwd_token_list(S, d_feat, list_bytes, dWs, dbs, side_job=None):
    """Dense forward (no token list of its own), un-gated: the table gradient still goes through a distinct-token list built
    here (16 us) instead of the window scatter's row of f32 atomics per (document, channel, tap)."""
    dev = S.table.device
    dtable = torch.empty_like(S.table)          # the token-list backwards overwrite the whole table gradient
    lws = torch.empty(list_bytes, dtype=torch.uint8, device=dev)
    fork = _Fork(dev)
    _call("textcnn_bwd_dtable", _lib.lib().rbr_textcnn_bwd_dtable_list, C.byref(S.desc), dev_ptr(S.ids, I64, "ids"),
          dev_ptr(S.mask8, U8, "mask"), ptr_array(S.ws, F32, "conv weight"), dev_ptr(S.feat, F32, "feat"),
          dev_ptr(S.argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"), lws.data_ptr(), dev_ptr(dtable, F32, "dtable"),
          current_stream())
    _bwd_dw(S, d_feat, dWs, dbs, fork, side_job)
    return dtable, None


def _bwd_window_scatter(S, d_feat, need_table, need_gate, dWs, dbs, side_job=None):
    """Window scatter (rbr_textcnn_bwd_dtable): a row of f32 atomics per (document, channel, tap) into zeros, dgate likewise.
    Also where a backward that owes neither gradient ends up: the call then returns at once.  Returns (dtable, dgate)."""
    L_ = _lib.lib()
    dev = S.table.device
    dtable = torch.zeros_like(S.table) if need_table else None
    dgate = torch.zeros_like(S.gate) if need_gate else None
    fork = _Fork(dev, on=need_table or need_gate)
    st = current_stream()
    with _timed("textcnn_bwd_dtable"):
        packed = S.packed
        if packed is None:
            packed = _TextCNN._pack(L_, S.desc, S.ws, L_.rbr_textcnn_packed_floats(C.byref(S.desc)), dev, st)
        _call(None, L_.rbr_textcnn_bwd_dtable, C.byref(S.desc), dev_ptr(S.ids, I64, "ids"), dev_ptr(S.mask8, U8, "mask"),
              dev_ptr(S.gate, F32, "gate"), dev_ptr(S.table, F32, "table"), dev_ptr(packed, F32, "packed"),
              dev_ptr(S.feat, F32, "feat"), dev_ptr(S.argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"),
              dev_ptr(dtable, F32, "dtable"), dev_ptr(dgate, F32, "dgate"), st)
    _bwd_dw(S, d_feat, dWs, dbs, fork, side_job)
    return dtable, dgate


# ---- compact row gradient of an embedding table (consumer: train_step.HipClipAdam) ------------------------------------------
# word-table data_ptr -> weakref of the sink: wants_row_grad(table) -> bool, put_row_grad(table, RowGradient).  Weak: a registry
# entry never keeps an optimizer (and with it the parameters and Adam state it holds) alive, and a sink that was dropped
# without being unregistered simply disappears (the backward then produces the dense gradient again).
_ROW_GRAD_SINKS: dict = {}


def set_row_grad_sink(table: torch.Tensor, sink) -> None:
    """Registers `sink` (None: removes it) for the gradient of `table` in compact row form.  A conv backward over `table` hands
    sink.put_row_grad(table, RowGradient) the rows of the batch's tokens and returns no dense [V, D] gradient ONLY while
    sink.wants_row_grad(table) answers True for that backward -- the sink says per step whether it is the one that will consume
    the gradient (train_step.HipClipAdam: inside its row_grad_scope(), which train_step() / GraphedTrainStep open around the
    forward + backward of a step this optimizer drives).  Every other backward gets the ordinary dense gradient."""
    if sink is None:
        _ROW_GRAD_SINKS.pop(table.data_ptr(), None)
    else:
        _ROW_GRAD_SINKS[table.data_ptr()] = weakref.ref(sink)


def _row_grad_sink_for(table: torch.Tensor):
    """The live sink that wants THIS backward's gradient of `table` in row form, or None."""
    ref = _ROW_GRAD_SINKS.get(table.data_ptr())
    if ref is None:
        return None
    sink = ref()
    if sink is None:                                   # the optimizer is gone: forget the entry
        _ROW_GRAD_SINKS.pop(table.data_ptr(), None)
        return None
    return sink if sink.wants_row_grad(table) else None


class RowGradient:
    """Gradient of an embedding table as the rows of the tokens one batch holds (rbr_textcnn_bwd_dtable_prod_ex, RBR_G_ROWS):
    rows [cap, D] (row r = token tok_of_row[r] of the forward's list), sq [partials] = sums of squares of the rows, and the
    list's inverse map row_of_token [V] inside the forward's workspace (kept alive here).  Every other row of the dense
    gradient nn.Embedding's backward would build is exactly zero.
    coef: None, or the device scalar a clipping optimizer step left (rbr_clip_adam_step_rows does not re-write `rows`): the
    gradient is then rows * coef, which to_dense() applies -- one f32 multiply per element, on the device (capturable)."""

    def __init__(self, table, rows, sq, row_of_token_ptr, keep_alive):
        self.V, self.D = int(table.shape[0]), int(table.shape[1])
        self.rows, self.sq, self.row_of_token_ptr, self._keep = rows, sq, int(row_of_token_ptr), keep_alive
        self.coef = None

    def to_dense(self) -> torch.Tensor:
        rows = self.rows if self.coef is None else self.rows * self.coef
        dense = torch.empty(self.V, self.D, dtype=F32, device=self.rows.device)
        _call(None, _lib.lib().rbr_row_grad_to_dense, self.V, self.D, self.row_of_token_ptr, dev_ptr(rows, F32, "rows"),
              dev_ptr(dense, F32, "dense"), current_stream())
        return dense


_SIDE_STREAMS: dict = {}


def _side_stream(dev):
    """The second stream of `dev` for the weight-gradient chain (None: RBR_BWD_OVERLAP=0)."""
    if os.environ.get("RBR_BWD_OVERLAP", "1") == "0":
        return None
    s = _SIDE_STREAMS.get(dev)
    if s is None:
        s = _SIDE_STREAMS[dev] = torch.cuda.Stream(device=dev)
        _lib.FORKED_STREAMS.add(s.cuda_stream)          # forked and joined with events by its users: fine inside a capture
    return s


def _join(event) -> None:
    if event is not None:
        torch.cuda.current_stream().wait_event(event)


def _pad_runs_flag(pad_runs: bool, mask, padding_idx) -> int:
    """CONV_PAD_RUNS when the caller vouches for the runs of padding (see textcnn), the conv is un-masked and has a padding
    token, and RBR_PAD_RUNS=0 does not switch the encoding off."""
    on = pad_runs and mask is None and padding_idx is not None and os.environ.get("RBR_PAD_RUNS", "1") != "0"
    return _lib.CONV_PAD_RUNS if on else 0


def textcnn(table: torch.Tensor, ids: torch.Tensor, mask: Optional[torch.Tensor], weights: Sequence[torch.Tensor],
            biases: Sequence[torch.Tensor], *, gate=None, pad_mode: int = PAD_SAME,
            act: int = ACT_RELU, padding_idx: Optional[int] = 0, return_argmax: bool = False, pad_runs: bool = False,
            gate_split: int = 0):
    """Fused WordEmbedding -> masked_tensor -> MyConv1d -> act -> MaxPool1d(seq_len).

    table [V,D] f32; ids [n_docs,L] int64; mask [n_docs,L] bool or None; weights[w] [C_w,D,kz_w];
    biases[w] [C_w].  Returns feat [n_docs, sum C_w] (width-major channels).
    pad_runs (un-masked convs only): the caller vouches that `gate` is the same at every position whose tokens are all
    padding_idx within 8 positions either side (RBR_CONV_PAD_RUNS): runs of padding are then encoded once, exactly."""
    kernel_sizes = tuple(int(w.shape[2]) for w in weights)
    flags = _pad_runs_flag(pad_runs, mask, padding_idx)
    if gate_split:
        # two gates (RBR_CONV_GATE_SPLIT): banks [0, gate_split) under gate[0], the rest under gate[1]; token-product path only
        if not (isinstance(gate, (tuple, list)) and len(gate) == 2 and 0 < gate_split < len(weights)):
            raise RuntimeError("gate_split needs gate=(gate_a, gate_b) and 0 < gate_split < number of banks")
        gate = torch.stack([gate[0], gate[1]])          # [2, n_docs, L]; its backward hands each gate its plane
        flags |= _lib.conv_gate_split(gate_split)
    feat, argmax = _TextCNN.apply(table, gate, ids, mask, kernel_sizes, pad_mode, act, padding_idx, flags, *weights, *biases)
    return (feat, argmax) if return_argmax else feat


def textcnn_product_applies(table: torch.Tensor, ids: torch.Tensor, weights: Sequence[torch.Tensor], pad_mode: int, act: int,
                            padding_idx: Optional[int]) -> bool:
    """True when textcnn() over these shapes runs the token-product formulation, forward AND table-gradient backward (the only
    one that takes a split gate)."""
    desc = _conv_desc(table, ids.shape[0], ids.shape[1], weights, pad_mode, act, padding_idx)
    L_ = _lib.lib()
    return bool(table.is_cuda and L_.rbr_textcnn_fwd_ws_bytes(C.byref(desc)) > 0 and L_.rbr_textcnn_bwd_prod_ws_bytes(C.byref(desc)) > 0)


def textcnn_saliency(table: torch.Tensor, ids: torch.Tensor, mask: Optional[torch.Tensor], weights: Sequence[torch.Tensor],
                     feat: torch.Tensor, argmax: torch.Tensor, d_feat: torch.Tensor, *, gate=None, pad_mode: int = PAD_SAME,
                     act: int = ACT_RELU, gate_split: int = 0) -> torch.Tensor:
    """sal [n_docs, L]: what every token position contributes to a score whose gradient on the pooled features of textcnn() is
    d_feat [n_docs, C] -- gradient x input of the embedded, masked, gated rows with the max-pool routing (feat / argmax
    [n_docs, C], as textcnn(return_argmax=True) returned them) held fixed; rbr_textcnn_saliency in rbr_hip.h has the formula.
    One launch, no autograd, no embedded rows are materialised; a document's row is bit-identical in every batch.
    gate_split: a split gate (see textcnn) is refused by the library."""
    table_c, ids, mask8, ws, desc = _conv_operands(table, ids, mask, weights, pad_mode, act, None,
                                                   _lib.conv_gate_split(gate_split) if gate_split else 0)
    n_docs, L = ids.shape
    Ctot = sum(int(w.shape[0]) for w in ws)
    for w in ws:
        if w.dim() != 3 or w.shape[1] != table_c.shape[1]:
            raise RuntimeError(f"conv weights must be [C_w, D = {table_c.shape[1]}, kz_w], got {tuple(w.shape)}")
    feat, argmax, d_feat = feat.detach().contiguous(), argmax.contiguous(), d_feat.detach().contiguous()
    for t, name in ((feat, "feat"), (argmax, "argmax"), (d_feat, "d_feat")):
        if tuple(t.shape) != (n_docs, Ctot):
            raise RuntimeError(f"{name} must be [n_docs, C] = {(n_docs, Ctot)}, got {tuple(t.shape)}")
    if gate is not None:
        gate = gate.detach().contiguous()
        if gate.shape != ids.shape:
            raise RuntimeError(f"gate must be [n_docs, L] = {tuple(ids.shape)}, got {tuple(gate.shape)}")
    ptrs = (dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"), dev_ptr(gate, F32, "gate"), dev_ptr(table_c.detach(), F32, "word table"),
            ptr_array([w.detach() for w in ws], F32, "conv weight"), dev_ptr(feat, F32, "feat"), dev_ptr(argmax, I32, "argmax"),
            dev_ptr(d_feat, F32, "d_feat"))
    sal = torch.empty(n_docs, L, dtype=F32, device=table_c.device)
    _call("textcnn_saliency", _lib.lib().rbr_textcnn_saliency, C.byref(desc), *ptrs, dev_ptr(sal, F32, "sal"), current_stream())
    return sal


class DattSaliency(NamedTuple):
    """datt_saliency: fixed / through / d_gate_l [n_docs, L], d_gate_g [n_docs]; fixed + through is gradient x input."""
    fixed: torch.Tensor
    through: torch.Tensor
    d_gate_l: torch.Tensor
    d_gate_g: torch.Tensor


def datt_saliency(table: torch.Tensor, ids: torch.Tensor, gates, weights: Sequence[torch.Tensor], feat: torch.Tensor,
                  argmax: torch.Tensor, d_feat: torch.Tensor, attn_weights, *, gate_split: int = 1, pad_mode: int = PAD_VALID,
                  act: int = ACT_TANH) -> DattSaliency:
    """What every token position of a D-ATT tower contributes to a score whose gradient on the tower's pooled features is
    d_feat [n_docs, C], followed THROUGH both attention gates: fixed + through = <d score / d x[t], x[t]> for the embedded rows
    x, with only the max-pool routing (feat / argmax [n_docs, C] as textcnn(return_argmax=True) returned them) held fixed;
    rbr_datt_saliency in rbr_hip.h has the formula.
    gates = (gate_l, gate_g) [n_docs, L] each, the planes the forward used (datt_gate), or the stacked [2, n_docs, L];
    weights: the conv banks, the first gate_split of them under gate_l; attn_weights = (w_l [1, E, win], w_g [1, E, L]), the
    gates' Conv1d weights.  Two launches, no autograd, no embedded rows are materialised; a document's rows are bit-identical
    in every batch."""
    if not (isinstance(attn_weights, (tuple, list)) and len(attn_weights) == 2):
        raise RuntimeError("attn_weights must be (w_l [1, E, win], w_g [1, E, L])")
    table_c, ids, _, ws, desc = _conv_operands(table, ids, None, weights, pad_mode, act, None, _lib.conv_gate_split(gate_split))
    n_docs, L = ids.shape
    E = table_c.shape[1]
    Ctot = sum(int(w.shape[0]) for w in ws)
    for w in ws:
        if w.dim() != 3 or w.shape[1] != E:
            raise RuntimeError(f"conv weights must be [C_w, D = {E}, kz_w], got {tuple(w.shape)}")
    feat, argmax, d_feat = feat.detach().contiguous(), argmax.contiguous(), d_feat.detach().contiguous()
    for t, name in ((feat, "feat"), (argmax, "argmax"), (d_feat, "d_feat")):
        if tuple(t.shape) != (n_docs, Ctot):
            raise RuntimeError(f"{name} must be [n_docs, C] = {(n_docs, Ctot)}, got {tuple(t.shape)}")
    gate = torch.stack([gates[0], gates[1]]) if isinstance(gates, (tuple, list)) else gates
    gate = gate.detach().contiguous()
    if tuple(gate.shape) != (2, n_docs, L):
        raise RuntimeError(f"gates must be two planes [n_docs, L] = {(n_docs, L)} each, got {tuple(gate.shape)}")
    w_l, w_g = (w.detach().contiguous() for w in attn_weights)
    if w_l.dim() != 3 or w_l.shape[0] != 1 or w_l.shape[1] != E:
        raise RuntimeError(f"the local gate's weight must be [1, E = {E}, win], got {tuple(w_l.shape)}")
    if tuple(w_g.shape) != (1, E, L):
        raise RuntimeError(f"the global gate's weight must be [1, E, L] = {(1, E, L)}, got {tuple(w_g.shape)}")
    ptrs = (dev_ptr(ids, I64, "ids"), dev_ptr(gate, F32, "gates"), dev_ptr(table_c.detach(), F32, "word table"),
            ptr_array([w.detach() for w in ws], F32, "conv weight"), dev_ptr(feat, F32, "feat"), dev_ptr(argmax, I32, "argmax"),
            dev_ptr(d_feat, F32, "d_feat"), int(w_l.shape[2]), dev_ptr(w_l, F32, "local gate weight"),
            dev_ptr(w_g, F32, "global gate weight"))
    dev = table_c.device
    fixed, through, d_gate_l = (torch.empty(n_docs, L, dtype=F32, device=dev) for _ in range(3))
    d_gate_g = torch.empty(n_docs, dtype=F32, device=dev)
    _call("datt_saliency", _lib.lib().rbr_datt_saliency, C.byref(desc), *ptrs, dev_ptr(fixed, F32, "fixed"),
          dev_ptr(through, F32, "through"), dev_ptr(d_gate_l, F32, "d_gate_l"), dev_ptr(d_gate_g, F32, "d_gate_g"), current_stream())
    return DattSaliency(fixed, through, d_gate_l, d_gate_g)


_HEAD_NAMES =("Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib")
_HEAD_ACC = ("Eu", "Ei", "ub", "ib")       # gradients accumulated with atomics (rows addressed by id)


class _PairHead(torch.autograd.Function):
    """pred[B] = FM(LastFeat_u(u_feat, u_id), LastFeat_i(i_feat, i_id))  -- rbr_pair_head_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, u_feat, i_feat, u_id, i_id, drop, pad_u, pad_i, Wu, bu, Eu, Wi, bi, Ei, h, g, ub, ib):
        # i_feat None: u_feat is the [2B,H] output of the shared encoder, user rows first -- one tensor in, one gradient
        # tensor out (slicing it outside costs autograd two zero fills, two copies and an add per step)
        ctx.stacked = i_feat is None
        if ctx.stacked:
            pair = u_feat.contiguous()
            if pair.shape[0] % 2:
                raise RuntimeError(f"stacked pair features need an even row count, got {tuple(pair.shape)}")
            u_feat, i_feat = pair[:pair.shape[0] // 2], pair[pair.shape[0] // 2:]
        B, H = u_feat.shape
        K = Wu.shape[1]
        dev = u_feat.device
        L_ = _lib.lib()
        u_feat, i_feat = u_feat.contiguous(), i_feat.contiguous()
        u_id, i_id = u_id.contiguous(), i_id.contiguous()
        params = [t.contiguous() for t in (Wu, bu, Eu, Wi, bi, Ei, h, g, ub, ib)]
        hp = _lib.HeadParams(*[dev_ptr(t, F32, n) for t, n in zip(params, ("Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib"))])
        ul = torch.empty(B, K, dtype=F32, device=dev)
        il = torch.empty(B, K, dtype=F32, device=dev)
        pred = torch.empty(B, dtype=F32, device=dev)
        ctx.flat = None
        if isinstance(drop, float):
            # training forward in one launch: the kernel draws the dropout multiplier itself (same stream of draws as
            # dropout_multiplier) and its spare workgroups clear the buffer the backward accumulates the embedding-style
            # gradients into
            p_drop = drop
            if p_drop >= 1.0:
                raise RuntimeError("pair_head: drop probability must be < 1 on the fused path")
            acc_n = sum(t.numel() for t, n in zip(params, _HEAD_NAMES) if n in _HEAD_ACC) if any(ctx.needs_input_grad[7:]) else 0
            flat = torch.empty(acc_n, dtype=F32, device=dev) if acc_n else None
            seed, state = _drop_rng(dev)
            drop = torch.empty(B, K, dtype=F32, device=dev) if p_drop > 0.0 else None
            _call(None, L_.rbr_pair_head_fwd_train, B, H, K, dev_ptr(u_feat, F32, "u_feat"), dev_ptr(i_feat, F32, "i_feat"),
                  dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), float(p_drop), seed, state.data_ptr(),
                  dev_ptr(drop, F32, "drop"), dev_ptr(flat, F32, "zero_buf"), acc_n, dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"),
                  dev_ptr(pred, F32, "pred"), current_stream())
            ctx.flat = flat
        else:
            if drop is not None:
                drop = drop.contiguous()
            _call(None, L_.rbr_pair_head_fwd, B, H, K, dev_ptr(u_feat, F32, "u_feat"), dev_ptr(i_feat, F32, "i_feat"),
                  dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), dev_ptr(drop, F32, "drop"),
                  dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(pred, F32, "pred"), current_stream())
        ctx.dims = (B, H, K, int(pad_u), int(pad_i))
        ctx.has_drop = drop is not None
        ctx.save_for_backward(u_feat, i_feat, u_id, i_id, ul, il, *params, *([drop] if drop is not None else []))
        return pred

    @staticmethod
    def backward(ctx, d_pred):
        B, H, K, pad_u, pad_i = ctx.dims
        saved = list(ctx.saved_tensors)
        u_feat, i_feat, u_id, i_id, ul, il = saved[:6]
        params = saved[6:16]
        drop = saved[16] if ctx.has_drop else None
        dev = u_feat.device
        L_ = _lib.lib()
        names = ("Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib")
        hp = _lib.HeadParams(*[dev_ptr(t, F32, n) for t, n in zip(params, names)])
        # embedding-style grads are accumulated with atomics -> start from zero (one fill for the four of them);
        # the rest is overwritten
        acc = [t for t, n in zip(params, names) if n in _HEAD_ACC]
        flat, ctx.flat = ctx.flat, None         # cleared by the training forward; a second backward gets a fresh one
        if flat is None:
            flat = torch.zeros(sum(t.numel() for t in acc), dtype=F32, device=dev)
        zeroed = iter(v.view_as(t) for v, t in zip(flat.split([t.numel() for t in acc]), acc))
        grads = [next(zeroed) if n in ("Eu", "Ei", "ub", "ib") else torch.empty_like(t) for t, n in zip(params, names)]
        hg = _lib.HeadGrads(*[dev_ptr(t, F32, "d" + n) for t, n in zip(grads, names)])
        d_pair = torch.empty(2 * B, H, dtype=F32, device=dev)
        d_uf, d_if = d_pair[:B], d_pair[B:]
        wsn = L_.rbr_pair_head_bwd_ws_floats(B, K)
        ws = torch.empty(wsn, dtype=F32, device=dev) if wsn else None
        d_pred = d_pred.contiguous()
        _call(None, L_.rbr_pair_head_bwd, B, H, K, dev_ptr(u_feat, F32, "u_feat"), dev_ptr(i_feat, F32, "i_feat"),
              dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), dev_ptr(drop, F32, "drop"),
              dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(d_pred, F32, "d_pred"), pad_u, pad_i, C.byref(hg),
              dev_ptr(d_uf, F32, "d_ufeat"), dev_ptr(d_if, F32, "d_ifeat"), dev_ptr(ws, F32, "ws"), current_stream())
        if ctx.stacked:
            return (d_pair, None, None, None, None, None, None, *grads)
        return (d_uf, d_if, None, None, None, None, None, *grads)


def pair_head(u_feat, i_feat, u_id, i_id, Wu, bu, Eu, Wi, bi, Ei, h, g, ub, ib, *, drop=None, pad_u=0, pad_i=0):
    """LastFeat x2 + FM.  u_feat/i_feat [B,H] (or u_feat [2B,H] = user rows then item rows, i_feat None);
    ids [B] int64; returns pred [B].  drop: None, a [B,K] multiplier tensor, or a float = dropout probability of a
    TRAINING forward (the kernel draws the multiplier itself: one launch less than dropout_multiplier + pair_head)."""
    return _PairHead.apply(u_feat, i_feat, u_id, i_id, drop, pad_u, pad_i, Wu, bu, Eu, Wi, bi, Ei, h, g, ub, ib)


# --------------------------------------------------------------------------- encoder + head of a two-tower model, fused
class _LossRequest:
    """fused_loss(target): the trainer's nn.MSELoss target, announced to the model's forward so that a fused head launch can
    compute the loss as well; loss_for(pred) hands it out (None: the forward did not take the offer).  after_backward: the
    caller reads the loss VALUE only after loss.backward() has run (train_step does) -- the forward may then leave computing it to
    the backward (_EncodeHead: RBR_LOSS_IN_BWD)."""

    def __init__(self, target, after_backward: bool = False):
        self.target, self.pred_ptr, self.loss, self.after_backward = target, None, None, bool(after_backward)

    def loss_for(self, pred: torch.Tensor):
        if self.loss is not None and self.pred_ptr == pred.data_ptr() and pred.numel() == self.target.numel():
            return self.loss
        return None


_LOSS_REQUEST: list = []


@contextlib.contextmanager
def fused_loss(target: torch.Tensor, after_backward: bool = False):
    """with fused_loss(ratings) as fl: pred = model(*batch); loss = fl.loss_for(pred) -- the mean-squared error against
    `target` (trainer/train_deepconn_pp.py:164) out of the model's last launch when the model supports it (DeepCoNN's fused
    encoder + head), else None and the caller computes mse_loss(pred, target) itself.  after_backward=True: a promise that the
    loss tensor is not READ before loss.backward() has been issued; DeepCoNN's fused head then writes it from its backward launch,
    off the step's serial chain, and until then the tensor holds no value."""
    req = _LossRequest(target, after_backward)
    _LOSS_REQUEST.append(req)
    try:
        yield req
    finally:
        _LOSS_REQUEST.remove(req)


_TICKETS: dict = {}


def _ticket(dev) -> torch.Tensor:
    """Arrival counter of rbr_pair_head_fwd_pool's MSE reduction (the last pair block to arrive sums the loss and puts the counter
    back to 0): one per (device, STREAM) -- launches on one stream are ordered, so they may share it; two fused heads in flight
    on different streams (a side-stream eval beside a training step, a graph replay beside an eager step) must not."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(4, dtype=I32, device=dev)
    return t


def prepare_stream_state(dev) -> None:
    """Creates the per-(device, stream) state of the CURRENT stream -- the arrival counter of the fused head's MSE reduction, and
    the all-pairs softmax loss's workspace at the largest size any stream of the device has needed so far (the warm-up steps
    ahead of a recording ran on another stream: they are what sizes it) -- so that its first use does not allocate it.  train_step.GraphedTrainStep /
    GraphedForward call it on their capture stream before recording: a counter buffer created during a capture would live in
    that graph's private memory pool and cost every replay a fill node."""
    dev = torch.device(dev)
    _ticket(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    need = max((t.numel() for (d, _), t in _PS_WS.items() if d == idx), default=0)
    if need:
        _pair_softmax_ws(dev, need)
    _kept_ws_prepare_stream(dev, idx)


def encode_head_applicable(table, n_docs, L, kernel_sizes, channels, padding_idx) -> bool:
    """True when the fused encoder + head function serves this conv: the token-product formulation applies and one
    pool-epilogue launch covers every channel slot."""
    if not table.is_cuda or table.dtype != F32 or n_docs % 2 or os.environ.get("RBR_FUSED_STEP", "1") == "0":
        return False
    ntiles, wpd = (sum(channels) + 31) // 32, (L + 31) // 32
    if ntiles > 8 or (2 * sum(channels) + 2 * wpd * ntiles * 32 + 2 * wpd) * 4 > 60 * 1024:      # rbr_pair_head_fwd_pool's limits
        return False
    desc = _lib.make_desc(n_docs, L, table.shape[1], table.shape[0], kernel_sizes, channels, PAD_SAME, ACT_RELU, padding_idx)
    return _lib.lib().rbr_textcnn_fwd_ws_bytes(C.byref(desc)) > 0


class _EncodeHead(torch.autograd.Function):
    """pred[B] (and the MSE loss against `target`) = rating head(TextCNN(user docs), TextCNN(item docs), ids): the training /
    eval forward of DeepCoNN++ (deepconn.py:43-53) as 6 launches -- id check + list state | token marks + slab scan | token list
    + weight images | distinct-token GEMM | gather + max-pool (+ clearing the backward's G) | pool epilogue + LastFeat x2 + FM
    (+ MSELoss) -- and its backward as head_bwd, then [zero G, G build, G @ Wprod^T] beside [dW] (see _textcnn_backward).
    With the fused loss the head launch also writes d loss / d feat for a unit root gradient (rbr_pair_head_fwd_pool_ex); a
    backward that is handed exactly that gradient starts the conv backward at once and runs what is left of head_bwd (id-row
    atomics, batch reductions) behind dW on the weight-gradient branch.  RBR_HEAD_BWD_IN_FWD=0 restores the old order."""

    @staticmethod
    def forward(ctx, table, id_sets, ids, mask, u_id, i_id, drop, target, padding_idx, pad_u, pad_i, n_widths, first, opts,
                *params):
        defer_loss, own_ws = opts
        bs_ = [b.contiguous() for b in params[n_widths:2 * n_widths]]
        head = [t.contiguous() for t in params[2 * n_widths:]]
        L_ = _lib.lib()
        dev = table.device
        st = current_stream()
        # ---- clean id tensors: token ids of both towers first (the conv's [2B, L] batch), then the rest
        sets = None
        if id_sets is not None:
            tens = [t.contiguous() for t, _, _ in id_sets]
            flat = torch.empty(sum(t.numel() for t in tens), dtype=I64, device=dev)
            arr = (_lib.IdSet * len(tens))()
            outs, o = [], 0
            for k, (t, (_, rows, rep)) in enumerate(zip(tens, id_sets)):
                dev_ptr(t, I64, "ids")
                v = flat[o:o + t.numel()].view(t.shape)
                outs.append(v)
                o += t.numel()
                arr[k] = _lib.IdSet(t.data_ptr(), v.data_ptr(), t.numel(), int(rows), 0 if rep is None or rep < 0 else int(rep))
            n_tok = tens[0].numel() + tens[1].numel()
            ids = flat[:n_tok].view(2 * tens[0].shape[0], tens[0].shape[1])
            u_id, i_id = outs[2], outs[3]
            sets = (len(tens), arr, _id_err(dev).data_ptr())
        else:
            u_id, i_id = u_id.contiguous(), i_id.contiguous()
        table_c, ids, mask8, ws_, desc = _conv_operands(table, ids, mask, params[:n_widths], PAD_SAME, ACT_RELU, padding_idx)
        B = ids.shape[0] // 2
        conv = _conv_fwd_buffers(_ConvSaved(), desc, dev, kept=own_ws and sets is not None)
        if conv.prod_ws is None:
            check(-1, "encode_head plan (encode_head_applicable() was not consulted)")
        pval, pidx, feat, argmax = conv.pval, conv.pidx, conv.feat, conv.argmax
        training = any(ctx.needs_input_grad)          # (grad mode itself is off inside forward)
        _prod_forward(desc, conv, table_c, ids, mask8, None, ws_, st, id_sets=sets)
        # ---- pool epilogue + rating head (+ loss)
        K = head[0].shape[1]
        hp = _lib.HeadParams(*[dev_ptr(t, F32, n) for t, n in zip(head, _HEAD_NAMES)])
        ul = torch.empty(B, K, dtype=F32, device=dev)
        il = torch.empty(B, K, dtype=F32, device=dev)
        pred = torch.empty(B, dtype=F32, device=dev)
        p_drop, drop_t, flat_zero, acc_n = 0.0, None, None, 0
        seed, state = 0, None
        if isinstance(drop, float):
            if drop >= 1.0:
                raise RuntimeError("pair_head: drop probability must be < 1 on the fused path")
            p_drop = drop
            acc_n = sum(t.numel() for t, n in zip(head, _HEAD_NAMES) if n in _HEAD_ACC) if training else 0
            flat_zero = torch.empty(acc_n, dtype=F32, device=dev) if acc_n else None
            if p_drop > 0.0:
                seed, state = _drop_rng(dev)
                drop_t = torch.empty(B, K, dtype=F32, device=dev)
        elif drop is not None:
            drop_t = drop.contiguous()
        loss = d_unit = d_feat_unit = None
        if target is not None:
            target = target.contiguous()
            loss = torch.empty((), dtype=F32, device=dev)
            d_unit = torch.empty(B, dtype=F32, device=dev)
            if training and first is None and os.environ.get("RBR_HEAD_BWD_IN_FWD", "1") != "0" \
                    and L_.rbr_pair_head_fwd_pool_lds_bytes(C.byref(desc), K, 1):
                d_feat_unit = torch.empty(2 * B, feat.shape[1], dtype=F32, device=dev)
        # The loss off the serial chain: with d_feat_unit nothing in the step reads the loss, so a caller that promised to read it
        # only after the backward (fused_loss(after_backward=True)) gets a head launch without the MSE ticket, its two agent-scope
        # fences and the last-block pass; rbr_pair_head_bwd_ex writes loss and d_unit from one more workgroup on the
        # weight-gradient branch.  RBR_LOSS_IN_BWD=0 keeps the ticketed tail.  Measured at cfg2: the head
        # launch 28.6 -> 22.3 us; with the switch off the step is 0.3454 / 0.3416 ms against 0.3374 - 0.3425 with it on.
        ctx.deferred = None
        if d_feat_unit is not None and defer_loss and os.environ.get("RBR_LOSS_IN_BWD", "1") != "0":
            ctx.deferred = (pred.detach(), target, loss.detach())
        ticketed = target is not None and ctx.deferred is None
        _call("pair_head_fwd_pool", L_.rbr_pair_head_fwd_pool_ex, C.byref(desc), dev_ptr(pval, F32, "pval"), dev_ptr(pidx, I32, "pidx"),
              ptr_array(bs_, F32, "conv bias"), dev_ptr(feat, F32, "feat"), dev_ptr(argmax, I32, "argmax"),
              dev_ptr(first, I64, "first"), K, dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp),
              dev_ptr(drop_t, F32, "drop") if p_drop == 0.0 else None, float(p_drop), seed,
              state.data_ptr() if state is not None else None,
              dev_ptr(drop_t, F32, "drop") if p_drop > 0.0 else None, dev_ptr(flat_zero, F32, "zero_buf"),
              acc_n, dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(pred, F32, "pred"),
              dev_ptr(target, F32, "target"), dev_ptr(loss, F32, "loss"), dev_ptr(d_unit, F32, "d_unit"),
              _ticket(dev).data_ptr() if ticketed else None, dev_ptr(d_feat_unit, F32, "d_feat_unit"), st)
        ctx.d_feat_unit = d_feat_unit
        ctx.conv = _ConvSaved(table=table_c, ids=ids, packed=None, feat=feat, argmax=argmax, mask8=mask8, gate=None, ws=ws_,
                              desc=desc, prod_ws=conv.prod_ws, fanout_acc=None)
        ctx.head = (u_id, i_id, ul, il, head, drop_t, flat_zero, d_unit)
        ctx.first = first
        ctx.dims = (B, feat.shape[1], K, int(pad_u), int(pad_i), n_widths)
        ctx.set_materialize_grads(False)
        if loss is None:
            loss = torch.empty((), dtype=F32, device=dev)      # no target: an unwritten placeholder nobody reads
            ctx.mark_non_differentiable(loss)
        return pred, loss

    @staticmethod
    def backward(ctx, d_pred, d_loss):
        B, H, K, pad_u, pad_i, n_widths = ctx.dims
        u_id, i_id, ul, il, head, drop_t, flat, d_unit = ctx.head
        S = ctx.conv
        dev = S.table.device
        L_ = _lib.lib()
        need_conv = any(ctx.needs_input_grad[14:14 + 2 * n_widths]) or ctx.needs_input_grad[0]
        unit = _UNIT.get(dev)
        # the forward launch wrote d_feat for exactly this upstream gradient: the conv backward does not wait for head_bwd
        early = (ctx.d_feat_unit is not None and need_conv and d_pred is None and ctx.first is None and d_loss is not None
                 and unit is not None and d_loss.data_ptr() == unit.data_ptr())
        deferred = ctx.deferred
        if deferred is not None and not early:
            # any other upstream gradient: the loss and d loss / d pred the forward launch left out, by the launch of their own
            # (rbr_mse_loss_fwd: the same bits), then the old order
            _call(None, L_.rbr_mse_loss_fwd, B, dev_ptr(deferred[0], F32, "pred"), dev_ptr(deferred[1], F32, "target"),
                  dev_ptr(deferred[2], F32, "loss"), dev_ptr(d_unit, F32, "d_pred_unit"), current_stream())
            deferred = None
        if d_loss is not None:                  # the fused loss: d loss / d pred was written by the forward launch
            g = d_unit if (unit is not None and d_loss.data_ptr() == unit.data_ptr()) else d_unit * d_loss
            d_pred = g if d_pred is None else d_pred + g
        if d_pred is None:
            d_pred = torch.zeros(B, dtype=F32, device=dev)
        d_pred = d_pred.contiguous()
        hp = _lib.HeadParams(*[dev_ptr(t, F32, n) for t, n in zip(head, _HEAD_NAMES)])
        accs = [t for t, n in zip(head, _HEAD_NAMES) if n in _HEAD_ACC]
        if flat is None:
            flat = torch.zeros(sum(t.numel() for t in accs), dtype=F32, device=dev)
        ctx.head = (u_id, i_id, ul, il, head, drop_t, None, d_unit)      # a second backward gets a fresh accumulation buffer
        zeroed = iter(v.view_as(t) for v, t in zip(flat.split([t.numel() for t in accs]), accs))
        grads = [next(zeroed) if n in _HEAD_ACC else torch.empty_like(t) for t, n in zip(head, _HEAD_NAMES)]
        hg = _lib.HeadGrads(*[dev_ptr(t, F32, "d" + n) for t, n in zip(grads, _HEAD_NAMES)])
        d_pair = ctx.d_feat_unit if early else torch.empty(2 * B, H, dtype=F32, device=dev)
        feat = S.feat

        def head_bwd():          # early: the pair blocks only accumulate the id-row gradients
            if deferred is not None:      # ... and one more workgroup writes the loss and d_unit (d_pred is taken from pred / target)
                _call(None, L_.rbr_pair_head_bwd_ex, B, H, K, dev_ptr(feat[:B], F32, "u_feat"), dev_ptr(feat[B:], F32, "i_feat"),
                      dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), dev_ptr(drop_t, F32, "drop"),
                      dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), None, pad_u, pad_i, C.byref(hg), None, None,
                      dev_ptr(deferred[0], F32, "pred"), dev_ptr(deferred[1], F32, "target"), dev_ptr(deferred[2], F32, "loss"),
                      dev_ptr(d_unit, F32, "d_pred_unit"), current_stream())
                return
            _call(None, L_.rbr_pair_head_bwd, B, H, K, dev_ptr(feat[:B], F32, "u_feat"), dev_ptr(feat[B:], F32, "i_feat"),
                  dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), dev_ptr(drop_t, F32, "drop"),
                  dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(d_pred, F32, "d_pred"), pad_u, pad_i, C.byref(hg),
                  None if early else dev_ptr(d_pair[:B], F32, "d_ufeat"), None if early else dev_ptr(d_pair[B:], F32, "d_ifeat"),
                  None, current_stream())

        if early:
            dtable, _, dWs, dbs = _textcnn_backward(S, d_pair, ctx.needs_input_grad[0], False, side_job=head_bwd)
            return (dtable, None, None, None, None, None, None, None, None, None, None, None, None, None, *dWs, *dbs, *grads)
        head_bwd()
        if need_conv and ctx.first is not None:      # in-batch dedup: the repeated documents' gradient rows onto their first occurrence
            _call(None, L_.rbr_dedup_fold_rows, 2 * B, H, dev_ptr(ctx.first, I64, "first"), dev_ptr(d_pair, F32, "d_feat"),
                  current_stream())
        if need_conv:
            dtable, _, dWs, dbs = _textcnn_backward(S, d_pair, ctx.needs_input_grad[0], False)
        else:
            dtable, dWs, dbs = None, [None] * n_widths, [None] * n_widths
        return (dtable, None, None, None, None, None, None, None, None, None, None, None, None, None, *dWs, *dbs, *grads)


def encode_head(table, ids, mask, u_id, i_id, conv_weights, conv_biases, head_params, *, id_sets=None, drop=None,
                padding_idx=0, pad_u=0, pad_i=0, first=None, own_workspace=False):
    """DeepCoNN++'s forward from token ids to predictions in one autograd function (see _EncodeHead).  ids / mask: the stacked
    [2B, L] towers (user rows first) -- or id_sets = [(u_docs, V, pad), (i_docs, V, pad), (u_ids, U, 0), (i_ids, I, 0)], the raw
    id tensors, whose range check then rides in the prepare stage's first launch (ids / u_id / i_id are ignored).
    head_params: (Wu, bu, Eu, Wi, bi, Ei, h, g, ub, ib).  drop: None, a [B, K] multiplier, or the dropout probability of a
    training forward.  first [2B] (dedup_rows; `mask` then carries the blanked rows): document r's features are document
    first[r]'s -- the in-batch dedup by id, inside the fused step.  Inside `with fused_loss(target)` the MSE against target is computed by the head launch as well.
    own_workspace (with id_sets): the conv's forward workspace comes from the kept workspaces (_kept_ws_checkout) and the prepare
    stage runs in two launches instead of three."""
    req = _LOSS_REQUEST[-1] if _LOSS_REQUEST else None
    target = None
    if req is not None and req.loss is None and req.target.is_cuda and req.target.dtype == F32 and req.target.dim() == 1 \
            and torch.is_grad_enabled():
        B = (id_sets[0][0].shape[0] if id_sets is not None else ids.shape[0] // 2)
        if req.target.shape[0] == B:
            target = req.target
    pred, loss = _EncodeHead.apply(table, id_sets, ids, mask, u_id, i_id, drop, target, padding_idx, pad_u, pad_i,
                                   len(conv_weights), first, (target is not None and req.after_backward, bool(own_workspace)),
                                   *conv_weights, *conv_biases, *head_params)
    if target is not None:
        req.pred_ptr, req.loss = pred.data_ptr(), loss
    return pred


def stack_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], 0) of two input tensors; no copy when b already follows a in the same allocation (the
    static batch buffers of train_step.GraphedTrainStep, or a loader that delivers both towers in one block)."""
    if (a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a.is_contiguous() and b.is_contiguous()
            and not a.requires_grad and not b.requires_grad and a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel()):
        return a.as_strided((a.shape[0] + b.shape[0], *a.shape[1:]), a.stride(), a.storage_offset())
    return torch.cat([a, b], dim=0)


def clone_adjacent(tensors):
    """Clones of `tensors`; neighbours (2k, 2k+1) of equal shape and dtype share one allocation, first then second,
    so stack_rows() on the clones is a view."""
    out = list(tensors)
    k = 0
    while k < len(out):
        a = out[k]
        b = out[k + 1] if k + 1 < len(out) else None
        if b is not None and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and a.dim() >= 1:
            both = torch.empty((2 * a.shape[0], *a.shape[1:]), dtype=a.dtype, device=a.device)
            both[:a.shape[0]].copy_(a)
            both[a.shape[0]:].copy_(b)
            out[k], out[k + 1] = both[:a.shape[0]], both[a.shape[0]:]
            k += 2
        else:
            out[k] = a.clone()
            k += 1
    return tuple(out)


def dropout_multiplier(shape, p: float, training: bool, device, lane: int = 0) -> Optional[torch.Tensor]:
    """The multiplier F.dropout would apply (0 or 1/(1-p)): rbr_dropout_multiplier, keyed by the device generator's seed
    (torch.manual_seed) and a per-device call counter that lives on the device."""
    if not training or p <= 0.0:
        return None
    if p >= 1.0:
        return torch.zeros(shape, dtype=F32, device=device)
    # own Philox kernel with the call counter in device memory: one launch, and -- unlike a torch RNG op -- nothing for the
    # host to patch before every replay of a captured step (the generator's seed / offset fills)
    dev = torch.device(device)
    seed, state = _drop_rng(dev, lane)
    out = torch.empty(shape, dtype=F32, device=dev)
    _call(None, _lib.lib().rbr_dropout_multiplier, out.numel(), float(p), seed, state.data_ptr(), dev_ptr(out, F32, "out"),
          current_stream())
    return out


def _drop_rng(dev, lane: int = 0):
    """(seed, device state) of the dropout draws on `dev`: the device generator's seed (torch.manual_seed) and the
    [call number, ticket] pair that lives on the device.  `lane` selects an independent stream of draws: launches that may
    run concurrently (the second tower on its own HIP stream, second_tower()) must not share a call counter."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError(f"dropout: device must be a HIP device (got {dev}); there is no CPU path")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    state = _DROP_STATE.get((idx, lane))
    if state is None:
        state = _DROP_STATE[(idx, lane)] = torch.zeros(2, dtype=torch.int64, device=dev)
    seed = (torch.cuda.default_generators[idx].initial_seed() + 0x9E3779B97F4A7C15 * lane) & 0xFFFFFFFFFFFFFFFF
    return seed, state


_DROP_STATE: dict = {}       # per device: [call number, workgroup ticket] (uint64 x 2), advanced on the device



class _MseLoss(torch.autograd.Function):
    """mean((pred - target)^2) -- the trainers' nn.MSELoss (train_deepconn_pp.py:137,164).  The forward launch also writes
    d loss / d pred for an upstream gradient of 1; a backward that is handed unit_scalar() (train_step does that) returns it
    without a launch, any other upstream gradient costs one launch."""

    @staticmethod
    def forward(ctx, pred, target):
        pred, target = pred.contiguous(), target.contiguous()
        if pred.shape != target.shape:
            raise RuntimeError(f"mse_loss: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
        loss = torch.empty((), dtype=F32, device=pred.device)
        d_unit = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        _call(None, _lib.lib().rbr_mse_loss_fwd, pred.numel(), dev_ptr(pred, F32, "pred"), dev_ptr(target, F32, "target"),
              dev_ptr(loss, F32, "loss"), dev_ptr(d_unit, F32, "d_pred_unit"), current_stream())
        ctx.save_for_backward(pred, target, *([d_unit] if d_unit is not None else []))
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        pred, target = ctx.saved_tensors[:2]
        unit = _UNIT.get(pred.device)
        if unit is not None and len(ctx.saved_tensors) == 3 and d_loss.data_ptr() == unit.data_ptr():
            return ctx.saved_tensors[2], None
        d_pred = torch.empty_like(pred)
        d_loss = d_loss.contiguous()
        _call(None, _lib.lib().rbr_mse_loss_bwd, pred.numel(), dev_ptr(pred, F32, "pred"), dev_ptr(target, F32, "target"),
              dev_ptr(d_loss, F32, "d_loss"), dev_ptr(d_pred, F32, "d_pred"), current_stream())
        return d_pred, None


_UNIT: dict = {}


def unit_scalar(device) -> torch.Tensor:
    """The constant 1.0 on `device` (one tensor per device, never written): pass it to loss.backward() as the root gradient
    to spare the per-step fill, and mse_loss's backward recognises it."""
    device = torch.device(device)
    t = _UNIT.get(device)
    if t is None:
        t = _UNIT[device] = torch.ones((), dtype=F32, device=device)
    return t


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """F.mse_loss(pred, target) (mean reduction) for f32 device tensors of equal shape."""
    return _MseLoss.apply(pred, target)


class _BprLoss(torch.autograd.Function):
    """The pairwise ranking loss over sampled negatives (rbr_bpr_loss_* in rbr_hip.h).  As _MseLoss: the forward launch also
    writes d loss / d pred for an upstream gradient of 1, and a backward that is handed unit_scalar() returns it without a launch."""

    @staticmethod
    def forward(ctx, pred, n_neg, valid):
        pred = pred.contiguous()
        n_neg = int(n_neg)
        if pred.dim() != 1 or n_neg < 1 or pred.shape[0] == 0 or pred.shape[0] % (1 + n_neg):
            raise RuntimeError(f"bpr_loss: pred must be [(1 + n_neg) * B] with n_neg >= 1, got {tuple(pred.shape)} for n_neg={n_neg}")
        B = pred.shape[0] // (1 + n_neg)
        if valid is not None:
            valid = valid.contiguous()
            if valid.shape != (n_neg * B,):
                raise RuntimeError(f"bpr_loss: valid must be [{n_neg * B}], got {tuple(valid.shape)}")
        loss = torch.empty((), dtype=F32, device=pred.device)
        d_unit = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        _call(None, _lib.lib().rbr_bpr_loss_fwd, B, n_neg, dev_ptr(pred, F32, "pred"), dev_ptr(valid, F32, "valid"),
              dev_ptr(loss, F32, "loss"), dev_ptr(d_unit, F32, "d_pred_unit"), current_stream())
        ctx.B, ctx.n_neg, ctx.has_valid = B, n_neg, valid is not None
        ctx.save_for_backward(pred, *([valid] if valid is not None else []), *([d_unit] if d_unit is not None else []))
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        saved = ctx.saved_tensors
        pred = saved[0]
        valid = saved[1] if ctx.has_valid else None
        d_unit = saved[-1] if len(saved) == 2 + int(ctx.has_valid) else None
        unit = _UNIT.get(pred.device)
        if unit is not None and d_unit is not None and d_loss.data_ptr() == unit.data_ptr():
            return d_unit, None, None
        d_pred = torch.empty_like(pred)
        d_loss = d_loss.contiguous()
        _call(None, _lib.lib().rbr_bpr_loss_bwd, ctx.B, ctx.n_neg, dev_ptr(pred, F32, "pred"), dev_ptr(valid, F32, "valid"),
              dev_ptr(d_loss, F32, "d_loss"), dev_ptr(d_pred, F32, "d_pred"), current_stream())
        return d_pred, None, None


def bpr_loss(pred: torch.Tensor, n_neg: int, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The BPR loss of pred f32 [(1 + n_neg) * B] in sample_negatives' layout (rows [0, B) score the observed pairs, rows
    [(j+1)B, (j+2)B) their j-th negatives): mean over the valid negatives of softplus(pred_neg - pred_pos) =
    -log sigmoid(pred_pos - pred_neg).  valid f32 [n_neg * B] (1 / 0, sample_negatives' third output; None = all ones) takes a
    negative out of the sum and the mean; no valid negative at all gives loss 0 and zero gradients.  Fixed summation order:
    the same bits on every run."""
    return _BprLoss.apply(pred, n_neg, valid)


_PS_WS: dict = {}


def _pair_softmax_ws(dev, nbytes: int) -> torch.Tensor:
    """Workspace of rbr_pair_softmax_* (ds [B, B], the row losses, the d_h partials): one per (device, STREAM), as _ticket --
    launches on one stream are ordered and may share it; it only grows.  prepare_stream_state() creates it ahead of a capture."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    t = _PS_WS.get(key)
    if t is None or t.numel() < nbytes:
        t = _PS_WS[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    return t


class _PairSoftmaxLoss(torch.autograd.Function):
    """The in-batch softmax loss over all B x B pairs (rbr_pair_softmax_* in rbr_hip.h) -> (loss, pos).  As _MseLoss: the forward's
    two launches also write the gradients for an upstream gradient of 1, and a backward that is handed unit_scalar() returns them
    without a launch; any other root re-runs the two launches with that scalar (and the forward's dropout call number)."""

    @staticmethod
    def forward(ctx, ul, il, h, row_bias, col_bias, u_ids, i_ids, mode, drop, p_drop, seen_csr, item_lo, logq, inv_temp):
        code = SCORE_MODES[mode]
        ul, il = ul.contiguous(), il.contiguous()
        dev = ul.device
        B, K = ul.shape
        ctx.shapes = tuple(None if t is None else t.shape for t in (h, row_bias, col_bias))
        flat = [None if t is None else t.contiguous().view(-1) for t in (h, row_bias, col_bias, logq)]
        for t, n, name in zip(flat, (K, B, B, B), ("h", "row_bias", "col_bias", "logq")):
            if t is not None and t.numel() != n:
                raise RuntimeError(f"pair_softmax_loss: {name} must hold {n} values, got {t.numel()}")
        h, row_bias, col_bias, logq = flat
        u_ids, i_ids = u_ids.contiguous(), i_ids.contiguous()
        if drop is not None:
            drop = drop.contiguous()
            if drop.shape != (B, B, K):
                raise RuntimeError(f"pair_softmax_loss: drop must be [{B}, {B}, {K}], got {tuple(drop.shape)}")
        off, items, nnz, U = seen_csr
        L_ = _lib.lib()
        # a shape the entry refuses has a workspace of 0 bytes: the call below then returns its error code and text before any launch
        ws = _pair_softmax_ws(dev, L_.rbr_pair_softmax_ws_bytes(B, K))
        p_drop = float(p_drop)
        seed, state = _drop_rng(dev) if p_drop > 0.0 else (0, None)
        call = torch.empty(1, dtype=I64, device=dev) if p_drop > 0.0 else None
        loss = torch.empty((), dtype=F32, device=dev)
        pos = torch.empty(B, dtype=F32, device=dev)
        grads = any(ctx.needs_input_grad[:5])
        d_ul = torch.empty_like(ul) if grads else None
        d_il = torch.empty_like(il) if grads else None
        d_h = torch.empty_like(h) if grads and h is not None and code == _lib.SCORE_FM else None
        d_cb = torch.empty_like(col_bias) if grads and col_bias is not None else None
        d_rb = torch.empty_like(row_bias) if grads and row_bias is not None else None
        ctx.ops = (code, B, K, dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(h, F32, "h"), dev_ptr(row_bias, F32, "row_bias"),
                   dev_ptr(col_bias, F32, "col_bias"), dev_ptr(drop, F32, "drop"), p_drop, seed)
        ctx.ids = (dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"), dev_ptr(off, I64, "seen offsets"),
                   dev_ptr(items, I32, "seen items"), nnz, U, int(item_lo), dev_ptr(logq, F32, "logq"), float(inv_temp))
        _call("pair_softmax_fwd", L_.rbr_pair_softmax_fwd, *ctx.ops, None if state is None else state.data_ptr(), *ctx.ids,
              dev_ptr(loss, F32, "loss"), dev_ptr(pos, F32, "pos"), dev_ptr(d_ul, F32, "d_ul"), dev_ptr(d_il, F32, "d_il"),
              dev_ptr(d_h, F32, "d_h"), dev_ptr(d_cb, F32, "d_col_bias"), dev_ptr(d_rb, F32, "d_row_bias"),
              None if call is None else call.data_ptr(), ws.data_ptr(), current_stream())
        ctx.keep = (ul, il, h, row_bias, col_bias, drop, u_ids, i_ids, off, items, logq, call)      # the pointers of ctx.ops / ctx.ids
        ctx.unit = (d_ul, d_il, d_h, d_rb, d_cb) if grads else None
        ctx.mark_non_differentiable(pos)
        return loss, pos

    @staticmethod
    def backward(ctx, d_loss, _d_pos):
        ul, il, h, row_bias, col_bias = ctx.keep[:5]
        call = ctx.keep[-1]
        unit = _UNIT.get(ul.device)
        if unit is not None and ctx.unit is not None and d_loss.data_ptr() == unit.data_ptr():
            d_ul, d_il, d_h, d_rb, d_cb = ctx.unit
        else:
            d_loss = d_loss.contiguous()
            d_ul, d_il = torch.empty_like(ul), torch.empty_like(il)
            d_h = torch.empty_like(h) if h is not None and ctx.ops[0] == _lib.SCORE_FM else None
            d_cb = torch.empty_like(col_bias) if col_bias is not None else None
            d_rb = torch.empty_like(row_bias) if row_bias is not None else None
            scratch = torch.empty(ctx.ops[1], dtype=F32, device=ul.device)
            L_ = _lib.lib()
            ws = _pair_softmax_ws(ul.device, L_.rbr_pair_softmax_ws_bytes(ctx.ops[1], ctx.ops[2]))
            _call("pair_softmax_bwd", L_.rbr_pair_softmax_bwd, *ctx.ops, None if call is None else call.data_ptr(), *ctx.ids,
                  dev_ptr(d_loss, F32, "d_loss"), dev_ptr(scratch, F32, "pos"), dev_ptr(d_ul, F32, "d_ul"), dev_ptr(d_il, F32, "d_il"),
                  dev_ptr(d_h, F32, "d_h"), dev_ptr(d_cb, F32, "d_col_bias"), dev_ptr(d_rb, F32, "d_row_bias"), ws.data_ptr(),
                  current_stream())
        d_h, d_rb, d_cb = (None if t is None else t.view(s) for t, s in zip((d_h, d_rb, d_cb), ctx.shapes))
        return (d_ul, d_il, d_h, d_rb, d_cb) + (None,) * 9


def pair_softmax_loss(ul, il, u_ids, i_ids, mode, h=None, row_bias=None, col_bias=None, drop=None, seen=None, item_lo=1, logq=None,
                      temperature=1.0, *, p_drop: float = 0.0):
    """(loss, pos) of the in-batch softmax over ALL B x B pairs of the latent rows ul / il [B, K] (rbr_pair_softmax_fwd): row a's
    positive is column a, its negatives the other items of the batch -- except an item below item_lo (the pad id), the row's own
    item again, and an item its user has rated (`seen`: a recommend.SeenItems / (off int64 [U + 1], items int32 sorted within a row),
    the form of sample_negatives; None = no list).  mode "fm": s = (relu(ul[a] * il[b]) * drop[a, b]) . h + row_bias[a] + col_bias[b]
    -- pass row_bias = ub[u_ids] + g and col_bias = ib[i_ids] for the model's own score --, mode "dot": s = ul[a] . il[b] + biases.
    z = s / temperature - logq[b]; loss = mean_a (logsumexp over the allowed b of z[a, b] - z[a, a]); pos [B] = s[a, a], detached.
    Dropout (fm only): drop [B, B, K] an explicit multiplier, or p_drop > 0: drawn in the kernel, the draw of
    dropout_multiplier((B, B, K), p_drop, ...) for the same call number.  Autograd through ul, il, h, col_bias; row_bias gets a
    gradient of exact zeros (a per-user constant cancels in a softmax over items).  Two launches, no float atomics: the same bits
    on every run; 1 <= B <= 4096, 1 <= K <= 256, there is no fallback."""
    if mode not in SCORE_MODES:
        raise ValueError(f"unknown score mode {mode!r}; one of {sorted(SCORE_MODES)}")
    if ul.dim() != 2 or ul.shape != il.shape:
        raise RuntimeError(f"pair_softmax_loss: ul / il must be [B, K] each, got {tuple(ul.shape)} / {tuple(il.shape)}")
    B = ul.shape[0]
    dev_ptr(ul.detach().contiguous(), F32, "user latents")        # device gate first: a CPU tensor is refused before anything else
    if u_ids.shape != (B,) or i_ids.shape != (B,):
        raise RuntimeError(f"pair_softmax_loss: u_ids / i_ids must be [{B}] each, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")
    seen_csr = _seen_csr(seen, ul.device)
    if not temperature > 0:
        raise ValueError(f"pair_softmax_loss: temperature must be positive, got {temperature}")
    return _PairSoftmaxLoss.apply(ul, il, h, row_bias, col_bias, u_ids, i_ids, mode, drop, p_drop, seen_csr, int(item_lo), logq,
                                  1.0 / float(temperature))


# --------------------------------------------------------------------------- NARRE attention pool
class _ReviewAttn(torch.autograd.Function):
    """out[B,H], att[B,R,1] = LinearAttention(feat[B,R,H], other_id[B,R])  -- rbr_review_attn_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, feat, other_id, pad_idx, W_rv, W_id, h, b1, b2, ebd, drop=None):
        B, R, H = feat.shape
        A = W_rv.shape[1]
        dev = feat.device
        L_ = _lib.lib()
        feat = feat.contiguous()
        other_id = other_id.contiguous()
        params = [t.contiguous() for t in (W_rv, W_id, h, b1, b2, ebd)]
        names = ("W_rv", "W_id", "h", "b1", "b2", "ebd")
        ap = _lib.AttnParams(*[dev_ptr(t, F32, n) for t, n in zip(params, names)])
        out = torch.empty(B, H, dtype=F32, device=dev)
        att = torch.empty(B, R, 1, dtype=F32, device=dev)
        hid = torch.empty(B, R, A, dtype=F32, device=dev)
        drop = drop.contiguous() if drop is not None else None
        if drop is not None and tuple(drop.shape) != (B, H):
            raise RuntimeError(f"review_attention: dropout multiplier {tuple(drop.shape)} is not [B, H] = {(B, H)}")
        _call(None, L_.rbr_review_attn_fwd, B, R, H, A, dev_ptr(feat, F32, "feat"), dev_ptr(other_id, I64, "other_id"), C.byref(ap),
              dev_ptr(drop, F32, "drop"), dev_ptr(out, F32, "out"), dev_ptr(att, F32, "att"), dev_ptr(hid, F32, "hid"),
              current_stream())
        ctx.dims = (B, R, H, A, int(pad_idx))
        ctx.has_drop = drop is not None
        ctx.set_materialize_grads(False)     # an unused `att` output arrives as None in backward, not as a freshly filled zero tensor
        ctx.save_for_backward(feat, other_id, att, hid, *params, *([drop] if drop is not None else []))
        return out, att

    @staticmethod
    def backward(ctx, d_out, d_att):
        B, R, H, A, pad_idx = ctx.dims
        feat, other_id, att, hid = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:10]
        drop = ctx.saved_tensors[10] if ctx.has_drop else None
        names = ("W_rv", "W_id", "h", "b1", "b2", "ebd")
        dev = feat.device
        L_ = _lib.lib()
        ap = _lib.AttnParams(*[dev_ptr(t, F32, n) for t, n in zip(params, names)])
        grads = [torch.zeros_like(t) if n == "ebd" else torch.empty_like(t) for t, n in zip(params, names)]
        ag = _lib.AttnGrads(*[dev_ptr(t, F32, "d" + n) for t, n in zip(grads, names)])
        d_feat = torch.empty_like(feat)
        ws = torch.empty(L_.rbr_review_attn_bwd_ws_floats(B, R, H, A), dtype=F32, device=dev)
        d_out = d_out.contiguous() if d_out is not None else torch.zeros(B, H, dtype=F32, device=dev)
        d_att = d_att.contiguous() if d_att is not None else None
        _call(None, L_.rbr_review_attn_bwd, B, R, H, A, dev_ptr(feat, F32, "feat"), dev_ptr(other_id, I64, "other_id"), C.byref(ap),
              dev_ptr(drop, F32, "drop"), dev_ptr(att, F32, "att"), dev_ptr(hid, F32, "hid"), dev_ptr(d_out, F32, "d_out"),
              dev_ptr(d_att, F32, "d_att"), pad_idx, C.byref(ag), dev_ptr(d_feat, F32, "d_feat"), dev_ptr(ws, F32, "ws"),
              current_stream())
        return (d_feat, None, None, *grads, None)


class _ReviewAttn2(torch.autograd.Function):
    """Both LinearAttention pools of a two-tower model in one launch per stage -- rbr_review_attn2_* in rbr_hip.h.
    feat [2,B,R,H], other_id [2,B,R], drop [2,B,H] or None, then the six parameters of side 0 and of side 1."""

    NAMES = ("W_rv", "W_id", "h", "b1", "b2", "ebd")

    @staticmethod
    def forward(ctx, feat, other_id, pad0, pad1, drop, *params):
        _, B, R, H = feat.shape
        A = params[0].shape[1]
        dev = feat.device
        L_ = _lib.lib()
        feat, other_id = feat.contiguous(), other_id.contiguous()
        params = [t.contiguous() for t in params]
        names = _ReviewAttn2.NAMES
        aps = [_lib.AttnParams(*[dev_ptr(t, F32, n) for t, n in zip(params[6 * k:6 * k + 6], names)]) for k in range(2)]
        drop = drop.contiguous() if drop is not None else None
        if drop is not None and tuple(drop.shape) != (2, B, H):
            raise RuntimeError(f"review_attention2: dropout multiplier {tuple(drop.shape)} is not [2, B, H] = {(2, B, H)}")
        out = torch.empty(2, B, H, dtype=F32, device=dev)
        att = torch.empty(2, B, R, 1, dtype=F32, device=dev)
        hid = torch.empty(2, B, R, A, dtype=F32, device=dev)
        _call(None, L_.rbr_review_attn2_fwd, B, R, H, A, dev_ptr(feat, F32, "feat"), dev_ptr(other_id, I64, "other_id"),
              C.byref(aps[0]), C.byref(aps[1]), dev_ptr(drop, F32, "drop"), dev_ptr(out, F32, "out"), dev_ptr(att, F32, "att"),
              dev_ptr(hid, F32, "hid"), current_stream())
        ctx.dims = (B, R, H, A, int(pad0), int(pad1))
        ctx.has_drop = drop is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(feat, other_id, att, hid, *params, *([drop] if drop is not None else []))
        return out, att

    @staticmethod
    def backward(ctx, d_out, d_att):
        B, R, H, A, pad0, pad1 = ctx.dims
        feat, other_id, att, hid = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:16]
        drop = ctx.saved_tensors[16] if ctx.has_drop else None
        names = _ReviewAttn2.NAMES
        dev = feat.device
        L_ = _lib.lib()
        aps = [_lib.AttnParams(*[dev_ptr(t, F32, n) for t, n in zip(params[6 * k:6 * k + 6], names)]) for k in range(2)]
        grads = [torch.empty_like(t) for t in params]           # the embedding-row gradients are zeroed by the call
        ags = [_lib.AttnGrads(*[dev_ptr(t, F32, "d" + n) for t, n in zip(grads[6 * k:6 * k + 6], names)]) for k in range(2)]
        d_feat = torch.empty_like(feat)
        ws = torch.empty(2 * L_.rbr_review_attn_bwd_ws_floats(B, R, H, A), dtype=F32, device=dev)
        d_out = d_out.contiguous() if d_out is not None else torch.zeros(2, B, H, dtype=F32, device=dev)
        d_att = d_att.contiguous() if d_att is not None else None
        _call(None, L_.rbr_review_attn2_bwd, B, R, H, A, dev_ptr(feat, F32, "feat"), dev_ptr(other_id, I64, "other_id"),
              C.byref(aps[0]), C.byref(aps[1]), dev_ptr(drop, F32, "drop"), dev_ptr(att, F32, "att"), dev_ptr(hid, F32, "hid"),
              dev_ptr(d_out, F32, "d_out"), dev_ptr(d_att, F32, "d_att"), pad0, pad1, C.byref(ags[0]), C.byref(ags[1]),
              params[5].shape[0], params[11].shape[0], dev_ptr(d_feat, F32, "d_feat"), dev_ptr(ws, F32, "ws"), current_stream())
        return (d_feat, None, None, None, None, *grads)


def review_attention2(feat, other_id, params0, params1, *, pad_idx=(0, 0), drop=None):
    """The user and the item LinearAttention of NARRE in one launch per stage: feat [2,B,R,H] (side 0 first), other_id [2,B,R],
    params0 / params1 = (W_rv, W_id, h, b1, b2, ebd) of the sides, drop [2,B,H] or None.  Returns (out [2,B,H], att [2,B,R,1])."""
    return _ReviewAttn2.apply(feat, other_id, pad_idx[0], pad_idx[1], drop, *params0, *params1)


def review_attention(feat, other_id, W_rv, W_id, h, b1, b2, ebd, *, pad_idx=0, drop=None):
    """NARRE LinearAttention: returns (out [B,H], att [B,R,1]).  `drop` [B,H]: the multiplier of the nn.Dropout that follows
    (dropout_multiplier), applied inside the kernels -- forward and backward -- instead of by two elementwise launches."""
    return _ReviewAttn.apply(feat, other_id, pad_idx, W_rv, W_id, h, b1, b2, ebd, drop)


class _BlockCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c, d):
        a, b, c, d = (t.contiguous() for t in (a, b, c, d))
        B, C1, C2 = a.shape[0], a.shape[1], b.shape[1]
        if c.shape != a.shape or d.shape != b.shape or b.shape[0] != B:
            raise RuntimeError("block_cat: expected a, c [B, C1] and b, d [B, C2]")
        out = torch.empty(2 * B, C1 + C2, dtype=F32, device=a.device)
        _call(None, _lib.lib().rbr_block_cat, B, C1, C2, dev_ptr(a, F32, "a"), dev_ptr(b, F32, "b"), dev_ptr(c, F32, "c"),
              dev_ptr(d, F32, "d"), dev_ptr(out, F32, "out"), current_stream())
        ctx.dims = (B, C1, C2)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C1, C2 = ctx.dims
        g = g.contiguous()
        a, c = (torch.empty(B, C1, dtype=F32, device=g.device) for _ in range(2))
        b, d = (torch.empty(B, C2, dtype=F32, device=g.device) for _ in range(2))
        _call(None, _lib.lib().rbr_block_split, B, C1, C2, dev_ptr(g, F32, "g"), dev_ptr(a, F32, "a"), dev_ptr(b, F32, "b"),
              dev_ptr(c, F32, "c"), dev_ptr(d, F32, "d"), current_stream())
        return a, b, c, d


def block_cat(a, b, c, d):
    """[[a, b], [c, d]] as one [2B, C1 + C2] tensor (a, c [B, C1]; b, d [B, C2]): torch.cat((cat((a, b), 1), cat((c, d), 1)), 0)
    in one launch, and contiguous gradient pieces from one launch in the backward."""
    return _BlockCat.apply(a, b, c, d)


class _PairDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, K = x.shape[0] // 2, x.shape[1]
        out = torch.empty(B, dtype=F32, device=x.device)
        _call(None, _lib.lib().rbr_pair_dot_fwd, B, K, dev_ptr(x, F32, "x"), dev_ptr(out, F32, "out"), current_stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        B, K = x.shape[0] // 2, x.shape[1]
        d_x = torch.empty_like(x)
        d_out = d_out.contiguous()
        _call(None, _lib.lib().rbr_pair_dot_bwd, B, K, dev_ptr(x, F32, "x"), dev_ptr(d_out, F32, "d_out"), dev_ptr(d_x, F32, "d_x"),
              current_stream())
        return d_x


def pair_dot(stacked: torch.Tensor) -> torch.Tensor:
    """ratings[b] = sum_k stacked[b, k] * stacked[B + b, k] for a [2B, K] block with the user rows first (D-ATT's
    `torch.sum(torch.mul(u_feat, i_feat), 1)`, dual_att.py:58, on the shared fc's stacked output)."""
    if stacked.dim() != 2 or stacked.shape[0] % 2:
        raise RuntimeError(f"pair_dot: expected a [2B, K] block, got {tuple(stacked.shape)}")
    return _PairDot.apply(stacked)


# --------------------------------------------------------------------------- nn.Linear on MFMA
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, relu, drop):
        N, IN = x.shape
        OUT = W.shape[0]
        L_ = _lib.lib()
        x, W = x.contiguous(), W.contiguous()
        b = b.contiguous() if b is not None else None
        drop = drop.contiguous() if drop is not None else None
        y = torch.empty(N, OUT, dtype=F32, device=x.device)
        wsn = L_.rbr_linear_fwd_ws_floats(N, IN, OUT)          # > 0: the product is split along K (few output tiles)
        ws = torch.empty(wsn, dtype=F32, device=x.device) if wsn else None
        _call(None, L_.rbr_linear_fwd_ex, N, IN, OUT, dev_ptr(x, F32, "x"), dev_ptr(W, F32, "W"), dev_ptr(b, F32, "b"), int(relu),
              dev_ptr(drop, F32, "drop"), dev_ptr(y, F32, "y"), dev_ptr(ws, F32, "ws"), current_stream())
        ctx.relu = int(relu)
        ctx.has_b = b is not None
        ctx.has_drop = drop is not None
        ctx.save_for_backward(x, W, y, *([drop] if drop is not None else []))
        return y

    @staticmethod
    def backward(ctx, d_y):
        x, W, y = ctx.saved_tensors[:3]
        drop = ctx.saved_tensors[3] if ctx.has_drop else None
        N, IN = x.shape
        OUT = W.shape[0]
        L_ = _lib.lib()
        dev = x.device
        d_y = d_y.contiguous()
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W)
        db = torch.empty(OUT, dtype=F32, device=dev) if ctx.has_b else None
        ws = torch.empty(L_.rbr_linear_bwd_ex_ws_floats(N, IN, OUT), dtype=F32, device=dev)
        _call(None, L_.rbr_linear_bwd_ex, N, IN, OUT, dev_ptr(x, F32, "x"), dev_ptr(W, F32, "W"), dev_ptr(y, F32, "y"),
              dev_ptr(d_y, F32, "d_y"), ctx.relu, dev_ptr(drop, F32, "drop"), dev_ptr(d_x, F32, "d_x"), dev_ptr(dW, F32, "dW"),
              dev_ptr(db, F32, "db"), dev_ptr(ws, F32, "ws"), current_stream())
        return d_x, dW, db, None, None


def linear(x, W, b=None, *, relu=False, drop=None, tanh=False):
    """y = act(x @ W^T + b) * drop  with torch's nn.Linear weight layout [OUT, IN]; act = ReLU, Tanh or none."""
    return _Linear.apply(x, W, b, 2 if tanh else int(bool(relu)), drop)


class _ConvShiftAdd(torch.autograd.Function):
    """out [bz, C, L] = bias + the kz shifted adds of the product T [bz * L, sum kz*ch]  -- rbr_conv_shift_add_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, t, bz, L, kernel_sizes, channels, *biases):
        t = t.contiguous()
        bs = [b.contiguous() for b in biases]
        n = len(kernel_sizes)
        kz = (C.c_int32 * n)(*[int(k) for k in kernel_sizes])
        ch = (C.c_int32 * n)(*[int(c) for c in channels])
        out = torch.empty(bz, sum(channels), L, dtype=F32, device=t.device)
        _call(None, _lib.lib().rbr_conv_shift_add_fwd, bz, L, n, kz, ch, dev_ptr(t, F32, "T"), ptr_array(bs, F32, "bias"),
              dev_ptr(out, F32, "out"), current_stream())
        ctx.job = (bz, L, tuple(kernel_sizes), tuple(channels), tuple(t.shape))
        return out

    @staticmethod
    def backward(ctx, d_out):
        bz, L, kernel_sizes, channels, tshape = ctx.job
        n = len(kernel_sizes)
        kz = (C.c_int32 * n)(*kernel_sizes)
        ch = (C.c_int32 * n)(*channels)
        d_out = d_out.contiguous()
        dT = torch.empty(tshape, dtype=F32, device=d_out.device)
        dbs = [torch.empty(c, dtype=F32, device=d_out.device) for c in channels]
        _call(None, _lib.lib().rbr_conv_shift_add_bwd, bz, L, n, kz, ch, dev_ptr(d_out, F32, "d_out"), dev_ptr(dT, F32, "dT"),
              ptr_array(dbs, F32, "dbias"), current_stream())
        return (dT, None, None, None, None, *dbs)


def conv_shift_add(t, bz, L, kernel_sizes, channels, biases):
    """MyConv1d.forward's epilogue (deepconn/layers.py:46-60): 'same' padding, shifted adds, bias, channel cat, N x C x L layout --
    one launch.  t [bz * L, sum kz*ch] is the layer's product (functional.linear); returns [bz, sum ch, L]."""
    return _ConvShiftAdd.apply(t, bz, L, kernel_sizes, channels, *biases)


# --------------------------------------------------------------------------- SimpleSiamese encoder
class _ReviewBag(torch.autograd.Function):
    """out[n_rev, D] = drop * masked mean of table[ids]  -- rbr_review_bag_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, table, ids, mask, drop, padding_idx):
        dev_ptr(table.contiguous(), F32, "word table")
        if ids.dim() != 2:
            raise RuntimeError("ids must be [n_reviews, review_len]")
        n_rev, T = ids.shape
        D = table.shape[1]
        L_ = _lib.lib()
        table_c, ids = table.contiguous(), ids.contiguous()
        mask8 = _mask_u8(mask)
        if mask8 is not None and mask8.shape != ids.shape:
            raise AssertionError("input_masks must be [n_reviews, review_len]")
        drop = drop.contiguous() if drop is not None else None
        out = torch.empty(n_rev, D, dtype=F32, device=table.device)
        inv_len = torch.empty(n_rev, dtype=F32, device=table.device)
        _call(None, L_.rbr_review_bag_fwd, n_rev, T, D, dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(table_c, F32, "word table"), dev_ptr(drop, F32, "drop"), dev_ptr(out, F32, "out"),
              dev_ptr(inv_len, F32, "inv_len"), current_stream())
        ctx.dims = (n_rev, T, D, -1 if padding_idx is None else int(padding_idx), tuple(table.shape))
        ctx.has_mask, ctx.has_drop = mask8 is not None, drop is not None
        ctx.save_for_backward(ids, inv_len, *([mask8] if mask8 is not None else []), *([drop] if drop is not None else []))
        return out

    @staticmethod
    def backward(ctx, d_out):
        n_rev, T, D, pad, shape = ctx.dims
        saved = list(ctx.saved_tensors)
        ids, inv_len = saved[:2]
        k = 2
        mask8 = drop = None
        if ctx.has_mask:
            mask8 = saved[k]; k += 1
        if ctx.has_drop:
            drop = saved[k]
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        dtable = torch.zeros(shape, dtype=F32, device=d_out.device)
        d_out = d_out.contiguous()
        L_ = _lib.lib()
        ws = torch.empty(L_.rbr_review_bag_bwd_ws_bytes(n_rev, T), dtype=torch.uint8, device=d_out.device)
        _call(None, L_.rbr_review_bag_bwd, n_rev, T, D, shape[0], dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(drop, F32, "drop"), dev_ptr(inv_len, F32, "inv_len"), dev_ptr(d_out, F32, "d_out"), pad,
              dev_ptr(dtable, F32, "dtable"), ws.data_ptr(), current_stream())
        return dtable, None, None, None, None


def review_bag(table, ids, mask, *, drop=None, padding_idx=0):
    """WordEmbedding -> VariationalDropout (multiplier `drop` [n_rev, D]) -> MaskedAvgPooling1d.  [n_rev, D]."""
    return _ReviewBag.apply(table, ids, mask, drop, padding_idx)


class _AdditiveAttn(torch.autograd.Function):
    """out[B,H], scores[B,R] = AddictiveAttention(node_drop * rev[B,R,H], mask[B,R])  -- rbr_additive_attn_*."""

    @staticmethod
    def forward(ctx, rev, mask, node_drop, Wp, bp, wi):
        if rev.dim() != 3:
            raise RuntimeError("inputs must be [bz, seq_len, hdim]")
        B, R, H = rev.shape
        K = Wp.shape[0]
        L_ = _lib.lib()
        rev, Wp, bp, wi = rev.contiguous(), Wp.contiguous(), bp.contiguous(), wi.contiguous().view(-1)
        mask8 = _mask_u8(mask)
        if mask8 is not None and mask8.dim() != 2:
            raise AssertionError("input_masks.dim() == 2")          # simple_siamese/layers.py:189
        node_drop = node_drop.contiguous() if node_drop is not None else None
        dev = rev.device
        out = torch.empty(B, H, dtype=F32, device=dev)
        scores = torch.empty(B, R, dtype=F32, device=dev)
        t = torch.empty(B, R, K, dtype=F32, device=dev)
        _call(None, L_.rbr_additive_attn_fwd, B, R, H, K, dev_ptr(rev, F32, "inputs"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(node_drop, F32, "node_drop"), dev_ptr(Wp, F32, "proj weight"), dev_ptr(bp, F32, "proj bias"),
              dev_ptr(wi, F32, "inner_product weight"), dev_ptr(out, F32, "out"), dev_ptr(scores, F32, "scores"),
              dev_ptr(t, F32, "t"), current_stream())
        ctx.dims = (B, R, H, K)
        ctx.has_mask, ctx.has_nd = mask8 is not None, node_drop is not None
        ctx.wi_shape = None
        ctx.save_for_backward(rev, Wp, wi, scores, t, *([mask8] if mask8 is not None else []),
                              *([node_drop] if node_drop is not None else []))
        ctx.mark_non_differentiable(scores)
        return out, scores

    @staticmethod
    def backward(ctx, d_out, _d_scores):
        B, R, H, K = ctx.dims
        saved = list(ctx.saved_tensors)
        rev, Wp, wi, scores, t = saved[:5]
        k = 5
        mask8 = node_drop = None
        if ctx.has_mask:
            mask8 = saved[k]; k += 1
        if ctx.has_nd:
            node_drop = saved[k]
        L_ = _lib.lib()
        dev = rev.device
        d_out = d_out.contiguous()
        d_rev = torch.empty_like(rev)
        d_Wp = torch.empty_like(Wp)
        d_bp = torch.empty(K, dtype=F32, device=dev)
        d_wi = torch.empty(K, dtype=F32, device=dev)
        ws = torch.empty(L_.rbr_additive_attn_bwd_ws_floats(B, R, H, K), dtype=F32, device=dev)
        _call(None, L_.rbr_additive_attn_bwd, B, R, H, K, dev_ptr(rev, F32, "inputs"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(node_drop, F32, "node_drop"), dev_ptr(Wp, F32, "proj weight"), dev_ptr(wi, F32, "inner_product weight"),
              dev_ptr(scores, F32, "scores"), dev_ptr(t, F32, "t"), dev_ptr(d_out, F32, "d_out"), dev_ptr(d_rev, F32, "d_inputs"),
              dev_ptr(d_Wp, F32, "d_Wp"), dev_ptr(d_bp, F32, "d_bp"), dev_ptr(d_wi, F32, "d_wi"), dev_ptr(ws, F32, "ws"),
              current_stream())
        return d_rev, None, None, d_Wp, d_bp, d_wi.view(1, K)


def additive_attention(rev, mask, Wp, bp, wi, *, node_drop=None):
    """AddictiveAttention over the reviews (+ NodeDropout multiplier [B,R]).  Returns (out [B,H], scores [B,R,1]).
    rev [B,R,H], Wp [K,H]: B, R, H, K >= 1, R <= 64 and, for the kernels' 64 KiB of LDS, K + H <= 256 and
    R * (H + K + 2) + H <= 16384; a shape outside is refused by the library (RBR_ERR_BAD_ARG) and raises RuntimeError."""
    out, scores = _AdditiveAttn.apply(rev, mask, node_drop, Wp, bp, wi)
    return out, scores.unsqueeze(2)


class SiameseSaliency(NamedTuple):
    """siamese_saliency: fixed / through [n, R, T], reviews [n, R]; fixed + through is gradient x input of the token rows."""
    fixed: torch.Tensor
    through: torch.Tensor
    reviews: torch.Tensor


def siamese_saliency(table, ids, word_mask, rev_mask, y, a, g, Wt, Wp, bp, wi) -> SiameseSaliency:
    """What every token and every review of a SimpleSiamese tower contributes to a score whose gradient on the tower's pooled
    feature is g [n, F]: ids [n, R, T] over table [V, E], y [n, R, F] the review vectors the attention read and a [n, R] (or
    [n, R, 1]) its weights, as review_bag / linear(tanh=True) / additive_attention left them; Wt [F, E] the latent transform's
    weight or None; Wp [K, F], bp [K], wi [1, K] the attention's parameters.  fixed + through = <d score / d row, row> of every
    token's embedded row, followed through the transform and the attention softmax; fixed holds the attention constant, and
    reviews = a * <g, y>.  rbr_siamese_saliency in rbr_hip.h has the formula.  One launch, no autograd, no embedded rows are
    materialised; a side row is bit-identical in every batch."""
    if ids.dim() != 3:
        raise RuntimeError(f"ids must be [n, R, T], got {tuple(ids.shape)}")
    n, R, T = ids.shape
    if table.dim() != 2:
        raise RuntimeError(f"the word table must be [V, E], got {tuple(table.shape)}")
    table_c = table.detach()
    table_c = table_c if table_c.is_contiguous() else table_c.contiguous()
    V, E = table_c.shape
    ids = ids.contiguous()
    wm8, rm8 = _mask_u8(word_mask), _mask_u8(rev_mask)
    if wm8 is not None and wm8.shape != ids.shape:
        raise RuntimeError(f"word_mask must be [n, R, T] = {tuple(ids.shape)}, got {tuple(wm8.shape)}")
    if rm8 is not None and tuple(rm8.shape) != (n, R):
        raise RuntimeError(f"rev_mask must be [n, R] = {(n, R)}, got {tuple(rm8.shape)}")
    y, g = y.detach().contiguous(), g.detach().contiguous()
    if y.dim() != 3 or tuple(y.shape[:2]) != (n, R):
        raise RuntimeError(f"y must be [n, R, F] with [n, R] = {(n, R)}, got {tuple(y.shape)}")
    F = y.shape[2]
    if tuple(a.shape) not in ((n, R), (n, R, 1)):
        raise RuntimeError(f"a must be [n, R] = {(n, R)} (or [n, R, 1]), got {tuple(a.shape)}")
    a = a.detach().reshape(n, R).contiguous()
    if tuple(g.shape) != (n, F):
        raise RuntimeError(f"g must be [n, F] = {(n, F)}, got {tuple(g.shape)}")
    Wp, bp, wi = Wp.detach().contiguous(), bp.detach().contiguous(), wi.detach().contiguous().view(-1)
    K = Wp.shape[0]
    if tuple(Wp.shape) != (K, F) or tuple(bp.shape) != (K,) or tuple(wi.shape) != (K,):
        raise RuntimeError(f"the attention's parameters must be Wp [K, F = {F}], bp [K], wi [K], got {tuple(Wp.shape)} / "
                           f"{tuple(bp.shape)} / {tuple(wi.shape)}")
    if Wt is not None:
        Wt = Wt.detach().contiguous()
        if tuple(Wt.shape) != (F, E):
            raise RuntimeError(f"the transform's weight must be [F, E] = {(F, E)}, got {tuple(Wt.shape)}")
    dev = table_c.device
    fixed, through = (torch.empty(n, R, T, dtype=F32, device=dev) for _ in range(2))
    reviews = torch.empty(n, R, dtype=F32, device=dev)
    _call("siamese_saliency", _lib.lib().rbr_siamese_saliency, n, R, T, V, E, F, K, dev_ptr(table_c, F32, "word table"),
          dev_ptr(ids, I64, "ids"), dev_ptr(wm8, U8, "word_mask"), dev_ptr(rm8, U8, "rev_mask"), dev_ptr(y, F32, "y"),
          dev_ptr(a, F32, "a"), dev_ptr(g, F32, "g"), dev_ptr(Wt, F32, "transform weight"), dev_ptr(Wp, F32, "proj weight"),
          dev_ptr(bp, F32, "proj bias"), dev_ptr(wi, F32, "inner_product weight"), dev_ptr(fixed, F32, "fixed"),
          dev_ptr(through, F32, "through"), dev_ptr(reviews, F32, "reviews"), current_stream())
    return SiameseSaliency(fixed, through, reviews)


# --------------------------------------------------------------------------- standalone embedding
class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, padding_idx):
        L_ = _lib.lib()
        table = table.contiguous()
        flat = ids.contiguous().view(-1)
        D = table.shape[1]
        out = torch.empty(flat.numel(), D, dtype=F32, device=table.device)
        if flat.numel():
            _call(None, L_.rbr_embedding_fwd, flat.numel(), D, dev_ptr(flat, I64, "ids"), dev_ptr(table, F32, "table"),
                  dev_ptr(out, F32, "out"), current_stream())
        ctx.pad = -1 if padding_idx is None else int(padding_idx)
        ctx.shape = table.shape
        ctx.save_for_backward(flat)
        return out.view(*ids.shape, D)

    @staticmethod
    def backward(ctx, d_out):
        (flat,) = ctx.saved_tensors
        L_ = _lib.lib()
        D = ctx.shape[1]
        dtable = torch.zeros(ctx.shape, dtype=F32, device=d_out.device)
        d_out = d_out.contiguous().view(-1, D)
        if flat.numel():
            _call(None, L_.rbr_embedding_bwd, flat.numel(), D, dev_ptr(flat, I64, "ids"), dev_ptr(d_out, F32, "d_out"), ctx.pad,
                  dev_ptr(dtable, F32, "dtable"), current_stream())
        return dtable, None, None


def embedding(table, ids, padding_idx=0):
    """Materialised row gather table[ids] -> [*ids.shape, D] (WordEmbedding.forward)."""
    return _Embedding.apply(table, ids, padding_idx)


# --------------------------------------------------------------------------- HierPooling
class _HierPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, mask, k, relu, padding_idx):
        n_docs, L = ids.shape
        V, D = table.shape
        L_ = _lib.lib()
        table = table.contiguous()
        ids = ids.contiguous()
        mask8 = _mask_u8(mask)
        pooled = torch.empty(n_docs, D, dtype=F32, device=table.device)
        argmax = torch.empty(n_docs, D, dtype=I32, device=table.device)
        _call(None, L_.rbr_hier_pool_fwd, n_docs, L, D, int(k), dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(table, F32, "table"), int(relu), dev_ptr(pooled, F32, "pooled"), dev_ptr(argmax, I32, "argmax"),
              current_stream())
        ctx.args = (n_docs, L, D, int(k), int(relu), -1 if padding_idx is None else int(padding_idx), tuple(table.shape))
        ctx.has_mask = mask8 is not None
        ctx.save_for_backward(ids, argmax, pooled, *([mask8] if mask8 is not None else []))
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        n_docs, L, D, k, relu, pad, shape = ctx.args
        ids, argmax, pooled = ctx.saved_tensors[:3]
        mask8 = ctx.saved_tensors[3] if ctx.has_mask else None
        L_ = _lib.lib()
        dtable = torch.zeros(shape, dtype=F32, device=d_pooled.device)
        d_pooled = d_pooled.contiguous()
        _call(None, L_.rbr_hier_pool_bwd, n_docs, L, D, k, dev_ptr(ids, I64, "ids"), dev_ptr(mask8, U8, "mask"),
              dev_ptr(argmax, I32, "argmax"), dev_ptr(pooled, F32, "pooled"), dev_ptr(d_pooled, F32, "d_pooled"), relu, pad,
              dev_ptr(dtable, F32, "dtable"), current_stream())
        return dtable, None, None, None, None, None


def hier_pool(table, ids, masks, kernel_size, proj_w, proj_b, padding_idx=0):
    """NgramFeat arch="HierPooling": window mean -> global max -> optional Linear -> ReLU.  [n_docs, H]."""
    if proj_w is None:
        return _HierPool.apply(table, ids, masks, kernel_size, True, padding_idx)
    pooled = _HierPool.apply(table, ids, masks, kernel_size, False, padding_idx)
    return linear(pooled, proj_w, proj_b, relu=True)


# --------------------------------------------------------------------------- D-ATT gates
class _DattGate(torch.autograd.Function):
    """gate[B,L] of LocalAttention (win odd) or GlobalAttention (is_global) -- rbr_datt_*_gate_* in rbr_hip.h."""

    @staticmethod
    def forward(ctx, table, w, b0, ids, is_global, padding_idx, rows=None):
        ctx.fanout_acc = _fanout_acc(table)
        ctx.gate_ws = None
        ctx.rows = rows                              # the tower's distinct-token rows (datt_token_rows) or None
        B, L = ids.shape
        E = table.shape[1]
        win = w.shape[2]
        L_ = _lib.lib()
        table, w, b0, ids = table.contiguous(), w.contiguous(), b0.contiguous(), ids.contiguous()
        gate = torch.empty(B, L, dtype=F32, device=table.device)
        if is_global:
            if win != L:
                raise RuntimeError(f"GlobalAttention weight spans {win} positions but documents have {L}")
            _call(None, L_.rbr_datt_global_gate_fwd, B, L, E, dev_ptr(ids, I64, "ids"), dev_ptr(table, F32, "table"),
                  dev_ptr(w, F32, "w"), dev_ptr(b0, F32, "b0"), dev_ptr(gate, F32, "gate"), current_stream())
        else:
            V = table.shape[0]
            ws_bytes = L_.rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V)     # > 0: token-product form of the gate
            if ws_bytes:
                ctx.gate_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=table.device)
                _call(None, L_.rbr_datt_local_gate_fwd_prod, B, L, E, win, V, dev_ptr(ids, I64, "ids"),
                      dev_ptr(table, F32, "table"), dev_ptr(w, F32, "w"), dev_ptr(b0, F32, "b0"), dev_ptr(gate, F32, "gate"),
                      ctx.gate_ws.data_ptr(), None if rows is None else rows.data_ptr(), current_stream())
            else:
                _call(None, L_.rbr_datt_local_gate_fwd, B, L, E, win, dev_ptr(ids, I64, "ids"), dev_ptr(table, F32, "table"),
                      dev_ptr(w, F32, "w"), dev_ptr(b0, F32, "b0"), dev_ptr(gate, F32, "gate"), current_stream())
        ctx.args = (B, L, E, win, bool(is_global), -1 if padding_idx is None else int(padding_idx))
        ctx.save_for_backward(table, w, ids, gate)
        return gate

    @staticmethod
    def backward(ctx, dgate):
        B, L, E, win, is_global, pad = ctx.args
        table, w, ids, gate = ctx.saved_tensors
        L_ = _lib.lib()
        dev = table.device
        dgate = dgate.contiguous()
        dw = torch.empty_like(w)
        db0 = torch.empty(1, dtype=F32, device=dev)
        acc = _table_acc(ctx.fanout_acc, dev) if ctx.needs_input_grad[0] else None      # the step's shared gradient buffer
        if ctx.gate_ws is not None:      # token-product local gate: the whole table gradient is overwritten (or its rows added)
            dtable = (acc if acc is not None else torch.empty_like(table)) if ctx.needs_input_grad[0] else None
            _call(None, L_.rbr_datt_local_gate_bwd_prod, B, L, E, win, table.shape[0], dev_ptr(ids, I64, "ids"),
                  dev_ptr(table, F32, "table"), dev_ptr(w, F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(dgate, F32, "dgate"), pad,
                  dev_ptr(dw, F32, "dw"), dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dtable"), ctx.gate_ws.data_ptr(),
                  None if ctx.rows is None else ctx.rows.data_ptr(), int(acc is not None), current_stream())
            return dtable, dw, db0, None, None, None, None
        V = table.shape[0]
        rows_floats = L_.rbr_datt_global_gate_bwd_rows_ws_floats(B, L, E, V) if (ctx.rows is not None and is_global) else 0
        if rows_floats:                  # global gate over the tower's token rows: occurrence matrix, dtable overwritten
            dtable = (acc if acc is not None else torch.empty_like(table)) if ctx.needs_input_grad[0] else None
            ws = torch.empty(rows_floats, dtype=F32, device=dev)
            _call(None, L_.rbr_datt_global_gate_bwd_rows, B, L, E, V, dev_ptr(ids, I64, "ids"), dev_ptr(table, F32, "table"),
                  dev_ptr(w, F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(dgate, F32, "dgate"), pad, dev_ptr(dw, F32, "dw"),
                  dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dtable"), dev_ptr(ws, F32, "ws"), ctx.rows.data_ptr(),
                  int(acc is not None), current_stream())
            return dtable, dw, db0, None, None, None, None
        dtable = torch.zeros_like(table) if ctx.needs_input_grad[0] else None
        ws = torch.empty(max(1, L_.rbr_datt_gate_bwd_ws_floats(B, L, E, win, int(is_global))), dtype=F32, device=dev)
        if is_global:
            _call(None, L_.rbr_datt_global_gate_bwd, B, L, E, dev_ptr(ids, I64, "ids"), dev_ptr(table, F32, "table"),
                  dev_ptr(w, F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(dgate, F32, "dgate"), pad, dev_ptr(dw, F32, "dw"),
                  dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dtable"), dev_ptr(ws, F32, "ws"), current_stream())
        else:
            _call(None, L_.rbr_datt_local_gate_bwd, B, L, E, win, dev_ptr(ids, I64, "ids"), dev_ptr(table, F32, "table"),
                  dev_ptr(w, F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(dgate, F32, "dgate"), pad, dev_ptr(dw, F32, "dw"),
                  dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dtable"), dev_ptr(ws, F32, "ws"), current_stream())
        return dtable, dw, db0, None, None, None, None


def datt_gate(table, w, b0, ids, *, is_global, padding_idx=0, rows=None):
    """sigmoid attention gate [B,L]; w is the Conv1d weight [1,E,win] (local) or [1,E,L] (global).  `rows`: the tower's
    distinct-token rows (datt_token_rows), shared by its two gates -- the token-product local gate uses them instead of
    building its own, the global gate's backward builds the table gradient from the occurrence matrix over them."""
    return _DattGate.apply(table, w, b0, ids, is_global, padding_idx, rows)


# --------------------------------------------------------------------------- D-ATT: both towers through every kernel in one pass
@contextlib.contextmanager
def _pair_region():
    """with _pair_region() as region: problem 0's calls; region.next(); problem 1's calls -- the C-ABI calls inside are recorded,
    and leave at the end as shared launches (rbr_pair_begin / _next / _end of rbr_hip.h).  Nothing but library calls and
    allocations may happen inside (a torch op would run ahead of the recorded launches)."""
    L_ = _lib.lib()
    _call(None, L_.rbr_pair_begin)

    class _Region:
        paired = singles = 0

        @staticmethod
        def next():
            _call(None, L_.rbr_pair_next)

    region = _Region()
    try:
        yield region
    except BaseException:
        L_.rbr_pair_abort()
        raise
    n_p, n_s = C.c_int32(0), C.c_int32(0)
    _call(None, L_.rbr_pair_end, C.byref(n_p), C.byref(n_s))
    region.paired, region.singles = n_p.value, n_s.value


PAIR_STATS = {"paired": 0, "singles": 0}      # launches of the last paired D-ATT forward + backward that left as pairs / singly


class _NoRegion:
    """Stands in for a pair region in bench.py's kernel-timing pass (TIMER.enabled): the same calls, launched where they are made,
    so that HIP events can bracket them -- the long kernels of the step (GEMM, gather, the G chain) leave singly in a region too
    (PairSolo), so what the events see is what a region launches."""
    paired = singles = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    @staticmethod
    def next():
        pass


def _region_or_timed():
    return _NoRegion() if TIMER.enabled else _pair_region()


def _token_rows_pay(V: int, B: int, L: int) -> bool:
    """The distinct-token rows of a tower's [B, L] documents pay: enough positions per vocabulary entry, and RBR_DATT_ROWS=0
    does not switch them off.  The rule is token_rows_pay() of csrc/rbr_common.h (the token-product conv and local gate); this
    is its copy for rbr_datt_token_rows, whose workspace query answers for every shape."""
    return not (V * 5 > B * L * 2 or B * L < 4096 or os.environ.get("RBR_DATT_ROWS", "1") == "0")


def datt_pair_applies(table, docs2, local_w, conv_ws) -> bool:
    """True when both D-ATT towers can go through datt_towers(): equal shapes by construction (one [2B, L] id block), the
    token-product forms of the local gate and of the merged four-bank conv apply, the distinct-token rows pay, and the GEMM is
    one of the bf16-plane kernels (the f32 MFMA kernel still launches directly)."""
    if not (table.is_cuda and table.dtype == F32 and docs2.dim() == 2 and docs2.shape[0] % 2 == 0):
        return False
    if os.environ.get("RBR_DATT_PAIRED", "1") == "0" or get_prod_precision() == "f32":
        return False
    B, L = docs2.shape[0] // 2, docs2.shape[1]
    V, E = table.shape
    win = int(local_w.shape[2])
    L_ = _lib.lib()
    if not _token_rows_pay(V, B, L):
        return False
    if not L_.rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V) or not L_.rbr_datt_global_gate_bwd_rows_ws_floats(B, L, E, V):
        return False
    desc = _conv_desc(table, B, L, conv_ws, PAD_VALID, ACT_TANH, 0, _lib.conv_gate_split(1))
    return bool(L_.rbr_textcnn_fwd_ws_bytes(C.byref(desc)) > 0 and L_.rbr_textcnn_bwd_prod_ws_bytes(C.byref(desc)) > 0
                and conv_ws[0].shape[2] == 1)


class _DattTowers(torch.autograd.Function):
    """feats [2B, l_out + 3 g_out] = both D-ATT towers' encoders (reference models/dual_att/dual_att.py:45-57, layers.py:43-53,
    81-89): per tower the distinct-token rows, the local gate, the global gate and the merged four-bank gated conv (local 1-wide
    bank under the local gate, global 2/3/4-wide banks under the global gate) -- the SAME C-ABI calls the single-tower functions
    make (_DattGate, _TextCNN), issued for tower 0 and tower 1 inside a pair region, so every kernel runs once for both towers
    (gridDim.z = 2).  The towers have separate parameters and share the word table; each tower adds its table-gradient rows
    into a buffer of its own (two towers' workgroups of one launch may meet in a row) and the buffers are summed at the end."""

    N_TOWER_PARAMS = 12        # local attn w, b | global attn w, b | conv weights x4 | conv biases x4

    @staticmethod
    def forward(ctx, table, docs2, padding_idx, pad_runs, *params):
        NP = _DattTowers.N_TOWER_PARAMS
        if len(params) != 2 * NP:
            raise RuntimeError("datt_towers: expected 2 x 12 tower parameters")
        L_ = _lib.lib()
        dev = table.device
        table_c = table.contiguous()
        dev_ptr(table_c, F32, "word table")
        docs2 = docs2.contiguous()
        dev_ptr(docs2, I64, "docs")
        B, L = docs2.shape[0] // 2, docs2.shape[1]
        V, E = table.shape
        pad = -1 if padding_idx is None else int(padding_idx)
        st = current_stream()
        towers = []
        for t in range(2):
            q = [x.contiguous() for x in params[t * NP:(t + 1) * NP]]
            tw = _ConvSaved(ids=docs2[t * B:(t + 1) * B], lw=q[0], lb=q[1], gw=q[2], gb=q[3], ws=q[4:8], bs=q[8:12])
            if tw.gw.shape[2] != L:
                raise RuntimeError(f"GlobalAttention weight spans {tw.gw.shape[2]} positions but documents have {L}")
            towers.append(tw)
        win = int(towers[0].lw.shape[2])

        def layer_dims(tw):
            return [int(w.shape[2]) for w in tw.ws], [int(w.shape[0]) for w in tw.ws], int(tw.lw.shape[2])

        if layer_dims(towers[0]) != layer_dims(towers[1]):
            raise RuntimeError("datt_towers: the towers' layers must have equal shapes")
        desc = _conv_desc(table, B, L, towers[0].ws, PAD_VALID, ACT_TANH, padding_idx,
                          _lib.conv_gate_split(1) | _pad_runs_flag(pad_runs, None, padding_idx))
        Ctot = sum(desc.ch[:desc.n_widths])
        rows_bytes = L_.rbr_datt_token_rows_ws_bytes(B, L, V)
        gws_bytes = L_.rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V)
        feats = torch.empty(2 * B, Ctot, dtype=F32, device=dev)
        argmax = torch.empty(2 * B, Ctot, dtype=I32, device=dev)
        for t, tw in enumerate(towers):          # allocations only: nothing here launches
            tw.rows = torch.empty(rows_bytes, dtype=torch.uint8, device=dev)
            tw.gate2 = torch.empty(2, B, L, dtype=F32, device=dev)          # plane 0: local gate, plane 1: global gate
            tw.gate_ws = torch.empty(gws_bytes, dtype=torch.uint8, device=dev)
            _conv_fwd_buffers(tw, desc, dev, feats[t * B:(t + 1) * B], argmax[t * B:(t + 1) * B])
        if not (rows_bytes and gws_bytes and towers[0].prod_ws is not None):
            check(-1, "datt_towers plan (datt_pair_applies() was not consulted)")
        tab = dev_ptr(table_c, F32, "table")
        # (Measured and dropped, round 4: tower 1's product-table GEMM on a second stream beside tower 0's gather -- MFMA / LDS work
        # beside L2-request work.  The GEMM's 137 MB of product-table writes push the table the gather is reading out of the L2s and
        # the Infinity Cache: the gather 125 -> 205 us, the GEMM 48 -> 150 us, the step +80 us.  Also dropped: both gates on the second
        # stream beside tower 0's GEMM, which needs the token list only -- the GEMM 49 -> 81 us, the gates' three kernels 102 -> 134,
        # the gather starts 4 us earlier: everything here queues at the same L2s.)
        with _timed("datt_towers_fwd"), _region_or_timed() as region:
            for t, tw in enumerate(towers):
                if t == 1:
                    region.next()
                ids_p = dev_ptr(tw.ids, I64, "ids")
                _call(None, L_.rbr_datt_token_rows, B, L, V, ids_p, tw.rows.data_ptr(), st)
                _call(None, L_.rbr_datt_local_gate_fwd_prod, B, L, E, win, V, ids_p, tab, dev_ptr(tw.lw, F32, "w"),
                      dev_ptr(tw.lb, F32, "b0"), dev_ptr(tw.gate2[0], F32, "gate"), tw.gate_ws.data_ptr(), tw.rows.data_ptr(), st)
                _call(None, L_.rbr_datt_global_gate_fwd, B, L, E, ids_p, tab, dev_ptr(tw.gw, F32, "w"), dev_ptr(tw.gb, F32, "b0"),
                      dev_ptr(tw.gate2[1], F32, "gate"), st)
                _prod_forward(desc, tw, table_c, tw.ids, None, tw.gate2, tw.ws, st, prepare_key=None)
                _pool_finalize(desc, tw, tw.bs, st)
        PAIR_STATS["paired"], PAIR_STATS["singles"] = region.paired, region.singles
        for tw in towers:
            tw.pval = tw.pidx = None           # only the backward's inputs stay
        ctx.towers, ctx.desc, ctx.table = towers, desc, table_c
        ctx.dims = (B, L, V, E, win, pad)
        ctx.keep = (feats, argmax, docs2)
        ctx.set_materialize_grads(False)
        return feats

    @staticmethod
    def backward(ctx, d_feats):
        NP = _DattTowers.N_TOWER_PARAMS
        towers, desc, table = ctx.towers, ctx.desc, ctx.table
        B, L, V, E, win, pad = ctx.dims
        L_ = _lib.lib()
        dev = table.device
        if d_feats is None:
            d_feats = torch.zeros_like(ctx.keep[0])
        d_feats = d_feats.contiguous()
        need_table = ctx.needs_input_grad[0]
        # Table-gradient buffers [4, V, E], allocated (and the gates' cleared) BEFORE the regions: [t] receives tower t's gate rows
        # (added: local gate, then global gate, one after the other on this stream), [2 + t] its conv rows (g_times_w's dense
        # form: every row written, absent tokens' rows zero).  Gates and conv of a tower run on DIFFERENT streams below, and two
        # towers' workgroups of one launch may meet in a row: four writers, four buffers, summed once at the end.
        dtab = torch.empty(4, V, E, dtype=F32, device=dev) if need_table else None
        if need_table:
            dtab[:2].zero_()
        bws_bytes = L_.rbr_textcnn_bwd_prod_ws_bytes(C.byref(desc))
        gg_floats = L_.rbr_datt_global_gate_bwd_rows_ws_floats(B, L, E, V)
        wsn = L_.rbr_textcnn_bwd_ws_floats(C.byref(desc))
        for tw in towers:
            tw.bws = torch.empty(bws_bytes, dtype=torch.uint8, device=dev)
            tw.dgate2 = torch.empty(2, B, L, dtype=F32, device=dev)          # zeroed by the launch that zeroes G's rows
            tw.gg_ws = torch.empty(gg_floats, dtype=F32, device=dev)
            tw.wsb = torch.empty(max(wsn, 1), dtype=F32, device=dev)
            tw.grads = ([torch.empty_like(tw.lw), torch.empty(1, dtype=F32, device=dev), torch.empty_like(tw.gw),
                         torch.empty(1, dtype=F32, device=dev)] + [torch.empty_like(w) for w in tw.ws]
                        + [torch.empty(w.shape[0], dtype=F32, device=dev) for w in tw.ws])
        st = current_stream()
        # Two streams, two regions.  Region A: G and d(gate) of both towers on this stream (zero_g_rows, build_g), the conv weight
        # gradient (dw_partial4, dw_reduce: it starts from d_feats alone) on the second one.  Region B: the gates' backwards on
        # this stream -- they need d(gate) -- and the conv's sparse product G @ Wprod^T on the second stream behind the weight
        # gradient -- it needs G.  (One stream for everything but the weight gradient, as in round 3: the second stream idle for
        # 600 us of the backward's 750.)
        side = _side_stream(dev)
        if side is not None:
            fork = torch.cuda.Event()
            fork.record()
            side.wait_event(fork)
        st2 = side.cuda_stream if side is not None else st
        st_prod = st if TIMER.enabled else st2      # (the timing pass brackets calls with events on THIS stream)
        tab = dev_ptr(table, F32, "table")
        paired = singles = 0
        with _timed("datt_towers_bwd"):
            with _region_or_timed() as region:
                for t, tw in enumerate(towers):
                    if t == 1:
                        region.next()
                    d_feat = d_feats[t * B:(t + 1) * B]
                    _call(None, L_.rbr_textcnn_bwd_dw, C.byref(desc), dev_ptr(tw.ids, I64, "ids"), None, dev_ptr(tw.gate2, F32, "gate"),
                          tab, dev_ptr(tw.feat, F32, "feat"), dev_ptr(tw.argmax, I32, "argmax"), dev_ptr(d_feat, F32, "d_feat"),
                          ptr_array(tw.grads[4:8], F32, "dW"), ptr_array(tw.grads[8:12], F32, "dbias"), dev_ptr(tw.wsb, F32, "ws"), st2)
                    _g_chain(None, _lib.G_BUILD, st, desc, (tw.ids, None, tw.gate2, tw.feat, tw.argmax, d_feat), tw.prod_ws, tw.bws,
                             None, tw.dgate2, None)
            paired, singles = paired + region.paired, singles + region.singles
            if side is not None:          # G is complete on this stream (the region's launches have left): the product may follow it
                g_done = torch.cuda.Event()
                g_done.record()
                side.wait_event(g_done)
            with _region_or_timed() as region:
                for t, tw in enumerate(towers):
                    if t == 1:
                        region.next()
                    ids_p = dev_ptr(tw.ids, I64, "ids")
                    dt = dev_ptr(dtab[t], F32, "dtable") if need_table else None
                    if need_table:
                        _g_chain("textcnn_bwd_g_product", _lib.G_PRODUCT, st_prod, desc, None, tw.prod_ws, tw.bws, dtab[2 + t], None, None)
                    _call(None, L_.rbr_datt_local_gate_bwd_prod, B, L, E, win, V, ids_p, tab, dev_ptr(tw.lw, F32, "w"),
                          dev_ptr(tw.gate2[0], F32, "gate"), dev_ptr(tw.dgate2[0], F32, "dgate"), pad, dev_ptr(tw.grads[0], F32, "dw"),
                          dev_ptr(tw.grads[1], F32, "db0"), dt, tw.gate_ws.data_ptr(), tw.rows.data_ptr(), 1, st)
                    # the global gate's weight phase (dpre, dw: both towers per launch); its table rows follow outside the region
                    _call(None, L_.rbr_datt_global_gate_bwd_rows, B, L, E, V, ids_p, tab, dev_ptr(tw.gw, F32, "w"),
                          dev_ptr(tw.gate2[1], F32, "gate"), dev_ptr(tw.dgate2[1], F32, "dgate"), pad, dev_ptr(tw.grads[2], F32, "dw"),
                          dev_ptr(tw.grads[3], F32, "db0"), None, dev_ptr(tw.gg_ws, F32, "ws"), tw.rows.data_ptr(), 1, st)
            paired, singles = paired + region.paired, singles + region.singles
            if need_table:
                # ... a chain of four launches over the tower's 120 MB occurrence matrix, one tower at a time either way: tower 0's
                # on this stream into its gate buffer, tower 1's on the second stream behind the sparse products, into the buffer
                # its conv rows were written to there (same stream: no fifth buffer) -- both streams then end about together
                if side is not None and not TIMER.enabled:
                    dpre_done = torch.cuda.Event()
                    dpre_done.record()
                    side.wait_event(dpre_done)
                for t, tw in enumerate(towers):
                    on_side = t == 1 and side is not None and not TIMER.enabled
                    _call(None, L_.rbr_datt_global_gate_bwd_rows, B, L, E, V, dev_ptr(tw.ids, I64, "ids"), None, dev_ptr(tw.gw, F32, "w"),
                          None, None, pad, None, None, dev_ptr(dtab[3] if on_side else dtab[t], F32, "dtable"),
                          dev_ptr(tw.gg_ws, F32, "ws"), tw.rows.data_ptr(), 1 | 2, st2 if on_side else st)
            if side is not None:
                with torch.cuda.stream(side):
                    join = torch.cuda.Event()
                    join.record()
                _join(join)
        PAIR_STATS["paired"] += paired
        PAIR_STATS["singles"] += singles
        dtable = dtab.sum(0) if need_table else None
        grads = towers[0].grads + towers[1].grads
        for tw in towers:
            tw.bws = tw.dgate2 = tw.gg_ws = tw.wsb = tw.grads = None
        return (dtable, None, None, None, *grads)


def datt_towers(table, docs2, u_params, i_params, *, padding_idx=0, pad_runs=True):
    """Both D-ATT towers' encoders in one pass (see _DattTowers): docs2 [2B, L] int64 (user documents, then item documents);
    u_params / i_params = (local attn weight [1,E,win], bias [1], global attn weight [1,E,L], bias [1], [4 conv weights],
    [4 conv biases]).  Returns feats [2B, l_out + 3 g_out], user rows first: cat((local, global), 1) per tower."""
    flat = []
    for q in (u_params, i_params):
        lw, lb, gw, gb, ws, bs = q
        flat += [lw, lb, gw, gb, *ws, *bs]
    return _DattTowers.apply(table, docs2, padding_idx, pad_runs, *flat)


def datt_token_rows(ids, vocab_size):
    """Distinct-token row maps of one tower's documents (rbr_datt_token_rows), or None where they do not pay (few positions
    per vocabulary entry: the same rule as the token-product conv)."""
    B, L = ids.shape
    if not _token_rows_pay(vocab_size, B, L):
        return None
    L_ = _lib.lib()
    rows = torch.empty(L_.rbr_datt_token_rows_ws_bytes(B, L, vocab_size), dtype=torch.uint8, device=ids.device)
    ids = ids.contiguous()
    _call(None, L_.rbr_datt_token_rows, B, L, vocab_size, dev_ptr(ids, I64, "ids"), rows.data_ptr(), current_stream())
    return rows


# --------------------------------------------------------------------------- scores and top-K from cached tower latents
@contextlib.contextmanager
def eval_mode(module):
    """no_grad + module.eval() for the block (the towers' encode_users / encode_items, Recommender.refresh): no dropout is drawn
    and nothing is recorded for a backward; the module's previous train / eval mode is restored afterwards."""
    was = module.training
    module.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        module.train(was)


SCORE_MODES = {"fm": _lib.SCORE_FM, "dot": _lib.SCORE_DOT}


def _score_operands(mode, ul, il, h, g, ub, ib):
    """The operands every pair_score_* entry shares: mode code, detached contiguous tables, the FM parameters as flat vectors
    (h [K, 1] -> [K], ub / ib [n, 1] -> [n]).  The dot mode ignores h, g, ub, ib."""
    if mode not in SCORE_MODES:
        raise ValueError(f"unknown score mode {mode!r}; one of {sorted(SCORE_MODES)}")
    ul, il = ul.detach().contiguous(), il.detach().contiguous()
    if ul.dim() != 2 or il.dim() != 2 or ul.shape[1] != il.shape[1]:
        raise RuntimeError(f"latent tables must be [U, K] / [I, K], got {tuple(ul.shape)} / {tuple(il.shape)}")
    dev_ptr(ul, F32, "user latents")        # device gate first: a CPU tensor is refused before anything else is looked at
    dev_ptr(il, F32, "item latents")
    K = ul.shape[1]
    if mode == "dot":
        return SCORE_MODES[mode], ul, il, None, None, None, None
    if h is None or g is None:
        raise RuntimeError("the fm score needs h [K] and g [1]")
    flat = [None if t is None else t.detach().contiguous().view(-1) for t in (h, g, ub, ib)]
    for t, n, name in zip(flat, (K, 1, ul.shape[0], il.shape[0]), ("h", "g", "ub", "ib")):
        if t is not None and t.numel() != n:
            raise RuntimeError(f"{name} must hold {n} values, got {t.numel()}")
    return (SCORE_MODES[mode], ul, il, *flat)


def pair_score(mode, ul, il, u_ids, i_ids, h=None, g=None, ub=None, ib=None):
    """scores [B] of the pairs (u_ids[b], i_ids[b]) from the latent tables ul [U, K] / il [I, K] (rbr_pair_score_ids): mode "fm" =
    relu(ul[u] * il[i]) . h + ub[u] + ib[i] + g (FM.forward in eval mode; ub / ib None = FMWithoutUIBias), mode "dot" =
    sum(ul[u] * il[i]) (D-ATT).  No autograd.  An id outside its table scores as row 0 and is recorded like sanitize_ids()
    records it: check_id_errors() raises the IndexError at the caller's next synchronisation point."""
    code, ul, il, h, g, ub, ib = _score_operands(mode, ul, il, h, g, ub, ib)
    u_ids, i_ids = u_ids.contiguous(), i_ids.contiguous()
    if u_ids.dim() != 1 or u_ids.shape != i_ids.shape:
        raise RuntimeError(f"u_ids / i_ids must be [B] each, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")
    B = u_ids.shape[0]
    out = torch.empty(B, dtype=F32, device=ul.device)
    if B:
        _call("pair_score_ids", _lib.lib().rbr_pair_score_ids, code, B, ul.shape[1], dev_ptr(ul, F32, "ul"), ul.shape[0],
              dev_ptr(il, F32, "il"), il.shape[0], dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"), dev_ptr(h, F32, "h"),
              dev_ptr(g, F32, "g"), dev_ptr(ub, F32, "ub"), dev_ptr(ib, F32, "ib"), dev_ptr(out, F32, "out"),
              _id_err(ul.device).data_ptr(), current_stream())
    return out


def pair_score_dense(mode, ul, il, h=None, g=None, ub=None, ib=None):
    """scores [Nu, Ni] of every user row of ul [Nu, K] (ub [Nu]) against every item row of il [Ni, K] (rbr_pair_score_dense): the
    same arithmetic, bit for bit, as pair_score and pair_score_topk.  For tests and small catalogues -- it IS the U x I matrix."""
    code, ul, il, h, g, ub, ib = _score_operands(mode, ul, il, h, g, ub, ib)
    out = torch.empty(ul.shape[0], il.shape[0], dtype=F32, device=ul.device)
    if out.numel():
        _call("pair_score_dense", _lib.lib().rbr_pair_score_dense, code, ul.shape[0], il.shape[0], ul.shape[1], dev_ptr(ul, F32, "ul"),
              dev_ptr(il, F32, "il"), dev_ptr(h, F32, "h"), dev_ptr(g, F32, "g"), dev_ptr(ub, F32, "ub"), dev_ptr(ib, F32, "ib"),
              dev_ptr(out, F32, "out"), current_stream())
    return out


def _exclusion_csr(exclude, Nu, dev):
    """(off, items, rows, nnz, n_rows) of the `exclude` argument of pair_score_topk / pair_score_rank for Nu user rows; all None /
    0 for no list."""
    if exclude is None:
        return None, None, None, 0, 0
    off, items = exclude[0].contiguous(), exclude[1].contiguous()
    rows = exclude[2].contiguous() if len(exclude) > 2 else None
    n_rows = off.shape[0] - 1
    if off.dim() != 1 or (rows is None and n_rows != Nu) or (rows is not None and (rows.shape != (Nu,) or n_rows < 1)):
        raise RuntimeError(f"exclude offsets must be [{Nu + 1}] (or [R + 1] with rows [{Nu}]), got {tuple(off.shape)}")
    nnz = items.numel()
    if nnz == 0:         # a zero-sized tensor has no pointer to hand over: one unused entry keeps the CSR form
        items = torch.zeros(1, dtype=I32, device=dev)
    return off, items, rows, nnz, n_rows if rows is not None else 0


def _seen_csr(seen, dev):
    """(off, items, nnz, U) of the `seen` argument of the samplers and pair_softmax_loss -- (off int64 [U + 1], items int32), the
    two-array form of `exclude` with one row per user id; None, None, 0, 0 for no list."""
    if seen is None:
        return None, None, 0, 0
    if len(seen) != 2:
        raise RuntimeError("seen must be (off [U + 1], items): one row per user id")
    U = seen[0].shape[0] - 1
    off, items, _, nnz, _ = _exclusion_csr(seen, U, dev)
    return off, items, nnz, U


def pair_score_topk(mode, ul, il, k, h=None, g=None, ub=None, ib=None, *, item_lo=0, exclude=None):
    """(items int64 [Nu, k], scores f32 [Nu, k]): for every user row of ul [Nu, K] the k best items of [item_lo, Ni), score
    descending, ties by the lower item id, the same bytes on every run (rbr_pair_score_topk; 1 <= k <= 128).  `exclude` lists
    the items a row must never get, CSR and sorted within a row: (excl_off int64 [Nu + 1], excl_item int32), or
    (excl_off [R + 1], excl_item, rows int64 [Nu]) where user row r takes row rows[r] of a CSR of R rows.  A row with fewer than
    k candidates ends in item -1, score -inf.  The [Nu, Ni] matrix is never built; no autograd, no host synchronisation, one
    workspace from the torch allocator: recordable into a graph on one stream."""
    code, ul, il, h, g, ub, ib = _score_operands(mode, ul, il, h, g, ub, ib)
    Nu, Ni, K, k = ul.shape[0], il.shape[0], ul.shape[1], int(k)
    dev = ul.device
    off, items, rows, nnz, n_rows = _exclusion_csr(exclude, Nu, dev)
    L_ = _lib.lib()
    if Nu == 0:
        return torch.empty(0, k, dtype=I64, device=dev), torch.empty(0, k, dtype=F32, device=dev)
    # a shape the entry refuses has a workspace of 0 bytes: the call below then returns its error code and text before any launch
    ws = torch.empty(max(L_.rbr_pair_score_topk_ws_bytes(Nu, Ni, K, k), 8), dtype=torch.uint8, device=dev)
    out_item = torch.empty(Nu, max(k, 0), dtype=I64, device=dev)
    out_score = torch.empty(Nu, max(k, 0), dtype=F32, device=dev)
    _call("pair_score_topk", L_.rbr_pair_score_topk, code, Nu, Ni, K, k, int(item_lo), dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"),
          dev_ptr(h, F32, "h"), dev_ptr(g, F32, "g"), dev_ptr(ub, F32, "ub"), dev_ptr(ib, F32, "ib"), dev_ptr(off, I64, "exclude offsets"),
          dev_ptr(items, I32, "exclude items"), nnz, dev_ptr(rows, I64, "exclude rows"), n_rows,
          dev_ptr(out_item, I64, "out_item"), dev_ptr(out_score, F32, "out_score"), ws.data_ptr(), current_stream())
    return out_item, out_score


def pair_score_rank(mode, ul, il, targets, h=None, g=None, ub=None, ib=None, *, item_lo=0, exclude=None):
    """(rank int32 [B], n_cand int32 [B]) of the held-out items `targets` int64 [B] for the user rows ul [B, K] (ub [B]), one row
    per pair (rbr_pair_score_rank): rank[b] is the number of candidates that come before targets[b] in the order of
    pair_score_topk (score descending, ties by the lower item id) -- its position in that row's top-k list of any k -- and
    n_cand[b] the number of candidates.  Candidates are the items of [item_lo, Ni) with a non-NaN score that `exclude` (the forms
    of pair_score_topk, a row per pair) does not list; the target is a candidate even when its row lists it.  rank -1: the target
    is outside [item_lo, Ni) or scores NaN (it is in no top-k list); one outside [0, Ni) is also recorded for check_id_errors().
    Exact integers from the arithmetic of every other pair_score entry; the [B, Ni] matrix is never built; no autograd, no host
    synchronisation, one workspace from the torch allocator: recordable into a graph on one stream."""
    code, ul, il, h, g, ub, ib = _score_operands(mode, ul, il, h, g, ub, ib)
    B, Ni, K = ul.shape[0], il.shape[0], ul.shape[1]
    dev = ul.device
    targets = targets.contiguous()
    if targets.shape != (B,):
        raise RuntimeError(f"targets must be [{B}], one per user row, got {tuple(targets.shape)}")
    off, items, rows, nnz, n_rows = _exclusion_csr(exclude, B, dev)
    rank = torch.empty(B, dtype=I32, device=dev)
    n_cand = torch.empty(B, dtype=I32, device=dev)
    if B == 0:
        return rank, n_cand
    L_ = _lib.lib()
    # a shape the entry refuses has a workspace of 0 bytes: the call below then returns its error code and text before any launch
    ws = torch.empty(max(L_.rbr_pair_score_rank_ws_bytes(B, Ni, K), 8), dtype=torch.uint8, device=dev)
    _call("pair_score_rank", L_.rbr_pair_score_rank, code, B, Ni, K, int(item_lo), dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"),
          dev_ptr(h, F32, "h"), dev_ptr(g, F32, "g"), dev_ptr(ub, F32, "ub"), dev_ptr(ib, F32, "ib"), dev_ptr(targets, I64, "targets"),
          dev_ptr(off, I64, "exclude offsets"), dev_ptr(items, I32, "exclude items"), nnz, dev_ptr(rows, I64, "exclude rows"), n_rows,
          dev_ptr(rank, I32, "rank"), dev_ptr(n_cand, I32, "n_cand"), _id_err(dev).data_ptr(), ws.data_ptr(), current_stream())
    return rank, n_cand


# --------------------------------------------------------------------------- negatives for a pairwise objective
def _sampler_operands(u_ids, i_ids, n_neg, seen, state, out):
    """The operands both samplers share, checked: contiguous ids, B, n_neg, the seen CSR (U rows, offsets, items, nnz) and the
    three output tensors (allocated where `out` is None)."""
    u_ids, i_ids = u_ids.contiguous(), i_ids.contiguous()
    if u_ids.dim() != 1 or u_ids.shape != i_ids.shape:
        raise RuntimeError(f"u_ids / i_ids must be [B] each, got {tuple(u_ids.shape)} / {tuple(i_ids.shape)}")
    B, n_neg, dev = u_ids.shape[0], int(n_neg), u_ids.device
    off, items, nnz, U = _seen_csr(seen, dev)
    if state.shape != (2,) or state.dtype != I64:
        raise RuntimeError(f"state must be int64 [2], got {state.dtype} {tuple(state.shape)}")
    rows = (1 + max(n_neg, 0)) * B
    if out is None:
        out = (torch.empty(rows, dtype=I64, device=dev), torch.empty(rows, dtype=I64, device=dev),
               torch.empty(max(n_neg, 0) * B, dtype=F32, device=dev))
    u_out, i_out, valid = out
    if u_out.shape != (rows,) or i_out.shape != (rows,) or valid.shape != (rows - B,):
        raise RuntimeError(f"out must be u_out [{rows}], i_out [{rows}], valid [{rows - B}]")
    return u_ids, i_ids, B, n_neg, U, off, items, nnz, (u_out, i_out, valid)


def sample_negatives(u_ids, i_ids, n_neg: int, n_items: int, seen=None, *, state, seed: int = 0, item_lo: int = 1,
                     max_tries: int = 16, replace_id: int = 0, out=None):
    """(u_out int64 [(1 + n_neg) * B], i_out int64 [(1 + n_neg) * B], valid f32 [n_neg * B]) for the observed pairs (u_ids[b],
    i_ids[b]) (rbr_sample_negatives, one launch): rows [0, B) are the pairs themselves, rows [(j+1)B, (j+2)B) pair b's j-th
    negative -- an item of [item_lo, n_items) that is neither i_ids[b] nor in the user's row of `seen`, with replacement across j;
    valid[j*B + b] = 0 (and item replace_id) where a user has no such item.  `seen`: a recommend.SeenItems / (off int64 [U + 1],
    items int32 sorted within a row) over all user ids -- the first exclusion form of pair_score_topk -- or None.
    `state`: int64 [2] on the device, [call number, 0]; the launch advances the call number itself, so two calls (or two replays of
    a recorded call) draw different sets, and (seed, call number) fixes a set exactly (the draw is stated in include/rbr_hip.h).
    `out`: the three tensors to write into.  No autograd, no host synchronisation, no allocation with `out`: graph-capturable."""
    u_ids, i_ids, B, n_neg, U, off, items, nnz, (u_out, i_out, valid) = _sampler_operands(u_ids, i_ids, n_neg, seen, state, out)
    if B == 0 and n_neg >= 1:
        return u_out, i_out, valid
    _call("sample_negatives", _lib.lib().rbr_sample_negatives, B, n_neg, int(n_items), int(item_lo), dev_ptr(u_ids, I64, "u_ids"),
          dev_ptr(i_ids, I64, "i_ids"), dev_ptr(off, I64, "seen offsets"), dev_ptr(items, I32, "seen items"), nnz, U,
          int(seed) & 0xFFFFFFFFFFFFFFFF, dev_ptr(state, I64, "state"), int(max_tries), int(replace_id), dev_ptr(u_out, I64, "u_out"),
          dev_ptr(i_out, I64, "i_out"), dev_ptr(valid, F32, "valid"), current_stream())
    return u_out, i_out, valid


def sample_hard_negatives(u_ids, i_ids, n_neg: int, n_items: int, seen=None, *, n_cand: int, mode, ul, il, h=None, g=None, ub=None,
                          ib=None, state, seed: int = 0, item_lo: int = 1, max_tries: int = 16, replace_id: int = 0, out=None,
                          return_candidates: bool = False):
    """sample_negatives with dynamic negative sampling (rbr_sample_hard_negatives, one launch): every negative is the best-scoring
    of n_cand (1..64) draws of sample_negatives' kind -- candidate m of draw d uses draw index d * n_cand + m -- scored from the
    latent tables ul [U, K] / il [I, K] with the arithmetic and the operands of pair_score (`mode`, h, g, ub, ib), bit for bit;
    score descending, ties by the lower item id, a NaN score never wins while another candidate has a number.  n_cand = 1 gives
    sample_negatives' outputs byte for byte.  U is the row count of ul AND of `seen`; a user id outside [0, U) scores as row 0.
    Returns (u_out, i_out, valid) in sample_negatives' layout; with return_candidates also (cand int64, cand_score f32), each
    [n_neg, B, n_cand]: every candidate (replace_id where a user has no acceptable item) and its score.  The tables and the head's
    parameters are read through their pointers at every launch: a recorded call sees what they hold at replay time.  No autograd,
    no host synchronisation, no allocation with `out` and without return_candidates: graph-capturable."""
    u_ids, i_ids, B, n_neg, seen_rows, off, items, nnz, (u_out, i_out, valid) = _sampler_operands(u_ids, i_ids, n_neg, seen, state, out)
    code, ul, il, h, g, ub, ib = _score_operands(mode, ul, il, h, g, ub, ib)
    U, n_cand = ul.shape[0], int(n_cand)
    if seen is not None and seen_rows != U:
        raise RuntimeError(f"seen must hold one row per row of ul ({U}), got {seen_rows}")
    if il.shape[0] != int(n_items):
        raise RuntimeError(f"il must hold n_items = {int(n_items)} rows, got {il.shape[0]}")
    cand = cand_score = None
    if return_candidates:
        cand = torch.empty(max(n_neg, 0), B, max(n_cand, 0), dtype=I64, device=u_ids.device)
        cand_score = torch.empty(max(n_neg, 0), B, max(n_cand, 0), dtype=F32, device=u_ids.device)
    if not (B == 0 and n_neg >= 1 and 1 <= n_cand <= 64):
        _call("sample_hard_negatives", _lib.lib().rbr_sample_hard_negatives, B, n_neg, n_cand, int(n_items), int(item_lo),
              dev_ptr(u_ids, I64, "u_ids"), dev_ptr(i_ids, I64, "i_ids"), dev_ptr(off, I64, "seen offsets"),
              dev_ptr(items, I32, "seen items"), nnz, U, code, ul.shape[1], dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"),
              dev_ptr(h, F32, "h"), dev_ptr(g, F32, "g"), dev_ptr(ub, F32, "ub"), dev_ptr(ib, F32, "ib"),
              int(seed) & 0xFFFFFFFFFFFFFFFF, dev_ptr(state, I64, "state"), int(max_tries), int(replace_id),
              dev_ptr(u_out, I64, "u_out"), dev_ptr(i_out, I64, "i_out"), dev_ptr(valid, F32, "valid"),
              dev_ptr(cand, I64, "cand"), dev_ptr(cand_score, F32, "cand_score"), current_stream())
    if return_candidates:
        return u_out, i_out, valid, cand, cand_score
    return u_out, i_out, valid


# --------------------------------------------------------------------------- AHN: the pair tail over cached sentence tables
class AhnUserState(NamedTuple):
    """Per-user rows of AHN's sentence tables (AHN.encode_users; rbr_ahn_user_state): everything of a user the pair tail reads."""
    X: torch.Tensor             # [U, Ru * Su, F] the encoder's sentence vectors
    Xt: torch.Tensor            # [U, Ru * Su, F] X @ Wt^T, user_review_trans_layer's product moved in front of the weighted sum
    sent_masks: torch.Tensor    # [U, Ru, Su] bool
    rev_masks: torch.Tensor     # [U, Ru] bool
    fm: torch.Tensor            # [U, K + 2] the id embedding's part of the FM


class AhnItemState(NamedTuple):
    """Per-item rows (AHN.encode_items; rbr_ahn_item_state), and the item's own two weight arrays, which no pair changes."""
    Ks: torch.Tensor            # [I, Ri * Si, F] (all-sentence weights * sentence vectors) @ Ws^T
    Kr: torch.Tensor            # [I, Ri, F] transformed reviews @ Wr^T
    fm: torch.Tensor            # [I, K + 2] the pooled item's and the id embedding's part of the FM
    item_sent_weights: torch.Tensor      # [I, Ri, Si]
    item_review_weights: torch.Tensor    # [I, Ri]


class AhnPairHead(NamedTuple):
    """The parameters the pair tail reads (AHN.pair_head; rbr_ahn_head)."""
    bt: torch.Tensor            # [F]
    VzT: torch.Tensor           # [K, F]
    vz2: torch.Tensor           # [F]
    lz: torch.Tensor            # [F]
    lin_b: torch.Tensor         # [1]


def _ahn_operands(user_state, item_state, head):
    """The four argument structs of the rbr_ahn_pair_score_* entries, the tensors they point into (kept alive by the caller) and
    the shape (Ru, Su, Ri, Si, F, K)."""
    us = [t.detach().contiguous() for t in user_state]
    its = [t.detach().contiguous() for t in item_state[:3]]
    hd = [t.detach().contiguous().view(-1) if k != 1 else t.detach().contiguous() for k, t in enumerate(head)]
    X, Xt, sm, rm, ufm = us
    Ks, Kr, ifm = its
    for t, name in ((X, "user_state.X"), (Xt, "user_state.Xt"), (ufm, "user_state.fm"), (Ks, "item_state.Ks"), (Kr, "item_state.Kr"),
                    (ifm, "item_state.fm"), *zip(hd, ("head.bt", "head.VzT", "head.vz2", "head.lz", "head.lin_b"))):
        dev_ptr(t, F32, name)               # device gate first: a CPU tensor is refused before anything else is looked at
    if X.dim() != 3 or sm.dim() != 3 or Ks.dim() != 3 or Kr.dim() != 3 or item_state[3].dim() != 3:
        raise RuntimeError("AHN states must be X [U, Ru*Su, F], sent_masks [U, Ru, Su], Ks [I, Ri*Si, F], Kr [I, Ri, F], "
                           "item_sent_weights [I, Ri, Si]")
    U, NU, F_ = X.shape
    _, Ru, Su = sm.shape
    I, NJ, _ = Ks.shape
    Ri, Si = item_state[3].shape[1:]
    K = ufm.shape[1] - 2
    want = {"Xt": (Xt, (U, NU, F_)), "sent_masks": (sm, (U, Ru, Su)), "rev_masks": (rm, (U, Ru)), "user fm": (ufm, (U, K + 2)),
            "Ks": (Ks, (I, NJ, F_)), "Kr": (Kr, (I, Ri, F_)), "item fm": (ifm, (I, K + 2)), "bt": (hd[0], (F_,)), "VzT": (hd[1], (K, F_)),
            "vz2": (hd[2], (F_,)), "lz": (hd[3], (F_,)), "lin_b": (hd[4], (1,))}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise RuntimeError(f"AHN pair score: {name} must be {shape}, got {tuple(t.shape)}")
    if NU != Ru * Su or NJ != Ri * Si or K < 1:
        raise RuntimeError(f"AHN pair score: {NU} user / {NJ} item sentence rows do not match {Ru} x {Su} / {Ri} x {Si}, or K = {K} < 1")
    sm8, rm8 = _mask_u8(sm), _mask_u8(rm)
    keep = (us, its, hd, sm8, rm8)
    shape = _lib.AhnShape(Ru, Su, Ri, Si, F_, K)
    c_user = _lib.AhnUserState(X.data_ptr(), Xt.data_ptr(), dev_ptr(sm8, U8, "sent_masks"), dev_ptr(rm8, U8, "rev_masks"),
                               ufm.data_ptr(), U)
    c_item = _lib.AhnItemState(Ks.data_ptr(), Kr.data_ptr(), ifm.data_ptr(), I)
    c_head = _lib.AhnHead(*(t.data_ptr() for t in hd))
    return shape, c_user, c_item, c_head, keep


def _ahn_rows(rows, name):
    rows = rows.contiguous()
    if rows.dim() != 1 or rows.dtype not in (I32, I64):
        raise RuntimeError(f"{name} must be a 1-D int32 or int64 tensor, got {rows.dtype} {tuple(rows.shape)}")
    return rows, dev_ptr(rows, rows.dtype, name), 64 if rows.dtype == I64 else 32


def ahn_pair_score(user_state, item_state, head, u_rows, i_rows, *, weights=False):
    """AHN's eval-mode scores [P] of the pairs (u_rows[p], i_rows[p]) -- row indices, int32 or int64, into the state tables of
    AHN.encode_users / encode_items -- in ONE launch (rbr_ahn_pair_score_ids): the encoder is not run, the tables are.  With
    weights=True: (scores, user_sent_weights [P, Ru, Su], user_review_weights [P, Ru]); the item's two weight arrays are per id
    (item_state.item_sent_weights / item_review_weights).  No autograd, no host synchronisation.  A row outside its table scores as
    row 0 and is recorded like sanitize_ids() records it (check_id_errors)."""
    shape, c_user, c_item, c_head, keep = _ahn_operands(user_state, item_state, head)
    dev = keep[0][0].device
    u_rows, pu, bits = _ahn_rows(u_rows, "u_rows")
    i_rows, pi, bits_i = _ahn_rows(i_rows, "i_rows")
    if u_rows.shape != i_rows.shape or bits != bits_i:
        raise RuntimeError(f"u_rows / i_rows must be [P] each of one dtype, got {tuple(u_rows.shape)} {u_rows.dtype} / "
                           f"{tuple(i_rows.shape)} {i_rows.dtype}")
    P = u_rows.shape[0]
    out = torch.empty(P, dtype=F32, device=dev)
    w = torch.empty(P, shape.Ru, shape.Su, dtype=F32, device=dev) if weights else None
    v = torch.empty(P, shape.Ru, dtype=F32, device=dev) if weights else None
    if P:
        _call("ahn_pair_score_ids", _lib.lib().rbr_ahn_pair_score_ids, C.byref(shape), C.byref(c_user), C.byref(c_item), C.byref(c_head),
              P, pu, pi, bits, dev_ptr(out, F32, "out"), dev_ptr(w, F32, "w"), dev_ptr(v, F32, "v"), _id_err(dev).data_ptr(),
              current_stream())
    return (out, w, v) if weights else out


def ahn_pair_score_dense(user_state, item_state, head, u_rows=None):
    """AHN's eval-mode scores [len(u_rows), I] of the user rows u_rows (None: every row of user_state) against every item row
    (rbr_ahn_pair_score_dense): the same arithmetic, bit for bit, as ahn_pair_score.  No autograd, no host synchronisation."""
    shape, c_user, c_item, c_head, keep = _ahn_operands(user_state, item_state, head)
    dev = keep[0][0].device
    if u_rows is None:
        Nu, pu, bits = c_user.rows, None, 64
    else:
        u_rows, pu, bits = _ahn_rows(u_rows, "u_rows")
        Nu = u_rows.shape[0]
    out = torch.empty(Nu, c_item.rows, dtype=F32, device=dev)
    if out.numel():
        _call("ahn_pair_score_dense", _lib.lib().rbr_ahn_pair_score_dense, C.byref(shape), C.byref(c_user), C.byref(c_item),
              C.byref(c_head), Nu, pu, bits, dev_ptr(out, F32, "out"), _id_err(dev).data_ptr(), current_stream())
    return out


class AhnExplainRows(NamedTuple):
    """What ahn_pair_explain reads beyond the score's operands (rbr_ahn_explain_rows): the item's own path into the FM.  Its
    review weights beta are item_state.item_review_weights."""
    Rp: torch.Tensor            # [I, Ri, F] r': the items' transformed reviews (AHN.item_reviews)
    VqT: torch.Tensor           # [K, F] block 2 of fm.V, transposed (AHN.explain_head)
    vq2: torch.Tensor           # [F]
    lq: torch.Tensor            # [F]


class AhnPairExplanation(NamedTuple):
    """ahn_pair_explain's outputs for P pairs (include/rbr_hip.h has the formulas)."""
    score: torch.Tensor                   # [P] ahn_pair_score's bits
    user_sent_weights: torch.Tensor       # [P, Ru, Su] w
    user_review_weights: torch.Tensor     # [P, Ru] v
    user_match: torch.Tensor              # int32 [P, Ru, Su] js: the item sentence ri * Si + si each user sentence matched
    review_match: torch.Tensor            # int32 [P, Ru] jr: the item review each user review matched
    user_sentences: torch.Tensor          # [P, Ru, Su] gradient x input of every sentence vector, through both attentions
    user_sentences_fixed: torch.Tensor    # [P, Ru, Su] the part with both attention weightings held constant
    user_reviews: torch.Tensor            # [P, Ru]; sums to user_text
    user_text: torch.Tensor               # [P]
    item_sentence_match: torch.Tensor     # [P, Ri, Si] what an item sentence adds as the match of user sentences
    item_review_match: torch.Tensor       # [P, Ri]
    item_reviews: torch.Tensor            # [P, Ri] the item's own path, its weights held constant; sums to item_text
    item_text: torch.Tensor               # [P]


def ahn_pair_explain(user_state, item_state, head, extra, u_rows, i_rows) -> AhnPairExplanation:
    """Why the pairs (u_rows[p], i_rows[p]) of ahn_pair_score scored as they did, in ONE launch (rbr_ahn_pair_explain_ids,
    csrc/ahn_explain.hip): the score and the user's two weight arrays with ahn_pair_score's bits, the max routing with
    ahn_pair_attend's, and what every user sentence, user review, matched item sentence / review and item review adds to the
    score.  `extra`: an AhnExplainRows.  No autograd, no host synchronisation, no [P, rows, F] gradient.  A row outside its table
    is explained as row 0 and recorded like sanitize_ids() records it (check_id_errors)."""
    shape, c_user, c_item, c_head, keep = _ahn_operands(user_state, item_state, head)
    dev = keep[0][0].device
    Ru, Su, Ri, Si, F_, K = shape.Ru, shape.Su, shape.Ri, shape.Si, shape.F, shape.K
    beta = item_state[4].detach().contiguous()
    ex = [t.detach().contiguous() for t in extra]
    want = {"extra.Rp": (ex[0], (c_item.rows, Ri, F_)), "extra.VqT": (ex[1], (K, F_)), "extra.vq2": (ex[2], (F_,)),
            "extra.lq": (ex[3], (F_,)), "item_review_weights": (beta, (c_item.rows, Ri))}
    for name, (t, shp) in want.items():
        dev_ptr(t, F32, name)
        if tuple(t.shape) != shp:
            raise RuntimeError(f"AHN pair explain: {name} must be {shp}, got {tuple(t.shape)}")
    u_rows, pu, bits = _ahn_rows(u_rows, "u_rows")
    i_rows, pi, bits_i = _ahn_rows(i_rows, "i_rows")
    if u_rows.shape != i_rows.shape or bits != bits_i:
        raise RuntimeError(f"u_rows / i_rows must be [P] each of one dtype, got {tuple(u_rows.shape)} {u_rows.dtype} / "
                           f"{tuple(i_rows.shape)} {i_rows.dtype}")
    P = u_rows.shape[0]
    f32 = lambda *s: torch.empty(P, *s, dtype=F32, device=dev)          # noqa: E731
    i32 = lambda *s: torch.empty(P, *s, dtype=I32, device=dev)          # noqa: E731
    res = AhnPairExplanation(f32(), f32(Ru, Su), f32(Ru), i32(Ru, Su), i32(Ru), f32(Ru, Su), f32(Ru, Su), f32(Ru), f32(), f32(Ri, Si),
                             f32(Ri), f32(Ri), f32())
    if P:
        c_extra = _lib.AhnExplainRows(ex[0].data_ptr(), beta.data_ptr(), ex[1].data_ptr(), ex[2].data_ptr(), ex[3].data_ptr())
        c_out = _lib.AhnExplainOut(*(dev_ptr(t, t.dtype, n) for n, t in zip(_lib.AHN_EXPLAIN_OUT, res)))
        _call("ahn_pair_explain_ids", _lib.lib().rbr_ahn_pair_explain_ids, C.byref(shape), C.byref(c_user), C.byref(c_item),
              C.byref(c_head), C.byref(c_extra), P, pu, pi, bits, C.byref(c_out), _id_err(dev).data_ptr(), current_stream())
    return res


class _AhnPairAttend(torch.autograd.Function):
    """rbr_ahn_pair_attend_fwd / rbr_ahn_pair_attend_bwd of rbr_hip.h: (z, w, v, js, jr), all but z non-differentiable."""

    @staticmethod
    def forward(ctx, X, Xt, sent_masks, rev_masks, Ks, Kr, bt, groups):
        X, Xt, Ks, Kr, bt = (t.detach().contiguous() for t in (X, Xt, Ks, Kr, bt))
        for t, name in ((X, "X"), (Xt, "Xt"), (Ks, "Ks"), (Kr, "Kr"), (bt, "bt")):
            dev_ptr(t, F32, name)               # device gate first: a CPU tensor is refused before anything else is looked at
        G = int(groups)
        if X.dim() != 3 or sent_masks.dim() != 3 or Ks.dim() != 3 or Kr.dim() != 3 or G < 1:
            raise RuntimeError("ahn_pair_attend: X [B, Ru*Su, F], sent_masks [B, Ru, Su], Ks [G*B, Ri*Si, F], Kr [G*B, Ri, F], "
                               f"groups >= 1; got {tuple(X.shape)}, {tuple(sent_masks.shape)}, {tuple(Ks.shape)}, {tuple(Kr.shape)}, {G}")
        B, NU, F_ = X.shape
        _, Ru, Su = sent_masks.shape
        P, NJ, _ = Ks.shape
        Ri = Kr.shape[1]
        want = {"Xt": (Xt, (B, NU, F_)), "sent_masks": (sent_masks, (B, Ru, Su)), "rev_masks": (rev_masks, (B, Ru)),
                "Ks": (Ks, (G * B, NJ, F_)), "Kr": (Kr, (G * B, Ri, F_)), "bt": (bt, (F_,))}
        for name, (t, shape) in want.items():
            if tuple(t.shape) != shape:
                raise RuntimeError(f"ahn_pair_attend: {name} must be {shape}, got {tuple(t.shape)}")
        if NU != Ru * Su or Ri < 1 or NJ % max(Ri, 1):
            raise RuntimeError(f"ahn_pair_attend: {NU} user / {NJ} item sentence rows do not match {Ru} x {Su} / {Ri} reviews")
        sm8, rm8 = _mask_u8(sent_masks), _mask_u8(rev_masks)
        dev = X.device
        shape = _lib.AhnShape(Ru, Su, Ri, NJ // Ri, F_, 1)
        z = torch.empty(P, F_, dtype=F32, device=dev)
        w = torch.empty(P, Ru, Su, dtype=F32, device=dev)
        v = torch.empty(P, Ru, dtype=F32, device=dev)
        js = torch.empty(P, NU, dtype=I32, device=dev)
        jr = torch.empty(P, Ru, dtype=I32, device=dev)
        p = torch.empty(P, Ru, F_, dtype=F32, device=dev)
        if P:
            _call("ahn_pair_attend_fwd", _lib.lib().rbr_ahn_pair_attend_fwd, C.byref(shape), B, G, dev_ptr(X, F32, "X"),
                  dev_ptr(Xt, F32, "Xt"), dev_ptr(sm8, U8, "sent_masks"), dev_ptr(rm8, U8, "rev_masks"), dev_ptr(Ks, F32, "Ks"),
                  dev_ptr(Kr, F32, "Kr"), dev_ptr(bt, F32, "bt"), dev_ptr(z, F32, "z"), dev_ptr(w, F32, "w"), dev_ptr(v, F32, "v"),
                  dev_ptr(js, I32, "js"), dev_ptr(jr, I32, "jr"), dev_ptr(p, F32, "p"), current_stream())
        ctx.job = (shape, B, G)
        ctx.save_for_backward(X, Xt, sm8, rm8, Ks, Kr, w, v, js, jr, p)
        ctx.mark_non_differentiable(w, v, js, jr)
        return z, w, v, js, jr

    @staticmethod
    def backward(ctx, dz, dw=None, dv=None, djs=None, djr=None):
        shape, B, G = ctx.job
        X, Xt, sm8, rm8, Ks, Kr, w, v, js, jr, p = ctx.saved_tensors
        dz = dz.contiguous()
        dX, dXt, dKs, dKr = torch.empty_like(X), torch.empty_like(Xt), torch.empty_like(Ks), torch.empty_like(Kr)
        dbt_part = torch.empty(B, shape.F, dtype=F32, device=X.device)
        if B:
            _call("ahn_pair_attend_bwd", _lib.lib().rbr_ahn_pair_attend_bwd, C.byref(shape), B, G, dev_ptr(X, F32, "X"),
                  dev_ptr(Xt, F32, "Xt"), dev_ptr(sm8, U8, "sent_masks"), dev_ptr(rm8, U8, "rev_masks"), dev_ptr(Ks, F32, "Ks"),
                  dev_ptr(Kr, F32, "Kr"), dev_ptr(w, F32, "w"), dev_ptr(v, F32, "v"), dev_ptr(js, I32, "js"), dev_ptr(jr, I32, "jr"),
                  dev_ptr(p, F32, "p"), dev_ptr(dz, F32, "dz"), dev_ptr(dX, F32, "dX"), dev_ptr(dXt, F32, "dXt"),
                  dev_ptr(dKs, F32, "dKs"), dev_ptr(dKr, F32, "dKr"), dev_ptr(dbt_part, F32, "dbt_part"), current_stream())
        return dX, dXt, None, None, dKs, dKr, dbt_part.sum(0), None


def ahn_pair_attend(X, Xt, sent_masks, rev_masks, Ks, Kr, bt, *, groups: int = 1, saved: bool = False):
    """AHN's user-side co-attention as one differentiable op (csrc/ahn_attend.hip; steps 1-4 of ahn_pair_score with a HIP
    backward).  Grouped layout: G = `groups` = 1 + n_neg groups of B pairs; pair p = g * B + b reads USER row b of X, Xt
    [B, Ru*Su, F] (sentence vectors and X @ Wt^T), sent_masks [B, Ru, Su], rev_masks [B, Ru] and ITEM row p of Ks [G*B, Ri*Si, F],
    Kr [G*B, Ri, F]; bt [F] is user_review_trans_layer's bias.  Returns (z [G*B, F], user_sent_weights [G*B, Ru, Su],
    user_review_weights [G*B, Ru]): z carries gradients to X, Xt, Ks, Kr and bt, the weights are non-differentiable and have
    ahn_pair_score's bits.  Each max routes its gradient to the lowest-index row that attained it, where torch.max on a tie
    picks an unspecified one.  No float atomics; the same inputs give the same bits, forward and backward, on every run.
    saved=True also returns the routing (js int32 [G*B, Ru*Su], jr int32 [G*B, Ru]) -- for tests."""
    z, w, v, js, jr = _AhnPairAttend.apply(X, Xt, sent_masks, rev_masks, Ks, Kr, bt, int(groups))
    return (z, w, v, js, jr) if saved else (z, w, v)


# --------------------------------------------------------------------------- bidirectional LSTM over padded sequences
LSTM_MAX_LEN = 1000      # the reference clamps sequence lengths there (models/ahn/ahn_layers.py:307)


def lstm_t_out(lengths: torch.Tensor, T: int) -> torch.Tensor:
    """The batch's output length max(clamp(lengths, 1, 1000)) as a DEVICE int32 [1] (no host synchronisation): what
    pad_packed_sequence trims the reference's output to (ahn_layers.py:307-311)."""
    return lengths.clamp(1, min(int(T), LSTM_MAX_LEN)).max().to(I32).view(1)


def _lstm_seq_fwd(xproj, w_f, w_r, lengths, t_out, pool):
    """The checks and the one rbr_lstm_seq_fwd call shared by _LstmSeq.forward and lstm_seq_states -> (out, pooled, argmax, saved,
    and the contiguous w_f, w_r, lengths the call read)."""
    if xproj.dim() != 3 or xproj.shape[2] % 8:
        raise RuntimeError(f"lstm_seq: xproj must be [N, T, 8 * Hh], got {tuple(xproj.shape)}")
    N, T, H8 = xproj.shape
    Hh = H8 // 8
    if tuple(w_f.shape) != (4 * Hh, Hh) or tuple(w_r.shape) != (4 * Hh, Hh):
        raise RuntimeError(f"lstm_seq: w_hh must be [{4 * Hh}, {Hh}] for both directions")
    if lengths.dtype != I64 or lengths.numel() != N:
        raise RuntimeError("lstm_seq: lengths must be int64 [N]")
    L_ = _lib.lib()
    dev = xproj.device
    xproj, w_f, w_r, lengths = xproj.contiguous(), w_f.contiguous(), w_r.contiguous(), lengths.contiguous().view(-1)
    per_seq = 0
    if pool:
        if t_out is None:
            t_out = lstm_t_out(lengths, T)
        t_out = t_out.contiguous().view(-1)
        if t_out.numel() not in (1, N):
            raise RuntimeError("lstm_seq: t_out must hold one value, or one per sequence")
        per_seq = int(t_out.numel() == N and N > 1)
    saved = torch.empty(L_.rbr_lstm_seq_ws_bytes(N, T, Hh), dtype=U8, device=dev)
    out = pooled = argmax = None
    if pool:
        pooled = torch.empty(N, 2 * Hh, dtype=F32, device=dev)
        argmax = torch.empty(N, 2 * Hh, dtype=I32, device=dev)
    else:
        out = torch.empty(N, T, 2 * Hh, dtype=F32, device=dev)
    _call("lstm_seq_fwd", L_.rbr_lstm_seq_fwd, N, T, Hh, dev_ptr(xproj, F32, "xproj"), dev_ptr(w_f, F32, "w_hh_fwd"),
          dev_ptr(w_r, F32, "w_hh_rev"), dev_ptr(lengths, I64, "lengths"), dev_ptr(t_out if pool else None, I32, "t_out"), per_seq,
          dev_ptr(out, F32, "out"), dev_ptr(pooled, F32, "pooled"), dev_ptr(argmax, I32, "argmax"),
          saved.data_ptr() if saved.numel() else None, current_stream())
    return out, pooled, argmax, saved, w_f, w_r, lengths


class _LstmSeq(torch.autograd.Function):
    """rbr_lstm_seq_fwd / rbr_lstm_seq_bwd of rbr_hip.h: the recurrence over xproj, returning out [N, T, 2 Hh] or the fused
    (pooled [N, 2 Hh], argmax int32 [N, 2 Hh])."""

    @staticmethod
    def forward(ctx, xproj, w_f, w_r, lengths, t_out, pool):
        out, pooled, argmax, saved, w_f, w_r, lengths = _lstm_seq_fwd(xproj, w_f, w_r, lengths, t_out, pool)
        N, T, H8 = xproj.shape
        ctx.job = (N, T, H8 // 8, bool(pool))
        ctx.save_for_backward(w_f, w_r, lengths, saved, *([argmax] if pool else []))
        if pool:
            ctx.mark_non_differentiable(argmax)
            return pooled, argmax
        return out

    @staticmethod
    def backward(ctx, d_a, d_argmax=None):
        N, T, Hh, pool = ctx.job
        w_f, w_r, lengths, saved = ctx.saved_tensors[:4]
        argmax = ctx.saved_tensors[4] if pool else None
        L_ = _lib.lib()
        dev = w_f.device
        d_a = d_a.contiguous()
        d_xproj = torch.empty(N, T, 8 * Hh, dtype=F32, device=dev)
        dwf, dwr = torch.empty_like(w_f), torch.empty_like(w_r)
        ws = torch.empty(L_.rbr_lstm_seq_bwd_ws_bytes(N, T, Hh), dtype=U8, device=dev)
        _call("lstm_seq_bwd", L_.rbr_lstm_seq_bwd, N, T, Hh, dev_ptr(w_f, F32, "w_hh_fwd"), dev_ptr(w_r, F32, "w_hh_rev"),
              dev_ptr(lengths, I64, "lengths"), saved.data_ptr() if saved.numel() else None,
              None if pool else dev_ptr(d_a, F32, "d_out"), dev_ptr(d_a, F32, "d_pooled") if pool else None,
              dev_ptr(argmax, I32, "argmax"), dev_ptr(d_xproj, F32, "d_xproj"), dev_ptr(dwf, F32, "d_w_hh_fwd"),
              dev_ptr(dwr, F32, "d_w_hh_rev"), ws.data_ptr() if ws.numel() else None, current_stream())
        return d_xproj, dwf, dwr, None, None, None


def lstm_seq(xproj, w_hh_fwd, w_hh_rev, lengths, *, pool: bool, t_out=None):
    """One-layer bidirectional LSTM recurrence over N padded sequences (torch.nn.LSTM's arithmetic on packed sequences; HIP
    forward and backward).  xproj [N, T, 8 Hh] = x W_ih^T + b_ih + b_hh of both directions (forward direction's gates first),
    w_hh_* [4 Hh, Hh], lengths int64 [N].  pool False: out [N, T, 2 Hh] with zeros behind each sequence's end and in empty
    rows.  pool True: (pooled [N, 2 Hh], argmax int32 [N, 2 Hh]) = the max over the steps of the output trimmed to `t_out` and
    zero-padded (AHN's torch.max(words, dim=1)); t_out: device int32, one value or one per sequence, default
    max(clamp(lengths, 1, 1000)) computed on the device -- no host synchronisation on this path."""
    return _LstmSeq.apply(xproj, w_hh_fwd, w_hh_rev, lengths, t_out, bool(pool))


def bilstm_encode(x, lstm_params, lengths, *, pool: bool, t_out=None):
    """x [N, T, E] through a bidirectional nn.LSTM layer given by lstm_params = (weight_ih_l0, weight_hh_l0, bias_ih_l0,
    bias_hh_l0, weight_ih_l0_reverse, weight_hh_l0_reverse, bias_ih_l0_reverse, bias_hh_l0_reverse).  The input projection of both
    directions is ONE product over [N * T, E] on the MFMA `linear` (the two W_ih stacked, b_ih + b_hh added once), whose own
    backward gives dW_ih, the bias gradients and dx; the recurrence is lstm_seq."""
    w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r = lstm_params
    N, T, E = x.shape
    W = torch.cat([w_ih_f, w_ih_r], dim=0)
    b = torch.cat([b_ih_f + b_hh_f, b_ih_r + b_hh_r], dim=0)
    xproj = linear(x.reshape(N * T, E), W, b).view(N, T, W.shape[0])
    return lstm_seq(xproj, w_hh_f, w_hh_r, lengths, pool=pool, t_out=t_out)


class LstmState(NamedTuple):
    """lstm_seq_states' handle: the forward's saved state (gate activations, cell states, the tile order) kept alive outside
    autograd, with the shape it belongs to.  Read by lstm_seq_word_saliency; never modified."""
    saved: torch.Tensor       # uint8 [rbr_lstm_seq_ws_bytes(N, T, Hh)]
    N: int
    T: int
    Hh: int


def lstm_seq_states(xproj, w_hh_fwd, w_hh_rev, lengths, t_out):
    """lstm_seq(..., pool=True, t_out=t_out) outside autograd -> (pooled [N, 2 Hh], argmax int32 [N, 2 Hh], state): the same
    launch, so pooled and argmax have lstm_seq's bits, and `state` keeps what the forward saved for lstm_seq_word_saliency.
    Nothing here is differentiable: the inputs' autograd history is ignored."""
    with torch.no_grad():
        _, pooled, argmax, saved, _, _, _ = _lstm_seq_fwd(xproj.detach(), w_hh_fwd.detach(), w_hh_rev.detach(), lengths, t_out, True)
    N, T, H8 = xproj.shape
    return pooled, argmax, LstmState(saved, N, T, H8 // 8)


def lstm_seq_word_saliency(state: LstmState, xw, w_hh_fwd, w_hh_rev, lengths, d_pooled, argmax) -> torch.Tensor:
    """rbr_lstm_seq_saliency of rbr_hip.h: gradient x input of every step through the recurrence, per direction, from the state of
    lstm_seq_states -> [N, T, 2] f32.  xw [N, T, 8 Hh] is the BIAS-FREE input projection x W_ih^T (xproj's layout), d_pooled
    [N, 2 Hh] the gradient of whatever is explained with respect to `pooled`, argmax the forward's.  out[n, t, d] = sum over
    direction d's four gates and Hh units of d pre-activation * xw = <d / d x_t, x_t> restricted to direction d; exactly 0 at
    t >= len and in empty rows.  No d_xproj, no weight gradient, no workspace; the same inputs give the same bits, and a
    sequence's values do not depend on the batch around it.  w_hh_*, lengths: what the forward was given."""
    N, T, Hh = state.N, state.T, state.Hh
    if tuple(xw.shape) != (N, T, 8 * Hh):
        raise RuntimeError(f"lstm_seq_word_saliency: xw must be [{N}, {T}, {8 * Hh}] like the forward's xproj, got {tuple(xw.shape)}")
    if tuple(w_hh_fwd.shape) != (4 * Hh, Hh) or tuple(w_hh_rev.shape) != (4 * Hh, Hh):
        raise RuntimeError(f"lstm_seq_word_saliency: w_hh must be [{4 * Hh}, {Hh}] for both directions")
    if lengths.dtype != I64 or lengths.numel() != N:
        raise RuntimeError("lstm_seq_word_saliency: lengths must be int64 [N]")
    if tuple(d_pooled.shape) != (N, 2 * Hh) or tuple(argmax.shape) != (N, 2 * Hh):
        raise RuntimeError(f"lstm_seq_word_saliency: d_pooled and argmax must be [{N}, {2 * Hh}]")
    L_ = _lib.lib()
    if state.saved.numel() != L_.rbr_lstm_seq_ws_bytes(N, T, Hh):
        raise RuntimeError("lstm_seq_word_saliency: the state does not belong to this shape")
    xw, d_pooled, argmax = xw.detach().contiguous(), d_pooled.detach().contiguous(), argmax.contiguous()
    w_f, w_r, lengths = w_hh_fwd.detach().contiguous(), w_hh_rev.detach().contiguous(), lengths.contiguous().view(-1)
    # the pointer checks come first: a CPU tensor is refused before anything is allocated on a device
    ptrs = (dev_ptr(w_f, F32, "w_hh_fwd"), dev_ptr(w_r, F32, "w_hh_rev"), dev_ptr(lengths, I64, "lengths"),
            dev_ptr(state.saved, U8, "state") if N else None, dev_ptr(xw, F32, "xw"), dev_ptr(d_pooled, F32, "d_pooled"),
            dev_ptr(argmax, I32, "argmax"))
    words = torch.empty(N, T, 2, dtype=F32, device=xw.device)
    _call("lstm_seq_saliency", L_.rbr_lstm_seq_saliency, N, T, Hh, *ptrs, dev_ptr(words, F32, "words_out"), current_stream())
    return words


def bilstm_encode_states(x, lstm_params, lengths, *, t_out):
    """bilstm_encode(x, lstm_params, lengths, pool=True, t_out=t_out) outside autograd, keeping what the word saliency reads ->
    (xw [N, T, 8 Hh], pooled, argmax, state).  The input projection runs once WITHOUT the bias (xw = x W_ih^T, the saliency's
    second operand) and the recurrence reads xproj = xw + (b_ih + b_hh): the MFMA `linear` adds its bias to the finished sum,
    so pooled has bilstm_encode's bits for the same rows."""
    w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r = (p.detach() for p in lstm_params)
    N, T, E = x.shape
    with torch.no_grad():
        W = torch.cat([w_ih_f, w_ih_r], dim=0)
        b = torch.cat([b_ih_f + b_hh_f, b_ih_r + b_hh_r], dim=0)
        xw = linear(x.detach().reshape(N * T, E), W, None).view(N, T, W.shape[0])
        pooled, argmax, state = lstm_seq_states(xw + b, w_hh_f, w_hh_r, lengths, t_out)
    return xw, pooled, argmax, state


def bilstm_word_saliency(x, lstm_params, lengths, d_pooled_of, *, t_out):
    """Gradient x input of every word of x [N, T, E] through bilstm_encode(x, lstm_params, lengths, pool=True, t_out=t_out), for
    the scalar whose gradient with respect to the pooled vectors the caller supplies: d_pooled_of(pooled [N, 2 Hh]) -> [N, 2 Hh].
    Returns (pooled, argmax, words [N, T, 2]); words.sum(-1)[n, t] = <d scalar / d x[n, t], x[n, t]>: bilstm_encode_states, the
    caller's gradient, lstm_seq_word_saliency.  The biases take no share (they are not part of x W_ih^T)."""
    xw, pooled, argmax, state = bilstm_encode_states(x, lstm_params, lengths, t_out=t_out)
    words = lstm_seq_word_saliency(state, xw, lstm_params[1], lstm_params[5], lengths, d_pooled_of(pooled), argmax)
    return pooled, argmax, words
