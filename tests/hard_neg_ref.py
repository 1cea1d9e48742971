"""Integer restatement of rbr_sample_hard_negatives (include/rbr_hip.h) in numpy, shared by its host and GPU tests: the
candidates come from tests/bpr_ref.py's draw, the choice from the ordering key restated here from the f32 bit pattern."""
import numpy as np

from bpr_ref import sample_negatives_ref


def sample_hard_negatives_ref(u_ids, i_ids, n_neg, n_cand, n_items, seen, seed, call, item_lo=1, max_tries=16, replace_id=0):
    """(cand int64 [n_neg, B, n_cand], found bool [n_neg, B]) of call number `call`.  Candidate m of negative j of pair b has draw
    index (b * n_neg + j) * n_cand + m = b * (n_neg * n_cand) + (j * n_cand + m): the uniform sampler's negative j * n_cand + m
    of pair b when it draws n_neg * n_cand of them.  Where a user has no acceptable item every candidate is replace_id."""
    B = len(u_ids)
    _, i_out, valid = sample_negatives_ref(u_ids, i_ids, n_neg * n_cand, n_items, seen, seed, call, item_lo=item_lo,
                                           max_tries=max_tries, replace_id=replace_id)
    cand = i_out[B:].reshape(n_neg, n_cand, B).transpose(0, 2, 1)
    found = valid.reshape(n_neg, n_cand, B).transpose(0, 2, 1) == 1.0
    assert (found == found[:, :, :1]).all()          # acceptability depends on (user, positive) alone
    return np.ascontiguousarray(cand), np.ascontiguousarray(found[:, :, 0])


def score_key(scores, items):
    """uint64 key of (f32 score, item): 0 for NaN, else (order-preserving bits of the score) << 32 | (2^32 - 1 - item) -- larger
    is score descending, then item ascending."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    bits = s.view(np.uint32).astype(np.uint64)
    full = np.uint64(0xFFFFFFFF)
    ordered = np.where((bits >> np.uint64(31)) != 0, ~bits & full, bits | np.uint64(0x80000000))
    key = (ordered << np.uint64(32)) | (full - np.asarray(items).astype(np.uint64))
    return np.where(np.isnan(s), np.uint64(0), key)


def choose(cand, scores):
    """The chosen item [n_neg, B] of candidates / scores [n_neg, B, n_cand]: the largest key, candidate 0 where every key is 0."""
    m = np.argmax(score_key(scores, cand), axis=-1)          # the first maximum: 0 where all keys are 0
    return np.take_along_axis(np.asarray(cand), m[..., None], axis=-1)[..., 0]


def expected_outputs(u_ids, i_ids, cand, found, scores):
    """(u_out, i_out int64 [(1 + n_neg) * B], valid f32 [n_neg * B]) the entry must write for these candidates and scores."""
    u_ids, i_ids = np.asarray(u_ids, dtype=np.int64), np.asarray(i_ids, dtype=np.int64)
    n_neg = cand.shape[0]
    u_out = np.tile(u_ids, 1 + n_neg)
    i_out = np.concatenate([i_ids, choose(cand, scores).reshape(-1)])
    return u_out, i_out, found.reshape(-1).astype(np.float32)
