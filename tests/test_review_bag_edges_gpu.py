"""SimpleSiamese's bag of embeddings (csrc/review_bag.hip: functional.review_bag) at the shapes where the backward's LDS
bucket code (csrc/lds_bucket.h: windows of 512 token positions, a 2048-slot hash table, output items walked 4 x 256 at a time)
can go wrong, forward and table gradient against the float64 restatement edge_refs.review_bag from the same f32 inputs, for
both backward forms: the default bucket kernel and the sorted-run form (RBR_BAG_BWD=sort).

Tolerances are per element, edge_refs' (n + 4) * EPS * Abs: for out[r, :] n = unmasked positions of review r and Abs = |drop|
* inv_len * sum |table rows|; for dtable[t, :] n = unmasked, non-pad occurrences of token t and Abs = sum |d_out * inv_len *
drop| over them.  An element with no terms (absent tokens, the padding row, fully masked reviews) must be exactly 0.

tests/test_edge_refs_host.py checks the restatement against autograd in float64 and the bounds against an f32 CPU evaluation
of the same cases (CASES below).  Every test prints its largest err / bound per tensor ("RATIO review-bag <tensor> <value>").
"""
import os
import zlib

import pytest
import torch

import edge_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIN, HASH = 512, 2048          # kBagWin, kBagHash of csrc/review_bag.hip


def bucket_of(t):
    """the hash table's home slot of token t"""
    return ((t * 2654435761) % 2 ** 32) >> 21


def colliding_tokens(V, bucket, count):
    toks = [t for t in range(1, V) if bucket_of(t) == bucket][:count]
    assert len(toks) == count and all(bucket_of(t) == bucket for t in toks), (bucket, len(toks))
    return toks


# name -> (n_rev, T, D, V, ids: None (uniform) | "one" | "distinct" | "collide" | ("cycle", k), mask: None | "rand" | "hole",
#          padding_idx, with_drop)
CASES = {
    # n_rev * T at the window edges 1, 511, 512, 513, 1025, over the row widths
    "pos1": (1, 1, 1, 2, None, None, None, False),
    "pos511": (7, 73, 3, 50, None, "rand", 0, True),
    "pos512": (8, 64, 64, 40, None, None, 3, False),
    "pos513": (19, 27, 65, 60, None, "rand", None, True),
    "pos1025": (25, 41, 300, 30, None, "rand", 0, True),
    # one token fills a window (one key, count 512); 512 distinct tokens in a window (512 keys)
    "one-token": (8, 64, 3, 8, "one", None, 0, False),
    "distinct": (8, 64, 3, 600, "distinct", None, 0, True),
    # tokens that share a hash slot, and a cluster in the last slot whose probe wraps to slot 0 (itself occupied)
    "collide": (8, 64, 3, 100003, "collide", "rand", 0, True),
    # a window with every position masked between two live ones
    "hole": (24, 64, 3, 50, None, "hole", 3, True),
    # keys * D around the 4 x 256 items one pass of the output loop takes: 1023, 1024, 1025
    "items1023": (8, 64, 3, 400, ("cycle", 341), None, 0, False),
    "items1024": (8, 64, 64, 400, ("cycle", 16), None, 0, True),
    "items1025": (8, 64, 5, 400, ("cycle", 205), None, 0, False),
}


def inputs(name):
    """One seed per case: table ~ N(0,1), d_out ~ N(0,1), drop = Bernoulli(0.8) / 0.8, mask "rand" keeps 70 % of the positions."""
    n_rev, T, D, V, kind, mkind, pad, with_drop = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    table, d_out = torch.randn(V, D, generator=g), torch.randn(n_rev, D, generator=g)
    n_pos = n_rev * T
    if kind is None:
        ids = torch.randint(0, V, (n_pos,), generator=g)
    elif kind == "one":
        ids = torch.full((n_pos,), 5)
    elif kind == "distinct":
        ids = 1 + torch.randperm(V - 1, generator=g)[:n_pos]
        assert ids.unique().numel() == n_pos == WIN
    elif kind == "collide":
        # 30 tokens of one home slot, 24 of the last slot (23 of them probe on into slots 0, 1, ...), 4 each whose home is slot 0 / 1
        pool = colliding_tokens(V, 777, 30) + colliding_tokens(V, HASH - 1, 24) + colliding_tokens(V, 0, 4) + colliding_tokens(V, 1, 4)
        pool = torch.tensor(pool + [0])                                     # and the padding token
        ids = pool[torch.randint(0, len(pool), (n_pos,), generator=g)]
        ids[:len(pool)] = pool[torch.randperm(len(pool), generator=g)]      # every one of them occurs
    else:
        ids = 1 + torch.arange(n_pos) % kind[1]
        assert ids[:WIN].unique().numel() == kind[1] and kind[1] * D == int(name[5:])
    ids = ids.reshape(n_rev, T)
    mask = None
    if mkind is not None:
        mask = torch.rand(n_rev, T, generator=g) > 0.3
        if mkind == "hole":
            assert T * 8 == WIN
            mask[8:16] = False                                              # positions 512 .. 1023
    drop = (torch.rand(n_rev, D, generator=g) > 0.2).float() / 0.8 if with_drop else None
    if pad is not None and kind in (None, "collide") and name != "pos1":
        assert bool((ids == pad).any())                                     # pad tokens are mixed in
    return table, ids, mask, drop, d_out, pad


def _backward(RF, table, ids, mask, drop, d_out, pad):
    leaf = table.to(DEV).requires_grad_(True)
    out = RF.review_bag(leaf, ids.to(DEV), None if mask is None else mask.to(DEV), drop=None if drop is None else drop.to(DEV),
                        padding_idx=pad)
    (out * d_out.to(DEV)).sum().backward()
    return out.detach(), leaf.grad


@pytest.mark.parametrize("name", list(CASES))
def test_review_bag_edges(name):
    """Largest err / bound seen on an MI355X over the cases: out 0.21, dtable 0.30 (bucket kernel), 0.30 (sorted runs)."""
    from review_based_recommender_amd import functional as RF
    table, ids, mask, drop, d_out, pad = inputs(name)
    ref = R.review_bag(table, ids, mask, drop, d_out, pad)
    out, dt_bucket = _backward(RF, table, ids, mask, drop, d_out, pad)
    os.environ["RBR_BAG_BWD"] = "sort"
    try:
        out2, dt_sort = _backward(RF, table, ids, mask, drop, d_out, pad)
    finally:
        del os.environ["RBR_BAG_BWD"]
    assert torch.equal(out, out2)
    val, ab, n = ref["out"]
    R.check("review-bag", f"{name} out", out, val, R.bound_of(n, ab))
    val, ab, n = ref["dtable"]
    R.check("review-bag", f"{name} dtable", dt_bucket, val, R.bound_of(n, ab))
    R.check("review-bag", f"{name} dtable-sort", dt_sort, val, R.bound_of(n, ab))
