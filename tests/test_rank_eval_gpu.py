"""Exact held-out ranks on the GPU (rbr_pair_score_rank through functional.pair_score_rank, Recommender.rank / evaluate, the CLI's
--eval-split, the trainer's rank_metrics key).

Yardstick: pair_score_dense, whose scores carry the bits of every other pair_score entry by construction.  They are turned into the
kernel's order (score descending, then the lower item id) on the CPU from their bit patterns, and the candidates that come before
the target are counted there.  Ranks are integers: every comparison is torch.equal, there is no tolerance anywhere."""
import json
import os
import re

import numpy as np
import pytest
import torch

import make_dataset
import synth
from helpers import quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ yardstick
def _tables(B, Ni, K, seed, biases=True, dup=0):
    """Random user rows [B, K] and item table [Ni, K] (+ head); `dup` item rows are copies of other rows: bit-equal scores."""
    gen = torch.Generator().manual_seed(seed)
    ul, il = torch.randn(B, K, generator=gen), torch.randn(Ni, K, generator=gen)
    h, g = torch.randn(K, 1, generator=gen), torch.randn(1, generator=gen)
    ub, ib = torch.randn(B, 1, generator=gen), torch.randn(Ni, 1, generator=gen)
    if dup:
        dst, src = torch.randint(0, Ni, (dup,), generator=gen), torch.randint(0, Ni, (dup,), generator=gen)
        il[dst], ib[dst] = il[src].clone(), ib[src].clone()
    return (ul, il, h, g, ub, ib) if biases else (ul, il, h, g, None, None)


def _to_dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _order_bits(dense):
    """Order-preserving integer of every float (larger = better), the upper half of the kernel's key."""
    b = dense.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def _lists(exclude, B):
    """The exclusion argument (CSR pair, or triple with a row map) as one python list of item ids per pair."""
    if exclude is None:
        return [[] for _ in range(B)]
    off, items = exclude[0].cpu().tolist(), exclude[1].cpu().tolist()
    rows = exclude[2].cpu().tolist() if len(exclude) > 2 else list(range(B))
    return [items[off[r]:off[r + 1]] if 0 <= r < len(off) - 1 else [] for r in rows]


def _yardstick(dense, targets, item_lo, exclude=None):
    """(rank, n_cand) int32 [B] from the dense scores [B, Ni], by the definition of include/rbr_hip.h."""
    dense, targets = dense.cpu(), targets.cpu()
    B, Ni = dense.shape
    ids = torch.arange(Ni)
    in_table = (targets >= 0) & (targets < Ni)
    t = targets.clamp(0, Ni - 1)
    excl = torch.zeros(B, Ni, dtype=torch.bool)
    for b, row in enumerate(_lists(exclude, B)):
        row = [j for j in row if 0 <= j < Ni]
        excl[b, row] = True
    excl[in_table, t[in_table]] = False                          # the target is never excluded
    cand = (ids[None, :] >= item_lo) & ~torch.isnan(dense) & ~excl
    ob = _order_bits(dense)
    ob_t = ob.gather(1, t[:, None])
    before = cand & ((ob > ob_t) | ((ob == ob_t) & (ids[None, :] < t[:, None])))
    ranked = in_table & (t >= item_lo) & ~torch.isnan(dense.gather(1, t[:, None])[:, 0])
    rank = torch.where(ranked, before.sum(1), torch.full((B,), -1))
    return rank.to(torch.int32), cand.sum(1).to(torch.int32)


def _assert_ranks(got, want, what):
    (gr, gc), (wr, wc) = got, want
    assert gr.dtype == torch.int32 and gc.dtype == torch.int32 and gr.shape == wr.shape and gc.shape == wc.shape, what
    gr, gc = gr.cpu(), gc.cpu()
    bad = (gr != wr) | (gc != wc)
    assert torch.equal(gr, wr) and torch.equal(gc, wc), (
        f"{what}: {int(bad.sum())} of {gr.numel()} pairs differ, first pair {int(bad.nonzero()[0])}: "
        f"rank {int(gr[bad][0])} vs {int(wr[bad][0])}, n_cand {int(gc[bad][0])} vs {int(wc[bad][0])}")


def _random_csr(B, Ni, gen, max_per_row, avoid=None):
    """Per-pair lists, sorted within a row, some empty; `avoid` [B]: an item each row must not hold."""
    off, items = [0], []
    for b in range(B):
        n = int(torch.randint(0, min(max_per_row, Ni) + 1, (1,), generator=gen))
        row = torch.randperm(Ni, generator=gen)[:n]
        if avoid is not None:
            row = row[row != int(avoid[b])]
        items.append(row.sort().values)
        off.append(off[-1] + row.numel())
    return torch.tensor(off, dtype=torch.int64), torch.cat(items).to(torch.int32)


def _targets(B, Ni, gen):
    """Random targets; the corners of the table are among them when there is room."""
    t = torch.randint(0, Ni, (B,), generator=gen)
    for b, v in zip(range(B), (0, Ni - 1, 1)):
        t[b] = v
    return t


MODES = (("fm", True), ("fm", False), ("dot", False))


def _check_shape(K, B, Ni, seed, dup=0, max_per_row=6):
    """All three score modes x item_lo 0 / 1, each without and with a per-pair exclusion list (which may name the target)."""
    from review_based_recommender_amd import functional as RF
    gen = torch.Generator().manual_seed(seed)
    tgt = _targets(B, Ni, gen)
    off, items = _random_csr(B, Ni, gen, max_per_row)
    excl = (off.to(DEV), items.to(DEV))
    for mode, biases in MODES:
        ul, il, h, g, ub, ib = _to_dev(*_tables(B, Ni, K, seed, biases, dup))
        dense = RF.pair_score_dense(mode, ul, il, h, g, ub, ib)
        for item_lo in (0, 1):
            for e in (None, excl):
                got = RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=item_lo, exclude=e)
                _assert_ranks(got, _yardstick(dense, tgt, item_lo, e),
                              f"K={K} B={B} Ni={Ni} {mode} biases={biases} item_lo={item_lo} exclusion={e is not None}")
    RF.check_id_errors(DEV)


# ------------------------------------------------------------------------------------------------ exact ranks
@pytest.mark.parametrize("Ni", [2, 65, 1003])      # a partial 64-item step, two steps, several slices
@pytest.mark.parametrize("B", [1, 9, 257])         # the tile of 8 pairs: a single pair, one pair past a tile, many tiles and a tail
@pytest.mark.parametrize("K", [4, 8, 50])          # vector path, the 8-chunk, 32 + 8 + 8 + 2 scalar tail without the float4 path
def test_ranks_and_candidate_counts_are_exact(K, B, Ni):
    _check_shape(K, B, Ni, seed=K * 1000 + B * 7 + Ni, dup=Ni // 5)


def test_ranks_are_exact_over_many_slices_17_by_20011():
    _check_shape(8, 17, 20011, seed=5, dup=2000, max_per_row=40)


@pytest.mark.parametrize("k", [10, 128])
def test_rank_is_the_position_in_the_topk_list(k):
    """rank < k: the target sits at that position of the pair's topk row; otherwise it is not in the row.  With exclusion the lists
    do not name the target (topk would drop it, rank never does); targets below item_lo are unranked and absent."""
    from review_based_recommender_amd import functional as RF
    B, Ni, K = 257, 1003, 32
    gen = torch.Generator().manual_seed(k)
    ul, il, h, g, ub, ib = _to_dev(*_tables(B, Ni, K, seed=40 + k, dup=200))
    # half of the targets from each pair's own head of the ranking, so that both sides of `rank < k` are well populated
    head = RF.pair_score_topk("fm", ul, il, 128, h, g, ub, ib, item_lo=1)[0].cpu()
    tgt = torch.where(torch.rand(B, generator=gen) < 0.5, head[torch.arange(B), torch.randint(0, 128, (B,), generator=gen)],
                      torch.randint(0, Ni, (B,), generator=gen))
    off, items = _random_csr(B, Ni, gen, 40, avoid=tgt)
    for excl in (None, (off.to(DEV), items.to(DEV))):
        rank = RF.pair_score_rank("fm", ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=1, exclude=excl)[0].cpu().long()
        top = RF.pair_score_topk("fm", ul, il, k, h, g, ub, ib, item_lo=1, exclude=excl)[0].cpu()
        inside = (rank >= 0) & (rank < k)
        assert 0 < int(inside.sum()) < B
        assert torch.equal(top[inside].gather(1, rank[inside, None])[:, 0], tgt[inside])
        assert not bool((top[~inside] == tgt[~inside, None]).any())
    RF.check_id_errors(DEV)


# ------------------------------------------------------------------------------------------------ exclusion
def test_exclusion_lists_subtract_exactly():
    """A CSR over ids served through a row map: a list that names the target (still ranked), one with items below item_lo, one
    with an item twice in a row, an empty one, one with everything but the target and one with everything (rank 0 of 1 candidate
    either way), a row outside the CSR (no list); then the same lists as a plain [B + 1] CSR."""
    from review_based_recommender_amd import functional as RF
    Ni, K, item_lo = 70, 8, 2
    tgt = torch.tensor([10, 20, 30, 40, 50, 60, 69, 5])
    every = list(range(Ni))
    by_id = [[3, 10, 11, 64], [0, 1, 2, 7], [5, 5, 9, 9, 9, 66], [], [j for j in every if j != 50], every, [68]]
    off = torch.tensor(np.cumsum([0] + [len(r) for r in by_id]), dtype=torch.int64)
    items = torch.tensor([j for r in by_id for j in r], dtype=torch.int32)
    rows = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7])                 # pair 7 points past the CSR's 7 rows: nothing is excluded
    for mode, biases in MODES:
        ul, il, h, g, ub, ib = _to_dev(*_tables(8, Ni, K, seed=9, biases=biases, dup=20))
        dense = RF.pair_score_dense(mode, ul, il, h, g, ub, ib)
        mapped = (off.to(DEV), items.to(DEV), rows.to(DEV))
        got = RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=item_lo, exclude=mapped)
        _assert_ranks(got, _yardstick(dense, tgt, item_lo, mapped), f"{mode}: mapped CSR")
        rank, n_cand = got[0].cpu().tolist(), got[1].cpu().tolist()
        assert rank[4] == 0 and n_cand[4] == 1 and rank[5] == 0 and n_cand[5] == 1
        assert n_cand[:4] == [Ni - item_lo - 3, Ni - item_lo - 2, Ni - item_lo - 3, Ni - item_lo] and n_cand[7] == Ni - item_lo
        # the same pairs in another order through the map, and against no list at all
        perm = torch.tensor([6, 5, 4, 3, 2, 1, 0, 0])
        shuffled = (off.to(DEV), items.to(DEV), perm.to(DEV))
        _assert_ranks(RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=item_lo, exclude=shuffled),
                      _yardstick(dense, tgt, item_lo, shuffled), f"{mode}: permuted map")
        plain_off = torch.cat([off, off[-1:]])                    # [B + 1]: pair 7 gets an empty row
        plain = (plain_off.to(DEV), items.to(DEV))
        _assert_ranks(RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=item_lo, exclude=plain),
                      _yardstick(dense, tgt, item_lo, plain), f"{mode}: [B + 1] CSR")
        empty = (torch.zeros(9, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
        _assert_ranks(RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=item_lo, exclude=empty),
                      _yardstick(dense, tgt, item_lo), f"{mode}: empty CSR")
    with pytest.raises(RuntimeError, match="exclude offsets"):
        RF.pair_score_rank("dot", ul, il, tgt.to(DEV), exclude=(off.to(DEV), items.to(DEV)))       # 7 rows for 8 pairs, no map


# ------------------------------------------------------------------------------------------------ ties, NaN, ids
def test_ties_go_to_the_lower_item_id():
    from review_based_recommender_amd import functional as RF
    B, Ni, K = 9, 200, 8
    gen = torch.Generator().manual_seed(3)
    tgt = torch.randint(1, Ni, (B,), generator=gen)
    off, items = _random_csr(B, Ni, gen, 30)
    excl = (off.to(DEV), items.to(DEV))
    # every item row is the same row: bit-equal scores within a pair
    ul, il, h, g, ub, ib = _tables(B, Ni, K, seed=4)
    il[:], ib[:] = il[0].clone(), ib[0].clone()
    ul, il, h, g, ub, ib = _to_dev(ul, il, h, g, ub, ib)
    # an all-zero item table in the dot mode: every score is +0
    zeros = torch.zeros(Ni, K, device=DEV)
    lists = _lists(excl, B)
    want = torch.tensor([sum(1 for j in range(1, int(t)) if j not in set(lists[b])) for b, t in enumerate(tgt)], dtype=torch.int32)
    want_n = torch.tensor([Ni - 1 - len({j for j in lists[b] if j >= 1 and j != int(tgt[b])}) for b in range(B)], dtype=torch.int32)
    for what, got in (("equal rows, fm", RF.pair_score_rank("fm", ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=1, exclude=excl)),
                      ("zero table, dot", RF.pair_score_rank("dot", ul, zeros, tgt.to(DEV), item_lo=1, exclude=excl))):
        _assert_ranks(got, (want, want_n), what)              # rank = the non-excluded ids below the target
    dense = RF.pair_score_dense("fm", ul, il, h, g, ub, ib)
    assert bool((dense.view(torch.int32) == dense.view(torch.int32)[:, :1]).all())
    _assert_ranks(RF.pair_score_rank("fm", ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=1, exclude=excl), _yardstick(dense, tgt, 1, excl),
                  "equal rows against the yardstick")


@pytest.mark.parametrize("mode", ["fm", "dot"])
def test_nan_items_are_no_candidates_and_a_nan_target_is_unranked(mode):
    from review_based_recommender_amd import functional as RF
    B, Ni, K = 9, 130, 8
    ul, il, h, g, ub, ib = _tables(B, Ni, K, seed=6)
    nan_items = [3, 64, 65, 129]
    il[nan_items], ib[nan_items] = NAN, NAN          # relu drops a NaN product in the fm mode: the item bias carries it there
    tgt = torch.tensor([3, 10, 129, 64, 5, 6, 7, 8, 100])
    off = torch.tensor([0, 2, 4, 4, 4, 4, 4, 4, 4, 4], dtype=torch.int64)
    items = torch.tensor([64, 70, 3, 65], dtype=torch.int32)       # lists that name NaN items: not subtracted a second time
    excl = (off.to(DEV), items.to(DEV))
    ul, il, h, g, ub, ib = _to_dev(ul, il, h, g, ub, ib)
    dense = RF.pair_score_dense(mode, ul, il, h, g, ub, ib)
    assert bool(torch.isnan(dense[:, nan_items]).all()) and int(torch.isnan(dense).sum()) == B * len(nan_items)
    for e in (None, excl):
        rank, n_cand = RF.pair_score_rank(mode, ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=1, exclude=e)
        _assert_ranks((rank, n_cand), _yardstick(dense, tgt, 1, e), f"{mode} exclusion={e is not None}")
        assert rank.cpu().tolist()[:4] == [-1, rank[1].item(), -1, -1] and int(rank[1]) >= 0
        want_n = Ni - 1 - len(nan_items)
        assert n_cand.cpu().tolist() == ([want_n - 1, want_n] + [want_n] * 7 if e is not None else [want_n] * 9)
    RF.check_id_errors(DEV)


def test_targets_outside_the_table_are_unranked_and_reported():
    from review_based_recommender_amd import functional as RF
    B, Ni, K = 5, 40, 8
    ul, il, h, g, ub, ib = _to_dev(*_tables(B, Ni, K, seed=8))
    dense = RF.pair_score_dense("fm", ul, il, h, g, ub, ib)
    RF.check_id_errors(DEV)
    tgt = torch.tensor([Ni, -1, 0, 7, 1 << 40])
    got = RF.pair_score_rank("fm", ul, il, tgt.to(DEV), h, g, ub, ib, item_lo=1)
    _assert_ranks(got, _yardstick(dense, tgt, 1), "ids")
    assert got[0].cpu().tolist()[:3] == [-1, -1, -1] and int(got[0][3]) >= 0 and int(got[0][4]) == -1
    assert got[1].cpu().tolist() == [Ni - 1] * B
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)                                        # the record is cleared
    # a target below item_lo is unranked and no id error
    got = RF.pair_score_rank("fm", ul, il, torch.tensor([0, 2, 3, 39, 5], device=DEV), h, g, ub, ib, item_lo=3)
    assert got[0].cpu().tolist()[:2] == [-1, -1] and int(got[0][2:].min()) >= 0
    RF.check_id_errors(DEV)
    empty = RF.pair_score_rank("fm", ul[:0], il, tgt[:0].to(DEV), h, g, ub[:0], ib)
    assert empty[0].shape == (0,) and empty[1].shape == (0,) and empty[0].dtype == torch.int32


# ------------------------------------------------------------------------------------------------ determinism and capture
def test_two_calls_return_the_same_bytes():
    from review_based_recommender_amd import functional as RF
    B, Ni, K = 257, 5000, 50
    gen = torch.Generator().manual_seed(12)
    ul, il, h, g, ub, ib = _to_dev(*_tables(B, Ni, K, seed=12, dup=500))
    tgt = torch.randint(0, Ni, (B,), generator=gen).to(DEV)
    off, items = _random_csr(B, Ni, gen, 20)
    excl = (off.to(DEV), items.to(DEV))
    a = RF.pair_score_rank("fm", ul, il, tgt, h, g, ub, ib, item_lo=1, exclude=excl)
    b = RF.pair_score_rank("fm", ul, il, tgt, h, g, ub, ib, item_lo=1, exclude=excl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _assert_ranks(a, _yardstick(RF.pair_score_dense("fm", ul, il, h, g, ub, ib), tgt, 1, excl), "257 x 5000")


def test_rank_records_into_a_graph_and_replays_with_new_inputs():
    """One capture on a single stream (the conventions of train_step.GraphedForward, as the topk capture test follows them:
    warm-up on a side stream, the library's capture guard around the recording), one replay after the latents, the biases and
    the targets changed in place."""
    from review_based_recommender_amd import _lib, functional as RF
    from review_based_recommender_amd.train_step import _capture_stream
    B, Ni, K = 64, 5000, 32
    gen = torch.Generator().manual_seed(2)
    ul, il, h, g, ub, ib = _to_dev(*_tables(B, Ni, K, seed=31))
    tgt = torch.randint(1, Ni, (B,), generator=gen).to(DEV)
    off, items = _random_csr(B, Ni, gen, max_per_row=20)
    excl = (off.to(DEV), items.to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RF.pair_score_rank("fm", ul, il, tgt, h, g, ub, ib, item_lo=1, exclude=excl)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    cs = _capture_stream(torch.device(DEV))
    with _lib.capture_guard(cs), torch.cuda.graph(graph, stream=cs, capture_error_mode="global"):
        out = RF.pair_score_rank("fm", ul, il, tgt, h, g, ub, ib, item_lo=1, exclude=excl)
    ul2, il2, _, _, ub2, ib2 = _to_dev(*_tables(B, Ni, K, seed=32))
    for dst, new in ((ul, ul2), (il, il2), (ub, ub2), (ib, ib2), (tgt, torch.randint(1, Ni, (B,), generator=gen).to(DEV))):
        dst.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    replayed = (out[0].clone(), out[1].clone())
    _assert_ranks(replayed, _yardstick(RF.pair_score_dense("fm", ul, il, h, g, ub, ib), tgt, 1, excl), "graph replay")
    eager = RF.pair_score_rank("fm", ul, il, tgt, h, g, ub, ib, item_lo=1, exclude=excl)
    assert torch.equal(replayed[0], eager[0]) and torch.equal(replayed[1], eager[1])
    RF.check_id_errors(DEV)


# ------------------------------------------------------------------------------------------------ through the models
def _deepconn_tiny():
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    c = synth.DEEPCONN_CFGS["tiny"]
    m = quiet(DeepCoNNpp, c["U"], c["I"], c["V"], c["kz"], c["D"], c["H"], c["K"], c["L"], None, 0.5)
    m.load_state_dict(synth.deepconn_params(c, 0))
    return m, c["U"], c["I"], c["L"], c["V"]


def _datt_tiny():
    from review_based_recommender_amd.models.dual_att.dual_att import DualAtt
    c = synth.DATT_CFGS["tiny"]
    m = quiet(DualAtt, c["V"], c["L"], c["win"], c["l_out"], c["g_out"], c["E"], c["h1"], c["h2"], 0.5, None)
    m.load_state_dict(synth.datt_params(c, 0))
    return m, 7, 9, c["L"], c["V"]            # D-ATT has no id tables: any number of documents per side


@pytest.mark.parametrize("build,mode", [(_deepconn_tiny, "fm"), (_datt_tiny, "dot")])
def test_recommender_rank_and_evaluate(build, mode):
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.recommend import Recommender, rank_metrics
    m, U, I, L, V = build()
    m.to(DEV).eval()
    assert m.score_mode_and_params()[0] == mode
    rng = np.random.default_rng(3)
    docs = [torch.from_numpy(synth._docs(rng, n, L, V)).to(torch.int32) for n in (U, I)]
    for d in docs:
        d[0] = 0                              # id 0: the all-pad document
    rec = Recommender(m, user=docs[0].to(DEV), item=docs[1].to(DEV)).refresh()
    pairs = [(u, i, 3.0) for u in range(1, U) for i in range(0, I)]          # item 0 is the padding id: unranked
    train = [(u, (u * 3 + j) % I) for u in range(1, U) for j in range(2)]
    seen = Recommender.seen_from(train, U, DEV)
    u_ids = torch.tensor([p[0] for p in pairs], device=DEV)
    i_ids = torch.tensor([p[1] for p in pairs], device=DEV)
    full = rec.score_all(u_ids)
    for excl in (None, seen):
        got = rec.rank(u_ids, i_ids, exclude=excl)
        want = _yardstick(full, i_ids, 1, None if excl is None else (seen.off, seen.items, u_ids))
        _assert_ranks(got, want, f"Recommender.rank exclusion={excl is not None}")
        assert int((got[0] < 0).sum()) == U - 1
        # the same integers summed on the same device in the same shape: the same float64 sums, bit for bit
        metrics = rank_metrics(want[0].to(DEV), want[1].to(DEV), (1, 3))
        assert metrics["n"] == len(pairs) and metrics["unranked"] == U - 1 and 0 < metrics["hr@3"] < 1
        # on the CPU the terms are added in another order: n <= 54 terms of at most 1, so the sums differ by less than
        # n * 2^-53 * n < 4e-13 and the means by less still
        on_cpu = rank_metrics(want[0], want[1], (1, 3))
        assert all(v == on_cpu[k] if isinstance(v, int) else abs(v - on_cpu[k]) <= 4e-13 for k, v in metrics.items())
        assert rec.evaluate(pairs, (1, 3), exclude=excl, chunk=7) == metrics          # ragged chunks, examples
        assert rec.evaluate((u_ids.cpu(), i_ids.cpu()), (1, 3), exclude=excl) == metrics      # id tensors, one chunk
    RF.check_id_errors(DEV)


def _doc_experiment_model(tmp_path):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)
    ds = D.DocDataset(data_dir, "train")
    torch.manual_seed(0)
    m = quiet(DeepCoNNpp, ds.user_num, ds.item_num, ds.vocab_size, [3, 5], 12, 8, 4, ds.doc_len, None, 0.5).to(DEV)
    return data_dir, ds, m


def test_cli_writes_one_line_of_metrics(tmp_path, capsys):
    from review_based_recommender_amd import data as D, recommend
    data_dir, ds, m = _doc_experiment_model(tmp_path)
    cfg = {"data_dir": data_dir, "model_name": "deepconn", "kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12,
           "latent_dim": 4, "dropout": 0.5}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    torch.save({"model": m.state_dict(), "optimizer": {}, "updates": 0, "args": cfg}, tmp_path / "best_model.pt")
    base = ["--model", "deepconn", "--config", str(tmp_path / "cfg.json"), "--checkpoint", str(tmp_path / "best_model.pt"),
            "--eval-split", "valid", "--ks", "5,10", "--chunk", "5"]
    out = tmp_path / "metrics.json"
    assert recommend.main(base + ["--exclude-train", "--metrics-out", str(out)]) == 0
    lines = out.read_text().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    valid = D.load_pickle(os.path.join(data_dir, "valid_exmaples.pkl"))
    rec = recommend.Recommender(m.eval(), D.DeviceDocCache(ds, DEV)).refresh()
    seen = recommend.Recommender.seen_from(ds.examples, ds.user_num, DEV)
    want = rec.evaluate(valid, (5, 10), exclude=seen)
    assert got == dict(want, split="valid", exclude_train=True)
    assert got["n"] == len(valid) and got["unranked"] == 0 and 0 < got["hr@5"] <= got["hr@10"] <= 1
    assert not (tmp_path / "recs.jsonl").exists()
    # without --metrics-out the line goes to stdout; without --exclude-train every item but the padding id competes
    capsys.readouterr()
    assert recommend.main(base) == 0
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(printed) == 1 and json.loads(printed[0]) == dict(rec.evaluate(valid, (5, 10)), split="valid", exclude_train=False)


VALID_RE = re.compile(r"^valid loss: \d+\.\d{3}, valid rmse: \d+\.\d{3}, best rmse: \d+\.\d{3}$")
RANK_RE = re.compile(r"^valid hr@5: [01]\.\d{3}, ndcg@5: [01]\.\d{3}, mrr: [01]\.\d{3}$")


def test_trainer_logs_rank_metrics_and_leaves_the_rmse_alone(tmp_path):
    from test_trainer_gpu import LOG_RE
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = str(tmp_path / "data")
    make_dataset.write_doc_split(data_dir)
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": "deepconn", "kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12, "latent_dim": 4, "dropout": 0.5,
           "epochs": 1, "batch_size": 16, "device_cache": True, "eval_from_towers": True, "patience": 100}
    logs, rmse, state = {}, {}, None
    for ranked in (True, False):
        path = tmp_path / f"cfg_{int(ranked)}.json"
        path.write_text(json.dumps(dict(cfg, rank_metrics=[5]) if ranked else cfg))
        exp = ReviewExperiment("deepconn", parse_args(str(path)), uid=f"r{int(ranked)}")
        if state is None:
            exp.train_one_epoch(0)
            state = {k: v.clone() for k, v in exp.model.state_dict().items()}
        else:
            exp.model.load_state_dict(state)
        exp.valid_one_epoch()
        rmse[ranked] = exp.last_valid_rmse
        logs[ranked] = open(os.path.join(exp.out_dir, "log.txt")).read().splitlines()
        if ranked:
            seen = Recommender.seen_from(exp.train_set.examples, exp.train_set.user_num, DEV)
            want = Recommender(exp.model, exp.cache).refresh().evaluate(exp.valid_set.examples, (5,), exclude=seen)
            assert exp.last_rank_metrics == want and want["n"] == len(exp.valid_set)
    steps = [l for l in logs[True] if l.startswith("epoch:")]
    assert len(steps) == 6 // 2 and all(LOG_RE.match(l) for l in steps)
    valid = [l for l in logs[True] if l.startswith("valid")]
    assert len(valid) == 2 and VALID_RE.match(valid[0]) and RANK_RE.match(valid[1]), valid
    assert [l for l in logs[False] if l.startswith("valid")] == valid[:1]          # the same RMSE line, and no other
    assert rmse[True] == rmse[False]
