"""One hostile seen / exclusion CSR through all five entries that take one (csrc/item_csr.h): pair_score_topk, pair_score_rank,
sample_negatives, sample_hard_negatives and pair_softmax_loss.  Each entry is compared with the reference it already has, fed the
CSR after one host-side `sanitise` -- a row's [a, e) clamped to [0, nnz], e raised to a, a row outside the CSR empty.  Integer and
score outputs must match exactly, the softmax within the bounds of tests/softmax_ref.py.

A lost clamp must show as a wrong answer, not as an out-of-bounds read: the item array is the slice [8 : 8 + nnz] of a longer
buffer whose 8 entries in front hold low valid item ids and whose 8 entries behind hold high ones, both ascending, and every
hostile offset stays within [-8, nnz + 8].  `unclamped` restates what a reader without the clamp would see; the tests assert that
the references tell the two apart for the rows where that matters.

  user  offsets     sanitised row        hazard
  0     [-5, 2)     {9, 10}              a negative offset (unclamped: items 4 .. 8 as well)
  1     [2, 13)     {1 .. 11}            the user who saw everything
  2     [13, 17)    {3, 5, 5, 7}         a repeated item
  3     [17, 26)    {1, 2, 3}            an offset past nnz (unclamped: items 4 .. 9 as well)
  4     [26, 20)    {}                   a decreasing pair, its start past nnz
  5     [20, 20)    {}                   an empty row
  6, -1                                  ids outside [0, U): user ids of the samplers and the softmax, excl_row of topk and rank
and the same offsets over an array of nnz = 0 entries: every row empty."""
import numpy as np
import pytest
import torch

import softmax_ref as SR
from bpr_ref import sample_negatives_ref
from edge_refs import check
from hard_neg_ref import expected_outputs, sample_hard_negatives_ref
from test_rank_eval_gpu import _assert_ranks, _yardstick as rank_yardstick
from test_recommend_gpu import _assert_same_ranking, _yardstick as topk_yardstick

DEV = "cuda:0"
U, I, K, N_NEG, N_CAND, TOPK, ITEM_LO, PAD = 6, 12, 4, 2, 3, 3, 1, 8
OFF = [-5, 2, 13, 17, 26, 20, 20]
ROWS = [[9, 10], list(range(1, 12)), [3, 5, 5, 7], [1, 2, 3]]
BUF = list(range(1, 9)) + [x for r in ROWS for x in r] + list(range(4, 12))      # 8 low ids | the 20 entries | 8 high ids
USERS = [0, 1, 2, 3, 4, 5, 6, -1]                 # one pair / user row per hazard
POS = [4, 6, 8, 5, 7, 2, 9, 4]                    # the pairs' own items: none in its user's sanitised row (user 1 aside)
CSRS = ["hostile", "nnz0"]


def _lists(nnz, clamp, rows=None):
    """One item list per row of `rows` (default: every user) of the hostile CSR over BUF[PAD : PAD + nnz]: sanitised (clamp), or
    as a reader without the clamp finds it."""
    out = []
    for r in range(U) if rows is None else rows:
        a, e = (OFF[r], OFF[r + 1]) if 0 <= r < U else (0, 0)
        if clamp:
            a, e = min(max(a, 0), nnz), min(max(e, 0), nnz)
        out.append(BUF[PAD + a:PAD + max(e, a)])
    return out


def sanitise(nnz, rows=None):
    return _csr(_lists(nnz, True, rows))


def unclamped(nnz, rows=None):
    return _csr(_lists(nnz, False, rows))


def _csr(lists):
    off = np.cumsum([0] + [len(r) for r in lists]).astype(np.int64)
    return off, np.array([x for r in lists for x in r], dtype=np.int32)


def _t(csr):
    return torch.from_numpy(csr[0]), torch.from_numpy(csr[1])


def _nnz(which):
    return 0 if which == "nnz0" else len(BUF) - 2 * PAD


def _device_csr(which):
    """(off, items) on the device: items IS the slice of the long buffer, its neighbours the valid ids of BUF."""
    nnz = _nnz(which)
    buf = torch.tensor(BUF, dtype=torch.int32, device=DEV)
    return torch.tensor(OFF, dtype=torch.int64, device=DEV), buf[PAD:PAD + nnz]


def _tables(mode):
    """Latents under which items 4 .. 8 score best for every user, in that order: what a lost clamp would hide is what topk must
    return and what the rank counts."""
    gen = torch.Generator().manual_seed(15)
    pop = torch.tensor([0.0, 1, 2, 3, 12, 11, 10, 9, 8, 4, 5, 6])
    ul = 1.0 + 0.01 * torch.rand(len(USERS), K, generator=gen)
    il = pop[:, None] * (1.0 + 0.01 * torch.rand(I, K, generator=gen))
    if mode == "dot":
        return dict(mode="dot", ul=ul.to(DEV), il=il.to(DEV))
    h, g = 1.0 + torch.rand(K, 1, generator=gen), torch.randn(1, generator=gen)
    ub, ib = 0.01 * torch.randn(len(USERS), 1, generator=gen), 0.01 * torch.randn(I, 1, generator=gen)
    return dict(mode="fm", ul=ul.to(DEV), il=il.to(DEV), h=h.to(DEV), g=g.to(DEV), ub=ub.to(DEV), ib=ib.to(DEV))


def _head_args(kw):
    return [kw.get(k) for k in ("h", "g", "ub", "ib")]


def test_the_fixture_meets_its_own_conditions():
    """No GPU needed: the buffer and the offsets are what the docstring says, and the sanitised rows leave every user but user 1 an
    acceptable item."""
    nnz = _nnz("hostile")
    assert nnz == 20 and len(BUF) == nnz + 2 * PAD and all(-PAD <= o <= nnz + PAD for o in OFF) and all(0 <= x < I for x in BUF)
    assert BUF[:PAD] == sorted(BUF[:PAD]) and BUF[-PAD:] == sorted(BUF[-PAD:])
    assert _lists(nnz, True) == ROWS + [[], []] and _lists(0, True) == [[]] * U
    assert _lists(nnz, False)[0] == [4, 5, 6, 7, 8, 9, 10] and _lists(nnz, False)[3] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    for u, pos, row in zip(USERS, POS, _lists(nnz, True, USERS)):
        left = set(range(ITEM_LO, I)) - set(row) - {pos}
        assert (not left) == (u == 1), (u, left)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fm", "dot"])
@pytest.mark.parametrize("which", CSRS)
def test_topk_and_rank(which, mode):
    from review_based_recommender_amd import functional as RF
    kw, nnz = _tables(mode), _nnz(which)
    off, items = _device_csr(which)
    exclude = (off, items, torch.tensor(USERS, dtype=torch.int64, device=DEV))
    clean, lost = _t(sanitise(nnz, USERS)), _t(unclamped(nnz, USERS))
    dense = RF.pair_score_dense(kw["mode"], kw["ul"], kw["il"], *_head_args(kw))
    want = topk_yardstick(dense, TOPK, ITEM_LO, clean)
    got = RF.pair_score_topk(kw["mode"], kw["ul"], kw["il"], TOPK, *_head_args(kw), item_lo=ITEM_LO, exclude=exclude)
    _assert_same_ranking(got, want, f"topk {which} {mode}")
    tgt = torch.tensor(POS[:-1] + [I + 3], dtype=torch.int64)           # the last target lies outside the table
    want_r = rank_yardstick(dense, tgt, ITEM_LO, clean)
    got_r = RF.pair_score_rank(kw["mode"], kw["ul"], kw["il"], tgt.to(DEV), *_head_args(kw), item_lo=ITEM_LO, exclude=exclude)
    _assert_ranks(got_r, want_r, f"rank {which} {mode}")
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)                                         # the target outside the table, and nothing else
    if which == "hostile":
        # the fixture: users 0 and 3 get other items and other counts from a reader that lost the clamp; user 1's row is all fill
        lost_k, lost_r = topk_yardstick(dense, TOPK, ITEM_LO, lost), rank_yardstick(dense, tgt, ITEM_LO, lost)
        for r in (0, 3):
            assert not torch.equal(lost_k[0][r], want[0][r]) and int(lost_r[1][r]) != int(want_r[1][r])
        assert want[0][0].tolist() == [4, 5, 6] and want[0][1].tolist() == [-1] * TOPK and want[0][3].tolist() == [4, 5, 6]
        assert int(want_r[1][2]) == I - ITEM_LO - 3                     # {3, 5, 5, 7}: the repeated 5 left once


@pytest.mark.gpu
@pytest.mark.parametrize("which", CSRS)
def test_both_samplers(which):
    from review_based_recommender_amd import functional as RF
    nnz, seed, call = _nnz(which), 31, 6
    u, i = np.array(USERS, dtype=np.int64), np.array(POS, dtype=np.int64)
    ud, idv, B = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), len(USERS)
    seen, clean = _device_csr(which), sanitise(nnz)
    for max_tries in (1, 16):
        ref = sample_negatives_ref(u, i, N_NEG, I, clean, seed, call, item_lo=ITEM_LO, max_tries=max_tries, replace_id=1)
        state = torch.tensor([call, 0], dtype=torch.int64, device=DEV)
        got = RF.sample_negatives(ud, idv, N_NEG, I, seen, state=state, seed=seed, item_lo=ITEM_LO, max_tries=max_tries, replace_id=1)
        for g, r in zip(got, ref):
            assert torch.equal(g.cpu(), torch.from_numpy(r)), (which, max_tries)
        assert state.tolist() == [call + 1, 0]
        valid = ref[2].reshape(N_NEG, B)                                 # only the user who saw everything is left without one
        assert np.delete(valid, 1, axis=1).min() == 1.0 and valid[:, 1].max() == (0.0 if which == "hostile" else 1.0)
        if which == "hostile":
            lost = sample_negatives_ref(u, i, N_NEG, I, unclamped(nnz), seed, call, item_lo=ITEM_LO, max_tries=max_tries, replace_id=1)
            assert not np.array_equal(lost[1], ref[1])                  # the fixture: a lost clamp draws other items

        for mode in ("fm", "dot"):
            kw = _tables(mode)
            kw["ul"], kw["ub"] = kw["ul"][:U].contiguous(), (kw["ub"][:U].contiguous() if "ub" in kw else None)      # U rows
            cand_ref, found_ref = sample_hard_negatives_ref(u, i, N_NEG, N_CAND, I, clean, seed, call, item_lo=ITEM_LO,
                                                            max_tries=max_tries, replace_id=1)
            state = torch.tensor([call, 0], dtype=torch.int64, device=DEV)
            u_out, i_out, v, cand, score = RF.sample_hard_negatives(ud, idv, N_NEG, I, seen, n_cand=N_CAND, state=state, seed=seed,
                                                                    item_lo=ITEM_LO, max_tries=max_tries, replace_id=1,
                                                                    return_candidates=True, **kw)
            assert torch.equal(cand.cpu(), torch.from_numpy(cand_ref)) and state.tolist() == [call + 1, 0]
            rows = torch.where((ud >= 0) & (ud < U), ud, torch.zeros_like(ud))                  # an id outside the table: row 0
            want = RF.pair_score(kw["mode"], kw["ul"], kw["il"], rows[None, :, None].expand(N_NEG, B, N_CAND).reshape(-1),
                                 cand.reshape(-1), *_head_args(kw))
            assert torch.equal(score.reshape(-1).view(torch.int32), want.view(torch.int32))
            for g, r in zip((u_out, i_out, v), expected_outputs(u, i, cand_ref, found_ref, score.cpu().numpy())):
                assert torch.equal(g.cpu(), torch.from_numpy(r)), (which, max_tries, mode)
    RF.check_id_errors(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("fm", [True, False], ids=["fm", "dot"])
@pytest.mark.parametrize("which", CSRS)
def test_softmax_loss(which, fm):
    from review_based_recommender_amd import functional as RF
    nnz, B = _nnz(which), len(USERS)
    c = SR.random_case(B, K, fm, 150 + fm, with_rb=True, with_cb=True, with_logq=False, with_drop=False)
    u_ids = torch.tensor(USERS, dtype=torch.int64)
    i_ids = torch.tensor([4, 6, 5, 2, 7, 9, 3, 10], dtype=torch.int64)           # items of the rows and of what a lost clamp adds
    leaves = {k: c[k].to(DEV).requires_grad_(True) for k in ("ul", "il", "h", "row_bias", "col_bias") if c[k] is not None}
    loss, pos = RF.pair_softmax_loss(leaves["ul"], leaves["il"], u_ids.to(DEV), i_ids.to(DEV), "fm" if fm else "dot", h=leaves.get("h"),
                                     row_bias=leaves["row_bias"], col_bias=leaves["col_bias"], seen=_device_csr(which), item_lo=ITEM_LO)
    loss.backward(RF.unit_scalar(DEV))
    clean = _t(sanitise(nnz))
    ref = SR.pair_softmax_ref(c["ul"], c["il"], u_ids, i_ids, fm, c["h"], c["row_bias"], c["col_bias"], None, clean, ITEM_LO)
    got = {"loss": loss.detach(), "pos": pos, "d_ul": leaves["ul"].grad, "d_il": leaves["il"].grad, "d_col_bias": leaves["col_bias"].grad}
    if fm:
        got["d_h"] = leaves["h"].grad
    for n in got:
        check(f"item_csr softmax {which} {'fm' if fm else 'dot'}", n, got[n], ref[n][0], ref[n][1])
    # a masked pair has P exactly 0 and bound 0: the gradient rows of a user whose every negative is masked are exact zeros
    assert ref["allowed"][0][1].sum() == (1 if which == "hostile" else B) and (which == "nnz0" or not bool(got["d_ul"][1].any()))
    if which == "hostile":
        lost = SR.allowed_mask(u_ids, i_ids, _t(unclamped(nnz)), ITEM_LO)
        assert not torch.equal(lost[0], ref["allowed"][0][0]) and not torch.equal(lost[3], ref["allowed"][0][3])      # the fixture
