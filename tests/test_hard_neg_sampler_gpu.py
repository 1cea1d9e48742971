"""rbr_sample_hard_negatives on the device: the candidates against the integer restatement of the draw (tests/hard_neg_ref.py),
their scores against functional.pair_score bit for bit, the chosen negative against the key rule restated on the host, n_cand = 1
against rbr_sample_negatives, the edge cases of the choice, and the call number across eager calls and graph replays.  Every
comparison is an integer or a bit comparison: no tolerance appears."""
import functools
import itertools

import numpy as np
import pytest
import torch

from hard_neg_ref import choose, expected_outputs, sample_hard_negatives_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS = 6
HEADS = ["fm", "fm_nobias", "dot"]


def _state(call):
    return torch.tensor([call, 0], dtype=torch.int64, device=DEV)


def _seen(I):
    """Six users over the items [1, I): 0 empty row; 1 every other item; 2 all but item 1; 3 everything; 4 all but the last item;
    5 item 1 only."""
    every = list(range(1, I))
    rows = [[], every[::2], every[1:], every, every[:-1], every[:1]]
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int64), np.array([x for r in rows for x in r], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _pairs(B, I):
    rng = np.random.default_rng(1000 * B + I)
    return rng.integers(0, N_USERS, size=B).astype(np.int64), rng.integers(1, I, size=B).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _ref(B, n_neg, n_cand, I, with_seen, max_tries, seed, call):
    """The restated candidates: computed once per draw, shared by every K and head, never written to."""
    u, i = _pairs(B, I)
    cand, found = sample_hard_negatives_ref(u, i, n_neg, n_cand, I, _seen(I) if with_seen else None, seed, call, max_tries=max_tries,
                                            replace_id=1)
    cand.setflags(write=False)
    found.setflags(write=False)
    return cand, found


def _unaligned(rows, K, gen):
    """f32 [rows, K] whose first element sits 4 bytes past an allocation's start: nothing beyond 4-byte alignment holds."""
    flat = torch.randn(rows * K + 1, generator=gen, device=DEV)
    return flat[1:].view(rows, K)


@functools.lru_cache(maxsize=None)
def _tables(I, K):
    gen = torch.Generator(device=DEV).manual_seed(97 * I + K)
    ul, il = _unaligned(N_USERS, K, gen), _unaligned(I, K, gen)
    h, g = torch.randn(K, 1, generator=gen, device=DEV), torch.randn(1, generator=gen, device=DEV)
    ub, ib = torch.randn(N_USERS, 1, generator=gen, device=DEV), torch.randn(I, 1, generator=gen, device=DEV)
    return ul, il, h, g, ub, ib


def _head(head, I, K):
    ul, il, h, g, ub, ib = _tables(I, K)
    if head == "dot":
        return dict(mode="dot", ul=ul, il=il)
    if head == "fm_nobias":
        return dict(mode="fm", ul=ul, il=il, h=h, g=g)
    return dict(mode="fm", ul=ul, il=il, h=h, g=g, ub=ub, ib=ib)


def _dev_seen(I):
    off, items = _seen(I)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(items).to(DEV)


def _check(got, u, i, cand_ref, found_ref, head_kw):
    """The exact-equality conditions of one launch; returns the chosen items [n_neg, B]."""
    from review_based_recommender_amd import functional as RF
    u_out, i_out, valid, cand, score = got
    n_neg, B, n_cand = cand_ref.shape
    assert cand.shape == score.shape == (n_neg, B, n_cand)
    assert torch.equal(cand.cpu(), torch.tensor(cand_ref))
    u_flat = torch.from_numpy(u).to(DEV)[None, :, None].expand(n_neg, B, n_cand).reshape(-1)
    want = RF.pair_score(head_kw["mode"], head_kw["ul"], head_kw["il"], u_flat, cand.reshape(-1),
                         *(head_kw.get(k) for k in ("h", "g", "ub", "ib")))
    assert torch.equal(score.reshape(-1).view(torch.int32), want.view(torch.int32))
    ref = expected_outputs(u, i, cand_ref, found_ref, score.cpu().numpy())
    for g, r in zip((u_out, i_out, valid), ref):
        assert torch.equal(g.cpu(), torch.from_numpy(r))
    return ref[1][B:].reshape(n_neg, B)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n_cand", [1, 2, 3, 5, 8, 64])
def test_hard_sampler_equals_the_restatement_and_pair_score(n_cand, head):
    """B in {1, 5, 70} (70 pairs of 64-lane draws are 18 workgroups) x n_neg in {1, 3} x I in {2, 9, 300} x K in {1, 5, 32, 33} x
    with / without a seen list x max_tries in {1, 16}, for this n_cand and head."""
    from review_based_recommender_amd import functional as RF
    seed, call = 77, 4
    for B, n_neg, I, with_seen, max_tries in itertools.product([1, 5, 70], [1, 3], [2, 9, 300], [True, False], [1, 16]):
        u, i = _pairs(B, I)
        cand_ref, found_ref = _ref(B, n_neg, n_cand, I, with_seen, max_tries, seed, call)
        ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
        seen = _dev_seen(I) if with_seen else None
        for K in (1, 5, 32, 33):
            kw = _head(head, I, K)
            state = _state(call)
            got = RF.sample_hard_negatives(ud, idv, n_neg, I, seen, n_cand=n_cand, state=state, seed=seed, max_tries=max_tries,
                                           replace_id=1, return_candidates=True, **kw)
            try:
                _check(got, u, i, cand_ref, found_ref, kw)
            except AssertionError as e:
                raise AssertionError(f"B={B} n_neg={n_neg} I={I} K={K} seen={with_seen} max_tries={max_tries}") from e
            assert state.tolist() == [call + 1, 0]


@pytest.mark.parametrize("with_seen", [True, False])
@pytest.mark.parametrize("B,n_neg", [(1, 1), (257, 3)])
def test_one_candidate_is_the_uniform_sampler(B, n_neg, with_seen):
    from review_based_recommender_amd import functional as RF
    I, seed, call = 11, 21, 5
    u, i = _pairs(B, I)
    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    seen = _dev_seen(I) if with_seen else None
    for max_tries in (1, 16):
        uniform = RF.sample_negatives(ud, idv, n_neg, I, seen, state=_state(call), seed=seed, max_tries=max_tries, replace_id=1)
        for head in HEADS:
            hard = RF.sample_hard_negatives(ud, idv, n_neg, I, seen, n_cand=1, state=_state(call), seed=seed, max_tries=max_tries,
                                            replace_id=1, **_head(head, I, 5))
            for a, b in zip(hard, uniform):
                assert a.dtype == b.dtype and torch.equal(a, b)


def _launch(u, i, n_neg, I, seen, n_cand, kw, call=0, seed=9, **extra):
    from review_based_recommender_amd import functional as RF
    return RF.sample_hard_negatives(torch.as_tensor(u, device=DEV), torch.as_tensor(i, device=DEV), n_neg, I, seen, n_cand=n_cand,
                                    state=_state(call), seed=seed, return_candidates=True, **extra, **kw)


def test_nan_and_infinite_latents():
    """Item rows of NaN, +inf and -inf (dot mode: the score of such a row is NaN / +-inf for the positive user row below).  A NaN
    candidate is never chosen while another candidate has a number; where all are NaN, candidate 0 is."""
    I, K, n_cand, B, n_neg = 9, 5, 8, 70, 3
    ul = torch.rand(N_USERS, K, device=DEV) + 0.5
    il = torch.randn(I, K, device=DEV)
    il[2], il[3], il[5], il[6] = float("nan"), float("inf"), float("-inf"), float("nan")
    kw = dict(mode="dot", ul=ul, il=il)
    u, i = _pairs(B, I)
    got = _launch(u, i, n_neg, I, None, n_cand, kw, replace_id=1)
    cand_ref, found_ref = sample_hard_negatives_ref(u, i, n_neg, n_cand, I, None, 9, 0, replace_id=1)
    chosen = _check(got, u, i, cand_ref, found_ref, kw)
    score = got[4].cpu().numpy()
    nan = np.isnan(score)
    assert nan.any() and (~nan).any() and np.isposinf(score).any() and np.isneginf(score).any()
    some = ~nan.all(-1)
    assert some.any() and not np.isin(chosen[some], [2, 6]).any()
    assert (chosen[(cand_ref == 3).any(-1)] == 3).all()          # +inf beats everything
    # a catalogue whose every item scores NaN, and one where only the items 2 and 6 do not
    il_nan = torch.full_like(il, float("nan"))
    kw_nan = dict(mode="dot", ul=ul, il=il_nan)
    got = _launch(u, i, n_neg, I, None, n_cand, kw_nan, replace_id=1)
    chosen = _check(got, u, i, cand_ref, found_ref, kw_nan)
    assert np.array_equal(chosen, cand_ref[:, :, 0])
    il_nan[2], il_nan[6] = 1.0, -1.0
    got = _launch(u, i, n_neg, I, None, n_cand, kw_nan, replace_id=1)
    chosen = _check(got, u, i, cand_ref, found_ref, kw_nan)
    has2, has6 = (cand_ref == 2).any(-1), (cand_ref == 6).any(-1)
    assert has2.any() and (has6 & ~has2).any() and (~has2 & ~has6).any()
    assert (chosen[has2] == 2).all() and (chosen[has6 & ~has2] == 6).all()
    assert np.array_equal(chosen[~has2 & ~has6], cand_ref[:, :, 0][~has2 & ~has6])


@pytest.mark.parametrize("head", HEADS)
def test_equal_latents_choose_the_lowest_candidate_id(head):
    I, K, n_cand, B, n_neg = 300, 5, 5, 70, 3
    kw = _head(head, I, K)
    kw = dict(kw, il=kw["il"][:1].expand(I, K).contiguous())
    if "ib" in kw:
        kw["ib"] = torch.zeros(I, 1, device=DEV)
    u, i = _pairs(B, I)
    got = _launch(u, i, n_neg, I, _dev_seen(I), n_cand, kw, replace_id=1)
    cand_ref, found_ref = sample_hard_negatives_ref(u, i, n_neg, n_cand, I, _seen(I), 9, 0, replace_id=1)
    chosen = _check(got, u, i, cand_ref, found_ref, kw)
    assert np.array_equal(chosen, cand_ref.min(-1)) and (cand_ref.min(-1) != cand_ref.max(-1)).any()


def test_nothing_to_draw_and_a_single_item_catalogue():
    # user 3 has seen everything; user 4 everything but the last item, which is its positive; user 2 all but item 1 (drawn)
    I, n_cand = 9, 4
    u, i = np.array([3, 4, 2, 4], dtype=np.int64), np.array([5, 8, 5, 2], dtype=np.int64)
    kw = _head("fm", I, 5)
    for replace_id in (0, 1):
        got = _launch(u, i, 2, I, _dev_seen(I), n_cand, kw, replace_id=replace_id)
        cand_ref, found_ref = sample_hard_negatives_ref(u, i, 2, n_cand, I, _seen(I), 9, 0, replace_id=replace_id)
        _check(got, u, i, cand_ref, found_ref, kw)
        assert got[2].view(2, 4).tolist() == [[0.0, 0.0, 1.0, 1.0]] * 2
        assert got[1][4:].view(2, 4).tolist() == [[replace_id, replace_id, 1, 8]] * 2
        assert (got[3][:, :2] == replace_id).all()
    # one item, item_lo = 0: it is the draw unless it is the positive
    kw = _head("dot", 1, 5)
    u, i = np.array([0, 5, 1], dtype=np.int64), np.array([0, 7, 0], dtype=np.int64)
    got = _launch(u, i, 2, 1, None, 3, kw, item_lo=0, replace_id=0)
    cand_ref, found_ref = sample_hard_negatives_ref(u, i, 2, 3, 1, None, 9, 0, item_lo=0, replace_id=0)
    _check(got, u, i, cand_ref, found_ref, kw)
    assert got[1].tolist() == [0, 7, 0] + [0] * 6 and got[2].tolist() == [0.0, 1.0, 0.0] * 2


def test_user_id_outside_the_tables_scores_as_row_0():
    """Nothing is read outside ul / ub / the seen CSR: the ids -1, U and 2^40 draw from an empty seen row and score as user 0."""
    from review_based_recommender_amd import functional as RF
    I, K, n_cand, n_neg = 300, 33, 8, 3
    kw = _head("fm", I, K)
    bad = np.array([-1, N_USERS, 1 << 40, -(1 << 40), 2, 0], dtype=np.int64)
    i = np.array([4, 5, 6, 7, 8, 9], dtype=np.int64)
    got = _launch(bad, i, n_neg, I, _dev_seen(I), n_cand, kw, replace_id=1)
    cand_ref, found_ref = sample_hard_negatives_ref(bad, i, n_neg, n_cand, I, _seen(I), 9, 0, replace_id=1)
    assert found_ref.all()
    assert torch.equal(got[3].cpu(), torch.from_numpy(cand_ref))
    stand_in = np.where((bad >= 0) & (bad < N_USERS), bad, 0)
    u_flat = torch.from_numpy(stand_in).to(DEV)[None, :, None].expand(n_neg, len(bad), n_cand).reshape(-1)
    want = RF.pair_score("fm", kw["ul"], kw["il"], u_flat, got[3].reshape(-1), kw["h"], kw["g"], kw["ub"], kw["ib"])
    assert torch.equal(got[4].reshape(-1).view(torch.int32), want.view(torch.int32))
    ref = expected_outputs(bad, i, cand_ref, found_ref, got[4].cpu().numpy())          # u_out carries the ids as they came
    for g, r in zip(got[:3], ref):
        assert torch.equal(g.cpu(), torch.from_numpy(r))


def test_calls_advance_and_a_replayed_launch_draws_like_eager_calls():
    """Three eager calls use call numbers k, k + 1, k + 2; a captured launch replayed three times from the same reseed equals
    them, candidates and scores included."""
    from review_based_recommender_amd import functional as RF
    I, K, n_neg, n_cand, B, seed, k = 300, 5, 3, 5, 70, 21, 5
    kw = _head("fm", I, K)
    u, i = _pairs(B, I)
    ud, idv, seen = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), _dev_seen(I)
    state = _state(k)
    eager = []
    for s in range(3):
        got = RF.sample_hard_negatives(ud, idv, n_neg, I, seen, n_cand=n_cand, state=state, seed=seed, replace_id=1,
                                       return_candidates=True, **kw)
        cand_ref, found_ref = sample_hard_negatives_ref(u, i, n_neg, n_cand, I, _seen(I), seed, k + s, replace_id=1)
        _check(got, u, i, cand_ref, found_ref, kw)
        eager.append([t.clone() for t in got[:3]])
    assert state.tolist() == [k + 3, 0]
    assert not torch.equal(eager[0][1], eager[1][1]) and not torch.equal(eager[1][1], eager[2][1])

    out = (torch.zeros((1 + n_neg) * B, dtype=torch.int64, device=DEV), torch.zeros((1 + n_neg) * B, dtype=torch.int64, device=DEV),
           torch.zeros(n_neg * B, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        RF.sample_hard_negatives(ud, idv, n_neg, I, seen, n_cand=n_cand, state=state, seed=seed, replace_id=1, out=out, **kw)
    state.copy_(_state(k))                       # "reseed": the recorded launch reads the call number from the device
    for s in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for g, e in zip(out, eager[s]):
            assert torch.equal(g, e), s
    assert state.tolist() == [k + 3, 0]
