"""Review sampling inside the id-fed gather, on the host: the uniformity and the properties of the restated draw
(review_sample_ref, written from include/rbr_hip.h), data.py's cpu feed against that restatement, the pooled cache against
today's, the trainer's config errors and the C entry's refusals (CPU only)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import make_review_dataset
import review_sample_ref as ref

ROWS, CALLS = 512, 40
SEEDS = (0, 7, 20261020)
# (m live, n kept) -> the 1 - 1e-6 quantile of chi2(m - 1) by Wilson-Hilferty
CASES = {(5, 2): 35.2, (12, 4): 49.9, (63, 8): 130.3}


def _draws(m, n, seed):
    """chosen candidates [ROWS * CALLS, n] with all m candidates live."""
    live = np.ones((ROWS, m), dtype=bool)
    return np.concatenate([ref.chosen(live, n, np.arange(ROWS), call, seed) for call in range(CALLS)])


@pytest.mark.parametrize("m,n", sorted(CASES))
@pytest.mark.parametrize("seed", SEEDS)
def test_the_restated_draw_is_uniform(m, n, seed):
    picks = _draws(m, n, seed)
    N = picks.shape[0]
    assert N == ROWS * CALLS and picks.min() >= 0 and picks.max() < m
    bound = CASES[(m, n)]
    worst = 0.0
    for k in range(n):                              # which candidate landed in output slot k: uniform over the m
        cnt = np.bincount(picks[:, k], minlength=m).astype(np.float64)
        chi = float(((cnt - N / m) ** 2 / (N / m)).sum())
        worst = max(worst, chi)
        assert chi < bound, (k, chi)
    inc = np.bincount(picks.ravel(), minlength=m).astype(np.float64)      # inclusion: N n / m each, variance factor 1 - n / m
    exp = N * n / m
    chi_inc = float(((inc - exp) ** 2 / (exp * (1.0 - n / m))).sum())
    print(f"m={m} n={n} seed={seed}: worst slot chi2 {worst:.1f}, inclusion chi2 {chi_inc:.1f}, bound {bound}")
    assert chi_inc < bound, chi_inc


@pytest.mark.parametrize("R,P,n_u,n_i", [(3, 3, 3, 3), (3, 7, 2, 1), (4, 12, 4, 2)])
def test_properties_of_the_restated_draw(R, P, n_u, n_i):
    rng = np.random.default_rng(R * 100 + P)
    N, T, B = 9, 5, 64
    ur, ud = ref.random_tables(rng, N, P, T)
    ir, idd = ref.random_tables(rng, N, P, T)
    u, i = rng.integers(0, N, size=B), rng.integers(0, N, size=B)
    for b in range(0, B, 2):                                    # half the pairs have a review of their own to leave out
        if ud[u[b]].any():
            i[b] = ud[u[b]][rng.integers(0, P + 1)] or i[b]
    got = ref.gather_ref(u, i, ur, ud, ir, idd, R, n_u, n_i, seed=3, call=11)
    again = ref.gather_ref(u, i, ur, ud, ir, idd, R, n_u, n_i, seed=3, call=11)
    nxt = ref.gather_ref(u, i, ur, ud, ir, idd, R, n_u, n_i, seed=3, call=12)
    for k in ("revs", "word_masks", "rev_masks", "rids", "ids", "slots"):
        assert np.array_equal(got[k], again[k]), k
    assert not np.array_equal(got["slots"], nxt["slots"])
    left_out = 0
    for r in range(2 * B):
        s, b = (0, r) if r < B else (1, r - B)
        a, c = ((u[b], i[b]), (i[b], u[b]))[s]
        tab, rid = ((ur, ud), (ir, idd))[s]
        first = [j for j in range(P) if rid[a, j] == c and c > 0]
        d = first[0] if first else P
        left_out += bool(first)
        cand = [q + (q >= d) for q in range(P)]
        live = [x for x in cand if (tab[a, x] != 0).any()]
        slots = got["slots"][r].tolist()
        keep = min((n_u, n_i)[s], len(live))
        kept = slots[:keep]
        assert all(x >= 0 for x in kept) and slots[keep:] == [-1] * (R - keep), (r, slots, keep)       # k_s = min(n, m), empty tail
        assert len(set(kept)) == len(kept)                      # no candidate twice
        assert d not in kept                                    # never the left-out slot
        assert set(kept) <= set(live)                           # never a dead slot (nor one outside the candidates)
        for k in range(R):
            if k < keep:
                assert np.array_equal(got["revs"][r, k], tab[a, slots[k]]) and got["rids"][r, k] == rid[a, slots[k]]
                assert got["rev_masks"][r, k]
            else:
                assert not got["revs"][r, k].any() and got["rids"][r, k] == 0 and not got["rev_masks"][r, k]
        assert np.array_equal(got["word_masks"][r], got["revs"][r] != 0)
    assert left_out > B // 4


# ------------------------------------------------------------------------------------------------ data.py
@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("review_sample_split")
    info = make_review_dataset.write_review_split(str(d))
    return str(d), info


def _ref_of(cache, u, i, n_u, n_i, seed, call):
    return ref.gather_ref(u.numpy(), i.numpy(), cache.user_pool_table.numpy(), cache.user_pool_rid_table.numpy(),
                          cache.item_pool_table.numpy(), cache.item_pool_rid_table.numpy(), cache.rv_num, n_u, n_i, seed, call)


@pytest.mark.parametrize("pool,n_u,n_i", [(None, None, None), (4, 2, 3), (6, 2, 2), (7, 4, 1)])
def test_cpu_sampled_feed_equals_the_restatement(split, pool, n_u, n_i):
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.ReviewDataset(d, "train")
    cache = D.DeviceReviewCache(ds, "cpu", pool=pool)
    R = info["rv_num"]
    assert cache.pool == (pool or R) and cache.user_pool_table.shape[1] == cache.pool + 1
    u = torch.tensor([p[0] for p in info["pairs"]] + [0, 3])
    i = torch.tensor([p[1] for p in info["pairs"]] + [2, 0])
    feed = cache.sampled_feed("narre", n_u, n_i, seed=9)
    assert isinstance(feed, D.ReviewFeed) and feed.leave_one_out and feed.order == cache.ORDER["narre"] and feed.seed == 9
    assert [t.shape for t in feed.empty_inputs(5)] == [t.shape for t in cache.feed("narre", True).empty_inputs(5)]
    for call in range(3):
        assert int(feed.state[0]) == call and int(feed.state[1]) == 0            # one call number per gather
        got = feed.gather(u, i, slots=True)
        want = _ref_of(cache, u, i, n_u or R, n_i or R, 9, call)
        for k in ("revs", "word_masks", "rids", "ids", "slots"):
            assert torch.equal(got[k], torch.from_numpy(want[k])), (call, k)
        assert got["rev_masks"] is None                          # not one of NARRE's arguments
    feed.reseed(5, 17)
    assert feed.seed == 5 and int(feed.state[0]) == 17
    got = cache.sampled_feed("simple_siamese", n_u, n_i, seed=5)
    got.reseed(5, 17)
    args = got.inputs(u, i)
    want = _ref_of(cache, u, i, n_u or R, n_i or R, 5, 17)
    B = u.shape[0]
    for k, name in enumerate(("revs", "word_masks", "rev_masks", "ids")):
        assert torch.equal(torch.cat([args[2 * k], args[2 * k + 1]]), torch.from_numpy(want[name])), name
        assert args[2 * k].shape[0] == B
    assert int(got.state[0]) == 18
    out = feed.gather(u, i, slots=True)                          # writes into given tensors, too
    into = torch.empty_like(out["slots"])
    feed.reseed(5, 17)
    assert feed.gather(u, i, slots=into)["slots"] is into and torch.equal(into, out["slots"])
    with pytest.raises(IndexError):
        feed.gather(torch.tensor([info["user_num"]]), torch.tensor([1]))
    for bad in (0, R + 1, True, 2.0):
        with pytest.raises(ValueError, match="n_user"):
            cache.sampled_feed("narre", bad, 1)
    with pytest.raises(ValueError):
        cache.sampled_feed("deepconn")


def test_full_sampling_keeps_every_review_of_the_plain_train_batch(split):
    """P = R, n = R: the draw only reorders -- each row's non-empty reviews, with their rids, are the plain feed's."""
    from review_based_recommender_amd import data as D
    d, info = split
    cache = D.DeviceReviewCache(D.ReviewDataset(d, "train"), "cpu")
    u = torch.tensor([p[0] for p in info["pairs"]])
    i = torch.tensor([p[1] for p in info["pairs"]])
    plain = D.ReviewFeed(cache, "narre", True).gather(u, i)
    got = cache.sampled_feed("narre", seed=1).gather(u, i)
    moved = filled = 0
    for r in range(2 * u.shape[0]):
        def rows(g):
            return sorted((int(rd), tuple(rv.tolist())) for rv, rd in zip(g["revs"][r], g["rids"][r]) if rv.any())
        assert rows(got) == rows(plain), r
        filled += bool(rows(plain))
        moved += not torch.equal(got["revs"][r], plain["revs"][r])
    assert moved > 0 and filled > u.shape[0]


def test_the_pooled_cache_keeps_the_plain_tables_byte_for_byte(split):
    from review_based_recommender_amd import data as D
    d, info = split
    ds = D.ReviewDataset(d, "train")
    R, T = info["rv_num"], info["rv_len"]
    today = D.DeviceReviewCache(ds, "cpu")
    same = D.DeviceReviewCache(ds, "cpu", pool=None)
    wide = D.DeviceReviewCache(ds, "cpu", pool=7)
    names = ("user_table", "user_rid_table", "item_table", "item_rid_table", "user", "item", "user_rids", "item_rids")
    for c in (same, wide):
        for n in names:
            a, b = getattr(today, n), getattr(c, n)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), n
        assert c.user_table.is_contiguous() and c.item_rid_table.is_contiguous()
    assert today.user_table.shape == (info["user_num"], R + 1, T)
    # pool = None holds nothing more: the sampler's tables ARE the plain ones
    assert same.user_pool_table.data_ptr() == same.user_table.data_ptr() and same.item_pool_rid_table is same.item_rid_table
    assert wide.user_pool_table.shape == (info["user_num"], 8, T) and wide.item_pool_rid_table.shape == (info["item_num"], 8)
    assert torch.equal(wide.user_pool_table[:, :R + 1], today.user_table)
    assert wide.user_pool_rid_table[4, :R + 3].tolist() == ds.user_rids[4][:R + 3]      # user 4 wrote R + 3 reviews: all resident
    u = torch.tensor([p[0] for p in info["pairs"]])
    i = torch.tensor([p[1] for p in info["pairs"]])
    for loo in (True, False):                                    # the plain gather reads the first R + 1 slots only
        for a, b in zip(today.gather(u, i, loo), wide.gather(u, i, loo)):
            assert torch.equal(a, b)
    for bad in (R - 1, 64, True, 5.0):
        with pytest.raises(ValueError, match="pool"):
            D.DeviceReviewCache(ds, "cpu", pool=bad)


def test_wrapped_in_a_negative_feed_the_sampled_feed_keeps_its_protocol(split):
    from review_based_recommender_amd import data as D
    d, info = split
    cache = D.DeviceReviewCache(D.ReviewDataset(d, "train"), "cpu", pool=6)
    feed = cache.sampled_feed("simple_siamese", 2, 2, seed=4)
    inb = D.InBatchFeed(feed, None)
    u, i = torch.tensor([1, 4, 5]), torch.tensor([1, 2, 2])
    got = inb.gather(u, i)
    want = _ref_of(cache, u, i, 2, 2, 4, 0)
    assert torch.equal(got["revs"], torch.from_numpy(want["revs"])) and int(feed.state[0]) == 1
    assert [t.shape for t in inb.empty_inputs(3)] == [t.shape for t in feed.empty_inputs(3)]


# ------------------------------------------------------------------------------------------------ trainer, C entry
def test_trainer_config_errors_give_the_reason(tmp_path):
    from review_based_recommender_amd.trainer import DEFAULTS, Args, ReviewExperiment, _feed_states
    assert DEFAULTS["sample_train_review"] is False
    assert all(DEFAULTS[k] is None for k in ("u_rv_num", "i_rv_num", "review_pool", "review_sample_seed"))
    base = {"data_dir": str(tmp_path), "sample_train_review": True}
    for kind in ("narre", "simple_siamese"):
        with pytest.raises(ValueError, match="device_reviews"):
            ReviewExperiment(kind, Args(dict(base)))
        with pytest.raises(ValueError, match="parallel"):
            ReviewExperiment(kind, Args(dict(base, device_reviews=True, parallel=True)))
        for key, bad in (("u_rv_num", 0), ("i_rv_num", -1), ("u_rv_num", True), ("i_rv_num", 2.0), ("review_pool", 0),
                         ("review_pool", 64)):
            with pytest.raises(ValueError, match=key):
                ReviewExperiment(kind, Args(dict(base, device_reviews=True, **{key: bad})))
    for kind in ("deepconn", "dual_att"):                       # no device_reviews for the doc split: no sampling either
        with pytest.raises(ValueError):
            ReviewExperiment(kind, Args(dict(base)))
        with pytest.raises(ValueError):
            ReviewExperiment(kind, Args(dict(base, device_reviews=True)))
    # the call numbers a recording must put back: the wrapper's and the wrapped sampler's
    inner = types.SimpleNamespace(state="inner")
    assert _feed_states(types.SimpleNamespace(state="outer", feed=inner)) == ["outer", "inner"]
    assert _feed_states(types.SimpleNamespace(feed=inner)) == ["inner"] and _feed_states(object()) == []


def test_header_binding_and_library_declare_the_entry_and_it_refuses_bad_arguments():
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rbr_hip.h")) as f:
        header = f.read()
    assert "int rbr_review_sample_gather(" in header and "train_simple_siamese.py:346-368" in header
    with open(os.path.join(root, "review-based-recommender_amd", "csrc", "review_sample.hip")) as f:
        assert "train_simple_siamese.py:346-368" in f.read()
    assert len(_lib.SIGNATURES["rbr_review_sample_gather"][1]) == 27
    L = _lib.lib()
    fn = L.rbr_review_sample_gather
    buf = (C.c_int64 * 8)()                                      # never dereferenced: every call below is refused on the host
    p64 = C.cast(buf, C.POINTER(C.c_int64))
    p32 = C.cast(buf, C.POINTER(C.c_int32))
    p8 = C.cast(buf, C.POINTER(C.c_uint8))
    pv = C.cast(buf, C.c_void_p)

    def call(B=2, R=3, T=4, P=5, U=6, I=7, loo=1, n_u=2, n_i=3, replace=0, null=False):
        a, b, c, v = (None, None, None, None) if null else (p64, p32, p8, pv)
        return fn(B, R, T, P, a, a, b, b, U, b, b, I, loo, n_u, n_i, 0, replace, 0, v, a, c, None, None, None, None, a, None)

    for kw, msg in (({"B": 0}, b"bad shape"), ({"R": 0}, b"bad shape"), ({"T": -1}, b"bad shape"), ({"U": 0}, b"bad shape"),
                    ({"I": 0}, b"bad shape"), ({"loo": 2}, b"bad shape"), ({"P": 2}, b"pool"), ({"P": 64}, b"pool"),
                    ({"R": 63, "P": 63, "n_u": 64}, b"keep counts"), ({"n_u": 0}, b"keep counts"), ({"n_i": 4}, b"keep counts"),
                    ({"n_i": 0}, b"keep counts"), ({"replace": -1}, b"replace_id"), ({"replace": 6}, b"replace_id"),
                    ({"null": True}, b"null pointer")):
        assert call(**kw) == -1 and msg in L.rbr_last_error(), (kw, L.rbr_last_error())
