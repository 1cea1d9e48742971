"""rbr_review_sample_gather on the GPU against the integer restatement of its draw (tests/review_sample_ref.py): every output
must be the same integers at every shape that takes another path, the call number must advance by one per launch -- also for a
launch replayed from a graph -- and the recorded id-fed step over the sampled feed must train like an example-fed step on the
restated batches, with no launch more than the plain id-fed step."""
import types

import numpy as np
import pytest
import torch

import make_review_dataset
import review_sample_ref as ref
import synth
from test_review_feed_gpu import NARRE_KEYS, SIAMESE_KEYS, _check_params, _narre, _rel, _siamese

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = ("revs", "word_masks", "rev_masks", "rids", "ids", "slots")
N_IDS = 12          # rows of every hand-made table
OTHER = 10          # the counterpart id of the hand-made pairs


def _crafted(rng, P, T):
    """Hand-made tables of N_IDS ids per side and the pairs that reach every rule of the draw (the user side carries the cases;
    the item side is random, with some rows that list the user)."""
    ur, ud = ref.random_tables(rng, N_IDS, P, T)
    ir, idd = ref.random_tables(rng, N_IDS, P, T)

    def fill(a, rids):
        ud[a] = 0
        ur[a] = 0
        ud[a, :len(rids)] = rids
        ur[a, :len(rids)] = rng.integers(1, 40, size=(len(rids), T))

    others = lambda k: [int(x) for x in rng.integers(1, OTHER, size=k)]     # never OTHER itself
    fill(1, others(P + 1))                                     # counterpart absent from the rid list: d = P
    fill(2, [OTHER] + others(P))                               # counterpart at slot 0
    fill(3, others(P - 1) + [OTHER] + others(1))               # counterpart at slot P - 1
    twice = others(P + 1)
    twice[P // 2] = twice[P - 1] = OTHER                       # listed twice (once where P = 1): the first match wins
    fill(4, twice)
    fill(5, others(max(P // 2, 1)))                            # with counterpart 0: the unused slots' rid 0 is no match
    fill(6, [OTHER])                                           # the only review is the pair's own
    fill(7, [OTHER] + others(1))                               # fewer live reviews than n (one, once its own is left out)
    fill(8, others(min(P + 1, 4)))
    ur[8, min(P, 1)] = 0                                       # an empty review in the middle of a list: dead, rid kept
    fill(9, others(P) + [OTHER])                               # counterpart only at slot P: beyond the P that are compared
    pairs = [(0, OTHER), (1, OTHER), (2, OTHER), (3, OTHER), (4, OTHER), (5, 0), (6, OTHER), (7, OTHER), (8, OTHER), (9, OTHER),
             (N_IDS, OTHER), (1, -3), (11, 11)]                # ... id 0 (all empty), ids outside their table, a random row
    u = np.array([p[0] for p in pairs], dtype=np.int64)
    i = np.array([p[1] for p in pairs], dtype=np.int64)
    return (ur, ud, ir, idd), u, i


def _dev(tabs, offset=False):
    """The four tables on the device; offset: each as a view 4 bytes into its buffer (no 16-byte alignment)."""
    out = []
    for t in tabs:
        t = torch.from_numpy(t)
        if offset:
            buf = torch.zeros(t.numel() + 1, dtype=torch.int32)
            buf[1:] = t.reshape(-1)
            d = buf.to(DEV)[1:].view(t.shape)
            assert d.data_ptr() % 16 == 4 and d.is_contiguous()
        else:
            d = t.to(DEV)
            assert d.data_ptr() % 16 == 0
        out.append(d)
    return out


def _state(call):
    return torch.tensor([call, 0], dtype=torch.int64, device=DEV)


def _launch(dtabs, u, i, R, n_u, n_i, seed, call, **kw):
    from review_based_recommender_amd import functional as RF
    state = _state(call)
    kw.setdefault("slots", True)
    got = RF.review_sample_gather(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), dtabs[0], dtabs[1], dtabs[2], dtabs[3],
                                  R, n_u, n_i, state=state, seed=seed, **kw)
    torch.cuda.synchronize()
    return dict(zip(NAMES, got)), state


def _same(got, want, where=None):
    for k in NAMES:
        if got[k] is not None:
            w = torch.from_numpy(want[k])
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, where)
            assert torch.equal(got[k].cpu(), w), (k, where)


def _id_errors(expect):
    """The id record holds `expect` offenders; it is cleared for the next test."""
    from review_based_recommender_amd import functional as RF
    assert int(RF._id_err(DEV).cpu()[0]) == expect
    if expect:
        with pytest.raises(IndexError):
            RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("T", [1, 3, 4, 50, 52])
@pytest.mark.parametrize("R,P", [(1, 1), (3, 3), (3, 7), (4, 63)])
def test_every_rule_of_the_draw_at_every_path(R, P, T):
    """The hand-made rows, all outputs: scalar path (T % 4 != 0) and vector path, P + 1 = 64 lanes, n_user != n_item, n = 1 and
    n = R, with and without leave-one-out; at T % 4 == 0 also from tables 4 bytes off, where the vector path must fall back."""
    _id_errors(0)
    rng = np.random.default_rng(1000 * R + 10 * P + T)
    tabs, u, i = _crafted(rng, P, T)
    for offset in ((False, True) if T % 4 == 0 else (False,)):
        dtabs = _dev(tabs, offset)
        for n_u, n_i, loo, seed, call in ((R, 1, True, 5, 0), (1, R, True, 2**40 + 3, 2**33 + 1), (max(R - 1, 1), R, False, 0, 7)):
            got, state = _launch(dtabs, u, i, R, n_u, n_i, seed, call, leave_one_out=loo)
            want = ref.gather_ref(u, i, *tabs, R, n_u, n_i, seed, call, leave_one_out=loo)
            _same(got, want, (offset, n_u, n_i, loo))
            assert state.tolist() == [call + 1, 0]
            assert want["bad"] == 2
            _id_errors(2)                                       # as the plain gather records them; row 0 stood in
            assert not got["revs"][10].any() and int(got["ids"][10]) == 0 and int(got["ids"][len(u) + 11]) == 0
            if loo:                                             # the cases are what they claim to be
                s = want["slots"]
                assert (s[0] == -1).all() and (s[6] == -1).all()                     # id 0; the only review is the pair's own
                assert 0 not in s[2] and P - 1 not in s[3] and P // 2 not in s[4]    # the left-out slots
                assert (s[7] >= 0).sum() == 1                                        # one live review for n >= 1 kept
                assert 1 not in s[8].tolist()                                        # the empty review is never drawn
                assert (s[5] >= 0).sum() == min(n_u, max(P // 2, 1))                 # counterpart 0: nothing left out


GRIDS = [(B, R, P, T) for R, P, T in ((3, 7, 3), (3, 7, 4), (4, 63, 52)) for B in (1, 3, 5, 130)] + [(2100, 3, 7, 3), (2100, 3, 7, 4)]


@pytest.mark.parametrize("B,R,P,T", GRIDS)
def test_batches_of_every_grid_shape(B, R, P, T):
    """A cut last workgroup (4 rows each), several workgroups -- the ticket has several takers -- and, at 2 * 2100 rows over
    the 1024 workgroups of the largest grid, the grid-stride round (at the two small shapes, one per path)."""
    _id_errors(0)
    rng = np.random.default_rng(B * 7 + P)
    tabs, cu, ci = _crafted(rng, P, T)
    pick = rng.permutation(3 * len(cu))                         # the hand-made pairs among twice as many random ones
    u = np.resize(np.concatenate([cu, rng.integers(0, N_IDS, size=2 * len(cu))])[pick], B)
    i = np.resize(np.concatenate([ci, rng.integers(0, N_IDS, size=2 * len(ci))])[pick], B)
    dtabs = _dev(tabs)
    got, state = _launch(dtabs, u, i, R, 2, R, 11, 3)
    want = ref.gather_ref(u, i, *tabs, R, 2, R, 11, 3)
    _same(got, want, B)
    assert state.tolist() == [4, 0]
    _id_errors(want["bad"])


def test_outputs_left_out_and_bytes_around_the_outputs():
    """Every nullable output omitted; and outputs written into views one element into their buffers (no alignment for the vector
    path at T % 4 == 0): nothing outside the views changes."""
    R, P, T = 3, 7, 4
    rng = np.random.default_rng(4)
    tabs, u, i = _crafted(rng, P, T)
    u, i = u[:10], i[:10]                                       # ids inside their tables only
    dtabs = _dev(tabs)
    want = ref.gather_ref(u, i, *tabs, R, 2, 3, 1, 0)
    for leave in ("rev_masks", "rids", "ids", "slots"):
        got, _ = _launch(dtabs, u, i, R, 2, 3, 1, 0, **{leave: None})
        assert got[leave] is None
        _same(got, want, leave)
    got, _ = _launch(dtabs, u, i, R, 2, 3, 1, 0, rev_masks=False, rids=False, ids=False, slots=False)
    assert [got[k] for k in NAMES[2:]] == [None] * 4
    _same(got, want)
    B2 = 2 * len(u)
    n = B2 * R * T
    rbuf = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    mbuf = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((B2 * R + 2,), 77, dtype=torch.int32, device=DEV)
    kbuf = torch.full((B2 * R + 2,), 0xAB, dtype=torch.uint8, device=DEV)
    revs, wm = rbuf[1:n + 1].view(B2, R, T), mbuf[1:n + 1].view(torch.bool).view(B2, R, T)
    slots, rm = sbuf[1:-1].view(B2, R), kbuf[1:-1].view(torch.bool).view(B2, R)
    assert revs.data_ptr() % 16 == 8 and wm.data_ptr() % 4 == 1
    got, _ = _launch(dtabs, u, i, R, 2, 3, 1, 0, revs=revs, word_masks=wm, slots=slots, rev_masks=rm)
    assert got["revs"].data_ptr() == revs.data_ptr() and got["slots"].data_ptr() == slots.data_ptr()
    _same(got, want)
    for buf, v in ((rbuf, -7), (mbuf, 0xAB), (sbuf, 77), (kbuf, 0xAB)):
        assert buf[0].item() == v and buf[-1].item() == v
    _id_errors(0)


def test_functional_refuses_bad_arguments():
    from review_based_recommender_amd import functional as RF
    rng = np.random.default_rng(0)
    tabs, u, i = _crafted(rng, 7, 4)
    d = _dev(tabs)
    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    for R, n_u, n_i, kw, msg in ((8, 1, 1, {}, "pool"), (3, 0, 1, {}, "keep counts"), (3, 1, 4, {}, "keep counts"),
                                 (3, 1, 1, {"replace_id": N_IDS}, "replace_id")):
        with pytest.raises(RuntimeError, match=msg):
            RF.review_sample_gather(ud, idv, *d, R, n_u, n_i, state=_state(0), **kw)
    with pytest.raises(RuntimeError, match="state"):
        RF.review_sample_gather(ud, idv, *d, 3, 1, 1, state=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="slots"):
        RF.review_sample_gather(ud, idv, *d, 3, 1, 1, state=_state(0), slots=torch.zeros(2 * len(u), 3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        RF.review_sample_gather(ud, idv[:2], *d, 3, 1, 1, state=_state(0))


# ------------------------------------------------------------------------------------------------ 2. the feed
_SPLITS = {}


def _split(cfg, pool):
    """(cache on the GPU, the pool tables as numpy, train examples), built once per shape and left unchanged."""
    from review_based_recommender_amd import data as D
    key = (cfg["U"], cfg["I"], cfg["V"], cfg["R"], cfg["T"], pool)
    if key not in _SPLITS:
        meta, train, _ = make_review_dataset.random_split(cfg["U"], cfg["I"], cfg["V"], cfg["R"], cfg["T"], 9 * cfg["U"], 8, seed=3)
        cache = D.DeviceReviewCache(types.SimpleNamespace(**meta), DEV, pool=pool)
        tabs = tuple(t.cpu().numpy() for t in (cache.user_pool_table, cache.user_pool_rid_table, cache.item_pool_table,
                                               cache.item_pool_rid_table))
        assert (tabs[1][:, cfg["R"] + 1:] != 0).any()           # some id has more reviews than the plain tables hold
        _SPLITS[key] = (cache, tabs, train)
    return _SPLITS[key]


def _pairs(train, rng, B):
    picks = [train[k] for k in rng.choice(len(train), size=B, replace=False)]
    return (torch.tensor([e[0] for e in picks]), torch.tensor([e[1] for e in picks]),
            torch.tensor([e[2] for e in picks], dtype=torch.float32))


def _model_args(want, order, B):
    return [torch.from_numpy(want[k][h * B:(h + 1) * B]) for k in order for h in (0, 1)]


def test_call_protocol_eager_reseeded_and_replayed():
    """Two eager launches are calls 0 and 1, reseed(seed, 5) gives call 5, and a launch captured once and replayed three times
    gives three consecutive calls; the ticket is back at 0 after every launch."""
    cfg = synth.SIAMESE_CFGS["tiny"]
    R = cfg["R"]
    cache, tabs, train = _split(cfg, R + 3)
    feed = cache.sampled_feed("simple_siamese", 2, R - 1, seed=21)
    B = 6                                                       # 12 rows: three workgroups take tickets
    u, i, _ = _pairs(train, np.random.default_rng(1), B)

    def want(call):
        return ref.gather_ref(u.numpy(), i.numpy(), *tabs, R, 2, R - 1, 21, call)

    for call in (0, 1):
        got = feed.gather(u, i, slots=True)
        torch.cuda.synchronize()
        _same(got, want(call), call)
        assert feed.state.tolist() == [call + 1, 0]
    feed.reseed(21, 5)
    _same(feed.gather(u, i, slots=True), want(5), 5)
    assert feed.state.tolist() == [6, 0]
    # captured: the launch reads the call number from the device at every replay
    views = feed.empty_inputs(B)
    slots = torch.zeros(2 * B, R, dtype=torch.int32, device=DEV)
    ud, idv = u.to(DEV), i.to(DEV)
    stacked = {k: torch.zeros((2 * B, *views[2 * n].shape[1:]), dtype=views[2 * n].dtype, device=DEV)
               for n, k in enumerate(feed.order)}
    from review_based_recommender_amd import functional as RF
    RF._id_err(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.sample_gather(ud, idv, 2, R - 1, 21, feed.state, revs=stacked["revs"], word_masks=stacked["word_masks"],
                            rev_masks=stacked["rev_masks"], rids=None, ids=stacked["ids"], slots=slots)
    feed.reseed(21, 40)
    for s in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = dict(stacked, rids=None, slots=slots)
        _same(got, want(40 + s), s)
        assert feed.state.tolist() == [41 + s, 0]
    _id_errors(0)


@pytest.mark.parametrize("kind,order", [("narre", NARRE_KEYS), ("simple_siamese", SIAMESE_KEYS)])
def test_sampled_gather_into_a_block_leaves_the_bytes_outside_its_views_untouched(kind, order):
    """The input block of a recorded step: the sampled feed writes through adjacent (user, item) views and nowhere else."""
    from review_based_recommender_amd.train_step import _flat_layout, _flat_views
    cfg = (synth.NARRE_CFGS if kind == "narre" else synth.SIAMESE_CFGS)["tiny"]
    R, B = cfg["R"], 5
    cache, tabs, train = _split(cfg, R + 3)
    feed = cache.sampled_feed(kind, R, 2, seed=8)
    like = feed.empty_inputs(B)
    layout = _flat_layout(list(like))
    guard = 256
    flat = torch.full((layout[-1] + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    views = _flat_views(flat[guard:guard + layout[-1]], layout, list(like))
    u, i, _ = _pairs(train, np.random.default_rng(2), B)
    feed.gather(u, i, out=views)
    torch.cuda.synchronize()
    want = ref.gather_ref(u.numpy(), i.numpy(), *tabs, R, R, 2, 8, 0)
    for v, w in zip(views, _model_args(want, order, B)):
        assert v.dtype == w.dtype and torch.equal(v.cpu(), w)
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for o, t in zip(layout, like):
        covered[guard + o:guard + o + t.numel() * t.element_size()] = True
    assert bool((flat.cpu()[~covered] == 0xAB).all())
    feed.reseed(8, 0)                                           # the eager inputs() are the same batch
    for v, w in zip(feed.inputs(u, i), _model_args(want, order, B)):
        assert torch.equal(v.cpu(), w)


def test_the_sampled_feed_inside_a_negative_feed():
    """NegativeFeed wraps it by protocol: the expanded batch is the restatement applied to the sampler's u_out / i_out."""
    from review_based_recommender_amd import data as D
    cfg = synth.SIAMESE_CFGS["tiny"]
    R = cfg["R"]
    cache, tabs, train = _split(cfg, R + 3)
    feed = cache.sampled_feed("simple_siamese", 2, 2, seed=13)
    neg = D.NegativeFeed(feed, None, cfg["I"], n_neg=1, seed=3)
    B = 4
    u, i, _ = _pairs(train, np.random.default_rng(3), B)
    assert [t.shape[0] for t in neg.empty_inputs(B)] == [2 * B] * 8
    got = neg.gather(u, i)
    torch.cuda.synchronize()
    uo, io = neg.u_out.cpu().numpy(), neg.i_out.cpu().numpy()
    assert uo.shape == (2 * B,) and (uo[:B] == u.numpy()).all() and (io[:B] == i.numpy()).all()
    want = ref.gather_ref(uo, io, *tabs, R, 2, 2, 13, 0)
    for k in SIAMESE_KEYS:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    assert feed.state.tolist() == [1, 0] and neg.state.tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ 3. the recorded step
@pytest.mark.parametrize("kind", ["simple_siamese", "narre"])
def test_recorded_step_over_the_sampled_feed_matches_the_example_fed_step_on_the_restated_batches(kind, capsys):
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    cfg = (synth.NARRE_CFGS if kind == "narre" else synth.SIAMESE_CFGS)["tiny"]
    make = (lambda: _narre(cfg)) if kind == "narre" else (lambda: _siamese(cfg))
    order = NARRE_KEYS if kind == "narre" else SIAMESE_KEYS
    R, B, n_steps = cfg["R"], cfg["B"], 3
    n_u, n_i, seed = 2, R - 1, 17
    cache, tabs, train = _split(cfg, R + 3)
    rng = np.random.default_rng(5)
    batches = [_pairs(train, rng, B) for _ in range(n_steps + 1)]
    m_e, m_i, m_p = make(), make(), make()
    o_e, o_i, o_p = (make_optimizer(m, capturable=True, hip_clip_adam=True) for m in (m_e, m_i, m_p))
    feed = cache.sampled_feed(kind, n_u, n_i, seed=seed)
    u0, i0, r0 = batches[-1]                                    # recorded on pairs that are not replayed
    w0 = ref.gather_ref(u0.numpy(), i0.numpy(), *tabs, R, n_u, n_i, seed, 0)
    st_e = GraphedTrainStep(m_e, o_e, [t.to(DEV) for t in _model_args(w0, order, B)], r0.to(DEV), slots=2, keep_graph=True)
    st_i = GraphedTrainStep.from_ids(m_i, o_i, feed, u0.to(DEV), i0.to(DEV), r0.to(DEV), slots=2, keep_graph=True)
    st_p = GraphedTrainStep.from_ids(m_p, o_p, cache.feed(kind, True), u0.to(DEV), i0.to(DEV), r0.to(DEV), slots=2, keep_graph=True)
    for a, b in zip(m_e.parameters(), m_i.parameters()):
        assert torch.equal(a, b)
    feed.reseed(seed, 0)                                        # the recording's warm-up launches drew, too
    for k, (u, i, r) in enumerate(batches[:n_steps]):
        s = k % 2
        want = ref.gather_ref(u.numpy(), i.numpy(), *tabs, R, n_u, n_i, seed, k)
        st_e.stage(s, [t.to(DEV) for t in _model_args(want, order, B)], r.to(DEV))
        st_i.stage(s, (u, i), r)
        le, ge, pe = st_e(slot=s)
        li, gi, pi = st_i(slot=s)
        torch.cuda.synchronize()
        for a, b in zip(st_i.slot_batch(s), st_e.slot_batch(s)):     # what the sampling gather wrote = the restated batch
            assert a.dtype == b.dtype and torch.equal(a, b), k
        assert _rel(li, le) <= 1e-5 and _rel(gi, ge) <= 1e-5, (k, float(li), float(le), float(gi), float(ge))
        assert float((pi - pe).abs().max()) <= 1e-5 * max(1.0, float(pe.abs().max())), k
    assert feed.state.tolist() == [n_steps, 0]
    _check_params(m_e, m_i)
    n_p, n_s = st_p.kernel_launches(), st_i.kernel_launches()
    with capsys.disabled():
        print(f"\n{kind}: launches per id-fed step, plain {n_p} -> sampled {n_s}")
    if n_p is not None and n_s is not None:
        assert n_s == n_p, (n_p, n_s)
    _id_errors(0)
