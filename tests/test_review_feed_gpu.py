"""The id-fed review split on the GPU: rbr_review_gather against the examples' own collate, the recorded id-fed step and eval
forward against the example-fed ones on the same pairs, and the trainer's `device_reviews` against its example-fed loop."""
import json
import math
import types

import numpy as np
import pytest
import torch

import make_review_dataset
import synth
from helpers import quiet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

NARRE_KEYS = ("revs", "word_masks", "ids", "rids")
SIAMESE_KEYS = ("revs", "word_masks", "rev_masks", "ids")


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(1.0, abs(b))


def _collate(examples):
    """ReviewDataset.collate_fn of the examples, as a dict of stacked tensors (user rows first) plus the ratings."""
    from review_based_recommender_amd import data as D
    b = D.ReviewDataset.collate_fn(types.SimpleNamespace(feed="examples"), [e[:7] for e in examples])
    wm = torch.cat([b[2], b[3]])
    return dict(revs=torch.cat([b[0], b[1]]), word_masks=wm, rev_masks=wm.any(-1), ids=torch.cat([b[4], b[5]]),
                rids=torch.cat([b[6], b[7]]), u_ids=b[4], i_ids=b[5], ratings=b[8])


def _model_args(c, order):
    """The stacked dict as the model's eight arguments."""
    B = c["u_ids"].shape[0]
    return [half for k in order for half in (c[k][:B], c[k][B:])]


_SPLITS = {}


def _split(U, I, V, R, T, n_train, seed=0):
    """(cache on the GPU, cache on the cpu, train examples, valid examples), built once per shape and left unchanged."""
    from review_based_recommender_amd import data as D
    key = (U, I, V, R, T, n_train, seed)
    if key not in _SPLITS:
        meta, train, valid = make_review_dataset.random_split(U, I, V, R, T, n_train, 48, seed)
        ds = types.SimpleNamespace(**meta)
        _SPLITS[key] = (D.DeviceReviewCache(ds, DEV), D.DeviceReviewCache(ds, "cpu"), train, valid)
    return _SPLITS[key]


# ------------------------------------------------------------------------------------------------ 1. the kernel
SHAPES = [(1, 1, 1), (3, 1, 3), (3, 4, 8), (5, 4, 6), (7, 3, 12)]


def _gather(cache, u, i, loo, **kw):
    from review_based_recommender_amd import functional as RF
    return RF.review_gather(u.to(DEV), i.to(DEV), cache.user_table, cache.user_rid_table, cache.item_table, cache.item_rid_table,
                            loo, **kw)


@pytest.mark.parametrize("B,R,T", SHAPES)
@pytest.mark.parametrize("loo", [True, False])
def test_review_gather_is_bit_equal_to_the_examples_collate(B, R, T, loo):
    """Every batch of B consecutive examples of the split (train under leave-one-out, valid without), all five outputs."""
    _parity(B, R, T, loo, 30)


# beyond the small shapes: several blocks (320 reviews at 64 per block), and reviews wider than one 64-lane group on either path
# (70 tokens one by one; 65 four-token chunks), where a lane takes a second unit
@pytest.mark.parametrize("B,R,T", [(40, 4, 12), (9, 2, 70), (4, 2, 260)])
@pytest.mark.parametrize("loo", [True, False])
def test_review_gather_beyond_one_block_and_one_group(B, R, T, loo):
    _parity(B, R, T, loo, 60)


def _parity(B, R, T, loo, n_train):
    from review_based_recommender_amd import functional as RF
    cache, cpu, train, valid = _split(7, 7, 40, R, T, n_train)
    examples = train if loo else valid
    if loo:      # the split exercises the rule: dropped slots inside and beyond the R that the kernel scans, and repeated pairs
        rows = [(_rids_of(cpu, 0, e[0]), e[1]) for e in train]
        d = {row.index(i) if i in row else R for row, i in rows}
        assert {0, R - 1, R} <= d, d
    RF.check_id_errors(DEV)
    for s in range(0, len(examples) - B + 1, B):
        want = _collate(examples[s:s + B])
        got = _gather(cache, want["u_ids"], want["i_ids"], loo)
        torch.cuda.synchronize()
        for name, g in zip(("revs", "word_masks", "rev_masks", "rids", "ids"), got):
            assert g.dtype == want[name].dtype and g.shape == want[name].shape, name
            assert torch.equal(g.cpu(), want[name]), (name, s)
    RF.check_id_errors(DEV)                                                   # no id was out of range
    # train pairs under the valid rule (and the reverse) have no examples: the cpu restatement is the cross-check there
    other = _collate((valid if loo else train)[:B])
    got = _gather(cache, other["u_ids"], other["i_ids"], loo)
    ref = cpu.gather(other["u_ids"], other["i_ids"], loo)
    for g, r in zip(got, ref):
        assert torch.equal(g.cpu(), r)


def _rids_of(cache, side, idx):
    return (cache.user_rid_table if side == 0 else cache.item_rid_table)[idx, :cache.rv_num].tolist()


@pytest.mark.parametrize("B,R,T", SHAPES)
def test_review_gather_forms(B, R, T):
    """Outputs left out one at a time, a misaligned output view (the one-token path at T % 4 == 0 too), and ids outside their
    table: row 0 stands in, and check_id_errors raises once."""
    from review_based_recommender_amd import functional as RF
    cache, cpu, train, _ = _split(7, 7, 40, R, T, 30)
    want = _collate(train[:B])
    u, i = want["u_ids"], want["i_ids"]
    RF.check_id_errors(DEV)
    for leave in ("rev_masks", "rids", "ids"):
        kw = {leave: None}
        got = dict(zip(("revs", "word_masks", "rev_masks", "rids", "ids"), _gather(cache, u, i, True, **kw)))
        assert got[leave] is None
        for name, g in got.items():
            assert g is None or torch.equal(g.cpu(), want[name]), (leave, name)
    got = _gather(cache, u, i, True, rev_masks=False, rids=False, ids=False)
    assert got[2:] == (None, None, None) and torch.equal(got[0].cpu(), want["revs"]) and torch.equal(got[1].cpu(), want["word_masks"])
    # views one element into their buffers: 8-byte-aligned int64 rows, 1-byte-aligned masks
    n = 2 * B * R * T
    rbuf = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    mbuf = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device=DEV)
    revs, wm = rbuf[1:n + 1].view(2 * B, R, T), mbuf[1:n + 1].view(torch.bool).view(2 * B, R, T)
    assert revs.data_ptr() % 16 == 8 and wm.data_ptr() % 4 == 1
    got = _gather(cache, u, i, True, revs=revs, word_masks=wm)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == revs.data_ptr() and got[1].data_ptr() == wm.data_ptr()
    for name, g in zip(("revs", "word_masks", "rev_masks", "rids", "ids"), got):
        assert torch.equal(g.cpu(), want[name]), name
    assert rbuf[0].item() == -7 and rbuf[-1].item() == -7 and mbuf[0].item() == 0xAB and mbuf[-1].item() == 0xAB
    # ids outside their table
    bad_u, bad_i = u.clone(), i.clone()
    bad_u[0] = cache.user_table.shape[0]
    bad_i[-1] = -3
    got = _gather(cache, bad_u, bad_i, True)
    torch.cuda.synchronize()
    ok_u, ok_i = bad_u.clone(), bad_i.clone()
    ok_u[0] = 0
    ok_i[-1] = 0
    ref = cpu.gather(ok_u, ok_i, True)
    # a replaced id is the padding id, which never matches: its partner keeps all its reviews
    for name, g, r in zip(("revs", "word_masks", "rev_masks", "rids", "ids"), got, ref):
        assert torch.equal(g.cpu(), r), name
    assert not got[0][0].any() and not got[0][2 * B - 1].any() and int(got[4][0]) == 0 and int(got[4][2 * B - 1]) == 0
    assert int(RF._id_err(DEV).cpu()[0]) == 2
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)


def test_review_gather_refuses_bad_arguments():
    from review_based_recommender_amd import functional as RF
    cache, _, train, _ = _split(7, 7, 40, 4, 8, 30)
    want = _collate(train[:3])
    u, i = want["u_ids"].to(DEV), want["i_ids"].to(DEV)
    with pytest.raises(RuntimeError):
        _gather(cache, want["u_ids"], want["i_ids"][:2], True)
    with pytest.raises(RuntimeError):
        _gather(cache, want["u_ids"], want["i_ids"], True, revs=torch.empty(6, 4, 7, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        _gather(cache, want["u_ids"], want["i_ids"], True, rids=torch.empty(6, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="replace_id"):
        RF.review_gather(u, i, cache.user_table, cache.user_rid_table, cache.item_table, cache.item_rid_table, True, 0, 7)


@pytest.mark.parametrize("kind,order", [("narre", NARRE_KEYS), ("simple_siamese", SIAMESE_KEYS)])
def test_gather_into_a_block_leaves_the_bytes_outside_its_views_untouched(kind, order):
    """The input block of a recorded step: the feed writes through adjacent (user, item) views and nowhere else."""
    from review_based_recommender_amd.train_step import _flat_layout, _flat_views
    B, R, T = 5, 4, 6
    cache, _, train, _ = _split(7, 7, 40, R, T, 30)
    feed = cache.feed(kind, True)
    like = feed.empty_inputs(B)
    layout = _flat_layout(list(like))
    guard = 256
    flat = torch.full((layout[-1] + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    views = _flat_views(flat[guard:guard + layout[-1]], layout, list(like))
    want = _collate(train[3:3 + B])
    feed.gather(want["u_ids"], want["i_ids"], out=views)
    torch.cuda.synchronize()
    for v, w in zip(views, _model_args(want, order)):
        assert v.dtype == w.dtype and torch.equal(v.cpu(), w)
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for o, t in zip(layout, like):
        covered[guard + o:guard + o + t.numel() * t.element_size()] = True
    assert bool((flat.cpu()[~covered] == 0xAB).all())
    # the eager inputs() are the same batch
    for v, w in zip(feed.inputs(want["u_ids"], want["i_ids"]), _model_args(want, order)):
        assert torch.equal(v.cpu(), w)


# ------------------------------------------------------------------------------------------------ 2. the recorded step
def _narre(cfg):
    from review_based_recommender_amd.models.narre.narre import NARRE
    c = cfg
    m = quiet(NARRE, c["U"], c["I"], c["V"], c["kz"], c["H"], c["D"], c["A"], c["K"], c["R"], c["T"], 0.0, 0, 0, 0, None, "CNN")
    m.load_state_dict(synth.narre_params(cfg, 0))
    m.validate_ids = False
    return m.to(DEV).train()


def _siamese(cfg):
    from review_based_recommender_amd.models.simple_siamese.simple_siamese import SimpleSiamese
    c = cfg
    m = quiet(SimpleSiamese, c["D"], c["K"], c["V"], c["U"], c["I"], None, False, 0.0, 0.0, 0.0, c["UB"], c["LT"])
    m.load_state_dict(synth.siamese_params(cfg, 0))
    m.validate_ids = False
    return m.to(DEV).train()


def _check_params(m_a, m_b, lr=2e-3):
    """helpers.check_params_after's gates: lr/2 max, 1e-4 RMS."""
    for (n, a), b in zip(m_a.named_parameters(), m_b.parameters()):
        d = (a.detach() - b.detach()).double()
        assert float(d.abs().max()) <= lr / 2, n
        assert float(d.pow(2).mean().sqrt()) <= 1e-4, n


MODELS = [("narre", "tiny"), ("narre", "small"), ("simple_siamese", "tiny"), ("simple_siamese", "small")]


def _setup(kind, name):
    cfg = (synth.NARRE_CFGS if kind == "narre" else synth.SIAMESE_CFGS)[name]
    make = (lambda: _narre(cfg)) if kind == "narre" else (lambda: _siamese(cfg))
    order = NARRE_KEYS if kind == "narre" else SIAMESE_KEYS
    cache, _, train, valid = _split(cfg["U"], cfg["I"], cfg["V"], cfg["R"], cfg["T"], 5 * cfg["U"], seed=3)
    return cfg, make, order, cache, train, valid


@pytest.mark.parametrize("kind,name", MODELS)
def test_id_fed_step_matches_the_example_fed_step(kind, name, capsys):
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    cfg, make, order, cache, train, _ = _setup(kind, name)
    B, n_steps = cfg["B"], 3
    rng = np.random.default_rng(5)
    picks = [[train[k] for k in rng.choice(len(train), size=B, replace=False)] for _ in range(n_steps + 1)]
    batches = [_collate(p) for p in picks]
    m_e, m_i = make(), make()
    o_e = make_optimizer(m_e, capturable=True, hip_clip_adam=True)
    o_i = make_optimizer(m_i, capturable=True, hip_clip_adam=True)
    c0 = batches[-1]                                              # recorded on pairs that are not replayed
    st_e = GraphedTrainStep(m_e, o_e, [t.to(DEV) for t in _model_args(c0, order)], c0["ratings"].to(DEV), slots=2, keep_graph=True)
    st_i = GraphedTrainStep.from_ids(m_i, o_i, cache.feed(kind, True), c0["u_ids"].to(DEV), c0["i_ids"].to(DEV),
                                     c0["ratings"].to(DEV), slots=2, keep_graph=True)
    for a, b in zip(m_e.parameters(), m_i.parameters()):
        assert torch.equal(a, b)
    bit_equal = True
    for k, c in enumerate(batches[:n_steps]):
        s = k % 2
        st_e.stage(s, [t.to(DEV) for t in _model_args(c, order)], c["ratings"].to(DEV))
        st_i.stage(s, (c["u_ids"], c["i_ids"]), c["ratings"])      # host ids: one host-to-device copy of the id block
        le, ge, pe = st_e(slot=s)
        li, gi, pi = st_i(slot=s)
        torch.cuda.synchronize()
        for a, b in zip(st_i.slot_batch(s), st_e.slot_batch(s)):     # what the gather wrote = what the loader staged
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert _rel(li, le) <= 1e-5 and _rel(gi, ge) <= 1e-5, (k, float(li), float(le), float(gi), float(ge))
        assert float((pi - pe).abs().max()) <= 1e-5 * max(1.0, float(pe.abs().max())), k
        bit_equal &= torch.equal(li, le) and torch.equal(gi, ge) and torch.equal(pi, pe)
    _check_params(m_e, m_i)
    n_e, n_i = st_e.kernel_launches(), st_i.kernel_launches()
    with capsys.disabled():
        print(f"\n{kind} {name}: id-fed step bit-equal to the example-fed one: {bit_equal}; launches {n_e} -> {n_i}")
    if n_e is not None and n_i is not None:
        assert n_i == n_e + 1, (n_e, n_i)


@pytest.mark.parametrize("kind,name", MODELS)
def test_id_fed_eval_forward_matches_the_example_fed_one(kind, name, capsys):
    from review_based_recommender_amd.train_step import GraphedForward
    cfg, make, order, cache, _, valid = _setup(kind, name)
    B = cfg["B"]
    m = make().eval()
    c0 = _collate(valid[-B:])
    g_e = GraphedForward(m, [t.to(DEV) for t in _model_args(c0, order)])
    g_i = GraphedForward.from_ids(m, cache.feed(kind, False), c0["u_ids"].to(DEV), c0["i_ids"].to(DEV))
    bit_equal = True
    for s in range(0, 3 * B, B):
        c = _collate(valid[s:s + B])
        p_e = g_e([t.to(DEV) for t in _model_args(c, order)]).clone()
        p_i = g_i((c["u_ids"].to(DEV), c["i_ids"].to(DEV))).clone()
        torch.cuda.synchronize()
        assert float((p_i - p_e).abs().max()) <= 1e-6 * max(1.0, float(p_e.abs().max()))
        bit_equal &= torch.equal(p_i, p_e)
    with capsys.disabled():
        print(f"\n{kind} {name}: id-fed eval forward bit-equal to the example-fed one: {bit_equal}")


# ------------------------------------------------------------------------------------------------ 3. trainer
def _cfg(tmp_path, kind, data_dir, tag, **extra):
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": kind, "parallel": False, "kernel_sizes": "3", "hidden_dim": 8, "embedding_dim": 12, "att_dim": 4,
           "latent_dim": 4, "dropout": 0.0, "word_dropout": 0.0, "review_dropout": 0.0, "arch": "CNN", "use_pretrain": False,
           "epochs": 2, "batch_size": 16, "lr": 0.002, "max_grad_norm": 5.0, "patience": 5, "fast_step": True, "shuffle": False,
           "record_steps": True}
    cfg.update(extra)
    path = tmp_path / f"{kind}_{tag}.json"
    path.write_text(json.dumps(cfg))
    return str(path)


@pytest.mark.parametrize("kind", ["narre", "simple_siamese"])
def test_trainer_device_reviews_follows_the_example_fed_trainer(tmp_path, kind):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = str(tmp_path / "data")
    info = make_review_dataset.write_review_split(data_dir)      # 43 train / 20 valid pairs: ragged last batches of 11 and 4
    runs = {}
    for on in (False, True):
        torch.manual_seed(0)
        exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, int(on), device_reviews=on)), uid=f"r{int(on)}")
        assert isinstance(exp.cache, D.DeviceReviewCache) == on and exp.train_set.feed == ("ids" if on else "examples")
        rmse = []
        for e in range(exp.args.epochs):
            exp.train_one_epoch(e)
            exp.valid_one_epoch()
            rmse.append(exp.last_valid_rmse)
        runs[on] = ([float(x) for x in exp.step_losses], rmse, exp.valid_count)
    (l_e, r_e, n_e), (l_i, r_i, n_i) = runs[False], runs[True]
    assert info["n_train"] == 43 and len(l_e) == len(l_i) == 2 * 3
    for k, (a, b) in enumerate(zip(l_i, l_e)):
        print(f"{kind} step {k}: id-fed loss {a!r}, example-fed {b!r}")
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    for a, b in zip(r_i, r_e):
        print(f"{kind}: id-fed valid rmse {a!r}, example-fed {b!r}")
        assert abs(a - b) <= 1e-5 * abs(b) and math.isfinite(a), (a, b)
    assert n_i == n_e == 20


@pytest.mark.parametrize("kind", ["narre", "simple_siamese"])
def test_trainer_validates_reviews_from_towers_like_the_id_fed_path(tmp_path, kind):
    """eval_from_towers on top of device_reviews against the default id-fed validation, same parameters.  RMSE is 1-Lipschitz in
    the largest prediction difference, so 2e-4 is the bound of the predictions themselves."""
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = str(tmp_path / "data")
    make_review_dataset.write_review_split(data_dir)
    rmse = {}
    state = None
    for towers in (False, True):
        path = _cfg(tmp_path, kind, data_dir, f"t{int(towers)}", device_reviews=True, eval_from_towers=towers, dropout=0.5,
                    epochs=1, patience=100, fast_step=False)
        exp = ReviewExperiment(kind, parse_args(path), uid=f"v{int(towers)}")
        if state is None:
            exp.train_one_epoch(0)
            state = {k: v.clone() for k, v in exp.model.state_dict().items()}
        else:
            exp.model.load_state_dict(state)
        exp.valid_one_epoch()
        assert exp.valid_count == len(exp.valid_set)
        rmse[towers] = exp.last_valid_rmse
    print(f"{kind}: validation rmse id-fed {rmse[False]:.7f}, from towers {rmse[True]:.7f}")
    assert math.isfinite(rmse[False]) and abs(rmse[True] - rmse[False]) <= 2e-4
    with pytest.raises(ValueError, match="eval_from_towers"):
        ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, "bad", eval_from_towers=True)), uid="bad")
