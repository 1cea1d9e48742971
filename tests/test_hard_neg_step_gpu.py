"""The BPR step over dynamically sampled negatives: train_step / GraphedTrainStep with data.NegativeFeed(n_cand=4) against the
manual composition and against each other, under the bounds tests/test_bpr_step_gpu.py holds the uniform step to (its helpers
and SIZES are used here); a set_tables() between replays keeps the recording and changes the negatives; the trainer's
`neg_candidates` / `neg_refresh_steps` path; and `neg_candidates: 1` against a config without the key."""
import copy
import os

import numpy as np
import pytest
import torch

import make_dataset
import make_review_dataset
from hard_neg_ref import choose
from helpers import check_grads, quiet
from test_bpr_step_gpu import KINDS, LOG_RE, RANK_RE, SIZES, _cfg, _check_params, _ids, _torch_bpr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NEG, N_CAND, B = 2, 4, 16


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    root = tmp_path_factory.mktemp("hardneg")
    make_dataset.write_doc_split(str(root / "doc"))
    make_review_dataset.write_review_split(str(root / "rev"))
    return {"doc": str(root / "doc"), "rev": str(root / "rev")}


def _setup(kind, splits, seed=3):
    """(model factory, training examples, inner id feed, the cache a Recommender reads, NegativeFeed factory, with_ids)"""
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.trainer import Args, make_model
    if kind in ("narre", "simple_siamese"):
        ds = D.ReviewDataset(splits["rev"], "train", feed="ids")
        cache = D.DeviceReviewCache(ds, DEV)
        inner = cache.feed(kind, True)
    else:
        ds = D.DocDataset(splits["doc"], "train", with_ids=kind == "deepconn", feed="ids")
        cache = inner = D.DeviceDocCache(ds, DEV)
    seen = Recommender.seen_from(ds.examples, ds.user_num, DEV)
    torch.manual_seed(0)
    proto = quiet(make_model, kind, Args(dict(SIZES)), ds)
    proto.validate_ids = False

    def model():
        return copy.deepcopy(proto).to(DEV).train()

    def feed():
        return D.NegativeFeed(inner, seen, cache.item.shape[0], n_neg=N_NEG, seed=seed, n_cand=N_CAND)

    return model, ds.examples, inner, cache, feed, kind != "dual_att"


def _set_tables(nf, model, ul, il):
    nf.set_tables(model.score_mode_and_params()[0], ul, il, *model.score_mode_and_params()[1:])


def _draw(nf, model, u, i):
    """The functional entry on the feed's tables, the model's live head and a COPY of the feed's state."""
    from review_based_recommender_amd import functional as RF
    mode, h, g, ub, ib = model.score_mode_and_params()
    ul, il = nf.tables
    return RF.sample_hard_negatives(
        u, i, nf.n_neg, nf.n_items, nf.seen, n_cand=nf.n_cand, mode=mode, ul=ul, il=il, h=h, g=g, ub=ub, ib=ib, state=nf.state.clone(),
        seed=nf.seed, item_lo=nf.item_lo, max_tries=nf.max_tries, replace_id=nf.item_lo, return_candidates=True)


def _expected_draw(nf, model, u, i):
    """What the feed's next sample() must draw; the chosen items are also checked against the key rule restated on the host."""
    u_out, i_out, valid, cand, score = _draw(nf, model, u, i)
    assert np.array_equal(i_out[u.shape[0]:].view(nf.n_neg, -1).cpu().numpy(), choose(cand.cpu().numpy(), score.cpu().numpy()))
    return u_out, i_out, valid


def _candidates(nf, model, u, i):
    """int64 [n_neg, B, n_cand]: the candidates of the feed's next sample() (they do not depend on the tables)."""
    return _draw(nf, model, u, i)[3]


@pytest.mark.parametrize("kind", KINDS)
def test_hard_negative_step_equals_the_manual_composition(kind, splits):
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.train_step import BprObjective, clip_and_step, make_optimizer, train_step
    model, examples, inner, cache, feed, with_ids = _setup(kind, splits)
    m_a, m_b = model(), model()
    o_a, o_b = make_optimizer(m_a, hip_clip_adam=True), make_optimizer(m_b, hip_clip_adam=True)
    nf = feed()
    rec = Recommender(m_a, cache).refresh()
    assert m_a.training                                   # refresh() restored the mode
    _set_tables(nf, m_a, rec.user_latents, rec.item_latents)
    nf.reseed(3, call=2)
    u, i, r = _ids(examples, 0, B)
    want = _expected_draw(nf, m_a, u, i)
    loss, gnorm, pred = train_step(m_a, o_a, nf.inputs(u, i, with_ids=with_ids), r, objective=BprObjective(nf))
    o_a.materialize_grads()
    assert pred.shape == ((1 + N_NEG) * B,) and torch.equal(nf.u_out, u.repeat(1 + N_NEG)) and torch.equal(nf.i_out[:B], i)
    for got, w in zip((nf.u_out, nf.i_out, nf.valid), want):
        assert torch.equal(got, w)
    assert nf.state.tolist() == [3, 0]

    # by hand on the copy: the same expanded ids through the inner feed, the loss in torch, the same optimizer
    o_b.zero_grad()
    out = m_b(*inner.inputs(nf.u_out.clone(), nf.i_out.clone(), with_ids=with_ids))
    pred_b = out[0] if isinstance(out, tuple) else out
    loss_b = _torch_bpr(pred_b, N_NEG, nf.valid)
    loss_b.backward()
    gnorm_b = clip_and_step(m_b, o_b, 5.0)
    torch.cuda.synchronize()
    print(f"{kind}: loss {float(loss)!r} vs {float(loss_b.detach())!r}; gnorm {float(gnorm)!r} vs {float(gnorm_b)!r}; "
          f"valid negatives {int(nf.valid.sum())}/{N_NEG * B}")
    assert float((pred - pred_b.detach()).abs().max()) <= 1e-4
    assert abs(float(loss) - float(loss_b)) <= 1e-4
    ref, got = {}, {}
    for (k, p), q in zip(m_b.named_parameters(), m_a.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            ref[f"grad/{k}"] = p.grad.detach().cpu().numpy()
            ref[f"gradl2/{k}"] = float(p.grad.double().norm())
            got[k] = q.grad
    assert got
    check_grads(got, ref)
    _check_params(m_a, m_b)


@pytest.mark.parametrize("kind", KINDS)
def test_recorded_hard_negative_step_follows_the_eager_one(kind, splits):
    """tests/test_bpr_step_gpu.py's test_recorded_bpr_step_follows_the_eager_one with n_cand = 4, same bounds: pred of the first
    step 1e-4, loss 1e-4, the pairwise differences 1e-4 and gnorm 2e-4 relative on every step, parameters afterwards lr/2 max and
    1e-4 RMS.  Before every step each side's draw is predicted from its own tables, its own model's live head and its own call
    number; after step 0 both feeds get NEW tables (constructed ones: any table is a valid input) through set_tables -- the
    recording keeps its pointers, and the negatives of step 1 are the ones the new values give, not the ones the old values
    would have."""
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.train_step import BprObjective, GraphedTrainStep, make_optimizer, train_step
    model, examples, inner, cache, feed, with_ids = _setup(kind, splits)
    m_g, m_e = model(), model()
    o_g, o_e = make_optimizer(m_g, hip_clip_adam=True), make_optimizer(m_e, hip_clip_adam=True)
    nf_g, nf_e = feed(), feed()
    rec = Recommender(m_e, cache).refresh()
    _set_tables(nf_g, m_g, rec.user_latents, rec.item_latents)
    _set_tables(nf_e, m_e, rec.user_latents, rec.item_latents)
    u0, i0, r0 = _ids(examples, B, B)                    # recorded on other pairs than it replays
    step = GraphedTrainStep.from_ids(m_g, o_g, nf_g, u0, i0, r0, with_ids=with_ids, objective=BprObjective(nf_g), keep_graph=True)
    for a, b in zip(m_g.parameters(), m_e.parameters()):
        assert torch.equal(a, b)                          # recording left the parameters alone
    nf_g.reseed(3, call=0)
    nf_e.reseed(3, call=0)
    u, i, r = _ids(examples, 0, B)
    obj_e = BprObjective(nf_e)
    ptrs = [t.data_ptr() for t in nf_g.tables]
    drawn = []
    for s in range(3):
        if s == 1:
            stale = _expected_draw(nf_g, m_g, u, i)       # what the old tables would give for this call number
            cand = _candidates(nf_g, m_g, u, i)
            assert bool((cand.min(-1).values != cand.max(-1).values).any())      # some draw has a choice to make
            # ul = 1 and il[c, :] = 1000 (c + 1), or 1000 (I - c): every score is that ramp times (the sum of h, or K) plus biases
            # of about 0.1, so one of the two tables makes the highest candidate id win and the other the lowest -- whatever
            # the old tables chose, one of them chooses differently in a draw with two distinct candidates
            ramp = 1000.0 * torch.arange(1, nf_g.n_items + 1, device=DEV, dtype=torch.float32)[:, None]
            for column in (ramp, ramp.flip(0)):
                ul, il = torch.ones_like(nf_g.tables[0]), column.expand_as(nf_g.tables[1]).contiguous()
                _set_tables(nf_g, m_g, ul, il)
                _set_tables(nf_e, m_e, ul, il)
                assert [t.data_ptr() for t in nf_g.tables] == ptrs and torch.equal(nf_g.tables[1], il)
                if not torch.equal(_expected_draw(nf_g, m_g, u, i)[1], stale[1]):
                    break
        want_g, want_e = _expected_draw(nf_g, m_g, u, i), _expected_draw(nf_e, m_e, u, i)
        if s == 1:
            assert not torch.equal(want_g[1], stale[1])
        lg, gg, pg = step((u, i), r)
        le, ge, pe = train_step(m_e, o_e, nf_e.inputs(u, i, with_ids=with_ids), r, objective=obj_e)
        torch.cuda.synchronize()
        for got, w in zip((nf_g.u_out, nf_g.i_out, nf_g.valid), want_g):
            assert torch.equal(got, w), s
        for got, w in zip((nf_e.u_out, nf_e.i_out, nf_e.valid), want_e):
            assert torch.equal(got, w), s
        assert torch.equal(nf_g.i_out, nf_e.i_out) and torch.equal(nf_g.u_out, nf_e.u_out) and torch.equal(nf_g.valid, nf_e.valid)
        drawn.append(nf_g.i_out.clone())
        assert pg.shape == ((1 + N_NEG) * B,)
        d_pred = float((pg - pe).abs().max())
        d_x = float(((pg[B:].view(N_NEG, B) - pg[:B]) - (pe[B:].view(N_NEG, B) - pe[:B])).abs().max())
        print(f"{kind} step {s}: max |pred - eager pred| {d_pred:.3e}, of the pairwise differences {d_x:.3e}; "
              f"loss {float(lg)!r} vs {float(le)!r}")
        if s == 0:
            assert d_pred <= 1e-4, (s, d_pred)
        assert d_x <= 1e-4, (s, d_x)
        assert abs(float(lg) - float(le)) <= 1e-4, (s, float(lg), float(le))
        assert abs(float(gg) - float(ge)) <= 2e-4 * float(ge), (s, float(gg), float(ge))
    assert nf_g.state.tolist() == [3, 0] == nf_e.state.tolist()
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    _check_params(m_g, m_e)
    print(f"{kind}: recorded hard-negative step launches {step.kernel_launches()} kernels")


# ------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize("kind,fast", [("deepconn", False), ("deepconn", True), ("narre", False)])
def test_trainer_trains_on_hard_negatives(tmp_path, kind, fast, splits):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = splits["rev" if kind == "narre" else "doc"]
    torch.manual_seed(0)
    exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, "h", epochs=2, neg_candidates=4, fast_step=fast)), uid="h0")
    nf = exp.train_feed
    assert isinstance(nf, D.NegativeFeed) and nf.n_cand == 4 and nf.n_neg == 2 and nf.tables is None
    exp.train_one_epoch(0)
    assert exp.model.training                             # the refresh before the first step restored the mode
    first = [t.clone() for t in nf.tables]
    ptrs = [t.data_ptr() for t in nf.tables]
    assert first[0].shape[0] == exp.train_set.user_num and first[1].shape[0] == nf.n_items
    exp.valid_one_epoch()
    second = [t.clone() for t in nf.tables]
    assert [t.data_ptr() for t in nf.tables] == ptrs
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])
    assert torch.equal(second[0], exp._towers.user_latents) and torch.equal(second[1], exp._towers.item_latents)
    exp.train_one_epoch(1)
    assert torch.equal(nf.tables[0], second[0]) and torch.equal(nf.tables[1], second[1])      # neg_refresh_steps 0: one snapshot an epoch
    exp.valid_one_epoch()
    log = open(os.path.join(exp.out_dir, "log.txt")).read().splitlines()
    steps = [l for l in log if l.startswith("epoch:")]
    n_steps = len(exp.train_loader)
    assert len(steps) == 2 * (n_steps // 2) and all(LOG_RE.match(l) for l in steps), steps[:2]
    rank_lines = [l for l in log if l.startswith("valid hr@5")]
    assert len(rank_lines) == 2 and all(RANK_RE.match(l) for l in rank_lines), rank_lines
    assert os.path.exists(os.path.join(exp.out_dir, "best_model.pt"))
    assert nf.state.tolist() == [2 * n_steps, 0]
    assert all(np.isfinite(float(x)) and float(x) >= 0.0 for x in exp.step_losses)
    print(f"{kind} fast_step={fast}: neg_candidates 4, validation ndcg@5 after two epochs {exp.last_rank_metrics['ndcg@5']:.3f}")


def test_trainer_refreshes_the_tables_every_neg_refresh_steps_updates(tmp_path, splits):
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    torch.manual_seed(0)
    exp = ReviewExperiment("deepconn", parse_args(_cfg(tmp_path, "deepconn", splits["doc"], "r", epochs=1, neg_candidates=4,
                                                       neg_refresh_steps=2)), uid="r0")
    calls, snapshots = [], []
    refresh = exp._refresh_negative_tables

    def counted():
        calls.append(exp.updates)
        refresh()
        snapshots.append(exp.train_feed.tables[1].clone())

    exp._refresh_negative_tables = counted
    exp.train_one_epoch(0)
    n_steps = len(exp.train_loader)
    assert n_steps >= 3 and calls == [0] + list(range(2, n_steps, 2)), (calls, n_steps)
    assert exp.model.training
    assert all(not torch.equal(a, b) for a, b in zip(snapshots[:-1], snapshots[1:]))


def _two_epochs(tmp_path, kind, data_dir, tag, **extra):
    """(step losses [steps] on the CPU, the (u_out, i_out, valid) of every step) of a two-epoch BPR run of the trainer."""
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    torch.manual_seed(0)
    exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, tag, epochs=2, **extra)), uid=f"k{tag}")
    nf = exp.train_feed
    assert nf.n_cand == 1 and nf.tables is None
    draws, sample = [], nf.sample

    def recorded(u_ids, i_ids):
        out = sample(u_ids, i_ids)
        draws.append([t.clone() for t in out])
        return out

    nf.sample = recorded
    for e in range(2):
        exp.train_one_epoch(e)
        exp.valid_one_epoch()
    assert nf.tables is None and len(draws) == len(exp.step_losses)
    return torch.stack(exp.step_losses).cpu(), draws


@pytest.mark.parametrize("kind", ["deepconn", "narre"])
def test_one_candidate_trains_like_a_config_without_the_key(tmp_path, kind, splits):
    """`neg_candidates: 1` is the uniform sampler, call for call: a run with the key and a run that never names it, via record_steps.

    Two runs of one and the same config are not bit-reproducible in this package once the parameters have moved: the head's
    id-addressed gradients (Eu, Ei, ub, ib) are f32 atomics, and with a user in the batch 1 + n_neg times their arrival order
    shows in the last bit.  Measured on an MI355X with NO neg_candidates key in either run: DeepCoNN++'s 12 step losses differ by
    5.96e-08 between two runs in about every second pair of runs (set_dtable_mode("fixed") or not), NARRE's 6 never did.  So the
    bit comparison of all step losses is made where a run is reproducible -- `lr: 0`, the parameters stay as initialised, every
    step still draws, gathers, runs forward, loss and backward, and the losses differ from step to step with the batch and its
    negatives -- and the run at the config's own lr is held to what is reproducible there: the three sampler outputs of every
    step bit for bit, and the loss of the first step, which the parameters' history cannot have touched."""
    data_dir = splits["rev" if kind == "narre" else "doc"]
    for lr in (0.0, 0.002):
        (loss_a, draws_a), (loss_b, draws_b) = (_two_epochs(tmp_path, kind, data_dir, f"{tag}{lr}", lr=lr, **extra)
                                                for tag, extra in (("none", {}), ("one", {"neg_candidates": 1})))
        print(f"{kind} lr {lr}: {len(loss_a)} step losses, max |difference| {float((loss_a - loss_b).abs().max()):.3e}")
        assert len(loss_a) == len(loss_b) >= 6 and len(draws_a) == len(draws_b)
        for a, b in zip(draws_a, draws_b):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert any(not torch.equal(draws_a[0][1], d[1]) for d in draws_a[1:])
        if lr == 0.0:
            assert torch.equal(loss_a, loss_b) and len(set(loss_a.tolist())) > 1
        else:
            assert torch.equal(loss_a[0], loss_b[0])


