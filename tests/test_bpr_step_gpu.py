"""The BPR step: train_step / GraphedTrainStep with data.NegativeFeed + train_step.BprObjective against the manual composition
(the same expanded ids through the inner feed, the loss written in torch), the recorded step against the eager one, the MSE
step untouched, and the trainer's `loss: "bpr"` / `select_by` path.  Tiny models: the sizes of tests/test_trainer_gpu.py."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_dataset
import make_review_dataset
from helpers import check_grads, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["deepconn", "dual_att", "narre", "simple_siamese"]
LOG_RE = re.compile(r"^epoch: \d+/\d+, step: \d+/\d+, loss: \d+\.\d{3}, rmse: \d+\.\d{3}, lr: [\d.e-]+, gnorm: \d+\.\d+, time: \d+\.\d{3}$")
RANK_RE = re.compile(r"^valid hr@5: \d\.\d{3}, ndcg@5: \d\.\d{3}, mrr: \d\.\d{3}, best ndcg@5: \d\.\d{3}$")
SIZES = {"kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12, "att_dim": 4, "latent_dim": 4, "dropout": 0.0, "arch": "CNN",
         "l_window_size": 5, "l_out_size": 8, "g_out_size": 4, "emb_size": 12, "hidden_size_1": 10, "hidden_size_2": 5,
         "word_dropout": 0.0, "review_dropout": 0.0}


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    root = tmp_path_factory.mktemp("bpr")
    make_dataset.write_doc_split(str(root / "doc"))
    make_review_dataset.write_review_split(str(root / "rev"))      # the review split the id feed accepts (leave-one-out examples)
    return {"doc": str(root / "doc"), "rev": str(root / "rev")}


def _setup(kind, splits, n_neg, seed=3):
    """(model factory, training examples, inner id feed, NegativeFeed factory, with_ids)"""
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.recommend import Recommender
    from review_based_recommender_amd.trainer import Args, make_model
    review = kind in ("narre", "simple_siamese")
    if review:
        ds = D.ReviewDataset(splits["rev"], "train", feed="ids")
        inner = D.DeviceReviewCache(ds, DEV).feed(kind, True)
        n_items = inner.cache.item.shape[0]
    else:
        ds = D.DocDataset(splits["doc"], "train", with_ids=kind == "deepconn", feed="ids")
        inner = D.DeviceDocCache(ds, DEV)
        n_items = inner.item.shape[0]
    seen = Recommender.seen_from(ds.examples, ds.user_num, DEV)
    torch.manual_seed(0)
    proto = quiet(make_model, kind, Args(dict(SIZES)), ds)
    proto.validate_ids = False

    def model():
        return copy.deepcopy(proto).to(DEV).train()

    def feed():
        return D.NegativeFeed(inner, seen, n_items, n_neg=n_neg, seed=seed)

    return model, ds.examples, inner, feed, kind != "dual_att"


def _ids(examples, lo, B):
    ex = examples[lo:lo + B]
    return (torch.tensor([int(e[0]) for e in ex], device=DEV), torch.tensor([int(e[1]) for e in ex], device=DEV),
            torch.tensor([float(e[2]) for e in ex], device=DEV))


def _torch_bpr(pred, n_neg, valid):
    B = pred.shape[0] // (1 + n_neg)
    x = pred[B:].view(n_neg, B) - pred[:B][None, :]
    v = valid.view(n_neg, B)
    return (v * F.softplus(x)).sum() / v.sum().clamp_min(1.0)


def _check_params(m_a, m_b, lr=2e-3):
    """helpers.check_params_after's gates (what tests/test_fused_step_gpu.py holds a recorded step to): lr/2 max, 1e-4 RMS, and
    like it no gate on a parameter whose gradient (m_b's, as the last step left it) is below 1e-6 in norm: Adam turns rounding
    noise of either sign into a step of lr.  Under BPR that is the rule for the head's global bias, whose exact gradient is 0 --
    every positive's gradient is minus the sum of its negatives' -- so that what reaches it is the rounding of that sum."""
    for (n, a), b in zip(m_a.named_parameters(), m_b.parameters()):
        if b.grad is None or float(b.grad.double().norm()) < 1e-6:
            continue
        d = (a.detach() - b.detach()).double()
        assert float(d.abs().max()) <= lr / 2, n
        assert float(d.pow(2).mean().sqrt()) <= 1e-4, n


@pytest.mark.parametrize("kind", KINDS)
def test_bpr_step_equals_the_manual_composition(kind, splits):
    from review_based_recommender_amd.train_step import BprObjective, clip_and_step, make_optimizer, train_step
    n_neg, B = 2, 16
    model, examples, inner, feed, with_ids = _setup(kind, splits, n_neg)
    m_a, m_b = model(), model()
    o_a, o_b = make_optimizer(m_a, hip_clip_adam=True), make_optimizer(m_b, hip_clip_adam=True)
    nf = feed()
    nf.reseed(3, call=2)
    u, i, r = _ids(examples, 0, B)
    loss, gnorm, pred = train_step(m_a, o_a, nf.inputs(u, i, with_ids=with_ids), r, objective=BprObjective(nf))
    o_a.materialize_grads()
    assert pred.shape == ((1 + n_neg) * B,) and torch.equal(nf.u_out, u.repeat(1 + n_neg)) and torch.equal(nf.i_out[:B], i)

    # by hand on the copy: the same expanded ids through the inner feed, the loss in torch, the same optimizer
    o_b.zero_grad()
    out = m_b(*inner.inputs(nf.u_out.clone(), nf.i_out.clone(), with_ids=with_ids))
    pred_b = out[0] if isinstance(out, tuple) else out
    loss_b = _torch_bpr(pred_b, n_neg, nf.valid)
    loss_b.backward()
    gnorm_b = clip_and_step(m_b, o_b, 5.0)
    torch.cuda.synchronize()
    print(f"{kind}: loss {float(loss)!r} vs {float(loss_b.detach())!r}; gnorm {float(gnorm)!r} vs {float(gnorm_b)!r}; "
          f"valid negatives {int(nf.valid.sum())}/{n_neg * B}")
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
def test_recorded_bpr_step_follows_the_eager_one(kind, splits):
    """from_ids(..., objective=...) against the eager step over three steps from the same reseed, on the SAME staged pairs every
    time: what changes from replay to replay is the negatives.  Bounds: those tests/test_fused_step_gpu.py holds a recorded step
    to: pred of the first step 1e-4, loss 1e-4, gnorm 2e-4 relative, parameters after the steps lr/2 max and 1e-4 RMS where the
    gradient is above 1e-6 in norm (_graphed_vs_golden there looks at pred on the first step only, for the reason that shows
    here).  Loss, gnorm and the pairwise differences pred_neg - pred_pos (1e-4) are held to their bounds on every step.  Later raw
    predictions are printed, not gated: the exact BPR
    gradient of a user's bias and of the global bias is 0 (a pair's positive gradient is minus the sum of its negatives', and
    they share the user), what arrives is the rounding of that sum in the order the atomics land, and Adam moves a parameter
    by up to lr / 10 per step on such noise.  Measured on an MI355X: step 0 equal for all four models; on the third step raw predictions
    differ by 6.7e-4 (DeepCoNN), 9.1e-4 (NARRE), 5.1e-4 (SimpleSiamese) and 1.5e-8 (D-ATT, which has no biases), the pairwise
    differences by at most 4.8e-7 -- a shift of all of a user's scores, which no pairwise difference sees."""
    from review_based_recommender_amd.train_step import BprObjective, GraphedTrainStep, make_optimizer, train_step
    n_neg, B = 2, 16
    model, examples, inner, feed, with_ids = _setup(kind, splits, n_neg)
    m_g, m_e = model(), model()
    o_g, o_e = make_optimizer(m_g, hip_clip_adam=True), make_optimizer(m_e, hip_clip_adam=True)
    nf_g, nf_e = feed(), feed()
    u0, i0, r0 = _ids(examples, B, B)                    # recorded on other pairs than it replays
    step = GraphedTrainStep.from_ids(m_g, o_g, nf_g, u0, i0, r0, with_ids=with_ids, objective=BprObjective(nf_g), keep_graph=True)
    for a, b in zip(m_g.parameters(), m_e.parameters()):
        assert torch.equal(a, b)                          # recording left the parameters alone
    nf_g.reseed(3, call=0)
    nf_e.reseed(3, call=0)
    u, i, r = _ids(examples, 0, B)
    obj_e = BprObjective(nf_e)
    drawn = []
    for s in range(3):
        lg, gg, pg = step((u, i), r)
        le, ge, pe = train_step(m_e, o_e, nf_e.inputs(u, i, with_ids=with_ids), r, objective=obj_e)
        torch.cuda.synchronize()
        assert torch.equal(nf_g.i_out, nf_e.i_out) and torch.equal(nf_g.u_out, nf_e.u_out) and torch.equal(nf_g.valid, nf_e.valid)
        drawn.append(nf_g.i_out.clone())
        assert pg.shape == ((1 + n_neg) * B,)
        d_pred = float((pg - pe).abs().max())
        d_x = float(((pg[B:].view(n_neg, B) - pg[:B]) - (pe[B:].view(n_neg, B) - pe[:B])).abs().max())
        print(f"{kind} step {s}: max |pred - eager pred| {d_pred:.3e}, of the pairwise differences {d_x:.3e}; "
              f"loss {float(lg)!r} vs {float(le)!r}")
        if s == 0:
            assert d_pred <= 1e-4, (s, d_pred)
        assert d_x <= 1e-4, (s, d_x)                    # what the objective sees of the predictions, on every step
        assert abs(float(lg) - float(le)) <= 1e-4, (s, float(lg), float(le))
        assert abs(float(gg) - float(ge)) <= 2e-4 * float(ge), (s, float(gg), float(ge))
    assert nf_g.state.tolist() == [3, 0] == nf_e.state.tolist()
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    _check_params(m_g, m_e)
    print(f"{kind}: recorded BPR step launches {step.kernel_launches()} kernels")


def test_mse_step_is_untouched_by_the_objective_argument(splits):
    """objective=None is today's path: the same bits as leaving it out.  Pairs with distinct users and distinct items and the
    fixed-point table gradient, so that no atomic's arrival order can differ between the two runs."""
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import make_optimizer, train_step
    model, examples, inner, _, with_ids = _setup("deepconn", splits, 1)
    u = torch.arange(1, 9, device=DEV)
    i = torch.tensor([3, 1, 4, 9, 5, 2, 6, 8], device=DEV)
    r = torch.linspace(1, 5, 8, device=DEV)
    RF.set_dtable_mode("fixed")
    try:
        res = []
        for kw in ({}, {"objective": None}):
            m = model()
            o = make_optimizer(m, hip_clip_adam=True)
            out = train_step(m, o, inner.inputs(u, i, with_ids=with_ids), r, **kw)
            torch.cuda.synchronize()
            res.append(([t.clone() for t in out], [p.detach().clone() for p in m.parameters()]))
    finally:
        RF.set_dtable_mode(None)
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a, b)
    assert res[0][0][2].shape == (8,)


# ------------------------------------------------------------------------------------------------ trainer
def _cfg(tmp_path, kind, data_dir, tag, **extra):
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": kind, "parallel": False, "use_pretrain": False, "epochs": 3, "batch_size": 16, "lr": 0.002,
           "max_grad_norm": 5.0, "patience": 5, "loss": "bpr", "n_neg": 2, "eval_from_towers": True, "rank_metrics": [5],
           "select_by": "ndcg@5", "shuffle": False, "record_steps": True}
    cfg.update(SIZES)
    cfg.update({"device_reviews": True} if kind in ("narre", "simple_siamese") else {"device_cache": True})
    cfg.update(extra)
    path = tmp_path / f"{kind}_{tag}.json"
    path.write_text(json.dumps(cfg))
    return str(path)


@pytest.mark.parametrize("kind", ["deepconn", "narre"])
def test_trainer_trains_for_ranking_and_selects_by_ndcg(tmp_path, kind, splits):
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = splits["rev" if kind == "narre" else "doc"]
    torch.manual_seed(0)
    exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, "t")), uid="b0")
    assert isinstance(exp.train_feed, D.NegativeFeed) and exp.train_feed.n_neg == 2 and exp.train_feed.seen is not None
    ndcg, updates = [], []
    for e in range(exp.args.epochs):
        exp.train_one_epoch(e)
        exp.valid_one_epoch()
        ndcg.append(exp.last_rank_metrics["ndcg@5"])
        updates.append(exp.updates)
    assert exp._seen[0].data_ptr() == exp.train_feed.seen[0].data_ptr()          # one CSR: the sampler's and the validation's
    log = open(os.path.join(exp.out_dir, "log.txt")).read().splitlines()
    steps = [l for l in log if l.startswith("epoch:")]
    n_steps = len(exp.train_loader)
    assert len(steps) == 3 * (n_steps // 2) and all(LOG_RE.match(l) for l in steps), steps[:2]
    assert sum(l.startswith("valid loss:") for l in log) == 3
    rank_lines = [l for l in log if l.startswith("valid hr@5")]
    assert len(rank_lines) == 3 and all(RANK_RE.match(l) for l in rank_lines), rank_lines
    best = int(np.argmax(ndcg))                          # the first epoch that reached the best NDCG (later ties do not replace it)
    assert rank_lines[-1].endswith("best ndcg@5: {:.3f}".format(max(ndcg)))
    ck = torch.load(os.path.join(exp.out_dir, "best_model.pt"), map_location="cpu", weights_only=False)
    assert ck["updates"] == updates[best], (ndcg, updates, ck["updates"])
    assert exp.patience == len(ndcg) - 1 - best
    assert all(np.isfinite(float(x)) and float(x) >= 0.0 for x in exp.step_losses)


@pytest.mark.parametrize("kind", ["deepconn", "narre"])
def test_fast_step_draws_and_trains_like_the_eager_bpr_step(tmp_path, kind, splits):
    """fast_step on and off: the same negatives from the same seed (recording the step does not use up draws), so the same
    per-step losses within test_fast_step_trains_like_the_eager_step's bound.  batch_size 20 leaves a ragged, eager last batch."""
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    data_dir = splits["rev" if kind == "narre" else "doc"]
    losses = {}
    for fast in (False, True):
        torch.manual_seed(0)
        exp = ReviewExperiment(kind, parse_args(_cfg(tmp_path, kind, data_dir, int(fast), fast_step=fast, epochs=2, batch_size=20,
                                                     neg_seed=11)), uid=f"f{int(fast)}")
        assert exp.train_feed.seed == 11
        for e in range(2):
            exp.train_one_epoch(e)
            exp.valid_one_epoch()
        losses[fast] = [float(x) for x in exp.step_losses]
        assert exp.train_feed.state.tolist() == [len(losses[fast]), 0]
    assert len(losses[True]) == len(losses[False]) >= 6
    for k, (a, b) in enumerate(zip(losses[False], losses[True])):
        print(f"{kind} step {k}: eager {a!r}, fast_step {b!r}")
        assert abs(a - b) <= 5e-3 * max(1.0, abs(a)), (k, a, b)
