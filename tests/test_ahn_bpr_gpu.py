"""AHN for ranking on the GPU: the opt-in fused pair tail (AHN.fused_tail) against the reference's fixtures, AHN.forward_groups
against AHN.forward on the expanded batch, and the trainer's `ahn_tables` paths -- BPR over NegativeFeed, validation and ranks
from recommend.AhnRecommender's sentence tables, `fused_pair_tail` -- on tests/make_sentence_dataset.py's tiny split."""
import json
import math
import os
import types

import pytest
import torch

import make_sentence_dataset
import synth_ahn
from helpers import check_grads, golden, max_err
from test_ahn_gpu import FWD_TOL, _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("tiny", "small")


def _aggregate_unfused(m, user_sents, item_sents, usm, ism, urm, irm, u_ids, i_ids):
    """aggregate() as it stood before fused_tail: the modules called one after the other."""
    ur, ir, usw, isw, _ = m.unbalanced_sentence_aggregator(user_sents, item_sents, usm, ism)
    rv_u, rv_i, urw, irw = m.unbalanced_review_aggregator(m.user_review_trans_layer(ur), m.item_review_trans_layer(ir), urm, irm)
    users = torch.cat([rv_u, m.user_embeddings(u_ids)], dim=-1)
    items = torch.cat([rv_i, m.item_embeddigns(i_ids)], dim=-1)
    return m.fm(m.dropout(torch.cat([users, items], dim=-1))).view(-1), usw, isw, urw, irw


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("name", NAMES)
def test_fused_tail_reproduces_the_reference_fixture(golden_dir, name):
    from review_based_recommender_amd.train_step import make_optimizer, train_step
    g = golden(golden_dir, "ahn_" + name)
    c = synth_ahn.AHN_CFGS[name]
    model = _model(c, g)
    assert model.fused_tail is False
    model.fused_tail = True
    args, ratings = _batch(g)
    model.eval()
    with torch.no_grad():
        pred, usw, isw, urw, irw = model(*args)
    assert max_err(pred.cpu().numpy(), g["pred_eval"]) <= FWD_TOL
    for got, key in ((usw, "user_sent_weights"), (isw, "item_sent_weights"), (urw, "user_review_weights"), (irw, "item_review_weights")):
        assert got.shape == g[key].shape and max_err(got.cpu().numpy(), g[key]) <= 1e-5, key
    model.train()
    out = model(*args)[0]
    assert max_err(out.detach().cpu().numpy(), g["pred"]) <= FWD_TOL
    loss = torch.nn.functional.mse_loss(out, ratings)
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    loss.backward()
    check_grads({k: p.grad for k, p in model.named_parameters()}, g)
    model.zero_grad()
    loss, gnorm, _ = train_step(model, make_optimizer(model, hip_clip_adam=True), args, ratings)
    assert abs(float(loss) - float(g["loss"])) <= 1e-4
    assert abs(float(gnorm) - float(g["gnorm"])) <= 2e-4 * float(g["gnorm"])


@pytest.mark.parametrize("name", NAMES)
def test_the_default_path_keeps_its_bits(golden_dir, name):
    g = golden(golden_dir, "ahn_" + name)
    model = _model(synth_ahn.AHN_CFGS[name], g).eval()
    args, _ = _batch(g)
    with torch.no_grad():
        got = model(*args)
        sents = model.encode_sentences(args[0], args[1], args[4], args[5])
        want = _aggregate_unfused(model, *sents, args[2], args[3], args[6], args[7], args[8], args[9])
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name,G", [("tiny", 2), ("small", 3)])
def test_forward_groups_equals_forward_on_the_expanded_batch(golden_dir, name, G):
    """The expanded batch: the B fixture rows, then G - 1 slabs whose items are the fixture's rolled by the slab number and whose
    user rows are the first B rows again -- the batch forward_groups defines itself by."""
    g = golden(golden_dir, "ahn_" + name)
    model = _model(synth_ahn.AHN_CFGS[name], g).train()                 # dropout 0: train mode, nothing drawn
    args, _ = _batch(g)
    B = args[0].shape[0]
    big = tuple(torch.cat([t.roll(k, 0) if n % 2 else t for k in range(G)]) for n, t in enumerate(args))      # odd slots: the item's
    up = torch.randn(G * B, generator=torch.Generator().manual_seed(5)).to(DEV)
    ref = model(*big)
    (ref[0] * up).sum().backward()
    want = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    junk = tuple(t if n % 2 else torch.cat([t[:B], torch.zeros_like(t[B:])]) for n, t in enumerate(big[:8])) + big[8:]
    got = model.forward_groups(*junk, groups=G)                          # user rows behind the first B are not read
    (got[0] * up).sum().backward()
    assert got[0].shape == (G * B,)
    assert max_err(got[0].detach().cpu().numpy(), ref[0].detach().cpu().numpy()) <= 1e-4
    for a, b in zip(got[1:], ref[1:]):
        assert a.shape == b.shape and max_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= 1e-5
    for k, p in model.named_parameters():
        scale = float(want[k].abs().max())
        err = float((p.grad - want[k]).abs().max())
        print(f"forward_groups {name} G={G}: grad {k} max err {err:.2e} / {scale:.2e}")
        assert err <= 2e-6 + 2e-4 * scale, k
    with pytest.raises(ValueError, match="groups"):
        model.forward_groups(*big, groups=G * B + 1)


# ------------------------------------------------------------------------------------------------ 2. the trainer
def _cfg(tmp_path, data_dir, tag, **extra):
    cfg = {"data_dir": data_dir, "dataset": "synthetic", "log_dir": str(tmp_path / "logs"), "log": True, "log_idx": 2,
           "model_name": "ahn", "parallel": False, "hidden_dim": 12, "embedding_dim": 12, "k_factor": 4, "dropout": 0.0,
           "rnn_dropout": 0.0, "use_pretrain": False, "epochs": 2, "batch_size": 16, "lr": 0.002, "max_grad_norm": 5.0, "patience": 5,
           "fast_step": False, "shuffle": False, "record_steps": True, "device_reviews": True}
    cfg.update(extra)
    path = tmp_path / f"ahn_{tag}.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def _run(tmp_path, data_dir, tag, epochs, **extra):
    from review_based_recommender_amd.trainer import ReviewExperiment, parse_args
    torch.manual_seed(0)
    exp = ReviewExperiment("ahn", parse_args(_cfg(tmp_path, data_dir, tag, epochs=epochs, **extra)), uid=tag)
    for e in range(epochs):
        exp.train_one_epoch(e)
        exp.valid_one_epoch()
    torch.cuda.synchronize()
    with open(exp.log_path) as f:
        log = f.read()
    return types.SimpleNamespace(exp=exp, losses=[float(x) for x in exp.step_losses], log=log)


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ahn_bpr")
    data_dir = str(tmp / "data")
    make_sentence_dataset.write_sentence_split(data_dir)
    return types.SimpleNamespace(tmp=tmp, data_dir=data_dir)


BPR = dict(ahn_tables=True, loss="bpr", n_neg=2, rank_metrics=[10], select_by="ndcg@10")


def test_trainer_bpr_over_the_sentence_tables(split):
    from review_based_recommender_amd.recommend import AhnRecommender
    from review_based_recommender_amd.train_step import AhnBprObjective
    a = _run(split.tmp, split.data_dir, "bpr_a", 2, **BPR)
    b = _run(split.tmp, split.data_dir, "bpr_b", 2, **BPR)
    assert isinstance(a.exp.objective, AhnBprObjective) and isinstance(a.exp._towers, AhnRecommender)
    assert len(a.losses) == 6 and all(math.isfinite(x) for x in a.losses)
    assert a.losses == b.losses                                                 # one seed: the same negatives, the same bits
    assert a.log.count("valid hr@10: ") == 2 and a.log.count("best ndcg@10: ") == 2 and "mrr: " in a.log
    assert a.log.count("bytes of per-id sentence tables") == 1                  # the memory opt-in is logged once
    ck = torch.load(os.path.join(a.exp.out_dir, "best_model.pt"), map_location="cpu")
    assert set(ck) == {"model", "optimizer", "updates", "args"} and ck["args"]["ahn_tables"] is True


def test_trainer_validates_from_the_sentence_tables(split):
    from review_based_recommender_amd.recommend import AhnRecommender
    r = _run(split.tmp, split.data_dir, "towers", 1, ahn_tables=True, eval_from_towers=True)
    ex = r.exp.valid_set.examples
    u = torch.tensor([int(e[0]) for e in ex], device=DEV)
    i = torch.tensor([int(e[1]) for e in ex], device=DEV)
    y = torch.tensor([float(e[2]) for e in ex], dtype=torch.float64)
    pred = AhnRecommender(r.exp.model, r.exp.cache).refresh().score(u, i)
    rmse = math.sqrt(float(((pred.double().cpu() - y) ** 2).mean()))
    print(f"ahn_tables valid rmse: trainer {r.exp.last_valid_rmse!r}, by hand {rmse!r}")
    assert r.exp.valid_count == len(ex) and abs(r.exp.last_valid_rmse - rmse) <= 1e-6 * max(1.0, rmse)


def test_trainer_fused_pair_tail_follows_the_unfused_step(split):
    plain = _run(split.tmp, split.data_dir, "mse_plain", 1, ahn_tables=True)
    fused = _run(split.tmp, split.data_dir, "mse_fused", 1, ahn_tables=True, fused_pair_tail=True)
    assert fused.exp.model.fused_tail is True and plain.exp.model.fused_tail is False
    assert len(plain.losses) == len(fused.losses) == 3
    for k, (a, b) in enumerate(zip(fused.losses, plain.losses)):
        print(f"ahn mse step {k}: fused {a!r}, unfused {b!r}")
        assert abs(a - b) <= 1e-5 * abs(b), k
