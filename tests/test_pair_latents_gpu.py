"""pair_latents of the four models: the towers' latent rows where the two-tower tail stops in front of the pair-dependent head.
In eval mode functional.pair_score of the rows is the model's own forward; in train mode the rows carry autograd to every tower
parameter -- the head written in torch on top of them gives the tower gradients of the model's own forward + backward.  Tiny
models: the sizes of tests/test_bpr_step_gpu.py."""
import copy

import pytest
import torch

import make_dataset
import make_review_dataset
from helpers import check_grads, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-4          # tests/test_recommend_gpu.py: encode_users / encode_items + pair_score against the forward
KINDS = ["deepconn", "dual_att", "narre", "simple_siamese"]
SIZES = {"kernel_sizes": "3,5", "hidden_dim": 8, "embedding_dim": 12, "att_dim": 4, "latent_dim": 4, "dropout": 0.0, "arch": "CNN",
         "l_window_size": 5, "l_out_size": 8, "g_out_size": 4, "emb_size": 12, "hidden_size_1": 10, "hidden_size_2": 5,
         "word_dropout": 0.0, "review_dropout": 0.0}


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    root = tmp_path_factory.mktemp("latents")
    make_dataset.write_doc_split(str(root / "doc"))
    make_review_dataset.write_review_split(str(root / "rev"))
    return {"doc": str(root / "doc"), "rev": str(root / "rev")}


def _setup(kind, splits, B=16):
    """(model on the device, the model's arguments for the first B training pairs, u_ids, i_ids)"""
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.trainer import Args, make_model
    if kind in ("narre", "simple_siamese"):
        ds = D.ReviewDataset(splits["rev"], "train", feed="ids")
        feed = D.DeviceReviewCache(ds, DEV).feed(kind, True)
    else:
        ds = D.DocDataset(splits["doc"], "train", with_ids=kind == "deepconn", feed="ids")
        feed = D.DeviceDocCache(ds, DEV)
    torch.manual_seed(0)
    model = quiet(make_model, kind, Args(dict(SIZES)), ds).to(DEV)
    u = torch.tensor([int(e[0]) for e in ds.examples[:B]], device=DEV)
    i = torch.tensor([int(e[1]) for e in ds.examples[:B]], device=DEV)
    return model, feed.inputs(u, i, with_ids=kind != "dual_att"), u, i


def _head(model, ul, il, u, i):
    """The model's own head over latent rows, in torch (dropout 0): FM.forward / D-ATT's inner product."""
    mode, h, g, ub, ib = model.score_mode_and_params()
    if mode == "dot":
        return (ul * il).sum(1)
    s = torch.relu(ul * il) @ h.view(-1) + g
    if ub is not None:
        s = s + ub.view(-1)[u] + ib.view(-1)[i]
    return s


@pytest.mark.parametrize("kind", KINDS)
def test_eval_latents_score_as_the_forward(kind, splits):
    from review_based_recommender_amd import functional as RF
    model, batch, u, i = _setup(kind, splits)
    model.eval()
    with torch.no_grad():
        out = model(*batch)
        pred = out[0] if isinstance(out, tuple) else out
        ul, il = model.pair_latents(*batch)
    B = u.shape[0]
    assert ul.shape == il.shape and ul.shape[0] == B and ul.dim() == 2
    mode, h, g, ub, ib = model.score_mode_and_params()
    rows = torch.arange(B, device=DEV)
    ub_rows = ub.detach()[u] if ub is not None else None
    ib_rows = ib.detach()[i] if ib is not None else None
    score = RF.pair_score(mode, ul, il, rows, rows, h, g, ub_rows, ib_rows)
    err = float((score - pred).abs().max())
    print(f"{kind}: max |pair_score(pair_latents) - forward| = {err:.3e}")
    assert err <= FWD_TOL
    RF.check_id_errors(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_train_latents_carry_the_tower_gradients(kind, splits):
    """Train mode (every dropout of the tiny models is 0, so the two forwards see the same function): sum of the head over
    pair_latents, backward, against the model's own forward + backward -- every parameter's gradient within check_grads' bounds,
    none missing, all finite."""
    model, batch, u, i = _setup(kind, splits)
    model.train()
    twin = copy.deepcopy(model)
    out = twin(*batch)
    (out[0] if isinstance(out, tuple) else out).sum().backward()
    ul, il = model.pair_latents(*batch)
    assert ul.requires_grad and il.requires_grad
    _head(model, ul, il, u, i).sum().backward()
    torch.cuda.synchronize()
    ref, got = {}, {}
    for (k, p), q in zip(twin.named_parameters(), model.parameters()):
        assert p.grad is not None and q.grad is not None, k
        assert bool(torch.isfinite(q.grad).all()), k
        ref[f"grad/{k}"] = p.grad.detach().cpu().numpy()
        ref[f"gradl2/{k}"] = float(p.grad.double().norm())
        got[k] = q.grad
    check_grads(got, ref)
