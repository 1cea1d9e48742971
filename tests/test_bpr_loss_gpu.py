"""functional.bpr_loss (rbr_bpr_loss_fwd / _bwd) against a float64 torch restatement: loss and d_pred to rtol 1e-5 / atol 1e-6 --
both are fixed-order f32 sums of at most 900 terms, whose rounding bound is of order 1e-6 relative."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-6


def _ref(pred, n_neg, valid, d_loss=1.0):
    """(loss, d_pred) in float64 through autograd."""
    p = pred.detach().double().cpu().requires_grad_(True)
    B = p.shape[0] // (1 + n_neg)
    x = p[B:].view(n_neg, B) - p[:B][None, :]
    v = torch.ones(n_neg, B, dtype=torch.float64) if valid is None else valid.detach().double().cpu().view(n_neg, B)
    loss = (v * F.softplus(x)).sum() / v.sum().clamp_min(1.0)
    (loss * d_loss).backward()
    return loss.detach(), p.grad


def _run(pred, n_neg, valid, root=None):
    from review_based_recommender_amd import functional as RF
    p = pred.clone().requires_grad_(True)
    loss = RF.bpr_loss(p, n_neg, valid)
    loss.backward(RF.unit_scalar(p.device) if root is None else root)
    return loss.detach(), p.grad


def _close(got, ref):
    return torch.allclose(got.double().cpu(), ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("B,n_neg", [(1, 1), (300, 3)])
@pytest.mark.parametrize("valid_kind", ["none", "ones", "partial"])
def test_loss_and_gradient_against_float64(B, n_neg, valid_kind):
    g = torch.Generator().manual_seed(B + n_neg)
    pred = (torch.randn((1 + n_neg) * B, generator=g) * 3).to(DEV)
    valid = {"none": None, "ones": torch.ones(n_neg * B),
             "partial": (torch.rand(n_neg * B, generator=g) < 0.6).float()}[valid_kind]
    if valid_kind == "partial" and B == 1:
        valid = torch.zeros(n_neg * B)            # the only negative is missing
    valid = None if valid is None else valid.to(DEV)
    loss, grad = _run(pred, n_neg, valid)
    ref_loss, ref_grad = _ref(pred, n_neg, valid)
    print(f"B={B} n_neg={n_neg} {valid_kind}: loss {float(loss)!r} vs {float(ref_loss)!r}, "
          f"max grad err {float((grad.double().cpu() - ref_grad).abs().max()):.3e}")
    assert _close(loss, ref_loss) and _close(grad, ref_grad)
    # a root gradient that is not the cached unit scalar takes the backward entry: 1.0 gives the same bits, 2.5 scales
    loss1, grad1 = _run(pred, n_neg, valid, root=torch.ones((), device=DEV))
    assert torch.equal(loss1, loss) and torch.equal(grad1, grad)
    _, grad2 = _run(pred, n_neg, valid, root=torch.full((), 2.5, device=DEV))
    assert _close(grad2, _ref(pred, n_neg, valid, d_loss=2.5)[1])
    # fixed order: the same bits again
    loss_b, grad_b = _run(pred, n_neg, valid)
    assert torch.equal(loss_b, loss) and torch.equal(grad_b, grad)


def test_extreme_scores_stay_finite():
    B, n_neg = 300, 3
    g = torch.Generator().manual_seed(0)
    pred = torch.where(torch.rand((1 + n_neg) * B, generator=g) < 0.5, -80.0, 80.0).to(DEV)
    loss, grad = _run(pred, n_neg, None)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    ref_loss, ref_grad = _ref(pred, n_neg, None)
    assert _close(loss, ref_loss) and _close(grad, ref_grad)


@pytest.mark.parametrize("B,n_neg", [(1, 1), (300, 3)])
def test_no_valid_negative_gives_exact_zeros(B, n_neg):
    pred = torch.randn((1 + n_neg) * B, device=DEV) * 50
    valid = torch.zeros(n_neg * B, device=DEV)
    loss, grad = _run(pred, n_neg, valid)
    assert float(loss) == 0.0 and torch.equal(grad, torch.zeros_like(grad))
    _, grad = _run(pred, n_neg, valid, root=torch.full((), 3.0, device=DEV))
    assert torch.equal(grad, torch.zeros_like(grad))


def test_forward_without_gradient_and_positive_gradient_is_minus_its_negatives():
    from review_based_recommender_amd import functional as RF
    B, n_neg = 300, 3
    pred = torch.randn((1 + n_neg) * B, device=DEV)
    with torch.no_grad():
        loss0 = RF.bpr_loss(pred, n_neg)
    loss, grad = _run(pred, n_neg, None)
    assert torch.equal(loss0, loss)
    own = grad[B:].view(n_neg, B)
    acc = torch.zeros(B, device=DEV)
    for j in range(n_neg):                       # the kernel's order: j ascending
        acc = acc + own[j]
    assert torch.equal(grad[:B], -acc) and float(grad[B:].min()) > 0.0
