"""rbr_clip_adam_step_rows leaves the compact rows as they are and the clip coefficient beside them: the update equals the
dense-gradient optimizer's, the clipped gradient is what functional.RowGradient.to_dense() / HipClipAdam.materialize_grads()
hand out (rows * coef, one rounding), and the rows buffer itself is not written.

Tables: V = 70, D = 8 (the generic row path) and V = 40, D = 260 (whole chunks on the wave path, the last chunk partial),
about 40 % of the rows listed, a 130-element dense tensor beside the table.

Three steps, as in test_fused_step_gpu.py, whose tolerances these are: the first two with a coefficient of exactly 1 (both
optimizers bit-equal), the third clipping in the `clipped` case.  The two norms are summed in different orders, so the
coefficients differ by an ulp or so; a clipping step that starts from equal state keeps that difference at rtol 1e-6 / 1e-5,
while several clipping steps in a row let it meet the cancellation in exp_avg = 0.9 m + 0.1 g c (measured: rtol 1e-5 missed at
the second of three clipping steps) -- that is the optimizers' arithmetic, not the row form's."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _optimizers(V, D, gen):
    from review_based_recommender_amd.train_step import HipClipAdam
    table0, other0 = torch.randn(V, D, generator=gen).to(DEV), torch.randn(130, generator=gen).to(DEV)
    pd = [table0.clone().requires_grad_(True), other0.clone().requires_grad_(True)]
    pr = [table0.clone().requires_grad_(True), other0.clone().requires_grad_(True)]
    keep, HipClipAdam.ROW_GRAD_MIN_ROWS = HipClipAdam.ROW_GRAD_MIN_ROWS, 1      # these small tables qualify for the row form
    try:
        orr = HipClipAdam(pr, lr=2e-3, row_grads=True)
    finally:
        HipClipAdam.ROW_GRAD_MIN_ROWS = keep
    assert len(orr._row_tables) == 1
    return pd, HipClipAdam(pd, lr=2e-3, row_grads=False), pr, orr


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("V,D", [(70, 8), (40, 260)])
def test_rows_stay_and_the_coefficient_is_applied_on_the_way_out(V, D, clipped):
    from review_based_recommender_amd import functional as RF
    gen = torch.Generator().manual_seed(11)
    pd, od, pr, orr = _optimizers(V, D, gen)
    F32 = torch.float32
    for step in range(3):
        max_norm = 0.05 if (clipped and step == 2) else 1e9
        exact = max_norm == 1e9
        listed = torch.rand(V, generator=gen) < 0.4
        listed[step] = True
        n = int(listed.sum())
        tok = listed.nonzero().flatten()
        order = torch.randperm(n, generator=gen)                     # list rows in no particular token order
        row_map = torch.full((V,), -1, dtype=torch.int32)
        row_map[tok] = order.to(torch.int32)
        rows = torch.zeros(n + 2, D)                                  # (spare rows behind the list, as the producer's capacity)
        rows[order] = torch.randn(n, D, generator=gen) * 0.1
        g = torch.zeros(V, D)
        g[tok] = rows[order]
        g_other = torch.randn(130, generator=gen)
        rows, row_map, g, g_other = rows.to(DEV), row_map.to(DEV), g.to(DEV), g_other.to(DEV)
        sq = rows.double().square().sum(1).view(-1).to(F32)           # one partial per list row
        rows_before = rows.clone()
        rg = RF.RowGradient(pr[0], rows, sq, row_map.data_ptr(), (row_map, rows))
        assert orr.put_exchanged_rows(pr[0], rg)
        pd[0].grad, pd[1].grad, pr[1].grad = g.clone(), g_other.clone(), g_other.clone()
        nd = od.clip_and_step(max_norm).clone()
        nr = orr.clip_and_step(max_norm).clone()
        torch.cuda.synchronize()
        assert abs(float(nd) - float(nr)) <= 1e-5 * float(nd)
        # the coefficient as the kernel derives it, in f32 from the norm it returned
        coef = torch.clamp(torch.tensor(max_norm, dtype=F32, device=DEV) / (nr + torch.tensor(1e-6, dtype=F32, device=DEV)), max=1.0)
        assert (float(coef) < 1.0) == (not exact)
        assert torch.equal(rg.rows, rows_before), "the rows buffer was written by the step"
        want = torch.zeros(V, D, device=DEV)
        want[tok.to(DEV)] = (rows_before * coef)[order.to(DEV)]
        assert torch.equal(rg.to_dense(), want)
        assert torch.equal(rg.to_dense(), want), "a second to_dense() scaled again"
        for a, b in zip(pd, pr):
            ma, mb, va, vb = od.state[a]["exp_avg"], orr.state[b]["exp_avg"], od.state[a]["exp_avg_sq"], orr.state[b]["exp_avg_sq"]
            if exact:
                assert torch.equal(a, b) and torch.equal(ma, mb) and torch.equal(va, vb), step
            else:
                assert torch.allclose(a, b, rtol=1e-6, atol=1e-7), step      # an ulp of the clip coefficient
                assert torch.allclose(ma, mb, rtol=1e-5, atol=1e-12), step
                assert torch.allclose(va, vb, rtol=1e-5, atol=1e-20), step
        assert pr[0].grad is None
        orr.materialize_grads()
        assert torch.equal(pr[0].grad, want)
        orr.materialize_grads()
        assert torch.equal(pr[0].grad, want), "materialize_grads() twice scaled or added twice"
        assert torch.equal(rg.rows, rows_before)
        if not exact:
            assert torch.allclose(pr[0].grad, pd[0].grad, rtol=1e-5, atol=0) and torch.allclose(pr[1].grad, pd[1].grad, rtol=1e-5, atol=0)
        else:
            assert torch.equal(pr[0].grad, pd[0].grad) and torch.equal(pr[1].grad, pd[1].grad)
        orr.zero_grad(); od.zero_grad()
