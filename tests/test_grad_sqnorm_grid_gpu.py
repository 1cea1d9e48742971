"""grad_sqnorm's grid follows the chunks it reads (csrc/clip_adam.hip): the norm HipClipAdam.clip_and_step returns against a
float64 norm, over tensor sizes around the 4096-element chunk, a misaligned view, 1 / 17 / 64 tensors, with and without a
table in compact row form whose sum of squares arrives as 1, 255 or 8192 partials.  Fixed summation order: two runs give
the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 4095, 4096, 4097, 3 * 4096 + 5)


def _misaligned(n, gen):
    """A contiguous leaf whose storage starts 4 bytes past a 16-byte boundary."""
    return torch.randn(n + 1, generator=gen).to(DEV)[1:].detach()


@pytest.mark.parametrize("n_sq", [0, 1, 255, 8192])          # 0: no row-form table
@pytest.mark.parametrize("n_tensors", [1, 17, 64])
def test_norm_matches_float64_and_is_reproducible(n_tensors, n_sq):
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import HipClipAdam
    gen = torch.Generator().manual_seed(100 * n_tensors + n_sq)
    params, grads = [], []
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    n_dense = n_tensors - (1 if n_sq else 0)
    for k in range(n_dense):
        n = SIZES[k % len(SIZES)]
        if k % 6 == 5:
            p, g = _misaligned(n, gen), _misaligned(n, gen)
            assert p.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4
        else:
            p, g = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
        p.requires_grad_(True)
        params.append(p)
        grads.append(g)
        total += g.double().square().sum()
    rg = None
    if n_sq:
        V, D = 300, 260                                   # 78000 elements: 19 whole chunks and a partial one, none of them read
        table = torch.randn(V, D, generator=gen).to(DEV).requires_grad_(True)
        listed = (torch.rand(V, generator=gen) < 0.4).to(DEV)
        row_map = torch.where(listed, torch.cumsum(listed, 0) - 1, -1).to(torch.int32)
        rows = torch.randn(int(listed.sum()), D, generator=gen).to(DEV)
        per_row = rows.double().square().sum(1)
        sq = torch.zeros(n_sq, dtype=torch.float64, device=DEV)
        sq.index_add_(0, torch.arange(per_row.numel(), device=DEV) % n_sq, per_row)
        total += per_row.sum()
        rg = RF.RowGradient(table, rows, sq.float(), row_map.data_ptr(), (row_map, rows))
        params.insert(len(params) // 2, table)             # the table in the middle: read chunks on both sides of the skipped ones
        grads.insert(len(grads) // 2 if len(grads) else 0, None)
    assert len(params) == n_tensors
    opt = HipClipAdam(params, lr=1e-3, row_grads=False)
    norms = []
    for _ in range(2):
        for p, g in zip(params, grads):
            p.grad = g
        if rg is not None:
            assert opt.put_exchanged_rows(table, rg)
        norms.append(opt.clip_and_step(None).clone())
    torch.cuda.synchronize()
    want = float(total.sqrt())
    assert abs(float(norms[0]) - want) <= 1e-6 * want, (float(norms[0]), want)
    assert torch.equal(norms[0], norms[1])
