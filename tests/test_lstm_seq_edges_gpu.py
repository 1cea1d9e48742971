"""The bidirectional LSTM kernels (csrc/lstm_seq.hip: lstm_wt_kernel, lstm_fwd_kernel, lstm_bwd_kernel and the recurrent weight
gradient's product on dense_misc.hip's GEMM) through functional.lstm_seq / bilstm_encode against the float64 loops of
tests/lstm_ref.py, at the edges of the kernel's own constants: one sentence, fewer hidden units than a wave (64 lanes along the
hidden units: Hh 3, 16), Hh = 75 / 150 (no multiple of any tile; 128 and 192 lanes), Hh = 256 (the 8-sentence register tile), and
N either side of the sentence tile of each workgroup shape (64 sentences at Hh <= 48, 16 at 128 < Hh <= 192, 8 above).

Lengths: all full; mixed with 0, 1 and T; all zero; longest < T.

Forward: out and pooled element-wise within 2e-6 + 2e-4 |ref|.  argmax is not compared for equality: its position holds a float64
value within that tolerance of the float64 max, or it is -1 and the float64 max is within tolerance of 0.
Backward: the reference is differentiated with the KERNEL's argmax as the routing (lstm_ref.pooled_by_argmax), so no near-tie
can flip a comparison and no case is excluded; every gradient within 2e-6 + 2e-4 ||ref||_2; rows with len == 0 and positions
t >= len have gradient exactly 0.  Two runs give identical bits; pool=True equals out followed by the trimmed max by hand, bit
for bit.  Every case prints "RATIO <tensor> <err / err of torch's f32 CPU LSTM on the same inputs>"."""
import zlib

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64

SHAPES = [          # (N, T, E, Hh)
    (1, 1, 5, 3), (5, 7, 5, 3), (70, 9, 12, 16), (33, 33, 20, 75), (9, 20, 300, 150), (6, 4, 10, 256),
    (63, 3, 4, 3), (64, 3, 4, 3), (65, 3, 4, 3),            # 64-sentence tile (Hh <= 48)
    (31, 3, 4, 100), (33, 3, 4, 100),                       # two sentence groups of 8 per workgroup (96 < Hh <= 128): tiles of 16
    (15, 3, 6, 150), (16, 3, 6, 150), (17, 3, 6, 150),      # 16-sentence tile (128 < Hh <= 192)
    (7, 2, 3, 200), (9, 2, 3, 200),                         # 8-sentence tile (Hh > 192)
]
PATTERNS = ("full", "mixed", "zero", "short")


def _lengths(pattern, N, T, g):
    if pattern == "full":
        return torch.full((N,), T, dtype=torch.int64)
    if pattern == "zero":
        return torch.zeros(N, dtype=torch.int64)
    if pattern == "short":                                  # the batch's longest is below T (T = 1: nothing but empty rows fits)
        hi = max(T - 1, 0)
        l = torch.randint(0, hi + 1, (N,), generator=g)
        l[0] = hi
        return l
    l = torch.randint(0, T + 1, (N,), generator=g)
    for k, v in enumerate((0, 1, T)):                       # 0, 1 and T are present whenever N allows
        if k < N:
            l[(k * 7 + 1) % N] = v
    if N >= 1:
        l[0] = T if N == 1 else l[0]
    return l


def _case(shape, pattern):
    N, T, E, Hh = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, pattern)).encode()))
    x = torch.randn(N, T, E, generator=g)
    params = [torch.randn(4 * Hh, E, generator=g) / np.sqrt(E), torch.randn(4 * Hh, Hh, generator=g) / np.sqrt(Hh),
              torch.randn(4 * Hh, generator=g) * 0.1, torch.randn(4 * Hh, generator=g) * 0.1]
    params += [torch.randn(4 * Hh, E, generator=g) / np.sqrt(E), torch.randn(4 * Hh, Hh, generator=g) / np.sqrt(Hh),
               torch.randn(4 * Hh, generator=g) * 0.1, torch.randn(4 * Hh, generator=g) * 0.1]
    lengths = _lengths(pattern, N, T, g)
    wo = torch.randn(N, T, 2 * Hh, generator=g)
    wm = torch.randn(N, 2 * Hh, generator=g)
    return x, params, lengths, wo, wm


def _elem_ok(got, ref, what):
    err = (got.double() - ref).abs()
    bound = 2e-6 + 2e-4 * ref.abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"BOUND {what} max err/bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: err/bound {worst}"
    return float(err.max()) if err.numel() else 0.0


def _norm_ok(got, ref, what):
    err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
    bound = 2e-6 + 2e-4 * float(ref.norm())
    print(f"BOUND {what} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{what}: err {err} > {bound}"
    return err


def _torch_f32(x, params, lengths, wo, wm, t_out):
    """torch's own f32 CPU LSTM on the same inputs (the reference model's encoder + max), with its gradients."""
    N, T, E = x.shape
    Hh = params[1].shape[1]
    lstm = torch.nn.LSTM(E, Hh, batch_first=True, bidirectional=True)
    for k, p in zip(R.PARAM_NAMES, params):
        getattr(lstm, k).data = p.clone()
    xl = x.clone().requires_grad_(True)
    out, _ = lstm(pack_padded_sequence(xl, lengths.clamp(1, 1000), batch_first=True, enforce_sorted=False))
    out, _ = pad_packed_sequence(out, batch_first=True)
    out = out * (lengths != 0).float().view(N, 1, 1)
    pooled, _ = torch.max(out, dim=1)
    ((out * wo[:, :out.shape[1]]).sum() + (pooled * wm).sum()).backward()
    full = torch.zeros(N, T, 2 * Hh)
    full[:, :out.shape[1]] = out.detach()
    return full, pooled.detach(), xl.grad, [getattr(lstm, k).grad for k in R.PARAM_NAMES]


def _backward(loss):
    if loss.requires_grad:                  # nothing but empty rows: the float64 loops touch no input, every gradient is zero
        loss.backward()


def _g(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)


def _ratio(what, err, ref_err):
    print(f"RATIO {what} {err / max(ref_err, 1e-12):.2f}  (kernel {err:.2e}, torch f32 {ref_err:.2e})")


def _gpu_run(x, params, lengths, wo, wm):
    from review_based_recommender_amd import functional as Fn
    xd = x.to(DEV).requires_grad_(True)
    pd = [p.to(DEV).requires_grad_(True) for p in params]
    ld = lengths.to(DEV)
    out = Fn.bilstm_encode(xd, pd, ld, pool=False)
    pooled, argmax = Fn.bilstm_encode(xd, pd, ld, pool=True)
    ((out * wo.to(DEV)).sum() + (pooled * wm.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), pooled.detach().cpu(), argmax.cpu(), xd.grad.cpu(), [p.grad.cpu() for p in pd]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bilstm_encode_against_float64(shape, pattern):
    N, T, E, Hh = shape
    x, params, lengths, wo, wm = _case(shape, pattern)
    t_out = R.t_out_of(lengths, T)
    out, pooled, argmax, dx, dps = _gpu_run(x, params, lengths, wo, wm)

    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in params]
    ref = R.bilstm(x64, p64, lengths)
    ref_max, _ = R.trimmed_max(ref.detach(), lengths, t_out)
    e_out = _elem_ok(out, ref.detach(), "out")
    e_pool = _elem_ok(pooled, ref_max, "pooled")
    for n in range(N):
        assert float(out[n, int(lengths[n]):].abs().sum()) == 0.0

    # the argmax: a position that holds the float64 max within tolerance, or -1 with the float64 max within tolerance of 0
    tol = 2e-6 + 2e-4 * ref_max.abs()
    a = argmax.to(torch.int64)
    assert bool((a >= -1).all()) and bool((a < lengths.clamp(max=T).view(N, 1)).all())
    at = R.pooled_by_argmax(ref.detach(), a)
    assert bool(((at - ref_max).abs() <= tol).all())
    assert bool((a[lengths == 0] == -1).all())

    # pool=True is out followed by the trimmed max computed by hand, bit for bit in value
    hand, _ = R.trimmed_max(out, lengths, t_out)
    assert torch.equal(hand, pooled)

    # backward with the kernel's own argmax as the routing
    _backward((ref * wo.double()).sum() + (R.pooled_by_argmax(ref, a) * wm.double()).sum())
    errs = {"dx": _norm_ok(dx, _g(x64), "dx")}
    for k, got, p in zip(R.PARAM_NAMES, dps, p64):
        errs[k] = _norm_ok(got, _g(p), "d_" + k)
    for n in range(N):
        assert float(dx[n, int(lengths[n]):].abs().sum()) == 0.0
    assert torch.equal(dps[2], dps[3]) and torch.equal(dps[6], dps[7])        # the biases are added once: one gradient

    # how far from tight: torch's f32 CPU LSTM on the same inputs
    t_o, t_p, t_dx, t_dp = _torch_f32(x, params, lengths, wo, wm, t_out)
    _ratio("out", e_out, float((t_o.double() - ref.detach()).abs().max()))
    _ratio("pooled", e_pool, float((t_p.double() - ref_max).abs().max()))
    _ratio("dx", errs["dx"], float((t_dx.double() - _g(x64)).abs().max()))
    for k, tg, p in zip(R.PARAM_NAMES, t_dp, p64):
        _ratio("d_" + k, errs[k], float((tg.double() - _g(p)).abs().max()))

    # two runs give identical bits
    again = _gpu_run(x, params, lengths, wo, wm)
    for a1, a2 in zip((out, pooled, argmax, dx, *dps), (again[0], again[1], again[2], again[3], *again[4])):
        assert torch.equal(a1, a2)


@pytest.mark.parametrize("pattern", ("mixed", "zero"))
@pytest.mark.parametrize("shape", [(5, 7, 5, 3), (33, 9, 6, 75), (17, 5, 6, 150)], ids=lambda s: "x".join(map(str, s)))
def test_lstm_seq_d_xproj_and_per_sequence_t_out(shape, pattern):
    """functional.lstm_seq on a given xproj: d_xproj and d_w_hh, with one t_out per sequence (two sides whose longest differ)."""
    from review_based_recommender_amd import functional as Fn
    N, T, E, Hh = shape
    x, params, lengths, wo, wm = _case(shape, pattern)
    half = N // 2
    lengths = lengths.clone()
    lengths[:half] = lengths[:half].clamp(max=max(T - 2, 0))                  # the first side's longest is shorter
    sides = torch.cat([torch.full((half,), R.t_out_of(lengths[:half], T)), torch.full((N - half,), R.t_out_of(lengths[half:], T))])
    xp = R.xproj_of(x, params).contiguous()
    xd = xp.to(DEV).requires_grad_(True)
    wf, wr = params[1].to(DEV).requires_grad_(True), params[5].to(DEV).requires_grad_(True)
    ld = lengths.to(DEV)
    out = Fn.lstm_seq(xd, wf, wr, ld, pool=False)
    pooled, argmax = Fn.lstm_seq(xd, wf, wr, ld, pool=True, t_out=sides.to(DEV).to(torch.int32))
    ((out * wo.to(DEV)).sum() + (pooled * wm.to(DEV)).sum()).backward()

    x64 = xp.double().requires_grad_(True)
    w64 = [params[1].double().requires_grad_(True), params[5].double().requires_grad_(True)]
    ref = R.lstm_from_xproj(x64, w64[0], w64[1], lengths)
    ref_max, _ = R.trimmed_max(ref.detach(), lengths, sides)
    _elem_ok(out.detach().cpu(), ref.detach(), "out")
    _elem_ok(pooled.detach().cpu(), ref_max, "pooled (per-sequence t_out)")
    hand, _ = R.trimmed_max(out.detach().cpu(), lengths, sides)
    assert torch.equal(hand, pooled.detach().cpu())
    a = argmax.cpu().to(torch.int64)
    _backward((ref * wo.double()).sum() + (R.pooled_by_argmax(ref, a) * wm.double()).sum())
    dxp = xd.grad.cpu()
    _norm_ok(dxp, _g(x64), "d_xproj")
    _norm_ok(wf.grad.cpu(), _g(w64[0]), "d_w_hh_fwd")
    _norm_ok(wr.grad.cpu(), _g(w64[1]), "d_w_hh_rev")
    for n in range(N):
        assert float(dxp[n, int(lengths[n]):].abs().sum()) == 0.0


def test_refusals_on_the_device():
    from review_based_recommender_amd import functional as Fn
    xp = torch.zeros(2, 3, 8 * 257, device=DEV)
    w = torch.zeros(4 * 257, 257, device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        Fn.lstm_seq(xp, w, w, torch.ones(2, dtype=torch.int64, device=DEV), pool=False)
    xp = torch.zeros(1, 1001, 8, device=DEV)
    w = torch.zeros(4, 1, device=DEV)
    with pytest.raises(RuntimeError, match="1000"):
        Fn.lstm_seq(xp, w, w, torch.ones(1, dtype=torch.int64, device=DEV), pool=True)
    # lengths beyond T count as T
    xp = torch.randn(2, 3, 8 * 2, device=DEV)
    w = torch.randn(8, 2, device=DEV)
    a = Fn.lstm_seq(xp, w, w, torch.tensor([9, 3], device=DEV), pool=False)
    b = Fn.lstm_seq(xp, w, w, torch.tensor([3, 3], device=DEV), pool=False)
    assert torch.equal(a, b)
