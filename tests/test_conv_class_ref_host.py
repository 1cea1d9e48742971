"""tests/conv_class_ref.py checked on the CPU, before any GPU sees it: the bf16 rounding against a bit-level round-to-nearest-even,
the f32-class formulas against torch autograd in float64, every case of tests/test_conv_classes_edges_gpu.py against an f32
computation of the same class (the bounds must hold for legitimate f32 arithmetic), the coverage of the kernel instantiations
by the cases, and the sensitivity of the bounds to a subtly wrong kernel (two perturbations of the reference)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_class_ref as R
from edge_refs import check

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------------------------- rounding
def _rne_bits(x):
    """f32 -> bf16 -> f32, round to nearest even, as integer arithmetic on the f32 bits (finite inputs): add 0x7fff plus the
    lowest kept bit, drop the low 16 bits."""
    u = x.numpy().view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return torch.from_numpy(r.astype(np.uint32).view(np.float32))


def _from_bits(u):
    return torch.from_numpy(np.asarray(u, dtype=np.uint32).view(np.float32))


def test_rb_is_bitlevel_round_to_nearest_even():
    g = torch.Generator().manual_seed(1)
    rnd = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-40, 40, (4096,), generator=g).float())
    hi16 = np.random.default_rng(2).integers(0x0080, 0x7F00, 512, dtype=np.uint32) << 16          # normal, finite, both parities
    ties = _from_bits(hi16 | 0x8000)                                                              # exactly half way: to even
    above, below = _from_bits(hi16 | 0x8001), _from_bits(hi16 | 0x7FFF)
    sub = _from_bits(np.random.default_rng(3).integers(1, 0x007FFFFF, 512, dtype=np.uint32))      # subnormal f32 (residues of tiny values)
    x = torch.cat([rnd, ties, -ties, above, below, sub, -sub, torch.tensor([0.0, -0.0, 1.0, 2.0 ** -126, 3.3895314e38])])
    got, want = R.rb(x), _rne_bits(x)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    # ties went both ways: half of them up (odd kept bit), half down
    up = (R.rb(ties) > ties)
    assert bool(up.any()) and bool((~up).any())
    assert torch.equal(up, torch.from_numpy(((hi16 >> 16) & 1).astype(bool)))


def test_three_planes_are_exact_for_normal_f32():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=g).float())
    hi, mid, lo = R.planes(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    # the magnitudes the bound constants assume: half a bf16 spacing per plane
    assert bool((mid.abs() <= 2.0 ** -8 * x.abs()).all()) and bool((lo.abs() <= 2.0 ** -16 * x.abs()).all())
    assert bool(((x.double() - hi.double()).abs() <= R.half_spacing(x.double().abs())).all())
    a = torch.tensor([1.0, 1.5, 2.0, 3.99, 0.0, 2.0 ** -20], dtype=F64)
    assert torch.equal(R.half_spacing(a), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -28], dtype=F64))


# ------------------------------------------------------------------------------------------- formulas against torch autograd
_TINY = [
    R._c("same", 3, 11, 8, 9, [1, 3, 5], [2, 3, 2], 31, mask_p=0.3),
    R._c("same-gate-tanh", 2, 9, 4, 7, [3, 7], [3, 2], 32, gate=True, tanh=True),
    R._c("same-gate-mask", 3, 10, 8, 6, [5], [4], 33, gate=True, mask_p=0.4),
    R._c("valid", 3, 9, 8, 9, [2, 3, 4], [2, 2, 3], 34, valid=True, mask_p=0.3),
    R._c("valid-gate-tanh", 2, 8, 4, 7, [2, 4], [3, 2], 35, valid=True, gate=True, tanh=True),
    R._c("same-pad", 3, 12, 4, 9, [3], [3], 36, padding_idx=0, right_pad=True),
]


@pytest.mark.parametrize("case", _TINY, ids=lambda c: c.name)
def test_f32_class_formulas_equal_autograd(case):
    inp = R.make_inputs(case)
    table = inp.table.double().requires_grad_(True)
    ws = [w.double().requires_grad_(True) for w in inp.ws]
    bs = [b.double().requires_grad_(True) for b in inp.bs]
    gate = inp.gate.double().requires_grad_(True) if inp.gate is not None else None
    x = F.embedding(inp.ids, table)
    if inp.mask is not None:
        x = x.masked_fill(~inp.mask.unsqueeze(-1), 0.0)
    if gate is not None:
        x = x * gate.unsqueeze(-1)
    outs = []
    for w, b in zip(ws, bs):
        k = w.shape[2]
        y = F.conv1d(x.transpose(1, 2), w, b, padding=0 if inp.valid else (k - 1) // 2)
        y = torch.tanh(y) if inp.tanh else torch.relu(y)
        outs.append(F.max_pool1d(y, y.shape[-1]).squeeze(-1))
    want = torch.cat(outs, 1)
    want.backward(inp.d_feat.double())

    def close(a, b, what):
        assert float((a - b).abs().max()) <= 1e-12 * (float(b.abs().max()) + 1e-300), what

    fw = R.forward(inp, "f32", False)
    close(fw.feat, want.detach(), "feat")
    bw = R.backward(inp, fw.T, fw.bT, fw.feat, fw.argmax, "f32", False, False)
    tg = table.grad.clone()
    if inp.padding_idx is not None:
        tg[inp.padding_idx] = 0            # nn.Embedding(padding_idx): no gradient for that row
    close(bw["dtable"][0], tg, "dtable")
    for k in range(len(ws)):
        close(bw[f"dW{k}"][0], ws[k].grad, f"dW{k}")
        close(bw[f"db{k}"][0], bs[k].grad, f"db{k}")
    if gate is not None:
        close(bw["dgate"][0], gate.grad, "dgate")


# ------------------------------------------------------------------------------------- the cases: emulation inside the bounds
_FWD = {}


def _fwd(run):
    key = R.run_id(run)
    if key not in _FWD:
        case, cls, st = run
        _FWD[key] = R.forward(R.make_inputs(case), cls, st)
    return _FWD[key]


def _row_sink(case, inp):
    return case.name.startswith("B") and inp.gate is None


@pytest.mark.parametrize("run", R.ALL_RUNS, ids=R.run_id)
def test_f32_emulation_of_the_class_stays_inside_the_bounds(run):
    """Operands rounded as the class says, f32 accumulation by torch, a stored table rounded with rb; the backward from the
    emulation's own feat and argmax.  Every err / bound must be <= 1."""
    case, cls, st = run
    inp = R.make_inputs(case)
    fam = "emu " + R.run_id(run)
    ref = _fwd(run)
    emu = R.forward(inp, cls, st, dt=F32)
    check(fam, "T", emu.T, ref.T, ref.bT)
    check(fam, "feat", emu.feat, ref.feat, ref.bfeat)
    dwg, rows = R.backward_form(inp, cls, _row_sink(case, inp))
    want = R.backward(inp, ref.T, ref.bT, emu.feat, emu.argmax, cls, dwg, rows)
    got = R.backward(inp, emu.T, None if inp.gate is None else ref.bT, emu.feat, emu.argmax, cls, dwg, rows, dt=F32)
    for name, (val, bound) in want.items():
        check(fam, name, got[name][0], val, bound)


def test_cases_reach_every_instantiation_they_are_there_for():
    seen = {"gemm": set(), "pool": set(), "bwd_table": set(), "bwd_dw": set()}
    for case, cls, st in R.ALL_RUNS:
        inp = R.make_inputs(case)
        for k, v in R.expected_kernels(inp, cls, st, _row_sink(case, inp)).items():
            seen[k].add(v)
    assert {"prod_gemm_b16_kernel<3>", "prod_gemm_b16_kernel<1>", "prod_gemm_b16d_kernel<3,8>", "prod_gemm_b16d_kernel<1,8>",
            "rows_to_b16_kernel+prod_gemm_b16s_kernel", "prod_gemm_b16sd_kernel"} <= seen["gemm"], seen["gemm"]
    assert "gather_pool_kernel<true>" in seen["pool"]
    assert {"rows prod_gemm_b16_kernel<6>", "rows prod_gemm_b16_kernel<1>", "g_times_w_kernel"} <= seen["bwd_table"]
    assert {"dw_from_g_b16_kernel<3>", "dw_from_g_b16_kernel<1>", "window rows f32"} <= seen["bwd_dw"]

    def k(name, cls, st):
        case = next(c for c in R.F_CASES + R.B_CASES if c.name == name)
        inp = R.make_inputs(case)
        return R.expected_kernels(inp, cls, st, _row_sink(case, inp))

    # what each row of the case tables names
    assert k("F1", "bf16", True)["gemm"].startswith("rows_to_b16") and k("F2", "bf16", True)["gemm"].startswith("rows_to_b16")
    assert k("F4", "bf16x2", False)["gemm"] == "prod_gemm_b16d_kernel<3,8>" and k("F4", "bf16", True)["gemm"] == "prod_gemm_b16sd_kernel"
    assert k("F5", "bf16", True)["gemm"] == "prod_gemm_b16sd_kernel" and k("F5", "bf16", False)["gemm"] == "prod_gemm_b16_kernel<1>"
    # both sides of the three rules of the many-short-documents class
    for on, off in (("B4-512", "B4-511"), ("B4b-128", "B4b-129"), ("B6-2048", "B6-2049")):
        assert k(on, "bf16x3", False)["bwd_dw"] == "dw_from_g_b16_kernel<3>" and k(on, "bf16", True)["bwd_table"] == "rows prod_gemm_b16_kernel<1>"
        assert k(off, "bf16x3", False)["bwd_dw"] == "window rows f32" and k(off, "bf16", True)["bwd_table"] == "g_times_w_kernel"
    assert k("B2g", "bf16", True) == dict(k("B2", "bf16", True), bwd_table="g_times_w_kernel")       # gated: dW from G, sparse table product


@pytest.mark.parametrize("run", [r for r in R.ALL_RUNS if r[1] in ("bf16x2", "bf16") and r[0].name != "F8"], ids=R.run_id)
def test_reduced_class_is_distinguishable_from_the_f32_class(run):
    """The GPU test shows that a reduced class was engaged in two ways (conv_class_ref.engaged): feat is nearer to the class's own
    reference than to the f32-class one, and -- where the class's centre itself is outside the f32-class bound by R.ENGAGED_FACTOR
    -- feat leaves the f32-class bound somewhere.  The second can be asked of every bf16 run; of bf16x2 it cannot in general: its
    dropped plane products are ~2^-17 of a product with random signs, the f32-class bound (D + 4) EPS of the magnitudes is a worst
    case (at F4, D = 180, the bf16x2 centre sits at 0.07 of it).  The first is shown askable here on the f32 emulation."""
    case, cls, st = run
    ref, f32 = _fwd(run), _fwd((case, "f32", False))
    if cls == "bf16":
        assert _worst(ref.feat, f32.feat, f32.bfeat) > 2 * R.ENGAGED_FACTOR
    emu = R.forward(R.make_inputs(case), cls, st, dt=F32)
    near, outside = R.engaged(emu.feat, ref, f32)
    assert near and outside


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _worst(got, ref, bound):
    err = (got.double() - ref).abs()
    inf = torch.full_like(err, float("inf"))
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf)).max())


@pytest.mark.parametrize("name", ["F1", "F2", "F4", "B2", "B3"])
def test_a_dropped_k_chunk_leaves_the_bounds(name):
    """Perturbation 1, in the loosest class (bf16 with bf16 storage): the contraction without its last K chunk (the last D % 16
    columns of the rows, or the last 16) -- in the forward GEMM, and for the many-short-documents class in the row GEMM too."""
    case = next(c for c in R.F_CASES + R.B_CASES if c.name == name)
    inp = R.make_inputs(case)
    ref = _fwd((case, "bf16", True))
    bad = R.forward(inp, "bf16", True, drop_k=True)
    assert _worst(bad.T, ref.T, ref.bT) > 1 and _worst(bad.feat, ref.feat, ref.bfeat) > 1
    if name.startswith("B"):
        dwg, rows = R.backward_form(inp, "bf16", True)
        assert rows
        want = R.backward(inp, ref.T, ref.bT, ref.feat, ref.argmax, "bf16", dwg, rows)["dtable"]
        got = R.backward(inp, ref.T, ref.bT, ref.feat, ref.argmax, "bf16", dwg, rows, drop_k=True)["dtable"]
        assert _worst(got[0], *want) > 1


@pytest.mark.parametrize("name", ["F1", "F2", "F6", "B1", "B2"])
def test_a_tap_shifted_by_one_channel_leaves_the_bounds(name):
    """Perturbation 2: the last tap of a bank whose channel count is no multiple of 4 reads its neighbour channel's segment."""
    case = next(c for c in R.F_CASES + R.B_CASES if c.name == name)
    inp = R.make_inputs(case)
    bank = next(w for w, ch in enumerate(inp.chans) if ch % 4 != 0)
    ref = _fwd((case, "bf16", True))
    bad = R.forward(inp, "bf16", True, shift_bank=bank)
    assert _worst(bad.feat, ref.feat, ref.bfeat) > 1
