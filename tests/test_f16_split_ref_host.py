"""Host checks of tests/f16_split_ref.py (no GPU): the rounding against a bit-level f16, the bound against an f32 CPU emulation of
the class (operands split as specified, f32 accumulation), and the bound's teeth: a dropped K chunk and an unscaled weight plane
lie outside it."""
import numpy as np
import pytest
import torch

import f16_split_ref as R
from edge_refs import check

F32, F64 = torch.float32, torch.float64


def _f16_bits_rne(x):
    """f32 -> f16 -> f32 by integer arithmetic on the bit patterns (finite inputs): round to nearest even at 10 stored bits, gradual
    underflow below 2^-14, overflow to inf from 65520."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign, mag = b & 0x80000000, b & 0x7FFFFFFF
    e = (mag >> 23) - 127
    out = np.zeros_like(mag, dtype=np.float64)
    for i, (m, ee) in enumerate(zip(mag, e)):
        if m == 0:
            continue
        sig = (m & 0x7FFFFF) | (0x800000 if ee > -127 else 0)          # 24-bit significand: value = sig * 2^(ee - 23)
        ee = max(ee, -126)
        drop = 13 if ee >= -14 else 13 + (-14 - ee)                     # bits below an f16 spacing (2^(ee-10), or 2^-24 when subnormal)
        if drop >= 26:
            q = 0
        else:
            q, rem = sig >> drop, sig & ((1 << drop) - 1)
            half = 1 << (drop - 1)
            q += 1 if rem > half or (rem == half and (q & 1)) else 0
        v = float(q) * 2.0 ** (ee - 23 + drop)
        out[i] = np.inf if v >= 65520.0 else v
    return np.where(sign != 0, -out, out)


def test_rounding_matches_a_bit_level_f16():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4000, generator=g) * torch.ldexp(torch.ones(4000), torch.randint(-30, 17, (4000,), generator=g)),
                   torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25,
                                 3 * 2.0 ** -25, 2.0 ** -26, 65504.0, 65519.0, 65520.0, -65520.0, 32768.0, -2.0 ** -15])]).to(F32)
    want = torch.from_numpy(_f16_bits_rne(x.numpy())).to(F32)
    assert torch.equal(R.rh(x), want)
    fl = R.rh(x, flush=True)
    assert torch.equal(fl, torch.where(want.abs() < 2.0 ** -14, torch.zeros_like(want), want))


def test_exponent_comes_from_the_exponent_field_and_lands_in_the_binade():
    a = torch.tensor([1.0, 1.5, 2.0, 0.02, 3.9e-20, 7e19, 2.0 ** -126, 1e-40, 65504.0], dtype=F32)
    s = R.exponent_of(a)
    y = torch.ldexp(a.double(), s)
    assert bool(((y >= 2.0 ** 14) & (y < 2.0 ** 15))[:7].all()) and float(y[7]) < 2.0 ** 15       # a subnormal amax stays below the binade
    assert float(R.rh(torch.ldexp(torch.tensor(np.nextafter(np.float32(2.0), np.float32(0))), torch.tensor(13))).max()) <= 32768.0
    assert R.exponent_of(torch.tensor([0.0, float("inf"), float("nan")])).tolist() == [0, 0, 0]
    normal = a >= 2.0 ** -126                                                                          # the supported domain
    assert R.exponent_of(torch.ldexp(a, torch.tensor(7)))[normal].tolist() == (s - 7)[normal].tolist()   # exponent-following
    x = torch.tensor([[1.0, float("nan"), 3.0], [1.0, float("inf"), -5.0], [0.0, 0.0, 0.0], [1.0, -4.0, 2.0]])
    am = R.amax_of(x, 1)
    assert torch.isnan(am[0]) and torch.isinf(am[1]) and am[2:].tolist() == [0.0, 4.0]


def test_two_planes_carry_22_bits_and_the_residue_is_exact():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(64, 300, generator=g)
    s = R.exponent_of(R.amax_of(x, 1))[:, None]
    h1, h2 = R.planes(x, s)
    y = torch.ldexp(x, s).double()
    normal = ~R.under_normal(x, s)
    t = (y - h1.double() - h2.double()).abs()
    assert bool((t[normal] <= 2.0 ** -22 * y.abs()[normal]).all())
    assert bool((t[~normal] <= 2.0 ** -25).all())
    assert float(h1.abs().max()) <= 32768.0 and bool((h2.abs() <= 2.0 ** -11 * y.abs().float() * (1 + 2.0 ** -10)).all())


def _operands(name):
    base = R.make_case("F4")
    if name == "F4":
        return base
    if name == "D300":
        return R.make_case("D300", D=300, seed=105)
    if name == "small-table":
        return R.with_table(base, name, base.table * 1e-3, [w * (10.0 / float(w.abs().max())) for w in base.ws])
    if name == "outlier":
        t = base.table.clone()
        t[:, 7] *= 2.0 ** 20
        return R.with_table(base, name, t)
    return R.scaled(base, int(name[1:]))          # "s40", "s-60": table * 2^s, weights * 2^-s


@pytest.mark.parametrize("name", ["F4", "D300", "s40", "s-40", "s60", "s-60", "small-table", "outlier"])
def test_f32_emulation_of_the_class_stays_inside_the_bound(name):
    inp = _operands(name)
    Wp = R.wprod(inp.ws)
    T, ab, bT = R.product_table(inp.table, Wp)
    for flush in (False, True):
        Te, _, _ = R.product_table(inp.table, Wp, dt=F32, flush=flush, exact=False)
        check(f"emu-{name}-{'flushed' if flush else 'honoured'}", "T", Te, T, bT)
    ref = R.forward(inp)
    emu = R.forward(inp, dt=F32, exact=False)
    check(f"emu-{name}", "feat", emu.feat, ref.feat, ref.bfeat)


@pytest.mark.parametrize("s", [40, -40, 60, -60])
def test_power_of_two_scales_give_the_same_table_bit_for_bit(s):
    base = R.make_case("F4")
    T0, _, _ = R.product_table(base.table, R.wprod(base.ws), dt=F32, exact=False)
    sc = R.scaled(base, s)
    Ts, _, _ = R.product_table(sc.table, R.wprod(sc.ws), dt=F32, exact=False)
    assert torch.equal(T0, Ts)


def _outside(got, ref, bound):
    return bool(((got.double() - ref).abs() > bound).any())


def test_a_dropped_k_chunk_lies_outside_the_bound():
    for name in ("F4", "D300"):
        inp = _operands(name)
        Wp = R.wprod(inp.ws)
        T, _, bT = R.product_table(inp.table, Wp)
        Td, _, _ = R.product_table(inp.table, Wp, dt=F32, drop_k=True, exact=False)
        assert _outside(Td, T, bT)
        assert float(((Td.double() - T).abs() > bT).double().mean()) > 0.9


def test_an_unscaled_weight_plane_lies_outside_the_bound():
    """Weights of magnitude 2^-45: without their scale both f16 planes underflow.  (At DeepCoNN's ~0.02 the unscaled split only loses
    the low plane's tail, 1.4e-6 against an accumulation bound of 1e-4: the scales are there for accuracy, this test for the bound.)"""
    inp = _operands("s40")
    Wp = R.wprod(inp.ws)
    T, _, bT = R.product_table(inp.table, Wp)
    Tu, _, _ = R.product_table(inp.table, Wp, dt=F32, unscaled_w=True, exact=False)
    assert _outside(Tu, T, bT)
    Ts, _, _ = R.product_table(inp.table, Wp, dt=F32, exact=False)
    assert not _outside(Ts, T, bT)


def test_cases_sit_on_the_sides_of_the_dispatch_rule_they_name():
    assert R.route(R.make_case("F4")) == (7, 12, True)
    assert R.route(R.make_case("D192", D=192)) == (7, 12, True)
    assert R.route(R.make_case("D300", D=300)) == (7, 19, True)
    assert R.route(R.make_case("six", chans=(56, 120))) == (6, 12, True)           # 3*56 + 5*120 = 768
    assert R.route(R.make_case("five", chans=(60, 92))) == (5, 12, False)          # 3*60 + 5*92 = 640
    assert R.route(R.make_case("D176", D=176)) == (7, 11, False)
