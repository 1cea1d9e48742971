"""The D-ATT gate kernels (csrc/datt_gates.hip) at the shapes where their own constants change the path taken, every form against
one plain float64 restatement on the CPU from the same f32 inputs:

    x = F.embedding(ids, table64);  pre = conv1d(x^T, w64, b0, padding (win-1)/2  |  kernel = L);  gate = sigmoid(pre)

The backward kernels consume the gate they saved, so the reference backward starts from the gate the GPU returned (cast to
float64): dpre = dgate * g * (1 - g) (global: (sum_l dgate[b,l]) * g_b * (1 - g_b)), pushed through the float64 graph.  With a
padding_idx the table row of that token gets no gradient; the token still feeds dw and db0.

Tolerances are per element.  For every compared element `Abs` is the same float64 formula evaluated on |table|, |w|, |b0| and
|dpre| (global: (sum_l |dgate|) * g (1 - g)) -- the sum of the magnitudes of the terms behind the element -- and the bound is

    (n + 4) * EPS * Abs,   EPS = 2^-24,   n = length of the longest sum behind an element of that tensor (any order):
        pre: win * E (local), L * E (global);   dw, db0: B * L;   dtable: B * L * win (local), B * L (global)

(n - 1 additions; the 4 covers the roundings inside a term: 1 - g, the two products of dpre and the product with x or w).
The gate gets 0.25 * bound(pre) + 4 * EPS: the sigmoid's slope is at most 1/4, expf and the division cost a few ulp of a value
<= 1.  In accumulate mode EPS * (|base| + Abs) is added for the final add.  An element with Abs == 0 (the pad row, rows of absent
tokens) has bound 0: it must be exactly 0, or bit-equal to the base in accumulate mode.  No element is left out.

Every test prints its largest err / bound per tensor ("RATIO <family> <tensor> <value>"); the largest seen on an MI355X stand in
the tests' docstrings (sums that go through atomics move in the last digit from run to run).
"""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24          # unit roundoff of f32
F32, I64 = torch.float32, torch.int64


# ------------------------------------------------------------------------------------------------------------------ inputs
def _inputs(case, B, L, E, kw, V, pad, distinct=False):
    """One seed per case.  table ~ 0.5 N(0,1), w ~ N(0,1) / sqrt(E * kw), b0 ~ 0.1 N(0,1), dgate ~ N(0,1), ids uniform in [0, V)
    (`distinct`: document 0 is a prefix of a permutation of the vocabulary) with right-padded tails of random length of the
    padding token (token 0 where there is no padding_idx); with B >= 2 document 0 has no tail and the last one is all padding."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    table = torch.randn(V, E, generator=g) * 0.5
    w = torch.randn(1, E, kw, generator=g) / np.sqrt(E * kw)
    b0 = torch.randn(1, generator=g) * 0.1
    dgate = torch.randn(B, L, generator=g)
    ids = torch.randint(0, V, (B, L), generator=g)
    if distinct:
        assert V >= L
        ids[0] = torch.randperm(V, generator=g)[:L]
    lens = torch.randint(0, L + 1, (B,), generator=g)
    if B >= 2:
        lens[0], lens[B - 1] = L, 0
    fill = 0 if pad is None else pad
    assert fill < V
    ids = torch.where(torch.arange(L).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, fill))
    return table, w, b0, ids, dgate, g


# --------------------------------------------------------------------------------------------------------------- reference
def _graph(table, w, b0, ids, is_global, pad, absolute):
    leaves = [(t.abs() if absolute else t).double().clone().requires_grad_(True) for t in (table, w, b0)]
    x = F.embedding(ids, leaves[0], padding_idx=pad).permute(0, 2, 1)
    pre = F.conv1d(x, leaves[1], leaves[2], padding=0 if is_global else (w.shape[2] - 1) // 2)
    return leaves, pre.reshape(ids.shape[0], -1)                       # [B, L] local, [B, 1] global


class _Ref:
    """Forward (pre, Abs(pre), gate) at construction; backward(gate_gpu, dgate) -> {name: (value, Abs)} for dtable, dw, db0."""

    def __init__(self, table, w, b0, ids, is_global, pad):
        self.B, self.L = ids.shape
        self.E, self.kw, self.is_global = table.shape[1], w.shape[2], is_global
        self.leaves, self.pre = _graph(table, w, b0, ids, is_global, pad, False)
        self.aleaves, self.apre = _graph(table, w, b0, ids, is_global, pad, True)
        self.gate = torch.sigmoid(self.pre.detach()).expand(self.B, self.L)
        # gate: |d sigmoid| <= 1/4 of the error of pre (n = kw * E terms), expf and the division: a few ulp of a value <= 1
        self.gate_bound = (0.25 * (self.kw * self.E + 4) * EPS * self.apre.detach() + 4 * EPS).expand(self.B, self.L)

    def backward(self, gate_gpu, dgate):
        g = gate_gpu.detach().cpu().double()
        d = dgate.cpu().double()
        if self.is_global:
            gb = g[:, :1]
            dpre, adpre = d.sum(1, keepdim=True) * gb * (1 - gb), d.abs().sum(1, keepdim=True) * gb * (1 - gb)
        else:
            dpre, adpre = d * g * (1 - g), d.abs() * g * (1 - g)
        self.pre.backward(dpre)
        self.apre.backward(adpre)
        names = ("dtable", "dw", "db0")
        n_pos = self.B * self.L
        self.n = {"dtable": n_pos * (1 if self.is_global else self.kw), "dw": n_pos, "db0": n_pos}
        return {k: (l.grad, a.grad) for k, l, a in zip(names, self.leaves, self.aleaves)}


def _check(family, name, got, ref, bound, base=None):
    """|got - ref| <= bound for EVERY element; where the bound is 0 that is exact equality (to 0, or bit for bit to `base`)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    if base is not None:
        zero = bound == 0
        assert torch.equal(got[zero], base[zero]), f"{family} {name}: an element without terms differs from the base"
        ref = ref + base.double()
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"RATIO {family} {name} {worst:.4f}")
    assert worst <= 1.0, f"{family} {name}: err / bound = {worst} at {int(ratio.argmax())}"


def _check_grads(family, ref, grads, got, bases=None):
    for k, t in got.items():
        val, ab = grads[k]
        bound = (ref.n[k] + 4) * EPS * ab
        base = None if bases is None or k not in bases else bases[k]
        if base is not None:
            # the final add of accumulate mode: one rounding of a value of magnitude <= |base| + Abs; Abs == 0 stays bound 0
            bound = torch.where(ab > 0, bound + EPS * (base.double().abs() + ab), torch.zeros_like(ab))
        _check(family, k, t.reshape(val.shape), val, bound, base)


def _functional_gate(table, w, b0, ids, dgate, is_global, pad, rows=None):
    """functional.datt_gate forward + backward -> gate, {dtable, dw, db0}"""
    from review_based_recommender_amd import functional as RF
    gl = [t.to(DEV).requires_grad_(True) for t in (table, w, b0)]
    gate = RF.datt_gate(gl[0], gl[1], gl[2], ids.to(DEV), is_global=is_global, padding_idx=pad, rows=rows)
    (gate * dgate.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return gate.detach(), {"dtable": gl[0].grad, "dw": gl[1].grad, "db0": gl[2].grad}


def _run_functional(family, case, B, L, E, kw, V, pad, is_global, distinct=False):
    table, w, b0, ids, dgate, _ = _inputs(case, B, L, E, kw, V, pad, distinct)
    ref = _Ref(table, w, b0, ids, is_global, pad)
    gate, got = _functional_gate(table, w, b0, ids, dgate, is_global, pad)
    _check(family, "gate", gate, ref.gate, ref.gate_bound)
    _check_grads(family, ref, ref.backward(gate, dgate), got)


# ----------------------------------------------------------------------------------------------------- 1. local gate, both forms
# (B, L, E, win, V), padding_idx, distinct ids in document 0
LOCAL_CASES = [
    # kGTile = 64 and the smallest shapes; documents shorter than the window's halo
    ((1, 1, 1, 1, 2), 0, False), ((1, 2, 3, 5, 4), 0, False), ((2, 3, 5, 7, 6), 0, False),
    ((3, 63, 4, 3, 50), 0, False), ((3, 64, 4, 3, 50), 0, False), ((3, 65, 4, 3, 50), 0, False),
    # kGWin = 256: many repeats per window / nearly all tokens distinct (256 keys in the 1024-slot hash) / one key, count 256
    ((2, 255, 12, 7, 40), 0, False), ((2, 256, 12, 7, 40), 0, False), ((2, 257, 12, 7, 40), 0, False),
    ((2, 257, 12, 5, 600), 0, True),
    ((2, 300, 8, 3, 1), None, False),     # V = 1: without a padding_idx, so that the single token is a key in the dense form too
    ((2, 300, 8, 3, 1), 0, False),        # the single token is the pad token: dtable all zero, dw and db0 not
    # lane and column passes
    ((2, 70, 63, 5, 30), 0, False), ((2, 70, 65, 5, 30), 0, False), ((2, 70, 127, 5, 30), 0, False),
    ((2, 70, 129, 5, 30), 0, False), ((2, 70, 257, 5, 30), 0, False),
    # documents across the 8 reduce groups
    ((9, 20, 5, 3, 11), 0, False), ((17, 20, 5, 3, 11), 0, False),
    # widths beyond kMaxKF = 9 (dense only); the last: win = 2 * kMaxKF + 1 and L < pad
    ((2, 40, 6, 9, 20), 0, False), ((2, 40, 6, 11, 20), 0, False), ((3, 12, 5, 19, 9), 0, False),
    # product-form bookkeeping: kGpRows = 128, cap = min(V, B * L)
    ((2, 40, 8, 3, 500), 0, False),
    ((4, 100, 8, 5, 127), 0, False), ((4, 100, 8, 5, 128), 0, False), ((4, 100, 8, 5, 129), 0, False),
    ((4, 100, 8, 5, 300), 0, False),
    # padding_idx in {0, 3, None}  (0: above)
    ((3, 65, 4, 3, 50), 3, False), ((3, 65, 4, 3, 50), None, False),
    ((2, 257, 12, 7, 40), 3, False), ((2, 257, 12, 7, 40), None, False),
]


@pytest.mark.parametrize("shape,pad,distinct", LOCAL_CASES)
def test_local_gate_edges(shape, pad, distinct, conv_mode):
    """functional.datt_gate(is_global=False) under conv_mode dense and product: gate, dtable, dw, db0 against float64.  Forced
    product mode applies for win <= 7; for win >= 9 rbr_datt_local_gate_prod_ws_bytes is 0 and both runs take the dense form.
    Largest err / bound on an MI355X -- dense: gate 0.14, dtable 0.04, dw 0.15, db0 0.11; product: gate 0.14, dtable 0.04,
    dw 0.21, db0 0.11."""
    from review_based_recommender_amd import _lib
    B, L, E, win, V = shape
    ws_bytes = _lib.lib().rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V)
    product = conv_mode == "product" and win <= 7
    assert (ws_bytes > 0) == product
    _run_functional("local-product" if product else "local-dense", (shape, pad, distinct), B, L, E, win, V, pad, False, distinct)


# ------------------------------------------------------------------------------------------------ 2. local gate above 64 KB of LDS
@pytest.mark.parametrize("shape", [(2, 70, 300, 5, 40), (1, 70, 400, 7, 40)])
def test_local_gate_above_64k_lds(shape):
    """The dense local gate with tiles above 64 KB of dynamic LDS: (64 + win - 1) * E * 4 = 81 600 / 112 000 bytes forward,
    (L + 2 pad + 64 E) * 4 = 77 096 / 102 704 bytes backward.  A launch the runtime refuses comes back as a RuntimeError.
    Largest err / bound on an MI355X: gate 0.0002, dtable 0.004, dw 0.04, db0 0.002."""
    from review_based_recommender_amd import _lib
    B, L, E, win, V = shape
    assert (64 + win - 1) * E * 4 > 64 * 1024 and (L + win - 1 + 64 * E) * 4 > 64 * 1024
    assert _lib.lib().rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V) == 0       # B * L < 4096: the dense form
    _run_functional("local-dense-64k", shape, B, L, E, win, V, 0, False)


# ------------------------------------------------------------------------------------------------- 3. global gate, plain backward
# (B, L, E, V), padding_idx
GLOBAL_CASES = (
    # vector and scalar forward, 16-column chunks with tail
    [((3, 37, E, 25), 0) for E in (1, 3, 4, 12, 16, 20, 100, 255)] +
    # thread loop over L
    [((2, L, 8, 50), 0) for L in (1, 255, 256, 257, 600)] +
    # document classes of global_gate_bwd_dw_kernel (256 / E classes, 8 rows in flight)
    [((17, 9, 100, 30), 0), ((33, 9, 128, 30), 0), ((5, 9, 129, 30), 0), ((3, 9, 256, 30), 0), ((3, 9, 300, 30), 0),
     ((600, 4, 1, 7), 0)] +
    # kStage = 2048 documents per pass
    [((2049, 4, 4, 9), 0)] +
    # padding_idx in {0, 3, None}  (0: above)
    [((3, 37, 12, 25), 3), ((3, 37, 12, 25), None)])


@pytest.mark.parametrize("shape,pad", GLOBAL_CASES)
def test_global_gate_edges(shape, pad):
    """functional.datt_gate(is_global=True, rows=None): gate, dtable, dw, db0 against float64.
    Largest err / bound on an MI355X: gate 0.18, dtable 0.11, dw 0.18, db0 0.02."""
    B, L, E, V = shape
    _run_functional("global-plain", (shape, pad), B, L, E, L, V, pad, True)


# --------------------------------------------------------------------- 4. global gate over token rows, and the accumulate forms
def _token_rows(ids_dev, V):
    """rbr_datt_token_rows directly (functional.datt_token_rows returns None below 4096 positions)."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd._lib import dev_ptr
    L_ = _lib.lib()
    B, L = ids_dev.shape
    rows = torch.empty(L_.rbr_datt_token_rows_ws_bytes(B, L, V), dtype=torch.uint8, device=DEV)
    assert L_.rbr_datt_token_rows(B, L, V, dev_ptr(ids_dev, I64, "ids"), rows.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream) == 0
    return rows


def _place(ids, doc, token, positions):
    ids[doc, torch.as_tensor(positions)] = token


def _rows_hot_5(ids, g):
    """token 5 at 100 positions of document 0 and 110 of document 1: its row of the occurrence matrix has more than kGgDense = 96
    non-zeros (L = 128 < 1024: one pass), the gg_dense_rows_kernel branch"""
    _place(ids, 0, 5, torch.randperm(ids.shape[1], generator=g)[:100])
    _place(ids, 1, 5, torch.randperm(ids.shape[1], generator=g)[:110])


def _rows_hot_7(n_early):
    def edit(ids, g):
        """token 7 nowhere but at every position of document 0 from 1000 on (28) and at n_early random ones below 1000.  The
        first pass of gg_rows_kernel sees positions 0..1023: n_early + 24 non-zeros; the row has n_early + 28.  n_early = 80
        (the issue's case): 104 in the first pass, dense at once.  n_early = 70: 94 <= kGgDense in the first pass, whose partial
        sums are dropped when the second pass reaches 98 -- dense only in the second pass."""
        ids[ids == 7] = 8
        _place(ids, 0, 7, torch.arange(1000, ids.shape[1]))
        _place(ids, 0, 7, torch.randperm(1000, generator=g)[:n_early])
    return edit


# (B, L, E, V), edit of the ids or None
ROWS_CASES = [((1, 4, 1, 3), None), ((3, 64, 12, 20), None), ((3, 68, 100, 20), None),
              ((2, 1028, 8, 40), None),                  # second 1024-position pass of gg_rows_kernel
              ((2, 128, 256, 30), None),                 # E at the four-chunk limit
              ((4, 128, 12, 9), _rows_hot_5), ((2, 1028, 8, 40), _rows_hot_7(80)), ((2, 1028, 8, 40), _rows_hot_7(70))]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ci", range(len(ROWS_CASES)))
def test_global_gate_rows_edges(ci, accumulate):
    """rbr_datt_global_gate_bwd_rows through the C ABI, on row maps from rbr_datt_token_rows, overwriting dtable (which starts
    as NaN: every element must be written) or adding to a random base (rows of absent tokens and the pad row bit-equal to it).
    The gate comes from rbr_datt_global_gate_fwd.
    Largest err / bound on an MI355X: gate 0.04, dtable 0.70, dw 0.05, db0 0.04."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd._lib import dev_ptr
    L_ = _lib.lib()
    (B, L, E, V), edit = ROWS_CASES[ci]
    pad = 0
    table, w, b0, ids, dgate, g = _inputs((ci, "rows"), B, L, E, L, V, pad)
    if edit is not None:
        edit(ids, g)
    ref = _Ref(table, w, b0, ids, True, pad)
    st = torch.cuda.current_stream().cuda_stream
    d = {k: t.to(DEV) for k, t in dict(table=table, w=w, b0=b0, ids=ids, dgate=dgate).items()}
    gate = torch.empty(B, L, device=DEV)
    assert L_.rbr_datt_global_gate_fwd(B, L, E, dev_ptr(d["ids"], I64, "ids"), dev_ptr(d["table"], F32, "t"), dev_ptr(d["w"], F32, "w"),
                                       dev_ptr(d["b0"], F32, "b0"), dev_ptr(gate, F32, "gate"), st) == 0
    rows = _token_rows(d["ids"], V)
    n_ws = L_.rbr_datt_global_gate_bwd_rows_ws_floats(B, L, E, V)
    assert n_ws > 0
    ws = torch.empty(n_ws, device=DEV)
    base = torch.randn(V, E, generator=g) if accumulate else None
    dtable = base.to(DEV) if accumulate else torch.full((V, E), float("nan"), device=DEV)
    dw, db0 = torch.full_like(d["w"], float("nan")), torch.full((1,), float("nan"), device=DEV)
    rc = L_.rbr_datt_global_gate_bwd_rows(B, L, E, V, dev_ptr(d["ids"], I64, "ids"), dev_ptr(d["table"], F32, "t"),
                                          dev_ptr(d["w"], F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(d["dgate"], F32, "dg"), pad,
                                          dev_ptr(dw, F32, "dw"), dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dt"),
                                          dev_ptr(ws, F32, "ws"), rows.data_ptr(), accumulate, st)
    assert rc == 0, L_.rbr_last_error()
    torch.cuda.synchronize()
    _check("global-rows", "gate", gate, ref.gate, ref.gate_bound)
    _check_grads("global-rows", ref, ref.backward(gate, dgate), {"dtable": dtable, "dw": dw, "db0": db0},
                 {"dtable": base} if accumulate else None)


@pytest.mark.parametrize("shape", [(2, 64, 257, 20), (2, 66, 12, 20)])
def test_global_gate_rows_refused_shapes_fall_back(shape):
    """E = 257 (more than four 64-column chunks) and L = 66 (L % 4 != 0): the workspace query answers 0, the entry point refuses
    with its message, and functional.datt_gate(rows=rows) gives the plain backward's result: dw and db0 bit for bit (fixed
    order), everything within the float64 bounds (the plain dtable is a sum of atomics)."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd._lib import dev_ptr
    L_ = _lib.lib()
    B, L, E, V = shape
    table, w, b0, ids, dgate, _ = _inputs((shape, "refused"), B, L, E, L, V, 0)
    assert L_.rbr_datt_global_gate_bwd_rows_ws_floats(B, L, E, V) == 0
    ids_dev = ids.to(DEV)
    rows = _token_rows(ids_dev, V)
    buf = torch.zeros(B * L + E * L + V * E + 64, device=DEV)
    p = dev_ptr(buf, F32, "buf")
    rc = L_.rbr_datt_global_gate_bwd_rows(B, L, E, V, dev_ptr(ids_dev, I64, "ids"), p, p, p, p, 0, p, p, p, p, rows.data_ptr(), 0,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    msg = L_.rbr_last_error().decode()
    assert "needs E <= 256 and L % 4 == 0" in msg and f"E={E} L={L}" in msg
    assert float(buf.abs().max()) == 0.0                       # refused before anything was launched
    ref = _Ref(table, w, b0, ids, True, 0)
    gate_p, plain = _functional_gate(table, w, b0, ids, dgate, True, 0, rows=None)
    gate_r, with_rows = _functional_gate(table, w, b0, ids, dgate, True, 0, rows=rows)
    assert torch.equal(gate_p, gate_r) and torch.equal(plain["dw"], with_rows["dw"]) and torch.equal(plain["db0"], with_rows["db0"])
    _check("global-plain", "gate", gate_r, ref.gate, ref.gate_bound)
    _check_grads("global-plain", ref, ref.backward(gate_r, dgate), with_rows)


PROD_SHARED_SHAPES = [(4, 100, 8, 5, 300), (2, 40, 8, 3, 500)]


@functools.lru_cache(maxsize=None)
def _prod_shared_and_private(shape, accumulate):
    """rbr_datt_local_gate_fwd_prod / _bwd_prod through the C ABI, once with the tower's shared row maps (rbr_datt_token_rows) and
    once with private ones -> (reference, its gradients, base, [(gate, grads) shared, (gate, grads) private]); run once per case
    and shared by the two tests below.  accumulate = 0 overwrites the whole dtable (it starts as NaN), accumulate = 1 adds the
    batch's rows to a random base (gp_dtable_rows_kernel)."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd._lib import dev_ptr
    L_ = _lib.lib()
    B, L, E, win, V = shape
    pad = 0
    table, w, b0, ids, dgate, g = _inputs((shape, "shared"), B, L, E, win, V, pad)
    ref = _Ref(table, w, b0, ids, False, pad)
    base = torch.randn(V, E, generator=g) if accumulate else None
    st = torch.cuda.current_stream().cuda_stream
    d = {k: t.to(DEV) for k, t in dict(table=table, w=w, b0=b0, ids=ids, dgate=dgate).items()}
    # the workspace query answers by the size rule unless the product form is forced; back to auto afterwards, the state every
    # test starts from (the library has no getter for the mode, and conftest's conv_mode fixture leaves auto behind as well)
    L_.rbr_set_conv_mode(2)
    try:
        ws_bytes = L_.rbr_datt_local_gate_prod_ws_bytes(B, L, E, win, V)
    finally:
        L_.rbr_set_conv_mode(0)
    assert ws_bytes > 0
    outs = []
    for rows in (_token_rows(d["ids"], V), None):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        gate = torch.empty(B, L, device=DEV)
        rp = None if rows is None else rows.data_ptr()
        rc = L_.rbr_datt_local_gate_fwd_prod(B, L, E, win, V, dev_ptr(d["ids"], I64, "ids"), dev_ptr(d["table"], F32, "t"),
                                             dev_ptr(d["w"], F32, "w"), dev_ptr(d["b0"], F32, "b0"), dev_ptr(gate, F32, "gate"),
                                             ws.data_ptr(), rp, st)
        assert rc == 0, L_.rbr_last_error()
        dtable = base.to(DEV) if accumulate else torch.full((V, E), float("nan"), device=DEV)
        dw, db0 = torch.full_like(d["w"], float("nan")), torch.full((1,), float("nan"), device=DEV)
        rc = L_.rbr_datt_local_gate_bwd_prod(B, L, E, win, V, dev_ptr(d["ids"], I64, "ids"), dev_ptr(d["table"], F32, "t"),
                                             dev_ptr(d["w"], F32, "w"), dev_ptr(gate, F32, "gate"), dev_ptr(d["dgate"], F32, "dg"), pad,
                                             dev_ptr(dw, F32, "dw"), dev_ptr(db0, F32, "db0"), dev_ptr(dtable, F32, "dt"),
                                             ws.data_ptr(), rp, accumulate, st)
        assert rc == 0, L_.rbr_last_error()
        torch.cuda.synchronize()
        outs.append((gate.cpu(), {"dtable": dtable.cpu(), "dw": dw.cpu(), "db0": db0.cpu()}))
    assert torch.equal(outs[0][0], outs[1][0])                 # one gate: the reference backward below starts from it
    return ref, ref.backward(outs[0][0], dgate), base, outs


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", PROD_SHARED_SHAPES)
def test_local_gate_prod_shared_rows_and_accumulate(shape, accumulate):
    """The token-product local gate with shared and with private row maps, overwriting and accumulating: gate, dtable, dw, db0
    of both against float64; in accumulate mode the pad row and the rows of absent tokens stay bit-equal to the base.
    Largest err / bound on an MI355X: gate 0.07, dtable 0.19, dw 0.012, db0 0.0003."""
    ref, grads, base, outs = _prod_shared_and_private(shape, accumulate)
    for fam, (gate, got) in zip(("local-product-shared", "local-product-private"), outs):
        _check(fam, "gate", gate, ref.gate, ref.gate_bound)
        _check_grads(fam, ref, grads, got, {"dtable": base} if accumulate else None)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", PROD_SHARED_SHAPES)
def test_local_gate_prod_shared_rows_bit_equal_private(shape, accumulate):
    """Between shared and private row maps: the same gate, dw and db0 bit for bit.  Rows are numbered in vocabulary order
    (gp_compact_kernel), a token's bucket of positions is ascending (gate_bwd_dx_kernel) and dw / db0 are summed in row order
    (gp_dw_partial_kernel), so the two runs do the same arithmetic -- as long as every (document, window) workgroup of
    gate_bwd_dx_kernel has one of the kGateCopies = 16 copies of the tap-sum table to itself: B * ceil(L / 256) <= 16.  Beyond
    that several workgroups add into one copy with f32 atomics, in arrival order."""
    B, L = shape[:2]
    assert B * ((L + 255) // 256) <= 16          # kGateCopies: the invariant holds up to here
    ref, grads, base, outs = _prod_shared_and_private(shape, accumulate)
    (gate_s, got_s), (gate_p, got_p) = outs
    for k in ("dw", "db0"):
        diff = (got_s[k].double() - got_p[k].double()).abs().reshape(grads[k][1].shape)
        bound = (ref.n[k] + 4) * EPS * grads[k][1]
        print(f"BITDIFF {k}: {int((diff > 0).sum())} of {diff.numel()} elements differ, largest difference "
              f"{float((diff / bound.clamp_min(1e-300)).max()):.4f} of the element's float64 bound")
    assert torch.equal(gate_s, gate_p)
    assert torch.equal(got_s["dw"], got_p["dw"]) and torch.equal(got_s["db0"], got_p["db0"])


# -------------------------------------------------------------------------------------------------- 5. the row maps themselves
def _uniform(lo=0, hi=None):
    return lambda B, L, V, g: torch.randint(lo, V if hi is None else hi, (B, L), generator=g)


# name: (B, L, V, ids(B, L, V, generator)) -- the edges of the ranking: block_rank_256 (rbr_wave.h) in gp_count_kernel and
# gp_compact_kernel, one workgroup per 256 vocabulary entries
ROW_MAP_CASES = {
    "one token, one position": (1, 1, 1, lambda B, L, V, g: torch.zeros(B, L, dtype=I64)),
    "V 255": (2, 40, 255, _uniform()),                       # one block, not full
    "V 256": (2, 40, 256, _uniform()),                       # one block, exactly full
    "V 257": (2, 40, 257, _uniform()),                       # one token into a second block
    "only token 256": (2, 40, 257, lambda B, L, V, g: torch.full((B, L), 256, dtype=I64)),      # the last block holds the only mark
    "empty leading blocks": (2, 64, 1000, _uniform(600, 1000)),                                 # base from zero block counts
    "one row": (4, 100, 300, lambda B, L, V, g: torch.full((B, L), 7, dtype=I64)),
    "cap full": (1, 70, 5000, lambda B, L, V, g: torch.randperm(V, generator=g)[:B * L].view(B, L)),      # cap = B * L < V
    "all waves full": (4, 64, 64, lambda B, L, V, g: torch.stack([torch.randperm(V, generator=g) for _ in range(B)])),
}


@functools.lru_cache(maxsize=None)
def _row_maps(name):
    """The ids of a case (host), and what rbr_datt_token_rows built for them, read through rbr_datt_token_rows_maps: n_rows,
    row_of_token [V], tok_of_row [cap] (all of it, not only the listed rows) and cap, as numpy arrays."""
    import ctypes as C
    from review_based_recommender_amd import _lib
    B, L, V, make = ROW_MAP_CASES[name]
    ids = make(B, L, V, torch.Generator().manual_seed(zlib.crc32(name.encode())))
    assert ids.shape == (B, L) and ids.dtype == I64 and 0 <= int(ids.min()) and int(ids.max()) < V
    rows = _token_rows(ids.to(DEV), V)
    torch.cuda.synchronize()
    rot, n, tor, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
    assert _lib.lib().rbr_datt_token_rows_maps(B, L, V, rows.data_ptr(), C.byref(rot), C.byref(n), C.byref(tor), C.byref(cap)) == 0

    def view(ptr, count):
        o = ptr.value - rows.data_ptr()
        assert 0 <= o and o + 4 * count <= rows.numel()
        return rows[o:o + 4 * count].view(torch.int32).cpu().numpy()

    return ids, int(view(n, 1)[0]), view(rot, V), view(tor, cap.value), cap.value


@pytest.mark.parametrize("name", list(ROW_MAP_CASES))
def test_token_rows_maps_exact(name):
    """rbr_datt_token_rows against numpy: with u = np.unique(ids), n_rows == len(u), tok_of_row[:n_rows] == u, row_of_token[u] ==
    arange(len(u)) and -1 at every other vocabulary entry.  Integers, no tolerance, no element left out."""
    B, L, V, _ = ROW_MAP_CASES[name]
    ids, n_rows, row_of_token, tok_of_row, cap = _row_maps(name)
    u = np.unique(ids.numpy())
    assert cap == min(V, B * L)
    assert n_rows == len(u)
    assert np.array_equal(tok_of_row[:n_rows], u)
    want = np.full(V, -1, dtype=np.int32)
    want[u] = np.arange(len(u), dtype=np.int32)
    assert np.array_equal(row_of_token, want)


@pytest.mark.parametrize("name", ["V 257", "empty leading blocks", "cap full"])
def test_conv_token_list_equals_gate_row_maps(name):
    """The token-product conv's list (compact_block<false> of textcnn_prod.hip: byte marks, the self-initialising prepare stage
    rbr_textcnn_prod_prepare on a 0xAB-filled workspace) on the same unmasked ids, a one-bank conv with the product form forced:
    the same n_rows, the same row_of_token, and tok_of_row (int64 there) equal to the gates' after the cast to int32.  The kept
    chain (compact_block<true>) is tied to this one by test_prepare_two_launch_gpu.py."""
    import ctypes as C
    from review_based_recommender_amd import _lib, functional as RF
    from review_based_recommender_amd._lib import dev_ptr, ptr_array
    L_ = _lib.lib()
    B, L, V, _ = ROW_MAP_CASES[name]
    ids, n_rows, row_of_token, tok_of_row, cap = _row_maps(name)
    table = torch.zeros(V, 8, device=DEV)
    ws = [torch.zeros(5, 8, 3, device=DEV)]
    L_.rbr_set_conv_mode(2)
    try:
        desc = RF._conv_desc(table, B, L, ws, RF.PAD_SAME, RF.ACT_RELU, 0)
        rec = RF._conv_fwd_buffers(type("Rec", (), {})(), desc, torch.device(DEV))
        assert rec.prod_ws is not None
        rec.prod_ws.fill_(0xAB)
        ids_dev = ids.to(DEV)
        rc = L_.rbr_textcnn_prod_prepare(C.byref(desc), dev_ptr(ids_dev, I64, "ids"), None, ptr_array(ws, F32, "w"),
                                         dev_ptr(rec.pidx, torch.int32, "pidx"), rec.prod_ws.data_ptr(), _lib.current_stream())
        assert rc == 0, L_.rbr_last_error()
        torch.cuda.synchronize()
        rot, n, tor, ccap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        assert L_.rbr_textcnn_token_list(C.byref(desc), rec.prod_ws.data_ptr(), C.byref(rot), C.byref(n), C.byref(tor), C.byref(ccap)) == 0
    finally:
        L_.rbr_set_conv_mode(0)

    def view(ptr, nbytes, dtype):
        o = ptr.value - rec.prod_ws.data_ptr()
        return rec.prod_ws[o:o + nbytes].view(dtype).cpu().numpy()

    assert ccap.value == cap
    assert int(view(n, 4, torch.int32)[0]) == n_rows
    assert np.array_equal(view(rot, 4 * V, torch.int32), row_of_token)
    conv_tok = view(tor, 8 * cap, torch.int64)[:n_rows]
    assert np.array_equal(conv_tok.astype(np.int32), tok_of_row[:n_rows]) and int(conv_tok.max()) < V


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
REFUSALS = {
    # name: ((B, L, E, kw, V), is_global, what the RuntimeError and -- for the C entry points -- rbr_last_error() must name)
    "even win": ((2, 10, 4, 4, 9), False, ("window must be odd", "got 4")),
    "win 21": ((2, 30, 4, 21, 9), False, ("window 21 exceeds",)),
    "E 500 at win 5": ((2, 10, 500, 5, 9), False, ("embedding dim 500 too large",)),      # forward tile of 136 000 bytes
    "global weight length": ((2, 10, 4, 9, 9), True, ("spans 9 positions", "have 10")),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gate_refusals(name):
    """Each refused call raises RuntimeError through functional with a message that names the offending value; for the three the
    library refuses, rbr_last_error() names it too (a global weight of the wrong length is refused by functional itself -- the C
    entry point takes no weight length -- so there the exception's text is what there is).  A valid call that follows gives the
    right result."""
    from review_based_recommender_amd import _lib
    (B, L, E, kw, V), is_global, words = REFUSALS[name]
    table, w, b0, ids, dgate, _ = _inputs(name, B, L, E, kw, V, 0)
    with pytest.raises(RuntimeError) as ei:
        _functional_gate(table, w, b0, ids, dgate, is_global, 0)
    for s in words:
        assert s in str(ei.value), (s, str(ei.value))
        if not is_global:
            assert s in _lib.lib().rbr_last_error().decode()
    _run_functional("global-plain" if is_global else "local-dense", (name, "after"), 3, 10, 4, 10 if is_global else 3, 9, 0, is_global)
