"""nn.Linear on the f32 MFMA GEMM (csrc/dense_misc.hip: gemm_body, gemm2_kernel, gemm_reduce_body, act_bwd_kernel, colsum_body)
through the C ABI -- rbr_linear_fwd / _bwd (one slice) and rbr_linear_fwd_ex / _bwd_ex (split along the contraction) -- at the
edges of the kernel's own constants: the 64 x 64 output tile, the 32-deep K chunk and the slices gemm_split cuts
(128 -> 64 + 64, 129 -> 96 + 33, 160 -> 96 + 64, 192 -> 3 x 64, 193 -> 96 + 96 + 1, 257 -> 96 + 96 + 65, 513 -> 5 x 96 + 33), on each of
the three contractions: IN in the forward, N for dW, OUT for d_x.

Every result against the float64 restatement of tests/edge_refs.py from the same f32 inputs:

    y = act(x @ W^T + b) * mul;   backward from the y the GPU saved:  g = d_y * mul * act'(y / mul),  dW = g^T x,  db = sum_n g,  d_x = g W

Per-element bounds (n + 4) * EPS * Abs with n = IN (pre), N (dW, db), OUT (d_x); y: bound(pre) * |mul|, Tanh (bound(pre) + 4 EPS) * |mul|.
Outputs start as 7.0: an output that is asked for is overwritten everywhere, one that is not (NULL) is not touched.
Every test prints its largest err / bound per tensor ("RATIO <family> <tensor> <value>")."""
import zlib

import numpy as np
import pytest
import torch

import edge_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _ceil(a, b):
    return (a + b - 1) // b


def gemm_split(M, N, K):
    """gemm_split of dense_misc.hip for an M x N x K product -> the slices' K extents (one entry: not split)."""
    tiles = _ceil(M, 64) * _ceil(N, 64)
    s = min(8, max(1, 512 // max(tiles, 1)))
    s = min(s, max(1, K // 64))
    kper = _ceil(_ceil(K, s), 32) * 32
    slices = _ceil(K, kper)
    if slices <= 1:
        return [K]
    return [min(kper, K - z * kper) for z in range(slices)]


def split_floats(M, N, K):
    s = len(gemm_split(M, N, K))
    return s * _ceil(M, 64) * _ceil(N, 64) * 4096 if s > 1 else 0


SLICES = {127: [127], 128: [64, 64], 129: [96, 33], 160: [96, 64], 192: [64, 64, 64], 193: [96, 96, 1], 257: [96, 96, 65],
          513: [96] * 5 + [33]}


def test_split_rule_of_this_file_is_the_issue_s():
    for K, want in SLICES.items():
        for M, N in ((1, 1), (65, 33), (130, 70)):
            assert gemm_split(M, N, K) == want, (M, N, K)


def _inputs(case, N, IN, OUT, bias, with_mul):
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x, W = torch.randn(N, IN, generator=g), torch.randn(OUT, IN, generator=g) / np.sqrt(IN)
    b = torch.randn(OUT, generator=g) * 0.1 if bias else None
    mul = (torch.rand(N, OUT, generator=g) > 0.4).float() * 2 if with_mul else None
    d_y = torch.randn(N, OUT, generator=g)
    return x, W, b, mul, d_y


def _dev(t):
    return None if t is None else t.to(DEV)


class _Linear:
    """One shape on the device; fwd / bwd through the plain (`ex` False) or the split entry points."""

    def __init__(self, N, IN, OUT, x, W, b, mul, act):
        from review_based_recommender_amd import _lib
        self.L_, self.N, self.IN, self.OUT, self.act = _lib.lib(), N, IN, OUT, act
        self.x, self.W, self.b, self.mul = _dev(x), _dev(W), _dev(b), _dev(mul)
        self.st = torch.cuda.current_stream().cuda_stream

    def fwd(self, ex, x=None):
        from review_based_recommender_amd._lib import dev_ptr as P
        L_, N, IN, OUT = self.L_, self.N, self.IN, self.OUT
        x = self.x if x is None else x
        y = torch.full((N, OUT), 7.0, device=DEV)
        a = (N, IN, OUT, P(x, F32, "x"), P(self.W, F32, "W"), P(self.b, F32, "b"), self.act, P(self.mul, F32, "mul"), P(y, F32, "y"))
        if ex:
            n_ws = L_.rbr_linear_fwd_ws_floats(N, IN, OUT)
            assert n_ws == split_floats(N, OUT, IN)              # split exactly when gemm_split says so
            ws = torch.empty(n_ws, device=DEV) if n_ws else None
            rc = L_.rbr_linear_fwd_ex(*a, P(ws, F32, "ws"), self.st)
        else:
            rc = L_.rbr_linear_fwd(*a, self.st)
        assert rc == 0, L_.rbr_last_error()
        torch.cuda.synchronize()
        return y

    def bwd(self, ex, y, d_y, want_dx, want_db):
        from review_based_recommender_amd._lib import dev_ptr as P
        L_, N, IN, OUT = self.L_, self.N, self.IN, self.OUT
        out = {"d_x": torch.full((N, IN), 7.0, device=DEV), "dW": torch.full((OUT, IN), 7.0, device=DEV),
               "db": torch.full((OUT,), 7.0, device=DEV)}
        if ex:
            n_ws = L_.rbr_linear_bwd_ex_ws_floats(N, IN, OUT)
            assert n_ws == N * OUT + split_floats(OUT, IN, N) + split_floats(N, IN, OUT)
            fn = L_.rbr_linear_bwd_ex
        else:
            n_ws = L_.rbr_linear_bwd_ws_floats(N, OUT)
            assert n_ws == N * OUT
            fn = L_.rbr_linear_bwd
        ws = torch.empty(n_ws, device=DEV)
        rc = fn(N, IN, OUT, P(self.x, F32, "x"), P(self.W, F32, "W"), P(y, F32, "y"), P(_dev(d_y), F32, "d_y"), self.act,
                P(self.mul, F32, "mul"), P(out["d_x"], F32, "d_x") if want_dx else None, P(out["dW"], F32, "dW"),
                P(out["db"], F32, "db") if want_db else None, P(ws, F32, "ws"), self.st)
        assert rc == 0, L_.rbr_last_error()
        torch.cuda.synchronize()
        return out


def _run(family, case, N, IN, OUT, act, bias, with_mul, idx):
    x, W, b, mul, d_y = _inputs(case, N, IN, OUT, bias, with_mul)
    lin = _Linear(N, IN, OUT, x, W, b, mul, act)
    _, _, ry, by = R.linear_fwd(x, W, b, act, mul)
    partial = [(False, True), (True, False), (False, False)][idx % 3]          # beside (d_x, db) both asked for
    for ex in (False, True):
        fam = f"{family}-{'split' if ex else 'plain'}"
        y = lin.fwd(ex)
        R.check(fam, "y", y, ry, by)
        ref = R.linear_bwd(x, W, y, d_y, act, mul)                                # from the y the GPU saved
        for want_dx, want_db in ((True, True), partial):
            got = lin.bwd(ex, y, d_y, want_dx, want_db)
            for k, (val, ab, n) in ref.items():
                if (k == "d_x" and not want_dx) or (k == "db" and not want_db):
                    assert bool((got[k] == 7.0).all()), f"{fam} {k}: written although NULL was passed"
                else:
                    R.check(fam, k, got[k], val, R.bound_of(n, ab))
        if ex and (len(gemm_split(N, OUT, IN)) > 1 or len(gemm_split(OUT, IN, N)) > 1 or len(gemm_split(N, IN, OUT)) > 1):
            y2 = lin.fwd(True)                                                   # partial tiles are added in slice order: same bits
            got2 = lin.bwd(True, y, d_y, True, True)
            got1 = lin.bwd(True, y, d_y, True, True)
            assert torch.equal(y, y2) and all(torch.equal(got1[k], got2[k]) for k in got1), f"{fam}: two runs differ"


def _options(idx):
    """act, bias, mul: the 12 combinations in 12 consecutive cases"""
    return idx % 3, (idx // 3) % 2 == 0, (idx // 6) % 2 == 1


# chunk (32) and tile (64) edges without a split: each boundary value on IN, on N (dW's contraction) and on OUT (d_x's)
_EDGE = (1, 31, 32, 33, 63, 64, 65, 97)
_SIDE = (1, 33, 64, 65)
TILE_CASES = []
for _i, _c in enumerate(_EDGE):
    TILE_CASES += [(_SIDE[_i % 4], _c, _SIDE[(_i // 2 + 1) % 4]), (_SIDE[(_i + 2) % 4], _c, _SIDE[(_i + 3) % 4]),
                   (_c, _SIDE[(_i + 1) % 4], _SIDE[_i % 4]), (_SIDE[(_i + 3) % 4], _SIDE[_i % 4], _c)]
TILE_CASES = list(dict.fromkeys(TILE_CASES))


@pytest.mark.parametrize("idx", range(len(TILE_CASES)))
def test_linear_tile_and_chunk_edges(idx):
    """N, IN, OUT over {1, 31, 32, 33, 63, 64, 65, 97} x {1, 33, 64, 65}: no contraction reaches 128, so the split entry points take
    one slice too (asserted from their workspace queries).
    Largest err / bound on an MI355X (plain and split alike): y 0.34, dW 0.30, db 0.15, d_x 0.32."""
    N, IN, OUT = TILE_CASES[idx]
    assert split_floats(N, OUT, IN) == 0 and split_floats(OUT, IN, N) == 0 and split_floats(N, IN, OUT) == 0
    act, bias, with_mul = _options(idx)
    _run("linear-tile", ("tile", N, IN, OUT), N, IN, OUT, act, bias, with_mul, idx)


SPLIT_CASES = [(N, IN, OUT) for IN in SLICES for N, OUT in ((1, 1), (65, 33), (130, 70))]


@pytest.mark.parametrize("idx", range(len(SPLIT_CASES)))
def test_linear_forward_contraction_slices(idx):
    """IN over {127, 128, 129, 160, 192, 193, 257, 513} (127: the last length that is not split; then every slice pattern above, the
    1-element slice of 193 and the odd slice counts 3 of 192 / 193 / 257 in the reduce kernel's pairwise loop) x (N, OUT) in
    {(1, 1), (65, 33), (130, 70)}; the plain entry points run the same shapes in one slice.  With N = 130 / 65 >= 128 / 64 the
    weight gradient's contraction is split too.
    Largest err / bound on an MI355X (plain and split alike): y 0.03, dW 0.19, db 0.01, d_x 0.20."""
    N, IN, OUT = SPLIT_CASES[idx]
    from review_based_recommender_amd import _lib
    assert (_lib.lib().rbr_linear_fwd_ws_floats(N, IN, OUT) > 0) == (len(SLICES[IN]) > 1)
    act, bias, with_mul = _options(idx)
    _run("linear-slices", ("split", N, IN, OUT), N, IN, OUT, act, bias, with_mul, idx)


# (N, IN, OUT): the split on dW's contraction N (127: not yet), then on d_x's contraction OUT
BWD_SPLIT_CASES = [(127, 5, 3), (128, 5, 3), (193, 33, 7), (128, 65, 64), (9, 5, 128), (7, 33, 193), (65, 64, 193), (193, 3, 193)]


@pytest.mark.parametrize("idx", range(len(BWD_SPLIT_CASES)))
def test_linear_backward_contraction_slices(idx):
    """N in {127, 128, 193} with small IN and OUT: gemm_split cuts dW = g^T x along N; OUT in {128, 193}: it cuts d_x = g W along
    OUT; (193, 3, 193): both, in the one gemm2_kernel launch, and their two reductions in the one gemm_reduce2_kernel launch.
    Largest err / bound on an MI355X (plain and split alike): y 0.36, dW 0.29, db 0.14, d_x 0.23."""
    N, IN, OUT = BWD_SPLIT_CASES[idx]
    from review_based_recommender_amd import _lib
    n_ws = _lib.lib().rbr_linear_bwd_ex_ws_floats(N, IN, OUT)
    assert (n_ws > N * OUT) == (N >= 128 or OUT >= 128)
    for act, bias, with_mul in ((idx % 3, True, True), ((idx + 1) % 3, False, False)):
        _run("linear-bwd-slices", ("bwd", N, IN, OUT, act), N, IN, OUT, act, bias, with_mul, idx)


@pytest.mark.parametrize("N,IN,OUT,row,col", [(33, 65, 64, 0, 64), (65, 193, 33, 64, 192), (65, 193, 33, 7, 0), (130, 128, 70, 129, 100)])
def test_linear_relu_keeps_nan(N, IN, OUT, row, col):
    """ReLU epilogues of gemm_body and gemm_reduce_body: one NaN in x[row, col] makes exactly row `row` of y NaN, as
    torch.relu(F.linear(x, W, b)) does; every other row is bit-equal to the clean run.  Both entry points (col = 192 is the
    1-element slice of IN = 193)."""
    x, W, b, _, _ = _inputs(("nan", N, IN, OUT), N, IN, OUT, True, False)
    lin = _Linear(N, IN, OUT, x, W, b, None, R.ACT_RELU)
    bad = x.clone()
    bad[row, col] = float("nan")
    want = torch.relu(torch.nn.functional.linear(bad.double(), W.double(), b.double()))
    assert bool(torch.isnan(want[row]).all()) and int(torch.isnan(want).sum()) == OUT
    for ex in (False, True):
        clean, y = lin.fwd(ex), lin.fwd(ex, _dev(bad))
        nan = torch.isnan(y).cpu()
        assert bool(nan[row].all()), f"ex={ex}: {int(nan[row].sum())} of {OUT} elements of the row that reads the NaN are NaN"
        assert int(nan.sum()) == OUT
        keep = torch.arange(N) != row
        assert torch.equal(y.cpu()[keep], clean.cpu()[keep])
