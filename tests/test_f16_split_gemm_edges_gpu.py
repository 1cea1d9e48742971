"""The "f16x2s" realisation of the bf16x3 class (rbr_set_prod_split; prod_gemm_f16d_kernel, the two-plane pack form and the
exponent blocks of the launch in front of it), element by element against the float64 restatement tests/f16_split_ref.py, at the
smallest shapes that reach the route: conv_class_ref's F4 (4 docs x 64 tokens, V = 300, D = 180, widths [3, 5] x [60, 120] channels:
7 column groups -- the second group of the last workgroup pair does not exist --, 12 K steps with 4 live columns in the last, a row
block cut by the end of the list) and its variants.  Every case runs the conv forward through the C ABI: the features through
functional.textcnn, the product table T through rbr_textcnn_prod_prepare + rbr_textcnn_prod_table on a workspace of the test's own,
read back where the layout puts it (the last region of the workspace).

Largest err / bound observed on an MI355X (the RATIO lines), per family:
                                              T        feat
  shapes (F4, D192, D300, six, short,
          three-blocks, masked-doc)           0.0055   0.0018     (T: six)
  operand range  2^+-40, 2^+-60               0.0044   0.0016     (bit-equal to the unscaled case)
                 small table, large weights   0.0056   0.0014
                 outlier row (floor term)     0.0243   0.0101
  subnormal low planes                        0.0001   --         the matrix pipe HONOURS f16 subnormal operands: squared distance
                                                                  6.0e-22 to the "honoured" variant, 1.6e-15 to the "flushed" one
  bf16x3 split / five groups (bound3)         0.0034   0.0012
The bf16x3 split is held to the six-product class's bound3 here; against the library built from the parent commit its features were
compared once on an MI355X and are equal bit for bit.
The bounds are worst-case accumulation bounds, (3 n + 4) EPS Abs: a correct kernel sits two orders below them, a dropped K chunk
or an unscaled plane above (tests/test_f16_split_ref_host.py).
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import conv_class_ref as CR
import f16_split_ref as R
from edge_refs import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


@pytest.fixture(autouse=True)
def product_mode():
    """Token-product formulation whatever the shape; the split and the mode restored."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import functional as RF
    lib = _lib.lib()
    try:
        lib.rbr_set_conv_mode(2)
        RF.set_prod_split(None)
        yield
    finally:
        lib.rbr_set_conv_mode(0)
        RF.set_prod_split(None)


def _features(inp, split=None):
    from review_based_recommender_amd import functional as RF
    RF.set_prod_split(split)
    feat = RF.textcnn(inp.table.to(DEV), inp.ids.to(DEV), inp.mask.to(DEV) if inp.mask is not None else None,
                      [w.to(DEV) for w in inp.ws], [b.to(DEV) for b in inp.bs], pad_mode=RF.PAD_SAME, act=RF.ACT_RELU)
    torch.cuda.synchronize()
    RF.set_prod_split(None)
    return feat.cpu()


def _table(inp, split=None):
    """-> (T [V, cp] on the CPU, listed [V] bool): the product-table rows of the tokens the batch lists."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import functional as RF
    RF.set_prod_split(split)
    L_ = _lib.lib()
    d = _lib.make_desc(inp.n_docs, inp.L, inp.D, inp.V, inp.kzs, inp.chans, RF.PAD_SAME, RF.ACT_RELU, None)
    RF.set_prod_split(None)
    nbytes = L_.rbr_textcnn_fwd_ws_bytes(C.byref(d))
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    pidx = torch.zeros(L_.rbr_textcnn_partial_elems(C.byref(d)), dtype=torch.int32, device=DEV)
    table, ids = inp.table.to(DEV).contiguous(), inp.ids.to(DEV).contiguous()
    mask8 = inp.mask.to(DEV).to(torch.uint8).contiguous() if inp.mask is not None else None
    wts = [w.to(DEV).contiguous() for w in inp.ws]
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L_.rbr_textcnn_prod_prepare(C.byref(d), ids.data_ptr(), mask8.data_ptr() if mask8 is not None else None,
                                           _lib.ptr_array(wts, F32, "W"), pidx.data_ptr(), ws.data_ptr(), st), "prod_prepare")
    _lib.check(L_.rbr_textcnn_prod_table(C.byref(d), table.data_ptr(), ws.data_ptr(), st), "prod_table")
    torch.cuda.synchronize()
    rot, cap = C.c_void_p(), C.c_int32()
    _lib.check(L_.rbr_textcnn_token_list(C.byref(d), ws.data_ptr(), C.byref(rot), None, None, C.byref(cap)), "token_list")
    off = rot.value - ws.data_ptr()
    row_of_token = ws[off:off + 4 * inp.V].view(torch.int32).cpu().long()
    cp = sum(k * c for k, c in zip(inp.kzs, inp.chans))
    pitch = -(-cp // 128) * 128
    tbytes = ((cap.value + 1) * pitch + 4) * 4
    tbytes = (tbytes + 255) // 256 * 256                         # the product table is the workspace's last region
    T = ws[nbytes - tbytes:nbytes - tbytes + (cap.value + 1) * pitch * 4].view(F32).view(cap.value + 1, pitch).cpu()
    assert float(T[cap.value].abs().max()) == 0.0                # the zero row: the region is where the layout puts it
    listed = row_of_token >= 0
    want = torch.zeros(inp.V, dtype=torch.bool)
    live = inp.ids if inp.mask is None else inp.ids[inp.mask]
    want[live.reshape(-1)] = True
    assert torch.equal(listed, want)
    out = torch.zeros(inp.V, cp)
    out[listed] = T[row_of_token[listed], :cp]
    finite = torch.isfinite(inp.table).all(1) & listed           # (a poisoned row is NaN in every column: inf * 0)
    assert float(T[row_of_token[finite], cp:].abs().max()) == 0.0 if pitch > cp else True      # padding columns: zero weights, exponent 0
    return out, listed


_REF = {}


def _ref(inp):
    if inp.name not in _REF:
        _REF[inp.name] = R.forward(inp)
    return _REF[inp.name]


def _check_case(inp, family):
    ref = _ref(inp)
    T, listed = _table(inp)
    check(family, f"{inp.name} T", T[listed], ref.T[listed], ref.bT[listed])
    feat = _features(inp)
    check(family, f"{inp.name} feat", feat, ref.feat, ref.bfeat)
    return T, listed, feat


SHAPES = {
    "F4": dict(),
    "D192": dict(D=192, seed=111),                               # a whole last K step
    "D300": dict(D=300, seed=112),                               # 19 steps: the ring wraps six times and ends on slot 0
    "six": dict(chans=(56, 120), seed=113),                      # exactly 6 groups: every workgroup pair whole
    "short": dict(n_rows=40, seed=114),                          # a list shorter than one row block
    "three-blocks": dict(n_docs=8, V=400, seed=115),             # three row blocks, the last one cut
    "masked-doc": dict(masked_doc=2, seed=116),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_that_reach_the_route(name):
    inp = R.make_case(name, **SHAPES[name])
    assert R.route(inp)[2]
    T, listed, feat = _check_case(inp, "shapes")
    if name == "F4":                                             # the route is taken: the six-product kernel rounds differently
        T6, _ = _table(inp, "bf16x3")
        assert not torch.equal(T, T6)
        check("shapes", "F4 T bf16x3", T6[listed], _ref(inp).T[listed], CR.bound3(inp.D, _ref(inp).AbsT)[listed])


def test_five_groups_keep_the_ring_kernel_and_its_bits():
    inp = R.make_case("five", chans=(60, 92), seed=117)          # 3 * 60 + 5 * 92 = 640 columns
    assert R.route(inp)[:2] == (5, 12) and not R.route(inp)[2]
    T, listed = _table(inp)
    T6, _ = _table(inp, "bf16x3")
    assert torch.equal(T, T6)
    assert torch.equal(_features(inp), _features(inp, "bf16x3"))
    check("bf16x3", "five T", T[listed], _ref(inp).T[listed], CR.bound3(inp.D, _ref(inp).AbsT)[listed])


def test_bf16x3_split_is_the_six_product_kernel():
    """RBR_SPLIT_BF16X3 on the route's own shape: inside the bound of the six-product class (conv_class_ref.bound3)."""
    inp = R.make_case("F4")
    ref6 = CR.forward(inp_as_conv_class(inp), "bf16x3", False)
    check("bf16x3", "F4 feat", _features(inp, "bf16x3"), ref6.feat, ref6.bfeat)


def inp_as_conv_class(inp):
    return SimpleNamespace(**{**vars(inp), "gate": None, "valid": False, "tanh": False, "padding_idx": None})


@pytest.mark.parametrize("s", [40, -40, 60, -60])
def test_power_of_two_scales_follow_the_exponents_bit_for_bit(s):
    base = R.make_case("F4")
    feat0 = _features(base)
    sc = R.scaled(base, s)
    T, listed, feat = _check_case(sc, "range")
    assert torch.equal(feat, feat0)
    assert torch.equal(T, _table(base)[0])


def test_small_table_against_large_weights():
    base = R.make_case("F4")
    inp = R.with_table(base, "small-table", base.table * 1e-3, [w * (10.0 / float(w.abs().max())) for w in base.ws])
    _check_case(inp, "range")


def test_a_row_with_one_element_far_above_the_others():
    base = R.make_case("F4")
    t = base.table.clone()
    t[:, 7] *= 2.0 ** 20
    inp = R.with_table(base, "outlier", t)
    assert float(_ref(inp).bT.max()) > 0 and bool(R.under_normal(inp.table, R.exponent_of(R.amax_of(inp.table, 1))[:, None]).any())
    _check_case(inp, "range")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_row_poisons_only_the_documents_that_read_it(bad):
    base = R.make_case("F4")
    ids = base.ids.clone()
    v = int(ids[0, 5])
    other = (v + 1) % base.V
    ids[1:][ids[1:] == v] = other                                # only document 0 reads token v
    clean = R.with_table(base, "clean", base.table)
    clean.ids = ids
    t = base.table.clone()
    t[v, 11] = bad
    dirty = R.with_table(clean, "dirty", t)
    f0, f1 = _features(clean), _features(dirty)
    assert torch.equal(f0[1:], f1[1:])
    T0, listed = _table(clean)
    T1, _ = _table(dirty)
    keep = listed.clone()
    keep[v] = False
    assert torch.equal(T0[keep], T1[keep])
    assert not bool(torch.isfinite(T1[v]).all())


def test_subnormal_low_planes_observation():
    """Every low plane of the table is subnormal by construction: column 0 holds 1.0 (it sets each row's exponent, its plane is exact
    and its weights are zero), every other element is below 2^-18.  Observation: which variant of the reference the matrix pipe's
    result is nearer to -- printed, not asserted; the bound holds either way and IS asserted."""
    base = R.make_case("F4")
    g = torch.Generator().manual_seed(9)
    t = torch.randn(base.V, base.D, generator=g).clamp(-4, 4) * 2.0 ** -20
    t[:, 0] = 1.0
    ws = [w.clone() for w in base.ws]
    for w in ws:
        w[:, 0, :] = 0.0
    inp = R.with_table(base, "subnormal", t, ws)
    s = R.exponent_of(R.amax_of(inp.table, 1))[:, None]
    y = torch.ldexp(inp.table, s)
    low = (y - R.rh(y))[:, 1:]
    assert bool((low.abs() < R.F16_MIN_NORMAL).all()) and bool((low != 0).any())
    ref = _ref(inp)
    T, listed = _table(inp)
    check("subnormal", "T", T[listed], ref.T[listed], ref.bT[listed])
    Wp = R.wprod(inp.ws)
    dist = {}
    for flush in (False, True):
        Tv, _, _ = R.product_table(inp.table, Wp, flush=flush, exact=False)
        dist["flushed" if flush else "honoured"] = float((T[listed].double() - Tv[listed]).square().sum())
    print(f"SUBNORMAL f16 MFMA operands: nearer to '{min(dist, key=dist.get)}' (squared distance honoured {dist['honoured']:.3e}, "
          f"flushed {dist['flushed']:.3e})")
