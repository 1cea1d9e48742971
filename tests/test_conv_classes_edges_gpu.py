"""The token-product TextCNN in the arithmetic classes of its bf16-pipe GEMMs, element by element against the float64 restatement
of each class (tests/conv_class_ref.py), at the smallest shapes that cut a row block, leave a K chunk or a column group partial,
give a bank an odd channel count, or sit on either side of the many-short-documents rule.  conv_class_ref.expected_kernels says
which instantiation each run reaches; tests/test_conv_class_ref_host.py checks that the cases cover them, that legitimate f32
arithmetic stays inside the bounds, and that a dropped K chunk or a tap shifted by one channel does not.

Per run, with edge_refs.check (|got - ref| <= bound for EVERY element, exact 0 where the bound is 0):
  1. feat within its bound;  2. 0 <= argmax < pool length;  3. the window the kernel picked is maximal up to the arithmetic:
  y_ref[argmax] >= max_p y_ref - 2 max_p bound_y;  4. every gradient (table, each W, each bias, gate) from the kernel's own feat
  and argmax;  5. reduced classes: the class was engaged (conv_class_ref.engaged).
The many-short-documents runs take the table gradient in compact row form (functional.set_row_grad_sink), the only form in
which that class multiplies G out with the row GEMM; a gated conv there keeps the sparse product and still takes dW from G.

Largest err / bound observed on an MI355X (the RATIO lines), per family:
                                   feat    dtable  dW      dbias   dgate
  forward cases  bf16 + storage    0.9032  0.1228  0.2020  0.1933  0.4578     (feat: F6; dgate: F3 -- half spacings of the stored T)
                 bf16              0.0847  0.1228  0.2020  0.1933  0.0099     (the backward of these shapes is f32 in every class)
                 bf16x2            0.0441  0.1228  0.2020  0.1933  0.0045
  short docs     bf16x3            0.0313  0.0290  0.0028  0.0036  0.0030
                 bf16 + storage    0.9996  0.8314  0.9207  0.0036  0.9815     (feat: B6-2049; dtable: B4b-128; dW: B5; dgate: B2g)
Where something is rounded to bf16 (the stored T, G in the bf16 class) the bound is half a bf16 spacing and is reached: a ratio
just under 1 there is a value that sat next to a tie, not a bound without margin.
"""
import pytest
import torch

import conv_class_ref as R
from edge_refs import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def conv_class(request):
    """Token-product formulation whatever the shape, in the class (and storage form) of the run; all three settings restored."""
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import functional as RF
    cls, storage = request.param
    lib = _lib.lib()
    try:
        lib.rbr_set_conv_mode(2)
        RF.set_prod_precision(cls)
        lib.rbr_set_b16_storage(1 if storage else 0)
        yield cls, storage
    finally:
        lib.rbr_set_conv_mode(0)
        RF.set_prod_precision(None)
        lib.rbr_set_b16_storage(-1)


class _RowSink:
    """Takes the compact row gradient of every backward over its table (functional.set_row_grad_sink)."""

    def __init__(self):
        self.got = None

    def wants_row_grad(self, table):
        return True

    def put_row_grad(self, table, row_grad):
        self.got = row_grad


_F32 = {}


def _f32_forward(case):
    if case.name not in _F32:
        _F32[case.name] = R.forward(R.make_inputs(case), "f32", False)
    return _F32[case.name]


def _run(case, cls, storage, row_sink):
    from review_based_recommender_amd import functional as RF
    inp = R.make_inputs(case)
    fam = R.run_id((case, cls, storage))
    nw = len(inp.ws)
    table = inp.table.to(DEV).requires_grad_(True)
    ws = [w.to(DEV).requires_grad_(True) for w in inp.ws]
    bs = [b.to(DEV).requires_grad_(True) for b in inp.bs]
    gate = inp.gate.to(DEV).requires_grad_(True) if inp.gate is not None else None
    row_sink = row_sink and gate is None
    sink = _RowSink()
    if row_sink:
        RF.set_row_grad_sink(table, sink)
    try:
        feat, argmax = RF.textcnn(table, inp.ids.to(DEV), inp.mask.to(DEV) if inp.mask is not None else None, ws, bs, gate=gate,
                                  pad_mode=RF.PAD_VALID if inp.valid else RF.PAD_SAME, act=RF.ACT_TANH if inp.tanh else RF.ACT_RELU,
                                  padding_idx=inp.padding_idx, return_argmax=True)
        feat.backward(inp.d_feat.to(DEV))
        torch.cuda.synchronize()
        if row_sink:
            assert table.grad is None and sink.got is not None
            dtable = sink.got.to_dense()
        else:
            dtable = table.grad
    finally:
        if row_sink:
            RF.set_row_grad_sink(table, None)
    feat_k, argmax_k = feat.detach().cpu(), argmax.cpu()

    ref = R.forward(inp, cls, storage)
    check(fam, "feat", feat_k, ref.feat, ref.bfeat)                                                       # 1
    coff = 0
    for w, (kz, ch) in enumerate(zip(inp.kzs, inp.chans)):
        am = argmax_k[:, coff:coff + ch].long()
        Lv = ref.y[w].shape[1]
        assert int(am.min()) >= 0 and int(am.max()) < Lv, f"{fam}: argmax of bank {w} outside [0, {Lv})"   # 2
        picked = ref.y[w].gather(1, am.unsqueeze(1)).squeeze(1)
        slack = 2 * ref.by[w].max(1).values
        assert bool((picked >= ref.y[w].max(1).values - slack).all()), f"{fam}: bank {w} pooled a window that is not maximal"   # 3
        coff += ch
    dwg, rows = R.backward_form(inp, cls, row_sink)
    want = R.backward(inp, ref.T, ref.bT, feat_k, argmax_k, cls, dwg, rows)                               # 4
    got = {"dtable": dtable}
    got.update({f"dW{k}": ws[k].grad for k in range(nw)})
    got.update({f"db{k}": bs[k].grad for k in range(nw)})
    if gate is not None:
        got["dgate"] = gate.grad
    assert set(got) == set(want)
    for name, (val, bound) in want.items():
        check(fam, name, got[name], val, bound)
    if cls in ("bf16x2", "bf16") and not case.all_masked:                                                 # 5
        near, outside = R.engaged(feat_k, ref, _f32_forward(case))
        assert near, f"{fam}: feat is no nearer to the {cls} reference than to the f32-class one"
        assert outside, f"{fam}: feat is inside the f32-class bound everywhere"
    if case.all_masked:
        act = torch.tanh if inp.tanh else torch.relu
        assert torch.equal(feat_k, act(torch.cat(inp.bs)).expand_as(feat_k))
        assert float(dtable.abs().max()) == 0.0 and all(float(w.grad.abs().max()) == 0.0 for w in ws)


@pytest.mark.parametrize("conv_class", R.F_RUNS, indirect=True, ids=lambda r: f"{r[0]}{'-t16' if r[1] else ''}")
@pytest.mark.parametrize("case", R.F_CASES, ids=lambda c: c.name)
def test_forward_classes_and_small_shape_backward(case, conv_class):
    """Forward GEMM instantiations (ring <3> / <1>, rows in registers <3,8> / <1,8>, bf16 storage: rows_to_b16 + b16s, b16sd), the
    bf16-table pool (odd bank widths, 16 / 32 / 64 lanes per position, the ends of a row) and the f32 backward of small shapes."""
    _run(case, *conv_class, row_sink=False)


@pytest.mark.parametrize("conv_class", R.B_RUNS, indirect=True, ids=lambda r: f"{r[0]}{'-t16' if r[1] else ''}")
@pytest.mark.parametrize("case", R.B_CASES, ids=lambda c: c.name)
def test_many_short_documents_backward(case, conv_class):
    """The row GEMM rows = G @ Wprod^T (<6> / <1> planes, rows in place, ncols = D) and dW from G (<3> / <1>, bias partials in the
    launch), and both sides of the n_docs >= 512, L <= 128, sum(kz * ch) <= 2048 rule on the same data."""
    _run(case, *conv_class, row_sink=True)
