"""The tap exchange kernels (taps_kernel, the key / bounds / weight / row kernels of the rebuild and its owner partition, all in
csrc/textcnn_prod.hip) through the C ABI, element by element against the float64 restatement tests/tap_ref.py, at the smallest
shapes that isolate their branches: both paddings, both activations, windows over either end, L < kz, odd bank widths, the
cold-row threshold 16 / 17 and the split threshold 4096 / 4097, a three-part split, all taps in one cell and taps in every cell,
padded G columns, the wave-quarter and the 64-lane borders of a row, D = 4 and D > 512, 1 / 2 / 8 sets, and vocabularies smaller
than or not divisible by the number of ranks.  tests/test_tap_ref_host.py checks on the CPU that the cases cover these, that the
kernels' f32 / fixed-point arithmetic stays inside the bounds and that a dropped tap, a shifted column, a missing 'same' offset,
a missing division by n_sets and a slot beyond the kernel do not.

No test here passes a token outside the table or an argmax outside the pool: those are outside the contract.

Largest err / bound observed on an MI355X (the RATIO lines), per family:
  taps tanh          0.4089   (valid-tanh)
  cold rows          0.1868   (wide)
  hot rows           0.3584   (thr-spread-2^-30: taps of ~1e-9, where the half unit of 2^-40 per tap is most of the bound; 0.0771
                               at most elsewhere)
  split rows         0.0008   (split: 4096, 4097 and 8193 taps over 64 cells)
  owner slabs        0.3163   (own-n3-V64; every slab is the replicated rebuild bit for bit)
  fixed-mode e2e     0.2181   (no-mask, both formulations of the forward)
A build with kTapsCold = 15 fails test_rebuild_matches_the_reference[thr-spread-2^-30] (a 16-tap row of tiny taps then goes through
the fixed point, and only there does that leave the f32 chain's bound) and the 16-taps case of
test_a_tap_beyond_the_fixed_point_range_tells_the_two_paths_apart (in value the two paths agree to rounding); one that leaves
the tap index out of the product column fails 35 tests here, and one whose owner partition keeps t % n_sets == 0 on every rank
fails the nine owner cases with n_sets > 1.
"""
import ctypes as C

import pytest
import torch

import tap_ref as R
from edge_refs import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RBR_ERR_BAD_ARG, RBR_ERR_UNSUPPORTED = -1, -2


def _lib():
    from review_based_recommender_amd import _lib as L
    return L


def _desc(s):
    return _lib().make_desc(s.n_docs, s.L, s.D, s.V, s.kz, s.ch, s.pad_mode, s.act, s.padding_idx)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Rebuild:
    """One case's device buffers: the conv weights, the workspace and the descriptor."""

    def __init__(self, case):
        L = _lib()
        self.case, self.s, self.n_sets = case, case.shape, case.n_sets
        self.d = _desc(case.shape)
        assert L.lib().rbr_textcnn_taps_count(C.byref(self.d)) * case.n_sets == case.tok.numel()
        self.ws_w = [w.to(DEV).contiguous() for w in case.Ws]
        self.W = L.ptr_array(self.ws_w, torch.float32, "w")
        n = L.lib().rbr_textcnn_dtable_from_taps_ws_bytes(C.byref(self.d), case.n_sets)
        assert n > 0
        self.ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        self.tok, self.val = case.tok.to(DEV), case.val.to(DEV)

    def run(self, tok=None, val=None):
        """The replicated rebuild into a NaN-filled [V, D]."""
        L = _lib()
        tok, val = self.tok if tok is None else tok, self.val if val is None else val
        out = torch.full((self.s.V, self.s.D), float("nan"), device=DEV)
        L.check(L.lib().rbr_textcnn_dtable_from_taps(C.byref(self.d), self.n_sets, tok.data_ptr(), val.data_ptr(), self.W,
                                                     self.ws.data_ptr(), out.data_ptr(), _stream()), "rebuild")
        torch.cuda.synchronize()
        return out

    def rows(self):
        return _lib().lib().rbr_textcnn_taps_owner_rows(C.byref(self.d), self.n_sets)

    def slab(self, rank, flag, tok=None, val=None):
        L = _lib()
        tok, val = self.tok if tok is None else tok, self.val if val is None else val
        out = torch.full((self.rows(), self.s.D), float("nan"), device=DEV)
        L.check(L.lib().rbr_textcnn_dtable_from_taps_owner(C.byref(self.d), self.n_sets, rank, tok.data_ptr(), val.data_ptr(), self.W,
                                                           self.ws.data_ptr(), out.data_ptr(), flag.data_ptr(), _stream()), "owner")
        torch.cuda.synchronize()
        return out


_REF = {}


def _ref(case):
    if case.name not in _REF:
        s = case.shape
        _REF[case.name] = R.rebuild(case.tok, case.val, case.Ws, s.kz, s.ch, s.V, s.D, case.n_sets)
    return _REF[case.name]


def _check_rows(name, got, ref, bound, cnt):
    """Every row against its bound, one RATIO line per path: cold (<= 16 taps, and the empty rows: exactly 0), hot, split."""
    got = got.cpu()
    for family, rows in (("cold-rows", cnt <= R.TAPS_COLD), ("hot-rows", (cnt > R.TAPS_COLD) & (cnt <= R.TAPS_SPLIT)),
                         ("split-rows", cnt > R.TAPS_SPLIT)):
        if bool(rows.any()):
            check(family, name, got[rows], ref[rows], bound[rows])
    assert bool((got[cnt == 0] == 0).all())


# ------------------------------------------------------------------------------------------------------ a. rbr_textcnn_bwd_taps
@pytest.mark.parametrize("case", R.taps_cases(), ids=lambda c: c.name)
def test_taps_match_the_reference(case):
    L = _lib()
    s = case.shape
    d = _desc(s)
    n = L.lib().rbr_textcnn_taps_count(C.byref(d))
    assert n == s.n_items
    ids = case.ids.to(DEV)
    mask = None if case.mask is None else case.mask.to(DEV).view(torch.uint8)
    feat, argmax, d_feat = case.feat.to(DEV), case.argmax.to(DEV), case.d_feat.to(DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((n,), float("nan"), device=DEV)
    L.check(L.lib().rbr_textcnn_bwd_taps(C.byref(d), ids.data_ptr(), None if mask is None else mask.data_ptr(), feat.data_ptr(),
                                         argmax.data_ptr(), d_feat.data_ptr(), tok.data_ptr(), val.data_ptr(), _stream()), "taps")
    torch.cuda.synchronize()
    ref = R.taps(s, case.ids, case.mask, case.feat, case.argmax, case.d_feat)
    R.check_taps("taps-tanh" if s.act == R.TANH else "taps-relu", case.name, tok, val, ref)


# ---------------------------------------------------------------------------------------------- b. rbr_textcnn_dtable_from_taps
@pytest.mark.parametrize("case", R.rebuild_cases(), ids=lambda c: c.name)
def test_rebuild_matches_the_reference(case):
    ref, bound, cnt = _ref(case)
    rb = _Rebuild(case)
    a, b = rb.run(), rb.run()
    assert torch.equal(a, b)                                   # the bits of a row do not depend on the order the atomics land in
    _check_rows(case.name, a, ref, bound, cnt)


# ----------------------------------------------------------------------------------------------------------- c. order freedom
@pytest.mark.parametrize("name", ["thr-spread", "split", "wide"])
def test_rebuild_does_not_depend_on_the_order_of_the_sets(name):
    """The sets in another order: the fixed-point rows (> 16 taps) are the same bits; a cold row is an f32 chain in array order,
    which moves inside its bound."""
    case = {c.name: c for c in R.rebuild_cases()}[name]
    ref, bound, cnt = _ref(case)
    rb = _Rebuild(case)
    base = rb.run()
    n = case.shape.n_items
    perm = torch.tensor([1, 0] if case.n_sets == 2 else [5, 2, 7, 0, 3, 6, 1, 4], device=DEV)
    got = rb.run(rb.tok.view(case.n_sets, n)[perm].reshape(-1).contiguous(), rb.val.view(case.n_sets, n)[perm].reshape(-1).contiguous())
    hot = (cnt > R.TAPS_COLD).to(DEV)
    assert bool(hot.any()) and bool((~hot & (cnt > 1).to(DEV)).any())
    assert torch.equal(got[hot], base[hot])
    _check_rows(name + "-permuted", got, ref, bound, cnt)


# --------------------------------------------------------------------------------------------------------- d. owner partition
@pytest.mark.parametrize("case", R.owner_cases(), ids=lambda c: c.name)
def test_owner_slabs_are_the_replicated_rebuild(case):
    ref, bound, cnt = _ref(case)
    rb = _Rebuild(case)
    V, n_sets = case.shape.V, case.n_sets
    whole = rb.run()
    check("owner-slabs", case.name + "-replicated", whole, ref, bound)
    v_own = rb.rows()
    assert v_own == (V + n_sets - 1) // n_sets
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    merged = torch.full((v_own * n_sets, case.shape.D), float("nan"), device=DEV)
    for r in range(n_sets):
        merged[r::n_sets] = rb.slab(r, flag)
    assert int(flag.item()) == 0
    assert torch.equal(merged[:V], whole)                      # bit for bit
    assert bool((merged[V:] == 0).all())                       # rows past the vocabulary
    check("owner-slabs", case.name, merged[:V], ref, bound)


# ---------------------------------------------------------------------------------------------------------- e. owner capacity
def test_owner_capacity_is_exact_and_the_flag_is_sticky():
    """Rank 0 owns exactly as many taps as the sort is sized for: a complete slab, flag 0.  One more: flag 1, and a clean call
    after it leaves the flag alone (the caller zeroes it)."""
    fits, over = R.cap_case(0), R.cap_case(1)
    ref, bound, _ = _ref(fits)
    rb = _Rebuild(fits)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    slab = rb.slab(0, flag)
    assert int(flag.item()) == 0
    check("owner-slabs", fits.name, slab, ref[0::3], bound[0::3])
    rb.slab(0, flag, over.tok.to(DEV), over.val.to(DEV))
    assert int(flag.item()) == 1
    again = rb.slab(0, flag)
    assert int(flag.item()) == 1
    assert torch.equal(again, slab)


# --------------------------------------------------------------------------------------------------------- f. non-finite taps
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("token", [6, 17, 11], ids=["cold", "hot", "split"])
def test_a_non_finite_tap_poisons_its_row_and_no_other(token, bad):
    case = {c.name: c for c in R.rebuild_cases()}["split"]
    assert case.counts[token] == {6: 16, 17: 100, 11: 8193}[token]
    rb = _Rebuild(case)
    clean = rb.run()
    val = rb.val.clone()
    val[int(torch.nonzero(case.tok == token)[case.counts[token] // 2])] = bad
    got = rb.run(val=val)
    assert not bool(torch.isfinite(got[token]).any())
    others = torch.arange(case.shape.V, device=DEV) != token
    assert torch.equal(got[others], clean[others])


@pytest.mark.parametrize("token, taps", [(3, 16), (4, 17)], ids=["16-taps", "17-taps"])
def test_a_tap_beyond_the_fixed_point_range_tells_the_two_paths_apart(token, taps):
    """rbr_hip.h's value domain at the threshold itself: a finite tap of 1e7 (> 8e6) is carried through by the f32 chain of a
    token with 16 taps -- its row stays inside the cold bound -- and makes the row of a token with 17 taps NaN.  No other row
    moves.  (In value the two paths agree to rounding; this is where they differ by contract.)"""
    case = {c.name: c for c in R.rebuild_cases()}["thr-spread"]
    assert case.counts[token] == taps
    s = case.shape
    rb = _Rebuild(case)
    clean = rb.run()
    val = case.val.clone()
    val[int(torch.nonzero(case.tok == token)[taps // 2])] = 1.0e7
    got = rb.run(val=val.to(DEV))
    others = torch.arange(s.V, device=DEV) != token
    assert torch.equal(got[others], clean[others])
    if taps <= R.TAPS_COLD:
        ref, bound, _ = R.rebuild(case.tok, val, case.Ws, s.kz, s.ch, s.V, s.D, case.n_sets)
        check("cold-rows", "thr-spread-1e7", got[token], ref[token], bound[token])
    else:
        assert bool(torch.isnan(got[token]).all())


# ---------------------------------------------------------------------------------------------------------------- g. refusals
def test_unsupported_shapes_and_bad_arguments_are_refused():
    L = _lib()
    lib = L.lib()
    s = R.Shape(2, 8, 6, 5, [3], [2])                          # D % 4 != 0
    d = _desc(s)
    assert lib.rbr_textcnn_dtable_from_taps_ws_bytes(C.byref(d), 1) == 0
    w = [torch.zeros(2, 6, 3, device=DEV)]
    W = L.ptr_array(w, torch.float32, "w")
    tok = torch.full((4 * s.n_items,), -1, dtype=torch.int32, device=DEV)
    val = torch.zeros(4 * s.n_items, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.full((s.V, s.D), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = _stream()
    assert lib.rbr_textcnn_dtable_from_taps(C.byref(d), 1, tok.data_ptr(), val.data_ptr(), W, ws.data_ptr(), out.data_ptr(),
                                            st) == RBR_ERR_UNSUPPORTED
    ok = _desc(R.Shape(2, 8, 8, 5, [3], [2]))
    w8 = [torch.zeros(2, 8, 3, device=DEV)]
    W8 = L.ptr_array(w8, torch.float32, "w")
    out8 = torch.full((5, 8), float("nan"), device=DEV)
    assert lib.rbr_textcnn_dtable_from_taps_ws_bytes(C.byref(ok), 0) == 0
    assert lib.rbr_textcnn_dtable_from_taps(C.byref(ok), 0, tok.data_ptr(), val.data_ptr(), W8, ws.data_ptr(), out8.data_ptr(), st) != 0
    assert lib.rbr_textcnn_taps_owner_rows(C.byref(ok), 0) == 0
    args = (tok.data_ptr(), val.data_ptr(), W8, ws.data_ptr(), out8.data_ptr())
    assert lib.rbr_textcnn_dtable_from_taps_owner(C.byref(ok), 2, 2, *args, flag.data_ptr(), st) == RBR_ERR_BAD_ARG      # rank >= n_sets
    assert lib.rbr_textcnn_dtable_from_taps_owner(C.byref(ok), 2, -1, *args, flag.data_ptr(), st) == RBR_ERR_BAD_ARG
    assert lib.rbr_textcnn_dtable_from_taps_owner(C.byref(ok), 2, 0, *args, None, st) == RBR_ERR_BAD_ARG                 # no flag
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out8).all()) and int(flag.item()) == 0                     # nothing ran


# ------------------------------------------------------------------------------------------------- h. end to end in fixed mode
@pytest.mark.parametrize("padding_idx", [0, None], ids=["pad0", "nopad"])
@pytest.mark.parametrize("shape", [
    dict(n_docs=1, L=1, D=8, V=5, kzs=[3], chans=[2], mask_p=0.2),
    dict(n_docs=5, L=33, D=16, V=40, kzs=[3, 7], chans=[33, 31], mask_p=0.2),
    dict(n_docs=3, L=48, D=24, V=50, kzs=[3, 5, 7], chans=[10, 10, 10], mask_p=1.1),          # every token masked
    dict(n_docs=3, L=48, D=24, V=50, kzs=[3, 5], chans=[6, 6], mask_p=None),                  # mask == NULL
], ids=["one-token", "two-slabs", "all-masked", "no-mask"])
def test_fixed_mode_table_gradient_end_to_end(shape, padding_idx, conv_mode, monkeypatch):
    """functional.textcnn under set_dtable_mode("fixed"): table.grad against rebuild(taps(the kernel's own feat and argmax)) at
    n_sets = 1, element by element; two runs the same bits; the padding row exactly 0."""
    from review_based_recommender_amd import functional as RF
    n_docs, L, D, V, kzs, chans = (shape[k] for k in ("n_docs", "L", "D", "V", "kzs", "chans"))
    g = torch.Generator().manual_seed(11)
    table = torch.randn(V, D, generator=g)
    ids = torch.randint(0, V, (n_docs, L), generator=g)
    if L > 1:
        ids[0, 0] = 0                                          # the padding token is present
    mask = (torch.rand(n_docs, L, generator=g) > shape["mask_p"]) if shape["mask_p"] is not None else None
    ws = [torch.randn(c, D, k, generator=g) * (D * k) ** -0.5 for k, c in zip(kzs, chans)]
    bs = [torch.randn(c, generator=g) * 0.1 for c in chans]
    d_out = torch.randn(n_docs, sum(chans), generator=g)
    calls = []
    fixed = RF._bwd_fixed
    monkeypatch.setattr(RF, "_bwd_fixed", lambda *a, **k: (calls.append(1), fixed(*a, **k))[1])
    RF.set_dtable_mode("fixed")
    try:
        grads = []
        for _ in range(2):
            t = table.to(DEV).requires_grad_(True)
            feat, argmax = RF.textcnn(t, ids.to(DEV), None if mask is None else mask.to(DEV), [w.to(DEV) for w in ws],
                                      [b.to(DEV) for b in bs], padding_idx=padding_idx, return_argmax=True)
            feat.backward(d_out.to(DEV))
            torch.cuda.synchronize()
            grads.append(t.grad.clone())
    finally:
        RF.set_dtable_mode(None)
    assert len(calls) == 2                                     # the fixed-point path is the one that ran
    assert torch.equal(grads[0], grads[1])
    s = R.Shape(n_docs, L, D, V, kzs, chans, R.PAD_SAME, R.RELU, -1 if padding_idx is None else padding_idx)
    tok, val, _ = R.taps(s, ids, mask, feat.detach(), argmax, d_out)
    ref, bound, cnt = R.rebuild(tok, val, ws, kzs, chans, V, D, 1)
    name = f"{n_docs}x{L}x{D}k{len(kzs)}-{conv_mode}-{'pad0' if padding_idx == 0 else 'nopad'}"
    check("fixed-e2e", name, grads[0], ref, bound)
    if padding_idx == 0:
        assert bool((grads[0][0] == 0).all()) and int(cnt[0]) == 0
    if shape["mask_p"] == 1.1:
        assert int(cnt.sum()) == 0 and bool((grads[0] == 0).all())
    elif L > 1:
        assert int(cnt.sum()) > 0
