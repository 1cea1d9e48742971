"""The rating head (csrc/pair_head.hip: rbr_pair_head_fwd, rbr_pair_head_fwd_train, rbr_pair_head_bwd) through the C ABI at the
edges of the kernels' own constants: the 4 thread groups and the 8-wide unrolled loop over H (`hh + 28 < H`: H = 28, 29, 32, 33,
61), the 32 lanes over K (K = 31, 32, 33, 64, 65) and the 256-thread loop of the backward's pair role (K = 260), the float4 path
of d_feat (K % 4 == 0 and Wu, Wi on 16 bytes), the 64 batch rows per round of the batch reductions (B = 63, 64, 65, 129), and
pad_u != pad_i.  U = 11, I = 13, ids repeated inside the batch.

Every result against the float64 restatement of tests/edge_refs.py from the same f32 inputs:

    ul = uf @ Wu + bu + Eu[uid] (n = H + 2), il likewise;  pred = (relu(ul * il) * drop) @ h + ub[uid] + ib[iid] + g (n = K + 3)

pred and the whole backward start from the ul, il (and dropout multiplier) the GPU saved, cast to float64.  Per-element bounds
(n + 4) * EPS * Abs, n = B for dWu dWi dbu dbi dh dg, K for d_ufeat d_ifeat, the id's multiplicity for dEu dEi dub dib.  The dense
outputs start as 7.0 (overwritten); the embedding-style outputs are added onto a random non-zero base, with EPS * (|base| + Abs)
for the add; rows of ids that do not occur and pad rows stay bit-equal to the base.

The base is small (N(0, 1) * 2^-30), for a reason that is a property of the kernel: head_bwd_kernel adds every pair's term onto
the buffer with an atomic of its own, so an id of multiplicity m costs m roundings of a value of magnitude |base| + partial sum,
where the allowance above pays for ONE rounding of |base|.  It is a valid a-priori bound as long as (m - 1) |base| <= 5 Abs,
which a base far below the terms guarantees.  With a base of the terms' magnitude (0.05 N(0, 1) under terms of ~0.05) the
same bound was missed on an MI355X where |base| >> Abs: largest err / bound dEu 1.58, dEi 1.42 (dub, dib 0.26) -- m roundings
of the base, not a wrong sum.  In the models the buffer is the one the forward launch has just cleared (base 0: the first add
is exact and the m - 1 others are the (n + 4) EPS Abs of any sum).
Every test prints its largest err / bound per tensor ("RATIO <family> <tensor> <value>")."""
import ctypes as C
import zlib

import pytest
import torch

import edge_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I64 = torch.float32, torch.int64
U, I = 11, 13
DENSE = ("dWu", "dbu", "dWi", "dbi", "dh", "dg")
ATOMIC = ("dEu", "dEi", "dub", "dib")

_H = (1, 3, 4, 5, 28, 29, 32, 33, 61)
_K = (1, 3, 4, 31, 32, 33, 64, 65, 260)
_B = (1, 7, 8, 9, 63, 64, 65, 129)
SHAPES = [(_B[i % 8], _H[i], _K[i]) for i in range(9)] + [(_B[(i + 3) % 8], _H[i], _K[(i + 5) % 9]) for i in range(9)] + \
         [(65, 33, 260), (129, 4, 64), (64, 61, 32)]


def test_shapes_cover_the_issue_s_values():
    """each H, K, B with at least two values of the other two; K = 260 with B = 65"""
    for pos, vals in ((1, _H), (2, _K), (0, _B)):
        for v in vals:
            rows = [s for s in SHAPES if s[pos] == v]
            for other in {0, 1, 2} - {pos}:
                assert len({s[other] for s in rows}) >= 2, (pos, v, other)
    assert (65, 33, 260) in SHAPES


def _inputs(case, B, H, K, pad_u, pad_i):
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    r = lambda *s: torch.randn(*s, generator=g)
    P = dict(Wu=r(H, K) * 0.1, bu=r(K) * 0.1, Eu=r(U, K) * 0.1, Wi=r(H, K) * 0.1, bi=r(K) * 0.1, Ei=r(I, K) * 0.1, h=r(K) * 0.3,
             g=r(1), ub=r(U) * 0.1, ib=r(I) * 0.1)
    uf, itf = r(B, H) * 0.3, r(B, H) * 0.3
    uid, iid = torch.randint(0, U, (B,), generator=g), torch.randint(0, I, (B,), generator=g)
    # ids equal to each side's pad and to the OTHER side's pad, as far as the batch has room
    for b, (ids, v, n) in enumerate(((uid, pad_u, U), (iid, pad_i, I), (uid, pad_i, U), (iid, pad_u, I))):
        if b < B and 0 <= v < n:
            ids[b] = v
    drop = (torch.rand(B, K, generator=g) > 0.5).float() * 2
    d_pred = r(B)
    base = {k: t * 2.0 ** -30 for k, t in (("dEu", r(U, K)), ("dEi", r(I, K)), ("dub", r(U)), ("dib", r(I)))}      # module docstring
    return P, uf, itf, uid, iid, drop, d_pred, base


class _Head:
    def __init__(self, B, H, K, P, uf, itf, uid, iid, misaligned=False):
        from review_based_recommender_amd import _lib
        self._lib, self.L_, self.B, self.H, self.K = _lib, _lib.lib(), B, H, K
        self.P = {k: t.to(DEV) for k, t in P.items()}
        if misaligned:                       # Wu 4 bytes past a 16-byte boundary: the float4 path of head_pair_dfeat is off
            buf = torch.empty(H * K + 1, device=DEV)
            assert buf.data_ptr() % 16 == 0
            self.P["Wu"] = buf[1:].view(H, K).copy_(self.P["Wu"])
            assert self.P["Wu"].data_ptr() % 16 == 4
        else:
            assert self.P["Wu"].data_ptr() % 16 == 0 and self.P["Wi"].data_ptr() % 16 == 0
        self.uf, self.itf, self.uid, self.iid = uf.to(DEV), itf.to(DEV), uid.to(DEV), iid.to(DEV)
        self.hp = _lib.HeadParams(*[self.P[k].data_ptr() for k in R.HEAD_PARAMS])
        self.st = torch.cuda.current_stream().cuda_stream

    def _common(self):
        p = self._lib.dev_ptr
        return (self.B, self.H, self.K, p(self.uf, F32, "uf"), p(self.itf, F32, "itf"), p(self.uid, I64, "uid"), p(self.iid, I64, "iid"),
                C.byref(self.hp))

    def _outs(self):
        return torch.full((self.B, self.K), 7.0, device=DEV), torch.full((self.B, self.K), 7.0, device=DEV), torch.full((self.B,), 7.0, device=DEV)

    def fwd(self, drop):
        p = self._lib.dev_ptr
        ul, il, pred = self._outs()
        rc = self.L_.rbr_pair_head_fwd(*self._common(), p(drop, F32, "drop"), p(ul, F32, "ul"), p(il, F32, "il"), p(pred, F32, "pred"), self.st)
        assert rc == 0, self.L_.rbr_last_error()
        torch.cuda.synchronize()
        return ul, il, pred

    def fwd_train(self, p_drop, seed, state, zero_buf=None, zero_n=0):
        p = self._lib.dev_ptr
        ul, il, pred = self._outs()
        drop_out = torch.full((self.B, self.K), 7.0, device=DEV)
        rc = self.L_.rbr_pair_head_fwd_train(*self._common(), p_drop, seed, None if state is None else state.data_ptr(),
                                             p(drop_out, F32, "drop_out"), p(zero_buf, F32, "zero_buf"), zero_n, p(ul, F32, "ul"),
                                             p(il, F32, "il"), p(pred, F32, "pred"), self.st)
        assert rc == 0, self.L_.rbr_last_error()
        torch.cuda.synchronize()
        return ul, il, pred, drop_out

    def bwd(self, drop, ul, il, d_pred, pad_u, pad_i, base, with_dfeat=True):
        p = self._lib.dev_ptr
        B, H, K = self.B, self.H, self.K
        shapes = {"dWu": (H, K), "dbu": (K,), "dWi": (H, K), "dbi": (K,), "dh": (K,), "dg": (1,)}
        out = {k: torch.full(s, 7.0, device=DEV) for k, s in shapes.items()}
        out.update({k: base[k].to(DEV) for k in ATOMIC})
        out["d_ufeat"], out["d_ifeat"] = torch.full((B, H), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
        hg = self._lib.HeadGrads(*[out[k].data_ptr() for k in ("dWu", "dbu", "dEu", "dWi", "dbi", "dEi", "dh", "dg", "dub", "dib")])
        rc = self.L_.rbr_pair_head_bwd(*self._common(), p(drop, F32, "drop"), p(ul, F32, "ul"), p(il, F32, "il"),
                                       p(d_pred.to(DEV), F32, "d_pred"), pad_u, pad_i, C.byref(hg),
                                       p(out["d_ufeat"], F32, "duf") if with_dfeat else None,
                                       p(out["d_ifeat"], F32, "dif") if with_dfeat else None, None, self.st)
        assert rc == 0, self.L_.rbr_last_error()
        torch.cuda.synchronize()
        return out


def _check_fwd(fam, hd, P, uf, itf, uid, iid, drop, outs):
    ul, il, pred = outs
    R.check(fam, "ul", ul, *R.head_latent(uf, uid, P["Wu"], P["bu"], P["Eu"]))
    R.check(fam, "il", il, *R.head_latent(itf, iid, P["Wi"], P["bi"], P["Ei"]))
    R.check(fam, "pred", pred, *R.head_pred(ul, il, uid, iid, P["h"], P["g"], P["ub"], P["ib"], drop))


def _check_bwd(fam, ref, got, base, with_dfeat=True):
    for k, (val, ab, n) in ref.items():
        if k in ATOMIC:
            R.check(fam, k, got[k], val, R.accumulated(R.bound_of(n, ab), ab, base[k]), base[k])
        elif k in DENSE or with_dfeat:
            R.check(fam, k, got[k], val, R.bound_of(n, ab))
        else:
            assert bool((got[k] == 7.0).all()), f"{fam} {k}: written although NULL was passed"


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_head_forward_and_backward_edges(idx):
    """rbr_pair_head_fwd without and with a multiplier, rbr_pair_head_fwd_train(p_drop = 0) bit-equal to the former, and
    rbr_pair_head_bwd from the saved ul / il / multiplier, pads (0, 3) on even cases and (5, 0) on odd ones: the pad rows stay
    bit-equal to the base, an id equal to the OTHER side's pad gets its gradient.  Two backward runs: the same bits in every
    output but the four atomic ones.
    Largest err / bound on an MI355X: ul 0.28, il 0.30, pred 0.14, dWu 0.41, dbu 0.25, dWi 0.42, dbi 0.26, dh 0.30, dg 0.04,
    d_ufeat 0.43, d_ifeat 0.47, dEu 0.32, dEi 0.29, dub 0.15, dib 0.14 (the four atomic ones move in the last digit between runs)."""
    B, H, K = SHAPES[idx]
    pad_u, pad_i = (0, 3) if idx % 2 == 0 else (5, 0)
    P, uf, itf, uid, iid, drop, d_pred, base = _inputs(("head", idx), B, H, K, pad_u, pad_i)
    if B >= 4:
        assert bool((uid == pad_u).any() and (iid == pad_i).any() and (uid == pad_i).any() and (iid == pad_u).any())
    hd = _Head(B, H, K, P, uf, itf, uid, iid)
    plain = hd.fwd(None)
    _check_fwd("head-fwd", hd, P, uf, itf, uid, iid, None, plain)
    train = hd.fwd_train(0.0, 0, None)
    assert all(torch.equal(a, b) for a, b in zip(plain, train[:3])), "fwd_train(p_drop = 0) differs from fwd"
    ul, il, pred = hd.fwd(drop.to(DEV))
    assert torch.equal(ul, plain[0]) and torch.equal(il, plain[1])
    _check_fwd("head-fwd-mul", hd, P, uf, itf, uid, iid, drop, (ul, il, pred))
    got = hd.bwd(drop.to(DEV), ul, il, d_pred, pad_u, pad_i, base)
    ref = R.head_bwd(uf, itf, uid, iid, P, ul, il, drop, d_pred, pad_u, pad_i)
    assert float(ref["dEu"][1][pad_u].abs().max()) == 0 and float(ref["dEi"][1][pad_i].abs().max()) == 0      # pad rows: no terms
    _check_bwd("head-bwd", ref, got, base)
    if B >= 4:                                # the other side's pad is an ordinary id
        assert float(got["dub"][pad_i]) != float(base["dub"][pad_i]) and float(got["dib"][pad_u]) != float(base["dib"][pad_u])
    again = hd.bwd(drop.to(DEV), ul, il, d_pred, pad_u, pad_i, base)
    for k in DENSE + ("d_ufeat", "d_ifeat"):
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"


@pytest.mark.parametrize("B,H,K", [(9, 5, 33), (65, 33, 260), (64, 29, 4)])
def test_head_backward_without_multiplier_pad_or_d_feat(B, H, K):
    """drop = NULL; pads that no id equals (-1 and 99: nn.Embedding without padding_idx -- every occurring id gets its gradient);
    then d_ufeat = d_ifeat = NULL: the same embedding gradients to their bounds, the dense ones bit-equal, d_feat not written.
    Largest err / bound on an MI355X: dWu 0.15, dWi 0.14, dEu 0.32, dEi 0.31, dub 0.05, dib 0.13, d_ufeat 0.28, d_ifeat 0.29."""
    P, uf, itf, uid, iid, _, d_pred, base = _inputs(("nopad", B, H, K), B, H, K, -1, 99)
    hd = _Head(B, H, K, P, uf, itf, uid, iid)
    ul, il, _ = hd.fwd(None)
    ref = R.head_bwd(uf, itf, uid, iid, P, ul, il, None, d_pred, -1, 99)
    full = hd.bwd(None, ul, il, d_pred, -1, 99, base)
    _check_bwd("head-bwd-nopad", ref, full, base)
    for k, ids in (("dEu", uid), ("dEi", iid), ("dub", uid), ("dib", iid)):
        for v in ids.unique().tolist():
            if float(ref[k][1][v].abs().max()) > 0:
                assert not torch.equal(full[k][v].cpu(), base[k][v]), (k, v)
    part = hd.bwd(None, ul, il, d_pred, -1, 99, base, with_dfeat=False)
    _check_bwd("head-bwd-nodfeat", ref, part, base, with_dfeat=False)
    for k in DENSE:
        assert torch.equal(part[k], full[k]), k


@pytest.mark.parametrize("B,H,K", [(9, 5, 4), (65, 33, 260), (8, 61, 32)])
def test_head_backward_with_misaligned_weights(B, H, K):
    """K % 4 == 0 with Wu a view 4 bytes past a 16-byte boundary: head_pair_dfeat takes the scalar loop; everything meets the
    bounds of the aligned run.
    Largest err / bound on an MI355X, aligned and misaligned alike: d_ufeat 0.22, d_ifeat 0.19, dWu 0.20, dEu 0.25, dEi 0.31."""
    P, uf, itf, uid, iid, drop, d_pred, base = _inputs(("misaligned", B, H, K), B, H, K, 0, 3)
    for mis in (False, True):
        hd = _Head(B, H, K, P, uf, itf, uid, iid, misaligned=mis)
        outs = hd.fwd(drop.to(DEV))
        fam = "head-misaligned" if mis else "head-aligned"
        _check_fwd(fam, hd, P, uf, itf, uid, iid, drop, outs)
        ref = R.head_bwd(uf, itf, uid, iid, P, outs[0], outs[1], drop, d_pred, 0, 3)
        _check_bwd(fam, ref, hd.bwd(drop.to(DEV), outs[0], outs[1], d_pred, 0, 3, base), base)


@pytest.mark.parametrize("zero_n", [1, 1023, 1025, 300000])
def test_head_train_forward_dropout_and_zero_buffer(zero_n):
    """rbr_pair_head_fwd_train(p_drop = 0.5): drop_out is what rbr_dropout_multiplier writes for the same seed and call number (two
    calls in a row: the call number advances once per launch), pred matches the float64 formula with that multiplier, and the
    spare workgroups clear zero_buf[0 : zero_n] (300000: more than the 256 spare workgroups' first pass) and nothing behind it.
    Largest err / bound on an MI355X: ul 0.07, il 0.06, pred 0.03."""
    from review_based_recommender_amd import _lib
    B, H, K = 65, 29, 33
    P, uf, itf, uid, iid, _, _, _ = _inputs(("train", zero_n), B, H, K, 0, 3)
    hd = _Head(B, H, K, P, uf, itf, uid, iid)
    seed = 1234 + zero_n
    state, state_ref = torch.zeros(2, dtype=I64, device=DEV), torch.zeros(2, dtype=I64, device=DEV)
    for call in range(2):
        buf = torch.full((zero_n + 1,), 5.0, device=DEV)
        ul, il, pred, drop_out = hd.fwd_train(0.5, seed, state, buf, zero_n)
        want = torch.full((B * K,), 7.0, device=DEV)
        rc = _lib.lib().rbr_dropout_multiplier(B * K, 0.5, seed, state_ref.data_ptr(), _lib.dev_ptr(want, F32, "want"), hd.st)
        assert rc == 0, _lib.lib().rbr_last_error()
        torch.cuda.synchronize()
        assert torch.equal(drop_out.view(-1), want), f"call {call}: the multiplier differs from rbr_dropout_multiplier's"
        assert set(drop_out.unique().tolist()) == {0.0, 2.0}
        assert state.tolist() == [call + 1, 0] and state_ref.tolist()[0] == call + 1
        assert float(buf[:zero_n].abs().max()) == 0.0 and float(buf[zero_n]) == 5.0
        _check_fwd("head-train", hd, P, uf, itf, uid, iid, drop_out.cpu(), (ul, il, pred))


@pytest.mark.parametrize("B,H,K,k_bad", [(9, 5, 4, 1), (65, 29, 33, 32), (64, 4, 65, 0)])
def test_head_relu_keeps_nan(B, H, K, k_bad):
    """One NaN in a row of Eu: pred is NaN for exactly the pairs of that user, as relu(ul * il) @ h gives in torch (torch.relu(NaN)
    is NaN); every other prediction is bit-equal to the clean run.  k_bad = 32: the second pass of the 32 lanes over K."""
    P, uf, itf, uid, iid, _, _, _ = _inputs(("nan", B, H, K), B, H, K, 0, 3)
    u_bad = int(uid[B // 2])
    clean = _Head(B, H, K, P, uf, itf, uid, iid).fwd(None)[2].cpu()
    P["Eu"][u_bad, k_bad] = float("nan")
    pred = _Head(B, H, K, P, uf, itf, uid, iid).fwd(None)[2].cpu()
    hit = uid == u_bad
    assert 1 <= int(hit.sum()) < B
    assert bool(torch.isnan(pred[hit]).all()), f"{int(torch.isnan(pred[hit]).sum())} of {int(hit.sum())} predictions of the NaN row's user are NaN"
    assert torch.equal(pred[~hit], clean[~hit])
