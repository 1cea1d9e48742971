"""The small HIP ops at edge shapes, each against a plain float64 (or bit-exact) CPU restatement of the same operation, through
functional.py or -- where it would refuse or sanitize the input -- the C ABI: HierPooling, MyConv1d's shift-add epilogue, the
standalone embedding, block_cat / pair_dot, the two-sided review attention (with a gradient through the attention weights) and
the in-batch dedup.  Every floating reference is float64 from the same f32 inputs; the tolerances are derived next to their use."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import max_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24         # unit roundoff of f32


def _leaf(t):
    return t.clone().requires_grad_(True)


def _cmp_grads(gpu_leaves, cpu_leaves, rtol=2e-4, atol=2e-6):
    for a, b in zip(gpu_leaves, cpu_leaves):
        scale = float(b.grad.norm()) + 1e-6
        assert max_err(a.grad.cpu().numpy(), b.grad.numpy()) <= atol + rtol * scale


# ------------------------------------------------------------------------------------------------------------ 1. HierPooling
HIER_SHAPES = [(1, 1, 1, 1), (2, 7, 5, 7), (3, 9, 4, 1), (4, 33, 64, 3), (2, 50, 256, 3), (3, 40, 257, 5), (2, 64, 300, 2),
               (5, 21, 520, 4), (1, 300, 8, 9)]          # (n_docs, L, D, k): k = L, k = 1, D across the kernel's 256-column pass
HIER_V = (6, 200)
MIN_GAP = 1e-6
# (shape, V index, projection, masks given): every shape x V x projection with masks, and each shape once without
HIER_CASES = [(s, v, p, True) for s in range(len(HIER_SHAPES)) for v in range(2) for p in (False, True)] + \
             [(s, 1, bool(s % 2), False) for s in range(len(HIER_SHAPES))]


def _hier_inputs(si, vi, use_mask):
    """table [V, D] (pad row 0 zero), ids [n_docs, L] (pad tokens behind a right-padded random length: the first document is
    full, the second empty; a single document is full for V = 6 and of random length, possibly 0, otherwise), mask or None."""
    n, L, D, k = HIER_SHAPES[si]
    V = HIER_V[vi]
    g = torch.Generator().manual_seed(1000 + 4 * si + 2 * vi + (0 if use_mask else 1))
    table = torch.randn(V, D, generator=g) * 0.5
    table[0] = 0.0
    lens = torch.randint(0, L + 1, (n,), generator=g)
    if n >= 2:
        lens[0], lens[1] = L, 0
    elif vi == 0:
        lens[0] = L
    else:
        lens[0] = int(torch.randint(0, L, (1,), generator=g))
    ids = torch.randint(0, V, (n, L), generator=g)
    mask = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    ids = ids * mask
    return table, ids, (mask if use_mask else None), k, g


def _smallest_positive_gap(table, ids, mask, k):
    """Smallest strictly positive gap between the two largest float64 window means of any (document, column); inf if none."""
    from oracle import ref_cpu as O
    m = torch.ones_like(ids, dtype=torch.bool) if mask is None else mask
    x = O.masked_tensor(F.embedding(ids, table.double()), m).transpose(1, 2)
    means = F.avg_pool1d(x, k, stride=1)                      # [n_docs, D, L - k + 1]
    if means.shape[-1] < 2:
        return float("inf")
    top = means.topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    pos = gap[gap > 0]
    return float(pos.min()) if pos.numel() else float("inf")


@pytest.mark.parametrize("si,vi,proj,use_mask", HIER_CASES)
def test_hier_pool_edges(si, vi, proj, use_mask):
    """functional.hier_pool vs O.ngram_feat_hier in float64: output, table gradient and (with the projection) proj_w / proj_b
    under a random upstream gradient.  The f32 kernel and the f64 reference must pick the same window: exact ties hold the same
    unmasked tokens (same gradient whichever is picked), so the precondition -- checked on the reference alone -- is that every
    strictly positive top-2 gap of the f64 window means is >= 1e-6; no element is left out of the comparison.  (Smallest gap
    over the 27 inputs below: 1.81e-5, shape (5, 21, 520, 4) with V = 200.  Which of several exactly tied windows is taken
    cannot show here for the same reason: `>=` for `>` in the kernel's comparison passes this test.)
    Tolerances: without projection the output is a k-term f32 sum and one division, 4 * k * 2^-24 * max|table|; with it the
    2e-5 of test_linear_and_head_random; gradients as _cmp_grads."""
    from oracle import ref_cpu as O
    from review_based_recommender_amd import functional as RF
    n, L, D, k = HIER_SHAPES[si]
    table, ids, mask, k, g = _hier_inputs(si, vi, use_mask)
    gap = _smallest_positive_gap(table, ids, mask, k)
    print(f"hier case {(si, vi, proj, use_mask)}: smallest positive top-2 gap {gap:.3e}")
    assert gap >= MIN_GAP, gap
    H = D
    params = []
    if proj:
        H = [4, 11, 70][si % 3]
        assert H != D
        params = [torch.randn(H, D, generator=g) / np.sqrt(D), torch.randn(H, generator=g) * 0.1]
    d = torch.randn(n, H, generator=g)
    cl = [_leaf(t.double()) for t in [table] + params]
    ref_mask = torch.ones_like(ids, dtype=torch.bool) if mask is None else mask
    ref = O.ngram_feat_hier(F.embedding(ids, cl[0], padding_idx=0), ref_mask, k, *cl[1:])
    (ref * d.double()).sum().backward()
    gl = [_leaf(t.to(DEV)) for t in [table] + params]
    out = RF.hier_pool(gl[0], ids.to(DEV), None if mask is None else mask.to(DEV), k, gl[1] if proj else None,
                       gl[2] if proj else None, padding_idx=0)
    (out * d.to(DEV)).sum().backward()
    tol = 2e-5 if proj else 4 * k * EPS * float(table.abs().max())
    err = max_err(out.detach().cpu().numpy(), ref.detach().numpy())
    print(f"  output err {err:.3e} (tol {tol:.3e})")
    assert out.shape == ref.shape and err <= tol
    _cmp_grads(gl, cl)


def test_hier_pool_propagates_nan():
    """A NaN table row under one unmasked token of document 0: ATen's max pooling propagates NaN (`val > max || isnan(val)`) and
    so does ReLU, so the reference is NaN in every column of document 0 and finite in document 1; the kernel must agree
    elementwise (it takes the first NaN window and keeps it), the finite entries to the tolerance of the un-projected output."""
    from oracle import ref_cpu as O
    from review_based_recommender_amd import functional as RF
    k = 3
    g = torch.Generator().manual_seed(77)
    table = torch.randn(6, 5, generator=g) * 0.5
    table[0] = 0.0
    table[4] = float("nan")
    ids = torch.tensor([[1, 2, 4, 3, 5, 1, 0], [2, 3, 1, 5, 2, 0, 0]])
    mask = torch.tensor([[1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 0, 0]], dtype=torch.bool)
    ref = O.ngram_feat_hier(F.embedding(ids, table.double(), padding_idx=0), mask, k)
    assert bool(torch.isnan(ref[0]).all()) and not bool(torch.isnan(ref[1]).any())
    out = RF.hier_pool(table.to(DEV), ids.to(DEV), mask.to(DEV), k, None, None, padding_idx=0).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref)), (out, ref)
    fin = ~torch.isnan(ref)
    tol = 4 * k * EPS * float(table[~torch.isnan(table)].abs().max())
    assert float((out.double()[fin] - ref[fin]).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------------- 2. conv_shift_add
SHIFT_CASES = [(1, 1, [1], [1]), (2, 2, [7], [3]), (3, 4, [9, 1], [2, 5]), (2, 37, [3, 5, 7], [3, 5, 2]), (1, 300, [3], [70]),
               (2, 5, [1, 3, 5, 7, 9, 3, 5, 7], [1, 2, 3, 1, 2, 3, 1, 2]), (5, 51, [5], [1])]        # (bz, L, kz, ch)


def _shift_add_ref(T, biases, bz, L, kz, ch):
    """out[b, off_w + c, l] = bias_w[c] + sum_j T[(b, l + j - pad_w), poff_w + j * ch_w + c], rows outside the document zero."""
    Tv = T.view(bz, L, -1)
    outs, poff = [], 0
    for k_, c_, b_ in zip(kz, ch, biases):
        pad = (k_ - 1) // 2
        P = F.pad(Tv[:, :, poff:poff + k_ * c_].reshape(bz, L, k_, c_), (0, 0, 0, 0, pad, pad))      # [bz, L + 2 pad, kz, ch]
        o = b_.view(1, 1, c_) + sum(P[:, j:j + L, j, :] for j in range(k_))
        outs.append(o.permute(0, 2, 1))
        poff += k_ * c_
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("case", range(len(SHIFT_CASES)))
def test_conv_shift_add_edges(case):
    """functional.conv_shift_add on a random T (the GEMM is not part of the test).  Forward: a (kz + 1)-term f32 sum,
    (kz_max + 1) * 2^-24 * (max|T| + max|bias|).  dT is a pure gather: torch.equal with the f32 reference gradient.  dbias: a
    fixed-order sum, 1e-6 * sum|d_out| per channel and the same bits on two runs."""
    from review_based_recommender_amd import functional as RF
    bz, L, kz, ch = SHIFT_CASES[case]
    g = torch.Generator().manual_seed(2000 + case)
    T = torch.randn(bz * L, sum(k_ * c_ for k_, c_ in zip(kz, ch)), generator=g)
    biases = [torch.randn(c_, generator=g) for c_ in ch]
    d = torch.randn(bz, sum(ch), L, generator=g)
    c64 = [_leaf(t.double()) for t in [T] + biases]
    ref = _shift_add_ref(c64[0], c64[1:], bz, L, kz, ch)
    (ref * d.double()).sum().backward()
    c32 = [_leaf(t) for t in [T] + biases]
    (_shift_add_ref(c32[0], c32[1:], bz, L, kz, ch) * d).sum().backward()
    runs = []
    for _ in range(2):
        gl = [_leaf(t.to(DEV)) for t in [T] + biases]
        out = RF.conv_shift_add(gl[0], bz, L, kz, ch, gl[1:])
        (out * d.to(DEV)).sum().backward()
        runs.append((out.detach().cpu(), [t.grad.cpu() for t in gl]))
    out, grads = runs[0]
    assert out.shape == ref.shape
    tol = (max(kz) + 1) * EPS * (float(T.abs().max()) + max(float(b.abs().max()) for b in biases))
    assert max_err(out.numpy(), ref.detach().numpy()) <= tol
    assert torch.equal(grads[0], c32[0].grad)
    off = 0
    for w, c_ in enumerate(ch):
        bound = 1e-6 * d[:, off:off + c_, :].double().abs().sum(dim=(0, 2))
        assert bool(((grads[1 + w].double() - c64[1 + w].grad).abs() <= bound).all())
        assert torch.equal(grads[1 + w], runs[1][1][1 + w])
        off += c_
    assert torch.equal(out, runs[1][0])


@pytest.mark.parametrize("kz,ch", [([4], [2]), ([11], [2]), ([3] * 9, [1] * 9)])
def test_conv_shift_add_refuses(kz, ch):
    """An even width, a width beyond 9 and more than 8 widths are refused before anything launches."""
    from review_based_recommender_amd import functional as RF
    bz, L = 2, 6
    T = torch.zeros(bz * L, sum(k_ * c_ for k_, c_ in zip(kz, ch)), device=DEV)
    biases = [torch.zeros(c_, device=DEV) for c_ in ch]
    with pytest.raises(RuntimeError):
        RF.conv_shift_add(T, bz, L, kz, ch, biases)


# ----------------------------------------------------------------------------------------- 3. embedding, block_cat, pair_dot
@pytest.mark.parametrize("padding_idx", [0, 3, None])
@pytest.mark.parametrize("V,D", [(1, 1), (5, 1), (7, 3), (40, 65), (9, 300)])
def test_embedding_edges(V, D, padding_idx):
    """functional.embedding: forward torch.equal with table[ids]; backward vs F.embedding in float64 within 1e-6 * (per-row sum of
    |contributions|) -- atomics give an order-free f32 sum.  padding_idx None goes down as -1: row 0 then gets its gradient."""
    from review_based_recommender_amd import functional as RF
    g = torch.Generator().manual_seed(3000 + 10 * V + D)
    table = torch.randn(V, D, generator=g)
    id_shapes = [(1,), (3,), (2, 5), (257,)] + ([(2000,)] if V == 5 else [])        # 2000 tokens over 5 rows: heavy duplicates
    ref_pad = padding_idx if padding_idx is not None and padding_idx < V else None      # a pad row outside the table never matches
    for shape in id_shapes:
        ids = torch.randint(0, V, shape, generator=g)
        ids.view(-1)[0] = 0
        d = torch.randn(*shape, D, generator=g)
        ct = _leaf(table.double())
        (F.embedding(ids, ct, padding_idx=ref_pad) * d.double()).sum().backward()
        contrib = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.view(-1), d.double().abs().view(-1, D))
        gt = _leaf(table.to(DEV))
        out = RF.embedding(gt, ids.to(DEV), padding_idx)
        (out * d.to(DEV)).sum().backward()
        assert torch.equal(out.detach().cpu(), table[ids])
        assert bool(((gt.grad.cpu().double() - ct.grad).abs() <= 1e-6 * contrib).all()), shape
        if ref_pad is not None:
            assert float(gt.grad[ref_pad].abs().sum()) == 0.0
        if ref_pad != 0:
            assert float(gt.grad[0].abs().sum()) > 0.0 and float(ct.grad[0].abs().sum()) > 0.0


@pytest.mark.parametrize("contiguous", [True, False])
@pytest.mark.parametrize("B,C1,C2", [(1, 1, 1), (3, 5, 2), (17, 1, 300), (64, 24, 12)])
def test_block_cat_edges(B, C1, C2, contiguous):
    """functional.block_cat is torch.equal with the two nested torch.cat, its four gradient pieces with slices of the upstream
    gradient; also from transposed (non-contiguous) views."""
    from review_based_recommender_amd import functional as RF
    g = torch.Generator().manual_seed(4000 + B)
    shapes = [(B, C1), (B, C2), (B, C1), (B, C2)]
    if contiguous:
        parts = [torch.randn(*s, generator=g) for s in shapes]
    else:
        parts = [torch.randn(s[1], s[0], generator=g).t() for s in shapes]
        assert all(p.is_contiguous() == (p.shape[0] == 1 or p.shape[1] == 1) for p in parts)
    up = torch.randn(2 * B, C1 + C2, generator=g)
    gl = [_leaf(p.to(DEV)) for p in parts]
    assert all(a.is_contiguous() == p.is_contiguous() for a, p in zip(gl, parts))
    out = RF.block_cat(*gl)
    (out * up.to(DEV)).sum().backward()
    a, b, c, d = parts
    assert torch.equal(out.detach().cpu(), torch.cat((torch.cat((a, b), 1), torch.cat((c, d), 1)), 0))
    want = [up[:B, :C1], up[:B, C1:], up[B:, :C1], up[B:, C1:]]
    for t, w in zip(gl, want):
        assert torch.equal(t.grad.cpu(), w)


@pytest.mark.parametrize("B,K", [(1, 1), (1, 17), (15, 16), (16, 5), (17, 33), (33, 300)])
def test_pair_dot_edges(B, K):
    """functional.pair_dot on a stacked [2B, K] block.  Forward vs float64: a K-term fma chain over 16 lanes and a shuffle tree,
    2 * K * 2^-24 * max_b sum_k |u * i|.  Backward is one multiply: torch.equal with d_out[:, None] * other in f32."""
    from review_based_recommender_amd import functional as RF
    g = torch.Generator().manual_seed(5000 + 100 * B + K)
    x = torch.randn(2 * B, K, generator=g)
    d = torch.randn(B, generator=g)
    prod = x[:B].double() * x[B:].double()
    gx = _leaf(x.to(DEV))
    out = RF.pair_dot(gx)
    (out * d.to(DEV)).sum().backward()
    assert out.shape == (B,)
    assert max_err(out.detach().cpu().numpy(), prod.sum(1).numpy()) <= 2 * K * EPS * float(prod.abs().sum(1).max())
    assert torch.equal(gx.grad.cpu(), torch.cat((d[:, None] * x[B:], d[:, None] * x[:B]), 0))


def test_pair_dot_refuses_odd_row_count():
    from review_based_recommender_amd import functional as RF
    with pytest.raises(RuntimeError):
        RF.pair_dot(torch.zeros(5, 4, device=DEV))


# ------------------------------------------------------------------------------------------------------ 4. review attention
ATTN2_CASES = [(1, 1, 5, 3, 4, 9, 0, 0), (4, 7, 24, 8, 17, 5, 0, 2), (33, 12, 150, 32, 11, 40, 3, 0), (9, 5, 12, 8, 6, 6, 0, 0)]


def _attn_params(H, A, n, g):
    return [torch.randn(H, A, generator=g) * 0.1, torch.randn(A, A, generator=g) * 0.1, torch.randn(A, 1, generator=g) * 0.1,
            torch.randn(A, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1, torch.randn(n, A, generator=g) * 0.1]


def _attn_ref(feat, oid, ps, pad, drop, d, e):
    """One side in float64 through O.linear_attention, whose id table has padding_idx 0 built in: rows 0 and `pad` of the table
    and of the ids change places on the way in, and the table gradient's rows on the way out.  Returns (out, att, leaves)."""
    from oracle import ref_cpu as O
    n = ps[5].shape[0]
    perm = torch.arange(n)
    perm[0], perm[pad] = pad, 0
    cl = [_leaf(feat.double())] + [_leaf(p.double()) for p in ps[:5]] + [_leaf(ps[5].double()[perm])]
    ro, ra = O.linear_attention(cl[0], perm[oid], *cl[1:])
    if drop is not None:
        ro = ro * drop.double()
    ((ro * d.double()).sum() + (ra * e.double()).sum()).backward()
    cl[6].grad = cl[6].grad[perm]
    return ro.detach(), ra.detach(), cl


@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("case", range(len(ATTN2_CASES)))
def test_review_attention2_edges(case, with_drop):
    """functional.review_attention2 vs O.linear_attention in float64 per side: id tables of different sizes, a pad row per side,
    B * R across the 16-row reduction chunks, and the loss (out * d).sum() + (att * e).sum(), so that d_att is not None.
    Tolerances of test_review_attention_random.  The sides equal two single-sided calls bit for bit; each table's own pad row
    gets exactly zero gradient, the other side's pad row does not."""
    from review_based_recommender_amd import functional as RF
    B, R, H, A, n0, n1, pad0, pad1 = ATTN2_CASES[case]
    ns, pads = (n0, n1), (pad0, pad1)
    g = torch.Generator().manual_seed(6000 + case)
    feat = torch.randn(2, B, R, H, generator=g) * 0.5
    oid = torch.stack([torch.randint(0, n, (B, R), generator=g) for n in ns])
    if B * R >= 2:
        for s in range(2):
            oid[s].view(-1)[0], oid[s].view(-1)[1] = pads[s], pads[1 - s]
    ps = [_attn_params(H, A, n, g) for n in ns]
    drop = ((torch.rand(2, B, H, generator=g) > 0.3).float() / 0.7) if with_drop else None
    d, e = torch.randn(2, B, H, generator=g), torch.randn(2, B, R, 1, generator=g)
    refs = [_attn_ref(feat[s], oid[s], ps[s], pads[s], None if drop is None else drop[s], d[s], e[s]) for s in range(2)]
    gf = _leaf(feat.to(DEV))
    gp = [[_leaf(t.to(DEV)) for t in ps[s]] for s in range(2)]
    dd = None if drop is None else drop.to(DEV)
    go, ga = RF.review_attention2(gf, oid.to(DEV), gp[0], gp[1], pad_idx=pads, drop=dd)
    ((go * d.to(DEV)).sum() + (ga * e.to(DEV)).sum()).backward()
    assert go.shape == (2, B, H) and ga.shape == (2, B, R, 1)
    for s in range(2):
        ro, ra, cl = refs[s]
        assert max_err(go[s].detach().cpu().numpy(), ro.numpy()) <= 1e-5
        assert max_err(ga[s].detach().cpu().numpy(), ra.numpy()) <= 1e-6
        _cmp_grads(gp[s], cl[1:], atol=1e-5)
        assert max_err(gf.grad[s].cpu().numpy(), cl[0].grad.numpy()) <= 1e-5 + 2e-4 * (float(cl[0].grad.norm()) + 1e-6)
        with torch.no_grad():
            so, sa = RF.review_attention(gf[s], oid[s].to(DEV), *gp[s], pad_idx=pads[s], drop=None if dd is None else dd[s])
        assert torch.equal(so, go[s].detach()) and torch.equal(sa, ga[s].detach())
        debd = gp[s][5].grad
        assert float(debd[pads[s]].abs().sum()) == 0.0
        other = pads[1 - s]
        if other != pads[s] and other < ns[s]:
            assert float(cl[6].grad[other].abs().sum()) > 0.0 and float(debd[other].abs().sum()) > 0.0


@pytest.mark.parametrize("with_drop", [False, True])
def test_review_attention_att_gradient(with_drop):
    """Single-sided functional.review_attention with a gradient through the attention weights (d_att not None)."""
    from review_based_recommender_amd import functional as RF
    B, R, H, A, n, pad = 4, 7, 24, 8, 17, 0
    g = torch.Generator().manual_seed(6100)
    feat = torch.randn(B, R, H, generator=g) * 0.5
    oid = torch.randint(0, n, (B, R), generator=g)
    oid.view(-1)[0] = pad
    ps = _attn_params(H, A, n, g)
    drop = ((torch.rand(B, H, generator=g) > 0.3).float() / 0.7) if with_drop else None
    d, e = torch.randn(B, H, generator=g), torch.randn(B, R, 1, generator=g)
    ro, ra, cl = _attn_ref(feat, oid, ps, pad, drop, d, e)
    gl = [_leaf(t.to(DEV)) for t in [feat] + ps]
    go, ga = RF.review_attention(gl[0], oid.to(DEV), *gl[1:], pad_idx=pad, drop=None if drop is None else drop.to(DEV))
    ((go * d.to(DEV)).sum() + (ga * e.to(DEV)).sum()).backward()
    assert max_err(go.detach().cpu().numpy(), ro.numpy()) <= 1e-5
    assert max_err(ga.detach().cpu().numpy(), ra.numpy()) <= 1e-6
    _cmp_grads(gl, cl, atol=1e-5)
    assert float(gl[6].grad[pad].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ 5. dedup
def _dedup_ref(u_ids, i_ids, U, I, mask_in, L):
    """dense_misc.hip's comment restated: an id inside [0, U) / [0, I) takes the smallest row of its side with that id as its
    first row, any other id is its own first; item rows are offset by B; a row that is not its own first gets a zero mask."""
    B = len(u_ids)
    first = np.zeros(2 * B, dtype=np.int64)
    for side, (ids, n) in enumerate(((u_ids, U), (i_ids, I))):
        seen = {}
        for b, v in enumerate(ids.tolist()):
            f = seen.setdefault(v, b) if 0 <= v < n else b
            first[side * B + b] = side * B + f
    mask = np.ones((2 * B, L), dtype=np.uint8) if mask_in is None else mask_in.copy()
    mask[first != np.arange(2 * B)] = 0
    return first, mask


def _dedup_case(name):
    rng = np.random.default_rng(7000)
    if name == "ids_outside":          # -1, U and I placed among valid ids: each is its own first, also when repeated
        B, L, U, I = 9, 4, 5, 4
        u, i = rng.integers(0, U, B), rng.integers(0, I, B)
        u[[2, 7]], u[5] = -1, U
        i[[1, 4]], i[3], i[8] = I, -1, I + 7
    elif name == "all_equal":          # every user id equal
        B, L, U, I = 40, 7, 3, 50
        u, i = np.full(B, 2), rng.integers(0, I, B)
    else:
        B, L, U, I = name
        u, i = rng.integers(0, U, B), rng.integers(0, I, B)
    return B, L, U, I, u.astype(np.int64), i.astype(np.int64)


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("name", [(1, 1, 1, 1), (5, 3, 2, 2), (64, 300, 7, 9), (257, 5, 300, 3), "ids_outside", "all_equal"],
                         ids=lambda n: n if isinstance(n, str) else "x".join(map(str, n)))
def test_dedup_rows_edges(name, with_mask):
    """rbr_dedup_rows through the C ABI (ids outside their table, mask_in NULL): first and mask_out exactly as restated."""
    from review_based_recommender_amd import _lib
    L_ = _lib.lib()
    B, L, U, I, u, i = _dedup_case(name)
    mask_in = (np.random.default_rng(B + L).random((2 * B, L)) > 0.4).astype(np.uint8) if with_mask else None
    ref_first, ref_mask = _dedup_ref(u, i, U, I, mask_in, L)
    ud, idd = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    md = torch.from_numpy(mask_in).to(DEV) if with_mask else None
    ws = torch.empty(L_.rbr_dedup_ws_bytes(U, I), dtype=torch.uint8, device=DEV)
    assert ws.numel() == 4 * (U + I)
    first = torch.full((2 * B,), -7, dtype=torch.int64, device=DEV)
    out = torch.full((2 * B, L), 9, dtype=torch.uint8, device=DEV)
    rc = L_.rbr_dedup_rows(B, L, ud.data_ptr(), idd.data_ptr(), U, I, None if md is None else md.data_ptr(), ws.data_ptr(),
                           first.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L_.rbr_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), ref_first)
    assert np.array_equal(out.cpu().numpy(), ref_mask)


@pytest.mark.parametrize("H", [1, 64, 65, 300])
def test_dedup_fold_rows_edges(H):
    """rbr_dedup_fold_rows: 40 rows fold onto one first row (f32 atomics: within 1e-6 * sum|rows| of the float64 sum), smaller
    groups beside it; the repeated rows end up exactly zero, rows without repeats keep their bits."""
    from review_based_recommender_amd import _lib
    L_ = _lib.lib()
    B = 45
    rng = np.random.default_rng(7100 + H)
    u = np.concatenate([np.full(41, 3), 100 + np.arange(4)])            # 41 rows of one id, 4 ids seen once
    rng.shuffle(u)
    i = np.concatenate([rng.integers(0, 6, 30), 200 + np.arange(15)])   # small groups over 6 ids, 15 ids seen once
    first, _ = _dedup_ref(u, i, 1000, 1000, None, 1)
    counts = np.bincount(first, minlength=2 * B)
    assert counts.max() == 41 and (counts == 1).sum() >= 19
    rows = torch.randn(2 * B, H, generator=torch.Generator().manual_seed(H))
    want = torch.zeros(2 * B, H, dtype=torch.float64).index_add_(0, torch.from_numpy(first), rows.double())
    bound = 1e-6 * torch.zeros(2 * B, H, dtype=torch.float64).index_add_(0, torch.from_numpy(first), rows.double().abs())
    rd, fd = rows.to(DEV), torch.from_numpy(first).to(DEV)
    rc = L_.rbr_dedup_fold_rows(2 * B, H, fd.data_ptr(), rd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L_.rbr_last_error()
    got = rd.cpu()
    own = first == np.arange(2 * B)
    assert float(got[~own].abs().max()) == 0.0
    assert bool(((got.double() - want).abs() <= bound).all())
    alone = own & (counts == 1)
    assert torch.equal(got[alone], rows[alone])
