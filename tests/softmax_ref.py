"""Float64 restatement, with per-element error bounds, of the in-batch softmax loss over all B x B pairs (rbr_pair_softmax_* of
include/rbr_hip.h), shared by tests/test_pair_softmax_host.py (which checks every formula here against torch autograd in float64)
and the GPU tests of the kernels.  Inputs are f32 (or float64) CPU tensors; everything is computed in float64.

Definition (the header's):

    core(a,b)    = FM : sum_k relu(ul[a,k] * il[b,k]) * drop[a,b,k] * h[k]      DOT: sum_k ul[a,k] * il[b,k]
    s[a,b]       = core(a,b) + row_bias[a] + col_bias[b]
    z[a,b]       = inv_temp * s[a,b] - logq[b]
    allowed[a,b] = (b == a) or (i_id[b] >= item_lo and i_id[b] != i_id[a] and i_id[b] not in seen(u_id[a]))
    lse[a]       = log sum over allowed b of exp(z[a,b])
    loss         = (1/B) sum_a (lse[a] - z[a,a]);   pos[a] = s[a,a]
    P[a,b]       = allowed ? exp(z[a,b] - lse[a]) : 0;   ds[a,b] = inv_temp * (P[a,b] - [a == b]) / B * d_loss
    d_ul[a,k] = sum_b ds[a,b] w(a,b,k) il[b,k],  d_il[b,k] = sum_a ds[a,b] w(a,b,k) ul[a,k],   w = [ul il > 0] drop h[k]  (DOT: 1)
    d_h[k]    = sum_ab ds[a,b] relu(ul[a,k] il[b,k]) drop[a,b,k],   d_col_bias[b] = sum_a ds[a,b],   d_row_bias = 0 (defined)

Bounds, in the style of tests/edge_refs.py: a sum of n terms computed in f32 in ANY order differs from the exact sum by at most

    bound = (n + 4) * EPS * Abs,     EPS = 2^-24, Abs = the sum of the magnitudes of the terms

(n - 1 additions; the 4 covers the roundings inside one term).  Derivation of what lies behind the sums:

  s: n = K + 2 terms (the K products and the two biases).
  z = inv_temp * s - logq: bound(z) = inv_temp * bound(s) + 2 EPS |inv_temp s| + EPS |z|  (inv_temp itself is a rounded f32, the
     product is rounded, the difference is rounded).
  softmax of a row: P is invariant under the shift m that the kernel subtracts, so an error of m costs nothing; what counts is
     t = z - m as the f32 code forms it: |t - (z_exact - m)| <= bound(z) + EPS |t|.  exp turns that absolute error into a
     relative one, and expf adds 4 EPS (the allowance edge_refs.py gives tanhf):
         r[a,b] = bound(z[a,b]) + EPS (|z[a,b] - m[a]| + 2 bzmax[a]) + 4 EPS                  bzmax[a] = max_b bound(z[a,b])
     (the 2 bzmax: the f32 m may differ from the float64 one by bzmax, and so may t).  The sum S of the n_a allowed, positive
     terms has the relative error rS[a] = max_b r[a,b] + (n_a + 4) EPS; P = e / S adds one rounding.  With (1 + x) <= exp(x) for
     the numerator and 1 / (1 - rS) = exp(lS), lS = -log(1 - rS), for the denominator (no first-order shortcut):
         |dP[a,b]| <= P[a,b] * expm1(r[a,b] + lS[a] + EPS) + TINY
     which to first order is the form P * (2 max_b bound(z[a,.]) + c EPS) with every expf / logf call counted at 4 EPS; TINY =
     2^-126 covers an f32 underflow of P itself.
  lse - z[a,a]: log S inherits lS as an absolute error, logf adds 4 EPS (|log S| + 1), the sum m + log S and the difference
     to z[a,a] a rounding each, z[a,a] its own bound.  The loss is a sum of B such terms, then one multiplication.
  ds = (P - [a == b]) * scale: |d ds| <= |dP| |scale| + 4 EPS |ds| (+ TINY): difference, product, and the two roundings of scale.
  the gradients: sums of n = B terms (d_h: n = B * B) of ds times an exactly representable-to-2-roundings factor:
         bound = sum |d ds| |factor| + (n + 4) EPS sum |ds factor|   (+ n TINY where there is any term)

A masked pair has P exactly 0, hence bound 0: the tests then demand exact zeros.  A row whose only allowed column is its own has
S = exp(0) = 1, lse = z[a,a]: loss term, P - 1 and every gradient term exactly 0, and bound 0 as well.
"""
import numpy as np
import torch

from edge_refs import EPS, bound_of, f64

TINY = 2.0 ** -126


def allowed_mask(u_ids, i_ids, seen, item_lo):
    """bool [B, B].  seen: None or (off int64 [U + 1], items int32 sorted within a row); offsets clamped to [0, nnz] as the kernel
    clamps them, a u_id outside [0, U) has an empty row."""
    u_ids, i_ids = [int(x) for x in u_ids], [int(x) for x in i_ids]
    B = len(u_ids)
    off = items = None
    if seen is not None:
        off, items = [int(x) for x in seen[0]], [int(x) for x in seen[1]]
    nnz = 0 if items is None else len(items)
    out = torch.zeros(B, B, dtype=torch.bool)
    for a in range(B):
        row = set()
        if off is not None and 0 <= u_ids[a] < len(off) - 1:
            lo, hi = max(off[u_ids[a]], 0), min(off[u_ids[a] + 1], nnz)
            row = set(items[lo:max(hi, lo)])
        for b in range(B):
            out[a, b] = b == a or (i_ids[b] >= item_lo and i_ids[b] != i_ids[a] and i_ids[b] not in row)
    return out


def loss_f64(ul, il, h, row_bias, col_bias, drop, logq, allowed, inv_temp, fm):
    """The definition in differentiable float64 torch ops -> (loss, s [B, B]): what autograd differentiates in the host test."""
    if fm:
        t = torch.relu(ul[:, None, :] * il[None, :, :])
        if drop is not None:
            t = t * drop
        s = (t * h.reshape(-1)).sum(-1)
    else:
        s = ul @ il.t()
    if row_bias is not None:
        s = s + row_bias.reshape(-1)[:, None]
    if col_bias is not None:
        s = s + col_bias.reshape(-1)[None, :]
    z = inv_temp * s
    if logq is not None:
        z = z - logq.reshape(-1)[None, :]
    lse = torch.logsumexp(torch.where(allowed, z, torch.full_like(z, -float("inf"))), dim=1)
    return (lse - z.diagonal()).mean(), s


def pair_softmax_ref(ul, il, u_ids, i_ids, fm, h=None, row_bias=None, col_bias=None, drop=None, seen=None, item_lo=1, logq=None,
                     inv_temp=1.0, d_loss=1.0):
    """{name: (value, bound)} for loss, pos, d_ul, d_il, d_h (fm), d_col_bias (with col_bias), plus "P" and "allowed" (no bound)."""
    ul, il, h, rb, cb, drop, lq = (f64(t) for t in (ul, il, h, row_bias, col_bias, drop, logq))
    B, K = ul.shape
    allowed = allowed_mask(u_ids, i_ids, seen, item_lo)
    prod = ul[:, None, :] * il[None, :, :]                         # [B, B, K]
    if fm:
        hv = h.reshape(-1)
        mult = torch.ones_like(prod) if drop is None else drop
        gate = (prod > 0).double()
        act = prod * gate * mult                                   # relu(ul il) drop
        core, core_abs = (act * hv).sum(-1), (act * hv).abs().sum(-1)
        w = gate * mult * hv                                       # d core / d (ul il)
    else:
        core, core_abs = prod.sum(-1), prod.abs().sum(-1)
        w = torch.ones_like(prod)
    s, s_abs = core.clone(), core_abs.clone()
    if rb is not None:
        s, s_abs = s + rb.reshape(-1)[:, None], s_abs + rb.reshape(-1).abs()[:, None]
    if cb is not None:
        s, s_abs = s + cb.reshape(-1)[None, :], s_abs + cb.reshape(-1).abs()[None, :]
    bs = bound_of(K + 2, s_abs)
    z = inv_temp * s
    if lq is not None:
        z = z - lq.reshape(-1)[None, :]
    bz = inv_temp * bs + 2 * EPS * (inv_temp * s).abs() + EPS * z.abs()

    neg_inf = torch.full_like(z, -float("inf"))
    zm = torch.where(allowed, z, neg_inf)
    m = zm.max(dim=1, keepdim=True).values
    e = torch.where(allowed, torch.exp(z - m), torch.zeros_like(z))
    S = e.sum(1, keepdim=True)
    P = e / S
    n_a = allowed.sum(1, keepdim=True).double()
    alone = n_a == 1                                               # rows whose only allowed column is their own: everything exact
    bz_al = torch.where(allowed, bz, torch.zeros_like(bz))
    bzmax = bz_al.max(dim=1, keepdim=True).values
    r = torch.where(allowed, bz + EPS * ((z - m).abs() + 2 * bzmax) + 4 * EPS, torch.zeros_like(z))
    rS = r.max(dim=1, keepdim=True).values + (n_a + 4) * EPS
    assert float(rS.max()) < 0.5, "the inputs leave the row sums no relative accuracy at all"
    lS = -torch.log1p(-rS)
    relP = r + lS + EPS
    dP = torch.where(allowed & ~alone, P * torch.expm1(relP) + TINY, torch.zeros_like(P))

    logS = torch.log(S)
    lse = m + logS
    L = (lse - z.diagonal()[:, None]).squeeze(1)
    bL = (lS + 4 * EPS * (logS.abs() + 1) + EPS * lse.abs()).squeeze(1) + bz.diagonal() + EPS * L.abs()
    L = torch.where(alone.squeeze(1), torch.zeros_like(L), L)
    bL = torch.where(alone.squeeze(1), torch.zeros_like(bL), bL)
    loss = L.sum() / B
    b_loss = (bL.sum() + bound_of(B, L.abs().sum())) / B + EPS * loss.abs()

    scale = inv_temp / B * d_loss
    ds = (P - torch.eye(B, dtype=torch.float64)) * scale
    ds = torch.where(alone, torch.zeros_like(ds), ds)
    bds = torch.where(allowed & ~alone, dP * abs(scale) + 4 * EPS * ds.abs() + TINY, torch.zeros_like(ds))

    def grad(terms, dterms, dims, n):
        """sum over `dims` of ds * factor: terms = ds * factor, dterms = bound(ds) * |factor|."""
        val, ab = terms.sum(dims), terms.abs().sum(dims)
        return val, torch.where(ab > 0, dterms.sum(dims) + bound_of(n, ab) + n * TINY, torch.zeros_like(ab))

    out = {"loss": (loss, b_loss), "pos": (s.diagonal().clone(), bs.diagonal().clone()), "P": (P, dP), "allowed": (allowed, None)}
    f_ul = w * il[None, :, :]
    f_il = w * ul[:, None, :]
    out["d_ul"] = grad(ds[:, :, None] * f_ul, bds[:, :, None] * f_ul.abs(), 1, B)
    out["d_il"] = grad(ds[:, :, None] * f_il, bds[:, :, None] * f_il.abs(), 0, B)
    if fm:
        out["d_h"] = grad(ds[:, :, None] * act, bds[:, :, None] * act.abs(), (0, 1), B * B)
    if cb is not None:
        out["d_col_bias"] = grad(ds, bds, 0, B)
    out["row_sums"] = (ds.sum(1), None)       # d_row_bias as a sum: 0 in exact arithmetic
    return out


def mask_fixture():
    """B = 8 pairs whose rows show every way a column leaves the softmax; item_lo = 1, a seen CSR of U = 5 users.

      row  u  i   what it shows
      0    0  3   every negative masked: seen(0) lists every other item of the batch (and the pad column is below item_lo)
      1    1  4   masked by the seen CSR (item 7, column 6) and by its user's other row (item 5, column 2)
      2    1  5   the second row of user 1
      3    2  4   masked by a duplicate item: column 1 holds item 4 too
      4    3  0   its item is the pad id below item_lo: column 4 leaves every other row
      5    9  6   a u_id outside the CSR: nothing seen
      6    4  7   seen_off[5] lies beyond nnz (clamped): the row still masks item 6 (column 5)
      7    2  8   the second row of user 2
    -> (u_ids, i_ids int64 [8], (seen_off int64 [6], seen_item int32 [12]), item_lo, allowed bool [8, 8])"""
    u_ids = torch.tensor([0, 1, 1, 2, 3, 9, 4, 2], dtype=torch.int64)
    i_ids = torch.tensor([3, 4, 5, 4, 0, 6, 7, 8], dtype=torch.int64)
    off = torch.tensor([0, 6, 9, 11, 11, 19], dtype=torch.int64)
    items = torch.tensor([3, 4, 5, 6, 7, 8, 4, 5, 7, 4, 8, 6], dtype=torch.int32)
    n, y = False, True
    allowed = torch.tensor([
        [y, n, n, n, n, n, n, n],
        [y, y, n, n, n, y, n, y],
        [y, n, y, n, n, y, n, y],
        [y, n, y, y, n, y, y, n],
        [y, y, y, y, y, y, y, y],
        [y, y, y, y, n, y, y, y],
        [y, y, y, y, n, n, y, y],
        [y, n, y, n, n, y, y, y],
    ])
    return u_ids, i_ids, (off, items), 1, allowed


def random_case(B, K, fm, seed, *, with_rb, with_cb, with_logq, with_drop, n_users=None, n_items=None, scale=1.0):
    """A reproducible case: normal latents (no product anywhere near the f32 underflow: asserted), ids from small ranges so that
    duplicate items, repeated users and seen items occur, a seen CSR over n_users users."""
    g = torch.Generator().manual_seed(seed)
    n_users = n_users or max(2, B // 2)
    n_items = n_items or max(3, (3 * B) // 4 + 2)
    c = {"fm": fm, "item_lo": 1}
    c["ul"] = (torch.randn(B, K, generator=g) * scale).float()
    c["il"] = torch.randn(B, K, generator=g).float()
    assert float((c["ul"].double()[:, None, :] * c["il"].double()[None, :, :]).abs().min()) > 1e-30
    c["h"] = torch.randn(K, generator=g).float() if fm else None
    c["row_bias"] = torch.randn(B, generator=g).float() if with_rb else None
    c["col_bias"] = torch.randn(B, generator=g).float() if with_cb else None
    c["logq"] = (-3.0 + torch.rand(B, generator=g)).float() if with_logq else None
    c["drop"] = ((torch.rand(B, B, K, generator=g) >= 0.5).float() * 2.0) if (with_drop and fm) else None
    c["u_ids"] = torch.randint(0, n_users + 1, (B,), generator=g)          # n_users itself lies outside the CSR
    c["i_ids"] = torch.randint(0, n_items, (B,), generator=g)              # 0 is the pad id
    rows = [sorted(set(torch.randint(1, n_items, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g).tolist()))
            for _ in range(n_users)]
    off = np.cumsum([0] + [len(r) for r in rows])
    c["seen"] = (torch.tensor(off, dtype=torch.int64), torch.tensor([x for r in rows for x in r] or [0], dtype=torch.int32)[:max(int(off[-1]), 1)])
    if int(off[-1]) == 0:
        c["seen"] = None
    return c
