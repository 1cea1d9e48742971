"""Plain float64 restatement, with a per-element error bound, of the "f16x2s" realisation of the bf16x3 class (rbr_set_prod_split;
include/rbr_hip.h): the distinct-token GEMM T = X @ Wprod with every operand split into TWO f16 planes of x * 2^s, three plane
products per f32 product, f32 accumulation, the scale taken back out of the sum.  tests/test_f16_split_gemm_edges_gpu.py compares
the HIP kernel with it; tests/test_f16_split_ref_host.py checks the rounding against a bit-level f16, the bound against an f32 CPU
emulation of the class, and that a dropped K chunk and an unscaled weight plane leave the bound.

Conventions of tests/edge_refs.py and tests/conv_class_ref.py: every value comes with `Abs`, the same expression on magnitudes, and
an f32 sum of n terms is bounded by bound_of(n, Abs).  Nothing here is taken from the kernels' code.

The class.  s(v) is an integer read off the exponent FIELD e of the f32 amax of a token row / a weight column: s = 14 + 127 - e, so
that amax * 2^s lies in [2^14, 2^15) (at most 32768 after rounding: under f16's 65504); s = 0 for an amax of 0 and for a non-finite
one.  With y = x * 2^s (exact: a power of two):  h1 = f16(y),  h2 = f16(y - h1)  (round to nearest even; the residue is exact in
f32), and
    T[i, j] = 2^-(s_i + s_j) * sum_k (xl wh + xh wl + xh wh)[i, k, j]              accumulated in f32, small terms first.

The bound, three parts (all in the UNSCALED units of T; a power-of-two scale moves value and error alike):
  1. f32 accumulation of 3 n products: bound_of(3 n, PLANES2_ABS * Abs).  |h1| <= (1 + 2^-11) |y| and |h2| <= 2^-11 |y| (half an
     f16 spacing), so the three products' magnitudes sum to less than (1 + 2^-11)(1 + 3 * 2^-11) |x w| < PLANES2_ABS |x w|.
  2. what the split leaves out: y = h1 + h2 + t with |t| <= 2^-22 |y| while y - h1 is a normal f16 (half a spacing of an 11-bit
     significand at a residue of at most 2^-11 |y|), so  x w - (kept products) = xl wl + tx w + x tw - tx tw, of magnitude at most
     (2^-22 + 2 * 2^-22)(1 + 2^-10) |x w| < SPLIT_DROPPED * |x w| = 13 EPS |x w|.
  3. a floor for the elements whose low plane lies under f16's normal range (|y - h1| < 2^-14, or |y| < 2^-14 itself): there t is
     not relative any more.  If the matrix pipe honours f16 subnormals, |t| <= 2^-25 (half the subnormal spacing); if it flushes
     them, the whole plane is lost, |t| < 2^-14.  In unscaled units 2^-s <= amax * 2^-14, so such an element carries an absolute
     error of at most FLOOR * amax(its row / column), FLOOR = 2^-28 (1 + 2^-10) (the factor covers the cross term), and
         floor[i, j] = FLOOR * (amax_x[i] * sum_k under_x[i, k] |w[k, j]| + amax_w[j] * sum_k |x[i, k]| under_w[k, j]).
     The bound holds whichever the hardware does; `flush` below only selects the VALUE of the class for the two variants.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from edge_refs import EPS, bound_of

F64, F32 = torch.float64, torch.float32
BINADE = 14
F16_MIN_NORMAL = 2.0 ** -14
PLANES2_ABS = (1 + 2.0 ** -10) ** 2
SPLIT_DROPPED = 13 * EPS
FLOOR = 2.0 ** -28 * (1 + 2.0 ** -10)


# ------------------------------------------------------------------------------------------------------------------- rounding
def rh(x, flush=False):
    """f32 -> f16, round to nearest even, and back to f32.  flush: a subnormal f16 result reads as zero."""
    h = x.to(F32).to(torch.float16).to(F32)
    return torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h) if flush else h


def exponent_of(amax):
    """The integer s of an f32 amax >= 0 (or NaN), read off its exponent field; 0 for 0 and for inf / NaN."""
    bits = amax.to(F32).contiguous().view(torch.int32) & 0x7FFFFFFF
    e = bits >> 23
    return torch.where((bits == 0) | (e == 255), torch.zeros_like(e), BINADE + 127 - e)


def amax_of(x, dim):
    """Largest magnitude along dim; NaN wins (the kernel takes an integer max of the magnitudes' bits, where NaN > inf)."""
    a = x.to(F32).abs()
    m = torch.where(torch.isnan(a), torch.full_like(a, float("inf")), a).amax(dim)
    return torch.where(torch.isnan(a).any(dim), torch.full_like(m, float("nan")), m)


def planes(x, s, flush=False):
    """(h1, h2) of y = x * 2^s, as f32 tensors; s broadcasts against x."""
    y = torch.ldexp(x.to(F32), s)
    h1 = rh(y)
    h2 = rh(y - h1)
    if flush:
        h1, h2 = rh(h1, True), rh(h2, True)
    return h1, h2


def under_normal(x, s):
    """Elements whose low plane (or the element itself) lies under f16's normal range: part 3 of the bound."""
    y = torch.ldexp(x.to(F32), s)
    r = y - rh(y)
    return ((r.abs() < F16_MIN_NORMAL) & (r != 0)) | ((y.abs() < F16_MIN_NORMAL) & (y != 0))


def bound_f16x2s(n, ab):
    """Parts 1 and 2: a sum of n f32 products computed as 3 n plane products of two-plane splits, `ab` = sum of |x w|."""
    return bound_of(3 * n, PLANES2_ABS * ab) + SPLIT_DROPPED * ab


# -------------------------------------------------------------------------------------------------------------- product table
def product_table(X, Wp, dt=F64, flush=False, drop_k=False, unscaled_w=False, exact=True):
    """T [V, cp] -> (T in dt, AbsT, bound of the f32-accumulated T), the last two in float64.
    exact (the centre the kernel is compared with): X @ Wp on the f32 operands, as conv_class_ref does for bf16x3.  exact = False:
    the VALUE of the class itself -- the three kept plane products, rescaled -- in dt; dt = f32 is the host test's emulation
    (f32 matmuls), dt = float64 with flush = False / True the two variants a subnormal-plane observation is compared with.
    drop_k (sensitivity): the last K chunk -- the last D % 16 columns of X, or the last 16 -- is left out.
    unscaled_w (sensitivity): the weight planes are split without their scale (s_col = 0)."""
    X, Wp = X.to(F32), Wp.to(F32)
    D = X.shape[1]
    sr, sc = exponent_of(amax_of(X, 1)), exponent_of(amax_of(Wp, 0))
    ab = X.double().abs() @ Wp.double().abs()
    ux, uw = under_normal(X, sr[:, None]).double(), under_normal(Wp, sc[None, :]).double()
    floor = FLOOR * (amax_of(X, 1).double()[:, None] * (ux @ Wp.double().abs()) + (X.double().abs() @ uw) * amax_of(Wp, 0).double()[None, :])
    bT = bound_f16x2s(D, ab) + floor
    Xk = X
    if drop_k:
        Xk = X.clone()
        Xk[:, D - (D % 16 or 16):] = 0.0
    if exact and not drop_k and not unscaled_w:
        return X.to(dt) @ Wp.to(dt), ab, bT
    scw = torch.zeros_like(sc) if unscaled_w else sc
    xh, xl = planes(Xk, sr[:, None], flush)
    wh, wl = planes(Wp, scw[None, :], flush)
    acc = xl.to(dt) @ wh.to(dt) + xh.to(dt) @ wl.to(dt) + xh.to(dt) @ wh.to(dt)
    T = torch.ldexp(acc, -(sr[:, None] + scw[None, :]))
    return T, ab, bT


# -------------------------------------------------------------------------------------------------------------------- forward
def wprod(ws):
    """Wprod [D, cp]: column (w, j, c) holds W_w[c, :, j]."""
    return torch.cat([w.permute(1, 2, 0).reshape(w.shape[1], -1) for w in ws], 1)


def forward(inp, dt=F64, **kw):
    """Un-gated PAD_SAME ReLU conv over `inp` (table, ids, mask or None, ws, bs, kzs, chans, V) from the product table of the class
    -> namespace T, AbsT, bT, feat, bfeat.  y[doc, p, c] = sum_j T[row(p + j - padl), (w, j, c)], a masked or out-of-range position
    reads the zero row;  by = sum_j bT + bound_of(kz, sum_j |T|);  feat = relu(max_p y + bias), bfeat = max_p by + EPS (|max y + bias|
    + max_p by) (|max a - max b| <= max |a - b|; relu is 1-Lipschitz; the bias add rounds once).  kw: product_table's."""
    n, L = inp.ids.shape
    Wp = wprod(inp.ws)
    cp, V = Wp.shape[1], inp.V
    T, AbsT, bT = product_table(inp.table, Wp, dt, **kw)
    Tz, bTz = torch.cat([T, torch.zeros(1, cp, dtype=dt)]), torch.cat([bT, torch.zeros(1, cp, dtype=F64)])
    KF = max(inp.kzs)
    live = torch.ones_like(inp.ids, dtype=torch.bool) if inp.mask is None else inp.mask
    tokp = F.pad(torch.where(live, inp.ids, torch.full_like(inp.ids, V)), (KF, KF), value=V)
    feats, bfeats = [], []
    poff = 0
    for w, (kz, ch) in enumerate(zip(inp.kzs, inp.chans)):
        padl = (kz - 1) // 2
        y, ay, by = torch.zeros(n, L, ch, dtype=dt), torch.zeros(n, L, ch, dtype=F64), torch.zeros(n, L, ch, dtype=F64)
        for j in range(kz):
            rows = tokp[:, KF + j - padl:KF + j - padl + L]
            cols = poff + j * ch + torch.arange(ch)
            t = Tz[:, cols][rows]
            y = y + t
            ay += t.double().abs()
            by += bTz[:, cols][rows]
        by = by + bound_of(kz, ay)
        m, bm = y.max(1).values, by.max(1).values
        pre = m + inp.bs[w].to(dt)
        feats.append(torch.relu(pre))
        bfeats.append(bm + torch.where(ay.max(1).values > 0, EPS * (pre.double().abs() + bm), torch.zeros_like(bm)))
        poff += kz * ch
    return SimpleNamespace(T=T, AbsT=AbsT, bT=bT, feat=torch.cat(feats, 1), bfeat=torch.cat(bfeats, 1))


# ---------------------------------------------------------------------------------------------------------------------- cases
def make_case(name, n_docs=4, L=64, D=180, V=300, kzs=(3, 5), chans=(60, 120), seed=104, n_rows=None, masked_doc=None):
    """Inputs in the form of conv_class_ref.make_inputs (F4 is the default shape: 7 column groups, 12 K steps with 4 live columns in
    the last, three row blocks with the last one cut).  n_rows: the documents use only the first n_rows token ids (a list shorter
    than one row block);  masked_doc: that document is masked out whole."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, D, generator=g)
    ids = torch.randint(0, n_rows or V, (n_docs, L), generator=g)
    ws = [torch.randn(c, D, k, generator=g) * (1.0 / (D * k) ** 0.5) for k, c in zip(kzs, chans)]
    bs = [torch.randn(c, generator=g) * 0.1 for c in chans]
    mask = None
    if masked_doc is not None:
        mask = torch.ones(n_docs, L, dtype=torch.bool)
        mask[masked_doc] = False
    return SimpleNamespace(name=name, table=table, ids=ids, mask=mask, ws=ws, bs=bs, kzs=list(kzs), chans=list(chans),
                           n_docs=n_docs, L=L, D=D, V=V)


def scaled(inp, s):
    """table * 2^s, weights * 2^-s (exact): the same T, bit for bit."""
    return SimpleNamespace(**{**vars(inp), "name": f"{inp.name}*2^{s}", "table": torch.ldexp(inp.table, torch.tensor(s)),
                              "ws": [torch.ldexp(w, torch.tensor(-s)) for w in inp.ws]})


def with_table(inp, name, table, ws=None):
    return SimpleNamespace(**{**vars(inp), "name": name, "table": table, "ws": inp.ws if ws is None else ws})


def route(inp):
    """-> (column groups, K steps, takes the f16x2s kernel?): six or more 128-column groups and twelve or more 16-deep steps."""
    cp = sum(k * c for k, c in zip(inp.kzs, inp.chans))
    ngroups, nchunks = -(-cp // 128), -(-inp.D // 16)
    return ngroups, nchunks, ngroups >= 6 and nchunks >= 12 and inp.D % 4 == 0
