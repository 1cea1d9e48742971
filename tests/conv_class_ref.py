"""Plain float64 restatement, with per-element error bounds, of the token-product TextCNN in each arithmetic class of its bf16-pipe
GEMMs (rbr_set_prod_precision: f32, bf16x3, bf16x2, bf16; rbr_set_b16_storage: the bf16 class with a bf16 product table), forward
and backward, and the cases tests/test_conv_classes_edges_gpu.py runs the HIP kernels at.  tests/test_conv_class_ref_host.py
checks the rounding against a bit-level one, the formulas against torch autograd, the bounds against an f32 CPU computation of
the same class, and that the cases reach the kernel instantiations they are there for.

Conventions of tests/edge_refs.py: every value comes with `Abs`, the same expression on magnitudes, and an f32 result is bounded by
bound_of(n, Abs) = (n + 4) * EPS * Abs, n the number of terms behind the element.  An element whose bound is 0 has no terms and
must be exactly 0.  Nothing here is taken from the kernels' code; `dt` = torch.float32 evaluates the same formulas in f32 (the
host test's emulation: operands rounded as the class says, f32 accumulation, a stored table rounded with rb).

Layout: product channel (w, j, c) of bank w, tap j, channel c is column poff[w] + j * ch[w] + c, poff[w] = sum_{v < w} kz[v] * ch[v];
T[token, (w, j, c)] = sum_d X[token, d] * W_w[c, d, j];  y[doc, c, p] = sum_j gate[p + j - padl] * T[row(p + j - padl), (w, j, c)] with
padl = (kz - 1) // 2 (PAD_SAME, pool length L) or 0 (PAD_VALID, pool length L - kz + 1);  feat = act(max_p y + bias).  A masked or
out-of-range position reads the zero row.  A padding_idx token reads its table row like any other token (nn.Embedding keeps that
row zero, and so do the cases here) and its table row gets no gradient.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from edge_refs import EPS, bound_of

F64, F32 = torch.float64, torch.float32
# bf16 keeps 8 significant bits (1 implicit + 7 stored): the spacing in [2^e, 2^(e+1)) is 2^(e-7), HALF a spacing 2^(e-8) <= 2^-8 |v|
BF16_SIG_BITS = 8
# |hi| <= (1 + 2^-8) |x|, |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|: the magnitudes of the six plane products kept by the three-plane
# split sum to less than (1 + 2^-7 + 2^-14)(1 + 2^-7 + 2^-14) |x w| < 1.016 |x w| ...
PLANES3_ABS = (1 + 2.0 ** -7 + 2.0 ** -14) ** 2
# ... and the three dropped ones, mid*lo + lo*mid + lo*lo, to (2 * 2^-8 * 2^-16 + 2^-32) |x w| < 2^-23 |x w| = 2 EPS |x w|
PLANES3_DROPPED = 2 * EPS


# ------------------------------------------------------------------------------------------------------------------- rounding
def rb(x):
    """f32 -> bf16, round to nearest even, and back to f32 (the rounding pack_bf16 of csrc/textcnn_b16.h states)."""
    return x.to(F32).to(torch.bfloat16).to(F32)


def planes(x):
    """hi = rb(x), mid = rb(x - hi), lo = rb(x - hi - mid); both residues are exact f32 subtractions."""
    x = x.to(F32)
    hi = rb(x)
    r = x - hi
    mid = rb(r)
    return hi, mid, rb(r - mid)


def half_spacing(a):
    """Half a bf16 spacing at magnitude a (float64, >= 0): 2^(floor(log2 a) - 8); 0 at 0.  frexp: a = m * 2^e, m in [0.5, 1), so
    floor(log2 a) = e - 1 and the half spacing is 2^(e - 1 - BF16_SIG_BITS)."""
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 1 - BF16_SIG_BITS), torch.zeros_like(a))


def bound3(n, ab):
    """Bound of a sum of n f32 products computed as 6 n plane products of three-plane splits, `ab` = sum of |x w|."""
    return bound_of(6 * n, PLANES3_ABS * ab) + PLANES3_DROPPED * ab


# -------------------------------------------------------------------------------------------------------------------- the cases
def _c(name, n_docs, L, D, V, kzs, chans, seed, **kw):
    d = dict(name=name, n_docs=n_docs, L=L, D=D, V=V, kzs=kzs, chans=chans, seed=seed, mask_p=None, gate=False, valid=False,
             tanh=False, padding_idx=None, all_masked=False, right_pad=False, take_docs=None, take_L=None, take_ch=None)
    d.update(kw)
    return SimpleNamespace(**d)


F_CASES = [
    _c("F1", 3, 20, 12, 30, [3, 5], [4, 5], 101, mask_p=0.2),
    _c("F2", 4, 64, 36, 150, [1, 9], [3, 33], 102, mask_p=0.2, gate=True, tanh=True),
    _c("F3", 3, 30, 20, 60, [2, 3, 4], [20, 20, 20], 103, valid=True, gate=True, tanh=True),
    _c("F4", 4, 64, 180, 300, [3, 5], [60, 120], 104),
    _c("F5", 2, 40, 20, 50, [5, 7], [65, 70], 105),
    _c("F6", 3, 33, 8, 40, [3], [130], 106),
    _c("F6b", 3, 33, 8, 40, [3], [70], 107),
    _c("F7", 1, 1, 8, 5, [3], [2], 108),
    _c("F8", 3, 20, 12, 30, [3, 5], [4, 5], 101, mask_p=0.2, all_masked=True),
    _c("F9", 4, 64, 36, 150, [1, 9], [3, 33], 102, gate=True, tanh=True, padding_idx=0, right_pad=True),
]
F_RUNS = [("bf16", True), ("bf16", False), ("bf16x2", False)]          # (class, bf16 storage)

B_CASES = [
    _c("B1", 512, 6, 8, 40, [3], [5], 201),
    _c("B2", 512, 12, 132, 200, [3, 5], [7, 9], 202, mask_p=0.3),
    _c("B2g", 512, 12, 132, 200, [3, 5], [7, 9], 202, mask_p=0.3, gate=True),
    _c("B3", 640, 50, 100, 700, [3], [100], 203, mask_p=0.3),
    _c("B4-512", 512, 8, 8, 40, [3], [5], 204),
    _c("B4-511", 512, 8, 8, 40, [3], [5], 204, take_docs=511),
    _c("B4b-128", 512, 129, 8, 40, [3], [5], 205, take_L=128),
    _c("B4b-129", 512, 129, 8, 40, [3], [5], 205),
    _c("B5", 512, 8, 16, 3, [1, 3], [6, 6], 206),
    _c("B6-2048", 512, 4, 8, 30, [1], [2049], 207, take_ch=2048),
    _c("B6-2049", 512, 4, 8, 30, [1], [2049], 207),
]
B_RUNS = [("bf16x3", False), ("bf16", True)]

ALL_RUNS = [(c, cls, st) for c in F_CASES for cls, st in F_RUNS] + [(c, cls, st) for c in B_CASES for cls, st in B_RUNS]


def run_id(run):
    c, cls, st = run
    return f"{c.name}-{cls}{'-t16' if st else ''}"


_INPUTS = {}


def make_inputs(case):
    """The CPU f32 operands of a case (built once per case, never modified).  take_docs / take_L / take_ch: the same data cut to the
    first documents / positions / channels, for the two sides of a dispatch rule."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    g = torch.Generator().manual_seed(case.seed)
    n, L, D, V = case.n_docs, case.L, case.D, case.V
    table = torch.randn(V, D, generator=g)
    lo = 1 if case.padding_idx is not None else 0
    ids = torch.randint(lo, V, (n, L), generator=g)
    mask = (torch.rand(n, L, generator=g) > case.mask_p) if case.mask_p is not None else None
    ws = [torch.randn(c, D, k, generator=g) * (1.0 / np.sqrt(D * k)) for k, c in zip(case.kzs, case.chans)]
    bs = [torch.randn(c, generator=g) * 0.1 for c in case.chans]
    gate = torch.rand(n, L, generator=g) * 0.8 + 0.1 if case.gate else None
    d_feat = torch.randn(n, sum(case.chans), generator=g)
    if case.all_masked:
        mask = torch.zeros(n, L, dtype=torch.bool)
    if case.right_pad:                                        # right-padded documents over a zero padding row, no mask
        lens = torch.randint(0, L + 1, (n,), generator=g)
        lens[0], lens[1] = 0, L
        ids[torch.arange(L)[None, :] >= lens[:, None]] = case.padding_idx
        table[case.padding_idx] = 0.0
        mask = None
    if case.take_docs is not None:
        k = case.take_docs
        ids, d_feat = ids[:k].contiguous(), d_feat[:k].contiguous()
        mask = mask[:k].contiguous() if mask is not None else None
        gate = gate[:k].contiguous() if gate is not None else None
    if case.take_L is not None:
        k = case.take_L
        ids = ids[:, :k].contiguous()
        mask = mask[:, :k].contiguous() if mask is not None else None
        gate = gate[:, :k].contiguous() if gate is not None else None
    chans = list(case.chans)
    if case.take_ch is not None:
        k = case.take_ch
        ws, bs, d_feat, chans = [ws[0][:k].contiguous()], [bs[0][:k].contiguous()], d_feat[:, :k].contiguous(), [k]
    inp = SimpleNamespace(table=table, ids=ids, mask=mask, ws=ws, bs=bs, gate=gate, d_feat=d_feat, kzs=list(case.kzs), chans=chans,
                          valid=case.valid, tanh=case.tanh, padding_idx=case.padding_idx, n_docs=ids.shape[0], L=ids.shape[1], D=D, V=V)
    _INPUTS[case.name] = inp
    return inp


# ------------------------------------------------------------------------------------------------------------- the dispatch
def expected_kernels(inp, cls, storage, row_sink=False):
    """Names of the kernels a conv of this shape runs in class `cls` (`storage`: rbr_set_b16_storage(1)) under the token-product
    formulation: {"gemm", "pool", "bwd_table", "bwd_dw"}.  A plain restatement of the dispatch rules of prod_b16_gemm,
    prod_b16_rows_applicable / dtable_through_list and dw_from_g_applicable (csrc/textcnn_prod_b16.hip, csrc/textcnn_prod.hip) with
    the process-static A/B switches at their defaults -- Python cannot observe which kernel ran, so THIS FUNCTION MUST FOLLOW THE
    DISPATCH WHEN THE DISPATCH CHANGES: it is how the cases above are shown to reach the instantiations they name.
    row_sink: the table gradient leaves in compact row form (functional.set_row_grad_sink; un-gated convs only) -- the only form in
    which the many-short-documents class multiplies G out with the row GEMM."""
    D, n_docs, L = inp.D, inp.n_docs, inp.L
    cp = sum(k * c for k, c in zip(inp.kzs, inp.chans))
    ngroups, nchunks = -(-cp // 128), -(-D // 16)
    b16 = cls != "f32" and D % 4 == 0
    t16 = bool(storage) and b16 and cls == "bf16"
    nprod = {"bf16x3": 6, "bf16x2": 3, "bf16": 1}.get(cls)
    if not b16:
        gemm = "f32 mfma"
    elif t16:
        gemm = "prod_gemm_b16sd_kernel" if ngroups >= 6 else "rows_to_b16_kernel+prod_gemm_b16s_kernel"
    elif cls == "bf16x3" and 4 <= nchunks <= 8 and ngroups >= 4:
        gemm = f"prod_gemm_b16k_kernel<6,{nchunks}>"
    elif ngroups >= 6 and nchunks >= 12:
        gemm = f"prod_gemm_b16d_kernel<{nprod},8>"
    else:
        gemm = f"prod_gemm_b16_kernel<{nprod}>"
    pool = "gather_pool_kernel<true>" if t16 else "gather_pool_kernel<false>"
    short_docs = D % 4 == 0 and L <= 128 and n_docs >= 512 and cp <= 2048
    rows_form = bool(row_sink) and inp.gate is None
    planes_bwd = 1 if cls == "bf16" else 3
    if short_docs:
        bwd_dw = f"dw_from_g_b16_kernel<{planes_bwd}>"
        bwd_table = f"rows prod_gemm_b16_kernel<{1 if cls == 'bf16' else 6}>" if rows_form else "g_times_w_kernel"
    else:
        bwd_dw = "window rows f32"
        bwd_table = "g_times_w_kernel"
    return {"gemm": gemm, "pool": pool, "bwd_table": bwd_table, "bwd_dw": bwd_dw}


def backward_form(inp, cls, row_sink):
    """(dW from G on the bf16 pipe?, dtable by the row GEMM?) -- the two class-dependent pieces of the backward."""
    k = expected_kernels(inp, cls, False, row_sink)
    return k["bwd_dw"].startswith("dw_from_g"), k["bwd_table"].startswith("rows")


# -------------------------------------------------------------------------------------------------------------- product table
def wprod(ws):
    """Wprod [D, cp]: column (w, j, c) holds W_w[c, :, j]."""
    return torch.cat([w.permute(1, 2, 0).reshape(w.shape[1], -1) for w in ws], 1)


def product_table(X, Wp, cls, storage, dt=F64, drop_k=False):
    """T [V, cp] of class `cls` -> (T in dt, AbsT, bound of an f32-accumulated T), the last two in float64.
      f32    : the f32 operands; D terms.
      bf16x3 : the f32 operands; 6 D plane products, bound3 (their magnitudes and the dropped cross terms, see PLANES3_*).
      bf16x2 : xh*wh + xh*wm + xm*wh, each exact in f32; 3 D terms.
      bf16   : rb(x) * rb(w); D terms.
    storage: the kernel stores rb(f32 sum).  The float64 T is NOT rounded (the two sums can sit on opposite sides of a tie); the
    bound grows by half a bf16 spacing at the largest magnitude the f32 sum can have, |T| + bound.  dt = f32: T is rounded.
    drop_k (sensitivity): the last K chunk -- the last D % 16 columns of X, or the last 16 -- is left out."""
    X, Wp = X.to(F32), Wp.to(F32)
    D = X.shape[1]
    if drop_k:
        X = X.clone()
        X[:, D - (D % 16 or 16):] = 0.0
    if cls in ("f32", "bf16x3"):
        pairs = [(X, Wp)]
    elif cls == "bf16x2":
        (xh, xm, _), (wh, wm, _) = planes(X), planes(Wp)
        pairs = [(xh, wh), (xh, wm), (xm, wh)]
    else:
        pairs = [(rb(X), rb(Wp))]
    T = sum(a.to(dt) @ b.to(dt) for a, b in pairs)
    ab = sum(a.double().abs() @ b.double().abs() for a, b in pairs)
    bT = bound3(D, ab) if cls == "bf16x3" else bound_of(len(pairs) * D, ab)
    if storage:
        if dt == F32:
            T = rb(T)
        bT = bT + half_spacing(T.double().abs() + bT)
    return T, ab, bT


# -------------------------------------------------------------------------------------------------------------------- forward
def _live(inp):
    return torch.ones_like(inp.ids, dtype=torch.bool) if inp.mask is None else inp.mask


def forward(inp, cls, storage, dt=F64, drop_k=False, shift_bank=None):
    """-> namespace: T, AbsT, bT, y / by (per bank, [n_docs, pool length, ch]), feat / bfeat [n_docs, C], argmax (an index of the maximum).
      by    = sum_j |gate| bT + bound_of(kz, sum_j |gate T|)             kz terms, one rounding each
      bfeat = max_p by + EPS (|max y + bias| + max_p by) [+ 4 EPS: tanhf]  |max a - max b| <= max |a - b|; relu and tanh are 1-Lipschitz; the
              bias add rounds once -- unless the pooled value has no terms at all (y == 0 exactly: 0 + bias is exact).
    shift_bank (sensitivity): that bank's last tap reads the columns of the next channel."""
    n, L = inp.ids.shape
    Wp = wprod(inp.ws)
    cp, V = Wp.shape[1], inp.V
    T, AbsT, bT = product_table(inp.table, Wp, cls, storage, dt, drop_k)
    Tz, bTz = torch.cat([T, torch.zeros(1, cp, dtype=dt)]), torch.cat([bT, torch.zeros(1, cp, dtype=F64)])
    KF = max(inp.kzs)
    tokp = F.pad(torch.where(_live(inp), inp.ids, torch.full_like(inp.ids, V)), (KF, KF), value=V)
    gp = F.pad(inp.gate if inp.gate is not None else torch.ones(n, L), (KF, KF), value=1.0)
    ys, bys, feats, bfeats, ams = [], [], [], [], []
    poff = 0
    for w, (kz, ch) in enumerate(zip(inp.kzs, inp.chans)):
        padl = 0 if inp.valid else (kz - 1) // 2
        Lv = L - kz + 1 if inp.valid else L
        y, ay, by = torch.zeros(n, Lv, ch, dtype=dt), torch.zeros(n, Lv, ch, dtype=F64), torch.zeros(n, Lv, ch, dtype=F64)
        for j in range(kz):
            sl = slice(KF + j - padl, KF + j - padl + Lv)
            cols = poff + j * ch + torch.arange(ch)
            if shift_bank == w and j == kz - 1:
                cols = poff + j * ch + (torch.arange(ch) + 1) % ch
            rows = tokp[:, sl]
            t, bt = Tz[:, cols][rows], bTz[:, cols][rows]
            gj = gp[:, sl].unsqueeze(-1)
            y = y + gj.to(dt) * t
            ay += gj.double().abs() * t.double().abs()
            by += gj.double().abs() * bt
        by = by + bound_of(kz, ay)
        m, am = y.max(1)
        bm = by.max(1).values
        pre = m + inp.bs[w].to(dt)
        round_add = torch.where(ay.max(1).values > 0, EPS * (pre.double().abs() + bm), torch.zeros_like(bm))
        feats.append(torch.tanh(pre) if inp.tanh else torch.relu(pre))
        bfeats.append(bm + round_add + (4 * EPS if inp.tanh else 0.0))
        ys.append(y); bys.append(by); ams.append(am)
        poff += kz * ch
    return SimpleNamespace(T=T, AbsT=AbsT, bT=bT, y=ys, by=bys, feat=torch.cat(feats, 1), bfeat=torch.cat(bfeats, 1), argmax=torch.cat(ams, 1))


ENGAGED_FACTOR = 2.0


def engaged(feat, ref, f32):
    """Was a reduced class engaged?  `ref` / `f32`: forward() of the class and of the f32 class.  -> (near, outside):
      near    : feat is nearer (sum of squares over all elements) to the class's reference than to the f32-class one -- an
                f32-class kernel sits at the distance between the two centres from `ref` and at its rounding noise from `f32`
                (no factor between the two: a stored table's rounding is noise of the size of that distance);
      outside : feat leaves the f32-class bound at some element.  Asked only where the class's CENTRE is outside that bound by
                ENGAGED_FACTOR at some element (a statement about the two references, not about the code under test); otherwise True."""
    got = feat.detach().cpu().double()
    near = float((got - ref.feat).square().sum()) < float((got - f32.feat).square().sum())
    centre = ((ref.feat - f32.feat).abs() > ENGAGED_FACTOR * f32.bfeat).any()
    outside = bool(((got - f32.feat).abs() > f32.bfeat).any()) if bool(centre) else True
    return near, outside


# ------------------------------------------------------------------------------------------------------------------- backward
def backward(inp, T, bT, feat, argmax, cls, dw_from_g, row_gemm, dt=F64, drop_k=False):
    """Backward from a forward's OWN feat and argmax (relu flips and pool ties are not part of the comparison), the upstream d_feat
    and the forward's product table T with its bound (d(gate) is read off it) -> {name: (value in dt, bound in float64)} for
    "dtable", "dW<w>", "db<w>" and, gated, "dgate".
      g = d_feat * act'(feat)                       relu: [feat > 0];  tanh: 1 - feat^2, of magnitude <= 1 + feat^2
      G[t, (w,j,c)] = sum g * gate over the (doc, c) windows whose tap j sits on an un-masked token t;  an f32 atomic sum:
                      bG = bound_of(hits, AbsG)
      dgate[doc, p] = sum g * T[t, (w,j,c)] over the windows with a tap on p:  sum |g| bT + bound_of(hits, sum |g T|)
      dbias[c]      = sum_doc g                                                  n = n_docs
      dtable = G @ Wprod^T, dW = G^T @ X (folded to [C, D, kz]), each by the form the shape selects:
        f32 (small shapes: sparse row product / window rows)   bG @ |W| + bound_of(non-zeros of the G row + 4 wave partials, AbsG @ |W|);
                                                               dW: bound_of(hits of the column, AbsG^T @ |X|) -- a term per window
        planes (every class but bf16, row GEMM / dW from G)    bG @ |W| + bound3(non-zeros [+ 32 partial sums of the K splits], AbsG @ |W|)
        bf16                                                   the kernel rounds ITS G (an f32 sum we cannot reproduce bit for bit), W and
                                                               X to bf16: centred on the unrounded G with rb(W), rb(X); each G differs
                                                               from the rounded one by at most eG = bG + half a bf16 spacing at |G| + bG:
                                                               eG @ |rb W| + bound_of(non-zeros [+ 32], (AbsG + eG) @ |rb W|)
    drop_k (sensitivity, row GEMM only): the last K chunk of the contraction -- the last cp % 16 columns of G, or the last 16 -- is left out."""
    n, L = inp.ids.shape
    V, D = inp.table.shape
    Wp = wprod(inp.ws)
    cp = Wp.shape[1]
    live = _live(inp)
    f, d = feat.to(dt), inp.d_feat.to(dt)
    if inp.tanh:
        g, ag = d * (1 - f * f), (d.abs() * (1 + f * f)).double()
    else:
        g = d * (f > 0).to(dt)
        ag = g.double().abs()
    G, AG, nG = torch.zeros(V * cp, dtype=dt), torch.zeros(V * cp, dtype=F64), torch.zeros(V * cp, dtype=F64)
    dg, Adg, Bdg, ndg = (torch.zeros(n * L, dtype=dt),) + tuple(torch.zeros(n * L, dtype=F64) for _ in range(3))
    doc = torch.arange(n).unsqueeze(1)
    out = {}
    coff = poff = 0
    for w, (kz, ch) in enumerate(zip(inp.kzs, inp.chans)):
        padl = 0 if inp.valid else (kz - 1) // 2
        gw, agw = g[:, coff:coff + ch], ag[:, coff:coff + ch]
        for j in range(kz):
            pos = argmax[:, coff:coff + ch].long() + j - padl
            posc = pos.clamp(0, L - 1)
            ok = (pos >= 0) & (pos < L) & live.gather(1, posc)
            tok = inp.ids.gather(1, posc)
            gv = inp.gate.gather(1, posc) if inp.gate is not None else torch.ones(n, ch)
            col = (poff + j * ch + torch.arange(ch)).unsqueeze(0).expand(n, ch)
            flat = (tok * cp + col)[ok]
            G.index_add_(0, flat, (gw * gv.to(dt))[ok])
            AG.index_add_(0, flat, (agw * gv.double().abs())[ok])
            nG.index_add_(0, flat, torch.ones(flat.shape[0], dtype=F64))
            if inp.gate is not None:
                at = (doc * L + posc)[ok]
                tv, btv = T[tok, col][ok], bT[tok, col][ok]
                dg.index_add_(0, at, gw[ok] * tv)
                Adg.index_add_(0, at, agw[ok] * tv.double().abs())
                Bdg.index_add_(0, at, agw[ok] * btv)
                ndg.index_add_(0, at, torch.ones(at.shape[0], dtype=F64))
        out[f"db{w}"] = (gw.sum(0), bound_of(n, agw.sum(0)))
        coff += ch
        poff += kz * ch
    G, AG, nG = G.view(V, cp), AG.view(V, cp), nG.view(V, cp)
    bG = bound_of(nG, AG) * (nG > 0)
    if inp.gate is not None:
        out["dgate"] = (dg.view(n, L), (Bdg + bound_of(ndg, Adg) * (ndg > 0)).view(n, L))
    nz_row, nz_col = (nG > 0).sum(1, keepdim=True).double(), (nG > 0).sum(0).double().unsqueeze(1)
    hits_col = nG.sum(0).unsqueeze(1)
    X = inp.table.to(F32)
    eG = (bG + half_spacing(G.double().abs() + bG)) * (nG > 0)

    def product(Gm, AGm, bGm, eGm, M, planes_form, n_small, n_planes):
        """Gm [r, k] @ M [k, c] in the form of the class: (value, bound)."""
        if not planes_form:
            return Gm @ M.to(dt), bGm @ M.double().abs() + bound_of(n_small, AGm @ M.double().abs())
        if cls == "bf16":
            Mr = rb(M)
            val = (rb(Gm) if dt == F32 else Gm) @ Mr.to(dt)
            return val, eGm @ Mr.double().abs() + bound_of(n_planes, (AGm + eGm) @ Mr.double().abs())
        return Gm @ M.to(dt), bGm @ M.double().abs() + bound3(n_planes, AGm @ M.double().abs())

    Gt = G
    if drop_k and row_gemm:
        Gt = G.clone()
        Gt[:, cp - (cp % 16 or 16):] = 0
    val, b = product(Gt, AG, bG, eG, Wp.t(), row_gemm, nz_row + 4, nz_row)
    if inp.padding_idx is not None:
        val, b = val.clone(), b.clone()
        val[inp.padding_idx], b[inp.padding_idx] = 0, 0
    out["dtable"] = (val, b)
    valw, bw = product(G.t(), AG.t(), bG.t(), eG.t(), X, dw_from_g, hits_col, nz_col + 32)
    poff = 0
    for w, (kz, ch) in enumerate(zip(inp.kzs, inp.chans)):
        fold = lambda t: t[poff:poff + kz * ch].reshape(kz, ch, D).permute(1, 2, 0)
        out[f"dW{w}"] = (fold(valw), fold(bw))
        poff += kz * ch
    return out
