"""Plain float64 restatements, with per-element error bounds, of the ops the edge tests of the rating head, nn.Linear,
clip + Adam, the SimpleSiamese review bag and SimpleSiamese's additive attention compare the HIP kernels with
(tests/test_pair_head_edges_gpu.py, test_linear_edges_gpu.py, test_clip_adam_edges_gpu.py, test_review_bag_edges_gpu.py,
test_additive_attn_edges_gpu.py).
tests/test_edge_refs_host.py checks every formula here against torch autograd / torch.optim.Adam in float64 on the CPU.

Every function takes f32 (or already float64) CPU tensors and computes in float64.  Beside each value it returns `Abs`, the same
expression evaluated on magnitudes -- the sum of the magnitudes of the terms behind the element -- and the tests bound an f32
result by

    bound = (n + 4) * EPS * Abs,   EPS = 2^-24,   n = number of terms behind the element

(n - 1 additions in any order; the 4 covers the roundings inside one term).  An element with Abs == 0 has no terms: it must be
exactly 0, or bit-equal to the base it is accumulated onto.  Where one stage feeds the next (adam_step, additive_attention) the
bound is propagated: every stage adds its own (n + 4) * EPS * Abs to what its inputs carry, and the function returns
(value, bound) per tensor.
"""
import math

import numpy as np
import torch

EPS = 2.0 ** -24          # unit roundoff of f32


def f64(t):
    return None if t is None else t.detach().cpu().double()


def bound_of(n, ab):
    return (n + 4) * EPS * ab


def check(family, name, got, ref, bound, base=None):
    """|got - ref| <= bound for EVERY element; where the bound is 0 that is exact equality (to 0, or bit for bit to `base`, onto
    which `got` was accumulated: ref then is the increment).  Prints the largest err / bound and returns it."""
    got = got.detach().cpu()
    ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
    assert bool(torch.isfinite(got).all()), f"{family} {name}: non-finite element"
    if base is not None:
        base = base.detach().cpu().reshape(got.shape)
        zero = bound == 0
        assert torch.equal(got[zero], base[zero]), f"{family} {name}: an element without terms differs from the base"
        ref = ref + base.double()
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"RATIO {family} {name} {worst:.4f}")
    assert worst <= 1.0, f"{family} {name}: err / bound = {worst} at flat index {int(ratio.argmax())}"
    return worst


def accumulated(bound, ab, base):
    """The bound of an output added onto `base`: one more rounding of a value of magnitude <= |base| + Abs; Abs == 0 stays 0."""
    return torch.where(ab > 0, bound + EPS * (f64(base).abs() + ab), torch.zeros_like(ab))


# ------------------------------------------------------------------------------------------------------------------ nn.Linear
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def linear_fwd(x, W, b, act, mul):
    """y = act(x @ W^T + b) * mul -> (pre, bound(pre), y, bound(y)).  pre: n = IN.  y: ReLU is 1-Lipschitz, Tanh too and gets
    4 * EPS for tanhf itself (a few ulp of a value <= 1)."""
    x, W, b, mul = f64(x), f64(W), f64(b), f64(mul)
    pre, ab = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        pre, ab = pre + b, ab + b.abs()
    bp = bound_of(x.shape[1], ab)
    y = torch.relu(pre) if act == ACT_RELU else torch.tanh(pre) if act == ACT_TANH else pre
    by = bp + 4 * EPS if act == ACT_TANH else bp
    if mul is not None:
        y, by = y * mul, by * mul.abs()
    return pre, bp, y, by


def linear_act_bwd(y, d_y, act, mul):
    """g = d_y * mul * act'(pre) from the SAVED output y = act(pre) * mul -> (g, Abs(g)).  act(pre) = y / mul where mul != 0 (where
    mul == 0, g is 0 whatever it was); ReLU: act' = [act(pre) > 0]; Tanh: act' = 1 - act(pre)^2, of magnitude <= 1 + act(pre)^2."""
    y, d, mul = f64(y), f64(d_y), f64(mul)
    if mul is None:
        a, dm = y, d
    else:
        a, dm = torch.where(mul != 0, y / torch.where(mul != 0, mul, torch.ones_like(mul)), torch.zeros_like(y)), d * mul
    if act == ACT_RELU:
        on = (a > 0).double()
        return dm * on, dm.abs() * on
    if act == ACT_TANH:
        return dm * (1 - a * a), dm.abs() * (1 + a * a)
    return dm, dm.abs()


def linear_bwd(x, W, y, d_y, act, mul):
    """{name: (value, Abs, n)} for dW [OUT, IN] = g^T x (n = N), db [OUT] = sum_n g (n = N), d_x [N, IN] = g W (n = OUT)."""
    x, W = f64(x), f64(W)
    g, ag = linear_act_bwd(y, d_y, act, mul)
    N, OUT = g.shape
    return {"dW": (g.t() @ x, ag.t() @ x.abs(), N), "db": (g.sum(0), ag.sum(0), N), "d_x": (g @ W, ag @ W.abs(), OUT)}


# ---------------------------------------------------------------------------------------------------------------- rating head
HEAD_PARAMS = ("Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib")


def head_latent(feat, ids, W, b, E):
    """LastFeat: l = feat @ W + b + E[id] -> (l, bound): n = H + 2."""
    feat, W, b, E = f64(feat), f64(W), f64(b), f64(E)
    val = feat @ W + b + E[ids]
    ab = feat.abs() @ W.abs() + b.abs() + E[ids].abs()
    return val, bound_of(feat.shape[1] + 2, ab)


def head_pred(ul, il, uid, iid, h, g, ub, ib, drop):
    """FM: pred = (relu(ul * il) * drop) @ h + ub[uid] + ib[iid] + g from the latents given -> (pred, bound): n = K + 3."""
    ul, il, h, g, ub, ib, drop = (f64(t) for t in (ul, il, h, g, ub, ib, drop))
    z = torch.relu(ul * il)
    if drop is not None:
        z = z * drop
    h = h.reshape(-1)
    val = z @ h + ub.reshape(-1)[uid] + ib.reshape(-1)[iid] + g.reshape(-1)[0]
    ab = z.abs() @ h.abs() + ub.reshape(-1)[uid].abs() + ib.reshape(-1)[iid].abs() + g.reshape(-1)[0].abs()
    return val, bound_of(ul.shape[1] + 3, ab)


def head_bwd(uf, itf, uid, iid, P, ul, il, drop, d_pred, pad_u, pad_i):
    """Backward of the head from the SAVED latents ul, il and dropout multiplier -> {name: (value, Abs, n)}, P a dict of HEAD_PARAMS.
    With z = relu(ul * il) * drop:  dz[b, k] = [ul il > 0] d_pred[b] h[k] drop[b, k];  dul = dz * il, dil = dz * ul;
      dWu = uf^T dul, dbu = sum_b dul, dh = sum_b z d_pred, dg = sum_b d_pred              n = B
      d_ufeat = dul Wu^T                                                                   n = K
      dEu[u] = sum_{b: uid[b] = u} dul[b], dub[u] = sum_{b: uid[b] = u} d_pred[b]          n = multiplicity of u; none for u == pad_u
    and the same on the item side.  The embedding-style outputs are increments (the kernel accumulates them)."""
    uf, itf, ul, il, drop, dp = (f64(t) for t in (uf, itf, ul, il, drop, d_pred))
    Wu, Wi, h = f64(P["Wu"]), f64(P["Wi"]), f64(P["h"]).reshape(-1)
    B, K = ul.shape
    U, I = P["Eu"].shape[0], P["Ei"].shape[0]
    dr = torch.ones_like(ul) if drop is None else drop
    on = (ul * il > 0).double()
    out = {}

    def both(sign):
        d = dp if sign else dp.abs()
        a = (lambda t: t) if sign else torch.abs
        dz = on * d.unsqueeze(1) * a(h).unsqueeze(0) * a(dr)
        dul, dil = dz * a(il), dz * a(ul)
        zdp = a(torch.relu(ul * il) * dr) * d.unsqueeze(1)
        res = {"dWu": a(uf).t() @ dul, "dbu": dul.sum(0), "dWi": a(itf).t() @ dil, "dbi": dil.sum(0), "dh": zdp.sum(0),
               "dg": d.sum().reshape(1), "d_ufeat": dul @ a(Wu).t(), "d_ifeat": dil @ a(Wi).t()}
        ku, ki = (uid != pad_u).double(), (iid != pad_i).double()
        res["dEu"] = torch.zeros(U, K, dtype=torch.float64).index_add_(0, uid, dul * ku.unsqueeze(1))
        res["dEi"] = torch.zeros(I, K, dtype=torch.float64).index_add_(0, iid, dil * ki.unsqueeze(1))
        res["dub"] = torch.zeros(U, dtype=torch.float64).index_add_(0, uid, d * ku)
        res["dib"] = torch.zeros(I, dtype=torch.float64).index_add_(0, iid, d * ki)
        return res

    val, ab = both(True), both(False)
    mu = torch.bincount(uid, minlength=U).double()
    mi = torch.bincount(iid, minlength=I).double()
    n = {"dWu": B, "dbu": B, "dWi": B, "dbi": B, "dh": B, "dg": B, "d_ufeat": K, "d_ifeat": K,
         "dEu": mu.unsqueeze(1), "dEi": mi.unsqueeze(1), "dub": mu, "dib": mi}
    for k in val:
        out[k] = (val[k], ab[k], n[k])
    return out


# ----------------------------------------------------------------------------------------------------------------- review bag
def review_bag(table, ids, mask, drop, d_out, padding_idx):
    """SimpleSiamese's bag of embeddings and its table gradient -> {name: (value, Abs, n)}.  With inv_len[r] = 1 / (sum_l mask[r,l]
    + 1e-8) (mask None: every position counts) and drop None = 1:
      out[r, :]    = drop[r, :] * inv_len[r] * sum_{l: mask[r,l]} table[ids[r,l], :]               n = unmasked positions of r
      dtable[t, :] = sum_{(r,l): ids[r,l] = t, mask[r,l], t != padding_idx} d_out[r, :] * inv_len[r] * drop[r, :]
                                                                                                 n = those occurrences of t
    A padding token is read like any other in the forward (its table row is what the model keeps there) and gets no gradient.
    A term's own roundings -- inv_len (the division; the 1e-8 is below f32 resolution from one position on), the products with
    inv_len and drop -- are the 4 of (n + 4)."""
    table, drop, d = f64(table), f64(drop), f64(d_out)
    n_rev, T = ids.shape
    V, D = table.shape
    m = torch.ones(n_rev, T, dtype=torch.float64) if mask is None else mask.cpu().double()
    dr = torch.ones(n_rev, D, dtype=torch.float64) if drop is None else drop
    inv = 1.0 / (m.sum(1) + 1e-8)
    rows = table[ids] * m.unsqueeze(2)
    scale = (inv.unsqueeze(1) * dr)
    out, aout = rows.sum(1) * scale, rows.abs().sum(1) * scale.abs()
    live = m if padding_idx is None else m * (ids != padding_idx).double()
    flat, w = ids.reshape(-1), live.reshape(-1, 1)
    g = (d * scale).repeat_interleave(T, 0) * w
    dt = torch.zeros(V, D, dtype=torch.float64).index_add_(0, flat, g)
    adt = torch.zeros(V, D, dtype=torch.float64).index_add_(0, flat, g.abs())
    occ = torch.zeros(V, dtype=torch.float64).index_add_(0, flat, w.reshape(-1))
    return {"out": (out, aout, m.sum(1, keepdim=True)), "dtable": (dt, adt, occ.unsqueeze(1))}


# ----------------------------------------------------------------------------------------------------------------- clip + Adam
def f32r(x):
    """the f32 rounding of a Python float, as the kernel receives lr, the betas and eps"""
    return float(np.float32(x))


def grad_norm(grads):
    return math.sqrt(sum(float(f64(g).square().sum()) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient; None / no clipping: 1.  A NaN norm gives NaN (torch.clamp keeps it), inf gives 0."""
    if max_norm is None:
        return 1.0
    r = max_norm / (norm + 1e-6)
    return r if (r < 1.0 or r != r) else 1.0


def adam_step(p, m, v, g, coef, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam step (no weight decay, no amsgrad) on the gradient g * coef, step number t, in float64 from the f32
    state -> {name: (value, bound)} for gc (the gradient left behind), m, v, p.  First-order bounds of the f32 kernel:
      gc: (1e-6 + 3 EPS) |gc| when clipping (the norm's relative bound, then the +1e-6, the division and the product), else 0
      m' = m + w1 (gc - m):           w1 bound(gc) + 3 EPS (|m| + w1 (|gc| + |m|))
      v' = b2 v + w2 gc^2:            no cancellation: relative, rel_v = 2 rel(gc) + 3 EPS
      u = s m' / (sqrt(v') / c + eps): s / denom * bound(m') + |u| (rel_v / 2 + 4 EPS)
      p' = p - u:                     bound(u) + EPS (|p| + |u|)"""
    p, m, v, g = f64(p), f64(m), f64(v), f64(g)
    lr, b1, b2, eps = f32r(lr), f32r(betas[0]), f32r(betas[1]), f32r(eps)
    w1, w2 = 1.0 - b1, 1.0 - b2
    s, c = lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
    gc = g * coef
    rel_g = (1e-6 + 3 * EPS) if coef != 1.0 else 0.0
    b_gc = rel_g * gc.abs()
    m1 = m + w1 * (gc - m)
    b_m = w1 * b_gc + 3 * EPS * (m.abs() + w1 * (gc.abs() + m.abs()))
    v1 = b2 * v + w2 * gc * gc
    rel_v = 2 * rel_g + 3 * EPS
    denom = v1.sqrt() / c + eps
    u = s * m1 / denom
    b_u = s / denom * b_m + u.abs() * (rel_v / 2 + 4 * EPS)
    p1 = p - u
    b_p = b_u + EPS * (p.abs() + u.abs())
    return {"gc": (gc, b_gc), "m": (m1, b_m), "v": (v1, rel_v * v1), "p": (p1, b_p)}


# --------------------------------------------------------------------------------------------------------- additive attention
TINY = 2.0 ** -126        # smallest normal f32: covers a result in the subnormal range, rounded there or flushed to 0


def _addatt_inputs(rev, mask, node_drop):
    rev = f64(rev)
    B, R, _ = rev.shape
    nd = torch.ones(B, R, dtype=torch.float64) if node_drop is None else f64(node_drop)
    m = torch.ones(B, R, dtype=torch.bool) if mask is None else mask.detach().cpu().bool()
    return rev, nd, m, nd.unsqueeze(2) * rev


def additive_attention_fwd(rev, mask, node_drop, Wp, bp, wi):
    """SimpleSiamese's NodeDropout + AddictiveAttention -> {name: (value, bound)} for pre, t [B,R,K], logit, scores [B,R], out [B,H].
      x = node_drop * rev                       its one rounding is one of the 4 of every (n + 4) it enters
      pre = x Wp^T + bp                         (H + 1 + 4) EPS (|x| |Wp|^T + |bp|)
      t = tanh(pre)                             bound(pre) (tanh is 1-Lipschitz) + 4 EPS for tanhf, a value <= 1
      logit = <t, wi>                           sum_k |wi_k| bound(t_k) + (K + 4) EPS sum_k |t_k wi_k|
      s = softmax_r(masked_fill(logit, ~mask, -1e8)), as the kernel has it: e_r = expf(logit_r - max), s_r = e_r * (1 / sum e).
        Logits moved by at most delta move s_r by at most a factor exp(2 delta): numerator and denominator by exp(delta) each.
        delta = max over the row's valid reviews of bound(logit_r) + EPS |logit_r - max| (the rounding of the subtraction).
        The roundings after it are relative, nothing cancels in a sum of positive terms: expf 4 EPS on the numerator and 4 EPS on
        the denominator's terms, R - 1 additions, 4 EPS for the division, 1 for the product: (R + 12) EPS.  Together
            bound(s_r) = s_r * expm1(2 delta + (R + 12) EPS) + 2 TINY
        (expf's and the division's 4 EPS are relative to a value <= 1 here, so inside the absolute 4 EPS that the other edge
        tests give a transcendental of magnitude <= 1; 2 TINY: e_r or s_r in the subnormal range, max e = 1 so sum e >= 1).
        A masked review in a row with a valid one: expf(-1e8 - max) = 0, s_r == 0 exactly, bound 0.
        A row without a valid review: every e_r = expf(0) = 1, their sum R is exact, s_r = 1/R to the division: 4 EPS / R.
      out = sum_r s_r x_r                       sum_r bound(s_r) |x_r| + (R + 4) EPS sum_r s_r |x_r|"""
    rev, nd, m, x = _addatt_inputs(rev, mask, node_drop)
    Wp, bp, wi = f64(Wp), f64(bp), f64(wi).reshape(-1)
    B, R, H = rev.shape
    K = Wp.shape[0]
    pre = x @ Wp.t() + bp
    b_pre = bound_of(H + 1, x.abs() @ Wp.abs().t() + bp.abs())
    t = torch.tanh(pre)
    b_t = b_pre + 4 * EPS
    logit = t @ wi
    b_logit = b_t @ wi.abs() + bound_of(K, t.abs() @ wi.abs())
    filled = torch.where(m, logit, torch.full_like(logit, -1e8))
    s = torch.softmax(filled, dim=1)
    mx = filled.max(1, keepdim=True).values
    zero = torch.zeros_like(logit)
    delta = torch.where(m, b_logit + EPS * (logit - mx).abs(), zero).max(1, keepdim=True).values
    b_s = s * torch.expm1(2 * delta + (R + 12) * EPS) + 2 * TINY
    any_valid = m.any(1, keepdim=True)
    b_s = torch.where(any_valid, torch.where(m, b_s, zero), torch.full_like(s, 4 * EPS / R))
    assert bool((s[any_valid.expand(B, R) & ~m] == 0).all())
    out = (s.unsqueeze(2) * x).sum(1)
    b_out = (b_s.unsqueeze(2) * x.abs()).sum(1) + bound_of(R, (s.unsqueeze(2) * x.abs()).sum(1))
    return {"pre": (pre, b_pre), "t": (t, b_t), "logit": (logit, b_logit), "scores": (s, b_s), "out": (out, b_out)}


def additive_attention_bwd(rev, mask, node_drop, Wp, wi, scores, t, d_out):
    """The backward of additive_attention_fwd from the SAVED scores [B,R] and t [B,R,K] (the kernel consumes what the forward
    kept, so the forward's error is no part of these bounds) -> {name: (value, bound)}.  With x = node_drop * rev, N = B * R:
      dsr_r = <d_out, x_r>                      (H + 4) EPS A_r,   A_r = <|d_out|, |x_r|>
      dot = sum_r s_r dsr_r                     sum_r s_r bound(dsr_r) + (R + 4) EPS sum_r s_r A_r
      dl_r = mask_r ? s_r (dsr_r - dot) : 0     s_r (bound(dsr_r) + bound(dot)) + 4 EPS Abs,  Abs = s_r (A_r + sum_j s_j A_j):
                                                the difference cancels, its roundings are relative to the operands' magnitudes
      d_pre = dl wi (1 - t^2)                   one term.  f32's 1 - t^2 is off by at most EPS (1 + t^2) ABSOLUTE (a saturated
                                                unit: most of what is left of it), so
                                                |wi| (bound(dl) (1 - t^2) + 4 EPS (|dl| + bound(dl)) (1 + t^2))
      d_wi = sum_{b,r} dl t                     sum bound(dl) |t| + (N + 4) EPS sum |dl t|          (atomics: any order)
      d_bp = sum_{b,r} d_pre                    sum bound(d_pre) + (N + 4) EPS sum |d_pre|
      d_Wp = d_pre^T x                          sum bound(d_pre) |x| + (N + 4) EPS sum |d_pre| |x|
      d_rev = node_drop (s d_out + d_pre Wp)    |node_drop| (sum_k bound(d_pre) |Wp| + (K + 1 + 4) EPS (s |d_out| + |d_pre| |Wp|))
    Bound 0, exact zeros: dl and the d_pre row of every masked review; the d_rev row of a masked review whose row has a valid
    one (s == 0 there) and of every review with node_drop == 0.  In a row WITHOUT a valid review s = 1/R and d_rev = node_drop *
    s * d_out: the masked_fill blocks the gradient of the logits, not the weighted sum's."""
    rev, nd, m, x = _addatt_inputs(rev, mask, node_drop)
    Wp, wi, s, t, dy = f64(Wp), f64(wi).reshape(-1), f64(scores).reshape(rev.shape[:2]), f64(t), f64(d_out)
    B, R, H = rev.shape
    K = Wp.shape[0]
    N = B * R
    dsr, adsr = torch.einsum("bh,brh->br", dy, x), torch.einsum("bh,brh->br", dy.abs(), x.abs())
    b_dsr = bound_of(H, adsr)
    dot, adot = (s * dsr).sum(1, keepdim=True), (s * adsr).sum(1, keepdim=True)
    b_dot = (s * b_dsr).sum(1, keepdim=True) + bound_of(R, adot)
    mf = m.double()
    dl = mf * s * (dsr - dot)
    b_dl = mf * s * (b_dsr + b_dot) + 4 * EPS * mf * s * (adsr + adot)
    f, af, w = 1 - t * t, 1 + t * t, wi.abs()
    d_pre = dl.unsqueeze(2) * wi * f
    b_dpre = w * (b_dl.unsqueeze(2) * f + 4 * EPS * (dl.abs() + b_dl).unsqueeze(2) * af)
    d_wi = torch.einsum("br,brk->k", dl, t)
    b_dwi = torch.einsum("br,brk->k", b_dl, t.abs()) + bound_of(N, torch.einsum("br,brk->k", dl.abs(), t.abs()))
    d_bp = d_pre.sum((0, 1))
    b_dbp = b_dpre.sum((0, 1)) + bound_of(N, d_pre.abs().sum((0, 1)))
    d_Wp = torch.einsum("brk,brh->kh", d_pre, x)
    b_dWp = torch.einsum("brk,brh->kh", b_dpre, x.abs()) + bound_of(N, torch.einsum("brk,brh->kh", d_pre.abs(), x.abs()))
    core = s.unsqueeze(2) * dy.unsqueeze(1) + d_pre @ Wp
    acore = s.unsqueeze(2) * dy.abs().unsqueeze(1) + d_pre.abs() @ Wp.abs()
    d_rev = nd.unsqueeze(2) * core
    b_drev = nd.abs().unsqueeze(2) * (b_dpre @ Wp.abs() + bound_of(K + 1, acore))
    return {"dl": (dl, b_dl), "d_pre": (d_pre, b_dpre), "d_wi": (d_wi, b_dwi), "d_bp": (d_bp, b_dbp), "d_Wp": (d_Wp, b_dWp),
            "d_rev": (d_rev, b_drev)}


def additive_attention(rev, mask, node_drop, Wp, bp, wi, d_out, scores=None, t=None):
    """Forward and backward in one dict {name: (value, bound)}.  `scores`, `t`: what the forward under test saved (the backward
    starts from them); None: the restatement's own float64 ones, for the comparison with autograd."""
    ref = additive_attention_fwd(rev, mask, node_drop, Wp, bp, wi)
    ref.update(additive_attention_bwd(rev, mask, node_drop, Wp, wi, ref["scores"][0] if scores is None else scores,
                                      ref["t"][0] if t is None else t, d_out))
    return ref
