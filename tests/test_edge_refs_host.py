"""The float64 formulas of tests/edge_refs.py -- the references of the GPU edge tests of the rating head, nn.Linear,
clip + Adam, the review bag and the additive attention -- against torch on the CPU: the head backward, the linear activation
backward from a saved output, the review bag and the additive attention (through oracle.ref_cpu.additive_attention) against
autograd, the one-step Adam against clip_grad_norm_ + torch.optim.Adam, all in float64 to 1e-12 relative.  Then the bound formulas on an f32 CPU computation of the same ops: the reference alone must stay inside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_refs as R

RTOL = 1e-12


def _close(name, a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert float((a - b).abs().max()) <= RTOL * max(scale, 1e-300), name


# ------------------------------------------------------------------------------------------------------------------ nn.Linear
@pytest.mark.parametrize("N,IN,OUT,act,with_mul", [(1, 1, 1, 0, False), (33, 65, 64, 1, True), (65, 193, 33, 2, True),
                                                   (130, 129, 70, 2, False), (64, 97, 65, 1, False)])
def test_linear_reference_matches_autograd(N, IN, OUT, act, with_mul):
    g = torch.Generator().manual_seed(N * 1000 + IN)
    x, W, b = torch.randn(N, IN, generator=g), torch.randn(OUT, IN, generator=g) / np.sqrt(IN), torch.randn(OUT, generator=g) * 0.1
    mul = (torch.rand(N, OUT, generator=g) > 0.5).float() * 2 if with_mul else None
    d_y = torch.randn(N, OUT, generator=g)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, W, b)]
    pre = F.linear(*leaves)
    y = torch.relu(pre) if act == 1 else torch.tanh(pre) if act == 2 else pre
    if mul is not None:
        y = y * mul.double()
    (y * d_y.double()).sum().backward()
    rpre, bpre, ry, by = R.linear_fwd(x, W, b, act, mul)
    _close("pre", rpre, pre.detach())
    _close("y", ry, y.detach())
    grads = R.linear_bwd(x, W, y.detach(), d_y, act, mul)
    for k, leaf in (("d_x", leaves[0]), ("dW", leaves[1]), ("db", leaves[2])):
        _close(k, grads[k][0], leaf.grad)
    # the bounds hold for an f32 CPU computation; its backward starts from ITS saved output, as the kernels' does
    pre32 = F.linear(x, W, b)
    y32 = torch.relu(pre32) if act == 1 else torch.tanh(pre32) if act == 2 else pre32
    if mul is not None:
        y32 = y32 * mul
    R.check("host-linear", "pre", pre32, rpre, bpre)
    R.check("host-linear", "y", y32, ry, by)
    g64, _ = R.linear_act_bwd(y32, d_y, act, mul)
    g32 = g64.float()                                    # one rounding of g: inside the 4 of (n + 4)
    got = {"dW": g32.t() @ x, "db": g32.sum(0), "d_x": g32 @ W}
    for k, (val, ab, n) in R.linear_bwd(x, W, y32, d_y, act, mul).items():
        R.check("host-linear", k, got[k], val, R.bound_of(n, ab))


# ---------------------------------------------------------------------------------------------------------------- rating head
def _head_inputs(B, H, K, U, I, seed, with_drop):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    P = dict(Wu=r(H, K) * 0.1, bu=r(K) * 0.1, Eu=r(U, K) * 0.1, Wi=r(H, K) * 0.1, bi=r(K) * 0.1, Ei=r(I, K) * 0.1, h=r(K) * 0.3,
             g=r(1), ub=r(U) * 0.1, ib=r(I) * 0.1)
    uf, itf = r(B, H) * 0.3, r(B, H) * 0.3
    uid, iid = torch.randint(0, U, (B,), generator=g), torch.randint(0, I, (B,), generator=g)
    drop = (torch.rand(B, K, generator=g) > 0.5).float() * 2 if with_drop else None
    return P, uf, itf, uid, iid, drop, r(B)


@pytest.mark.parametrize("B,H,K,pads,with_drop", [(1, 1, 1, (0, 3), False), (9, 5, 33, (0, 3), True), (65, 29, 260, (5, 0), True),
                                                  (129, 61, 4, (99, -1), False)])
def test_head_reference_matches_autograd(B, H, K, pads, with_drop):
    U, I = 11, 13
    P, uf, itf, uid, iid, drop, d_pred = _head_inputs(B, H, K, U, I, B * 100 + K, with_drop)
    pad_u, pad_i = pads
    L = {k: t.double().clone().requires_grad_(True) for k, t in dict(P, uf=uf, itf=itf).items()}
    pu, pi = (pad_u if 0 <= pad_u < U else None), (pad_i if 0 <= pad_i < I else None)
    ul = L["uf"] @ L["Wu"] + L["bu"] + F.embedding(uid, L["Eu"], padding_idx=pu)
    il = L["itf"] @ L["Wi"] + L["bi"] + F.embedding(iid, L["Ei"], padding_idx=pi)
    z = torch.relu(ul * il)
    if drop is not None:
        z = z * drop.double()
    pred = z @ L["h"] + F.embedding(uid, L["ub"].unsqueeze(1), padding_idx=pu).view(-1) + \
        F.embedding(iid, L["ib"].unsqueeze(1), padding_idx=pi).view(-1) + L["g"]
    (pred * d_pred.double()).sum().backward()
    rul, bul = R.head_latent(uf, uid, P["Wu"], P["bu"], P["Eu"])
    ril, bil = R.head_latent(itf, iid, P["Wi"], P["bi"], P["Ei"])
    _close("ul", rul, ul.detach())
    _close("il", ril, il.detach())
    rpred, bpred = R.head_pred(rul, ril, uid, iid, P["h"], P["g"], P["ub"], P["ib"], drop)
    _close("pred", rpred, pred.detach())
    grads = R.head_bwd(uf, itf, uid, iid, P, rul, ril, drop, d_pred, pad_u, pad_i)
    names = {"dWu": "Wu", "dbu": "bu", "dEu": "Eu", "dWi": "Wi", "dbi": "bi", "dEi": "Ei", "dh": "h", "dg": "g", "dub": "ub",
             "dib": "ib", "d_ufeat": "uf", "d_ifeat": "itf"}
    assert set(grads) == set(names)
    for k, leaf in names.items():
        _close(k, grads[k][0], L[leaf].grad)
    # the bounds hold for an f32 CPU computation from ITS saved latents
    ul32 = uf @ P["Wu"] + P["bu"] + P["Eu"][uid]
    il32 = itf @ P["Wi"] + P["bi"] + P["Ei"][iid]
    R.check("host-head", "ul", ul32, rul, bul)
    R.check("host-head", "il", il32, ril, bil)
    z32 = torch.relu(ul32 * il32) * (drop if drop is not None else 1.0)
    pred32 = z32 @ P["h"] + P["ub"][uid] + P["ib"][iid] + P["g"]
    r2, b2 = R.head_pred(ul32, il32, uid, iid, P["h"], P["g"], P["ub"], P["ib"], drop)
    R.check("host-head", "pred", pred32, r2, b2)
    dz32 = (ul32 * il32 > 0).float() * d_pred.unsqueeze(1) * P["h"].unsqueeze(0) * (drop if drop is not None else 1.0)
    dul32, dil32 = dz32 * il32, dz32 * ul32
    got = {"dWu": uf.t() @ dul32, "dbu": dul32.sum(0), "dWi": itf.t() @ dil32, "dbi": dil32.sum(0),
           "dh": (z32 * d_pred.unsqueeze(1)).sum(0), "dg": d_pred.sum().reshape(1), "d_ufeat": dul32 @ P["Wu"].t(),
           "d_ifeat": dil32 @ P["Wi"].t(),
           "dEu": torch.zeros(U, K).index_add_(0, uid, dul32 * (uid != pad_u).float().unsqueeze(1)),
           "dEi": torch.zeros(I, K).index_add_(0, iid, dil32 * (iid != pad_i).float().unsqueeze(1)),
           "dub": torch.zeros(U).index_add_(0, uid, d_pred * (uid != pad_u).float()),
           "dib": torch.zeros(I).index_add_(0, iid, d_pred * (iid != pad_i).float())}
    for k, (val, ab, n) in R.head_bwd(uf, itf, uid, iid, P, ul32, il32, drop, d_pred, pad_u, pad_i).items():
        R.check("host-head", k, got[k], val, R.bound_of(n, ab))


# ----------------------------------------------------------------------------------------------------------------- review bag
def _bag_cases():
    import test_review_bag_edges_gpu as G
    return G


@pytest.mark.parametrize("name", list(_bag_cases().CASES))
def test_review_bag_reference_matches_autograd(name):
    """Every case of tests/test_review_bag_edges_gpu.py: the restatement against autograd, then its bounds on an f32 evaluation."""
    table, ids, mask, drop, d_out, pad = _bag_cases().inputs(name)
    n_rev, T = ids.shape
    leaf = table.double().clone().requires_grad_(True)
    m = torch.ones(n_rev, T, dtype=torch.float64) if mask is None else mask.double()
    x = F.embedding(ids, leaf, padding_idx=pad) * m.unsqueeze(2)
    out = x.sum(1) / (m.sum(1, keepdim=True) + 1e-8) * (1.0 if drop is None else drop.double())
    (out * d_out.double()).sum().backward()
    ref = R.review_bag(table, ids, mask, drop, d_out, pad)
    _close("out", ref["out"][0], out.detach())
    _close("dtable", ref["dtable"][0], leaf.grad)
    # f32, operation by operation as the kernels: inv_len once per review, the sums in torch's order
    m32 = m.float()
    inv32 = 1.0 / (m32.sum(1) + np.float32(1e-8))
    dr32 = torch.ones(n_rev, table.shape[1]) if drop is None else drop
    out32 = (table[ids] * m32.unsqueeze(2)).sum(1) * inv32.unsqueeze(1) * dr32
    live = m32 if pad is None else m32 * (ids != pad).float()
    g32 = (d_out * inv32.unsqueeze(1) * dr32).repeat_interleave(T, 0) * live.reshape(-1, 1)
    dt32 = torch.zeros_like(table).index_add_(0, ids.reshape(-1), g32)
    assert out32.dtype == dt32.dtype == torch.float32
    for k, got in (("out", out32), ("dtable", dt32)):
        R.check("host-bag", f"{name} {k}", got, ref[k][0], R.bound_of(ref[k][2], ref[k][1]))


# --------------------------------------------------------------------------------------------------------- additive attention
def _att_cases():
    import test_additive_attn_edges_gpu as G
    return G


def _additive_attention_f32(inp):
    """NodeDropout + AddictiveAttention and its backward in f32 on the CPU, operation by operation in the kernels' order: the
    softmax as max, exp, sum, one reciprocal, products; the backward from the saved f32 scores and t."""
    rev, mask, nd, Wp, bp, d_out = (inp[k] for k in ("rev", "mask", "node_drop", "Wp", "bp", "d_out"))
    wi = inp["wi"].reshape(-1)
    B, R_, H = rev.shape
    K = Wp.shape[0]
    m = torch.ones(B, R_, dtype=torch.bool) if mask is None else mask
    x = rev if nd is None else rev * nd.unsqueeze(2)
    t = torch.tanh(x @ Wp.t() + bp)
    lg = torch.where(m, t @ wi, torch.tensor(-1e8))
    e = torch.exp(lg - lg.max(1, keepdim=True).values)
    s = e * (1.0 / e.sum(1, keepdim=True))
    out = (s.unsqueeze(2) * x).sum(1)
    dsr = torch.einsum("bh,brh->br", d_out, x)
    dot = (s * dsr).sum(1, keepdim=True)
    dl = torch.where(m, s * (dsr - dot), torch.tensor(0.0))
    d_pre = dl.unsqueeze(2) * wi * (1.0 - t * t)
    d_rev = s.unsqueeze(2) * d_out.unsqueeze(1) + d_pre @ Wp
    if nd is not None:
        d_rev = d_rev * nd.unsqueeze(2)
    got = {"t": t, "scores": s, "out": out, "d_pre": d_pre, "d_wi": torch.einsum("br,brk->k", dl, t), "d_bp": d_pre.sum((0, 1)),
           "d_Wp": d_pre.reshape(B * R_, K).t() @ x.reshape(B * R_, H), "d_rev": d_rev}
    assert all(v.dtype == torch.float32 for v in got.values())
    return got


@pytest.mark.parametrize("name", list(_att_cases().CASES))
def test_additive_attention_reference_matches_autograd(name):
    """Every case of tests/test_additive_attn_edges_gpu.py: the restatement (its backward fed its own float64 scores and t)
    against float64 autograd through oracle.ref_cpu.additive_attention on node_drop * rev, forward and all five gradients; then
    its bounds on an f32 evaluation, whose backward starts from ITS saved scores and t, as the kernels' does."""
    from oracle import ref_cpu as O
    inp = _att_cases().inputs(name)
    B, R_, H = inp["rev"].shape
    m = torch.ones(B, R_, dtype=torch.bool) if inp["mask"] is None else inp["mask"]
    leaves = {k: inp[k].double().clone().requires_grad_(True) for k in ("rev", "Wp", "bp", "wi")}
    x = leaves["rev"] if inp["node_drop"] is None else leaves["rev"] * inp["node_drop"].double().unsqueeze(2)
    out, scores = O.additive_attention(x, m, leaves["Wp"], leaves["bp"], leaves["wi"])
    (out * inp["d_out"].double()).sum().backward()
    args = (inp["rev"], inp["mask"], inp["node_drop"], inp["Wp"], inp["bp"], inp["wi"], inp["d_out"])
    ref = R.additive_attention(*args)
    _close("out", ref["out"][0], out.detach())
    _close("scores", ref["scores"][0], scores.detach())
    for k, leaf in (("d_rev", "rev"), ("d_Wp", "Wp"), ("d_bp", "bp"), ("d_wi", "wi")):
        _close(k, ref[k][0], leaves[leaf].grad)
    # d_pre, the gradient of the pre-activation: autograd's through the same graph, cut at pre
    pre = (x.detach() @ leaves["Wp"].detach().t() + leaves["bp"].detach()).requires_grad_(True)
    lg = torch.tanh(pre) @ leaves["wi"].detach().reshape(-1)
    s = torch.softmax(torch.masked_fill(lg, ~m, -1e8), dim=1)
    ((s.unsqueeze(2) * x.detach()).sum(1) * inp["d_out"].double()).sum().backward()
    _close("d_pre", ref["d_pre"][0], pre.grad)
    got = _additive_attention_f32(inp)
    ref32 = R.additive_attention(*args, scores=got["scores"], t=got["t"])
    for k, v in got.items():
        R.check("host-additive-attn", f"{name} {k}", v, *ref32[k])


# ----------------------------------------------------------------------------------------------------------------- clip + Adam
@pytest.mark.parametrize("max_norm", [None, 1e9, 0.05])
def test_adam_reference_matches_torch(max_norm):
    lr, betas, eps = R.f32r(2e-3), (R.f32r(0.9), R.f32r(0.999)), R.f32r(1e-8)
    g = torch.Generator().manual_seed(5)
    sizes = [1, 5, 4097, 130]
    ps32 = [torch.randn(n, generator=g) for n in sizes]
    ps = [t.double().clone().requires_grad_(True) for t in ps32]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    m32, v32 = [torch.zeros(n) for n in sizes], [torch.zeros(n) for n in sizes]
    w1, w2 = np.float32(1) - np.float32(betas[0]), np.float32(1) - np.float32(betas[1])
    for t in (1, 2, 3):
        grads = [torch.randn(n, generator=g) * 0.1 for n in sizes]
        before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone() if t > 1 else torch.zeros_like(p),
                   opt.state[p]["exp_avg_sq"].clone() if t > 1 else torch.zeros_like(p)) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.double().clone()
        norm = R.grad_norm(grads)
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            assert abs(float(tn) - norm) <= RTOL * norm
        opt.step()
        coef = R.clip_coef(norm, max_norm)
        assert (coef == 1.0) == (max_norm != 0.05)
        for i, (p, gr, (p0, m0, v0)) in enumerate(zip(ps, grads, before)):
            ref = R.adam_step(p0, m0, v0, gr, coef, t, lr, betas, eps)
            _close("gc", ref["gc"][0], p.grad)
            _close("m", ref["m"][0], opt.state[p]["exp_avg"])
            _close("v", ref["v"][0], opt.state[p]["exp_avg_sq"])
            _close("p", ref["p"][0], p.detach())
            # the bounds on an f32 computation of the same step from f32 state, operation by operation as the kernel's
            ref32 = R.adam_step(ps32[i], m32[i], v32[i], gr, coef, t, lr, betas, eps)
            c32 = torch.tensor(coef, dtype=torch.float32)
            gc = gr * c32
            m32[i] = m32[i] + w1 * (gc - m32[i])
            v32[i] = np.float32(betas[1]) * v32[i] + (w2 * gc) * gc
            s32 = np.float32(lr) / np.float32(1.0 - betas[0] ** t)
            c2 = np.float32(np.sqrt(1.0 - betas[1] ** t))
            ps32[i] = ps32[i] - (s32 * m32[i]) / (v32[i].sqrt() / c2 + np.float32(eps))
            for k, got in (("gc", gc), ("m", m32[i]), ("v", v32[i]), ("p", ps32[i])):
                assert got.dtype == torch.float32
                R.check("host-adam", k, got, *ref32[k])


def test_clip_coefficient_of_a_non_finite_norm():
    """clip_grad_norm_ keeps a NaN coefficient (torch.clamp(nan, max=1) is NaN) and turns an infinite norm into coefficient 0."""
    for bad, want_nan in ((float("nan"), True), (float("inf"), False)):
        p = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        p.grad = torch.tensor([1.0, bad, 2.0], dtype=torch.float64)
        norm = R.grad_norm([p.grad])
        torch.nn.utils.clip_grad_norm_([p], 0.05)
        coef = R.clip_coef(norm, 0.05)
        if want_nan:
            assert coef != coef and bool(torch.isnan(p.grad).all())
        else:
            assert coef == 0.0 and float(p.grad[0]) == 0.0 and float(p.grad[2]) == 0.0 and bool(torch.isnan(p.grad[1]))
    assert bool(torch.isnan(torch.relu(torch.tensor(float("nan")))))
