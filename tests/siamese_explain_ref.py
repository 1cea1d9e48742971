"""Float64 restatements behind SimpleSiamese's explanation (tests/test_siamese_explain_host.py,
test_siamese_saliency_edges_gpu.py, test_siamese_contributions_gpu.py), in the convention of tests/explain_ref.py and
tests/edge_refs.py: every value comes with `Abs`, the same expression on magnitudes (1 - x^2 becomes 1 + x^2, a difference
becomes a sum).

  saliency(...)            the closed form of rbr_siamese_saliency (include/rbr_hip.h).  y and a are INPUTS, as they are for the
                           kernel, so the forward pass's rounding never enters a comparison.
  autograd_saliency(...)   gradient x input of rows -> masked average -> (Linear + Tanh) -> AddictiveAttention by torch
                           autograd in float64, with and without the attention detached.
  siamese_pair(...)        the whole pair score of the model in float64, explained by autograd.
  saliency_f32(...)        the closed form again in f32 on the CPU, summed in ANOTHER order than the kernel's (BLAS products,
                           reversed rows): the host test holds it against the bound the GPU test uses.
  edge_cases()             the shapes and masks both of those tests run.

Term counts n of bound = (n + 4) * 2^-24 * Abs, per element, for E the row width, F the review vector's width, K the attention's
projection width, R the reviews of a side row (a fused multiply-add rounds once; adding an exact 0.0f rounds nothing):
  reviews   c_r is a sum of F products, times s_r:                                              n = F + 1
  fixed     gy = s_r * g (1) [, times 1 - x^2 (3), the F-term product with Wt], the E-term dot
            with the row, inv_r (the sum, the division) and the product with it (3):            n = E + 4 [+ F + 3]
  through   d logit_r = s_r * (c_r - cbar): c_r (F), cbar adds R terms of them (R), the
            difference and the product (2);  u = wi * (1 - tp^2): the pre-activation (F + 1
            terms of magnitude Abs(pre) <= 1, A PRECONDITION every case here meets -- tanh is
            1-Lipschitz and 2 |tp| / (1 + tp^2) <= 1, so its error carries over), tanhf itself
            (4), the square, the difference and the product (3);  q sums K of them (K);
            gy = d logit * q (1); then as for fixed:                     n = E + 2 F + K + R + 14 [+ F + 3]
An element with Abs == 0 has no terms and must be exactly 0."""
import torch

from edge_refs import f64


def _masks(ids, word_mask, rev_mask):
    n, R, T = ids.shape
    wm = torch.ones(n, R, T, dtype=torch.float64) if word_mask is None else word_mask.cpu().double()
    rm = torch.ones(n, R, dtype=torch.float64) if rev_mask is None else rev_mask.cpu().double()
    return wm, rm


def term_counts(E, F, K, R, has_wt):
    extra = F + 3 if has_wt else 0
    return {"reviews": F + 1, "fixed": E + 4 + extra, "through": E + 2 * F + K + R + 14 + extra}


def saliency(table, ids, word_mask, rev_mask, y, a, g, Wt, Wp, bp, wi):
    """{name: (value, Abs, n)} for fixed / through [n, R, T] and reviews [n, R] in float64, plus "pre_abs": the largest magnitude
    sum of an attention pre-activation (the precondition of the `through` count is pre_abs <= 1)."""
    table, y, a, g, Wt, Wp, bp, wi = (f64(t) for t in (table, y, a, g, Wt, Wp, bp, wi))
    ids = ids.cpu().long()
    n, R, T = ids.shape
    a, wi = a.reshape(n, R), wi.reshape(-1)
    wm, rm = _masks(ids, word_mask, rev_mask)
    E, F, K = table.shape[1], y.shape[2], Wp.shape[0]
    gx = g.unsqueeze(1)
    c, ac = (gx * y).sum(-1), (gx.abs() * y.abs()).sum(-1)
    reviews, areviews = a * c, a.abs() * ac
    cbar, acbar = (a * c).sum(1, keepdim=True), (a.abs() * ac).sum(1, keepdim=True)
    dl, adl = rm * a * (c - cbar), rm * a.abs() * (ac + acbar)
    pre, apre = y @ Wp.t() + bp, y.abs() @ Wp.abs().t() + bp.abs()
    tp = torch.tanh(pre)
    u, au = wi * (1 - tp * tp), wi.abs() * (1 + tp * tp)
    q, aq = u @ Wp, au @ Wp.abs()
    gyf, agyf = a.unsqueeze(-1) * gx, a.abs().unsqueeze(-1) * gx.abs()
    gyt, agyt = dl.unsqueeze(-1) * q, adl.unsqueeze(-1) * aq
    if Wt is not None:
        d, ad = 1 - y * y, 1 + y * y
        gmf, agmf = (gyf * d) @ Wt, (agyf * ad) @ Wt.abs()
        gmt, agmt = (gyt * d) @ Wt, (agyt * ad) @ Wt.abs()
    else:
        gmf, agmf, gmt, agmt = gyf, agyf, gyt, agyt
    inv = (1.0 / (wm.sum(-1) + 1e-8)).unsqueeze(-1)
    rows = table[ids]                                                         # [n, R, T, E]
    scale = wm * inv
    out = {"reviews": (reviews, areviews)}
    for name, gm, agm in (("fixed", gmf, agmf), ("through", gmt, agmt)):
        out[name] = (scale * (rows * gm.unsqueeze(2)).sum(-1), scale * (rows.abs() * agm.unsqueeze(2)).sum(-1))
    counts = term_counts(E, F, K, R, Wt is not None)
    res = {k: (v, ab, counts[k]) for k, (v, ab) in out.items()}
    res["pre_abs"] = float(apre.max())
    return res


def _tower(x, wm, rm, Wt, bt, Wp, bp, wi, detach):
    """rows x [n, R, T, E] (already masked) -> (y [n, R, F], a [n, R], pooled [n, F]); detach: the attention weights are constants."""
    avg = x.sum(2) / (wm.sum(-1, keepdim=True) + 1e-8)
    y = torch.tanh(avg @ Wt.t() + bt) if Wt is not None else avg
    logit = torch.tanh(y @ Wp.t() + bp) @ wi.reshape(-1)
    a = torch.softmax(logit.masked_fill(rm == 0, -1e8), dim=1)
    if detach:
        a = a.detach()
    return y, a, (a.unsqueeze(-1) * y).sum(1)


def autograd_saliency(table, ids, word_mask, rev_mask, g, Wt, bt, Wp, bp, wi):
    """(y, a, tokens, tokens_fixed): tokens[b, r, t] = <d score / d x[b, r, t, :], x[b, r, t, :]> for score = sum(pooled * g) over
    the float64 tower, tokens_fixed the same with the attention weights detached."""
    table, g, Wt, bt, Wp, bp, wi = (f64(t) for t in (table, g, Wt, bt, Wp, bp, wi))
    ids = ids.cpu().long()
    wm, rm = _masks(ids, word_mask, rev_mask)
    res = []
    for detach in (False, True):
        x = (table[ids] * wm.unsqueeze(-1)).detach().requires_grad_(True)
        y, a, pooled = _tower(x, wm, rm, Wt, bt, Wp, bp, wi, detach)
        (pooled * g).sum().backward()
        res.append((x.grad * x.detach()).sum(-1))
    return y.detach(), a.detach(), res[0], res[1]


def siamese_pair(sd, u_revs, i_revs, u_ids, i_ids):
    """SimpleSiamese's eval-mode score of the pairs in float64 and its explanation by autograd, masks derived as
    Recommender._encode derives them (token != 0; a review counts when it holds any token): dict of score [B] and, per side,
    tokens / tokens_fixed [B, R, T], text [B], review_weights / reviews [B, R]."""
    p = {k: f64(v) for k, v in sd.items()}
    table = p["word_embedding.embedding.weight"]
    Wt, bt = p.get("latent_transform_layer.0.weight"), p.get("latent_transform_layer.0.bias")
    Wp, bp = p["review_att_layer.proj_layer.0.weight"], p["review_att_layer.proj_layer.0.bias"]
    wi = p["review_att_layer.inner_product.weight"]
    out = {}
    for detach in (False, True):
        side = {}
        for name, revs in (("user", u_revs), ("item", i_revs)):
            revs = revs.cpu().long()
            wm = (revs != 0).double()
            rm = (wm.sum(-1) > 0).double()
            x = (table[revs] * wm.unsqueeze(-1)).detach().requires_grad_(True)
            y, a, pooled = _tower(x, wm, rm, Wt, bt, Wp, bp, wi, detach)
            y.retain_grad()
            side[name] = (x, y, a, pooled)
        fu, fi = side["user"][3], side["item"][3]
        ul = fu @ p["user_last_feat_layer.W"] + p["user_last_feat_layer.b"] + p["user_last_feat_layer.ebd.weight"][u_ids]
        il = fi @ p["item_last_feat_layer.W"] + p["item_last_feat_layer.b"] + p["item_last_feat_layer.ebd.weight"][i_ids]
        score = (torch.relu(ul * il) @ p["fm.h"]).view(-1) + p["fm.g_bias"]
        if "fm.user_bias.weight" in p:
            score = score + p["fm.user_bias.weight"][u_ids].view(-1) + p["fm.item_bias.weight"][i_ids].view(-1)
        score.sum().backward()
        for name, (x, y, a, _) in side.items():
            tok = (x.grad * x.detach()).sum(-1)
            if detach:
                out[f"{name}_tokens_fixed"] = tok
                out[f"{name}_reviews"] = (y.grad * y.detach()).sum(-1)        # y.grad = a * g with a constant
                out[f"{name}_text"] = out[f"{name}_reviews"].sum(1)
            else:
                out[f"{name}_tokens"] = tok
                out[f"{name}_review_weights"] = a.detach()
        out["score"] = score.detach()
    return out


def saliency_f32(table, ids, word_mask, rev_mask, y, a, g, Wt, Wp, bp, wi):
    """The closed form in f32 on the CPU, in an order of summation that is not the kernel's: matrix products for the sums over
    F and K, the rows and the reviews taken in reverse."""
    f = lambda t: None if t is None else t.detach().cpu().float()                # noqa: E731
    table, y, a, g, Wt, Wp, bp, wi = (f(t) for t in (table, y, a, g, Wt, Wp, bp, wi))
    ids = ids.cpu().long()
    n, R, T = ids.shape
    a, wi = a.reshape(n, R), wi.reshape(-1)
    wm = torch.ones(n, R, T) if word_mask is None else word_mask.cpu().float()
    rm = torch.ones(n, R) if rev_mask is None else rev_mask.cpu().float()
    c = torch.bmm(y, g.unsqueeze(-1)).squeeze(-1)
    cbar = (a * c).flip(1).sum(1, keepdim=True)
    dl = rm * a * (c - cbar)
    tp = torch.tanh(y @ Wp.t() + bp)
    q = (wi * (1 - tp * tp)) @ Wp
    gyf, gyt = a.unsqueeze(-1) * g.unsqueeze(1), dl.unsqueeze(-1) * q
    if Wt is not None:
        d = 1 - y * y
        gyf, gyt = (gyf * d) @ Wt, (gyt * d) @ Wt
    inv = (1.0 / (wm.sum(-1) + 1e-8)).unsqueeze(-1)
    rows = table[ids].flip(-1)
    fixed = wm * inv * (rows * gyf.flip(-1).unsqueeze(2)).sum(-1)
    through = wm * inv * (rows * gyt.flip(-1).unsqueeze(2)).sum(-1)
    return {"fixed": fixed, "through": through, "reviews": a * c}


# ------------------------------------------------------------------------------------------------------------------ edge cases
def make_case(n, R, T, E, K, V, seed, F=None, masks="holes"):
    """Hand-made inputs of the op.  F None: no transform (F = E).  y lies in (-1, 1) as a tanh leaves it, a is a softmax over the
    reviews rev_mask keeps (uniform where it keeps none), and the attention's projection is small enough that the magnitude
    sum of every pre-activation stays below 1 (the precondition of the `through` bound) while wi spreads the logits.
    masks: "null" (no masks at all), "holes" (random word-mask holes, every review kept) or "edges": row 0 has a fully masked
    review between live ones (where R >= 3) and a kept review whose words are all masked, the LAST row keeps no review."""
    gen = torch.Generator().manual_seed(seed)
    has_wt = F is not None
    F = E if F is None else F
    c = dict(n=n, R=R, T=T, E=E, F=F, K=K, V=V)
    c["table"] = torch.randn(V, E, generator=gen)
    ids = torch.randint(0, V, (n, R, T), generator=gen)
    c["ids"] = ids
    c["y"] = torch.tanh(torch.randn(n, R, F, generator=gen))
    c["g"] = torch.randn(n, F, generator=gen)
    c["Wt"] = torch.randn(F, E, generator=gen) / E ** 0.5 if has_wt else None
    c["Wp"] = (torch.rand(K, F, generator=gen) - 0.5) * (1.6 / F)          # sum_f |Wp| |y| < 0.8
    c["bp"] = (torch.rand(K, generator=gen) - 0.5) * 0.2
    c["wi"] = torch.randn(1, K, generator=gen) * 3.0
    wm = rm = None
    if masks != "null":
        wm = torch.rand(n, R, T, generator=gen) < 0.7
        wm[:, :, 0] = True
        rm = torch.ones(n, R, dtype=torch.bool)
        if masks == "edges":
            if R >= 3:
                rm[0, 1], wm[0, 1] = False, False                            # a fully masked review between live ones
            wm[0, R - 1] = False                                             # a live review whose words are all masked
            rm[n - 1] = False                                                # a side row with every review masked
    live = (torch.ones(n, R, T, dtype=torch.bool) if wm is None else wm).view(-1).nonzero().view(-1)
    ids.view(-1)[live[0]], ids.view(-1)[live[-1]] = 0, V - 1               # the padding row and the table's last row, both on
    logit = torch.randn(n, R, generator=gen)                               # UNMASKED tokens: the gather reads them
    if rm is not None:
        logit = logit.masked_fill(~rm, -1e8)
    c["a"] = torch.softmax(logit, dim=1)
    c["word_mask"], c["rev_mask"] = wm, rm
    return c


OP_ARGS = ("table", "ids", "word_mask", "rev_mask", "y", "a", "g", "Wt", "Wp", "bp", "wi")


def edge_cases(stretch=64, flight=8):
    """name -> make_case arguments.  stretch / flight: the kernel's token tiles (a group of G lanes keeps `flight` rows in flight
    and a wave takes min(stretch, 64 / G * flight) tokens of a review at a time: 8 at G = 64, 16 at G = 32, `stretch` at G = 1)."""
    cases = {
        "degenerate": dict(n=1, R=1, T=1, E=1, K=1, V=1, masks="null"),
        "e3_scalar_rows": dict(n=2, R=2, T=9, E=3, K=1, V=10),
        "e4_one_lane_per_token": dict(n=2, R=2, T=9, E=4, K=33, V=10, F=5),
        "e260_second_round_of_lanes": dict(n=2, R=2, T=9, E=260, K=1, V=12),
        "e300_transform": dict(n=2, R=3, T=9, E=300, K=33, V=12, F=7, masks="edges"),
        "e300_plain_edges": dict(n=3, R=3, T=5, E=300, K=2, V=12, masks="edges"),
        "r1": dict(n=3, R=1, T=5, E=8, K=3, V=9, masks="edges"),
        "r2_null_masks": dict(n=2, R=2, T=5, E=8, K=3, V=9, F=6, masks="null"),
        "r64": dict(n=2, R=64, T=3, E=8, K=3, V=9, masks="edges"),
        "r64_transform": dict(n=2, R=64, T=3, E=12, K=2, V=9, F=5, masks="edges"),
    }
    for T in (1, flight - 1, flight, flight + 1, stretch + 1):                # G = 64: a tile is `flight` tokens
        cases[f"t{T}_e260"] = dict(n=2, R=2, T=T, E=260, K=2, V=12)
    for T in (2 * flight - 1, 2 * flight, 2 * flight + 1):                    # G = 32: two tokens side by side in a wave
        cases[f"t{T}_e128"] = dict(n=2, R=2, T=T, E=128, K=2, V=12)
    for T in (stretch - 1, stretch, stretch + 1):                             # G = 1: a tile is the whole stretch
        cases[f"t{T}_e4"] = dict(n=2, R=2, T=T, E=4, K=2, V=12, masks="edges")
    return cases
