"""Float64 restatements behind the D-ATT explanation tests (tests/test_datt_explain_host.py, test_datt_saliency_edges_gpu.py,
test_datt_attention_gpu.py), in the convention of tests/edge_refs.py: every value comes with `Abs`, the same expression on
magnitudes, and a term count n where the bound (n + 4) * 2^-24 * Abs needs one.

  saliency(...)    the closed form of rbr_datt_saliency (include/rbr_hip.h).  feat, argmax and the gates are INPUTS, as they are
                   for the kernel, so a near-tie of the max-pool can never flip a comparison.
  datt_pair(...)   the whole eval-mode pair score of D-ATT in float64, explained by torch autograd on the embedded rows, with
                   the max-pool margins the GPU comparison asks for as a precondition.

Term counts of saliency (D = row width, cl[t] / cg[t] = taps of the local / global banks landing on position t):
  d_gate_l[t]   n = D * cl[t]: each tap is a D-long dot product; the + 4 covers g = d_feat * act'(feat) and the product.
  fixed[t]      n = D * (cl[t] + cg[t]) + 3: both sums, a gate multiply on each and the final add.
  d_gate_g      n = D * sum_t cg[t] + L: every raw_g[t], then L of them added.
  through[t]    n = max(D * max_s cl[s], D * sum_t cg[t] + L) + D + win + 8 with s over the local window around t: a term is
                dpre * <x[t], w[:, j]> -- the d_gate behind dpre with its own count, three roundings for
                d_gate * gate * (1 - gate), the D-long dot product, the product -- and win + 1 of them are added; every term is
                weighed by its own magnitude in Abs, so the largest count bounds them all.
"""
import torch
import torch.nn.functional as F

from edge_refs import f64


def _act_grad(feat, d, tanh):
    if tanh:
        return d * (1 - feat * feat), d.abs() * (1 + feat * feat)
    on = (feat > 0).double()
    return d * on, d.abs() * on


def saliency(table, ids, gate_l, gate_g, ws, split, feat, argmax, d_feat, w_l, w_g, valid=True, tanh=True):
    """{name: (value, Abs, n)} in float64 for fixed / through / d_gate_l [n_docs, L] and d_gate_g [n_docs].
    gate_l [n_docs, L], gate_g [n_docs]; ws: the conv banks, the first `split` under gate_l; w_l [1, D, win], w_g [1, D, L].
    A token id outside the table counts as a zero row."""
    table, gl, gg, feat, d = f64(table), f64(gate_l), f64(gate_g), f64(feat), f64(d_feat)
    w_l, w_g = f64(w_l)[0], f64(w_g)[0]                                   # [D, win], [D, L]
    ids, argmax = ids.cpu().long(), argmax.cpu().long()
    n_docs, L = ids.shape
    V, D = table.shape
    win = w_l.shape[1]
    ok = ((ids >= 0) & (ids < V)).double().unsqueeze(-1)
    x = table[ids.clamp(0, V - 1)] * ok                                   # [n_docs, L, D]
    g, ga = _act_grad(feat, d, tanh)
    raw = [torch.zeros(n_docs, L, dtype=torch.float64) for _ in range(2)]
    rab = [torch.zeros(n_docs, L, dtype=torch.float64) for _ in range(2)]
    cnt = [torch.zeros(n_docs, L, dtype=torch.float64) for _ in range(2)]
    c0 = 0
    for b, w in enumerate(ws):
        w = f64(w)
        ch, _, kz = w.shape
        which = 0 if b < split else 1
        p = argmax[:, c0:c0 + ch]
        in_pool = (p >= 0) & (p < (L - kz + 1 if valid else L))
        for j in range(kz):
            t = p + j - (0 if valid else (kz - 1) // 2)
            tc = t.clamp(0, L - 1)
            rows = x.gather(1, tc.unsqueeze(-1).expand(-1, -1, D))       # [n_docs, ch, D]
            wj = w[:, :, j].unsqueeze(0)
            coef = (in_pool & (t >= 0) & (t < L)).double()
            raw[which].scatter_add_(1, tc, g[:, c0:c0 + ch] * coef * (rows * wj).sum(-1))
            mag = ga[:, c0:c0 + ch] * coef * (rows.abs() * wj.abs()).sum(-1)
            rab[which].scatter_add_(1, tc, mag)
            cnt[which].scatter_add_(1, tc, (mag != 0).double())
        c0 += ch
    (raw_l, raw_g), (ab_l, ab_g), (cl, cg) = raw, rab, cnt
    ggc = gg.unsqueeze(1)
    fixed, fixed_ab = gl * raw_l + ggc * raw_g, gl.abs() * ab_l + ggc.abs() * ab_g
    dgg, dgg_ab, dgg_n = raw_g.sum(1), ab_g.sum(1), D * cg.sum(1) + L
    dpre_l, dpre_l_ab = raw_l * gl * (1 - gl), ab_l * gl.abs() * (1 - gl).abs()
    dpre_g, dpre_g_ab = dgg * gg * (1 - gg), dgg_ab * gg.abs() * (1 - gg).abs()
    through = dpre_g.unsqueeze(1) * (x * w_g.t().unsqueeze(0)).sum(-1)
    through_ab = dpre_g_ab.unsqueeze(1) * (x.abs() * w_g.t().abs().unsqueeze(0)).sum(-1)
    n_win = torch.zeros(n_docs, L, dtype=torch.float64)
    pos = torch.arange(L)
    for j in range(win):
        s = pos - j + (win - 1) // 2
        live = ((s >= 0) & (s < L)).double().unsqueeze(0)
        sc = s.clamp(0, L - 1)
        through = through + live * dpre_l[:, sc] * (x * w_l[:, j]).sum(-1)
        through_ab = through_ab + live * dpre_l_ab[:, sc] * (x.abs() * w_l[:, j].abs()).sum(-1)
        n_win = torch.maximum(n_win, live * D * cl[:, sc])
    through_n = torch.maximum(n_win, dgg_n.unsqueeze(1)) + D + win + 8
    return {"fixed": (fixed, fixed_ab, D * (cl + cg) + 3), "through": (through, through_ab, through_n),
            "d_gate_l": (raw_l, ab_l, D * cl), "d_gate_g": (dgg, dgg_ab, dgg_n)}


TIE = 1e-12      # gaps up to TIE * (1 + |best|) are exact ties: float64 rounding of equal sums (<= 400 terms of 2^-53 each)


def _bad_margins(pre, docs, kz, rel=1e-4):
    """Channels of pre [n, C, P] ('valid' conv of width kz over docs [n, L]) whose best window holds a non-padding token and leads
    the runner-up by more than an exact tie but less than rel * (1 + |best|).  An exact tie is harmless (both sides take the
    first argmax of identical windows); the float64 conv may give identical windows values that differ in their last bits,
    depending on the host's conv routine, so a gap within TIE -- eight orders of magnitude below the band -- counts as one.
    Windows of pure padding are zero rows and exempt."""
    if pre.shape[-1] < 2:
        return 0
    top = torch.topk(pre, 2, dim=-1)
    best, second, p = top.values[..., 0], top.values[..., 1], top.indices[..., 0]
    live = torch.zeros_like(best, dtype=torch.bool)
    for j in range(kz):
        live |= (docs != 0).gather(1, (p + j).clamp(0, docs.shape[1] - 1))
    gap, scale = best - second, 1 + best.abs()
    return int((live & (gap > TIE * scale) & (gap < rel * scale)).sum())


def _tower(p, side, docs):
    """One tower in float64 under autograd: dict of the leaf rows x, both gates, feat, argmax, the conv banks and bad margins."""
    table = p["word_embeddings.embedding.weight"]
    x = table[docs].detach().requires_grad_(True)                        # [n, L, E]
    xt = x.transpose(1, 2)
    lo, gl = f"{side}_local_atten", f"{side}_global_atten"
    w_l, w_g = p[f"{lo}.attn.0.weight"], p[f"{gl}.attn.0.weight"]
    gate_l = torch.sigmoid(F.conv1d(xt, w_l, p[f"{lo}.attn.0.bias"], padding=(w_l.shape[2] - 1) // 2))     # [n, 1, L]
    gate_g = torch.sigmoid(F.conv1d(xt, w_g, p[f"{gl}.attn.0.bias"]))                                      # [n, 1, 1]
    gate_l.retain_grad(); gate_g.retain_grad()
    names = [f"{lo}.conv.0", f"{gl}.conv1.0", f"{gl}.conv2.0", f"{gl}.conv3.0"]
    ws = [p[f"{n}.weight"] for n in names]
    feats, idxs, bad = [], [], 0
    for b, n in enumerate(names):
        pre = F.conv1d(xt * (gate_l if b == 0 else gate_g), ws[b], p[f"{n}.bias"])
        f, i = F.max_pool1d(torch.tanh(pre), pre.shape[-1], return_indices=True)
        feats.append(f.squeeze(-1)); idxs.append(i.squeeze(-1))
        bad += _bad_margins(pre.detach(), docs, ws[b].shape[2])
    feat = torch.cat(feats, 1)
    feat.retain_grad()
    return dict(x=x, gate_l=gate_l, gate_g=gate_g, feat=feat, argmax=torch.cat(idxs, 1).to(torch.int32), ws=ws, w_l=w_l, w_g=w_g,
                bad=bad, k=ws[0].shape[0])


def datt_pair(sd, u_docs, i_docs):
    """D-ATT's eval-mode score of the pairs (u_docs[b], i_docs[b]) (reference models/dual_att/dual_att.py:45-58) and its
    explanation by autograd on the embedded rows.  Dict of score [B], bad_margins, and per side s in (user, item): s_tokens
    [B, L] = <d score / d x[t], x[t]>, s_tokens_fixed [B, L] (the same with the gates held constant), s_local_gate [B, L], s_global_gate [B], s_d_gate_l [B, L], s_d_gate_g [B], s_local_text /
    s_global_text [B] = <d score / d feat, feat> over the local / global channels, and the closed form's inputs s_feat, s_argmax,
    s_d_feat [B, C], s_ws, s_w_l, s_w_g."""
    p = {k: f64(v) for k, v in sd.items()}
    u_docs, i_docs = u_docs.cpu().long(), i_docs.cpu().long()
    towers = {"user": _tower(p, "u", u_docs), "item": _tower(p, "i", i_docs)}

    def fc(feat):
        return F.relu(feat @ p["fc.0.weight"].t() + p["fc.0.bias"]) @ p["fc.3.weight"].t() + p["fc.3.bias"]

    score = (fc(towers["user"]["feat"]) * fc(towers["item"]["feat"])).sum(1)
    score.sum().backward(retain_graph=True)
    out = dict(score=score.detach(), bad_margins=towers["user"]["bad"] + towers["item"]["bad"])
    for s, t in towers.items():
        text = t["feat"].grad * t["feat"].detach()
        # the share that runs through the gates: the gates' own gradients, sent on to the rows
        # (copies: a retained gradient goes on accumulating in the second pass)
        d_gl, d_gg = t["gate_l"].grad.clone(), t["gate_g"].grad.clone()
        (gx,) = torch.autograd.grad((t["gate_l"] * d_gl).sum() + (t["gate_g"] * d_gg).sum(), t["x"])
        tokens = (t["x"].grad * t["x"].detach()).sum(-1)
        out.update({f"{s}_tokens": tokens, f"{s}_tokens_fixed": tokens - (gx * t["x"].detach()).sum(-1), f"{s}_local_gate": t["gate_l"].detach()[:, 0],
                    f"{s}_global_gate": t["gate_g"].detach()[:, 0, 0], f"{s}_d_gate_l": d_gl[:, 0],
                    f"{s}_d_gate_g": d_gg[:, 0, 0], f"{s}_local_text": text[:, :t["k"]].sum(1),
                    f"{s}_global_text": text[:, t["k"]:].sum(1), f"{s}_feat": t["feat"].detach(), f"{s}_argmax": t["argmax"],
                    f"{s}_d_feat": t["feat"].grad, f"{s}_ws": t["ws"], f"{s}_w_l": t["w_l"], f"{s}_w_g": t["w_g"]})
    return out
