"""Float64 restatements behind the explanation tests (tests/test_explain_host.py, test_textcnn_saliency_gpu.py,
test_explain_gpu.py), in the convention of tests/edge_refs.py: every value comes with `Abs`, the same expression on magnitudes.

  saliency(...)            the closed form of rbr_textcnn_saliency (include/rbr_hip.h).  feat and argmax are INPUTS, as they are
                           for the kernel, so a near-tie of the max-pool can never flip a comparison.
  autograd_saliency(...)   gradient x input of embedding -> mask -> gate -> conv1d -> act -> max_pool1d by torch autograd.
  deepconn_pair / narre_pair   the whole pair score of the two models in float64, explained by autograd (NARRE: attention
                           detached), with the max-pool margins the GPU comparison asks for as a precondition.
"""
import torch
import torch.nn.functional as F

from edge_refs import f64


def saliency(table, ids, mask, gate, ws, feat, argmax, d_feat, valid=False, tanh=False, counts=False):
    """(sal, Abs[, count]) [n_docs, L] in float64; count = number of (channel, tap) terms of non-zero magnitude landing on the
    element (an f32 result has D * count terms behind it)."""
    table, gate, feat, d = f64(table), f64(gate), f64(feat), f64(d_feat)
    ids, argmax = ids.cpu().long(), argmax.cpu().long()
    n_docs, L = ids.shape
    sal, ab, cnt = (torch.zeros(n_docs, L, dtype=torch.float64) for _ in range(3))
    m = torch.ones(n_docs, L, dtype=torch.float64) if mask is None else mask.cpu().double()
    gt = torch.ones(n_docs, L, dtype=torch.float64) if gate is None else gate
    if tanh:
        g, ga = d * (1 - feat * feat), d.abs() * (1 + feat * feat)
    else:
        on = (feat > 0).double()
        g, ga = d * on, d.abs() * on
    c0 = 0
    for w in ws:
        w = f64(w)
        ch, _, kz = w.shape
        p = argmax[:, c0:c0 + ch]
        in_pool = (p >= 0) & (p < (L - kz + 1 if valid else L))
        for j in range(kz):
            t = p + j - (0 if valid else (kz - 1) // 2)
            tc = t.clamp(0, L - 1)
            rows = table[ids.gather(1, tc)]                                  # [n_docs, ch, D]
            wj = w[:, :, j].unsqueeze(0)
            coef = (in_pool & (t >= 0) & (t < L)).double() * m.gather(1, tc) * gt.gather(1, tc)
            sal.scatter_add_(1, tc, g[:, c0:c0 + ch] * coef * (rows * wj).sum(-1))
            mag = ga[:, c0:c0 + ch] * coef.abs()
            ab.scatter_add_(1, tc, mag * (rows.abs() * wj.abs()).sum(-1))
            cnt.scatter_add_(1, tc, (mag != 0).double())
        c0 += ch
    return (sal, ab, cnt) if counts else (sal, ab)


def _rows(table, ids, mask, gate):
    x = f64(table)[ids]
    if mask is not None:
        x = x.masked_fill(~mask.unsqueeze(-1), 0.0)
    if gate is not None:
        x = x * f64(gate).unsqueeze(-1)
    return x.detach().requires_grad_(True)


def _conv_pool(x, ws, bs, valid=False, tanh=False):
    """(feat [n, C], argmax [n, C], pre-activations [n, C, positions] per bank) of conv1d -> act -> max_pool1d over rows x."""
    feats, idxs, pres = [], [], []
    for w, b in zip(ws, bs):
        k = w.shape[2]
        pre = F.conv1d(x.transpose(1, 2), f64(w), f64(b), padding=0 if valid else (k - 1) // 2)
        y = torch.tanh(pre) if tanh else F.relu(pre)
        f, i = F.max_pool1d(y, y.shape[-1], return_indices=True)
        feats.append(f.squeeze(-1)); idxs.append(i.squeeze(-1)); pres.append(pre)
    return torch.cat(feats, 1), torch.cat(idxs, 1), pres


def autograd_saliency(table, ids, mask, gate, ws, bs, d_feat, valid=False, tanh=False):
    """(feat, argmax int32, sal) where sal[doc, t] = <d score / d x[doc, t, :], x[doc, t, :]>, score = sum(feat * d_feat)."""
    x = _rows(table, ids, mask, gate)
    feat, argmax, _ = _conv_pool(x, ws, bs, valid, tanh)
    (feat * f64(d_feat)).sum().backward()
    return feat.detach(), argmax.to(torch.int32), (x.grad * x.detach()).sum(-1)


def relu_completeness(feat, d_feat, bs):
    """sum over the channels with feat > 0 of d_feat * (feat - bias): what sum_t sal[doc, t] equals for ReLU."""
    feat, d = f64(feat), f64(d_feat)
    bias = torch.cat([f64(b) for b in bs]).unsqueeze(0)
    return ((feat > 0).double() * d * (feat - bias)).sum(1)


def margins_ok(pres, masks, kzs, rel=1e-4):
    """The precondition of the float64 comparison on the GPU: for every channel whose best pre-activation is positive and whose
    best window holds an unmasked token, that window beats every other position by at least rel * (1 + |best|).  Returns the
    number of channels that miss it (0 = the reference is safe to compare with)."""
    bad = 0
    L = masks.shape[1]
    for pre, kz in zip(pres, kzs):
        if pre.shape[-1] < 2:
            continue
        top = torch.topk(pre, 2, dim=-1)
        best, second, p = top.values[..., 0], top.values[..., 1], top.indices[..., 0]
        live = torch.zeros_like(best, dtype=torch.bool)
        for j in range(kz):
            t = p + j - (kz - 1) // 2
            live |= (t >= 0) & (t < L) & masks.gather(1, t.clamp(0, L - 1))
        bad += int(((best > 0) & live & (best - second < rel * (1 + best.abs()))).sum())
    return bad


def _head(p, fu, fi, u_ids, i_ids):
    ul = fu @ p["user_feat.W"] + p["user_feat.b"] + p["user_feat.ebd.weight"][u_ids]
    il = fi @ p["item_feat.W"] + p["item_feat.b"] + p["item_feat.ebd.weight"][i_ids]
    return (F.relu(ul * il) @ p["fm.h"]).view(-1) + p["fm.user_bias.weight"][u_ids].view(-1) + \
        p["fm.item_bias.weight"][i_ids].view(-1) + p["fm.g_bias"]


def _conv_of(p):
    ws, bs, i = [], [], 0
    while f"ngram.feature_layer.0.list_of_conv1d.{i}.weight" in p:
        ws.append(p[f"ngram.feature_layer.0.list_of_conv1d.{i}.weight"])
        bs.append(p[f"ngram.feature_layer.0.list_of_conv1d.{i}.bias"])
        i += 1
    return ws, bs


def deepconn_pair(sd, u_docs, u_masks, i_docs, i_masks, u_ids, i_ids):
    """DeepCoNN++'s eval-mode score of the pairs and its explanation by autograd: dict of score [B], user_tokens / item_tokens
    [B, L], user_text / item_text [B] (= <d score / d feat, feat>) and bad_margins (margins_ok over both towers)."""
    p = {k: f64(v) for k, v in sd.items()}
    ws, bs = _conv_of(p)
    table = p["word_embeddings.embedding.weight"]
    xu, xi = _rows(table, u_docs, u_masks, None), _rows(table, i_docs, i_masks, None)
    fu, _, pu = _conv_pool(xu, ws, bs)
    fi, _, pi = _conv_pool(xi, ws, bs)
    fu.retain_grad(); fi.retain_grad()
    score = _head(p, fu, fi, u_ids, i_ids)
    score.sum().backward()
    kzs = [w.shape[2] for w in ws]
    return dict(score=score.detach(), user_tokens=(xu.grad * xu.detach()).sum(-1), item_tokens=(xi.grad * xi.detach()).sum(-1),
                user_text=(fu.grad * fu.detach()).sum(1), item_text=(fi.grad * fi.detach()).sum(1),
                bad_margins=margins_ok(pu, u_masks, kzs) + margins_ok(pi, i_masks, kzs))


def narre_pair(sd, u_text, u_masks, i_text, i_masks, u_ids, i_ids, reuid, reiid):
    """NARRE's eval-mode score and its explanation by autograd with the attention weights DETACHED: the DeepCoNN++ fields
    (tokens [B, R, T]) plus user/item_review_weights [B, R] and user/item_reviews [B, R]."""
    p = {k: f64(v) for k, v in sd.items()}
    ws, bs = _conv_of(p)
    table = p["word_embeddings.embedding.weight"]
    B, R, T = u_text.shape
    kzs = [w.shape[2] for w in ws]

    def tower(text, masks, other, att):
        x = _rows(table, text.reshape(B * R, T), masks.reshape(B * R, T), None)
        f, _, pres = _conv_pool(x, ws, bs)
        f.retain_grad()
        fr = f.view(B, R, -1)
        e = p[f"{att}.ebd_vals.weight"][other]
        logit = F.relu(fr @ p[f"{att}.W_rv"] + e @ p[f"{att}.W_id"] + p[f"{att}.b_1"]) @ p[f"{att}.h"] + p[f"{att}.b_2"]
        ex = logit.exp()
        a = (ex / (ex.sum(1, keepdim=True) + 1e-8)).detach()
        return x, f, (a * fr).sum(1), a.view(B, R), margins_ok(pres, masks.reshape(B * R, T), kzs)

    xu, fu, pu, au, bu = tower(u_text, u_masks, reuid, "user_att")
    xi, fi, pi, ai, bi = tower(i_text, i_masks, reiid, "item_att")
    score = _head(p, pu, pi, u_ids, i_ids)
    score.sum().backward()
    ur, ir = (fu.grad * fu.detach()).sum(1).view(B, R), (fi.grad * fi.detach()).sum(1).view(B, R)
    return dict(score=score.detach(), user_tokens=(xu.grad * xu.detach()).sum(-1).view(B, R, T),
                item_tokens=(xi.grad * xi.detach()).sum(-1).view(B, R, T), user_text=ur.sum(1), item_text=ir.sum(1),
                user_review_weights=au, user_reviews=ur, item_review_weights=ai, item_reviews=ir, bad_margins=bu + bi)
