"""functional.ahn_pair_explain (csrc/ahn_explain.hip) restated in float64 numpy, one pair at a time, with none of the package's
code.  The kernel reduces every gradient to a scalar on the fly; this restatement goes the long way round instead: the forward
and the VECTOR gradients dX, dXt, dKs, dKr of tests/ahn_attend_ref.py (attend_fwd_ref / attend_bwd_ref, driven by the FM's dz),
then their dots with the inputs -- so the kernel's scalar shortcuts are checked against an independent derivation.  The FM's
score and its two gradients are explicit loops.  The routing (js, jr) is computed -- lowest index on ties -- or passed in.
Reference of tests/test_ahn_explain_host.py, test_ahn_explain_edges_gpu.py and test_ahn_sentences_gpu.py."""
import numpy as np

import ahn_attend_ref as A

FIELDS = ("user_sentences", "user_sentences_fixed", "user_reviews", "user_text", "item_sentence_match", "item_review_match",
          "item_reviews", "item_text")


def _f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def explain_pair_ref(X, Xt, sent_mask, rev_mask, Ks, Kr, bt, ufm, ifm, VzT, vz2, lz, lin_b, Rp, beta, VqT, vq2, lq, js=None, jr=None):
    """One pair: X, Xt [NU, F], sent_mask [Ru, Su], rev_mask [Ru], Ks [NJ, F], Kr [Ri, F], bt [F], ufm, ifm [K + 2], VzT [K, F],
    vz2, lz [F], lin_b [1], Rp [Ri, F], beta [Ri], VqT [K, F], vq2, lq [F] -> dict of score, w [Ru, Su], v [Ru], js [NU], jr [Ru],
    the eight FIELDS, and the intermediates S [NU, NJ], T [Ru, Ri], s, t, p, z, dz, dq, q and ds, dt, e (the scalar chain's, for the sum
    identities).  js / jr given: the maxima are read at those rows."""
    X, Xt, Ks, Kr, bt, ufm, ifm, VzT, vz2, lz, Rp, beta, VqT, vq2, lq = (
        _f64(a) for a in (X, Xt, Ks, Kr, bt, ufm, ifm, VzT, vz2, lz, Rp, beta, VqT, vq2, lq))
    lin_b = float(_f64(lin_b).reshape(-1)[0])
    m, M = np.asarray(sent_mask, bool), np.asarray(rev_mask, bool)
    Ru, Su = m.shape
    K, F = VzT.shape
    Ri = Kr.shape[0]
    fwd = A.attend_fwd_ref(X[None], Xt[None], m[None], M[None], Ks[None], Kr[None], bt, 1,
                           js=None if js is None else np.asarray(js)[None], jr=None if jr is None else np.asarray(jr)[None])
    z, p, w, v = fwd["z"][0], fwd["p"][0], fwd["w"][0], fwd["v"][0]
    # ---- the FM, by loops: xv[k], the score, d score / d z
    xv = np.zeros(K)
    for k in range(K):
        acc = 0.0
        for f in range(F):
            acc += z[f] * VzT[k, f]
        xv[k] = acc + ufm[k] + ifm[k]
    sq = sum(xv[k] * xv[k] for k in range(K))
    zz = sum(z[f] * z[f] * vz2[f] for f in range(F))
    lin = sum(z[f] * lz[f] for f in range(F))
    score = 0.5 * (sq - zz - ufm[K] - ifm[K]) + lin + ufm[K + 1] + ifm[K + 1] + lin_b
    dz = np.zeros(F)
    for f in range(F):
        acc = 0.0
        for k in range(K):
            acc += xv[k] * VzT[k, f]
        dz[f] = acc - z[f] * vz2[f] + lz[f]
    # ---- the user side through the vector gradients
    g = A.attend_bwd_ref(X[None], Xt[None], m[None], M[None], Ks[None], Kr[None], fwd, dz[None], 1)
    dX, dXt, dKs, dKr = g["dX"][0], g["dXt"][0], g["dKs"][0], g["dKr"][0]
    out = dict(score=score, w=w, v=v, js=fwd["js"][0], jr=fwd["jr"][0], S=fwd["S"][0], T=fwd["T"][0], s=fwd["s"][0], t=fwd["t"][0],
               p=p, z=z, dz=dz, xv=xv)
    out["user_sentences"] = ((dX * X).sum(1) + (dXt * Xt).sum(1)).reshape(Ru, Su)
    fixed = np.zeros((Ru, Su))
    for r in range(Ru):
        held = np.where(p[r] > 0, v[r] * dz, 0.0)                      # d z / d a[r] with w and v held constant
        for k in range(Su):
            fixed[r, k] = w[r, k] * float(held @ Xt[r * Su + k])
    out["user_sentences_fixed"] = fixed
    out["user_reviews"] = v * (p @ dz)
    out["user_text"] = float(dz @ z)
    out["item_sentence_match"] = (dKs * Ks).sum(1)
    out["item_review_match"] = (dKr * Kr).sum(1)
    # ---- the item's own path: q = sum_i beta[i] r'[i], d score / d q by loops
    qv = np.zeros(F)
    for r in range(Ri):
        qv += beta[r] * Rp[r]
    dq = np.zeros(F)
    for f in range(F):
        acc = 0.0
        for k in range(K):
            acc += xv[k] * VqT[k, f]
        dq[f] = acc - qv[f] * vq2[f] + lq[f]
    out["item_reviews"] = beta * (Rp @ dq)
    out["item_text"] = float(dq @ qv)
    out["q"], out["dq"] = qv, dq
    # ---- ds of the scalar chain (rbr_ahn_pair_attend_bwd's formulas), for the sum identities of the host test
    dv = p @ dz
    dt = np.where(M, v * (dv - float(v @ dv)), 0.0)
    ds, es = np.zeros(Ru * Su), np.zeros(Ru * Su)
    for r in range(Ru):
        da = np.where(p[r] > 0, v[r] * dz + dt[r] * Kr[out["jr"][r]], 0.0)
        rows = np.arange(r * Su, (r + 1) * Su)
        e = Xt[rows] @ da
        ds[rows], es[rows] = np.where(m[r], w[r] * (e - float(w[r] @ e)), 0.0), e
    out["ds"], out["dt"], out["e"] = ds, dt, es
    return out


def make_head(B, P, Ri, F, K, seed):
    """Seeded float32 torch CPU tensors for B user rows and P item rows: the ids' FM rows ufm [B, K + 2], ifm [P, K + 2], the head
    VzT [K, F], vz2, lz [F], lin_b [1], and the item's own path Rp [P, Ri, F], beta [P, Ri] (positive, rows sum to 1), VqT [K, F],
    vq2, lq [F].  vz2 / vq2 are the column sums of the squares, as AHN.pair_head cuts them."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale          # noqa: E731
    VzT, VqT = rnd(K, F, scale=1.5 / F ** 0.5), rnd(K, F, scale=1.5 / F ** 0.5)
    return dict(ufm=rnd(B, K + 2, scale=0.5), ifm=rnd(P, K + 2, scale=0.5), VzT=VzT, vz2=(VzT * VzT).sum(0), lz=rnd(F, scale=0.3),
                lin_b=rnd(1), Rp=rnd(P, Ri, F), beta=torch.softmax(rnd(P, Ri, scale=2.0), dim=1), VqT=VqT, vq2=(VqT * VqT).sum(0),
                lq=rnd(F, scale=0.3))


def explain_ref(t, h, G, js=None, jr=None):
    """ahn_attend_ref.make_inputs' dict t (B users, P = G * B items; pair q reads user q % B and item q) and make_head's dict h
    -> list of explain_pair_ref's dicts, one per pair.  js [P, NU] / jr [P, Ru] given: the kernel's routing."""
    B = t["X"].shape[0]
    P = t["Ks"].shape[0]
    assert P == G * B
    m, M = t["sent_mask"].numpy(), t["rev_mask"].numpy()
    return [explain_pair_ref(t["X"][q % B], t["Xt"][q % B], m[q % B], M[q % B], t["Ks"][q], t["Kr"][q], t["bt"], h["ufm"][q % B],
                             h["ifm"][q], h["VzT"], h["vz2"], h["lz"], h["lin_b"], h["Rp"][q], h["beta"][q], h["VqT"], h["vq2"], h["lq"],
                             js=None if js is None else js[q], jr=None if jr is None else jr[q]) for q in range(P)]


def explain_torch(t, h, G, dev=None, attend=None):
    """The same numbers through a torch composition in the inputs' dtype on device `dev`: the user side's op (`attend`: a callable
    with attend_torch's signature and (z, w, v) result; default attend_torch itself), a torch FM over the hoisted rows,
    autograd.grad down to X, Xt, Ks, Kr of every pair -- the [P, rows, F] gradients the kernel never writes -- and row dots.
    Dict of score, w, v and the eight FIELDS, each [P, ...]."""
    import torch
    attend = attend or A.attend_torch
    mv = lambda x: x.to(dev) if dev is not None else x                                   # noqa: E731
    B, P = t["X"].shape[0], t["Ks"].shape[0]
    K = h["VzT"].shape[0]
    X, Xt = (mv(t[k]).repeat(G, 1, 1).requires_grad_(True) for k in ("X", "Xt"))          # a leaf per pair: per-pair gradients
    Ks, Kr = (mv(t[k]).clone().requires_grad_(True) for k in ("Ks", "Kr"))
    m, M = mv(t["sent_mask"]).repeat(G, 1, 1), mv(t["rev_mask"]).repeat(G, 1)
    H = {k: mv(x) for k, x in h.items()}
    z, w, v = attend(X, Xt, m, M, Ks, Kr, mv(t["bt"]), 1)
    ufm, ifm = H["ufm"].repeat(G, 1), H["ifm"]
    xv = z @ H["VzT"].t() + ufm[:, :K] + ifm[:, :K]
    score = 0.5 * ((xv * xv).sum(1) - (z * z) @ H["vz2"] - ufm[:, K] - ifm[:, K]) + z @ H["lz"] + ufm[:, K + 1] + ifm[:, K + 1] + H["lin_b"]
    dX, dXt, dKs, dKr, dz = torch.autograd.grad(score.sum(), [X, Xt, Ks, Kr, z])
    with torch.no_grad():
        Ru, Su = m.shape[1:]
        F = X.shape[2]
        p = torch.relu((w.unsqueeze(-1) * Xt.view(P, Ru, Su, F)).sum(2) + mv(t["bt"]))
        held = (p > 0) * v.unsqueeze(-1) * dz.unsqueeze(1)                                # [P, Ru, F]
        q = (H["beta"].unsqueeze(-1) * H["Rp"]).sum(1)
        dq = xv @ H["VqT"] - q * H["vq2"] + H["lq"]
        return dict(score=score.detach(), w=w.detach(), v=v.detach(),
                    user_sentences=((dX * X).sum(2) + (dXt * Xt).sum(2)).view(P, Ru, Su),
                    user_sentences_fixed=w * (held.unsqueeze(2) * Xt.view(P, Ru, Su, F)).sum(3),
                    user_reviews=v * (p * dz.unsqueeze(1)).sum(2), user_text=(dz * z).sum(1),
                    item_sentence_match=(dKs * Ks).sum(2), item_review_match=(dKr * Kr).sum(2),
                    item_reviews=H["beta"] * (H["Rp"] * dq.unsqueeze(1)).sum(2), item_text=(dq * q).sum(1))


def item_reviews_ref(p, Y, sent_mask):
    """The transformed reviews r' [Ri, F] of one item from its sentence vectors Y [Ri, Si, F] and a state_dict p, in float64:
    what ahn_pair_ref.item_state_ref makes Kr and the pooled q of (AHN.item_reviews)."""
    import ahn_pair_ref as R
    Ri, Si, F = Y.shape
    Y = _f64(Y)
    sm = np.asarray(sent_mask, bool).reshape(Ri, Si)
    sc = R._gated_scores(Y.reshape(Ri * Si, F), p, "unbalanced_sentence_aggregator.item_aggregator").reshape(Ri, Si)
    r = (R.masked_softmax(sc, sm)[:, :, None] * Y).sum(1)
    return np.maximum(r @ _f64(p["item_review_trans_layer.0.weight"]).T + _f64(p["item_review_trans_layer.0.bias"]), 0.0)
