"""functional.ahn_pair_attend (csrc/ahn_attend.hip) restated in float64 numpy over the grouped layout, forward and backward, as
plain loops with none of the package's code: G groups of B pairs, pair p = g * B + b reads user row b and item row p.  The
routing (js, jr: which item row attained each max) is computed -- lowest index on ties -- or passed in, so that a kernel's own
routing can be differentiated.  Reference of tests/test_ahn_attend_host.py, test_ahn_attend_edges_gpu.py and tools/bench_ahn_bpr.py's
input generator."""
import numpy as np

MASK_FILL = -1e8


def _f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def _softmax(scores, mask):
    s = np.where(mask, scores, MASK_FILL)
    e = np.exp(s - s.max())
    return e / e.sum()


def attend_fwd_ref(X, Xt, sent_mask, rev_mask, Ks, Kr, bt, G, js=None, jr=None):
    """X, Xt [B, NU, F], sent_mask [B, Ru, Su], rev_mask [B, Ru], Ks [G*B, NJ, F], Kr [G*B, Ri, F], bt [F] -> dict of z [P, F],
    w [P, Ru, Su], v [P, Ru], p [P, Ru, F], a [P, Ru, F] (p before the relu), s [P, NU], t [P, Ru], js [P, NU], jr [P, Ru] and
    the score rows S [P, NU, NJ], T [P, Ru, Ri].  js / jr given: s and t are read at those rows instead of the max."""
    X, Xt, Ks, Kr, bt = (_f64(a) for a in (X, Xt, Ks, Kr, bt))
    m, M = np.asarray(sent_mask, bool), np.asarray(rev_mask, bool)
    B, Ru, Su = m.shape
    P, NJ, F = Ks.shape
    Ri = Kr.shape[1]
    assert P == G * B and X.shape == (B, Ru * Su, F)
    out = dict(z=np.zeros((P, F)), w=np.zeros((P, Ru, Su)), v=np.zeros((P, Ru)), p=np.zeros((P, Ru, F)), a=np.zeros((P, Ru, F)),
               s=np.zeros((P, Ru * Su)), t=np.zeros((P, Ru)), js=np.zeros((P, Ru * Su), np.int64), jr=np.zeros((P, Ru), np.int64),
               S=np.zeros((P, Ru * Su, NJ)), T=np.zeros((P, Ru, Ri)))
    for q in range(P):
        b = q % B
        S = X[b] @ Ks[q].T                                             # [NU, NJ]
        out["S"][q] = S
        out["js"][q] = S.argmax(1) if js is None else np.asarray(js[q])  # argmax: the first of equals
        s = S[np.arange(Ru * Su), out["js"][q]]
        out["s"][q] = s
        for r in range(Ru):
            w = _softmax(s[r * Su:(r + 1) * Su], m[b, r])
            out["w"][q, r] = w
            acc = np.zeros(F)
            for k in range(Su):
                acc += w[k] * Xt[b, r * Su + k]
            out["a"][q, r] = acc + bt
        p = np.maximum(out["a"][q], 0.0)
        out["p"][q] = p
        T = p @ Kr[q].T                                                # [Ru, Ri]
        out["T"][q] = T
        out["jr"][q] = T.argmax(1) if jr is None else np.asarray(jr[q])
        t = T[np.arange(Ru), out["jr"][q]]
        out["t"][q] = t
        v = _softmax(t, M[b])
        out["v"][q] = v
        out["z"][q] = (v[:, None] * p).sum(0)
    return out


def attend_bwd_ref(X, Xt, sent_mask, rev_mask, Ks, Kr, fwd, dz, G):
    """The gradients of sum(z * dz) given attend_fwd_ref's dict (its routing included): dict of dX, dXt [B, NU, F], dKs [P, NJ, F],
    dKr [P, Ri, F], dbt [F]."""
    X, Xt, Ks, Kr, dz = (_f64(a) for a in (X, Xt, Ks, Kr, dz))
    m, M = np.asarray(sent_mask, bool), np.asarray(rev_mask, bool)
    B, Ru, Su = m.shape
    P, NJ, F = Ks.shape
    g = dict(dX=np.zeros_like(X), dXt=np.zeros_like(Xt), dKs=np.zeros_like(Ks), dKr=np.zeros_like(Kr), dbt=np.zeros(F))
    for q in range(P):
        b = q % B
        p, w, v, js, jr = (fwd[k][q] for k in ("p", "w", "v", "js", "jr"))
        dv = p @ dz[q]
        c = float(v @ dv)
        dt = np.where(M[b], v * (dv - c), 0.0)
        da = np.zeros((Ru, F))
        for r in range(Ru):
            dp = v[r] * dz[q] + dt[r] * Kr[q, jr[r]]
            da[r] = np.where(p[r] > 0, dp, 0.0)
            g["dKr"][q, jr[r]] += dt[r] * p[r]
        g["dbt"] += da.sum(0)
        for r in range(Ru):
            rows = np.arange(r * Su, (r + 1) * Su)
            e = Xt[b, rows] @ da[r]
            cs = float(w[r] @ e)
            ds = np.where(m[b, r], w[r] * (e - cs), 0.0)
            for k, n in enumerate(rows):
                g["dXt"][b, n] += w[r, k] * da[r]
                g["dX"][b, n] += ds[k] * Ks[q, js[n]]
                g["dKs"][q, js[n]] += ds[k] * X[b, n]
    return g


def attend_torch(X, Xt, sent_mask, rev_mask, Ks, Kr, bt, G):
    """The op's arithmetic as a torch composition (the reassociated restatement of the modules' user side: Xt, Ks, Kr are given),
    in the inputs' dtype on the inputs' device, differentiable by autograd: (z [P, F], w [P, Ru, Su], v [P, Ru])."""
    import torch
    B, Ru, Su = sent_mask.shape
    P, F = Ks.shape[0], Ks.shape[2]
    Xg, Xtg = X.repeat(G, 1, 1), Xt.repeat(G, 1, 1)                    # pair g * B + b reads user row b
    m, M = sent_mask.repeat(G, 1, 1), rev_mask.repeat(G, 1)
    s = torch.bmm(Xg, Ks.transpose(1, 2)).max(dim=2)[0].view(P, Ru, Su)
    w = torch.softmax(s.masked_fill(~m, MASK_FILL), dim=-1)
    p = torch.relu((w.unsqueeze(-1) * Xtg.view(P, Ru, Su, F)).sum(2) + bt)
    t = torch.bmm(p, Kr.transpose(1, 2)).max(dim=2)[0]
    v = torch.softmax(t.masked_fill(~M, MASK_FILL), dim=-1)
    return (v.unsqueeze(-1) * p).sum(1), w, v


def routing_margins(fwd):
    """(the least relative lead of a routing max over its runner-up -- lead / (1 + |best|) over both maxima, inf where an item
    has one row --, the least |a[r, f]|): the generators' precondition, under which a float32 run takes the same routes and the
    same relu branches as the float64 one."""
    lead = np.inf
    for scores in (fwd["S"], fwd["T"]):
        if scores.shape[-1] > 1:
            top = np.sort(scores, axis=-1)
            lead = min(lead, float(((top[..., -1] - top[..., -2]) / (1.0 + np.abs(top[..., -1]))).min()))
    return lead, float(np.abs(fwd["a"]).min())


def attains_max(scores, chosen, tol=1e-5):
    """Does row chosen[...] of every score row attain the row's max within tol * (1 + |best|)?"""
    best = scores.max(-1)
    got = np.take_along_axis(scores, np.asarray(chosen, np.int64)[..., None], -1)[..., 0]
    return bool((best - got <= tol * (1.0 + np.abs(best))).all())


def make_inputs(B, G, Ru, Su, Ri, Si, F, seed, special=True):
    """Seeded float32 inputs (torch CPU tensors) whose float64 routing has margins (routing_margins: lead >= 1e-4, |a| >= 1e-5,
    asserted here, over the rows that are not special).  special: user 0 has one fully masked review; with B >= 2 user 1 has no
    live review, with B >= 3 user 2 is a zero padding user (zero vectors, every mask off), and the LAST pair's item is all-zero
    (every product exactly 0: the tie rule's case).  Special rows are excluded from the margin check (their ties are the point)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale          # noqa: E731
    P, NU, NJ = G * B, Ru * Su, Ri * Si
    X, Xt = rnd(B, NU, F), rnd(B, NU, F, scale=0.5)
    sm = torch.rand(B, Ru, Su, generator=g) < 0.7
    sm[:, :, 0] = True                                             # ordinary reviews keep a live sentence
    Ks, Kr = rnd(P, NJ, F, scale=2.0 / F ** 0.5), rnd(P, Ri, F, scale=2.0 / F ** 0.5)
    bt = rnd(F, scale=0.2)
    plain = np.ones(P, bool)
    if special:
        sm[0, 0] = False
        if B >= 2:
            sm[1] = False
        if B >= 3:
            X[2], Xt[2], sm[2] = 0.0, 0.0, False
            plain[np.arange(P) % B == 2] = False
        if P >= 2:
            Ks[P - 1], Kr[P - 1] = 0.0, 0.0
            plain[P - 1] = False
    rm = sm.any(-1)
    fwd = attend_fwd_ref(X, Xt, sm.numpy(), rm.numpy(), Ks, Kr, bt, G)
    sub = {k: fwd[k][plain] for k in ("S", "T", "a")}
    if plain.any():
        lead, a_min = routing_margins(sub)
        assert lead >= 1e-4 and a_min >= 1e-5, (seed, lead, a_min)
    return dict(X=X, Xt=Xt, sent_mask=sm, rev_mask=rm, Ks=Ks, Kr=Kr, bt=bt), fwd
