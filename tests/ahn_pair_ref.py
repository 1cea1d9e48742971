"""AHN's pair decomposition restated in float64 numpy, one pair at a time, with none of the package's module code: the per-id
states (user_state_ref / item_state_ref, from sentence vectors and a state_dict) and the pair tail over them (pair_tail_ref:
steps 1-5 of csrc/ahn_pair.hip).  Reference of tests/test_ahn_pair_host.py, test_ahn_pair_edges_gpu.py and
test_ahn_recommend_gpu.py."""
import numpy as np

MASK_FILL = -1e8


def _f64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def masked_softmax(scores, mask):
    s = np.where(mask, scores, MASK_FILL)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _gated_scores(x, p, prefix):
    t = np.tanh(x @ _f64(p[prefix + ".trans_layer.0.weight"]).T)
    g = 1.0 / (1.0 + np.exp(-(x @ _f64(p[prefix + ".gate_layer.0.weight"]).T)))
    return (t * g) @ _f64(p[prefix + ".proj_layer.weight"]).reshape(-1)


def fm_partial(x, V, lw):
    """[K + 2]: x V, sum_k (x^2 V^2)_k, x . lw of one block x [F] of the FM's input."""
    return np.concatenate([x @ V, [((x * x) @ (V * V)).sum()], [x @ lw]])


def head_ref(p):
    F = _f64(p["user_review_trans_layer.0.bias"]).shape[0]
    V, lw = _f64(p["fm.V"]), _f64(p["fm.lin.weight"]).reshape(-1)
    return dict(bt=_f64(p["user_review_trans_layer.0.bias"]), VzT=V[:F].T.copy(), vz2=(V[:F] ** 2).sum(1), lz=lw[:F].copy(),
                lin_b=_f64(p["fm.lin.bias"]).reshape(1))


def user_state_ref(p, X, sent_mask, rev_mask, u_id):
    """X [Ru, Su, F] sentence vectors of one user -> dict(X [Ru*Su, F], Xt, sent_mask [Ru, Su], rev_mask [Ru], fm [K + 2])."""
    Ru, Su, F = X.shape
    X = _f64(X).reshape(Ru * Su, F)
    V, lw = _f64(p["fm.V"]), _f64(p["fm.lin.weight"]).reshape(-1)
    e_u = _f64(p["user_embeddings.embedding.weight"])[int(u_id)]
    return dict(X=X, Xt=X @ _f64(p["user_review_trans_layer.0.weight"]).T, sent_mask=np.asarray(sent_mask, bool).reshape(Ru, Su),
                rev_mask=np.asarray(rev_mask, bool).reshape(Ru), fm=fm_partial(e_u, V[F:2 * F], lw[F:2 * F]))


def item_state_ref(p, Y, sent_mask, rev_mask, i_id):
    """Y [Ri, Si, F] sentence vectors of one item -> dict(Ks [Ri*Si, F], Kr [Ri, F], fm [K + 2], item_sent_weights [Ri, Si],
    item_review_weights [Ri])."""
    Ri, Si, F = Y.shape
    Y = _f64(Y)
    sm, rm = np.asarray(sent_mask, bool).reshape(Ri, Si), np.asarray(rev_mask, bool).reshape(Ri)
    sa, ra = "unbalanced_sentence_aggregator", "unbalanced_review_aggregator"
    sc = _gated_scores(Y.reshape(Ri * Si, F), p, sa + ".item_aggregator").reshape(Ri, Si)
    sent_w = masked_softmax(sc, sm)                                             # per review
    all_w = masked_softmax(sc.reshape(Ri * Si), sm.reshape(Ri * Si))            # over all of the item's sentences
    r = (sent_w[:, :, None] * Y).sum(1)
    Ks = (all_w[:, None] * Y.reshape(Ri * Si, F)) @ _f64(p[sa + ".bilinear.weight"]).T
    r = np.maximum(r @ _f64(p["item_review_trans_layer.0.weight"]).T + _f64(p["item_review_trans_layer.0.bias"]), 0.0)
    rev_w = masked_softmax(_gated_scores(r, p, ra + ".item_aggregator"), rm)
    q = (rev_w[:, None] * r).sum(0)
    Kr = r @ _f64(p[ra + ".bilinear.weight"]).T
    V, lw = _f64(p["fm.V"]), _f64(p["fm.lin.weight"]).reshape(-1)
    e_i = _f64(p["item_embeddigns.embedding.weight"])[int(i_id)]
    fm = fm_partial(q, V[2 * F:3 * F], lw[2 * F:3 * F]) + fm_partial(e_i, V[3 * F:], lw[3 * F:])
    return dict(Ks=Ks, Kr=Kr, fm=fm, item_sent_weights=sent_w, item_review_weights=rev_w)


def pair_tail_ref(us, its, head):
    """Steps 1-5 for ONE pair, as loops: (score, w [Ru, Su], v [Ru]) from a user state, an item state and the head (dicts of
    float64 arrays as user_state_ref / item_state_ref / head_ref return them)."""
    X, Xt, Ks, Kr = (_f64(a) for a in (us["X"], us["Xt"], its["Ks"], its["Kr"]))
    m, M = np.asarray(us["sent_mask"], bool), np.asarray(us["rev_mask"], bool)
    Ru, Su = m.shape
    F = X.shape[1]
    bt, VzT, vz2, lz = (_f64(head[k]) for k in ("bt", "VzT", "vz2", "lz"))
    K = VzT.shape[0]
    s = np.empty(Ru * Su)
    for n in range(Ru * Su):                                                   # 1. over ALL of the item's rows
        s[n] = max(float(X[n] @ Ks[j]) for j in range(Ks.shape[0]))
    w = np.empty((Ru, Su))
    p = np.empty((Ru, F))
    for r in range(Ru):
        w[r] = masked_softmax(s[r * Su:(r + 1) * Su], m[r])                    # 2.
        acc = np.zeros(F)
        for q in range(Su):
            acc += w[r, q] * Xt[r * Su + q]
        p[r] = np.maximum(acc + bt, 0.0)                                       # 3.
    t = np.array([max(float(p[r] @ Kr[j]) for j in range(Kr.shape[0])) for r in range(Ru)])
    v = masked_softmax(t, M)                                                   # 4.
    z = np.zeros(F)
    for r in range(Ru):
        z += v[r] * p[r]
    fu, fi = _f64(us["fm"]), _f64(its["fm"])
    xv = np.array([z @ VzT[k] for k in range(K)]) + fu[:K] + fi[:K]            # 5.
    score = 0.5 * ((xv ** 2).sum() - (z * z) @ vz2 - fu[K] - fi[K]) + z @ lz + fu[K + 1] + fi[K + 1] + float(_f64(head["lin_b"])[0])
    return float(score), w, v


def pair_ref(p, X, u_sent_mask, u_rev_mask, u_id, Y, i_sent_mask, i_rev_mask, i_id):
    """One pair from the two sides' sentence vectors and a state_dict: (score, user_sent_weights, item_sent_weights,
    user_review_weights, item_review_weights) -- AHN.forward's five outputs in eval mode."""
    us, its = user_state_ref(p, X, u_sent_mask, u_rev_mask, u_id), item_state_ref(p, Y, i_sent_mask, i_rev_mask, i_id)
    score, w, v = pair_tail_ref(us, its, head_ref(p))
    return score, w, its["item_sent_weights"], v, its["item_review_weights"]
