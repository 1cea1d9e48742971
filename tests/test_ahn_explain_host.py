"""AHN's sentence explanation without a GPU: the float64 restatement (tests/ahn_explain_ref.py) against torch's float64 autograd
through the op's composition and a full torch FM, its sum identities, the --sentences rules of the command line, and the argument
validation of rbr_ahn_pair_explain_ids (csrc/ahn_explain.hip).  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ahn_attend_ref as A
import ahn_explain_ref as E
from helpers import quiet

BAD_ARG = -1
PTR = 0x1000      # a non-NULL pointer that is never dereferenced: every check below fails before the first device call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, G, Ru, Su, Ri, Si, F, K, seed): two small shapes, the second with special rows in play (B >= 3) and K beyond one wave round
SMALL = [(2, 1, 3, 4, 2, 5, 12, 3, 100), (3, 2, 2, 3, 3, 2, 10, 5, 100)]


def _case(B, G, Ru, Su, Ri, Si, F, K, seed):
    t, _ = A.make_inputs(B, G, Ru, Su, Ri, Si, F, seed)
    return t, E.make_head(B, G * B, Ri, F, K, seed + 1)


# ------------------------------------------------------------------ 1. the restatement against torch's float64 autograd
@pytest.mark.parametrize("cfg", SMALL, ids=lambda c: "x".join(str(v) for v in c[:8]))
def test_reference_equals_float64_autograd_through_the_composition(cfg):
    B, G, Ru, Su, Ri, Si, F, K, seed = cfg
    P = G * B
    t, h = _case(*cfg)
    d = lambda x: x.double()                                                             # noqa: E731
    leaf = {k: d(t[k]).requires_grad_(True) for k in ("X", "Xt", "Ks", "Kr")}
    Rp = d(h["Rp"]).requires_grad_(True)
    z, w, v = A.attend_torch(leaf["X"], leaf["Xt"], t["sent_mask"], t["rev_mask"], leaf["Ks"], leaf["Kr"], d(t["bt"]), G)
    # TorchFM over final_features = [z, e_u, q, e_i] with n = 4 F: blocks 0 and 2 of V / lin_w are the head's, 1 and 3 random here
    gen = torch.Generator().manual_seed(seed + 2)
    eu, ei = torch.randn(B, F, generator=gen, dtype=torch.float64), torch.randn(P, F, generator=gen, dtype=torch.float64)
    V = torch.cat([d(h["VzT"]).t(), torch.randn(F, K, generator=gen, dtype=torch.float64) * 0.3, d(h["VqT"]).t(),
                   torch.randn(F, K, generator=gen, dtype=torch.float64) * 0.3])
    lw = torch.cat([d(h["lz"]), torch.randn(F, generator=gen, dtype=torch.float64), d(h["lq"]), torch.randn(F, generator=gen, dtype=torch.float64)])
    q = (d(h["beta"]).unsqueeze(-1) * Rp).sum(1)
    x = torch.cat([z, eu.repeat(G, 1), q, ei], dim=1)
    score = 0.5 * ((x @ V) ** 2 - (x * x) @ (V * V)).sum(1) + x @ lw + d(h["lin_b"])
    # the ids' hoisted rows, as AHN._fm_partial cuts them: block 1 for the user, blocks 2 + 3 for the item
    part = lambda y, k: torch.cat([y @ V[k * F:(k + 1) * F], ((y * y) @ (V[k * F:(k + 1) * F] ** 2)).sum(1, keepdim=True),       # noqa: E731
                                   (y @ lw[k * F:(k + 1) * F]).unsqueeze(1)], dim=1)
    with torch.no_grad():
        h = dict(h, ufm=part(eu, 1), ifm=part(q, 2) + part(ei, 3), vz2=(V[:F] ** 2).sum(1), vq2=(V[2 * F:3 * F] ** 2).sum(1))
    ref = E.explain_ref(t, h, G)
    attend_p = torch.relu((w.unsqueeze(-1) * leaf["Xt"].repeat(G, 1, 1).view(P, Ru, Su, F)).sum(2) + d(t["bt"])).detach()      # [P, Ru, F]
    gX, gXt, gKs, gKr = torch.autograd.grad(score.sum(), [leaf[k] for k in ("X", "Xt", "Ks", "Kr")], retain_graph=True)
    (gz,) = torch.autograd.grad(score.sum(), z, retain_graph=True)
    (gRp,) = torch.autograd.grad(score.sum(), Rp, retain_graph=True)
    (gq,) = torch.autograd.grad(score.sum(), q, retain_graph=True)
    worst = 0.0
    for p in range(P):
        b, r = p % B, ref[p]
        assert abs(r["score"] - float(score[p].detach())) <= 1e-12 * (1 + abs(r["score"]))
        assert np.abs(r["w"] - w[p].detach().numpy()).max() <= 1e-13 and np.abs(r["v"] - v[p].detach().numpy()).max() <= 1e-13
        assert np.abs(r["dz"] - gz[p].numpy()).max() <= 1e-12 and np.abs(r["dq"] - gq[p].numpy()).max() <= 1e-12
        # a user's gradient is the sum over its G pairs: compare pair by pair on a graph of that pair alone
        one = torch.autograd.grad(score[p], [leaf["X"], leaf["Xt"]], retain_graph=True)
        want = {"user_sentences": ((one[0][b] * leaf["X"][b]).sum(1) + (one[1][b] * leaf["Xt"][b]).sum(1)).detach().numpy().reshape(Ru, Su),
                "user_reviews": (v[p] * (attend_p[p] @ gz[p])).detach().numpy(), "user_text": float(gz[p] @ z[p].detach()),
                "item_sentence_match": (gKs[p] * leaf["Ks"][p]).sum(1).detach().numpy(),
                "item_review_match": (gKr[p] * leaf["Kr"][p]).sum(1).detach().numpy(),
                "item_reviews": (gRp[p] * Rp[p]).sum(1).detach().numpy(), "item_text": float(gq[p] @ q[p].detach())}
        for k, val in want.items():
            err = float(np.abs(np.asarray(r[k]) - val).max())
            worst = max(worst, err)
            assert err <= 1e-12 * (1 + float(np.abs(val).max())), (p, k, err)
    assert G == 1 or any(float(np.abs(gX[b].numpy()).max()) > 0 for b in range(B))
    print(f"reference vs float64 autograd: largest difference {worst:.2e}")


# ------------------------------------------------------------------ 2. the sum identities
@pytest.mark.parametrize("cfg", SMALL, ids=lambda c: "x".join(str(v) for v in c[:8]))
def test_reference_sum_identities(cfg):
    t, h = _case(*cfg)
    G = cfg[1]
    for r in E.explain_ref(t, h, G):
        tol = lambda x: 1e-12 * (1 + abs(x))                                             # noqa: E731
        assert abs(r["user_reviews"].sum() - r["user_text"]) <= tol(r["user_text"])
        assert abs(r["item_reviews"].sum() - r["item_text"]) <= tol(r["item_text"])
        bias = sum(r["v"][k] * float(np.where(r["p"][k] > 0, r["dz"], 0.0) @ t["bt"].double().numpy()) for k in range(len(r["v"])))
        assert abs(r["user_sentences_fixed"].sum() - (r["user_text"] - bias)) <= tol(r["user_text"])
        assert abs(r["item_sentence_match"].sum() - float(r["ds"] @ r["s"])) <= tol(float(np.abs(r["ds"] * r["s"]).sum()))
        assert abs(r["item_review_match"].sum() - float(r["dt"] @ r["t"])) <= tol(float(np.abs(r["dt"] * r["t"]).sum()))
        # the kernel's scalar shortcut for a sentence, element by element: w e + ds s = <dX, X> + <dXt, Xt>
        short = r["w"].reshape(-1) * r["e"] + r["ds"] * r["s"]
        assert np.abs(short - r["user_sentences"].reshape(-1)).max() <= tol(float(np.abs(short).max()))
        # rows nobody matched are exactly 0
        assert not r["item_sentence_match"][np.setdiff1d(np.arange(r["S"].shape[1]), r["js"])].any()
        assert not r["item_review_match"][np.setdiff1d(np.arange(r["T"].shape[1]), r["jr"])].any()


# ------------------------------------------------------------------ 3. the command line
def test_cli_sentences_rules():
    from review_based_recommender_amd.recommend import parse_cli
    base = ["--config", "c", "--checkpoint", "m"]
    a = parse_cli(["--model", "ahn", *base, "--out", "o", "--sentences", "3"])
    assert a.sentences == 3 and a.explain is None
    assert parse_cli(["--model", "ahn", *base, "--out", "o"]).sentences is None
    for bad in (["--model", "ahn", *base, "--eval-split", "test", "--sentences", "3"],            # no --out
                ["--model", "ahn", *base, "--out", "o", "--sentences", "0"],
                ["--model", "ahn", *base, "--out", "o", "--sentences", "-2"],
                *(["--model", m, *base, "--out", "o", "--sentences", "3"] for m in ("deepconn", "narre", "dual_att", "simple_siamese")),
                ["--model", "ahn", *base, "--out", "o", "--attention", "3"],
                ["--model", "ahn", *base, "--out", "o", "--contributions", "3"]):
        with pytest.raises(SystemExit):
            parse_cli(bad)


# ------------------------------------------------------------------ 4. the entry: declared, bound, exported, and its refusals
def test_entry_is_declared_bound_and_exported():
    from review_based_recommender_amd import _lib
    name = "rbr_ahn_pair_explain_ids"
    header = open(os.path.join(ROOT, "include", "rbr_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    for struct, cls in (("rbr_ahn_explain_rows", _lib.AhnExplainRows), ("rbr_ahn_explain_out", _lib.AhnExplainOut)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()] == [n for n, _ in cls._fields_]      # one to one, in order
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 12
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert hasattr(_lib.lib(), name)


def _explain(L, **kw):
    from review_based_recommender_amd import _lib
    s = dict(Ru=3, Su=4, Ri=2, Si=5, F=12, K=4)
    s.update({k: v for k, v in kw.items() if k in s})
    shape = _lib.AhnShape(*(s[k] for k in ("Ru", "Su", "Ri", "Si", "F", "K")))
    user = _lib.AhnUserState(*(kw.get(k, PTR) for k in ("X", "Xt", "sent_mask", "rev_mask", "ufm")), kw.get("U", 5))
    item = _lib.AhnItemState(*(kw.get(k, PTR) for k in ("Ks", "Kr", "ifm")), kw.get("I", 6))
    head = _lib.AhnHead(*(kw.get(k, PTR) for k in ("bt", "VzT", "vz2", "lz", "lin_b")))
    extra = _lib.AhnExplainRows(*(kw.get(k, PTR) for k in ("Rp", "beta", "VqT", "vq2", "lq")))
    out = _lib.AhnExplainOut(*(kw.get("out_" + k, PTR) for k in _lib.AHN_EXPLAIN_OUT))
    ref = lambda name, st: None if kw.get(name, 1) is None else C.byref(st)              # noqa: E731
    return L.rbr_ahn_pair_explain_ids(ref("shape", shape), ref("user", user), ref("item", item), ref("head", head), ref("extra", extra),
                                      kw.get("P", 4), kw.get("u_rows", PTR), kw.get("i_rows", PTR), kw.get("bits", 64), ref("out", out),
                                      None, None)


def test_entry_refuses_bad_arguments_before_any_launch():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    null_ptrs = [{k: None} for k in ("X", "Xt", "sent_mask", "rev_mask", "ufm", "Ks", "Kr", "ifm", "bt", "VzT", "vz2", "lz", "lin_b",
                                     "Rp", "beta", "VqT", "vq2", "lq", "u_rows", "i_rows", "shape", "user", "item", "head", "extra", "out")]
    null_ptrs += [{"out_" + k: None} for k in _lib.AHN_EXPLAIN_OUT]
    caps = [dict(Ru=65, Su=1), dict(Su=65, Ru=1), dict(Ru=13, Su=10), dict(Ri=13, Si=10), dict(F=2049), dict(F=2048, Ru=4, Su=2),
            dict(K=65), dict(Ru=0), dict(Su=0), dict(Ri=0), dict(Si=0), dict(F=0), dict(K=0), dict(U=0), dict(I=0)]
    for kw in null_ptrs + caps + [dict(P=0), dict(P=-3), dict(P=1 << 31), dict(bits=16), dict(bits=0)]:
        assert _explain(L, **kw) == BAD_ARG, kw
        assert len(L.rbr_last_error()) > 0
    assert _explain(L, Ru=13, Su=10) == BAD_ARG and b"128" in L.rbr_last_error()          # the caps are named in the text
    assert _explain(L, bits=16) == BAD_ARG and b"index_bits" in L.rbr_last_error()


def test_functional_entry_refuses_cpu_tensors():
    from review_based_recommender_amd import functional as RF
    us = RF.AhnUserState(torch.zeros(3, 6, 4), torch.zeros(3, 6, 4), torch.ones(3, 2, 3, dtype=torch.bool), torch.ones(3, 2, dtype=torch.bool),
                         torch.zeros(3, 5))
    its = RF.AhnItemState(torch.zeros(2, 4, 4), torch.zeros(2, 2, 4), torch.zeros(2, 5), torch.zeros(2, 2, 2), torch.zeros(2, 2))
    head = RF.AhnPairHead(torch.zeros(4), torch.zeros(3, 4), torch.zeros(4), torch.zeros(4), torch.zeros(1))
    extra = RF.AhnExplainRows(torch.zeros(2, 2, 4), torch.zeros(3, 4), torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.ahn_pair_explain(us, its, head, extra, torch.tensor([1]), torch.tensor([1]))


# ------------------------------------------------------------------ 5. the recommender before refresh(), and the model's two cuts
def test_sentences_before_refresh_raises_and_the_model_cuts_the_q_block():
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.recommend import AhnRecommender, SentenceContributions
    m = quiet(AHN, 8, 8, 3, 4, 5, 20, None, item_review_num=2)
    rec = AhnRecommender(m, user=torch.zeros(4, 2, 3, 5, dtype=torch.int32), item=torch.zeros(5, 2, 3, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="refresh"):
        rec.sentences(torch.tensor([1]), torch.tensor([1]))
    assert SentenceContributions._fields == (
        "score", "user_sent_weights", "item_sent_weights", "user_review_weights", "item_review_weights", "user_sentences",
        "user_sentences_fixed", "user_reviews", "user_text", "user_match", "review_match", "item_sentence_match", "item_review_match",
        "item_reviews", "item_text")
    VqT, vq2, lq = m.explain_head()
    V, lw = m.fm.V.detach(), m.fm.lin.weight.detach().view(-1)
    assert torch.equal(VqT, V[16:24].t()) and torch.equal(vq2, (V[16:24] * V[16:24]).sum(1)) and torch.equal(lq, lw[16:24])
    # r' is what item_state's Kr and pooled q are made of (CPU torch composition: no kernel)
    Y, sm = torch.randn(3, 2, 3, 8), torch.rand(3, 2, 3) < 0.7
    rp = m.item_reviews(Y, sm)
    assert rp.shape == (3, 2, 8) and not rp.requires_grad and m.training
    m.eval()
    with torch.no_grad():
        r, _, _ = m.unbalanced_sentence_aggregator.item_aggregator(Y.reshape(6, 3, 8), sm.reshape(6, 3))
        assert torch.equal(rp, m.item_review_trans_layer(r).view(3, 2, 8))
