"""AHN's pair decomposition without a GPU: the float64 restatement (tests/ahn_pair_ref.py) against the reference's own run and
against AHN.aggregate at the mask edges, the argument validation of the two C entry points of csrc/ahn_pair.hip, and
AhnRecommender's selection logic and command line on the CPU.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import ahn_pair_ref as R
import synth_ahn
from helpers import golden, max_err, quiet

BAD_ARG = -1
P = 0x1000        # a non-NULL pointer that is never dereferenced: every check below fails before the first device call


def _params(g):
    return {k[len("param/"):]: g[k] for k in g.files if k.startswith("param/")}


# ------------------------------------------------------------------ 1. the restatement on the reference's own run
@pytest.mark.parametrize("name", ("tiny", "small"))
def test_decomposition_reproduces_the_reference_fixture(golden_dir, name):
    g = golden(golden_dir, "ahn_" + name)
    c = synth_ahn.AHN_CFGS[name]
    B, Rn, S, H = c["B"], c["R"], c["S"], c["H"]
    p = _params(g)
    us, its = g["user_sents"].reshape(B, Rn, S, H), g["item_sents"].reshape(B, Rn, S, H)
    assert us.dtype == np.float64
    assert (~g["in/item_sent_masks"]).any() and (~g["in/user_review_masks"]).any()       # item-side zero candidates, a dead review
    for b in range(B):
        score, w, isw, v, irw = R.pair_ref(p, us[b], g["in/user_sent_masks"][b], g["in/user_review_masks"][b], g["in/user_ids"][b],
                                           its[b], g["in/item_sent_masks"][b], g["in/item_review_masks"][b], g["in/item_ids"][b])
        assert abs(score - float(g["pred_eval"][b])) <= 1e-9
        for got, key in ((w, "user_sent_weights"), (isw, "item_sent_weights"), (v, "user_review_weights"), (irw, "item_review_weights")):
            assert max_err(got, g[key][b]) <= 1e-9, (key, b)


# ------------------------------------------------------------------ 2. against AHN.aggregate in double, at the mask edges
EDGE_SHAPES = [dict(Ru=3, Su=4, Ri=2, Si=5), dict(Ru=1, Su=3, Ri=3, Si=2), dict(Ru=4, Su=1, Ri=2, Si=3)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(str(v) for v in s.values()))
def test_decomposition_equals_aggregate_at_the_mask_edges(shape):
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    Ru, Su, Ri, Si = shape["Ru"], shape["Su"], shape["Ri"], shape["Si"]
    F, K, U, I, B = 10, 3, 5, 6, 4
    torch.manual_seed(17 + Ru)
    model = quiet(AHN, F, F, K, U, I, 30, None, dropout=0.0, item_review_num=Ri).double().eval()
    with torch.no_grad():
        for prm in model.parameters():
            prm.copy_(torch.randn_like(prm) * 0.4)
    X, Y = torch.randn(B, Ru, Su, F, dtype=torch.float64), torch.randn(B, Ri, Si, F, dtype=torch.float64)
    um, im = torch.rand(B, Ru, Su) < 0.7, torch.rand(B, Ri, Si) < 0.7
    um[0, 0] = False                    # a fully masked user review (the only one when Ru == 1)
    um[1] = False                       # a user with no live review
    im[2] = False                       # an item with no live sentence
    um[3], im[3] = True, True
    uM, iM = um.any(-1), im.any(-1)
    u_ids, i_ids = torch.tensor([1, 2, 0, 4]), torch.tensor([5, 0, 3, 1])          # the padding ids too
    with torch.no_grad():
        pred, usw, isw, urw, irw = model.aggregate(X, Y, um, im, uM, iM, u_ids, i_ids)
    p = {k: v.numpy() for k, v in model.state_dict().items()}
    for b in range(B):
        score, w, sw, v, rw = R.pair_ref(p, X[b].numpy(), um[b].numpy(), uM[b].numpy(), int(u_ids[b]), Y[b].numpy(), im[b].numpy(),
                                         iM[b].numpy(), int(i_ids[b]))
        assert abs(score - float(pred[b])) <= 1e-9 * (1 + abs(float(pred[b]))), b
        for got, want in ((w, usw), (sw, isw), (v, urw), (rw, irw)):
            assert max_err(got, want[b].numpy()) <= 1e-12, b
    assert max_err(usw[1].numpy(), np.full((Ru, Su), 1.0 / Su)) <= 1e-15           # fully masked: uniform, as in the reference
    assert max_err(urw[1].numpy(), np.full(Ru, 1.0 / Ru)) <= 1e-15


# ------------------------------------------------------------------ 3. argument validation of the C entry points
def _structs(L, **kw):
    from review_based_recommender_amd import _lib
    s = dict(Ru=3, Su=4, Ri=2, Si=5, F=12, K=4)
    s.update({k: v for k, v in kw.items() if k in s})
    shape = _lib.AhnShape(*(s[k] for k in ("Ru", "Su", "Ri", "Si", "F", "K")))
    user = _lib.AhnUserState(*(kw.get(k, P) for k in ("X", "Xt", "sent_mask", "rev_mask", "ufm")), kw.get("U", 5))
    item = _lib.AhnItemState(*(kw.get(k, P) for k in ("Ks", "Kr", "ifm")), kw.get("I", 6))
    head = _lib.AhnHead(*(kw.get(k, P) for k in ("bt", "VzT", "vz2", "lz", "lin_b")))
    return shape, user, item, head


def _ids(L, **kw):
    shape, user, item, head = _structs(L, **kw)
    ref = lambda name, st: None if kw.get(name, 1) is None else C.byref(st)          # noqa: E731
    return L.rbr_ahn_pair_score_ids(ref("shape", shape), ref("user", user), ref("item", item), ref("head", head), kw.get("P", 4),
                                    kw.get("u_rows", P), kw.get("i_rows", P), kw.get("bits", 64), kw.get("out", P), kw.get("w_out"),
                                    kw.get("v_out"), None, None)


def _dense(L, **kw):
    shape, user, item, head = _structs(L, **kw)
    ref = lambda name, st: None if kw.get(name, 1) is None else C.byref(st)          # noqa: E731
    return L.rbr_ahn_pair_score_dense(ref("shape", shape), ref("user", user), ref("item", item), ref("head", head), kw.get("Nu", 4),
                                      kw.get("u_rows", P), kw.get("bits", 64), kw.get("out", P), None, None)


BAD_COMMON = [dict(Ru=0), dict(Su=-1), dict(Ri=0), dict(Si=0), dict(F=0), dict(K=0), dict(K=-2),
              dict(Ru=65, Su=1), dict(Su=65, Ru=1), dict(Ru=13, Su=10), dict(Ri=13, Si=10), dict(Ri=1 << 16, Si=1 << 16),
              dict(F=2049), dict(F=2048, Ru=4, Su=2), dict(K=65), dict(F=1 << 30),
              dict(U=0), dict(I=-4), dict(X=None), dict(Xt=None), dict(sent_mask=None), dict(rev_mask=None), dict(ufm=None),
              dict(Ks=None), dict(Kr=None), dict(ifm=None), dict(bt=None), dict(VzT=None), dict(vz2=None), dict(lz=None),
              dict(lin_b=None), dict(shape=None), dict(user=None), dict(item=None), dict(head=None), dict(out=None), dict(bits=16),
              dict(bits=0)]


def test_pair_score_entries_refuse_bad_arguments():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    for n in ("rbr_ahn_pair_score_ids", "rbr_ahn_pair_score_dense"):
        assert n in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), n), n
    for kw in BAD_COMMON + [dict(P=0), dict(P=-1), dict(P=1 << 31), dict(P=1 << 40), dict(u_rows=None), dict(i_rows=None)]:
        assert _ids(L, **kw) == BAD_ARG, kw
        assert len(L.rbr_last_error()) > 0
    for kw in BAD_COMMON + [dict(Nu=0), dict(Nu=-7), dict(Nu=6, u_rows=None), dict(Nu=1 << 30, I=1 << 30)]:
        assert _dense(L, **kw) == BAD_ARG, kw
        assert len(L.rbr_last_error()) > 0
    assert _ids(L, Ru=13, Su=10) == BAD_ARG and b"128" in L.rbr_last_error()         # the caps are named in the text
    with pytest.raises(RuntimeError, match="failed"):
        _lib.check(BAD_ARG, "rbr_ahn_pair_score_ids")


def test_functional_entries_refuse_cpu_tensors_and_bad_shapes():
    from review_based_recommender_amd import functional as RF
    us = RF.AhnUserState(torch.zeros(3, 6, 4), torch.zeros(3, 6, 4), torch.ones(3, 2, 3, dtype=torch.bool), torch.ones(3, 2, dtype=torch.bool),
                         torch.zeros(3, 5))
    its = RF.AhnItemState(torch.zeros(2, 4, 4), torch.zeros(2, 2, 4), torch.zeros(2, 5), torch.zeros(2, 2, 2), torch.zeros(2, 2))
    head = RF.AhnPairHead(torch.zeros(4), torch.zeros(3, 4), torch.zeros(4), torch.zeros(4), torch.zeros(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.ahn_pair_score(us, its, head, torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.ahn_pair_score_dense(us, its, head, torch.tensor([1]))


# ------------------------------------------------------------------ 4. selection over a hand-made score block, and the CLI
NAN, INF = float("nan"), float("inf")
BLOCK = torch.tensor([[9.0, 1.0, 3.0, 3.0, 2.0, 3.0],          # ties between items 2, 3, 5; item 0 scores best and never shows
                      [0.0, NAN, 5.0, -INF, 5.0, 4.0],         # a NaN score, a genuine -inf, a tie
                      [1.0, 2.0, NAN, NAN, NAN, NAN]])         # one candidate only


def test_select_topk_ties_exclusion_and_short_rows():
    from review_based_recommender_amd.recommend import SeenItems, exclusion_mask, select_topk
    items, scores = select_topk(BLOCK, 4)
    assert items.tolist() == [[2, 3, 5, 4], [2, 4, 5, 3], [1, -1, -1, -1]]
    assert scores[0].tolist() == [3.0, 3.0, 3.0, 2.0] and scores[1].tolist() == [5.0, 5.0, 4.0, -INF]
    assert scores[2].tolist() == [2.0, -INF, -INF, -INF]
    assert items.dtype == torch.int64
    # exclusion: a CSR over all user ids, rows 0 and 1 both user 3 (a duplicate), row 2 user 1; an item outside the table lists nothing
    seen = SeenItems(torch.tensor([0, 0, 1, 1, 4]), torch.tensor([1, 2, 4, 77], dtype=torch.int32))
    u_ids = torch.tensor([3, 3, 1])
    ex = exclusion_mask(seen, u_ids, 6)
    assert ex.tolist() == [[False, False, True, False, True, False]] * 2 + [[False, True, False, False, False, False]]
    items, scores = select_topk(BLOCK, 3, ex)
    assert items.tolist() == [[3, 5, 1], [5, 3, -1], [-1, -1, -1]]
    # the same lists as a CSR pair aligned with the rows
    pair = (torch.tensor([0, 2, 4, 5]), torch.tensor([2, 4, 2, 4, 1], dtype=torch.int32))
    assert torch.equal(exclusion_mask(pair, u_ids, 6), ex)
    # a user id outside the CSR excludes nothing; k beyond the item count is fill
    assert not exclusion_mask(seen, torch.tensor([9, -1]), 6).any()
    items, _ = select_topk(BLOCK[:1], 8)
    assert items.tolist() == [[2, 3, 5, 4, 1, -1, -1, -1]]
    with pytest.raises(ValueError):
        select_topk(BLOCK, 0)


def test_rank_in_block_matches_the_topk_order_and_marks_the_unranked():
    from review_based_recommender_amd.recommend import exclusion_mask, rank_in_block, rank_metrics, select_topk
    rows = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, 0, 0])
    tgt = torch.tensor([2, 3, 5, 1, 3, 4, 1, 1, 2, 0, 6])
    rank, n_cand = rank_in_block(BLOCK[rows], tgt)
    assert rank.tolist() == [0, 1, 2, 4, 3, 1, -1, 0, -1, -1, -1]           # NaN target, padding item, id outside the table: -1
    assert n_cand.tolist() == [5, 5, 5, 5, 4, 4, 4, 1, 1, 5, 5]
    assert rank.dtype == torch.int32 and n_cand.dtype == torch.int32
    # consistent with select_topk: the target stands at position rank of its row's list
    full, _ = select_topk(BLOCK, 5)
    for b in range(len(rows)):
        if rank[b] >= 0:
            assert int(full[rows[b], rank[b]]) == int(tgt[b])
    # the target is never excluded, other excluded items stop counting
    pair = (torch.tensor([0, 2, 4]), torch.tensor([2, 3, 2, 3], dtype=torch.int32))
    ex = exclusion_mask(pair, torch.tensor([0, 0]), 6)
    rank, n_cand = rank_in_block(BLOCK[[0, 0]], torch.tensor([3, 5]), ex)
    assert rank.tolist() == [0, 0] and n_cand.tolist() == [4, 3]
    assert rank_metrics(rank, n_cand, (1,))["hr@1"] == 1.0


def test_cli_accepts_ahn_and_refuses_explain_with_it():
    from review_based_recommender_amd.recommend import AhnRecommender, parse_cli
    a = parse_cli(["--model", "ahn", "--config", "c", "--checkpoint", "m", "--out", "o", "--k", "5", "--exclude-train"])
    assert (a.model, a.k, a.exclude_train) == ("ahn", 5, True)
    b = parse_cli(["--model", "ahn", "--config", "c", "--checkpoint", "m", "--eval-split", "test", "--ks", "1,3"])
    assert b.ks == (1, 3) and b.out is None
    with pytest.raises(SystemExit):
        parse_cli(["--model", "ahn", "--config", "c", "--checkpoint", "m", "--out", "o", "--explain", "3"])
    with pytest.raises(ValueError, match="AHN"):
        AhnRecommender(torch.nn.Linear(2, 2), user=torch.zeros(2, 1, 1, 1), item=torch.zeros(2, 1, 1, 1))


def test_ahn_recommender_on_the_cpu_is_refused_and_restores_the_mode():
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.recommend import AhnRecommender
    m = quiet(AHN, 8, 8, 3, 4, 5, 20, None, item_review_num=2)
    rec = AhnRecommender(m, user=torch.zeros(4, 2, 3, 5, dtype=torch.int32), item=torch.zeros(5, 2, 3, 5, dtype=torch.int32))
    assert rec.stale and rec.item_lo == 1 and (rec.n_users, rec.n_items) == (4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        rec.refresh()
    assert m.training
    with pytest.raises(RuntimeError, match="refresh"):
        rec.score(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError):
        AhnRecommender(m, user=torch.zeros(4, 6), item=torch.zeros(5, 6))
