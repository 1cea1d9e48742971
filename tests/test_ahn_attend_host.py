"""functional.ahn_pair_attend without a GPU: the float64 restatement of the op (tests/ahn_attend_ref.py) against
ahn_pair_ref.pair_tail_ref (forward) and against torch.autograd in float64 over the module composition on the CPU (forward and
every gradient), the argument validation of the two C entry points of csrc/ahn_attend.hip, and the trainer's `ahn_tables` opt-in.
No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import ahn_attend_ref as A
import ahn_pair_ref as R
from helpers import max_err, quiet

BAD_ARG = -1
PTR = 0x1000      # a non-NULL pointer that is never dereferenced: every check below fails before the first device call


# ------------------------------------------------------------------ 1. the forward against the pair tail's restatement
@pytest.mark.parametrize("B,G,u,i,F,seed", [(3, 2, (3, 4), (2, 5), 12, 1), (1, 1, (1, 1), (1, 1), 12, 2), (2, 3, (3, 11), (11, 3), 34, 3)])
def test_forward_restatement_equals_pair_tail_ref(B, G, u, i, F, seed):
    t, fwd = A.make_inputs(B, G, *u, *i, F, seed)
    head = dict(bt=t["bt"], VzT=np.zeros((1, F)), vz2=np.zeros(F), lz=np.zeros(F), lin_b=np.zeros(1))
    for q in range(G * B):
        b = q % B
        us = dict(X=t["X"][b], Xt=t["Xt"][b], sent_mask=t["sent_mask"][b].numpy(), rev_mask=t["rev_mask"][b].numpy(), fm=np.zeros(3))
        its = dict(Ks=t["Ks"][q], Kr=t["Kr"][q], fm=np.zeros(3))
        _, w, v = R.pair_tail_ref(us, its, head)
        assert max_err(fwd["w"][q], w) <= 1e-12 and max_err(fwd["v"][q], v) <= 1e-12, q
    if G * B >= 2:                                                     # the all-zero item: every max is a tie, index 0 wins
        assert not fwd["js"][-1].any() and not fwd["jr"][-1].any()
    # routing passed in reproduces the computed one
    again = A.attend_fwd_ref(t["X"], t["Xt"], t["sent_mask"].numpy(), t["rev_mask"].numpy(), t["Ks"], t["Kr"], t["bt"], G,
                             js=fwd["js"], jr=fwd["jr"])
    assert np.array_equal(again["z"], fwd["z"])


# ------------------------------------------------------------------ 2. the whole restatement against torch.autograd in double
MODULE_CASES = [dict(B=3, G=2, Ru=3, Su=4, Ri=2, Si=5, seed=17), dict(B=2, G=1, Ru=1, Su=3, Ri=3, Si=2, seed=18),
                dict(B=2, G=3, Ru=4, Su=1, Ri=2, Si=3, seed=19)]


@pytest.mark.parametrize("c", MODULE_CASES, ids=lambda c: "B{B}G{G}_{Ru}x{Su}_{Ri}x{Si}".format(**c))
def test_restatement_equals_autograd_over_the_module_composition(c):
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    B, G, Ru, Su, Ri, Si = (c[k] for k in ("B", "G", "Ru", "Su", "Ri", "Si"))
    F, P = 10, c["B"] * c["G"]
    torch.manual_seed(c["seed"])
    model = quiet(AHN, F, F, 3, 5, 6, 30, None, dropout=0.0, item_review_num=Ri).double()
    with torch.no_grad():
        for prm in model.parameters():
            prm.copy_(torch.randn_like(prm) * 0.4)
    sa, ra, trans = model.unbalanced_sentence_aggregator, model.unbalanced_review_aggregator, model.user_review_trans_layer
    Wt, bt, Ws, Wr = trans[0].weight, trans[0].bias, sa.bilinear.weight, ra.bilinear.weight
    X = torch.randn(B, Ru, Su, F, dtype=torch.float64, requires_grad=True)
    Y = torch.randn(P, Ri, Si, F, dtype=torch.float64, requires_grad=True)
    um, im = torch.rand(B, Ru, Su) < 0.7, torch.ones(P, Ri, Si, dtype=torch.bool)
    im[1::2, 0, Si - 1] = False         # at most ONE masked sentence per item: two would be two all-zero rows of Ks, a tie at 0
    um[:, :, 0] = True
    um[0, 0] = False                    # a fully masked user review (the only one when Ru == 1)
    um[1] = False                       # a user with no live review
    uM, iM = um.any(-1), im.any(-1)
    dz = torch.randn(P, F, dtype=torch.float64)
    leaves = [X, Y, Wt, bt, Ws, Wr]

    # the module composition on the expanded batch: pair g * B + b reads user row b
    ur, ir, usw, _, _ = sa(X.repeat(G, 1, 1, 1), Y, um.repeat(G, 1, 1), im)
    z_mod, _, urw, _ = ra(trans(ur), model.item_review_trans_layer(ir), uM.repeat(G, 1), iM)
    want = torch.autograd.grad((z_mod * dz).sum(), leaves)

    # the restatement: the op in numpy, the three products and the item side's own chain around it by autograd
    Yr = Y.reshape(P * Ri, Si, F)
    r_i, _, all_w = sa.item_aggregator(Yr, im.reshape(P * Ri, Si))
    Ks = ((all_w.reshape(P * Ri * Si, 1) * Yr.reshape(P * Ri * Si, F)) @ Ws.t()).view(P, Ri * Si, F)
    Kr = (model.item_review_trans_layer(r_i).reshape(P * Ri, F) @ Wr.t()).view(P, Ri, F)
    Xf = X.reshape(B, Ru * Su, F)
    Xt = Xf @ Wt.t()
    fwd = A.attend_fwd_ref(Xf, Xt, um.numpy(), uM.numpy(), Ks, Kr, bt, G)
    lead, a_min = A.routing_margins(fwd)
    assert lead >= 1e-4 and a_min >= 1e-5, (lead, a_min)               # the seeds' precondition: no tie, no relu kink nearby
    assert max_err(fwd["z"], z_mod.detach().numpy()) <= 1e-9
    assert max_err(fwd["w"], usw.detach().numpy()) <= 1e-12 and max_err(fwd["v"], urw.detach().numpy()) <= 1e-12
    g = A.attend_bwd_ref(Xf, Xt, um.numpy(), uM.numpy(), Ks, Kr, fwd, dz, G)
    outer = torch.autograd.grad([Xt, Ks, Kr], [X, Y, Wt, Ws, Wr],
                                grad_outputs=[torch.from_numpy(g[k]) for k in ("dXt", "dKs", "dKr")], allow_unused=True)
    got = dict(zip(("X", "Y", "Wt", "Ws", "Wr"), (o.numpy() for o in outer)))
    got["X"] = got["X"] + g["dX"].reshape(B, Ru, Su, F)
    got["bt"] = g["dbt"]
    for name, ref in zip(("X", "Y", "Wt", "bt", "Ws", "Wr"), want):
        assert max_err(got[name], ref.numpy()) <= 1e-9, name
    # masked_fill routes nothing through a fully masked row: the user with no live review gets no gradient through t
    assert not g["dKr"][1::B].any()


# ------------------------------------------------------------------ 3. argument validation of the C entry points
def _shape(**kw):
    from review_based_recommender_amd import _lib
    s = dict(Ru=3, Su=4, Ri=2, Si=5, F=12, K=1)
    s.update({k: v for k, v in kw.items() if k in s})
    return _lib.AhnShape(*(s[k] for k in ("Ru", "Su", "Ri", "Si", "F", "K")))


FWD_PTRS = ("X", "Xt", "sent_mask", "rev_mask", "Ks", "Kr", "bt", "z", "w", "v", "js", "jr", "p")
BWD_PTRS = ("X", "Xt", "sent_mask", "rev_mask", "Ks", "Kr", "w", "v", "js", "jr", "p", "dz", "dX", "dXt", "dKs", "dKr", "dbt_part")


def _entry(L, which, **kw):
    fn, names = (L.rbr_ahn_pair_attend_fwd, FWD_PTRS) if which == "fwd" else (L.rbr_ahn_pair_attend_bwd, BWD_PTRS)
    shape = None if kw.get("shape", 1) is None else C.byref(_shape(**kw))
    return fn(shape, kw.get("B", 2), kw.get("G", 2), *(kw.get(n, PTR) for n in names), None)


BAD_SHAPES = [dict(Ru=0), dict(Su=-1), dict(Ri=0), dict(Si=0), dict(F=0), dict(Ru=65, Su=1), dict(Su=65, Ru=1), dict(Ru=13, Su=10),
              dict(Ri=13, Si=10), dict(Ri=1 << 16, Si=1 << 16), dict(F=2049), dict(F=2048, Ru=4, Su=2), dict(F=1 << 30),
              dict(shape=None), dict(G=0), dict(G=-3), dict(B=-1), dict(B=1 << 20, G=1 << 12), dict(B=(1 << 31) - 1, G=2)]


@pytest.mark.parametrize("which", ("fwd", "bwd"))
def test_attend_entries_refuse_bad_arguments(which):
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    name = "rbr_ahn_pair_attend_" + which
    assert name in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), name)
    for kw in BAD_SHAPES + [{n: None} for n in (FWD_PTRS if which == "fwd" else BWD_PTRS)]:
        assert _entry(L, which, **kw) == BAD_ARG, kw
        assert name.encode() in L.rbr_last_error(), kw
    assert _entry(L, which, Ru=13, Su=10) == BAD_ARG and b"128" in L.rbr_last_error()       # the caps are named in the text
    assert _entry(L, which, F=2048, Ru=4, Su=2) == BAD_ARG and b"9216" in L.rbr_last_error()
    assert _entry(L, which, B=0) == 0                                                       # P = 0: no launch, no error


def test_functional_entry_refuses_cpu_tensors():
    from review_based_recommender_amd import functional as RF
    t, _ = A.make_inputs(2, 1, 2, 3, 2, 2, 8, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.ahn_pair_attend(t["X"], t["Xt"], t["sent_mask"], t["rev_mask"], t["Ks"], t["Kr"], t["bt"])


# ------------------------------------------------------------------ 4. the trainer's opt-in
AHN_TABLES = {"device_reviews": True, "ahn_tables": True}


@pytest.mark.parametrize("cfg", [
    dict(AHN_TABLES, eval_from_towers=True),
    dict(AHN_TABLES, eval_from_towers=True, rank_metrics=[10]),
    dict(AHN_TABLES, eval_from_towers=True, rank_metrics=[10], select_by="ndcg@10"),
    dict(AHN_TABLES, loss="bpr", n_neg=2, rank_metrics=[10], select_by="ndcg@10"),
    dict(AHN_TABLES, fused_pair_tail=True),
], ids=("eval_from_towers", "rank_metrics", "select_by", "bpr", "fused_pair_tail"))
def test_trainer_accepts_the_ranking_keys_with_ahn_tables(tmp_path, cfg):
    """The configuration passes every argument check: what stops the constructor is the missing GPU (RuntimeError) or, with
    one, the empty data directory (OSError) -- never a ValueError."""
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises((RuntimeError, OSError)):
        ReviewExperiment("ahn", Args(dict(cfg, data_dir=str(tmp_path))))


@pytest.mark.parametrize("key,cfg", [
    ("loss", dict(AHN_TABLES, loss="softmax", rank_metrics=[10], select_by="mrr")),
    ("neg_candidates", dict(AHN_TABLES, loss="bpr", rank_metrics=[10], select_by="mrr", neg_candidates=4)),
    ("sample_train_review", dict(AHN_TABLES, sample_train_review=True)),
    ("parallel", dict(AHN_TABLES, parallel=True)),
    ("device_cache", dict(AHN_TABLES, device_cache=True)),
])
def test_trainer_still_refuses_with_ahn_tables(tmp_path, key, cfg):
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises(ValueError, match=rf"^{key} is not available with --model ahn: \w"):
        ReviewExperiment("ahn", Args(dict(cfg, data_dir=str(tmp_path))))


def test_ahn_tables_needs_device_reviews_and_ahn(tmp_path):
    from review_based_recommender_amd.trainer import Args, ReviewExperiment
    with pytest.raises(ValueError, match="ahn_tables needs device_reviews"):
        ReviewExperiment("ahn", Args(dict(ahn_tables=True, data_dir=str(tmp_path))))
    with pytest.raises(ValueError, match="fused_pair_tail needs ahn_tables"):
        ReviewExperiment("ahn", Args(dict(device_reviews=True, fused_pair_tail=True, data_dir=str(tmp_path))))
    for kind in ("narre", "deepconn"):
        with pytest.raises(ValueError, match="valid for --model ahn"):
            ReviewExperiment(kind, Args(dict(ahn_tables=True, data_dir=str(tmp_path))))
    # without the key the refusals stand, and their text names it
    with pytest.raises(ValueError, match=r"^loss is not available with --model ahn: .*ahn_tables"):
        ReviewExperiment("ahn", Args(dict(device_reviews=True, loss="bpr", data_dir=str(tmp_path))))
