"""CPU-only checks of the scoring / top-K feature (csrc/pair_score.hip, functional.pair_score*, recommend.py): exported
symbols, argument validation before any device call, the "never materialised" workspace bound, the host-side CSR builder, the
command line and the HIP-device gate.  No kernel is launched."""
import ctypes as C

import pytest
import torch

import synth
from helpers import quiet

NAMES = ("rbr_pair_score_ids", "rbr_pair_score_dense", "rbr_pair_score_topk", "rbr_pair_score_topk_ws_bytes")
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x1000        # a non-NULL pointer that is never dereferenced: every check below fails before the first device call


def test_symbols_are_exported_and_bound():
    from review_based_recommender_amd import _lib
    handle = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(handle, n), n
        assert n in _lib.SIGNATURES, n
    assert (_lib.SCORE_FM, _lib.SCORE_DOT) == (0, 1)


def _topk(L, mode=0, Nu=4, Ni=10, K=8, k=3, item_lo=1, ul=P, il=P, h=P, g=P, ub=P, ib=P, off=None, items=None, nnz=0, rows=None,
          n_rows=0, out_item=P, out_score=P, ws=P):
    return L.rbr_pair_score_topk(mode, Nu, Ni, K, k, item_lo, ul, il, h, g, ub, ib, off, items, nnz, rows, n_rows, out_item,
                                 out_score, ws, None)


@pytest.mark.parametrize("kw,code", [
    (dict(ul=None), BAD_ARG), (dict(il=None), BAD_ARG), (dict(h=None), BAD_ARG), (dict(g=None), BAD_ARG),
    (dict(Nu=0), BAD_ARG), (dict(Nu=-3), BAD_ARG), (dict(Ni=0), BAD_ARG), (dict(K=0), BAD_ARG), (dict(K=-1), BAD_ARG),
    (dict(k=0), BAD_ARG), (dict(k=-5), BAD_ARG), (dict(k=129), UNSUPPORTED), (dict(K=1 << 20), UNSUPPORTED),
    (dict(item_lo=10), BAD_ARG), (dict(item_lo=11), BAD_ARG), (dict(item_lo=-1), BAD_ARG),
    (dict(off=P), BAD_ARG), (dict(items=P), BAD_ARG), (dict(nnz=4), BAD_ARG), (dict(off=P, items=P, nnz=-1), BAD_ARG),
    (dict(rows=P, n_rows=4), BAD_ARG), (dict(off=P, items=P, rows=P, n_rows=0), BAD_ARG),
    (dict(out_item=None), BAD_ARG), (dict(out_score=None), BAD_ARG), (dict(ws=None), BAD_ARG), (dict(mode=2), BAD_ARG),
])
def test_topk_refuses_bad_arguments_before_touching_a_device(kw, code):
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    assert _topk(L, **kw) == code, kw
    assert len(L.rbr_last_error()) > 0
    with pytest.raises(RuntimeError, match="failed"):
        _lib.check(code, "rbr_pair_score_topk")


def test_dot_mode_needs_no_head_parameters_but_still_validates():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    # h / g / ub / ib NULL are fine in the dot mode: the refusal below is the k range, not a missing head
    assert _topk(L, mode=1, h=None, g=None, ub=None, ib=None, k=129) == UNSUPPORTED
    assert _topk(L, mode=1, h=None, g=None, ub=None, ib=None, ul=None) == BAD_ARG


def test_ids_and_dense_refuse_bad_arguments():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    ids = lambda **k: L.rbr_pair_score_ids(k.get("mode", 0), k.get("B", 4), k.get("K", 8), k.get("ul", P), k.get("U", 5), k.get("il", P),  # noqa: E731
                                           k.get("I", 6), k.get("u", P), k.get("i", P), k.get("h", P), P, None, None, k.get("out", P),
                                           None, None)
    for kw in (dict(B=0), dict(K=0), dict(U=0), dict(I=-1), dict(ul=None), dict(il=None), dict(u=None), dict(i=None), dict(h=None),
               dict(out=None), dict(mode=7)):
        assert ids(**kw) == BAD_ARG, kw
    assert ids(K=1 << 20) == UNSUPPORTED
    dense = lambda **k: L.rbr_pair_score_dense(k.get("mode", 0), k.get("Nu", 4), k.get("Ni", 6), k.get("K", 8), k.get("ul", P),  # noqa: E731
                                               k.get("il", P), k.get("h", P), k.get("g", P), None, None, k.get("out", P), None)
    for kw in (dict(Nu=0), dict(Ni=0), dict(K=0), dict(ul=None), dict(il=None), dict(h=None), dict(g=None), dict(out=None)):
        assert dense(**kw) == BAD_ARG, kw


def test_workspace_is_a_small_fraction_of_the_score_matrix():
    """The "never materialised" condition: at 4096 users x 100 003 items the workspace is at most 1/16 of the [Nu, Ni] f32
    matrix, and it is Nu * k * 8 bytes times a bounded number of item slices."""
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    Nu, Ni, K, k = 4096, 100003, 32, 10
    ws = L.rbr_pair_score_topk_ws_bytes(Nu, Ni, K, k)
    assert 0 < ws <= Nu * Ni * 4 // 16
    assert ws % (Nu * k * 8) == 0 and 1 <= ws // (Nu * k * 8) <= 64
    for Nu_, Ni_ in ((1, 2), (1, 1 << 30), (1 << 20, 3), (257, 1003)):
        w = L.rbr_pair_score_topk_ws_bytes(Nu_, Ni_, 32, 128)
        assert 0 < w <= Nu_ * 128 * 8 * 64
    assert L.rbr_pair_score_topk_ws_bytes(0, 10, 8, 3) == 0
    assert L.rbr_pair_score_topk_ws_bytes(4, 10, 8, 0) == 0
    assert L.rbr_pair_score_topk_ws_bytes(4, 10, 8, 129) == 0
    assert b"129" in L.rbr_last_error()


def test_seen_from_builds_a_sorted_csr():
    from review_based_recommender_amd.recommend import Recommender, SeenItems
    ex = [[3, 7, 5.0, [1], [2]], [1, 4, 1.0, [1], [2]], [3, 2, 4.0, [1], [2]], [3, 7, 2.0, [1], [2]], (1, 9, 3.0), [5, 1, 3.0]]
    seen = Recommender.seen_from(ex, 6)
    assert isinstance(seen, SeenItems)
    assert seen.off.dtype == torch.int64 and seen.items.dtype == torch.int32
    assert seen.off.tolist() == [0, 0, 2, 2, 4, 4, 5]
    assert seen.items.tolist() == [4, 9, 2, 7, 1]
    empty = Recommender.seen_from([], 3)
    assert empty.off.tolist() == [0, 0, 0, 0] and empty.items.numel() == 0
    with pytest.raises(IndexError):
        Recommender.seen_from([[6, 1, 1.0]], 6)


def test_cli_arguments():
    from review_based_recommender_amd.recommend import parse_cli
    a = parse_cli(["--model", "deepconn", "--config", "cfg.json", "--checkpoint", "best_model.pt", "--k", "7", "--exclude-train",
                   "--out", "recs.jsonl"])
    assert (a.model, a.config, a.checkpoint, a.k, a.exclude_train, a.out) == ("deepconn", "cfg.json", "best_model.pt", 7, True,
                                                                              "recs.jsonl")
    b = parse_cli(["--model", "dual_att", "--config", "c", "--checkpoint", "m", "--out", "o"])
    assert b.k == 10 and b.exclude_train is False and b.chunk == 256
    for bad in (["--model", "deepconn", "--config", "c", "--checkpoint", "m", "--out", "o", "--k", "0"],
                ["--model", "deepconn", "--config", "c", "--checkpoint", "m", "--out", "o", "--k", "129"],
                ["--model", "bert", "--config", "c", "--checkpoint", "m", "--out", "o"],
                ["--model", "deepconn", "--config", "c", "--checkpoint", "m"]):
        with pytest.raises(SystemExit):
            parse_cli(bad)


def test_recommender_and_scores_refuse_cpu_tensors():
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    from review_based_recommender_amd.recommend import Recommender
    cfg = synth.DEEPCONN_CFGS["tiny"]
    m = quiet(DeepCoNNpp, cfg["U"], cfg["I"], cfg["V"], cfg["kz"], cfg["D"], cfg["H"], cfg["K"], cfg["L"], None, 0.0)
    docs_u = torch.zeros(cfg["U"], cfg["L"], dtype=torch.int32)
    docs_i = torch.zeros(cfg["I"], cfg["L"], dtype=torch.int32)
    rec = Recommender(m, user=docs_u, item=docs_i)
    assert rec.stale and rec.item_lo == 1
    with pytest.raises(RuntimeError, match="HIP device"):
        rec.refresh()
    assert m.training                                   # the mode is restored when the encode fails, too
    with pytest.raises(RuntimeError, match="refresh"):
        rec.score(torch.tensor([1]), torch.tensor([1]))
    ul, il = torch.zeros(3, 4), torch.zeros(5, 4)
    h, g = torch.zeros(4, 1), torch.zeros(1)
    for call in (lambda: RF.pair_score("fm", ul, il, torch.tensor([1]), torch.tensor([2]), h, g),
                 lambda: RF.pair_score_dense("fm", ul, il, h, g),
                 lambda: RF.pair_score_topk("dot", ul, il, 2)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(ValueError):
        RF.pair_score_dense("cosine", ul, il)
    with pytest.raises(ValueError):
        Recommender(torch.nn.Linear(2, 2), user=docs_u, item=docs_i)
    with pytest.raises(ValueError):
        Recommender(m, user=docs_u.view(cfg["U"], 1, cfg["L"]), item=docs_i.view(cfg["I"], 1, cfg["L"]))


def test_eval_from_towers_is_validated_by_the_trainer_defaults():
    from review_based_recommender_amd import trainer
    assert trainer.DEFAULTS["eval_from_towers"] is False
