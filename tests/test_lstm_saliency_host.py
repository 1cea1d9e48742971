"""The BiLSTM word saliency without a GPU: the float64 restatement (tests/lstm_saliency_ref.py) against float64 autograd's
<dx_t, x_t> through the same loops -- the identity <W_ih^T dpre, x> = <dpre, W_ih x> the kernel rests on --, the declaration,
binding and host-side refusals of rbr_lstm_seq_saliency, the functional entries' device gate, AhnRecommender.words before
refresh(), and the --words rules of the command line.  No kernel is launched."""
import ctypes as C
import os
import re

import pytest
import torch

import lstm_ref as R
import lstm_saliency_ref as S
from helpers import quiet

F64 = torch.float64
BAD_ARG, UNSUPPORTED = -1, -2
PTR = 0x1000      # a non-NULL pointer that is never dereferenced: every check below fails before the first device call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rbr_lstm_seq_saliency"

CASES = {                                   # (N, T, E, Hh, lengths): 0, 1 and T are present
    "mixed_0_1_T": (6, 5, 4, 3, [0, 1, 5, 3, 0, 2]),
    "longest_below_T": (5, 7, 3, 2, [4, 0, 1, 4, 2]),
    "all_full": (3, 4, 5, 3, [4, 4, 4]),
    "single_step": (2, 1, 2, 1, [1, 0]),
    "all_empty": (3, 4, 2, 2, [0, 0, 0]),
}


def _setup(name):
    N, T, E, Hh, lens = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    params = [torch.randn(s, generator=g, dtype=F64) * 0.6 for s in ((4 * Hh, E), (4 * Hh, Hh), (4 * Hh,), (4 * Hh,)) * 2]
    x = torch.randn(N, T, E, generator=g, dtype=F64)
    lengths = torch.tensor(lens, dtype=torch.int64)
    _, argmax = R.trimmed_max(R.bilstm(x, params, lengths), lengths, R.t_out_of(lengths, T))
    return x, params, lengths, argmax, torch.randn(N, 2 * Hh, generator=g, dtype=F64)


# ------------------------------------------------------------------ 1. the restatement against float64 autograd down to x
@pytest.mark.parametrize("name", sorted(CASES))
def test_dpre_dot_xw_equals_autograd_gradient_times_input(name):
    x, params, lengths, argmax, d_pooled = _setup(name)
    N, T, _ = x.shape
    ref = S.word_saliency(x, params, lengths, argmax, d_pooled)
    want = S.grad_times_input(x, params, lengths, argmax, d_pooled)
    assert ref["words"].shape == (N, T, 2)
    assert float((ref["words"] - want).abs().max()) <= 1e-12 * (1.0 + float(want.abs().max()))
    for n in range(N):                                   # nothing behind a sequence's end, nothing in an empty row
        assert float(ref["words"][n, int(lengths[n]):].abs().sum()) == 0.0
        assert float(ref["abs"][n, int(lengths[n]):].sum()) == 0.0
    if int(lengths.max()) > 0:
        assert float(want.abs().max()) > 0.0              # the case is not vacuous
    # the biases take no share: with them in the second operand the identity fails wherever a bias is non-zero
    with_bias = (ref["dpre"] * R.xproj_of(x, params)).view(N, T, 2, -1).sum(-1)
    if int(lengths.max()) > 0:
        assert float((with_bias - want).abs().max()) > 1e-6
    # a unit whose argmax is -1 adds nothing
    masked = torch.where(argmax >= 0, d_pooled, torch.zeros_like(d_pooled))
    assert torch.equal(S.word_saliency(x, params, lengths, argmax, masked)["words"], ref["words"])
    assert float(S.error_bound(ref, params[1].shape[1]).min()) >= 0.0


# ------------------------------------------------------------------ 2. the entry: declared, bound, exported, and its refusals
def test_entry_is_declared_bound_and_exported():
    from review_based_recommender_amd import _lib
    header = open(os.path.join(ROOT, "include", "rbr_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 12
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    assert hasattr(_lib.lib(), NAME)


def _saliency(L, N=4, T=5, Hh=3, **kw):
    names = ("w_hh_fwd", "w_hh_rev", "lengths", "saved", "xw", "d_pooled", "argmax", "words_out")
    return L.rbr_lstm_seq_saliency(N, T, Hh, *(kw.get(k, PTR) for k in names), None)


def test_entry_refuses_bad_arguments_before_any_launch():
    from review_based_recommender_amd import _lib
    L = _lib.lib()
    for k in ("w_hh_fwd", "w_hh_rev", "lengths", "saved", "xw", "d_pooled", "argmax", "words_out"):
        assert _saliency(L, **{k: None}) == BAD_ARG and b"null pointer" in L.rbr_last_error(), k
    assert _saliency(L, N=-1) == BAD_ARG
    assert _saliency(L, T=0) == BAD_ARG
    assert _saliency(L, Hh=0) == BAD_ARG
    assert _saliency(L, T=1001) == UNSUPPORTED and b"1000" in L.rbr_last_error()
    assert _saliency(L, Hh=257) == UNSUPPORTED and b"256" in L.rbr_last_error()
    assert _saliency(L, N=1 << 20, T=1000, Hh=256) == UNSUPPORTED and b"2^31" in L.rbr_last_error()
    assert _saliency(L, N=0) == 0                                                      # nothing to do: no launch
    assert _saliency(L, N=0, xw=None, saved=None, words_out=None) == 0


def test_functional_entries_refuse_cpu_tensors():
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import functional as RF
    N, T, Hh, E = 2, 3, 2, 4
    w = torch.zeros(4 * Hh, Hh)
    lengths = torch.tensor([3, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.lstm_seq_states(torch.zeros(N, T, 8 * Hh), w, w, lengths, torch.tensor([3], dtype=torch.int32))
    state = RF.LstmState(torch.zeros(_lib.lib().rbr_lstm_seq_ws_bytes(N, T, Hh), dtype=torch.uint8), N, T, Hh)
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.lstm_seq_word_saliency(state, torch.zeros(N, T, 8 * Hh), w, w, lengths, torch.zeros(N, 2 * Hh),
                                  torch.zeros(N, 2 * Hh, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="xw must be"):
        RF.lstm_seq_word_saliency(state, torch.zeros(N, T, 8), w, w, lengths, torch.zeros(N, 2 * Hh), torch.zeros(N, 2 * Hh, dtype=torch.int32))
    params = [torch.zeros(4 * Hh, E), w, torch.zeros(4 * Hh), torch.zeros(4 * Hh)] * 2
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.bilstm_word_saliency(torch.zeros(N, T, E), params, lengths, lambda pooled: pooled, t_out=torch.tensor([3], dtype=torch.int32))


# ------------------------------------------------------------------ 3. the recommender before refresh()
def test_words_before_refresh_raises():
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.recommend import AhnRecommender, WordContributions
    m = quiet(AHN, 8, 8, 3, 4, 5, 20, None, item_review_num=2)
    rec = AhnRecommender(m, user=torch.zeros(4, 2, 3, 5, dtype=torch.int32), item=torch.zeros(5, 2, 3, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="refresh"):
        rec.words(torch.tensor([1]), torch.tensor([1]))
    with pytest.raises(ValueError, match="chunk"):
        rec.words(torch.tensor([1]), torch.tensor([1]), chunk=0)
    assert WordContributions._fields == ("score", "user_words", "item_words", "user_sentences", "item_sentences", "user_words_dir",
                                         "item_words_dir")


# ------------------------------------------------------------------ 4. the command line
def test_cli_words_rules():
    from review_based_recommender_amd.recommend import parse_cli
    base = ["--config", "c", "--checkpoint", "m"]
    a = parse_cli(["--model", "ahn", *base, "--out", "o", "--sentences", "3", "--words", "2"])
    assert (a.sentences, a.words) == (3, 2)
    assert parse_cli(["--model", "ahn", *base, "--out", "o", "--sentences", "3"]).words is None
    for bad in (["--model", "ahn", *base, "--out", "o", "--words", "2"],                                 # no --sentences
                ["--model", "ahn", *base, "--eval-split", "test", "--sentences", "3", "--words", "2"],    # no --out
                ["--model", "ahn", *base, "--out", "o", "--sentences", "3", "--words", "0"],
                ["--model", "ahn", *base, "--out", "o", "--sentences", "3", "--words", "-1"],
                *(["--model", m, *base, "--out", "o", "--words", "2"] for m in ("deepconn", "narre", "dual_att", "simple_siamese")),
                ["--model", "deepconn", *base, "--out", "o", "--explain", "3", "--words", "2"]):
        with pytest.raises(SystemExit):
            parse_cli(bad)
