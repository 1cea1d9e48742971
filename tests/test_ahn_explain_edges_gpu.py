"""csrc/ahn_explain.hip at edge shapes against float64: functional.ahn_pair_explain on ahn_attend_ref.make_inputs' seeded inputs --
exactly the shapes, (B, G) and seeds of test_ahn_attend_edges_gpu.py -- against tests/ahn_explain_ref.py, which goes through the
vector gradients the kernel never forms.  F = 12 / 34 / 300 crosses the 32-column slice; 1, 12 against 10, 33 and 100 rows cross
the MFMA tiles; P = 1, 4, 5, 9 crosses the 4-pair tile; K = 1, 5, 10 (by (B, G)) crosses the four waves of the FM's loop.  The
tables hold B user rows and P item rows, u_rows = arange(P) % B; the ids' FM rows, the head, r', beta and the q block are seeded
at random (ahn_explain_ref.make_head).  Special rows come with the generator: a fully masked review (uniform w, ds = 0), a user
with no live review (uniform v, dt = 0), a zero padding user, an all-zero item (js = jr = 0, both match arrays exactly 0).

Tolerances are the project's edge rule: the score within 2e-6 + 2e-4 |ref|, w and v within 1e-5, every contribution tensor within
2e-6 + 2e-4 max|ref| per tensor.  The reference is evaluated under the KERNEL's routing (js, jr), after each chosen row has been
shown to attain the reference's max within 1e-5 (1 + |best|).  The generator asserts the routing and relu margins on the CPU.

Each case prints its measured maxima beside torch's own f32 composition of the same numbers on the same inputs (attend_torch, a
torch FM, autograd.grad down to the [P, rows, F] gradients, row dots)."""
import numpy as np
import pytest
import torch

import ahn_attend_ref as A
import ahn_explain_ref as E
from test_ahn_attend_edges_gpu import CASES, IDS, SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_OF = {(1, 1): 1, (5, 1): 5, (3, 3): 10, (2, 2): 10}
_BUILT = {}


def _tables(t, h):
    from review_based_recommender_amd import functional as RF
    d = lambda x: x.to(DEV)                                                              # noqa: E731
    P, Ri = h["beta"].shape
    Si = t["Ks"].shape[1] // Ri
    us = RF.AhnUserState(d(t["X"]), d(t["Xt"]), d(t["sent_mask"]), d(t["rev_mask"]), d(h["ufm"]))
    its = RF.AhnItemState(d(t["Ks"]), d(t["Kr"]), d(h["ifm"]), torch.zeros(P, Ri, Si, device=DEV), d(h["beta"]))
    head = RF.AhnPairHead(d(t["bt"]), d(h["VzT"]), d(h["vz2"]), d(h["lz"]), d(h["lin_b"]))
    extra = RF.AhnExplainRows(d(h["Rp"]), d(h["VqT"]), d(h["vq2"]), d(h["lq"]))
    return us, its, head, extra


def _case(key):
    """Inputs, tables, one run of the op, and the float64 reference under the kernel's routing: built once, left unchanged."""
    if key in _BUILT:
        return _BUILT[key]
    from review_based_recommender_amd import functional as RF
    s, B, G = key
    F, u, i = SHAPES[s]
    P = B * G
    t, _ = A.make_inputs(B, G, *u, *i, F, CASES[key])
    h = E.make_head(B, P, i[0], F, K_OF[(B, G)], CASES[key] + 1)
    tabs = _tables(t, h)
    rows = torch.arange(P, device=DEV)
    got = RF.ahn_pair_explain(*tabs, rows % B, rows)
    ref = E.explain_ref(t, h, G, js=got.user_match.view(P, -1).cpu().numpy(), jr=got.review_match.cpu().numpy())
    _BUILT[key] = (t, h, tabs, rows, got, ref)
    return _BUILT[key]


def _stack(ref, k):
    return np.stack([np.asarray(r[k], np.float64) for r in ref])


def _err(a, ref):
    return float(np.abs(a.double().cpu().numpy().reshape(ref.shape) - ref).max())


@pytest.mark.parametrize("key", list(CASES), ids=IDS)
def test_explanation_against_float64(key):
    t, h, tabs, rows, got, ref = _case(key)
    s, B, G = key
    P = B * G
    (Ru, Su), (Ri, Si) = SHAPES[s][1], SHAPES[s][2]
    assert got.score.shape == (P,) and got.user_sentences.shape == (P, Ru, Su) and got.user_sentences_fixed.shape == (P, Ru, Su)
    assert got.user_reviews.shape == (P, Ru) and got.user_text.shape == (P,) and got.item_sentence_match.shape == (P, Ri, Si)
    assert got.item_review_match.shape == (P, Ri) and got.item_reviews.shape == (P, Ri) and got.item_text.shape == (P,)
    assert got.user_match.dtype == torch.int32 and got.user_match.shape == (P, Ru, Su) and got.review_match.shape == (P, Ru)
    # the kernel's routing attains the reference's maxima (with the margins of the generator it IS the reference's)
    assert A.attains_max(_stack(ref, "S"), got.user_match.view(P, -1).cpu().numpy())
    assert A.attains_max(_stack(ref, "T"), got.review_match.cpu().numpy())
    tc = E.explain_torch(t, h, G, DEV)
    rs = _stack(ref, "score")
    line = [f"score {_err(got.score, rs):.2e} (torch {_err(tc['score'], rs):.2e})",
            f"w {_err(got.user_sent_weights, _stack(ref, 'w')):.2e} (torch {_err(tc['w'], _stack(ref, 'w')):.2e})",
            f"v {_err(got.user_review_weights, _stack(ref, 'v')):.2e} (torch {_err(tc['v'], _stack(ref, 'v')):.2e})"]
    line += [f"{k} {_err(getattr(got, k), _stack(ref, k)):.2e} / {float(np.abs(_stack(ref, k)).max()):.2e} (torch {_err(tc[k], _stack(ref, k)):.2e})"
             for k in E.FIELDS]
    print(f"{IDS[list(CASES).index(key)]}: max err " + ", ".join(line))
    assert (np.abs(got.score.double().cpu().numpy() - rs) <= 2e-6 + 2e-4 * np.abs(rs)).all()
    assert _err(got.user_sent_weights, _stack(ref, "w")) <= 1e-5 and _err(got.user_review_weights, _stack(ref, "v")) <= 1e-5
    for k in E.FIELDS:
        want = _stack(ref, k)
        assert _err(getattr(got, k), want) <= 2e-6 + 2e-4 * float(np.abs(want).max()), k
    # item rows nobody matched are exactly 0; the all-zero item: the lowest index wins every tie and nothing flows through it
    chosen = torch.zeros(P, Ri * Si, dtype=torch.bool, device=DEV).scatter_(1, got.user_match.view(P, -1).long(), True)
    assert not got.item_sentence_match.view(P, -1)[~chosen].any()
    hit = torch.zeros(P, Ri, dtype=torch.bool, device=DEV).scatter_(1, got.review_match.long(), True)
    assert not got.item_review_match[~hit].any()
    if P >= 2:
        assert not got.user_match[-1].any() and not got.review_match[-1].any()
        assert not got.item_sentence_match[-1].any() and not got.item_review_match[-1].any()
    m, M = t["sent_mask"], t["rev_mask"]
    # a fully masked review (user 0, review 0): uniform w; a user with no live review (user 1): uniform v
    assert _err(got.user_sent_weights[0, 0], np.full(Su, 1.0 / Su)) <= 1e-6 and not m[0, 0].any()
    if B >= 2:
        assert _err(got.user_review_weights[1], np.full(Ru, 1.0 / Ru)) <= 1e-6 and not M[1].any()


@pytest.mark.parametrize("key", list(CASES), ids=IDS)
def test_bits_of_the_score_kernel_and_of_the_training_op_and_of_a_second_run(key):
    from review_based_recommender_amd import functional as RF
    t, h, (us, its, head, extra), rows, got, _ = _case(key)
    s, B, G = key
    P = B * G
    score, w, v = RF.ahn_pair_score(us, its, head, rows % B, rows, weights=True)
    assert torch.equal(got.score, score) and torch.equal(got.user_sent_weights, w) and torch.equal(got.user_review_weights, v)
    _, _, _, js, jr = RF.ahn_pair_attend(us.X, us.Xt, us.sent_masks, us.rev_masks, its.Ks, its.Kr, head.bt, groups=G, saved=True)
    assert torch.equal(got.user_match.view(P, -1), js) and torch.equal(got.review_match, jr)
    again = RF.ahn_pair_explain(us, its, head, extra, rows % B, rows)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    narrow = RF.ahn_pair_explain(us, its, head, extra, (rows % B).to(torch.int32), rows.to(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(got, narrow))


@pytest.mark.parametrize("key", list(CASES), ids=IDS)
def test_a_pair_keeps_its_bits_in_another_place_and_another_launch_length(key):
    from review_based_recommender_amd import functional as RF
    t, h, (us, its, head, extra), rows, got, _ = _case(key)
    B = key[1]
    P = rows.shape[0]
    # one more pair in front and the rest reversed: every pair in another tile position, with other neighbours, in a longer launch
    order = torch.cat([rows[:1], rows.flip(0)])
    moved = RF.ahn_pair_explain(us, its, head, extra, order % B, order)
    assert all(torch.equal(a[1:].flip(0), b) for a, b in zip(moved, got))
    assert all(torch.equal(a[0], b[0]) for a, b in zip(moved, got))
    alone = RF.ahn_pair_explain(us, its, head, extra, rows[P - 1:] % B, rows[P - 1:])
    assert all(torch.equal(a, b[P - 1:]) for a, b in zip(alone, got))


def test_a_row_outside_its_table_is_explained_as_row_0_and_is_recorded():
    from review_based_recommender_amd import functional as RF
    key = ("f12_3x4_2x5", 5, 1)
    _, _, (us, its, head, extra), _, _, _ = _case(key)
    RF.check_id_errors(DEV)
    bad = RF.ahn_pair_explain(us, its, head, extra, torch.tensor([5, 1], device=DEV), torch.tensor([2, -1], device=DEV))
    good = RF.ahn_pair_explain(us, its, head, extra, torch.tensor([0, 1], device=DEV), torch.tensor([2, 0], device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(bad, good))
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)                                     # the record is cleared


def test_zero_pairs_launch_nothing():
    from review_based_recommender_amd import functional as RF
    _, _, (us, its, head, extra), _, _, _ = _case(("f12_3x4_2x5", 5, 1))
    none = RF.ahn_pair_explain(us, its, head, extra, torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert none.score.shape == (0,) and none.user_sentences.shape == (0, 3, 4) and none.item_sentence_match.shape == (0, 2, 5)

