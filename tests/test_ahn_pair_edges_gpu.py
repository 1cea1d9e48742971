"""csrc/ahn_pair.hip at edge shapes against float64: both entry points (functional.ahn_pair_score / ahn_pair_score_dense) on
seeded state tensors against tests/ahn_pair_ref.py::pair_tail_ref, at the smallest shapes that cross each constant of the
kernel -- the 32-column slice of F (12: below one slice; 34: one slice and a remainder; 300: the default), the 32-row MFMA tiles
of both sides (1 row, 12 against 10, 33, 100), the 4-pair workgroup tile (P = 1, 5, 9; dense I = 1, 4, 5) and K = 1 / 6.

Tolerances are the project's: scores within FWD_TOL = 1e-4 of tests/test_ahn_gpu.py, weights within 1e-5.  The forward is
continuous in its inputs (max and softmax route no gradient here), so there is no margin precondition.  Largest errors measured
on an MI355X over all cases: score 7.7e-8, sentence weights 3.9e-8, review weights 9.9e-9 (each case prints its own)."""
import numpy as np
import pytest
import torch

import ahn_pair_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, W_TOL = 1e-4, 1e-5
TILE = 4                     # pairs per workgroup (kAhnTile)

# name -> F, (Ru, Su), (Ri, Si), K, users, items, pairs of the ids entry.  F = 300 stays at P <= 8 in either entry.
CASES = {
    "f12_1x1": dict(F=12, u=(1, 1), i=(1, 1), K=1, U=3, I=1, P=1),
    "f12_3x4_2x5": dict(F=12, u=(3, 4), i=(2, 5), K=6, U=4, I=TILE + 1, P=TILE + 1),
    "f34_33rows": dict(F=34, u=(3, 11), i=(11, 3), K=6, U=4, I=TILE, P=2 * TILE + 1),
    "f34_10x10": dict(F=34, u=(10, 10), i=(10, 10), K=1, U=4, I=TILE + 1, P=TILE + 1),
    "f300_10x10": dict(F=300, u=(10, 10), i=(10, 10), K=6, U=4, I=TILE + 1, P=TILE + 1),
    "f300_3x4_2x5": dict(F=300, u=(3, 4), i=(2, 5), K=6, U=4, I=TILE, P=1),
}
_BUILT = {}


def _case(name):
    """Seeded states on the device, the pair list and the float64 reference of every (user, item) pair: built once, left unchanged.
    User 0 / item 0 are padding rows (zero vectors, every mask off); user 1 has a fully masked review, user 2 no live review."""
    if name in _BUILT:
        return _BUILT[name]
    from review_based_recommender_amd import functional as RF
    c = CASES[name]
    (Ru, Su), (Ri, Si), F, K, U, I = c["u"], c["i"], c["F"], c["K"], c["U"], c["I"]
    g = torch.Generator().manual_seed(500 + F + Ru * Su)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale          # noqa: E731
    X, Xt = rnd(U, Ru * Su, F), rnd(U, Ru * Su, F, scale=0.5)
    sm = torch.rand(U, Ru, Su, generator=g) < 0.7
    sm[1, 0] = False
    if U > 2:
        sm[2] = False
    X[0], Xt[0], sm[0] = 0.0, 0.0, False
    us = RF.AhnUserState(X, Xt, sm, sm.any(-1), rnd(U, K + 2, scale=0.3))
    Ks, Kr = rnd(I, Ri * Si, F, scale=2.0 / F ** 0.5), rnd(I, Ri, F, scale=2.0 / F ** 0.5)
    Ks[0], Kr[0] = 0.0, 0.0
    its = RF.AhnItemState(Ks, Kr, rnd(I, K + 2, scale=0.3), torch.zeros(I, Ri, Si), torch.zeros(I, Ri))
    head = RF.AhnPairHead(rnd(F, scale=0.2), rnd(K, F, scale=0.2), rnd(F, scale=0.05).abs(), rnd(F, scale=0.2), rnd(1))
    u_rows = torch.arange(c["P"]) % U
    i_rows = (torch.arange(c["P"]) * 3 + 1) % I
    if c["P"] > 1:
        u_rows[1], i_rows[1] = 0, 0                                                     # the padding pair
    hd = {k: v.double().numpy() for k, v in head._asdict().items()}
    ref = {}
    for u in range(U):
        for i in range(I):
            if c["F"] == 300 and not (u == 1 or (u, i) in set(zip(u_rows.tolist(), i_rows.tolist()))):
                continue                                                                # F = 300: only the pairs that are run
            ud = dict(X=X[u].double().numpy(), Xt=Xt[u].double().numpy(), sent_mask=sm[u].numpy(), rev_mask=sm[u].any(-1).numpy(),
                      fm=us.fm[u].double().numpy())
            idt = dict(Ks=Ks[i].double().numpy(), Kr=Kr[i].double().numpy(), fm=its.fm[i].double().numpy())
            ref[(u, i)] = R.pair_tail_ref(ud, idt, hd)
    dev = lambda nt: type(nt)(*(t.to(DEV) for t in nt))                                 # noqa: E731
    _BUILT[name] = (c, dev(us), dev(its), dev(head), u_rows, i_rows, ref)
    return _BUILT[name]


def _errors(ref, pairs, scores, w=None, v=None):
    es = max(abs(float(scores[p]) - ref[k][0]) for p, k in enumerate(pairs))
    ew = max(float(np.abs(w[p].double().numpy() - ref[k][1]).max()) for p, k in enumerate(pairs)) if w is not None else 0.0
    ev = max(float(np.abs(v[p].double().numpy() - ref[k][2]).max()) for p, k in enumerate(pairs)) if v is not None else 0.0
    return es, ew, ev


@pytest.mark.parametrize("name", sorted(CASES))
def test_ids_entry_against_float64(name):
    from review_based_recommender_amd import functional as RF
    c, us, its, head, u_rows, i_rows, ref = _case(name)
    u, i = u_rows.to(DEV), i_rows.to(DEV)
    scores, w, v = RF.ahn_pair_score(us, its, head, u, i, weights=True)
    pairs = list(zip(u_rows.tolist(), i_rows.tolist()))
    es, ew, ev = _errors(ref, pairs, scores.cpu(), w.cpu(), v.cpu())
    print(f"{name}: ids entry max err score {es:.3e} sentence weights {ew:.3e} review weights {ev:.3e}")
    assert scores.shape == (c["P"],) and w.shape == (c["P"], *c["u"]) and v.shape == (c["P"], c["u"][0])
    assert es <= FWD_TOL and ew <= W_TOL and ev <= W_TOL
    # fully masked review / user without a live review: uniform weights, as in the reference
    for p, (a, _) in enumerate(pairs):
        if a == 1:
            assert torch.allclose(w[p, 0], torch.full_like(w[p, 0], 1.0 / c["u"][1]), atol=1e-7)
        if a in (0, 2):
            assert torch.allclose(v[p], torch.full_like(v[p], 1.0 / c["u"][0]), atol=1e-7)
    # the scores do not depend on asking for the weights, on the index width or on the run
    plain = RF.ahn_pair_score(us, its, head, u, i)
    narrow = RF.ahn_pair_score(us, its, head, u.to(torch.int32), i.to(torch.int32))
    again = RF.ahn_pair_score(us, its, head, u, i, weights=True)
    assert torch.equal(plain, scores) and torch.equal(narrow, scores)
    assert all(torch.equal(a, b) for a, b in zip(again, (scores, w, v)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_entry_against_float64_and_the_ids_entry_bit_for_bit(name):
    from review_based_recommender_amd import functional as RF
    c, us, its, head, _, _, ref = _case(name)
    users = [1] if c["F"] == 300 and c["I"] > TILE else ([1, 1] if c["F"] == 300 else list(range(c["U"])) + [1])
    rows = torch.tensor(users, device=DEV)
    block = RF.ahn_pair_score_dense(us, its, head, rows)
    assert block.shape == (len(users), c["I"])
    pairs = [(u, i) for u in users for i in range(c["I"])]
    es, _, _ = _errors(ref, pairs, block.cpu().reshape(-1))
    print(f"{name}: dense entry max err score {es:.3e}")
    assert es <= FWD_TOL
    assert torch.equal(block, RF.ahn_pair_score_dense(us, its, head, rows))                          # two runs
    pu = torch.tensor([p[0] for p in pairs], device=DEV)
    pi = torch.tensor([p[1] for p in pairs], device=DEV)
    assert torch.equal(RF.ahn_pair_score(us, its, head, pu, pi), block.reshape(-1))                  # the same bits in both entries
    if c["F"] != 300:
        assert torch.equal(RF.ahn_pair_score_dense(us, its, head), block[:c["U"]])                   # u_rows None: the table's rows


@pytest.mark.parametrize("name", ["f12_3x4_2x5", "f34_33rows", "f300_10x10"])
def test_a_pair_s_bits_do_not_depend_on_its_neighbours(name):
    from review_based_recommender_amd import functional as RF
    c, us, its, head, u_rows, i_rows, _ = _case(name)
    u, i = u_rows.to(DEV), i_rows.to(DEV)
    scores, w, v = RF.ahn_pair_score(us, its, head, u, i, weights=True)
    # the same pairs in reverse order (other tile positions, other neighbours), and each alone
    rs, rw, rv = RF.ahn_pair_score(us, its, head, u.flip(0), i.flip(0), weights=True)
    assert torch.equal(rs.flip(0), scores) and torch.equal(rw.flip(0), w) and torch.equal(rv.flip(0), v)
    for p in (0, c["P"] - 1):
        alone = RF.ahn_pair_score(us, its, head, u[p:p + 1], i[p:p + 1], weights=True)
        assert torch.equal(alone[0], scores[p:p + 1]) and torch.equal(alone[1], w[p:p + 1]) and torch.equal(alone[2], v[p:p + 1])


def test_a_row_outside_its_table_scores_as_row_0_and_is_recorded():
    from review_based_recommender_amd import functional as RF
    c, us, its, head, _, _, _ = _case("f12_3x4_2x5")
    RF.check_id_errors(DEV)
    bad = RF.ahn_pair_score(us, its, head, torch.tensor([c["U"], 1], device=DEV), torch.tensor([2, -1], device=DEV))
    good = RF.ahn_pair_score(us, its, head, torch.tensor([0, 1], device=DEV), torch.tensor([2, 0], device=DEV))
    assert torch.equal(bad, good)
    with pytest.raises(IndexError):
        RF.check_id_errors(DEV)
    RF.check_id_errors(DEV)                                     # the record is cleared
