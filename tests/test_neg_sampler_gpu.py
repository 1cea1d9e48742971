"""rbr_sample_negatives on the device against the integer restatement of its draw (tests/bpr_ref.py): every output must be the
same integers, the call number must advance by one per launch -- also for a launch replayed from a graph -- and no negative may
be the pair's own item, an item its user has seen, or an item outside [item_lo, I)."""
import numpy as np
import pytest
import torch

from bpr_ref import sample_negatives_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _state(call):
    return torch.tensor([call, 0], dtype=torch.int64, device=DEV)


def _crowd(I, item_lo):
    """Six users over I items: 0 empty row; 1 a few items; 2 everything but item_lo (a walk that starts above it wraps round);
    3 everything; 4 everything but item I - 2; 5 a few items."""
    every = list(range(item_lo, I))
    rows = [[], [item_lo + 1, item_lo + 2, I - 3, I - 1], [x for x in every if x != item_lo], every, [x for x in every if x != I - 2],
            [item_lo, I - 1]]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    items = np.array([x for r in rows for x in r], dtype=np.int32)
    return off, items, rows


def _pairs(B, I, item_lo, rows, seed):
    """B pairs that meet every kind of row: positives inside and outside their user's seen row, the one unseen item as the
    positive (user 4: nothing is left), and user ids outside [0, U) on both sides."""
    rng = np.random.default_rng(seed)
    u = rng.choice(np.array([0, 1, 2, 3, 4, 5, -1, 6, 99]), size=B)
    i = rng.integers(item_lo, I, size=B)
    if B >= 16:
        u[:6] = [1, 1, 4, 4, 2, 3]
        i[:6] = [rows[1][0], item_lo, I - 2, item_lo, I - 1, I - 1]      # seen, unseen, the last unseen one, seen, seen, seen
    else:
        u[0], i[0] = 1, rows[1][0]
    return u.astype(np.int64), i.astype(np.int64)


def _launch(u, i, n_neg, I, seen, state, **kw):
    from review_based_recommender_amd import functional as RF
    dev_seen = None if seen is None else (torch.from_numpy(seen[0]).to(DEV), torch.from_numpy(seen[1]).to(DEV))
    return RF.sample_negatives(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), n_neg, I, dev_seen, state=state, **kw)


def _same(got, ref):
    for g, r in zip(got, ref):
        assert torch.equal(g.cpu(), torch.from_numpy(r))


def _check_never_forbidden(u, i, n_neg, I, item_lo, rows, got, replace_id):
    B = len(u)
    i_out, valid = got[1].cpu().numpy(), got[2].cpu().numpy()
    for j in range(n_neg):
        for b in range(B):
            c, v = int(i_out[(j + 1) * B + b]), float(valid[j * B + b])
            row = rows[int(u[b])] if rows is not None and 0 <= int(u[b]) < len(rows) else []
            if v == 1.0:
                assert item_lo <= c < I and c != int(i[b]) and c not in row, (b, j, c)
            else:
                assert v == 0.0 and c == replace_id
                assert all(x == int(i[b]) or x in row for x in range(item_lo, I)), (b, j)      # really nothing to draw


@pytest.mark.parametrize("max_tries", [16, 1])
@pytest.mark.parametrize("with_seen", [True, False])
@pytest.mark.parametrize("item_lo", [0, 1])
@pytest.mark.parametrize("B,n_neg", [(1, 1), (257, 3)])
def test_sampler_equals_the_integer_restatement(B, n_neg, item_lo, with_seen, max_tries):
    I, seed, call, replace_id = 11, 77, 4, item_lo
    off, items, rows = _crowd(I, item_lo)
    seen = (off, items) if with_seen else None
    u, i = _pairs(B, I, item_lo, rows, seed=B + n_neg)
    state = _state(call)
    got = _launch(u, i, n_neg, I, seen, state, seed=seed, item_lo=item_lo, max_tries=max_tries, replace_id=replace_id)
    ref = sample_negatives_ref(u, i, n_neg, I, seen, seed, call, item_lo=item_lo, max_tries=max_tries, replace_id=replace_id)
    _same(got, ref)
    assert state.tolist() == [call + 1, 0]          # 257 * 3 draws are four workgroups: the last one to finish moved the call on
    _check_never_forbidden(u, i, n_neg, I, item_lo, rows if with_seen else None, got, replace_id)
    if with_seen and B > 1:
        valid = got[2].cpu().numpy().reshape(n_neg, B)
        assert valid[:, 2].max() == 0.0 and valid[:, 5].max() == 0.0      # user 4's last unseen item is the positive; user 3 saw all
        assert valid[:, 0].min() == 1.0 and got[1].cpu().numpy().reshape(1 + n_neg, B)[1:, 4].tolist() == [item_lo] * n_neg


def test_empty_seen_list_and_single_item_catalogue():
    # a CSR with no entry at all (every row empty)
    u, i = np.array([0, 1, 2], dtype=np.int64), np.array([1, 2, 3], dtype=np.int64)
    seen = (np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32))
    state = _state(0)
    _same(_launch(u, i, 2, 6, seen, state, seed=3), sample_negatives_ref(u, i, 2, 6, seen, 3, 0))
    # I - item_lo = 1 and that item is the positive: replace_id, valid 0 -- whichever replace_id
    for replace_id in (0, 1):
        u, i = np.array([0, 5], dtype=np.int64), np.array([1, 1], dtype=np.int64)
        got = _launch(u, i, 2, 2, None, _state(9), seed=3, item_lo=1, replace_id=replace_id)
        _same(got, sample_negatives_ref(u, i, 2, 2, None, 3, 9, item_lo=1, replace_id=replace_id))
        assert got[1].tolist() == [1, 1] + [replace_id] * 4 and got[2].tolist() == [0.0] * 4 and got[0].tolist() == [0, 5] * 3


def test_calls_advance_and_a_replayed_launch_draws_like_eager_calls():
    """Two eager calls use call numbers k and k + 1; a captured launch replayed three times equals three eager calls from the same
    reseed (and the restatement's calls k, k + 1, k + 2)."""
    from review_based_recommender_amd import functional as RF
    I, n_neg, B, seed, k = 11, 3, 257, 21, 5
    off, items, rows = _crowd(I, 1)
    u, i = _pairs(B, I, 1, rows, seed=1)
    refs = [sample_negatives_ref(u, i, n_neg, I, (off, items), seed, k + s) for s in range(3)]
    state = _state(k)
    eager = []
    for s in range(3):
        eager.append([t.clone() for t in _launch(u, i, n_neg, I, (off, items), state, seed=seed)])
        _same(eager[-1], refs[s])
    assert state.tolist() == [k + 3, 0]
    assert not torch.equal(eager[0][1], eager[1][1])

    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    seen = (torch.from_numpy(off).to(DEV), torch.from_numpy(items).to(DEV))
    out = (torch.zeros((1 + n_neg) * B, dtype=torch.int64, device=DEV), torch.zeros((1 + n_neg) * B, dtype=torch.int64, device=DEV),
           torch.zeros(n_neg * B, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        RF.sample_negatives(ud, idv, n_neg, I, seen, state=state, seed=seed, out=out)
    state.copy_(_state(k))                       # "reseed": the recorded launch reads the call number from the device
    for s in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for g, e in zip(out, eager[s]):
            assert torch.equal(g, e), s
    assert state.tolist() == [k + 3, 0]


def test_uniform_over_the_eligible_items_on_the_device():
    """The condition of tests/test_bpr_host.py on the device's own output: 7 eligible items, 28672 draws, every count within
    4 sigma (sigma = 59.3) of 4096; and the crowded row returns only its two unseen items."""
    B, n_neg = 4096, 7
    u, i = np.ones(B, dtype=np.int64), np.full(B, 3, dtype=np.int64)
    got = _launch(u, i, n_neg, 9, None, _state(0), seed=0, item_lo=1)
    _same(got, sample_negatives_ref(u, i, n_neg, 9, None, 0, 0, item_lo=1))
    counts = torch.bincount(got[1][B:], minlength=9).cpu().numpy()
    assert counts[0] == counts[3] == 0
    dev = np.abs(counts[[1, 2, 4, 5, 6, 7, 8]] - B * n_neg / 7) / 59.3
    print("device counts", counts.tolist(), "worst deviation %.2f sigma" % dev.max())
    assert dev.max() <= 4.0
    seen = (np.array([0, 0, 5], dtype=np.int64), np.array([1, 3, 4, 6, 8], dtype=np.int32))
    u, i = np.ones(256, dtype=np.int64), np.full(256, 2, dtype=np.int64)
    got = _launch(u, i, 4, 9, seen, _state(3), seed=5, item_lo=1)
    _same(got, sample_negatives_ref(u, i, 4, 9, seen, 5, 3, item_lo=1))
    assert set(got[1][256:].tolist()) == {5, 7} and float(got[2].min()) == 1.0
