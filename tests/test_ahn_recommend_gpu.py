"""AHN's query surface on the GPU: the pair kernel fed with the reference fixtures' own sentence vectors, AhnRecommender's whole
chain (tables by the plain rule -> encoder -> states -> kernel) against AHN.forward on plain-gathered batches, and the
consistency of score / score_all / topk / rank / evaluate.  Tolerances: scores within FWD_TOL = 1e-4 of tests/test_ahn_gpu.py,
weights within 1e-5.  Each comparison prints its largest error, beside the error of torch's own f32 `aggregate` on the same
inputs where there is one."""
import os

import numpy as np
import pytest
import torch

import make_sentence_dataset
import synth_ahn
from helpers import golden, max_err, quiet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FWD_TOL, W_TOL = 1e-4, 1e-5
WEIGHT_KEYS = ("user_sent_weights", "item_sent_weights", "user_review_weights", "item_review_weights")


def _ahn(*a, **k):
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    return quiet(AHN, *a, **k)


# ------------------------------------------------------------------ the kernel against the reference's own run
@pytest.mark.parametrize("name", ("tiny", "small"))
def test_kernel_on_the_fixture_sentence_vectors(golden_dir, name):
    from review_based_recommender_amd import functional as RF
    g = golden(golden_dir, "ahn_" + name)
    c = synth_ahn.AHN_CFGS[name]
    B, Rn, S, H = c["B"], c["R"], c["S"], c["H"]
    model = _ahn(c["E"], H, c["K"], c["U"], c["I"], c["V"], None, dropout=0.0, item_review_num=Rn)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    model.to(DEV).train()
    t = {k: torch.from_numpy(g["in/" + k]).to(DEV) for k in synth_ahn.FORWARD_KEYS}
    u_sents = torch.from_numpy(g["user_sents"]).float().view(B, Rn, S, H).to(DEV)
    i_sents = torch.from_numpy(g["item_sents"]).float().view(B, Rn, S, H).to(DEV)
    us = model.user_state(u_sents, t["user_sent_masks"], t["user_review_masks"], t["user_ids"])          # one state row per example
    its = model.item_state(i_sents, t["item_sent_masks"], t["item_review_masks"], t["item_ids"])
    assert model.training                                                                              # the mode is restored
    rows = torch.arange(B, device=DEV)
    score, w, v = RF.ahn_pair_score(us, its, model.pair_head(), rows, rows, weights=True)
    got = dict(zip(WEIGHT_KEYS, (w, its.item_sent_weights, v, its.item_review_weights)))
    model.eval()
    with torch.no_grad():
        eager = model.aggregate(u_sents, i_sents, t["user_sent_masks"], t["item_sent_masks"], t["user_review_masks"],
                                t["item_review_masks"], t["user_ids"], t["item_ids"])
    print(f"{name}: score err kernel {max_err(score.cpu().numpy(), g['pred_eval']):.3e} / torch f32 aggregate "
          f"{max_err(eager[0].cpu().numpy(), g['pred_eval']):.3e}")
    for k, e in zip(WEIGHT_KEYS, eager[1:]):
        print(f"{name}: {k} err kernel {max_err(got[k].cpu().numpy(), g[k]):.3e} / torch f32 aggregate {max_err(e.cpu().numpy(), g[k]):.3e}")
    assert max_err(score.cpu().numpy(), g["pred_eval"]) <= FWD_TOL
    for k in WEIGHT_KEYS:
        assert max_err(got[k].cpu().numpy(), g[k]) <= W_TOL, k
    # every example's user against every example's item: the dense entry, the diagonal is the pairs above bit for bit
    block = RF.ahn_pair_score_dense(us, its, model.pair_head())
    assert torch.equal(block.diagonal(), score)


# ------------------------------------------------------------------ the whole chain on a written sentence split
E_H, K_FM = 12, 4


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """(info, cache, model, recommender refreshed once, ids that own a full-length sentence per side): left unchanged."""
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd.recommend import AhnRecommender
    data_dir = str(tmp_path_factory.mktemp("ahn_split"))
    info = make_sentence_dataset.write_sentence_split(data_dir)
    ds = D.SentenceDataset(data_dir, "train")
    cache = D.DeviceSentenceCache(ds, DEV)
    torch.manual_seed(5)
    model = _ahn(E_H, E_H, K_FM, info["user_num"], info["item_num"], info["vocab"], None, dropout=0.0, item_review_num=info["rv_num"]).to(DEV)
    model.train()
    rec = AhnRecommender(model, cache)
    assert rec.stale
    rec.refresh(chunk=5)                       # 12 users / 10 items in chunks of 5: whole chunks and a remainder
    assert not rec.stale and model.training
    R, W = info["rv_num"], info["word_num"]
    full = []
    for tab in (cache.user_table, cache.item_table):
        longest = D.sentence_masks(tab[:, :R], 0)[0].reshape(tab.shape[0], -1).max(1).values
        ids = (longest == W).nonzero().view(-1)
        assert ids.numel() > 0                 # a sentence of length word_num on this side, inside the first rv_num slots
        full.append(int(ids[0]))
    return dict(info=info, cache=cache, model=model, rec=rec, full=tuple(full), held_out=D.load_pickle(os.path.join(data_dir, "valid_exmaples.pkl")),
                train=ds.examples)


def test_whole_chain_against_forward_on_plain_gathered_batches(split):
    info, cache, model, rec = split["info"], split["cache"], split["model"], split["rec"]
    U, I = info["user_num"], info["item_num"]
    g = torch.Generator().manual_seed(9)
    worst = [0.0] * 5
    for batch in range(3):
        u = torch.cat([torch.randint(0, U, (15,), generator=g), torch.tensor([split["full"][0]])]).to(DEV)      # the last pair owns a
        i = torch.cat([torch.randint(0, I, (15,), generator=g), torch.tensor([split["full"][1]])]).to(DEV)      # full-length sentence per side
        model.eval()
        with torch.no_grad():
            want = model(*cache.feed(False).inputs(u, i))
        model.train()
        got = (rec.score(u, i), *rec.attention(u, i))
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape
            worst[k] = max(worst[k], max_err(a.cpu().numpy(), b.cpu().numpy()))
    print("whole chain vs AHN.forward: score %.3e, weights %s" % (worst[0], " ".join(f"{e:.3e}" for e in worst[1:])))
    assert worst[0] <= FWD_TOL and max(worst[1:]) <= W_TOL


def test_score_all_topk_rank_and_evaluate_are_consistent(split):
    from review_based_recommender_amd.recommend import AhnRecommender, rank_metrics
    info, rec = split["info"], split["rec"]
    U, I = info["user_num"], info["item_num"]
    u = torch.tensor([3, 1, 11, 3, 0, 7], device=DEV)
    block = rec.score_all(u)
    assert block.shape == (6, I)
    ii = torch.arange(I, device=DEV)
    for r in range(6):
        assert torch.equal(rec.score(u[r].expand(I).contiguous(), ii), block[r])                     # bit-equal to score()
    assert torch.equal(block[0], block[3])
    seen = AhnRecommender.seen_from(split["train"], U, DEV)
    cpu, off, items = block.cpu(), seen.off.cpu(), seen.items.cpu()
    for exclude in (None, seen):
        k = I + 2                                                                                    # short rows: -1 / -inf fill
        top_i, top_s = (t.cpu() for t in rec.topk(u, k, exclude))
        tgt = torch.tensor([2, 5, 0, I - 1, 4, I + 3], device=DEV)
        rank, n_cand = (t.cpu() for t in rec.rank(u, tgt, exclude))
        for r, uid in enumerate(u.tolist()):
            gone = set(items[off[uid]:off[uid + 1]].tolist()) if exclude is not None else set()
            order = sorted((j for j in range(1, I) if j not in gone), key=lambda j: (-float(cpu[r, j]), j))
            assert top_i[r].tolist() == order + [-1] * (k - len(order))
            assert top_s[r, :len(order)].tolist() == [float(cpu[r, j]) for j in order]
            assert bool(torch.isinf(top_s[r, len(order):]).all())
            t = int(tgt[r])
            if 1 <= t < I:
                with_t = sorted((j for j in range(1, I) if j not in gone or j == t), key=lambda j: (-float(cpu[r, j]), j))
                assert (int(rank[r]), int(n_cand[r])) == (with_t.index(t), len(with_t))              # the target is never excluded
            else:
                assert int(rank[r]) == -1
    # evaluate = rank_metrics of the ranks, by hand from score_all
    pairs = [(int(e[0]), int(e[1])) for e in split["held_out"]]
    got = rec.evaluate(split["held_out"], ks=(1, 3), exclude=seen, chunk=7)
    ranks, cands = [], []
    for uid, t in pairs:
        row = rec.score_all(torch.tensor([uid], device=DEV))[0].cpu()
        gone = set(items[off[uid]:off[uid + 1]].tolist())
        with_t = sorted((j for j in range(1, I) if j not in gone or j == t), key=lambda j: (-float(row[j]), j))
        ranks.append(with_t.index(t) if 1 <= t < I else -1)
        cands.append(len(with_t))
    # the hand-made ranks go through rank_metrics on evaluate's own device: a float64 sum on the host adds in another order
    # (seen: ndcg@3 differing in the 16th digit), and the ranks themselves are integers
    assert got == rank_metrics(torch.tensor(ranks, dtype=torch.int32, device=DEV), torch.tensor(cands, dtype=torch.int32, device=DEV), (1, 3))
    assert got["n"] == len(pairs) and got == rec.evaluate((torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])),
                                                          ks=(1, 3), exclude=seen)


def test_stale_flips_and_recommender_still_refuses_ahn(split):
    from review_based_recommender_amd.recommend import AhnRecommender, Recommender
    model, cache = split["model"], split["cache"]
    rec = AhnRecommender(model, user=cache.user_table[:, :cache.rv_num], item=cache.item_table[:, :cache.rv_num]).refresh()
    u, i = torch.tensor([3, 4], device=DEV), torch.tensor([1, 2], device=DEV)
    assert torch.equal(rec.score(u, i), split["rec"].score(u, i))                # per-id tables given directly: the same rows
    assert not rec.stale
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    assert rec.stale and split["rec"].stale
    split["rec"].refresh(chunk=5)
    assert not split["rec"].stale
    with pytest.raises(ValueError, match="AHN is not one of"):
        Recommender(model, user=cache.user_table, item=cache.item_table)
