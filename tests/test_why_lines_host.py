"""The "why" lists of recommend.py's JSON lines, element for element, on the CPU: every _why* function runs against a stub
recommender whose entry point (explain / attention / contributions / sentences / words) returns fixed small tensors in the real
NamedTuple, and the result must equal tests/golden/why_lines.json exactly.  No kernel runs.

Every stub tensor comes from integer arithmetic (no RNG): per pair the non-zero values have distinct magnitudes k / 64 (exact in
float32; the per-sentence word pick is a topk, which is not stable on ties) and about a quarter of them are exact zeros, which
the lists must drop.  3 users x k = 3 items, one row with a -1 fill and one all -1: five pairs.

    python tests/test_why_lines_host.py --write      records the fixture from the recommend.py at hand"""
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                        # pytest's conftest has done this; the --write run has not
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "why_lines.json")
U_IDS = torch.tensor([1, 2, 3])
ITEMS = torch.tensor([[2, 1, 3], [4, 2, -1], [-1, -1, -1]])
N_USERS, N_ITEMS, N = 4, 5, 2
VOCAB = {t: f"w{t}" for t in (1, 2, 3, 5, 8)}                  # ids 4, 6, 7, 9, 10 have no word: they stay ids
R, T, L = 2, 3, 5                                               # NARRE / SimpleSiamese reviews, D-ATT / DeepCoNN++ document
RU, RI, SU, SI, W = 2, 2, 2, 3, 3                               # AHN: Su != Si catches a swapped divisor


def vals(salt, B, *shape):
    """float32 [B, *shape]: within a pair every non-zero magnitude is distinct (j -> (37 j + c) % 101 + 1 over fewer than 101
    places), signs alternate in threes, a quarter are exact zeros."""
    m = 1
    for s in shape:
        m *= s
    assert m < 101
    j, b = torch.arange(m).view(1, m), torch.arange(B).view(B, 1)
    mag = (j * 37 + b * 11 + salt * 5) % 101 + 1
    sign = 1 - 2 * ((j + b + salt) % 3 == 0).to(torch.int64)
    zero = (j * 3 + b + salt) % 4 == 0
    return (torch.where(zero, torch.zeros_like(mag), mag * sign).to(torch.float32) / 64).view(B, *shape)


def ids(salt, n, *shape, mod=11):
    """int32 token / counterpart ids [n, *shape] in [0, mod), row 0 all padding."""
    m = 1
    for s in shape:
        m *= s
    t = ((torch.arange(n * m) * 31 + salt * 7) % mod).to(torch.int32).view(n, *shape)
    t[0] = 0
    return t


def explain_stub(narre):
    from review_based_recommender_amd.recommend import Explanation
    shape = (R, T) if narre else (L,)
    cache = SimpleNamespace(user=ids(1, N_USERS, *shape), item=ids(2, N_ITEMS, *shape),
                            user_rids=ids(3, N_USERS, R, mod=N_ITEMS).long() if narre else None,
                            item_rids=ids(4, N_ITEMS, R, mod=N_USERS).long() if narre else None)

    def explain(pu, pi):
        B = pu.shape[0]
        ex = Explanation(vals(0, B), vals(1, B, *shape), vals(2, B, *shape), vals(3, B), vals(4, B))
        return ex._replace(user_review_weights=vals(5, B, R), user_reviews=vals(6, B, R), item_review_weights=vals(7, B, R),
                           item_reviews=vals(8, B, R)) if narre else ex
    return SimpleNamespace(cache=cache, explain=explain)


def attention_stub():
    from review_based_recommender_amd.recommend import Attention
    cache = SimpleNamespace(user=ids(5, N_USERS, L), item=ids(6, N_ITEMS, L), user_rids=None, item_rids=None)

    def attention(pu, pi):
        B = pu.shape[0]
        side = lambda s: (vals(s, B, L), vals(s + 1, B), vals(s + 2, B, L), vals(s + 3, B, L), vals(s + 4, B), vals(s + 5, B))  # noqa: E731
        return Attention(vals(0, B), *side(10), *side(20))
    return SimpleNamespace(cache=cache, attention=attention)


def contributions_stub(with_rids):
    from review_based_recommender_amd.recommend import Contributions
    cache = SimpleNamespace(user=ids(7, N_USERS, R, T), item=ids(8, N_ITEMS, R, T),
                            user_rids=ids(9, N_USERS, R, mod=N_ITEMS).long() if with_rids else None,
                            item_rids=ids(10, N_ITEMS, R, mod=N_USERS).long() if with_rids else None)

    def contributions(pu, pi):
        B = pu.shape[0]
        return Contributions(vals(0, B), vals(31, B, R, T), vals(32, B, R, T), vals(33, B, R, T), vals(34, B, R, T), vals(35, B),
                             vals(36, B), vals(37, B, R), vals(38, B, R), vals(39, B, R), vals(40, B, R))
    return SimpleNamespace(cache=cache, contributions=contributions)


def ahn_stub():
    from review_based_recommender_amd.recommend import SentenceContributions, WordContributions

    def sentences(pu, pi):
        B = pu.shape[0]
        j, b = torch.arange(RU * SU).view(1, RU, SU), torch.arange(B).view(B, 1, 1)
        match = (j * 5 + b) % (RI * SI)
        return SentenceContributions(vals(0, B), vals(41, B, RU, SU), vals(42, B, RI, SI), vals(43, B, RU), vals(44, B, RI),
                                     vals(45, B, RU, SU), vals(46, B, RU, SU), vals(47, B, RU), vals(48, B), match,
                                     (torch.arange(RU).view(1, RU) + b.view(B, 1)) % RI, vals(49, B, RI, SI), vals(50, B, RI),
                                     vals(51, B, RI), vals(52, B))

    def words(pu, pi):
        B = pu.shape[0]
        uw, iw = vals(53, B, RU, SU, W, 2), vals(54, B, RI, SI, W, 2)
        return WordContributions(vals(0, B), vals(55, B, RU, SU, W), vals(56, B, RI, SI, W), vals(57, B, RU, SU),
                                 vals(58, B, RI, SI), uw, iw)
    return SimpleNamespace(user=ids(11, N_USERS, RU, SU, W), item=ids(12, N_ITEMS, RI, SI, W), sentences=sentences, words=words)


def cases():
    """name -> thunk of the "why" lists: every path with the dict vocabulary and with None."""
    from review_based_recommender_amd import recommend as R_
    none = torch.full_like(ITEMS, -1)
    out = {}
    for tag, words in (("vocab", VOCAB), ("ids", None)):
        out[f"explain_deepconn_{tag}"] = lambda words=words: R_._why(explain_stub(False), U_IDS, ITEMS, N, words)
        out[f"explain_narre_{tag}"] = lambda words=words: R_._why(explain_stub(True), U_IDS, ITEMS, N, words)
        out[f"attention_{tag}"] = lambda words=words: R_._why_attention(attention_stub(), U_IDS, ITEMS, N, words)
        for rids in (True, False):
            out[f"contributions_{'rids' if rids else 'norids'}_{tag}"] = (
                lambda words=words, rids=rids: R_._why_contributions(contributions_stub(rids), U_IDS, ITEMS, N, words))
        out[f"sentences_{tag}"] = lambda words=words: R_._why_sentences(ahn_stub(), U_IDS, ITEMS, N, words)
        out[f"sentences_words_{tag}"] = lambda words=words: R_._why_sentences(ahn_stub(), U_IDS, ITEMS, N, words, 2)
    out["explain_no_item_kept"] = lambda: R_._why(explain_stub(True), U_IDS, none, N, VOCAB)
    out["attention_no_item_kept"] = lambda: R_._why_attention(attention_stub(), U_IDS, none, N, VOCAB)
    out["contributions_no_item_kept"] = lambda: R_._why_contributions(contributions_stub(True), U_IDS, none, N, VOCAB)
    out["sentences_no_item_kept"] = lambda: R_._why_sentences(ahn_stub(), U_IDS, none, N, VOCAB, 2)
    # n beyond every list: all entries compete, so the exact zeros reach the lists' ends and must be dropped
    out["explain_every_entry"] = lambda: R_._why(explain_stub(True), U_IDS, ITEMS, 99, VOCAB)
    out["attention_every_entry"] = lambda: R_._why_attention(attention_stub(), U_IDS, ITEMS, 99, VOCAB)
    out["contributions_every_entry"] = lambda: R_._why_contributions(contributions_stub(True), U_IDS, ITEMS, 99, None)
    out["sentences_every_entry"] = lambda: R_._why_sentences(ahn_stub(), U_IDS, ITEMS, 99, VOCAB, 99)
    return out


NAMES = sorted(cases())


def test_the_fixture_holds_exactly_these_cases():
    with open(FIXTURE) as f:
        assert sorted(json.load(f)) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_why_lists_are_the_recorded_ones(name):
    with open(FIXTURE) as f:
        expected = json.load(f)[name]
    got = cases()[name]()
    assert json.loads(json.dumps(got)) == expected
    if "no_item_kept" in name:
        assert got == [[], [], []]
    else:
        assert [len(row) for row in got] == [3, 2, 0] and all(e is not None for row in got for e in row)


def test_the_stub_values_reach_every_branch():
    """Distinct non-zero magnitudes within a pair, exact zeros present, and lists that really lost entries to them."""
    v = vals(53, 5, RI, SI, W).reshape(5, -1)
    for row in v.tolist():
        live = [abs(x) for x in row if x != 0.0]
        assert 0 < len(live) < len(row) and len(set(live)) == len(live)
    with open(FIXTURE) as f:
        fx = json.load(f)
    every = [e for row in fx["explain_every_entry"] for e in row]
    assert all(0 < len(e["user_tokens"]) < R * T and 0 not in [t[2] for t in e["user_tokens"]] for e in every)     # zeros dropped
    assert any(len(e["item_reviews"]) < N for row in fx["explain_narre_ids"] for e in row)
    sents = [s for row in fx["sentences_every_entry"] for e in row for s in e["user_sentences"]]
    assert any(len(s[-1]) < W for s in sents) and all(0.0 not in [w[2] for w in s[-1]] for s in sents)
    assert any(isinstance(t[1], str) for row in fx["attention_vocab"] for e in row for t in e["user_tokens"])
    assert any(isinstance(t[1], int) for row in fx["attention_vocab"] for e in row for t in e["user_tokens"])
    assert all(r[1] == -1 for row in fx["contributions_norids_ids"] for e in row for r in e["user_reviews"])


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit(__doc__)
    with open(FIXTURE, "w") as f:
        json.dump({name: fn() for name, fn in sorted(cases().items())}, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
