"""AhnRecommender.words and its kernel (csrc/lstm_seq.hip: lstm_saliency_kernel) against the forward that saves the state and
against the composition a user could write without the kernel, on the same GPU and the same sentences, as one JSON line.

    timeout -k 10 600 python tools/bench_ahn_words.py [--repeats 5] [--iters 10] [--warmup 3] [--limit 540] [--out FILE]

Shape: the reference's default config (models/ahn/default_ahn.json: 10 reviews x 10 sentences x 20 words per side, E = H = 300,
so Hh = 150; k = 10), a 65 x 65 catalogue (id 0 = padding) of seeded random reviews, V = 20000, and 8 random pairs: one chunk of
words(), 1600 sentences.  The composition is timed on those 1600 sentences too: its d_xproj is 147 MiB there, under the 1 GiB cap
of the backward's product (which 64 pairs would pass).  Device events, medians over --repeats blocks of --iters calls after
--warmup calls:
  saliency_ms        functional.lstm_seq_word_saliency alone on the chunk's 1600 sentences: one launch
  states_ms          functional.lstm_seq_states alone: the recurrence's forward that keeps the state (three launches)
  encode_states_ms   functional.bilstm_encode_states: the bias-free input projection, the bias add and states_ms
  words_ms           one AhnRecommender.words(u_ids, i_ids) call: gathers, the embedding, encode_states, the tail under autograd
                     pair by pair, the saliency launch
  composed_ms        what a user could write today for the same 1600 sentences and the same d_pooled: bilstm_encode(pool=True)
                     under autograd, backward, (x.grad * x).sum(-1) -- d_xproj, both dW_hh products, the projection's backward
  composed_over_new  composed_ms / (encode_states_ms + saliency_ms)
  max_abs_diff_x_grad, max_abs_diff_d_xproj   the kernel against the two compositions -- (x.grad * x).sum(-1) for the two
                     directions added, <d_xproj, xw> from lstm_seq's backward per direction -- beside the largest |value|
  saliency_bytes     what the launch reads and writes once (gates, c twice, xw, words), beside W_hh streamed once per step and
                     workgroup (w_hh_stream_bytes: from L2)
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import torch

from benchlib import arm, parser, quiet, rounded_ms as timed_ms

DEV = "cuda:0"
RV, SN, WN, E, K = 10, 10, 20, 300, 10
N_IDS, V, PAIRS = 65, 20000, 8


def main():
    ap = parser(__doc__, repeats=5, iters=10, warmup=3, limit=540)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    arm("bench_ahn_words.py", a.limit)
    from review_based_recommender_amd import data as D
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.recommend import AhnRecommender

    g = torch.Generator().manual_seed(23)

    def table():
        lens = torch.randint(0, WN + 1, (N_IDS, RV, SN), generator=g)
        lens[1, 0, 0] = WN                                                   # the table's longest sentence is a full one
        t = torch.randint(1, V, (N_IDS, RV, SN, WN), generator=g) * (torch.arange(WN) < lens.unsqueeze(-1))
        t[0] = 0
        return t.to(torch.int32).to(DEV)

    user, item = table(), table()
    model = quiet(AHN, E, E, K, N_IDS, N_IDS, V, None, rnn_dropout=0.0, dropout=0.5, item_review_num=RV).to(DEV).eval()
    rec = AhnRecommender(model, user=user, item=item).refresh()
    pu = torch.randint(1, N_IDS, (PAIRS,), generator=g).to(DEV)
    pi = torch.randint(1, N_IDS, (PAIRS,), generator=g).to(DEV)

    # the chunk's sentences as words() lays them out: the users' rows, then the items', each with its side's t_out
    ids = torch.cat([user.index_select(0, pu).reshape(-1, WN), item.index_select(0, pi).reshape(-1, WN)]).to(torch.int64)
    lens = D.sentence_masks(ids, 0)[0]
    n_side = PAIRS * RV * SN
    t_out = torch.cat([rec.t_out[0].expand(n_side), rec.t_out[1].expand(n_side)])
    params = [p.detach() for p in model.word_encoder.lstm_params()]
    Hh = params[1].shape[1]
    N = ids.shape[0]
    with torch.no_grad():
        x = RF.embedding(model.word_embeddings.weight, ids, model.word_embeddings.padding_idx)
    d_pooled = torch.randn(N, 2 * Hh, generator=g).to(DEV)
    xw, pooled, argmax, state = RF.bilstm_encode_states(x, params, lens, t_out=t_out)
    xproj = xw + torch.cat([params[2] + params[3], params[6] + params[7]])

    saliency = lambda: RF.lstm_seq_word_saliency(state, xw, params[1], params[5], lens, d_pooled, argmax)      # noqa: E731
    states = lambda: RF.lstm_seq_states(xproj, params[1], params[5], lens, t_out)                               # noqa: E731
    encode_states = lambda: RF.bilstm_encode_states(x, params, lens, t_out=t_out)                               # noqa: E731
    words = lambda: rec.words(pu, pi)                                                                           # noqa: E731

    def composed():
        leaf = x.detach().requires_grad_(True)
        p, _ = RF.bilstm_encode(leaf, params, lens, pool=True, t_out=t_out)
        (g_x,) = torch.autograd.grad(p, leaf, d_pooled)
        return (g_x * leaf.detach()).sum(-1)

    got, want = saliency(), composed()
    leaf = xproj.detach().requires_grad_(True)
    p2, _ = RF.lstm_seq(leaf, params[1], params[5], lens, pool=True, t_out=t_out)
    (d_xproj,) = torch.autograd.grad(p2, leaf, d_pooled)
    want_dir = (d_xproj * xw).view(N, WN, 2, 4 * Hh).sum(-1)
    torch.cuda.synchronize()
    res = {"bench": "ahn_words", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"pairs": PAIRS, "sentences": N, "users": N_IDS, "items": N_IDS, "reviews": RV, "sentences_per_review": SN,
                     "words": WN, "E": E, "Hh": Hh, "positions": int(lens.sum())}}
    res["pooled_bits_equal"] = bool(torch.equal(p2.detach(), pooled))
    res["max_abs_diff_x_grad"] = float((got.sum(-1) - want).abs().max())
    res["max_abs_diff_d_xproj"] = float((got - want_dir).abs().max())
    res["max_abs_value"] = float(got.abs().max())
    del leaf, p2, d_xproj, want_dir, want
    for name, fn, iters in (("saliency_ms", saliency, a.iters), ("states_ms", states, a.iters), ("encode_states_ms", encode_states, a.iters),
                            ("words_ms", words, max(1, a.iters // 5)), ("composed_ms", composed, max(1, a.iters // 2))):
        res[name], res[name + "_min"], res[name + "_max"] = timed_ms(fn, iters, a.warmup, a.repeats)
    res["composed_over_new"] = round(res["composed_ms"] / (res["encode_states_ms"] + res["saliency_ms"]), 2)
    res["saliency_over_states"] = round(res["saliency_ms"] / res["states_ms"], 3)
    positions = int(lens.sum())
    # per valid position and direction: 4 Hh gates + c_t + c_{t-1} + 4 Hh of xw read, one float written; both directions
    res["saliency_bytes"] = positions * 2 * (4 * Hh + 2 * Hh + 4 * Hh) * 4 + N * WN * 2 * 4
    tile = 16 if 16 * max(1, 256 // ((Hh + 63) // 64 * 64)) * 16 * Hh <= 49152 else 8
    tile *= max(1, 256 // ((Hh + 63) // 64 * 64))
    tiles = (N + tile - 1) // tile
    res["w_hh_stream_bytes"] = tiles * 2 * int(lens.max()) * 4 * Hh * Hh * 4      # an upper estimate: every tile to the longest length
    res["state_mb"] = round(state.saved.numel() / 2 ** 20, 1)
    res["xw_mb"] = round(xw.numel() * 4 / 2 ** 20, 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
