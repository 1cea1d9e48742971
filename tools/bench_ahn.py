"""AHN's sentence encoder on the HIP LSTM kernels (csrc/lstm_seq.hip) against what a user would run today -- torch.nn.LSTM on
packed sequences followed by torch.max -- on the same GPU and the same inputs, and the whole AHN training step, as one JSON line.

    timeout -k 10 600 python tools/bench_ahn.py [--repeats 5] [--iters 10] [--warmup 3] [--limit 540]

Shape: the reference's default config (models/ahn/default_ahn.json): batch 32, both sides, 10 reviews of 10 sentences of 20 words
-> N = 2 * 32 * 10 * 10 = 6400 sentences, E = 300, 150 hidden units per direction; sentence lengths drawn from a fixed seed
(uniform on 0..20, so about one sentence in 21 is empty).
Device events, medians over --repeats blocks of --iters calls after --warmup calls:
  hip_fwd_ms / hip_fwd_bwd_ms       functional.bilstm_encode(pool=True): input projection (MFMA linear) + recurrence with the fused
                                    max; and the same plus the backward to x and all eight LSTM tensors
  torch_fwd_ms / torch_fwd_bwd_ms   clamp(lengths, 1) -> pack_padded_sequence(enforce_sorted=False) -> nn.LSTM -> pad_packed_sequence
                                    -> zero the empty rows -> torch.max(dim=1), as the reference's encoder does
  hip_*_kernel_ms                   the C-ABI calls of the recurrence alone (rbr_lstm_seq_fwd / _bwd), event pairs around each call
  recurrence_gflop                  2 * 4Hh * Hh * 2 directions * sum(lengths) -- what the forward recurrence needs; the backward
                                    needs twice that (d h_{t-1} and d W_hh); *_gflops = that over the kernel time
  ahn_step_ms                       one whole AHN training step (forward, MSE loss, backward, clip + Adam by HipClipAdam) at the same
                                    shape, V = 20000, U = I = 1000, k = 10
  max_abs_diff                      largest difference between the two encoders' pooled outputs
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import json

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from benchlib import arm, parser, quiet, rounded_ms as timed_ms

DEV = "cuda:0"
BZ, RV, SN, WN, E, HH = 32, 10, 10, 20, 300, 150


def main():
    ap = parser(__doc__, repeats=5, iters=10, warmup=3, limit=540)
    a = ap.parse_args()
    arm("bench_ahn.py", a.limit)
    from review_based_recommender_amd import _lib
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.train_step import make_optimizer, train_step

    g = torch.Generator().manual_seed(17)
    N = 2 * BZ * RV * SN
    lengths = torch.randint(0, WN + 1, (N,), generator=g)
    x = (torch.randn(N, WN, E, generator=g) * 0.5).to(DEV).requires_grad_(True)
    lstm = torch.nn.LSTM(E, HH, batch_first=True, bidirectional=True).to(DEV)
    params = [getattr(lstm, k) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse",
                                         "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")]
    len_dev = lengths.to(DEV)
    len_cpu = lengths.clamp(min=1, max=1000)
    live = (lengths != 0).to(DEV).float().view(N, 1, 1)
    up = torch.randn(N, 2 * HH, generator=g).to(DEV)

    def hip_fwd():
        return RF.bilstm_encode(x, params, len_dev, pool=True)[0]

    def torch_fwd():
        out, _ = lstm(pack_padded_sequence(x, len_cpu, batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True)
        return torch.max(out * live, dim=1)[0]

    def with_bwd(fwd):
        def run():
            x.grad = None
            lstm.zero_grad(set_to_none=True)
            (fwd() * up).sum().backward()
        return run

    res = {"bench": "ahn", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"sentences": N, "words": WN, "E": E, "Hh": HH, "sum_lengths": int(lengths.sum()), "empty": int((lengths == 0).sum())}}
    with torch.no_grad():
        res["max_abs_diff"] = float((hip_fwd() - torch_fwd()).abs().max())
    for name, fn in (("hip_fwd_ms", hip_fwd), ("torch_fwd_ms", torch_fwd), ("hip_fwd_bwd_ms", with_bwd(hip_fwd)),
                     ("torch_fwd_bwd_ms", with_bwd(torch_fwd))):
        res[name], res[name + "_min"], res[name + "_max"] = timed_ms(fn, a.iters, a.warmup, a.repeats)
    res["torch_over_hip_fwd"] = round(res["torch_fwd_ms"] / res["hip_fwd_ms"], 3)
    res["torch_over_hip_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"], 3)

    # the recurrence's own launches
    _lib.TIMER.start()
    for _ in range(a.iters):
        with_bwd(hip_fwd)()
    torch.cuda.synchronize()
    _lib.TIMER.stop()
    summ = _lib.TIMER.summary()
    gflop = 2.0 * 4 * HH * HH * 2 * float(lengths.sum()) / 1e9
    res["recurrence_gflop"] = round(gflop, 3)
    for key, mult in (("lstm_seq_fwd", 1.0), ("lstm_seq_bwd", 2.0)):
        ms = summ[key][1]
        res[f"hip_{key}_kernel_ms"] = round(ms, 4)
        res[f"hip_{key}_gflops"] = round(mult * gflop / (ms * 1e-3), 1)

    # the whole model's training step
    V, U, I, K = 20000, 1000, 1000, 10
    model = quiet(AHN, E, 2 * HH, K, U, I, V, None, rnn_dropout=0.0, dropout=0.5, item_review_num=RV).to(DEV)
    lens = lengths.view(2, BZ, RV, SN)
    ids = torch.randint(1, V, (2, BZ, RV, SN, WN), generator=g) * (torch.arange(WN) < lens.unsqueeze(-1))
    sm = lens > 0
    sm[:, :, 0, 0] = True                                      # every example keeps a live review
    lens = torch.where(sm & (lens == 0), torch.ones_like(lens), lens)
    rm = sm.any(dim=3)
    batch = tuple(t.to(DEV) for t in (ids[0], ids[1], sm[0], sm[1], lens[0], lens[1], rm[0], rm[1], torch.randint(1, U, (BZ,), generator=g),
                                      torch.randint(1, I, (BZ,), generator=g)))
    ratings = torch.randint(1, 6, (BZ,), generator=g).float().to(DEV)
    opt = make_optimizer(model, hip_clip_adam=True)
    model.train()
    res["ahn_step_ms"], res["ahn_step_ms_min"], res["ahn_step_ms_max"] = timed_ms(
        lambda: train_step(model, opt, batch, ratings), a.iters, a.warmup, a.repeats)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
