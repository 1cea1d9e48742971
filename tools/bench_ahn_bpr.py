"""AHN's differentiable pair tail (functional.ahn_pair_attend, csrc/ahn_attend.hip) and the steps built on it, as one JSON line.

    timeout -k 10 600 python tools/bench_ahn_bpr.py [--repeats 5] [--iters 10] [--warmup 3] [--limit 540]

Shape: the reference's default config (models/ahn/default_ahn.json): batch 32, 10 reviews of 10 sentences of 20 words per side,
F = 300, k = 10; V = 20000, U = I = 1000 as in tools/bench_ahn.py.  Device events, medians over --repeats blocks of --iters calls
after --warmup calls ([median, min, max] per key), everything in one process on one GPU:
  attend_g{G}_{fwd,fwd_bwd}_ms        the op alone at G = 1, 2, 5 groups of 32 pairs: forward, and forward + backward to X, Xt, Ks, Kr, bt
  torch_g{G}_{fwd,fwd_bwd}_ms         the torch composition of the same user-side arithmetic on the same inputs (the reassociated
                                      restatement the tests use, tests/ahn_attend_ref.py::attend_torch)
  attend_g{G}_max_abs_diff            largest difference between the two forwards' z
  mse_step_{unfused,fused}_ms         the eager MSE training step (forward, loss, backward, HipClipAdam) with AHN.fused_tail off / on
  bpr_n{n}_b{B}_{grouped,generic}_ms  the eager BPR step at n_neg = 1 and 4 on one expanded batch of (1 + n_neg) * B rows: grouped =
                                      AHN.forward_groups (every user encoded once, the tail one op) + functional.bpr_loss; generic =
                                      AHN.forward on the expanded batch + functional.bpr_loss.  B = 32, and the largest halving of
                                      it at which BOTH routes run: the LSTM backward refuses a gate operand beyond 1 GiB (about 11 000
                                      sentences of 20 words), which a route that exceeds it reports as null with the refusal's text
                                      (..._refused); bpr_n{n}_b{B}_sentences = [grouped, generic] sentences through the encoder
The process ends itself after --limit seconds (SIGALRM); run it under `timeout` as above."""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import signal
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_ahn import BZ, DEV, E, HH, RV, SN, WN, timed_ms  # noqa: E402

F = 2 * HH
GRADS = ("X", "Xt", "Ks", "Kr", "bt")


def op_inputs(G, g):
    rnd = lambda *s, scale=1.0: ((torch.rand(*s, generator=g) * 2 - 1) * scale).to(DEV)          # noqa: E731
    P, N = G * BZ, RV * SN
    sm = torch.rand(BZ, RV, SN, generator=g) < 0.7
    sm[:, :, 0] = True
    t = dict(X=rnd(BZ, N, F), Xt=rnd(BZ, N, F, scale=0.5), Ks=rnd(P, N, F, scale=2.0 / F ** 0.5), Kr=rnd(P, RV, F, scale=2.0 / F ** 0.5),
             bt=rnd(F, scale=0.2))
    for k in GRADS:
        t[k].requires_grad_(True)
    return t, sm.to(DEV), sm.any(-1).to(DEV), rnd(P, F)


def expanded_batch(rows, g, V, U, I):
    """AHN's ten arguments for `rows` pairs, drawn as tools/bench_ahn.py draws them."""
    lens = torch.randint(0, WN + 1, (2, rows, RV, SN), generator=g)
    ids = torch.randint(1, V, (2, rows, RV, SN, WN), generator=g) * (torch.arange(WN) < lens.unsqueeze(-1))
    sm = lens > 0
    sm[:, :, 0, 0] = True
    lens = torch.where(sm & (lens == 0), torch.ones_like(lens), lens)
    rm = sm.any(dim=3)
    return tuple(t.to(DEV) for t in (ids[0], ids[1], sm[0], sm[1], lens[0], lens[1], rm[0], rm[1],
                                     torch.randint(1, U, (rows,), generator=g), torch.randint(1, I, (rows,), generator=g)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=540, help="seconds after which the process ends itself")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ahn_bpr.py needs an MI355X: there is no CPU fallback and no CPU timing")
    signal.alarm(a.limit)
    import ahn_attend_ref as A
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.models.ahn.ahn_model import AHN
    from review_based_recommender_amd.train_step import AhnBprObjective, BprObjective, make_optimizer, train_step

    g = torch.Generator().manual_seed(23)
    res = {"bench": "ahn_bpr", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters,
           "shape": {"B": BZ, "Ru": RV, "Su": SN, "Ri": RV, "Si": SN, "F": F}}

    def record(key, fn):
        res[key] = timed_ms(fn, a.iters, a.warmup, a.repeats)

    # ---- the op alone against the torch composition of the same arithmetic
    for G in (1, 2, 5):
        t, sm, rm, dz = op_inputs(G, g)
        hip = lambda: RF.ahn_pair_attend(t["X"], t["Xt"], sm, rm, t["Ks"], t["Kr"], t["bt"], groups=G)[0]      # noqa: E731
        ref = lambda: A.attend_torch(t["X"], t["Xt"], sm, rm, t["Ks"], t["Kr"], t["bt"], G)[0]                 # noqa: E731

        def with_bwd(fwd):
            def run():
                for k in GRADS:
                    t[k].grad = None
                fwd().backward(dz)
            return run

        with torch.no_grad():
            res[f"attend_g{G}_max_abs_diff"] = float((hip() - ref()).abs().max())
        for name, fn in ((f"attend_g{G}_fwd_ms", hip), (f"torch_g{G}_fwd_ms", ref), (f"attend_g{G}_fwd_bwd_ms", with_bwd(hip)),
                         (f"torch_g{G}_fwd_bwd_ms", with_bwd(ref))):
            record(name, fn)
        res[f"torch_over_attend_g{G}_fwd_bwd"] = round(res[f"torch_g{G}_fwd_bwd_ms"][0] / res[f"attend_g{G}_fwd_bwd_ms"][0], 3)

    # ---- the training steps
    V, U, I, K = 20000, 1000, 1000, 10
    with contextlib.redirect_stdout(io.StringIO()):
        model = AHN(E, F, K, U, I, V, None, rnn_dropout=0.0, dropout=0.5, item_review_num=RV).to(DEV)
    opt = make_optimizer(model, hip_clip_adam=True)
    model.train()
    batch = expanded_batch(BZ, g, V, U, I)
    ratings = torch.randint(1, 6, (BZ,), generator=g).float().to(DEV)
    for name, on in (("mse_step_unfused_ms", False), ("mse_step_fused_ms", True)):
        model.fused_tail = on
        record(name, lambda: train_step(model, opt, batch, ratings))
    model.fused_tail = False
    res["mse_unfused_over_fused"] = round(res["mse_step_unfused_ms"][0] / res["mse_step_fused_ms"][0], 3)
    for n_neg, bz in ((1, BZ), (4, BZ), (1, BZ // 2), (4, BZ // 4)):
        big = expanded_batch((1 + n_neg) * bz, g, V, U, I)
        big = tuple(torch.cat([t[:bz]] * (1 + n_neg)) if k in (0, 2, 4, 6, 8) else t for k, t in enumerate(big))   # a user's rows repeat
        valid = torch.ones(n_neg * bz, device=DEV)
        feed = types.SimpleNamespace(n_neg=n_neg, buffers=lambda B, v=valid: (None, None, v))
        keys = [f"bpr_n{n_neg}_b{bz}_{kind}_ms" for kind in ("grouped", "generic")]
        res[f"bpr_n{n_neg}_b{bz}_sentences"] = [(1 + (1 + n_neg)) * bz * RV * SN, 2 * (1 + n_neg) * bz * RV * SN]
        for name, obj in zip(keys, (AhnBprObjective(feed), BprObjective(feed))):
            try:
                record(name, lambda: train_step(model, opt, big, None, objective=obj))
            except RuntimeError as e:          # the LSTM backward refuses an operand beyond 1 GiB: the step does not exist at this size
                res[name], res[name + "_refused"] = None, str(e)[:200]
                opt.zero_grad()
        if res[keys[0]] and res[keys[1]]:
            res[f"bpr_n{n_neg}_b{bz}_generic_over_grouped"] = round(res[keys[1]][0] / res[keys[0]][0], 3)
    RF.check_id_errors(DEV)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
