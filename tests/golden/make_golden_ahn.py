#!/usr/bin/env python3
"""Generate tests/golden/ahn_tiny.npz and ahn_small.npz by running the REFERENCE's AHN (models/ahn/ahn_model.py) on the CPU in
float64.  Needs the reference checkout on sys.path (REFERENCE_ROOT, default /root/reference); only data is stored: parameters,
inputs, outputs, gradients and parameters after 1 and 3 steps of the trainer's loop (zero_grad -> forward -> MSELoss -> backward ->
clip_grad_norm_(5.0) -> Adam(lr=2e-3)).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ahn.py

Precondition, asserted here on the float64 reference alone and stored in each file (margin_misses == 0): every max that routes
a gradient leads its runner-up by 1e-4 * (1 + |best|) (the margin of tests/explain_ref.py::margins_ok) --
  * each sentence channel's max over its words, the candidates being the valid positions plus ONE zero when the sentence is
    shorter than its side's longest;
  * each max over the bilinear similarities (a live user sentence over the item's sentences, a live user review over the item's
    reviews); the columns of the item's empty sentences / reviews are exact zeros that carry no gradient and count as one.
An f32 implementation then routes every gradient as the reference does."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("REFERENCE_ROOT", "/root/reference"))
sys.dont_write_bytecode = True

import synth_ahn  # noqa: E402

LR, MAX_GNORM, MARGIN = 2e-3, 5.0, 1e-4


def _np(t):
    return t.detach().cpu().numpy().copy()


def _margin_misses(values, valid, merge=None):
    """values [rows, cand], valid bool [rows, cand]; merge bool [rows, cand]: candidates that are one and the same exact zero.
    Returns (misses, smallest lead / (1 + |best|)) over the rows with at least two distinct candidates."""
    misses, worst = 0, float("inf")
    for r in range(values.shape[0]):
        v = values[r][valid[r]]
        if merge is not None:
            m = merge[r][valid[r]]
            if bool(m.any()):
                v = torch.cat([v[~m], v[m][:1]])
        if v.numel() < 2:
            continue
        top = torch.topk(v, 2).values
        lead = float(top[0] - top[1]) / (1.0 + abs(float(top[0])))
        worst = min(worst, lead)
        misses += lead < MARGIN
    return misses, worst


def gen(name):
    from models.ahn.ahn_model import AHN
    c = synth_ahn.AHN_CFGS[name]
    with redirect_stdout(io.StringIO()):
        model = AHN(c["E"], c["H"], c["K"], c["U"], c["I"], c["V"], None, rnn_dropout=0.0, dropout=0.0, item_review_num=c["R"])
    sd = synth_ahn.ahn_params(c)
    assert list(model.state_dict().keys()) == list(sd.keys()), "synth_ahn.ahn_shapes is not the reference's state_dict"
    model.load_state_dict(sd)
    model.double()
    b = synth_ahn.ahn_batch(c)
    args = [b[k] for k in synth_ahn.FORWARD_KEYS]
    out = {f"param/{k}": _np(v) for k, v in sd.items()}
    out.update({f"in/{k}": _np(v) for k, v in b.items()})

    # ---- eval forward with the routing maxes' candidates captured
    enc_out, sent_scores, rev_scores = [], [], []
    hooks = [model.word_encoder.register_forward_hook(lambda m, i, o: enc_out.append((o.detach(), i[1].detach()))),
             model.unbalanced_sentence_aggregator.bilinear.register_forward_hook(lambda m, i, o: sent_scores.append(o.detach())),
             model.unbalanced_review_aggregator.bilinear.register_forward_hook(lambda m, i, o: rev_scores.append(o.detach()))]
    model.eval()
    with torch.no_grad():
        pred, usw, isw, urw, irw = model(*args)
    for h in hooks:
        h.remove()
    out["pred_eval"] = _np(pred)
    out["user_sent_weights"], out["item_sent_weights"] = _np(usw), _np(isw)
    out["user_review_weights"], out["item_review_weights"] = _np(urw), _np(irw)
    misses, worst, live = 0, float("inf"), 0
    for side, (o, lens) in zip(("user", "item"), enc_out):
        n, t_out, H = o.shape
        out[f"{side}_sents"] = _np(o.max(dim=1).values)
        vals = o.permute(0, 2, 1).reshape(n * H, t_out)                                     # one row per (sentence, channel)
        ln = lens.view(n, 1).expand(n, H).reshape(n * H, 1)
        pos = torch.arange(t_out).view(1, t_out)
        valid = (pos < ln.clamp(max=t_out)) | ((pos == ln) & (ln < t_out))                   # valid steps + ONE padded zero
        valid = valid & (ln > 0)                                                            # an empty sentence routes nothing
        m, w = _margin_misses(vals, valid)
        misses, worst, live = misses + m, min(worst, w), live + int((valid.sum(1) >= 2).sum())
    B, R, S = c["B"], c["R"], c["S"]
    item_dead = ~b["item_sent_masks"].view(B, 1, R * S)
    for r, sc in enumerate(sent_scores):                                                    # one call per user review: [B, S, R*S]
        rows_live = b["user_sent_masks"][:, r].reshape(B * S)
        vals = sc.reshape(B * S, R * S)[rows_live]
        merge = item_dead.expand(B, S, R * S).reshape(B * S, R * S)[rows_live]
        m, w = _margin_misses(vals, torch.ones_like(merge), merge)
        misses, worst, live = misses + m, min(worst, w), live + vals.shape[0]
    (sc,) = rev_scores                                                                      # [B, R, R]
    rows_live = b["user_review_masks"].reshape(B * R)
    vals = sc.reshape(B * R, R)[rows_live]
    m, w = _margin_misses(vals, torch.ones_like(vals, dtype=torch.bool))
    misses, worst, live = misses + m, min(worst, w), live + vals.shape[0]
    print(f"{name}: {live} live maxima, {misses} within the margin, smallest lead {worst:.3e}")
    assert misses == 0, f"{name}: {misses} routing maxima lead by less than {MARGIN} * (1 + |best|): pick another seed in synth_ahn"
    out["margin_misses"], out["margin_min"], out["margin_live"] = np.int64(misses), np.float64(worst), np.int64(live)

    # ---- the trainer's step, three times
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    loss_fn = nn.MSELoss()
    ratings = b["ratings"].double()
    model.train()
    for step in range(3):
        opt.zero_grad()
        pred = model(*args)[0]
        loss = loss_fn(pred, ratings)
        loss.backward()
        if step == 0:
            out["pred"], out["loss"] = _np(pred), _np(loss)
            for k, p in model.named_parameters():
                g = _np(p.grad)
                out[f"grad/{k}"] = g
                out[f"gradl2/{k}"] = np.float64(np.sqrt((g ** 2).sum()))
        gnorm = nn.utils.clip_grad_norm_(model.parameters(), MAX_GNORM)
        if step == 0:
            out["gnorm"] = _np(gnorm)
        opt.step()
        if step in (0, 2):
            for k, p in model.named_parameters():
                out[f"after{step + 1}/{k}"] = _np(p)
    return out


if __name__ == "__main__":
    for name in (sys.argv[1:] or sorted(synth_ahn.AHN_CFGS)):
        np.savez_compressed(os.path.join(HERE, f"ahn_{name}.npz"), **gen(name))
