"""float64 restatement of the BiLSTM word saliency (rbr_lstm_seq_saliency of rbr_hip.h, functional.lstm_seq_word_saliency),
built on the loops of tests/lstm_ref.py (bilstm = lstm_from_xproj over xproj_of) and on pooled_by_argmax.

The input projection is linear, so gradient x input of a word needs no gradient with respect to the word:

    <d s / d x_t, x_t> = <W_ih^T dpre_t, x_t> = <dpre_t, W_ih x_t> = <dpre_t, xw_t>,     xw = x W_ih^T WITHOUT the bias

with dpre_t = d s / d (gate pre-activations of step t), which is the gradient with respect to xproj.  Per direction the dot runs
over that direction's four gates and Hh units: words[n, t, dir]."""
import torch

import lstm_ref as R

F64 = torch.float64


def xw_of(x, params):
    """[N, T, 8 Hh]: x W_ih^T of both directions, no bias (xproj_of's layout)."""
    return torch.cat([x @ params[0].t(), x @ params[4].t()], dim=-1)


def word_saliency(x, params, lengths, argmax, d_pooled):
    """float64 tensors (argmax int64 [N, 2 Hh], -1: no gradient) -> dict of
        words   [N, T, 2]      sum over direction dir's 4 Hh columns of dpre * xw
        abs     [N, T, 2]      the same sum of |dpre * xw| (the f32 dot's rounding scale)
        xw_l1   [N, T, 2]      ||xw[n, t, dir, :]||_1
        dpre    [N, T, 8 Hh]   d s / d xproj, s = sum(pooled_by_argmax(out, argmax) * d_pooled)
        xw      [N, T, 8 Hh]"""
    N, T, _ = x.shape
    Hh = params[1].shape[1]
    xw = xw_of(x, params).detach()
    xproj = R.xproj_of(x, params).detach().requires_grad_(True)
    out = R.lstm_from_xproj(xproj, params[1], params[5], lengths)
    s = (R.pooled_by_argmax(out, argmax) * d_pooled).sum()
    dpre = torch.autograd.grad(s, xproj)[0] if s.requires_grad and N else torch.zeros_like(xproj)
    prod = (dpre * xw).view(N, T, 2, 4 * Hh)
    return {"words": prod.sum(-1), "abs": prod.abs().sum(-1), "xw_l1": xw.view(N, T, 2, 4 * Hh).abs().sum(-1), "dpre": dpre, "xw": xw}


def grad_times_input(x, params, lengths, argmax, d_pooled):
    """[N, T, 2] by float64 autograd through the same loops down to x itself: <d s_dir / d x_t, x_t>, s_dir the part of s that
    direction dir's half of the pooled vector carries."""
    N, T, _ = x.shape
    Hh = params[1].shape[1]
    cols = []
    for d in range(2):
        xl = x.detach().clone().requires_grad_(True)
        half = torch.zeros_like(d_pooled)
        half[:, d * Hh:(d + 1) * Hh] = d_pooled[:, d * Hh:(d + 1) * Hh]
        s = (R.pooled_by_argmax(R.bilstm(xl, params, lengths), argmax) * half).sum()
        g = torch.autograd.grad(s, xl)[0] if s.requires_grad and N else torch.zeros_like(xl)
        cols.append((g * xl.detach()).sum(-1))
    return torch.stack(cols, dim=-1)


def error_bound(ref, Hh):
    """[N, T, 2]: b * ||xw_ref[n, t, dir, :]||_1 + 4 Hh * 2^-24 * sum_k |dpre_ref,k * xw_ref,k| with b = 2e-6 + 2e-4 ||dpre_ref||_2,
    the bound tests/test_lstm_seq_edges_gpu.py places on every element of d_xproj (Hoelder), plus the f32 dot's rounding."""
    b = 2e-6 + 2e-4 * float(ref["dpre"].norm())
    return b * ref["xw_l1"] + 4 * Hh * 2.0 ** -24 * ref["abs"]
