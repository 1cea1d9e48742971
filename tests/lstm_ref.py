"""float64 restatement of the bidirectional LSTM ops (rbr_lstm_seq_* of rbr_hip.h, functional.lstm_seq / bilstm_encode), written as
explicit loops over time on torch float64 tensors, so that autograd differentiates the loops themselves -- not a call of nn.LSTM.

    gates_t = x_t W_ih^T + b_ih + b_hh + h_{t-1} W_hh^T        gate order i, f, g, o
    c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),   h_t = sigmoid(o) tanh(c_t),   h_{-1} = c_{-1} = 0

The forward direction walks t = 0 .. len-1 of a sequence, the reverse direction t = len-1 .. 0 of the same sequence (a packed
sequence).  Positions t >= len of the output are 0; a sequence of length 0 is a row of zeros that no gradient reaches.

The pooled form is the reference model's max over the steps of the output after it has been trimmed to the batch's output length
t_out = max(clamp(lengths, 1, 1000)) and zero-padded: a sequence shorter than t_out competes with ONE zero, a sequence of full
length with none.  argmax = the winning step, -1 where the zero wins and in empty rows."""
import torch

F64 = torch.float64
PARAM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
               "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def t_out_of(lengths, T=None):
    hi = 1000 if T is None else min(int(T), 1000)
    return int(lengths.clamp(1, hi).max())


def xproj_of(x, params):
    """[N, T, 8 Hh]: x W_ih^T + b_ih + b_hh, the forward direction's four gates first."""
    w_ih_f, _, b_ih_f, b_hh_f, w_ih_r, _, b_ih_r, b_hh_r = params
    return torch.cat([x @ w_ih_f.t() + b_ih_f + b_hh_f, x @ w_ih_r.t() + b_ih_r + b_hh_r], dim=-1)


def _cell(pre, h, c, w_hh):
    Hh = w_hh.shape[1]
    g = pre + h @ w_hh.t()
    i, f, gg, o = torch.sigmoid(g[:Hh]), torch.sigmoid(g[Hh:2 * Hh]), torch.tanh(g[2 * Hh:3 * Hh]), torch.sigmoid(g[3 * Hh:])
    c = f * c + i * gg
    return o * torch.tanh(c), c


def lstm_from_xproj(xproj, w_hh_f, w_hh_r, lengths):
    """out [N, T, 2 Hh] float64 by explicit loops (differentiable)."""
    N, T, H8 = xproj.shape
    Hh = H8 // 8
    rows = []
    for n in range(N):
        ln = max(0, min(int(lengths[n]), T))
        zero = xproj.new_zeros(Hh)
        fw = [zero] * T
        bw = [zero] * T
        h, c = zero, zero
        for t in range(ln):
            h, c = _cell(xproj[n, t, :4 * Hh], h, c, w_hh_f)
            fw[t] = h
        h, c = zero, zero
        for t in range(ln - 1, -1, -1):
            h, c = _cell(xproj[n, t, 4 * Hh:], h, c, w_hh_r)
            bw[t] = h
        rows.append(torch.cat([torch.stack(fw), torch.stack(bw)], dim=1))
    return torch.stack(rows) if N else xproj.new_zeros(0, T, 2 * Hh)


def bilstm(x, params, lengths):
    return lstm_from_xproj(xproj_of(x, params), params[1], params[5], lengths)


def trimmed_max(out, lengths, t_out):
    """(pooled [N, 2 Hh], argmax int64 [N, 2 Hh]): the max over the steps of `out` trimmed to t_out steps and zero-padded.
    t_out: an int, or one per sequence.  Among equal candidates the first step wins; the padded zero wins only when it is
    strictly larger than every valid step (or equal: then -1 is reported -- no gradient flows either way at an exact tie)."""
    N, T, C = out.shape
    vals, args = [], []
    for n in range(N):
        ln = max(0, min(int(lengths[n]), T))
        to = int(t_out[n]) if torch.is_tensor(t_out) and t_out.numel() > 1 else int(t_out)
        if ln == 0:
            vals.append(out.new_zeros(C))
            args.append(torch.full((C,), -1, dtype=torch.int64))
            continue
        m, a = out[n, :ln].max(dim=0)
        if ln < to:
            lose = ~(m > 0)
            m = torch.where(lose, torch.zeros_like(m), m)
            a = torch.where(lose, torch.full_like(a, -1), a)
        vals.append(m)
        args.append(a)
    return torch.stack(vals), torch.stack(args)


def pooled_by_argmax(out, argmax):
    """pooled[n, c] = out[n, argmax[n, c], c], or 0 where argmax is -1: the pooled value with the routing GIVEN (differentiable
    in `out`), as explain_ref.saliency takes its argmax as an input."""
    a = argmax.to(torch.int64)
    g = out.gather(1, a.clamp(min=0).unsqueeze(1)).squeeze(1)
    return torch.where(a >= 0, g, torch.zeros_like(g))
