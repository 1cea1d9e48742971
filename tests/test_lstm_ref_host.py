"""tests/lstm_ref.py (the float64 loops the GPU tests of the LSTM kernels are held to) against torch.nn.LSTM in float64 on packed
sequences, as the reference's Seq2SeqEncoder runs it (clamp the lengths to >= 1, pack with enforce_sorted=False, pad, zero the empty
rows in place): outputs, the trimmed zero-tailed max, and the gradients to x and all eight LSTM tensors -- none for an empty row.
Plus the C ABI's declaration, binding arity and host-side refusals (no GPU needed)."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_ref as R

F64 = torch.float64

CASES = {                                   # (N, T, E, Hh, lengths)
    "mixed_0_1_T": (6, 5, 4, 3, [0, 1, 5, 3, 0, 2]),
    "longest_below_T": (5, 7, 3, 2, [4, 0, 1, 4, 2]),
    "all_full": (3, 4, 5, 3, [4, 4, 4]),
    "single": (1, 1, 2, 1, [1]),
}


def _setup(name):
    N, T, E, Hh, lens = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    lstm = torch.nn.LSTM(E, Hh, num_layers=1, bias=True, batch_first=True, bidirectional=True).double()
    for p in lstm.parameters():
        p.data = torch.randn(p.shape, generator=g, dtype=F64) * 0.6
    x = torch.randn(N, T, E, generator=g, dtype=F64)
    return lstm, x, torch.tensor(lens, dtype=torch.int64)


def _torch_encoder(lstm, x, lengths):
    """Seq2SeqEncoder.forward of the reference without its dropout."""
    clamped = torch.clamp(lengths, min=1, max=1000)
    out, _ = lstm(pack_padded_sequence(x, clamped, batch_first=True, enforce_sorted=False))
    out, _ = pad_packed_sequence(out, batch_first=True)
    out[lengths == 0] = 0.
    return out                              # [N, t_out, 2 Hh]


@pytest.mark.parametrize("name", sorted(CASES))
def test_loops_equal_packed_nn_lstm_forward_and_backward(name):
    lstm, x, lengths = _setup(name)
    N, T, E = x.shape
    x1 = x.clone().requires_grad_(True)
    want = _torch_encoder(lstm, x1, lengths)
    t_out = R.t_out_of(lengths)
    assert want.shape[1] == t_out
    params = [getattr(lstm, k).detach().clone().requires_grad_(True) for k in R.PARAM_NAMES]
    x2 = x.clone().requires_grad_(True)
    got = R.bilstm(x2, params, lengths)
    assert got.shape == (N, T, want.shape[2])
    assert float((got[:, :t_out] - want).abs().max()) <= 1e-12
    assert float(got[:, t_out:].abs().sum()) == 0.0
    for n in range(N):
        assert float(got[n, int(lengths[n]):].abs().sum()) == 0.0

    # the max of the trimmed, zero-tailed output
    want_max, _ = torch.max(want, dim=1)
    got_max, arg = R.trimmed_max(got, lengths, t_out)
    assert float((got_max - want_max).abs().max()) <= 1e-12
    assert bool((arg[lengths == 0] == -1).all())
    assert float((R.pooled_by_argmax(got, arg) - got_max).abs().max()) == 0.0

    # gradients of one scalar through the output AND the max
    g = torch.Generator().manual_seed(7)
    wo = torch.randn(want.shape, generator=g, dtype=F64)
    wm = torch.randn(want_max.shape, generator=g, dtype=F64)
    ((want * wo).sum() + (want_max * wm).sum()).backward()
    ((got[:, :t_out] * wo).sum() + (got_max * wm).sum()).backward()
    assert float((x2.grad - x1.grad).abs().max()) <= 1e-11
    for k, p in zip(R.PARAM_NAMES, params):
        ref = getattr(lstm, k).grad
        assert float((p.grad - ref).abs().max()) <= 1e-11 * (1 + float(ref.abs().max())), k
    for n in range(N):
        if int(lengths[n]) == 0:
            assert float(x2.grad[n].abs().sum()) == 0.0 and float(x1.grad[n].abs().sum()) == 0.0
        assert float(x2.grad[n, int(lengths[n]):].abs().sum()) == 0.0


def test_per_sequence_t_out_is_each_side_s_own_zero_candidate():
    lstm, x, lengths = _setup("longest_below_T")
    params = [getattr(lstm, k).detach() for k in R.PARAM_NAMES]
    out = R.bilstm(x, params, lengths)
    sides = [slice(0, 2), slice(2, 5)]                        # longest 4 and 4 -> make the first side's longest 1
    lengths = torch.tensor([1, 0, 1, 4, 2])
    out = R.bilstm(x, params, lengths)
    per_seq = torch.cat([torch.full((s.stop - s.start,), R.t_out_of(lengths[s])) for s in sides])
    got, _ = R.trimmed_max(out, lengths, per_seq)
    for s in sides:
        to = R.t_out_of(lengths[s])
        want, _ = torch.max(out[s, :to], dim=1)
        assert float((got[s] - want).abs().max()) == 0.0
    one, _ = R.trimmed_max(out, lengths, R.t_out_of(lengths))
    assert float((one[0] - got[0]).abs().max()) > 0.0          # a full-length row of the short side has no zero candidate


def test_lstm_seq_is_declared_in_header_binding_and_library():
    import os
    from review_based_recommender_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rbr_hip.h")).read()
    for name, arity in (("rbr_lstm_seq_fwd", 14), ("rbr_lstm_seq_bwd", 15), ("rbr_lstm_seq_ws_bytes", 3), ("rbr_lstm_seq_bwd_ws_bytes", 3)):
        assert f" {name}(" in header
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
    L = _lib.lib()
    assert L.rbr_lstm_seq_ws_bytes(4, 5, 3) >= 4 * 5 * (8 + 2 + 2) * 3 * 4
    # host-side refusals need no GPU
    nul = [None] * 3
    assert L.rbr_lstm_seq_fwd(4, 5, 3, *nul, None, None, 0, None, None, None, None, None) == -1 and b"null pointer" in L.rbr_last_error()
    assert L.rbr_lstm_seq_fwd(4, 1001, 3, *nul, None, None, 0, None, None, None, None, None) == -2 and b"1000" in L.rbr_last_error()
    assert L.rbr_lstm_seq_fwd(4, 5, 257, *nul, None, None, 0, None, None, None, None, None) == -2
    assert L.rbr_lstm_seq_fwd(4, 0, 3, *nul, None, None, 0, None, None, None, None, None) == -1
    assert L.rbr_lstm_seq_fwd(-1, 5, 3, *nul, None, None, 0, None, None, None, None, None) == -1
    assert L.rbr_lstm_seq_fwd(0, 5, 3, *nul, None, None, 0, None, None, None, None, None) == 0
    assert L.rbr_lstm_seq_bwd(4, 5, 3, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.rbr_lstm_seq_bwd(4, 1001, 3, None, None, None, None, None, None, None, None, None, None, None, None) == -2
