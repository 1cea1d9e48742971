"""rbr_textcnn_saliency through functional.textcnn_saliency at the shapes that reach each of its branches, against the float64
closed form of tests/explain_ref.py.  feat, argmax and d_feat are HAND-MADE inputs (the kernel takes them as given), so every
edge is hit on purpose and no near-tie of a max-pool can flip a comparison.

Bound, per element (tests/edge_refs.py): (n + 4) * 2^-24 * Abs with n = D * (number of (channel, tap) terms landing on the
element) -- each term is a D-long dot product, the 4 covers g * act' (up to 3 roundings for tanh), the gate and the final
product.  An element with Abs == 0 has no terms and must be exactly 0.0."""
import numpy as np
import pytest
import torch

import edge_refs as E
import explain_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(n_docs, L, D, V, kzs, chans, seed, valid=False, tanh=False, gate=False, mask_p=0.2):
    g = torch.Generator().manual_seed(seed)
    c = dict(valid=valid, tanh=tanh, kzs=kzs, chans=chans, D=D, L=L)
    c["table"] = torch.randn(V, D, generator=g)
    c["ids"] = torch.randint(0, V, (n_docs, L), generator=g)
    c["mask"] = (torch.rand(n_docs, L, generator=g) > mask_p) if mask_p is not None else None
    c["gate"] = (torch.rand(n_docs, L, generator=g) * 1.6 - 0.8) if gate else None
    c["ws"] = [torch.randn(ch, D, k, generator=g) / np.sqrt(D * k) for k, ch in zip(kzs, chans)]
    c["argmax"] = torch.cat([torch.randint(0, (L - k + 1) if valid else L, (n_docs, ch), generator=g) for k, ch in zip(kzs, chans)],
                            1).to(torch.int32)
    feat = torch.randn(n_docs, sum(chans), generator=g)                  # about half the channels are off under ReLU
    c["feat"] = torch.tanh(feat) if tanh else feat
    d = torch.randn(n_docs, sum(chans), generator=g)
    d[torch.rand(d.shape, generator=g) < 0.15] = 0.0                     # channels without a gradient
    c["d_feat"] = d
    return c


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(c, table=None):
    from review_based_recommender_amd import functional as RF
    return RF.textcnn_saliency(_dev(c["table"]) if table is None else table, _dev(c["ids"]), _dev(c["mask"]), [_dev(w) for w in c["ws"]],
                               _dev(c["feat"]), _dev(c["argmax"]), _dev(c["d_feat"]), gate=_dev(c["gate"]),
                               pad_mode=RF.PAD_VALID if c["valid"] else RF.PAD_SAME, act=RF.ACT_TANH if c["tanh"] else RF.ACT_RELU)


def _check(name, c, got=None):
    got = _run(c) if got is None else got
    ref, ab, cnt = X.saliency(c["table"], c["ids"], c["mask"], c["gate"], c["ws"], c["feat"], c["argmax"], c["d_feat"], c["valid"],
                              c["tanh"], counts=True)
    assert got.shape == c["ids"].shape and got.dtype == torch.float32
    E.check("saliency", name, got, ref, E.bound_of(c["D"] * cnt, ab))
    return got, ref, ab


CASES = {
    "scalar_rows": dict(n_docs=3, L=20, D=10, V=30, kzs=[3, 5], chans=[4, 4]),
    "clipped_both_ends": dict(n_docs=2, L=40, D=12, V=50, kzs=[1, 9], chans=[3, 5]),
    "window_wider_than_doc": dict(n_docs=1, L=1, D=8, V=9, kzs=[3], chans=[5], mask_p=None),
    "second_position_per_thread": dict(n_docs=5, L=300, D=16, V=60, kzs=[3, 7], chans=[33, 31]),
    "two_lds_chunks": dict(n_docs=4, L=64, D=20, V=40, kzs=[3], chans=[260]),
    "workload_banks": dict(n_docs=3, L=64, D=300, V=80, kzs=[3, 5, 7], chans=[50, 50, 50]),
    "valid_tanh_gate_nomask": dict(n_docs=3, L=30, D=104, V=50, kzs=[2, 3, 4], chans=[5, 6, 7], valid=True, tanh=True, gate=True,
                                   mask_p=None),
    "second_pass_of_positions": dict(n_docs=2, L=1100, D=8, V=30, kzs=[3, 5], chans=[6, 6]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_saliency_at_edge_shapes(name):
    c = _make(seed=sorted(CASES).index(name) + 1, **CASES[name])
    L = c["L"]
    if name == "window_wider_than_doc":
        c["feat"] = c["feat"].abs() + 0.1
    if name == "clipped_both_ends":                      # every window hangs over an end of the document
        c["argmax"][:, ::2] = 0
        c["argmax"][:, 1::2] = L - 1
        c["feat"] = c["feat"].abs() + 0.1
    if name == "second_pass_of_positions":               # windows on both sides of, and across, the boundary between two passes
        c["argmax"][0, :6] = torch.tensor([1022, 1023, 1024, 1025, 1099, 0], dtype=torch.int32)
        c["argmax"][1, 6:] = torch.tensor([1021, 1022, 1023, 1024, 1025, 1026], dtype=torch.int32)
        c["feat"][:, :] = c["feat"].abs() + 0.1
        c["mask"][:, 1015:1035] = True
    got, ref, ab = _check(name, c)
    assert float(ab.max()) > 0 and bool((got != 0).any())
    if c["mask"] is not None:
        assert bool((got.cpu()[~c["mask"]] == 0).all())
    if name == "clipped_both_ends":
        assert bool((got[:, 0] != 0).any()) and bool((got[:, L - 1] != 0).any())
    if name == "second_pass_of_positions":
        assert bool((got[:, 1020:1030] != 0).any())


def test_misaligned_table_takes_the_scalar_rows():
    """D % 4 == 0 but the table starts 4 bytes off a 16-byte boundary: no float4 loads, same bounds."""
    c = _make(3, 20, 12, 30, [3, 5], [4, 4], seed=21)
    buf = torch.empty(30 * 12 + 1, device=DEV)
    table = buf[1:].view(30, 12)
    table.copy_(c["table"])
    assert table.data_ptr() % 16 == 4 and table.is_contiguous()
    _check("misaligned", c, _run(c, table))


def test_nothing_to_explain_gives_exact_zeros():
    base = dict(n_docs=3, L=20, D=12, V=30, kzs=[3, 5], chans=[4, 4])
    c = _make(seed=31, **base)
    c["mask"] = torch.zeros_like(c["mask"])                              # every token masked
    assert bool((_run(c) == 0).all())
    c = _make(seed=32, **base)
    c["feat"] = torch.zeros_like(c["feat"])                              # ReLU gate closed everywhere, gradient present
    assert bool((c["d_feat"] != 0).any()) and bool((_run(c) == 0).all())
    c = _make(seed=33, **base)
    c["d_feat"] = torch.zeros_like(c["d_feat"])
    assert bool((_run(c) == 0).all())


def test_mask_none_and_a_shared_window():
    c = _make(3, 20, 12, 30, [3, 5], [4, 4], seed=41, mask_p=None)
    _check("mask_none", c)
    c = _make(3, 20, 12, 30, [3, 5], [40, 40], seed=42)
    c["argmax"][:] = 7                                                   # 80 channels route to one window
    c["feat"] = c["feat"].abs() + 0.1
    c["mask"][:, 5:10] = True
    got, _, ab = _check("shared_window", c)
    assert bool((ab[:, :5] == 0).all()) and bool((ab[:, 10:] == 0).all()) and bool((got[:, 5:10] != 0).all())


def test_argmax_outside_the_pooled_range_contributes_nothing():
    c = _make(4, 24, 12, 30, [3, 5], [6, 6], seed=51)
    c["feat"] = c["feat"].abs() + 0.1
    c["argmax"][0, 0], c["argmax"][1, 3], c["argmax"][2, 7], c["argmax"][3, 11] = -1, 24 + 5, -1, 24 + 5
    c["argmax"][0, 1] = 24                                               # first index past the pooled range
    clean = dict(c, d_feat=c["d_feat"].clone())
    for cell in ((0, 0), (1, 3), (2, 7), (3, 11), (0, 1)):
        clean["d_feat"][cell] = 0.0
    clean["argmax"] = c["argmax"].clamp(0, 23)
    got, _, _ = _check("argmax_out_of_range", c)                         # the reference drops those cells; every other one in bound
    assert torch.equal(got, _run(clean))                                 # and bit for bit what the call without them gives


def test_empty_batch_split_gate_and_cpu_tensors():
    from review_based_recommender_amd import functional as RF
    c = _make(2, 16, 8, 20, [1, 3], [3, 3], seed=61)
    empty = RF.textcnn_saliency(_dev(c["table"]), torch.zeros(0, 16, dtype=torch.int64, device=DEV), None, [_dev(w) for w in c["ws"]],
                                torch.zeros(0, 6, device=DEV), torch.zeros(0, 6, dtype=torch.int32, device=DEV),
                                torch.zeros(0, 6, device=DEV))
    assert empty.shape == (0, 16)
    args = (_dev(c["table"]), _dev(c["ids"]), _dev(c["mask"]), [_dev(w) for w in c["ws"]], _dev(c["feat"]), _dev(c["argmax"]),
            _dev(c["d_feat"]))
    with pytest.raises(RuntimeError, match="GATE_SPLIT"):
        RF.textcnn_saliency(*args, gate_split=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.textcnn_saliency(c["table"], c["ids"], c["mask"], c["ws"], c["feat"], c["argmax"], c["d_feat"])
    with pytest.raises(RuntimeError, match="n_docs, C"):
        RF.textcnn_saliency(*args[:4], _dev(c["feat"][:, :5]), *args[5:])
    torch.cuda.synchronize()


def test_rows_are_deterministic_and_batch_independent():
    c = _make(5, 300, 16, 60, [3, 7], [33, 31], seed=71)
    a, b = _run(c), _run(c)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in range(5):
        one = {key: (v[k:k + 1] if key in ("ids", "mask", "argmax", "feat", "d_feat") else v) for key, v in c.items()}
        assert torch.equal(_run(one).view(torch.int32), a[k:k + 1].view(torch.int32)), f"document {k} differs alone"
