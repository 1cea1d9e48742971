"""tests/tap_ref.py on the CPU: the float64 restatement of the tap exchange agrees with torch autograd, an f32 emulation of both
row paths of the rebuild (the cold array-order chain, the hot fixed-point cells) and of the tap kernel stays inside the bounds on
every case the GPU test runs, five wrong variants of that arithmetic do not, and the case list covers what it claims to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tap_ref as R

F32 = np.float32


# ----------------------------------------------------------------------------------------------------- agreement with autograd
def _autograd_case(s, seed, use_mask):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(s.V, s.D, generator=g, dtype=torch.float64).requires_grad_(True)
    ids = torch.randint(0, s.V, (s.n_docs, s.L), generator=g)
    mask = (torch.rand(s.n_docs, s.L, generator=g) > 0.25) if use_mask else None
    Ws = [torch.randn(h, s.D, k, generator=g, dtype=torch.float64) * (s.D * k) ** -0.5 for k, h in zip(s.kz, s.ch)]
    bs = [torch.randn(h, generator=g, dtype=torch.float64) * 0.1 for h in s.ch]
    x = F.embedding(ids, table, padding_idx=s.padding_idx if s.padding_idx >= 0 else None)
    if mask is not None:
        x = x.masked_fill(~mask.unsqueeze(-1), 0.0)
    x = x.transpose(1, 2)
    feats, args = [], []
    for w, b, k in zip(Ws, bs, s.kz):
        y = F.conv1d(x, w, b, padding=(k - 1) // 2 if s.pad_mode == R.PAD_SAME else 0)
        y = torch.tanh(y) if s.act == R.TANH else torch.relu(y)
        v, a = y.max(dim=2)                                     # max-pool over the whole length
        feats.append(v)
        args.append(a)
    feat, argmax = torch.cat(feats, 1), torch.cat(args, 1)
    d_feat = torch.randn(feat.shape, generator=g, dtype=torch.float64)
    feat.backward(d_feat)
    return ids, mask, Ws, feat.detach(), argmax, d_feat, table.grad


@pytest.mark.parametrize("shape, use_mask", [
    (R.Shape(3, 14, 8, 9, [1, 3, 5], [3, 4, 2], R.PAD_SAME, R.RELU, 0), True),
    (R.Shape(4, 11, 12, 7, [2, 3, 4], [5, 3, 1], R.PAD_VALID, R.TANH, -1), False),
    (R.Shape(1, 1, 4, 3, [3], [2], R.PAD_SAME, R.RELU, -1), False),                      # a one-token document
], ids=["same-relu-mask-pad", "valid-tanh", "one-token"])
def test_taps_and_rebuild_agree_with_autograd(shape, use_mask):
    """embedding -> masked_fill -> conv1d -> act -> max over the length, in float64: the table gradient is rebuild(taps(...)) at
    n_sets = 1 to 1e-12 relative.  (The reference gives a padding_idx token no gradient; nn.Embedding's padding_idx does that.)"""
    ids, mask, Ws, feat, argmax, d_feat, grad = _autograd_case(shape, 5, use_mask)
    tok, val, _ = R.taps(shape, ids, mask, feat, argmax, d_feat)
    got, _, cnt = R.rebuild(tok, val, Ws, shape.kz, shape.ch, shape.V, shape.D, 1)
    assert int(cnt.sum()) > 0
    assert float((got - grad).abs().max()) <= 1e-12 * float(grad.abs().max())


# ----------------------------------------------------------------------------------------------- f32 emulation of the kernels
def emulate_taps(case, no_same_offset=False, slot_present=False):
    """taps_kernel in f32.  no_same_offset: the 'same' offset (kz - 1) / 2 left out; slot_present: a slot j >= kz treated as one of
    the kernel's."""
    s = case.shape
    C, KF = s.C, s.KF
    j, c, w, _, present = R.entry_maps(s.kz, s.ch, C * KF)
    kzc = torch.tensor(s.kz)[w]
    if slot_present:
        present = torch.ones_like(present)
    off = (kzc - 1) // 2 if (s.pad_mode == R.PAD_SAME and not no_same_offset) else torch.zeros_like(kzc)
    f, d = case.feat.numpy().astype(F32), case.d_feat.numpy().astype(F32)
    g = np.where(f > 0, d, F32(0)) if s.act == R.RELU else d * (F32(1) - f * f)
    g = torch.from_numpy(g.astype(F32))[:, c]
    p = case.argmax.long()[:, c] + (j - off).unsqueeze(0)
    inside = (p >= 0) & (p < s.L)
    pc = p.clamp(0, s.L - 1)
    t = torch.gather(case.ids, 1, pc)
    ok = present.unsqueeze(0) & (g != 0) & inside & (t != s.padding_idx)
    if case.mask is not None:
        ok = ok & torch.gather(case.mask, 1, pc)
    return torch.where(ok, t, torch.full_like(t, -1)).reshape(-1), torch.where(ok, g, torch.zeros_like(g)).reshape(-1)


def emulate_rebuild(case, drop_tap=False, shift_col=False, no_div=False):
    """taps_rows_kernel's arithmetic in f32 numpy, a token at a time, the taps in array order (the stable sort keeps it).
    cnt <= 16: sum += (val * inv_sets) * WT[col, :], one chain.  cnt > 16: rint(val * 2^40) summed per cell in int64, the cell
    converted to f32 and scaled by gscale = 1 / (2^40 * n_sets); each wave quarter of KGW cells is one chain over its non-zero
    cells, and the four partials are added.  drop_tap / shift_col: the first tap of the token with the most taps is lost / lands
    one channel to the side; no_div: the division by n_sets is left out."""
    s, n_sets = case.shape, case.n_sets
    V, D, cp, KGW = s.V, s.D, s.cp_real, s.KGW
    tok, val = case.tok.long().clone(), case.val.numpy().astype(F32)
    _, _, _, col, _ = R.entry_maps(s.kz, s.ch, tok.numel())
    col = col.clone()
    WT = torch.cat([w.permute(2, 0, 1).reshape(-1, D) for w in case.Ws]).numpy().astype(F32)
    if drop_tap or shift_col:
        victim = int(torch.tensor(case.counts).argmax())
        k = int(torch.nonzero(tok == victim)[0])
        if drop_tap:
            tok[k] = -1
        else:
            col[k] = col[k] + 1 if col[k] + 1 < cp else col[k] - 1
    two40 = F32(2.0 ** 40)
    gscale = F32(1.0) / (two40 * F32(1 if no_div else n_sets))
    inv_sets = gscale * two40
    out = np.zeros((V, D), dtype=F32)
    tok_np, col_np = tok.numpy(), col.numpy()
    order = np.argsort(tok_np, kind="stable")
    for v in range(V):
        ks = order[np.searchsorted(tok_np[order], v, "left"):np.searchsorted(tok_np[order], v, "right")]
        if len(ks) == 0:
            continue
        if len(ks) <= R.TAPS_COLD:
            acc = np.zeros(D, dtype=F32)
            for k in ks:
                acc = (acc + (val[k] * inv_sets) * WT[col_np[k]]).astype(F32)
            out[v] = acc
            continue
        cells = np.zeros(cp, dtype=np.int64)
        np.add.at(cells, col_np[ks], np.rint(val[ks].astype(np.float64) * 2.0 ** 40).astype(np.int64))
        x = cells.astype(F32) * gscale
        parts = []
        for wv in range(R.WAVES):
            acc = np.zeros(D, dtype=F32)
            for kk in range(wv * KGW, min(cp, (wv + 1) * KGW)):
                if x[kk] != 0:
                    acc = (acc + x[kk] * WT[kk]).astype(F32)
            parts.append(acc)
        out[v] = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    return torch.from_numpy(out)


_REF = {}


def _rebuild_ref(case):
    if case.name not in _REF:
        s = case.shape
        _REF[case.name] = R.rebuild(case.tok, case.val, case.Ws, s.kz, s.ch, s.V, s.D, case.n_sets)
    return _REF[case.name]


REBUILD = R.rebuild_cases() + R.owner_cases() + [R.cap_case(0)]
TAPS = R.taps_cases()


def _taps_ref(case):
    return R.taps(case.shape, case.ids, case.mask, case.feat, case.argmax, case.d_feat)


@pytest.mark.parametrize("case", REBUILD, ids=lambda c: c.name)
def test_f32_rebuild_stays_inside_the_bounds(case):
    ref, bound, cnt = _rebuild_ref(case)
    assert cnt.tolist() == case.counts
    got = emulate_rebuild(case)
    assert bool((got[cnt == 0] == 0).all())
    r = R.ratio_of(got, ref, bound)
    print(f"RATIO host-rebuild {case.name} {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", TAPS, ids=lambda c: c.name)
def test_f32_taps_stay_inside_the_bounds(case):
    tok, val = emulate_taps(case)
    r = R.taps_ratio(tok, val, *_taps_ref(case))
    print(f"RATIO host-taps {case.name} {r:.4f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mutation", ["drop_tap", "shift_col", "no_div"])
def test_a_wrong_rebuild_leaves_the_bounds(mutation):
    """One tap dropped, one tap's column shifted by one channel, the division by n_sets left out: err / bound > 1 on at least
    one case (no_div can only show where n_sets > 1)."""
    caught = []
    for case in REBUILD:
        ref, bound, _ = _rebuild_ref(case)
        if R.ratio_of(emulate_rebuild(case, **{mutation: True}), ref, bound) > 1.0:
            caught.append(case.name)
    print(f"{mutation}: caught on {len(caught)} of {len(REBUILD)} cases")
    assert caught, mutation
    # the hot paths notice too: one tap among the 8193 of a split token, one among the 594 of the wide row
    assert {"split", "wide"} <= set(caught)


@pytest.mark.parametrize("mutation", ["no_same_offset", "slot_present"])
def test_wrong_taps_are_noticed(mutation):
    """The 'same' offset (kz - 1) / 2 left out; a slot j >= kz treated as present."""
    caught = [case.name for case in TAPS if R.taps_ratio(*emulate_taps(case, **{mutation: True}), *_taps_ref(case)) > 1.0]
    print(f"{mutation}: caught on {len(caught)} of {len(TAPS)} cases")
    assert caught, mutation


def test_rebuild_refuses_a_tap_beyond_its_kernel():
    case = R.rebuild_cases()[1]
    s = case.shape
    j, _, _, _, present = R.entry_maps(s.kz, s.ch, case.tok.numel())
    tok = case.tok.clone()
    tok[int(torch.nonzero(~present)[0])] = 0
    with pytest.raises(ValueError):
        R.rebuild(tok, case.val, case.Ws, s.kz, s.ch, s.V, s.D, case.n_sets)


# ------------------------------------------------------------------------------------------------------------------- coverage
def test_the_cases_cover_the_thresholds_and_paths():
    cases = R.rebuild_cases()
    counts = {c for case in cases for c in case.counts}
    assert {0, 1, 16, 17, 4096, 4097} <= counts and any(c > 8192 for c in counts)
    assert {15, 18} <= counts
    assert any(case.shape.cp_real % 4 != 0 for case in cases)
    assert any(case.shape.KG > 256 and case.shape.KGW > 64 for case in cases)
    assert {4, 300, 516} <= {case.shape.D for case in cases}
    assert {1, 2, 8} <= {case.n_sets for case in cases}
    assert all(case.tok.numel() <= 41000 for case in cases + R.owner_cases() + [R.cap_case(1)])
    # all taps of a token in one cell, and a token with a tap in every cell, the cells either side of each KGW border among them
    by = {case.name: case for case in cases}
    for name, token, n_cells in (("thr-single", 5, 1), ("thr-spread", 6, 45), ("wide", 1, 297), ("split", 11, 64)):
        case = by[name]
        _, _, _, col, _ = R.entry_maps(case.shape.kz, case.shape.ch, case.tok.numel())
        assert len(set(col[case.tok == token].tolist())) == n_cells, name
    s = by["thr-spread"].shape
    _, _, _, col, _ = R.entry_maps(s.kz, s.ch, by["thr-spread"].tok.numel())
    cells17 = set(col[by["thr-spread"].tok == 4].tolist())
    assert {s.cp_real - 1} | {b + d for b in (s.KGW, 2 * s.KGW, 3 * s.KGW) for d in (-1, 0)} <= cells17
    # a token's taps come from more than one set (the order of the sets matters to the array-order chain)
    n = by["thr-spread"].shape.n_items
    assert len(set((torch.nonzero(by["thr-spread"].tok == 3).flatten() // n).tolist())) == 2
    # owner partition: V < n_sets, V % n_sets != 0, a rank with tokens and no taps; the capacity case sits exactly on the cap
    own = {(c.n_sets, c.shape.V): c for c in R.owner_cases()}
    assert set(own) == {(n, v) for n in (1, 2, 3, 8) for v in (1, 10, 64)}
    c = own[(3, 10)]
    assert not bool(((c.tok >= 0) & (c.tok % 3 == 1)).any()) and bool((c.tok % 3 == 2).any())
    assert any(x > 16 for x in own[(8, 64)].counts) and any(0 < x <= 16 for x in own[(8, 64)].counts)
    for extra in (0, 1):
        c = R.cap_case(extra)
        total = c.tok.numel()
        assert total == 13824 and R.owner_cap(total, 3) == 13312
        assert int(((c.tok >= 0) & (c.tok % 3 == 0)).sum()) == 13312 + extra
    # taps: every branch the kernel has is met by some case
    tc = {c.name: c for c in TAPS}
    assert any(c.shape.n_items < 256 for c in TAPS) and any(c.shape.n_items > 256 and c.shape.n_items % 256 for c in TAPS)
    assert any(c.shape.n_items % 256 == 0 for c in TAPS)
    assert any(c.mask is None for c in TAPS) and any(c.mask is not None and not bool(c.mask.any()) for c in TAPS)
    assert {-1, 0} <= {c.shape.padding_idx for c in TAPS} and any(c.shape.padding_idx == c.shape.V - 1 for c in TAPS)
    assert any(c.shape.L < max(c.shape.kz) for c in TAPS)
    for c in TAPS:
        if c.shape.padding_idx >= 0:
            assert bool((c.ids == c.shape.padding_idx).any()), c.name
    v = tc["valid-tanh"]
    assert bool((v.feat == 1.0).any()) and bool((v.feat == -1.0).any()) and bool((v.d_feat == 0).any())
    assert bool((tc["same-k139-pad0"].feat == 0).any())
    o = 0
    for k, h in zip(v.shape.kz, v.shape.ch):                    # argmax 0 and L - kz in every bank
        am = v.argmax[:, o:o + h]
        assert int(am.min()) == 0 and int(am.max()) == v.shape.L - k
        o += h
    w = tc["same-k139-pad-1"]
    o = 0
    for h in w.shape.ch:
        am = w.argmax[:, o:o + h]
        assert int(am.min()) == 0 and int(am.max()) == w.shape.L - 1
        o += h
    # ... and has an effect: windows over either end, masked positions, padding tokens and slots beyond the kernel all drop taps
    tok, _, _ = _taps_ref(w)
    assert bool((tok == -1).any()) and bool((tok >= 0).any())
