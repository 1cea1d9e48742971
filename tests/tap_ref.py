"""Plain float64 restatement, with per-element error bounds, of the tap exchange of the word-table gradient (rbr_textcnn_bwd_taps,
rbr_textcnn_dtable_from_taps and its owner partition; taps_*_kernel in csrc/textcnn_prod.hip), and the edge cases the tests run:
tests/test_tap_kernels_edges_gpu.py compares the kernels with it, tests/test_tap_ref_host.py checks the formulas against torch
autograd in float64, that an f32 emulation of the kernels' arithmetic stays inside the bounds, and that wrong variants do not.

The tap layout is rbr_hip.h's: one set holds n_docs * C * KF entries (C = all channels, KF = the widest kernel), entry
e = ((doc * C + c) * KF + j).  Bank w owns the channels [ch_off[w], ch_off[w] + ch[w]) and the product columns
poff[w] + j * ch[w] + cl, j < kz[w]: a row of G has cp_real = sum kz[w] * ch[w] columns ("cells").

Bounds of the rebuild (EPS = 2^-24; Abs = the expression on magnitudes; cnt = taps of the token, nnz = its non-empty cells,
m[v, k] = taps in cell (v, k)):
  cnt <= 16  one wave adds val / n_sets * WT[col, :] in array order in f32:            (cnt + 4) * EPS * Abs
  cnt >  16  every tap is rounded to 2^-40 units (half a unit each), the cells are summed exactly in 64-bit integers, converted
             to f32 and scaled (int64 -> f32, the scale and its own rounding), multiplied out in four per-wave f32 chains whose
             partials are added (three adds):                  (nnz + 8) * EPS * Abs + 2^-41 / n_sets * (m @ |WT|)
  cnt == 0   no terms: the row is exactly 0.
"""
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from edge_refs import EPS, bound_of, check, f64

PAD_SAME, PAD_VALID = 0, 1        # RBR_PAD_* of rbr_hip.h
RELU, TANH = 0, 1                 # RBR_ACT_*
TAPS_COLD = 16                    # kTapsCold of textcnn_prod.hip: wave-per-token rows up to here
TAPS_SPLIT = 4096                 # kTapsSplit: taps of one token summed by one workgroup
WAVES = 4                         # kWavesPerWG: the sparse product cuts a row of G into four wave quarters of KGW cells


@dataclass
class Shape:
    n_docs: int
    L: int
    D: int
    V: int
    kz: List[int]
    ch: List[int]
    pad_mode: int = PAD_SAME
    act: int = RELU
    padding_idx: int = -1

    @property
    def C(self):
        return sum(self.ch)

    @property
    def KF(self):
        return max(self.kz)

    @property
    def n_items(self):
        return self.n_docs * self.C * self.KF

    @property
    def cp_real(self):
        return sum(k * c for k, c in zip(self.kz, self.ch))

    @property
    def KG(self):
        return (self.cp_real + 3) // 4 * 4

    @property
    def KGW(self):
        return ((self.KG // 4 + WAVES - 1) // WAVES) * 4


def shape_of(d):
    """A Shape from a Shape or from anything with the descriptor's fields (a ctypes rbr_textcnn_desc: kz / ch hold n_widths banks)."""
    if isinstance(d, Shape):
        return d
    n = int(getattr(d, "n_widths", len(d.kz)))
    return Shape(int(d.n_docs), int(d.L), int(d.D), int(d.V), [int(k) for k in list(d.kz)[:n]], [int(c) for c in list(d.ch)[:n]],
                 int(d.pad_mode), int(d.act), -1 if d.padding_idx is None else int(d.padding_idx))


def entry_maps(kz, ch, n_entries, device="cpu"):
    """For the entries k = 0 .. n_entries - 1 of whole concatenated sets: (j, c, bank, column, present).  `present`: j < kz[bank];
    the column of an absent slot is meaningless."""
    C, KF = sum(ch), max(kz)
    bank_of_c, ch_off, poff, o, p = [], [], [], 0, 0
    for w, (k, h) in enumerate(zip(kz, ch)):
        bank_of_c += [w] * h
        ch_off.append(o)
        poff.append(p)
        o, p = o + h, p + k * h
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=device)
    k = torch.arange(n_entries, dtype=torch.int64, device=device)          # a set is a whole number of documents of C * KF entries
    j, c = k % KF, (k // KF) % C
    w = t(bank_of_c)[c]
    col = t(poff)[w] + j * t(ch)[w] + (c - t(ch_off)[w])
    return j, c, w, col, j < t(kz)[w]


# --------------------------------------------------------------------------------------------------------------------- taps
def taps(desc_like, ids, mask, feat, argmax, d_feat):
    """rbr_textcnn_bwd_taps -> (tok int64 [n], val f64 [n], bval f64 [n]).  Entry ((doc * C + c) * KF + j) is the tap of channel
    c's window at p = argmax + j - (kz - 1) / 2 ('same') or argmax + j (valid); tok = -1, val = 0 for a slot beyond the bank's
    kernel, g == 0, a masked position, a position outside [0, L) and padding_idx.  ReLU: g = d_feat where feat > 0, bound 0
    (exact); tanh: g = d_feat * (1 - feat^2), bound 3 * EPS * |d_feat| * (1 + feat^2)."""
    s = shape_of(desc_like)
    n_docs, L, C, KF = s.n_docs, s.L, s.C, s.KF
    ids = ids.detach().cpu().long()
    f, d, am = f64(feat), f64(d_feat), argmax.detach().cpu().long()
    j, c, w, _, present = entry_maps(s.kz, s.ch, C * KF)
    kzc = torch.tensor(s.kz)[w]
    off = (kzc - 1) // 2 if s.pad_mode == PAD_SAME else torch.zeros_like(kzc)
    p = am[:, c] + (j - off).unsqueeze(0)                                        # [n_docs, C * KF]
    if s.act == RELU:
        g, bg = torch.where(f > 0, d, torch.zeros_like(d)), torch.zeros_like(d)
    else:
        g, bg = d * (1 - f * f), 3 * EPS * d.abs() * (1 + f * f)
    g, bg = g[:, c], bg[:, c]
    inside = (p >= 0) & (p < L)
    pc = p.clamp(0, L - 1)
    t = torch.gather(ids, 1, pc)
    ok = present.unsqueeze(0) & (g != 0) & inside & (t != s.padding_idx)
    if mask is not None:
        ok = ok & torch.gather(mask.detach().cpu() != 0, 1, pc)
    tok = torch.where(ok, t, torch.full_like(t, -1)).reshape(-1)
    zero = torch.zeros_like(g)
    return tok, torch.where(ok, g, zero).reshape(-1), torch.where(ok, bg, zero).reshape(-1)


def taps_ratio(tok_got, val_got, tok_ref, val_ref, bval):
    """Largest err / bound of a tap set; inf when a token differs, or when an absent tap's value is not exactly 0."""
    tok_got, val_got = tok_got.detach().cpu().long(), val_got.detach().cpu().double()
    if not torch.equal(tok_got, tok_ref) or bool((val_got[tok_ref < 0] != 0).any()):
        return float("inf")
    return ratio_of(val_got, val_ref, bval)


def ratio_of(got, ref, bound):
    got = got.detach().cpu().double()
    ref, bound = ref.cpu().reshape(got.shape), bound.cpu().reshape(got.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    return float(r.max()) if r.numel() else 0.0


def check_taps(family, name, tok_got, val_got, ref):
    """tok exactly equal, val == 0 exactly where tok == -1, val inside bval (edge_refs.check prints the RATIO line)."""
    tok_ref, val_ref, bval = ref
    tok_got = tok_got.detach().cpu().long()
    assert torch.equal(tok_got, tok_ref), f"{family} {name}: tokens differ at entries {torch.nonzero(tok_got != tok_ref).flatten()[:8].tolist()}"
    assert bool((val_got.detach().cpu()[tok_ref < 0] == 0).all()), f"{family} {name}: an absent tap carries a value"
    return check(family, name, val_got, val_ref, bval)


# ------------------------------------------------------------------------------------------------------------------ rebuild
def rebuild(tok, val, Ws, kz, ch, V, D, n_sets):
    """rbr_textcnn_dtable_from_taps from ANY tap arrays of n_sets concatenated sets -> (dtable f64 [V, D], bound f64 [V, D],
    count int64 [V]).  The column of entry e is poff[w] + j * ch[w] + (c - ch_off[w]), WT[col, :] = W_w[cl, :, j], the value
    (G @ WT) / n_sets; the bounds are the module docstring's.  Computes on the device of `tok` (the cfg2-sized check runs it
    on the GPU).  A tap in a slot beyond its bank's kernel is outside the contract and refused."""
    dev = tok.device
    tok, val = tok.detach().long(), val.detach().double()
    cp = sum(k * c for k, c in zip(kz, ch))
    _, _, _, col, present = entry_maps(kz, ch, tok.numel(), dev)
    keep = tok >= 0
    if bool((keep & ~present).any()):
        raise ValueError("a tap sits in a slot beyond its bank's kernel")
    if bool((tok[keep] >= V).any()):
        raise ValueError("a tap names a token outside the table")
    idx = tok[keep] * cp + col[keep]
    z = lambda: torch.zeros(V * cp, dtype=torch.float64, device=dev)
    G = z().index_add_(0, idx, val[keep]).view(V, cp)
    A = z().index_add_(0, idx, val[keep].abs()).view(V, cp)
    m = z().index_add_(0, idx, torch.ones_like(val[keep])).view(V, cp)
    WT = torch.cat([w.detach().to(dev).double().permute(2, 0, 1).reshape(-1, D) for w in Ws])           # [(w, j, cl), D]
    value, ab = (G @ WT) / n_sets, (A @ WT.abs()) / n_sets
    cnt, nnz = m.sum(1, keepdim=True), (m > 0).double().sum(1, keepdim=True)
    hot = (nnz + 8) * EPS * ab + (2.0 ** -41 / n_sets) * (m @ WT.abs())
    bound = torch.where(cnt <= TAPS_COLD, bound_of(cnt, ab), hot)
    return value, bound, cnt.reshape(-1).long()


def owner_cap(total, n_sets):
    """Entries the owner partition's sort is sized for.  Mirrors taps_owner_cap in csrc/textcnn_prod.hip."""
    return min(total, 2 * ((total + n_sets - 1) // n_sets) + 4096)


# -------------------------------------------------------------------------------------------------------------------- cases
@dataclass
class TapsCase:
    """Hand-built inputs of rbr_textcnn_bwd_taps."""
    name: str
    shape: Shape
    ids: torch.Tensor
    mask: Optional[torch.Tensor]
    feat: torch.Tensor
    argmax: torch.Tensor
    d_feat: torch.Tensor


def _taps_case(name, shape, seed, mask_p, edge_argmax=True, all_masked=False):
    s = shape
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, s.V, (s.n_docs, s.L), generator=g)
    ids[:, 0], ids[:, -1] = 0, s.V - 1                      # the tokens a padding_idx of 0 / V - 1 names are present, at both ends
    if s.L > 2:
        ids[0, 1], ids[0, s.L // 2] = s.V - 1, 0
    mask = None if mask_p is None else torch.rand(s.n_docs, s.L, generator=g) >= mask_p
    if all_masked:
        mask = torch.zeros(s.n_docs, s.L, dtype=torch.bool)
    C = s.C
    kzc = torch.tensor([k for k, h in zip(s.kz, s.ch) for _ in range(h)])
    last = (s.L - kzc) if s.pad_mode == PAD_VALID else torch.full_like(kzc, s.L - 1)       # the last window of each channel's pool
    argmax = (torch.rand(s.n_docs, C, generator=g) * (last + 1)).long().clamp(max=last.unsqueeze(0).expand(s.n_docs, C))
    if edge_argmax:                                         # the first and the last window in every bank (windows over either end)
        o = 0
        for h in s.ch:
            argmax[0, o] = 0
            argmax[-1, o + h - 1] = last[o + h - 1]
            o += h
    d_feat = torch.randn(s.n_docs, C, generator=g)
    if s.act == TANH:
        feat = torch.tanh(torch.randn(s.n_docs, C, generator=g) * 1.5)
        feat.view(-1)[1::7] = 1.0                           # saturated: g == 0 exactly
        feat.view(-1)[3::11] = -1.0
    else:
        feat = torch.randn(s.n_docs, C, generator=g)
        feat.view(-1)[1::5] = 0.0                           # ReLU at 0: no gradient
    d_feat.view(-1)[2::9] = 0.0
    return TapsCase(name, s, ids, mask, feat.float(), argmax.int(), d_feat.float())


def taps_cases():
    out = []
    for pad in (-1, 0, 6):                                  # none, the first and the last token (V = 7)
        out.append(_taps_case(f"same-k139-pad{pad}", Shape(3, 12, 4, 7, [1, 3, 9], [3, 5, 2], PAD_SAME, RELU, pad), 1, 0.3))   # 270 entries
    out.append(_taps_case("same-L1", Shape(1, 1, 4, 3, [3], [2], PAD_SAME, RELU, -1), 2, None))                       # 6 entries
    out.append(_taps_case("same-L3-k9", Shape(2, 3, 4, 5, [9, 1], [2, 1], PAD_SAME, RELU, 0), 3, 0.2))                # L < kz
    out.append(_taps_case("valid-tanh", Shape(2, 9, 4, 6, [2, 3, 4], [33, 31, 1], PAD_VALID, TANH, 5), 4, None))      # 520 entries
    out.append(_taps_case("valid-tanh-mask", Shape(4, 16, 4, 6, [2, 3, 4], [33, 31, 1], PAD_VALID, TANH, -1), 5, 0.4))
    out.append(_taps_case("same-nomask", Shape(4, 16, 4, 9, [3, 5], [7, 9], PAD_SAME, RELU, 0), 6, None))             # 320 entries
    out.append(_taps_case("same-tanh", Shape(4, 16, 4, 9, [3, 5], [7, 9], PAD_SAME, TANH, 8), 7, 0.3))
    out.append(_taps_case("all-masked", Shape(2, 10, 4, 5, [3, 5], [2, 3], PAD_SAME, RELU, -1), 8, 0.0, all_masked=True))
    out.append(_taps_case("grid-768", Shape(16, 8, 4, 5, [1, 3], [8, 8], PAD_VALID, RELU, -1), 9, 0.2))               # whole workgroups
    return out


@dataclass
class RebuildCase:
    """Synthetic taps of n_sets concatenated sets: every token's tap count and cells chosen exactly."""
    name: str
    shape: Shape
    n_sets: int
    tok: torch.Tensor            # int32 [n_sets * n_items]
    val: torch.Tensor            # f32
    Ws: List[torch.Tensor]       # [ch, D, kz] per bank
    counts: List[int] = field(default_factory=list)


class _Slots:
    """The slots of n_sets tap sets by product column; a column's slots are handed out document by document, the sets in turn."""

    def __init__(self, shape, n_sets):
        n, total = shape.n_items, shape.n_items * n_sets
        _, _, _, col, present = entry_maps(shape.kz, shape.ch, total)
        k = torch.arange(total)
        order = torch.argsort((k % n) * n_sets + k // n)
        self.free = [deque() for _ in range(shape.cp_real)]
        for i in order.tolist():
            if present[i]:
                self.free[int(col[i])].append(i)
        self.tok = torch.full((total,), -1, dtype=torch.int32)

    def put(self, token, cols):
        for c in cols:
            self.tok[self.free[c].popleft()] = token


def border_cells(shape):
    """The last real column, then the cells either side of every wave-quarter (KGW) border and of every 64-lane ballot border
    inside a quarter, then every other cell."""
    cp, KGW = shape.cp_real, shape.KGW
    first = [cp - 1]
    for w in range(WAVES):
        for b in ([w * KGW] if w else []) + list(range(w * KGW + 64, (w + 1) * KGW, 64)):
            first += [b - 1, b]
    first = [c for i, c in enumerate(first) if 0 <= c < cp and c not in first[:i]]
    return first + [c for c in range(cp) if c not in first]


def _rebuild_case(name, shape, n_sets, plan, seed, scale=1.0):
    """plan: (token, count, 'spread' | 'single' | column) -- spread walks border_cells() round and round, single puts every tap
    into one cell of the token's own (border_cells()[token])."""
    slots, cells = _Slots(shape, n_sets), border_cells(shape)
    counts = [0] * shape.V
    for token, count, where in plan:
        cols = [cells[i % len(cells)] for i in range(count)] if where == "spread" else \
            [cells[token % len(cells)] if where == "single" else int(where)] * count
        slots.put(token, cols)
        counts[token] += count
    g = torch.Generator().manual_seed(seed)
    val = torch.randn(slots.tok.numel(), generator=g) * scale
    val = torch.where(slots.tok >= 0, val, torch.zeros_like(val))
    Ws = [torch.randn(h, shape.D, k, generator=g) * (shape.D * k) ** -0.5 for k, h in zip(shape.kz, shape.ch)]
    return RebuildCase(name, shape, n_sets, slots.tok, val.float(), [w.float() for w in Ws], counts)


def rebuild_cases():
    out = [_rebuild_case("minimal", Shape(1, 1, 4, 1, [1], [1]), 1, [(0, 1, "single")], 20)]
    # thresholds of the cold path: cp_real = 45 (KG = 48, KGW = 12), 24 slots per cell
    thr = Shape(12, 8, 12, 11, [3, 5], [5, 6])
    ladder = lambda how: [(1, 1, how), (2, 15, how), (3, 16, how), (4, 17, how), (5, 18, how), (10, 3, how)]
    out.append(_rebuild_case("thr-single", thr, 2, ladder("single") + [(6, 20, 0)], 21))
    out.append(_rebuild_case("thr-spread", thr, 2, ladder("spread") + [(6, 45, "spread"), (7, 100, "spread")], 22))
    out.append(_rebuild_case("thr-spread-2^-30", thr, 2, ladder("spread") + [(6, 45, "spread"), (7, 100, "spread")], 23, 2.0 ** -30))
    out.append(_rebuild_case("thr-spread-2^10", thr, 2, ladder("spread") + [(6, 45, "spread"), (7, 100, "spread")], 24, 2.0 ** 10))
    # split tokens: 64 cells, 512 slots per cell, 32768 valid slots in 8 sets; V % n_sets != 0
    split = Shape(64, 8, 20, 29, [3, 5], [8, 8])
    plan = [(3, 4096, "spread"), (4, 4097, "spread"), (11, 8193, "spread"), (28, 200, "single"), (5, 17, "spread"), (6, 16, "spread"),
            (0, 1, "spread"), (9, 7, "single"), (17, 100, "spread"), (27, 2, 63)]
    out.append(_rebuild_case("split", split, 8, plan, 25))
    # wide rows: KG = 300 (297 real), KGW = 76: two ballot rounds per wave quarter; 16 slots per cell
    wide = Shape(8, 9, 300, 9, [9], [33])
    plan = [(0, 594, "spread"), (1, 297, "spread"), (2, 16, "spread"), (3, 17, "spread"), (4, 8, "single"), (8, 1, "single")]
    out.append(_rebuild_case("wide", wide, 2, plan, 26))
    # D > 512: the second pass over the row's float4 columns (one float4 in it)
    d516 = Shape(8, 4, 516, 5, [3], [4])
    out.append(_rebuild_case("d516", d516, 1, [(0, 24, "spread"), (1, 16, "spread"), (2, 17, "spread"), (4, 3, "single")], 27))
    return out


def owner_cases():
    """(n_sets, V) in {1, 2, 3, 8} x {1, 10, 64}: V < n_sets, V % n_sets != 0, ranks whose share of the vocabulary is empty; in
    (3, 10) rank 1 owns tokens but no taps.  Tokens are drawn with a heavy head so that cold and hot rows both occur."""
    out = []
    for n_sets in (1, 2, 3, 8):
        for V in (1, 10, 64):
            s = Shape(8, 8, 8, V, [3, 5], [3, 2])                      # cp_real = 19, 152 valid slots per set
            g = torch.Generator().manual_seed(100 * n_sets + V)
            total = s.n_items * n_sets
            _, _, _, _, present = entry_maps(s.kz, s.ch, total)
            t = (torch.rand(total, generator=g) ** 3 * V).long().clamp(max=V - 1)
            if (n_sets, V) == (3, 10):
                t = torch.where(t % 3 == 1, t - 1, t)
            live = present & (torch.rand(total, generator=g) < 0.9)
            tok = torch.where(live, t, torch.full_like(t, -1)).int()
            val = torch.where(live, torch.randn(total, generator=g), torch.zeros(total)).float()
            Ws = [(torch.randn(h, s.D, k, generator=g) * (s.D * k) ** -0.5).float() for k, h in zip(s.kz, s.ch)]
            out.append(RebuildCase(f"own-n{n_sets}-V{V}", s, n_sets, tok, val, Ws, torch.bincount(t[live], minlength=V).tolist()))
    return out


def cap_case(extra):
    """Rank 0 of 3 owns exactly owner_cap + extra taps: 8 documents, one 'same' bank of 9 x 64 -> 13824 slots, cap 13312."""
    s, n_sets = Shape(8, 9, 4, 7, [9], [64]), 3
    total = s.n_items * n_sets
    cap = owner_cap(total, n_sets)
    assert total > cap
    g = torch.Generator().manual_seed(300)
    where = torch.randperm(total, generator=g)
    tok = torch.empty(total, dtype=torch.int32)
    tok[where[:cap + extra]] = (torch.randint(0, 3, (cap + extra,), generator=g) * 3).int()             # 0, 3, 6: rank 0's
    rest = torch.tensor([1, 2, 4, 5, -1], dtype=torch.int32)[torch.randint(0, 5, (total - cap - extra,), generator=g)]
    tok[where[cap + extra:]] = rest
    val = torch.where(tok >= 0, torch.randn(total, generator=g), torch.zeros(total)).float()
    Ws = [(torch.randn(64, s.D, 9, generator=g) * (s.D * 9) ** -0.5).float()]
    return RebuildCase(f"cap+{extra}", s, n_sets, tok, val, Ws, torch.bincount(tok[tok >= 0].long(), minlength=s.V).tolist())
