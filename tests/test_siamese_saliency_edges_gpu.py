"""rbr_siamese_saliency through functional.siamese_saliency at the shapes that reach each of its branches, against the float64
closed form of tests/siamese_explain_ref.py.  y, a and g are HAND-MADE inputs (the kernel takes them as given), so every edge is
hit on purpose and the forward pass's rounding enters no comparison.

The kernel's tiles (csrc/siamese_saliency.hip): a row is shared by G lanes, the power of two >= min(columns, 64) with a column =
four floats (one on the scalar path: E % 4 != 0 or a table off a 16-byte boundary); a group keeps FLIGHT = 8 rows in flight, so a
wave takes a tile of min(STRETCH, 64 / G * FLIGHT) tokens of one review at a time, STRETCH = 64 being one row index per lane: 8
tokens at E = 260 (G = 64), 16 at E = 128 (G = 32), 64 at E = 4 (G = 1); at most MAX_R = 64 reviews per side row.

Bound, per element (tests/edge_refs.py): (n + 4) * 2^-24 * Abs with the term counts siamese_explain_ref derives on the longest
chain behind an element -- E the row width, F the review vector's width, K the projection's, R the reviews of a side row:
    reviews  n = F + 1          fixed  n = E + 4 [+ F + 3 under the transform]
    through  n = E + 2 F + K + R + 14 [+ F + 3], for pre-activations whose magnitude sum is <= 1 (every case here; asserted)
tests/test_siamese_explain_host.py holds an f32 CPU evaluation in another summation order to the same bound at the same cases.
An element with Abs == 0 has no terms and must be exactly 0.0."""
import functools

import pytest
import torch

import edge_refs as E
import siamese_explain_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRETCH, FLIGHT, MAX_R = 64, 8, 64
NAMES = ("fixed", "through", "reviews")
PER_ROW = ("ids", "word_mask", "rev_mask", "y", "a", "g")
CASES = X.edge_cases(STRETCH, FLIGHT)


def _run(c, table=None):
    from review_based_recommender_amd import functional as RF
    args = [None if c[k] is None else c[k].to(DEV) for k in X.OP_ARGS]
    if table is not None:
        args[0] = table
    return RF.siamese_saliency(*args)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, float64 reference), computed once and shared."""
    c = X.make_case(seed=sorted(CASES).index(name) + 1, **CASES[name])
    ref = X.saliency(*(c[k] for k in X.OP_ARGS))
    assert ref["pre_abs"] <= 1.0
    return c, ref


def _check(name, c, ref, got):
    n, R, T = c["ids"].shape
    for k in NAMES:
        val, ab, cnt = ref[k]
        out = getattr(got, k)
        assert out.dtype == torch.float32 and tuple(out.shape) == ((n, R) if k == "reviews" else (n, R, T)), k
        E.check("siamese-saliency", f"{name}.{k}", out, val, E.bound_of(cnt, ab))


@pytest.mark.parametrize("name", sorted(CASES))
def test_siamese_saliency_at_edge_shapes(name):
    c, ref = _case(name)
    got = _run(c)
    _check(name, c, ref, got)
    assert float(ref["fixed"][1].max()) > 0 and bool((got.fixed != 0).any()) and bool((got.reviews != 0).any())
    read = c["ids"] if c["word_mask"] is None else c["ids"][c["word_mask"]]  # the rows of the unmasked tokens are what is gathered
    assert bool((read == 0).any()) and bool((read == c["V"] - 1).any())      # the padding row and the table's last row among them
    if c["R"] > 1:
        assert bool((got.through != 0).any())
    if CASES[name].get("masks") == "edges":
        wm, last = c["word_mask"], c["n"] - 1
        assert bool((got.fixed.cpu()[~wm] == 0).all()) and bool((got.through.cpu()[~wm] == 0).all())
        assert bool((got.through[last] == 0).all()), "a side row that keeps no review passes nothing through the softmax"
        assert float((c["a"][last] - 1.0 / c["R"]).abs().max()) < 1e-6 and bool((got.fixed[last] != 0).any())
        assert bool((got.fixed[0, c["R"] - 1] == 0).all())                   # the kept review without a word: inv = 1e8, exact 0


def test_fixed_is_complete_without_the_transform():
    """With y the masked average of the very rows the op reads (no transform), sum_t fixed[b, r, t] == reviews[b, r]: each side
    within the bounds of the elements behind it, plus the rounding of y to f32 and the 1e-8 of inv_r."""
    c = X.make_case(3, 4, 2 * FLIGHT + 3, 20, 3, 30, seed=101, masks="edges")
    c["table"] = c["table"] * 0.25                                           # |y| stays below 1, as make_case's projection assumes
    wm = c["word_mask"].double()
    avg = (E.f64(c["table"])[c["ids"]] * wm.unsqueeze(-1)).sum(2) / (wm.sum(-1, keepdim=True) + 1e-8)
    c["y"] = avg.float()
    ref = X.saliency(*(c[k] for k in X.OP_ARGS))
    assert ref["pre_abs"] <= 1.0
    got = _run(c)
    _check("complete", c, ref, got)
    lhs, rhs = got.fixed.double().sum(-1).cpu(), got.reviews.double().cpu()
    y_rounding = E.EPS * E.f64(c["a"]) * (E.f64(c["g"]).abs().unsqueeze(1) * E.f64(c["y"]).abs()).sum(-1)
    slack = (E.bound_of(ref["fixed"][2], ref["fixed"][1]).sum(-1) + E.bound_of(ref["reviews"][2], ref["reviews"][1]) + y_rounding
             + 1e-7 * rhs.abs())
    live = c["word_mask"].any(-1)
    assert int(live.sum()) >= 8 and float(rhs[live].abs().max()) > 0
    ratio = ((lhs - rhs).abs() / slack.clamp_min(1e-300))[live]
    print(f"RATIO siamese-saliency complete.sum_of_fixed_vs_reviews {float(ratio.max()):.4f}")
    assert float(ratio.max()) <= 1.0


def test_misaligned_table_takes_the_scalar_rows():
    """E % 4 == 0 but the table starts 4 bytes off a 16-byte boundary: no 16-byte loads, same bounds."""
    c = X.make_case(3, 3, 9, 8, 3, 11, seed=71, F=6, masks="edges")
    ref = X.saliency(*(c[k] for k in X.OP_ARGS))
    buf = torch.empty(11 * 8 + 1, device=DEV)
    table = buf[1:].view(11, 8)
    table.copy_(c["table"])
    assert table.data_ptr() % 16 == 4 and table.is_contiguous()
    _check("misaligned", c, ref, _run(c, table))


def test_nothing_to_explain_gives_exact_zeros():
    c = X.make_case(3, 3, 9, 12, 3, 11, seed=81, masks="holes")
    c["g"] = torch.zeros_like(c["g"])
    got = _run(c)
    for k in NAMES:
        assert bool((getattr(got, k) == 0).all()), k


def test_empty_batch_cpu_tensors_and_wrong_shapes():
    from review_based_recommender_amd import functional as RF
    c = X.make_case(2, 3, 5, 8, 3, 11, seed=91, F=6)
    args = [None if c[k] is None else c[k].to(DEV) for k in X.OP_ARGS]
    empty = [t if k not in PER_ROW or t is None else t[:0] for k, t in zip(X.OP_ARGS, args)]
    out = RF.siamese_saliency(*empty)
    assert out.fixed.shape == (0, 3, 5) and out.through.shape == (0, 3, 5) and out.reviews.shape == (0, 3)

    def swapped(name, v):
        return [v if k == name else t for k, t in zip(X.OP_ARGS, args)]

    assert RF.siamese_saliency(*swapped("a", args[5].unsqueeze(-1))).fixed.shape == (2, 3, 5)      # the attention's own [n, R, 1]
    with pytest.raises(RuntimeError, match="HIP device"):
        RF.siamese_saliency(*(c[k] for k in X.OP_ARGS))
    with pytest.raises(RuntimeError, match=r"\[n, R, T\]"):
        RF.siamese_saliency(*swapped("ids", args[1][:, :, 0]))
    with pytest.raises(RuntimeError, match="g must be"):
        RF.siamese_saliency(*swapped("g", args[6][:, :5].contiguous()))
    with pytest.raises(RuntimeError, match="transform's weight"):
        RF.siamese_saliency(*swapped("Wt", args[7][:, :7].contiguous()))
    with pytest.raises(RuntimeError, match="needs the transform"):            # F != E without Wt: the library refuses
        RF.siamese_saliency(*swapped("Wt", None))
    big = X.make_case(1, MAX_R + 1, 2, 4, 2, 5, seed=92)
    with pytest.raises(RuntimeError, match=f"R={MAX_R + 1}"):
        _run(big)
    torch.cuda.synchronize()


def test_rows_are_deterministic_and_batch_independent():
    c = X.make_case(5, 7, STRETCH + 9, 108, 32, 60, seed=61, masks="edges")
    a, b = _run(c), _run(c)
    for k in NAMES:
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k
    for r in range(5):
        one = _run({key: (v[r:r + 1] if key in PER_ROW and v is not None else v) for key, v in c.items()})
        for k in NAMES:
            assert torch.equal(getattr(one, k).view(torch.int32), getattr(a, k)[r:r + 1].view(torch.int32)), f"side row {r}: {k} differs alone"
