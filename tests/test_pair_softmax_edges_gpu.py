"""The in-batch softmax kernels (csrc/pair_softmax.hip) at edge shapes against the float64 restatement of tests/softmax_ref.py,
within its per-element bounds: both score modes, B at wave and workgroup boundaries, K below, off and above the 32-lane chunk,
with and without each bias and logq, two temperatures, with and without an explicit dropout multiplier; the mask fixture; exact
zeros, run-to-run bits and the two backward routes; extreme scores; the in-kernel dropout draw; refused shapes."""
import pytest
import torch

import softmax_ref as SR
from edge_refs import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (row_bias, col_bias, logq, temperature, explicit drop): with and without each, both temperatures, both dropout settings
CONFIGS = [(True, True, True, 1.0, False), (False, False, False, 0.25, True), (True, False, False, 0.25, False),
           (False, True, True, 1.0, True)]


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(c, temperature=1.0, root=None, p_drop=0.0, seen="case", u_ids=None, i_ids=None):
    """functional.pair_softmax_loss on the device for the case -> {name: tensor} (loss, pos and the gradients after backward)."""
    from review_based_recommender_amd import functional as RF
    leaves = {k: _dev(c[k]).requires_grad_(True) for k in ("ul", "il", "h", "row_bias", "col_bias") if c.get(k) is not None}
    seen = c["seen"] if seen == "case" else seen
    loss, pos = RF.pair_softmax_loss(leaves["ul"], leaves["il"], _dev(c["u_ids"] if u_ids is None else u_ids),
                                     _dev(c["i_ids"] if i_ids is None else i_ids), "fm" if c["fm"] else "dot", h=leaves.get("h"),
                                     row_bias=leaves.get("row_bias"), col_bias=leaves.get("col_bias"), drop=_dev(c.get("drop")),
                                     seen=None if seen is None else (_dev(seen[0]), _dev(seen[1])), item_lo=c["item_lo"],
                                     logq=_dev(c.get("logq")), temperature=temperature, p_drop=p_drop)
    assert not pos.requires_grad
    loss.backward(RF.unit_scalar(DEV) if root is None else root)
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "pos": pos}
    for name, leaf in (("d_ul", "ul"), ("d_il", "il"), ("d_h", "h"), ("d_col_bias", "col_bias"), ("d_row_bias", "row_bias")):
        if leaf in leaves:
            out[name] = leaves[leaf].grad
    return out


def _ref(c, temperature=1.0, d_loss=1.0, seen="case", u_ids=None, i_ids=None):
    seen = c["seen"] if seen == "case" else seen
    return SR.pair_softmax_ref(c["ul"], c["il"], c["u_ids"] if u_ids is None else u_ids, c["i_ids"] if i_ids is None else i_ids, c["fm"],
                               c["h"], c["row_bias"], c["col_bias"], c.get("drop"), seen, c["item_lo"], c.get("logq"), 1.0 / temperature,
                               d_loss)


def _compare(family, got, ref):
    """Every element of every output against the restatement, within its bound; d_row_bias exactly zeros."""
    names = [n for n in ("loss", "pos", "d_ul", "d_il", "d_h", "d_col_bias") if n in ref]
    assert set(names) <= set(got), (names, sorted(got))
    for n in names:
        check(family, n, got[n], ref[n][0], ref[n][1])
    if "d_row_bias" in got:
        assert int(torch.count_nonzero(got["d_row_bias"])) == 0 and not bool(torch.signbit(got["d_row_bias"]).any())


@pytest.mark.parametrize("K", [1, 5, 33])
@pytest.mark.parametrize("B", [1, 2, 65, 257])
@pytest.mark.parametrize("fm", [True, False], ids=["fm", "dot"])
def test_every_output_within_the_float64_bounds(fm, B, K):
    for n, (rb, cb, lq, temp, drop) in enumerate(CONFIGS):
        c = SR.random_case(B, K, fm, 1000 * n + 10 * B + K, with_rb=rb, with_cb=cb, with_logq=lq, with_drop=drop)
        _compare(f"softmax {'fm' if fm else 'dot'} B={B} K={K} cfg{n}", _run(c, temp), _ref(c, temp))


@pytest.mark.parametrize("fm", [True, False], ids=["fm", "dot"])
def test_mask_fixture_rows(fm):
    u_ids, i_ids, seen, item_lo, allowed = SR.mask_fixture()
    c = SR.random_case(8, 5, fm, 77, with_rb=True, with_cb=True, with_logq=True, with_drop=True)
    c["item_lo"] = item_lo
    ref = _ref(c, seen=seen, u_ids=u_ids, i_ids=i_ids)
    assert torch.equal(ref["allowed"][0], allowed)
    got = _run(c, seen=seen, u_ids=u_ids, i_ids=i_ids)
    _compare(f"softmax fixture {'fm' if fm else 'dot'}", got, ref)
    # row 0: every negative masked -> its loss term and its gradients are exactly 0 (bound 0 in the restatement: checked above;
    # here by name).  Column 4, the pad id, is masked in every row other than its own: its d_il is row 4's term alone.
    assert int(torch.count_nonzero(got["d_ul"][0])) == 0
    assert float(ref["d_ul"][1][0].max()) == 0.0
    ds4 = (ref["P"][0][4, 4] - 1.0) / 8
    ul4 = c["ul"][4].double()
    if fm:
        w = ((ul4 * c["il"][4].double()) > 0).double() * c["drop"][4, 4].double() * c["h"].double()
        own = ds4 * w * ul4
    else:
        own = ds4 * ul4
    assert torch.allclose(ref["d_il"][0][4], own, rtol=0, atol=1e-15)
    # ... and so is the kernel's, by name: within the bound of that ONE term (a nonzero P in a masked row would add to it)
    assert bool(((got["d_il"][4].cpu().double() - own).abs() <= ref["d_il"][1][4]).all())
    # without the row that sees nothing but itself the mean is over the same B: the loss is the sum of the other rows' terms / B
    assert float(got["loss"]) > 0.0


def test_exact_zeros_same_bits_and_both_backward_routes():
    from review_based_recommender_amd import functional as RF
    c = SR.random_case(65, 33, True, 5, with_rb=True, with_cb=True, with_logq=True, with_drop=True)
    a, b = _run(c, 0.25), _run(c, 0.25)
    assert set(a) == {"loss", "pos", "d_ul", "d_il", "d_h", "d_col_bias", "d_row_bias"}
    for n in a:
        assert torch.equal(a[n], b[n]), n                          # the same bits on a second run
    assert int(torch.count_nonzero(a["d_row_bias"])) == 0 and a["d_row_bias"].shape == (65,)
    # a root of ones(()) is not the cached unit scalar: it takes rbr_pair_softmax_bwd, and gives the unit route's bits
    one = _run(c, 0.25, root=torch.ones((), device=DEV))
    assert torch.ones((), device=DEV).data_ptr() != RF.unit_scalar(DEV).data_ptr()
    for n in a:
        assert torch.equal(a[n], one[n]), n
    # a root of 2.5 against the restatement scaled
    got = _run(c, 0.25, root=torch.full((), 2.5, device=DEV))
    ref = _ref(c, 0.25, d_loss=2.5)
    for n in ("d_ul", "d_il", "d_h", "d_col_bias"):
        check("softmax root 2.5", n, got[n], ref[n][0], ref[n][1])
    assert int(torch.count_nonzero(got["d_row_bias"])) == 0
    assert torch.equal(got["loss"], a["loss"]) and torch.equal(got["pos"], a["pos"])
    # dot mode, same three routes
    c = SR.random_case(65, 5, False, 6, with_rb=False, with_cb=True, with_logq=False, with_drop=False)
    a, one = _run(c), _run(c, root=torch.ones((), device=DEV))
    for n in a:
        assert torch.equal(a[n], one[n]), n


@pytest.mark.parametrize("fm", [True, False], ids=["fm", "dot"])
def test_extreme_scores_stay_finite_and_within_bounds(fm):
    """Scores of +-80 before the temperature: the biases carry them (row r gets +40 or -40 by parity, column c the same), so a
    row holds scores around -80, 0 and +80, z = 4 s at temperature 0.25 spans +-320, and a row softmax without the max
    subtraction would overflow f32 (exp(88.7))."""
    B, K = 65, 5
    c = SR.random_case(B, K, fm, 9, with_rb=True, with_cb=True, with_logq=False, with_drop=False)
    sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    c["row_bias"] = (40.0 * sign).float()
    c["col_bias"] = (40.0 * sign).float()
    for temp in (1.0, 0.25):
        ref = _ref(c, temp)
        assert 70.0 < float(ref["pos"][0].abs().min()) and float(ref["pos"][0].abs().max()) < 90.0
        got = _run(c, temp)
        for n, t in got.items():
            assert bool(torch.isfinite(t).all()), n
        _compare(f"softmax extreme {'fm' if fm else 'dot'} T={temp}", got, ref)


@pytest.mark.parametrize("B,K", [(2, 1), (65, 5), (257, 33)])
def test_in_kernel_dropout_is_the_draw_of_dropout_multiplier(B, K):
    """p_drop drawn in the kernel == the same call with drop = dropout_multiplier((B, B, K), p) of the same seed and call number:
    every output torch.equal, and the call number has advanced by one."""
    from review_based_recommender_amd import functional as RF
    p = 0.5
    c = SR.random_case(B, K, True, 40 + B, with_rb=True, with_cb=True, with_logq=True, with_drop=False)
    torch.manual_seed(1234)
    _, state = RF._drop_rng(torch.device(DEV))
    state.copy_(torch.tensor([7, 0]))
    drop = RF.dropout_multiplier((B, B, K), p, True, DEV)
    torch.cuda.synchronize()
    assert state.tolist() == [8, 0]
    if drop.numel() >= 4096:
        assert 0.4 < float((drop == 0).float().mean()) < 0.6
    assert set(drop.unique().tolist()) <= {0.0, 2.0}
    explicit = _run(dict(c, drop=drop.cpu()))
    state.copy_(torch.tensor([7, 0]))
    drawn = _run(c, p_drop=p)
    assert state.tolist() == [8, 0]                                 # read by both launches, advanced once
    for n in explicit:
        assert torch.equal(explicit[n], drawn[n]), n
    # the non-unit root re-draws the forward's set from the saved call number, although the counter has moved on
    state.copy_(torch.tensor([7, 0]))
    again = _run(c, p_drop=p, root=torch.ones((), device=DEV))
    assert state.tolist() == [8, 0]
    for n in explicit:
        assert torch.equal(explicit[n], again[n]), n


@pytest.mark.parametrize("B,K", [(4097, 4), (4, 257)])
def test_refused_shapes_raise_and_launch_nothing(B, K):
    from review_based_recommender_amd import functional as RF
    ul = torch.zeros(B, K, device=DEV, requires_grad=True)
    ids = torch.arange(B, device=DEV)
    with pytest.raises(RuntimeError, match="no fallback"):
        RF.pair_softmax_loss(ul, ul.detach(), ids, ids, "dot")
    torch.cuda.synchronize()
    assert ul.grad is None
