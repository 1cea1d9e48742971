"""csrc/ahn_attend.hip at edge shapes against float64: functional.ahn_pair_attend, forward and backward, on seeded inputs against
tests/ahn_attend_ref.py, at the smallest shapes that cross each constant -- test_ahn_pair_edges_gpu.py's shape list (the 32-column
slice of F: 12, 34, 300; the 32-row MFMA tiles: 1 row, 12 against 10, 33, 100) times (B, G) = (1, 1), (5, 1), (3, 3), and (2, 2) at
F = 300, so that P = 1, 5, 9 crosses the 4-pair forward tile and a user's gradients are sums over 1, 2 and 3 pairs.  Special rows
(ahn_attend_ref.make_inputs): a user with one fully masked review, a user with no live review, a zero padding user, an all-zero
item (every product exactly 0: js and jr must be all 0 there, the tie rule).

Tolerances are the project's LSTM edge rule: z within 2e-6 + 2e-4 |ref| per element, w and v within 1e-5, every gradient within
2e-6 + 2e-4 max|ref| per tensor.  The reference is differentiated with the KERNEL's routing (js, jr), after each chosen row has
been shown to attain the reference's max within 1e-5 (1 + |best|).  The generators assert the routing margins on the CPU.

Each case prints its measured maxima beside torch's own f32 composition of the same arithmetic on the same inputs.  Largest
errors measured on an MI355X over all 13 cases, the op / torch's composition: z 5.1e-8 / 5.9e-8, w 2.4e-7 / 2.4e-7, v 5.9e-8 / 3.5e-8,
dX 2.6e-8 / 2.3e-8 (of at most 0.18), dXt 3.0e-7 / 3.0e-7 (of 4.3), dKs 6.6e-8 / 6.3e-8 (of 0.29), dKr 5.9e-8 / 8.1e-8 (of 0.15), dbt 6.8e-7 /
6.3e-7 (of 5.8): three orders of magnitude inside the tolerances, and the same size as torch's own f32 error."""
import numpy as np
import pytest
import torch

import ahn_attend_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("X", "Xt", "Ks", "Kr", "bt")

SHAPES = {"f12_1x1": (12, (1, 1), (1, 1)), "f12_3x4_2x5": (12, (3, 4), (2, 5)), "f34_33rows": (34, (3, 11), (11, 3)),
          "f34_10x10": (34, (10, 10), (10, 10)), "f300_10x10": (300, (10, 10), (10, 10))}
# (shape, B, G) -> a seed whose float64 routing leads by 1e-4 (1 + |best|) and keeps |a| >= 1e-5 (make_inputs asserts it)
CASES = {(s, B, G): 100 for s in ("f12_1x1", "f12_3x4_2x5", "f34_33rows", "f34_10x10") for B, G in ((1, 1), (5, 1), (3, 3))}
CASES[("f34_10x10", 3, 3)] = 101
CASES[("f300_10x10", 2, 2)] = 108
IDS = [f"{s}-B{B}G{G}" for s, B, G in CASES]
_BUILT = {}


def _run(t, G, dz):
    """One forward + backward of the op on device copies of the inputs: (z, w, v, js, jr, grads by name)."""
    from review_based_recommender_amd import functional as RF
    leaf = {k: t[k].to(DEV).requires_grad_(True) for k in GRADS}
    z, w, v, js, jr = RF.ahn_pair_attend(leaf["X"], leaf["Xt"], t["sent_mask"].to(DEV), t["rev_mask"].to(DEV), leaf["Ks"], leaf["Kr"],
                                         leaf["bt"], groups=G, saved=True)
    z.backward(dz.to(DEV))
    return z.detach(), w, v, js, jr, {k: leaf[k].grad for k in GRADS}


def _case(key):
    """Inputs, the float64 forward with its own routing, one run of the op, and the float64 forward + backward under the
    kernel's routing: built once per case, left unchanged."""
    if key in _BUILT:
        return _BUILT[key]
    s, B, G = key
    F, u, i = SHAPES[s]
    t, fwd = A.make_inputs(B, G, *u, *i, F, CASES[key])
    dz = torch.randn(G * B, F, generator=torch.Generator().manual_seed(7 + CASES[key]))
    got = _run(t, G, dz)
    m, M = t["sent_mask"].numpy(), t["rev_mask"].numpy()
    routed = A.attend_fwd_ref(t["X"], t["Xt"], m, M, t["Ks"], t["Kr"], t["bt"], G, js=got[3].cpu().numpy(), jr=got[4].cpu().numpy())
    grads = A.attend_bwd_ref(t["X"], t["Xt"], m, M, t["Ks"], t["Kr"], routed, dz, G)
    _BUILT[key] = (t, fwd, dz, got, routed, {k: grads["d" + k] for k in GRADS})
    return _BUILT[key]


def _torch_f32(t, G, dz):
    leaf = {k: t[k].to(DEV).requires_grad_(True) for k in GRADS}
    z, w, v = A.attend_torch(leaf["X"], leaf["Xt"], t["sent_mask"].to(DEV), t["rev_mask"].to(DEV), leaf["Ks"], leaf["Kr"], leaf["bt"], G)
    z.backward(dz.to(DEV))
    return z.detach(), w.detach(), v.detach(), {k: leaf[k].grad for k in GRADS}


def _err(a, ref):
    return float(np.abs(a.double().cpu().numpy() - ref).max())


@pytest.mark.parametrize("key", list(CASES), ids=IDS)
def test_forward_and_backward_against_float64(key):
    t, fwd, dz, (z, w, v, js, jr, g), routed, ref_g = _case(key)
    s, B, G = key
    P = B * G
    assert z.shape == (P, SHAPES[s][0]) and w.shape == (P, *SHAPES[s][1]) and v.shape == (P, SHAPES[s][1][0])
    assert js.dtype == torch.int32 and jr.dtype == torch.int32
    # the kernel's routing attains the reference's maxima (with the margins of the generator it IS the reference's)
    assert A.attains_max(routed["S"], js.cpu().numpy()) and A.attains_max(routed["T"], jr.cpu().numpy())
    tz, tw, tv, tg = _torch_f32(t, G, dz)
    line = [f"z {_err(z, routed['z']):.2e} (torch {_err(tz, routed['z']):.2e})", f"w {_err(w, routed['w']):.2e} (torch {_err(tw, routed['w']):.2e})",
            f"v {_err(v, routed['v']):.2e} (torch {_err(tv, routed['v']):.2e})"]
    line += [f"d{k} {_err(g[k], ref_g[k]):.2e} / {float(np.abs(ref_g[k]).max()):.2e} (torch {_err(tg[k], ref_g[k]):.2e})" for k in GRADS]
    print(f"{IDS[list(CASES).index(key)]}: max err " + ", ".join(line))
    assert (np.abs(z.double().cpu().numpy() - routed["z"]) <= 2e-6 + 2e-4 * np.abs(routed["z"])).all()
    assert _err(w, routed["w"]) <= 1e-5 and _err(v, routed["v"]) <= 1e-5
    for k in GRADS:
        assert g[k].shape == t[k].shape
        assert _err(g[k], ref_g[k]) <= 2e-6 + 2e-4 * float(np.abs(ref_g[k]).max()), k
    if P >= 2:                                     # the all-zero item: every product is exactly 0 and the lowest index wins
        assert not js[-1].any() and not jr[-1].any()
    # dKs rows that nobody selected are exactly 0
    chosen = torch.zeros(P, t["Ks"].shape[1], dtype=torch.bool, device=DEV).scatter_(1, js.long(), True)
    assert not g["Ks"][~chosen].any()
    hit = torch.zeros(P, t["Kr"].shape[1], dtype=torch.bool, device=DEV).scatter_(1, jr.long(), True)
    assert not g["Kr"][~hit].any()


@pytest.mark.parametrize("key", list(CASES), ids=IDS)
def test_weights_have_the_pair_score_kernel_s_bits_and_two_runs_agree(key):
    from review_based_recommender_amd import functional as RF
    t, _, dz, (z, w, v, js, jr, g), _, _ = _case(key)
    s, B, G = key
    P, F = B * G, SHAPES[s][0]
    (Ri, Si) = SHAPES[s][2]
    zeros = lambda *sh: torch.zeros(*sh, device=DEV)                                    # noqa: E731
    us = RF.AhnUserState(t["X"].to(DEV), t["Xt"].to(DEV), t["sent_mask"].to(DEV), t["rev_mask"].to(DEV), zeros(B, 3))
    its = RF.AhnItemState(t["Ks"].to(DEV), t["Kr"].to(DEV), zeros(P, 3), zeros(P, Ri, Si), zeros(P, Ri))
    head = RF.AhnPairHead(t["bt"].to(DEV), zeros(1, F), zeros(F), zeros(F), zeros(1))
    rows = torch.arange(P, device=DEV)
    _, pw, pv = RF.ahn_pair_score(us, its, head, rows % B, rows, weights=True)
    assert torch.equal(w, pw) and torch.equal(v, pv)
    z2, w2, v2, js2, jr2, g2 = _run(t, G, dz)
    assert torch.equal(z, z2) and torch.equal(w, w2) and torch.equal(v, v2) and torch.equal(js, js2) and torch.equal(jr, jr2)
    assert all(torch.equal(g[k], g2[k]) for k in GRADS)


@pytest.mark.parametrize("key", [k for k in CASES if k[2] == 3], ids=[i for i, k in zip(IDS, CASES) if k[2] == 3])
def test_a_pair_s_item_gradients_do_not_depend_on_its_place(key):
    """Group g of the G = 3 call against the G = 1 call on that slab: dKs and dKr bit for bit, z too; and the user-side
    gradients of the G = 3 call are the sum of the three, g ascending."""
    t, _, dz, (z, w, v, js, jr, g), _, _ = _case(key)
    s, B, G = key
    dX = dXt = dbt = None
    for k in range(G):
        sl = slice(k * B, (k + 1) * B)
        one = dict(t, Ks=t["Ks"][sl], Kr=t["Kr"][sl])
        z1, _, _, js1, jr1, g1 = _run(one, 1, dz[sl])
        assert torch.equal(z1, z[sl]) and torch.equal(js1, js[sl]) and torch.equal(jr1, jr[sl])
        assert torch.equal(g1["Ks"], g["Ks"][sl]) and torch.equal(g1["Kr"], g["Kr"][sl])
        dX, dXt = (g1["X"], g1["Xt"]) if k == 0 else (dX + g1["X"], dXt + g1["Xt"])
    assert torch.equal(dX, g["X"]) and torch.equal(dXt, g["Xt"])


def test_zero_pairs_launch_nothing():
    from review_based_recommender_amd import functional as RF
    F = 12
    e = lambda *sh: torch.zeros(*sh, device=DEV, requires_grad=True)                    # noqa: E731
    X, Xt, Ks, Kr, bt = e(0, 12, F), e(0, 12, F), e(0, 10, F), e(0, 2, F), e(F)
    z, w, v = RF.ahn_pair_attend(X, Xt, torch.zeros(0, 3, 4, dtype=torch.bool, device=DEV), torch.zeros(0, 3, dtype=torch.bool, device=DEV),
                                 Ks, Kr, bt, groups=2)
    assert z.shape == (0, F) and w.shape == (0, 3, 4) and v.shape == (0, 3)
    assert not w.requires_grad and not v.requires_grad
    z.sum().backward()
    assert bt.grad.shape == (F,) and not bt.grad.any()
