"""The MSE loss computed by the head's BACKWARD launch (rbr_pair_head_bwd_ex: one more workgroup, d_pred taken from pred and
target) against the ticketed tail of the forward's head launch it replaces (RBR_LOSS_IN_BWD; functional.fused_loss(...,
after_backward=True) is the opt-in).

Shapes: B = 1, 3, 256 and 300 (300: the loss workgroup's threads stride the batch twice), K = 32 and 5, H = 150 and 7; L = 40
(two slabs, the second partial), a non-prefix mask, one fully masked document, the padding id 0.

As in test_head_bwd_in_fwd_gpu.py every token and every user / item id occurs at most TWICE in a batch, so no f32 atomic sum
has more than two addends and the order of arrival cannot change it: every comparison below is for equal bits, the atomically
summed gradients (table through G, id embeddings, id biases) included."""
import os

import pytest
import torch

import synth
from helpers import quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, L = 8, 40
KZ = (3, 5)
NAMES = ("table", "w0", "w1", "b0", "b1", "Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib")


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def _product_conv():
    from review_based_recommender_amd import _lib
    _lib.lib().rbr_set_conv_mode(2)
    yield
    _lib.lib().rbr_set_conv_mode(0)


def _sizes(B):
    return B * L + 1, B // 2 + 2, B // 2 + 2


class _Net(torch.nn.Module):
    """functional.encode_head over two conv widths with ch[0] + ch[1] = H channels."""

    def __init__(self, B, K, H):
        super().__init__()
        V, U, I = _sizes(B)
        self.sizes, self.ch = (V, U, I), (H // 2, H - H // 2)
        g = torch.Generator().manual_seed(3)
        P = torch.nn.Parameter

        def rnd(*shape, s=0.3):
            return P((torch.rand(*shape, generator=g) * 2 - 1) * s)

        self.table = rnd(V, D, s=1.0)
        self.w0, self.w1 = rnd(self.ch[0], D, KZ[0]), rnd(self.ch[1], D, KZ[1])
        self.b0, self.b1 = rnd(self.ch[0]), rnd(self.ch[1])
        self.Wu, self.bu, self.Eu = rnd(H, K), rnd(K), rnd(U, K)
        self.Wi, self.bi, self.Ei = rnd(H, K), rnd(K), rnd(I, K)
        self.h, self.g = rnd(K, 1, s=1.0), rnd(1)
        self.ub, self.ib = rnd(U, 1), rnd(I, 1)

    def forward(self, u_docs, i_docs, u_masks, i_masks, u_ids, i_ids):
        from review_based_recommender_amd import functional as RF
        masks = RF.stack_rows(u_masks, i_masks)
        head = (self.Wu, self.bu, self.Eu, self.Wi, self.bi, self.Ei, self.h, self.g, self.ub, self.ib)
        V, U, I = self.sizes
        sets = [(u_docs, V, 0), (i_docs, V, 0), (u_ids, U, 0), (i_ids, I, 0)]
        assert RF.encode_head_applicable(self.table, 2 * u_docs.shape[0], L, KZ, self.ch, 0)
        return RF.encode_head(self.table, None, masks, None, None, [self.w0, self.w1], [self.b0, self.b1], head, id_sets=sets,
                              drop=None, padding_idx=0, pad_u=0, pad_i=0)


def _batch(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    V, U, I = _sizes(B)
    docs = (torch.randperm(2 * B * L, generator=g) // 2 + 1).view(2 * B, L)
    masks = torch.rand(2 * B, L, generator=g) < 0.8
    masks[B] = False                                         # one fully masked document
    u_ids = (torch.arange(B) // 2 + 1)[torch.randperm(B, generator=g)]
    i_ids = (torch.arange(B) // 2 + 1)[torch.randperm(B, generator=g)]
    assert int(docs.max()) < V and int(u_ids.max()) < U and int(i_ids.max()) < I
    if B > 1:
        u_ids[0], i_ids[B - 1] = 0, 0                        # the padding id: no gradient row
    ratings = torch.randint(1, 6, (B,), generator=g).float()
    args = (docs[:B], docs[B:], masks[:B], masks[B:], u_ids, i_ids)
    return tuple(t.contiguous().to(DEV) for t in args), ratings.to(DEV)


def _bwd_unit(loss, pred):
    from review_based_recommender_amd import functional as RF
    loss.backward(RF.unit_scalar(pred.device))


def _bwd_scaled(loss, pred):
    (2 * loss).backward()


def _bwd_explicit_d_pred(loss, pred):
    from review_based_recommender_amd import functional as RF
    torch.autograd.backward([loss, pred], [RF.unit_scalar(pred.device), torch.full_like(pred, 0.25)])


def _run(B, K, H, after_backward, backward=_bwd_unit, switch="1"):
    """Forward inside fused_loss + backward on a fresh net: (pred, loss, d_unit, d_feat_unit, grads, deferred?, early?, ex calls)."""
    from review_based_recommender_amd import _lib, functional as RF
    net = _Net(B, K, H).to(DEV).train()
    args, ratings = _batch(B)
    early, real = [], RF._textcnn_backward

    def watched(S, d_feat, need_table, need_gate, side_job=None):
        early.append(side_job is not None)
        return real(S, d_feat, need_table, need_gate, side_job=side_job)

    L_ = _lib.lib()
    calls = {"ex": 0, "old": 0}
    real_call = RF._call

    def counting(key, fn, *a):
        if fn is L_.rbr_pair_head_bwd_ex:
            calls["ex"] += 1
        elif fn is L_.rbr_pair_head_bwd:
            calls["old"] += 1
        return real_call(key, fn, *a)

    RF._textcnn_backward, RF._call = watched, counting
    try:
        with _env(RBR_LOSS_IN_BWD=switch), RF.fused_loss(ratings, after_backward=after_backward) as req:
            pred = net(*args)
            loss = req.loss_for(pred)
            assert loss is not None
        node = pred.grad_fn
        deferred = node.deferred is not None
        d_feat_unit, d_unit = node.d_feat_unit, node.head[7]
        backward(loss, pred)
    finally:
        RF._textcnn_backward, RF._call = real, real_call
    torch.cuda.synchronize()
    grads = {n: getattr(net, n).grad.clone() for n in NAMES}
    return dict(pred=pred.detach().clone(), loss=loss.detach().clone(), d_unit=d_unit.clone(), d_feat=d_feat_unit.clone(),
                grads=grads, deferred=deferred, early=early, calls=calls)


def _same(a, b):
    for k in ("pred", "loss", "d_unit", "d_feat"):
        assert torch.equal(a[k], b[k]), k
    for n in NAMES:
        assert torch.equal(a["grads"][n], b["grads"][n]), n
    assert all(float(g.abs().max()) > 0 for g in a["grads"].values())
    assert torch.isfinite(a["loss"]) and float(a["loss"]) > 0


@pytest.mark.parametrize("H", [150, 7])
@pytest.mark.parametrize("K", [32, 5])
@pytest.mark.parametrize("B", [1, 3, 256, 300])
def test_loss_from_the_backward_launch_has_the_ticketed_bits(B, K, H):
    new = _run(B, K, H, after_backward=True)
    old = _run(B, K, H, after_backward=False)
    assert new["deferred"] and not old["deferred"]
    assert new["early"] == [True] and old["early"] == [True]
    assert new["calls"] == {"ex": 1, "old": 0} and old["calls"] == {"ex": 0, "old": 1}
    _same(new, old)
    # ... and they are nn.MSELoss's value and gradient
    args, ratings = _batch(B)
    ref = torch.nn.functional.mse_loss(new["pred"].double(), ratings.double())
    # f32: at most 16 roundings on the way of any term (difference, square, <= 2 adds in the thread, 6 + 3 in the reduction, the
    # division), all terms positive
    assert abs(float(new["loss"]) - float(ref)) <= 16 * 2.0 ** -24 * float(ref)
    two_over_b = torch.tensor(2.0, device=DEV) / torch.tensor(float(B), device=DEV)
    assert torch.equal(new["d_unit"], (new["pred"] - ratings) * two_over_b)


def test_switch_off_keeps_the_ticketed_tail():
    off = _run(3, 5, 7, after_backward=True, switch="0")
    assert not off["deferred"] and off["calls"] == {"ex": 0, "old": 1}
    _same(off, _run(3, 5, 7, after_backward=False))


@pytest.mark.parametrize("case", ["scaled_loss", "explicit_d_pred"])
def test_other_upstream_gradients_take_the_old_launch(case):
    """The forward left the loss out (after_backward), the backward is handed something else than the unit root gradient: the
    loss and d loss / d pred come from rbr_mse_loss_fwd, then the old order runs -- the results of the ticketed path."""
    B, K, H = 300, 5, 7
    bwd = {"scaled_loss": _bwd_scaled, "explicit_d_pred": _bwd_explicit_d_pred}[case]
    new = _run(B, K, H, after_backward=True, backward=bwd)
    old = _run(B, K, H, after_backward=False, backward=bwd)
    assert new["deferred"] and new["early"] == [False] and old["early"] == [False]
    assert new["calls"] == {"ex": 0, "old": 1} and old["calls"] == {"ex": 0, "old": 1}
    _same(new, old)


TINY = dict(B=4, L=40, D=8, kz=[3, 5], H=6, K=4, V=300, U=5, I=5)


def _tiny_batch(seed):
    g = torch.Generator().manual_seed(seed)
    B, Lt = TINY["B"], TINY["L"]
    docs = (torch.randperm(2 * B * Lt, generator=g) // 2 + 1).view(2 * B, Lt)      # every token twice, all below V = 300
    masks = torch.rand(2 * B, Lt, generator=g) < 0.8
    u_ids, i_ids = torch.tensor([1, 2, 2, 1])[torch.randperm(B, generator=g)], torch.tensor([3, 4, 4, 3])[torch.randperm(B, generator=g)]
    ratings = torch.randint(1, 6, (B,), generator=g).float()
    args = (docs[:B], docs[B:], masks[:B], masks[B:], u_ids, i_ids)
    return tuple(t.contiguous().to(DEV) for t in args), ratings.to(DEV)


def _recorded_steps(switch):
    from review_based_recommender_amd.models.deepconn.deepconn import DeepCoNNpp
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer
    c = TINY
    with _env(RBR_LOSS_IN_BWD=switch, RBR_PREP_TWO_LAUNCH=switch):
        m = quiet(DeepCoNNpp, c["U"], c["I"], c["V"], c["kz"], c["D"], c["H"], c["K"], c["L"], None, 0.0)
        m.load_state_dict(synth.deepconn_params(c, 0))
        m = m.to(DEV).train()
        opt = make_optimizer(m, hip_clip_adam=True)
        cap_args, cap_r = _tiny_batch(9)
        stepper = GraphedTrainStep(m, opt, cap_args, cap_r, keep_graph=True)
        out = []
        for seed in (1, 2):
            args, r = _tiny_batch(seed)
            loss, gnorm, pred = stepper(args, r)
            torch.cuda.synchronize()
            out.append((loss.clone(), gnorm.clone(), pred.clone(), [p.detach().clone() for p in m.parameters()]))
        return stepper.kernel_launches(), out


def test_recorded_deepconn_step_equals_the_step_with_both_switches_off():
    """B = 4, L = 40, V = 300 through DeepCoNNpp and GraphedTrainStep, two replays on two batches: loss, gradient norm, predictions
    and the updated parameters.  No atomic sum of these batches has more than two addends (tokens and ids occur twice), so they
    are order-free and everything is compared for equal bits -- tighter than the rtol 1e-5 / atol 1e-7 |max| that
    test_fused_step_gpu.py::test_fused_encoder_head_equals_the_separate_functions allows the same atomically summed gradients."""
    n_on, on = _recorded_steps("1")
    n_off, off = _recorded_steps("0")
    if n_on is not None and n_off is not None:
        assert n_on == n_off - 1, (n_on, n_off)          # the prepare stage lost a launch; the loss moved, it cost none
    for (la, ga, pa, qa), (lb, gb, pb, qb) in zip(on, off):
        assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(pa, pb)
        for x, y in zip(qa, qb):
            assert torch.equal(x, y)
        assert torch.isfinite(la) and float(ga) > 0
