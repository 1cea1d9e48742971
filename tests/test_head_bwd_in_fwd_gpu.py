"""The pair part of the head's backward inside the forward's head launch (rbr_pair_head_fwd_pool_ex: d_feat_unit) against
the backward launch it replaces, and the step built on it -- the conv backward starting from the forward's d_feat, what is
left of rbr_pair_head_bwd on the weight-gradient branch -- against the old order (RBR_HEAD_BWD_IN_FWD=0).

Shapes: widths (3, 5) with (5, 6) channels (H = 11, no multiple of 4), L = 40 (two slabs, the second partial), a non-prefix
mask and one fully masked document, ids that repeat (atomics collide) and the padding id 0.

Every token and every user / item id occurs at most TWICE in a batch, so no f32 atomic sum has more than two addends and the
order in which they arrive cannot change it: the comparisons of the atomically summed gradients (rtol 1e-6, atol 1e-9) then
test the change and not the atomics.  Measured with free collisions (V = 60 tokens, 9 / 7 ids, B = 66), largest
|a - b| / (1e-9 + 1e-6 |b|) per tensor: table 1.5-4.1 new order against old and 1.2-6.8 OLD AGAINST OLD (two runs of the
unchanged path miss the bound by themselves), id embeddings up to 0.92 / 0.76, id biases up to 0.23 / 0.23; B = 3: 0 throughout."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, L = 8, 40
KZ, CH = (3, 5), (5, 6)
H = sum(CH)
ATOMIC = ("Eu", "Ei", "ub", "ib", "table")          # summed with f32 atomics (the table through its G)


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RBR_HEAD_BWD_IN_FWD")
        os.environ["RBR_HEAD_BWD_IN_FWD"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("RBR_HEAD_BWD_IN_FWD", None)
        else:
            os.environ["RBR_HEAD_BWD_IN_FWD"] = self.old


@pytest.fixture(autouse=True)
def _product_conv():
    from review_based_recommender_amd import _lib
    _lib.lib().rbr_set_conv_mode(2)
    yield
    _lib.lib().rbr_set_conv_mode(0)


class _Net(torch.nn.Module):
    """DeepCoNN++'s fused encoder + head (functional.encode_head) over conv widths with UNEQUAL channel counts."""

    def __init__(self, B, K, p_drop, use_first=False):
        super().__init__()
        V, U, I = _sizes(B)
        self.sizes = (V, U, I)
        g = torch.Generator().manual_seed(3)
        P = torch.nn.Parameter

        def rnd(*shape, s=0.3):
            return P((torch.rand(*shape, generator=g) * 2 - 1) * s)

        self.table = rnd(V, D, s=1.0)
        self.w0, self.w1 = rnd(CH[0], D, KZ[0]), rnd(CH[1], D, KZ[1])
        self.b0, self.b1 = rnd(CH[0]), rnd(CH[1])
        self.Wu, self.bu, self.Eu = rnd(H, K), rnd(K), rnd(U, K)
        self.Wi, self.bi, self.Ei = rnd(H, K), rnd(K), rnd(I, K)
        self.h, self.g = rnd(K, 1, s=1.0), rnd(1)
        self.ub, self.ib = rnd(U, 1), rnd(I, 1)
        self.p_drop, self.use_first = p_drop, use_first

    NAMES = ("table", "w0", "w1", "b0", "b1", "Wu", "bu", "Eu", "Wi", "bi", "Ei", "h", "g", "ub", "ib")

    def forward(self, u_docs, i_docs, u_masks, i_masks, u_ids, i_ids):
        from review_based_recommender_amd import functional as RF
        masks = RF.stack_rows(u_masks, i_masks)          # (a view over the recorded step's input block: no launch)
        first = torch.arange(2 * u_docs.shape[0], device=u_docs.device) if self.use_first else None      # every document its own first
        head = (self.Wu, self.bu, self.Eu, self.Wi, self.bi, self.Ei, self.h, self.g, self.ub, self.ib)
        V, U, I = self.sizes
        sets = [(u_docs, V, 0), (i_docs, V, 0), (u_ids, U, 0), (i_ids, I, 0)]
        drop = float(self.p_drop) if self.training else None
        assert RF.encode_head_applicable(self.table, 2 * u_docs.shape[0], L, KZ, CH, 0)
        return RF.encode_head(self.table, None, masks, None, None, [self.w0, self.w1], [self.b0, self.b1], head, id_sets=sets,
                              drop=drop, padding_idx=0, pad_u=0, pad_i=0, first=first)


def _sizes(B):
    """(V, U, I): every token id in [1, V) twice in the 2 B L tokens of a batch, every id in [1, U) twice among the B pairs."""
    return B * L + 1, B // 2 + 2, B // 2 + 2


def _batch(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    V, U, I = _sizes(B)
    docs = (torch.randperm(2 * B * L, generator=g) // 2 + 1).view(2 * B, L)
    assert int(docs.max()) < V
    masks = torch.rand(2 * B, L, generator=g) < 0.8          # holes anywhere: no prefix mask
    masks[B + 1] = False                                    # one fully masked document
    u_ids = (torch.arange(B) // 2 + 1)[torch.randperm(B, generator=g)]
    i_ids = (torch.arange(B) // 2 + 1)[torch.randperm(B, generator=g)]
    assert int(u_ids.max()) < U and int(i_ids.max()) < I
    u_ids[0], i_ids[B - 1] = 0, 0                            # the padding id: no gradient row
    ratings = torch.randint(1, 6, (B,), generator=g).float()
    args = (docs[:B], docs[B:], masks[:B], masks[B:], u_ids, i_ids)
    return tuple(t.contiguous().to(DEV) for t in args), ratings.to(DEV)


def _reset_dropout():
    from review_based_recommender_amd import functional as RF
    torch.manual_seed(5)
    for st in RF._DROP_STATE.values():
        st.zero_()


def _net(B, K, p_drop, **kw):
    return _Net(B, K, p_drop, **kw).to(DEV).train()


SHAPES = [(B, K, p) for B in (3, 66) for K in (5, 33) for p in (0.0, 0.5)]


@pytest.mark.parametrize("B,K,p_drop", SHAPES)
def test_forward_d_feat_equals_the_backward_launch(B, K, p_drop):
    from review_based_recommender_amd import _lib, functional as RF
    from review_based_recommender_amd._lib import dev_ptr
    F32, I64 = torch.float32, torch.int64
    net = _net(B, K, p_drop)
    args, ratings = _batch(B)
    _reset_dropout()
    with _env("1"), RF.fused_loss(ratings) as req:
        pred = net(*args)
        assert req.loss_for(pred) is not None
    node = pred.grad_fn
    d_feat_unit = node.d_feat_unit
    assert d_feat_unit is not None and d_feat_unit.shape == (2 * B, H)
    u_id, i_id, ul, il, head, drop_t, _flat, d_unit = node.head
    assert (drop_t is not None) == (p_drop > 0)
    two_over_b = torch.tensor(2.0, dtype=F32, device=DEV) / torch.tensor(float(B), dtype=F32, device=DEV)
    d_pred = ((pred.detach() - ratings) * two_over_b).contiguous()
    assert torch.equal(d_pred, d_unit)
    feat = node.conv.feat
    hp = _lib.HeadParams(*[dev_ptr(t, F32, n) for t, n in zip(head, RF._HEAD_NAMES)])
    grads = [torch.zeros_like(t) for t in head]
    hg = _lib.HeadGrads(*[dev_ptr(t, F32, "d" + n) for t, n in zip(grads, RF._HEAD_NAMES)])
    d_pair = torch.full((2 * B, H), float("nan"), dtype=F32, device=DEV)
    RF._call(None, _lib.lib().rbr_pair_head_bwd, B, H, K, dev_ptr(feat[:B], F32, "u_feat"), dev_ptr(feat[B:], F32, "i_feat"),
             dev_ptr(u_id, I64, "u_id"), dev_ptr(i_id, I64, "i_id"), C.byref(hp), dev_ptr(drop_t, F32, "drop"),
             dev_ptr(ul, F32, "ul"), dev_ptr(il, F32, "il"), dev_ptr(d_pred, F32, "d_pred"), 0, 0, C.byref(hg),
             dev_ptr(d_pair[:B], F32, "d_ufeat"), dev_ptr(d_pair[B:], F32, "d_ifeat"), None, _lib.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(d_feat_unit, d_pair)
    assert float(d_pair.abs().max()) > 0


def _one_step(switch, B, K, p_drop, backward=None, use_first=False, spy=None):
    """One train_step (or forward + the given backward) from a fresh model: (pred, loss, {name: grad})."""
    from review_based_recommender_amd import functional as RF
    from review_based_recommender_amd.train_step import make_optimizer, train_step
    net = _net(B, K, p_drop, use_first=use_first)
    args, ratings = _batch(B)
    _reset_dropout()
    taken = []
    real = RF._textcnn_backward

    def watched(S, d_feat, need_table, need_gate, side_job=None):
        taken.append(side_job is not None)
        return real(S, d_feat, need_table, need_gate, side_job=side_job)

    RF._textcnn_backward = watched
    try:
        with _env(switch):
            if backward is None:
                opt = make_optimizer(net, hip_clip_adam=True)
                loss, _, pred = train_step(net, opt, args, ratings, max_grad_norm=1e9)      # coefficient 1: .grad stays as computed
            else:
                with RF.fused_loss(ratings) as req:
                    pred = net(*args)
                    loss = req.loss_for(pred)
                backward(loss, pred)
    finally:
        RF._textcnn_backward = real
    torch.cuda.synchronize()
    if spy is not None:
        spy.extend(taken)
    return pred.detach().clone(), loss.detach().clone(), {n: getattr(net, n).grad.clone() for n in _Net.NAMES}


def _compare(a, b):
    pa, la, ga = a
    pb, lb, gb = b
    assert torch.equal(pa, pb) and torch.equal(la, lb)
    for n in _Net.NAMES:
        if n in ATOMIC:
            assert torch.allclose(ga[n], gb[n], rtol=1e-6, atol=1e-9), n
        else:
            assert torch.equal(ga[n], gb[n]), n
    assert all(float(g.abs().max()) > 0 for g in ga.values())


@pytest.mark.parametrize("B,K,p_drop", SHAPES)
def test_step_with_the_switch_on_equals_the_old_order(B, K, p_drop):
    on_taken, off_taken = [], []
    on = _one_step("1", B, K, p_drop, spy=on_taken)
    off = _one_step("0", B, K, p_drop, spy=off_taken)
    assert on_taken == [True] and off_taken == [False]
    _compare(on, off)


def _bwd_scaled(loss, pred):
    (2 * loss).backward()


def _bwd_explicit_d_pred(loss, pred):
    from review_based_recommender_amd import functional as RF
    torch.autograd.backward([loss, pred], [RF.unit_scalar(pred.device), torch.full_like(pred, 0.25)])


def _bwd_unit(loss, pred):
    from review_based_recommender_amd import functional as RF
    loss.backward(RF.unit_scalar(pred.device))


@pytest.mark.parametrize("case", ["scaled_loss", "explicit_d_pred", "first"])
def test_other_upstream_gradients_take_the_old_path(case):
    B, K, p_drop = 66, 33, 0.5
    bwd = {"scaled_loss": _bwd_scaled, "explicit_d_pred": _bwd_explicit_d_pred, "first": _bwd_unit}[case]
    on_taken, off_taken = [], []
    on = _one_step("1", B, K, p_drop, backward=bwd, use_first=case == "first", spy=on_taken)
    off = _one_step("0", B, K, p_drop, backward=bwd, use_first=case == "first", spy=off_taken)
    assert on_taken == [False] and off_taken == [False]
    _compare(on, off)


def test_graphed_step_keeps_14_launches_and_matches_eager():
    from review_based_recommender_amd.train_step import GraphedTrainStep, make_optimizer, train_step
    B, K = 4, 5
    with _env("1"):
        m_e, m_g = _net(B, K, 0.0), _net(B, K, 0.0)
        o_e, o_g = make_optimizer(m_e, hip_clip_adam=True), make_optimizer(m_g, hip_clip_adam=True)
        cap_args, cap_r = _batch(B, seed=9)
        stepper = GraphedTrainStep(m_g, o_g, cap_args, cap_r, max_grad_norm=1e9, keep_graph=True)
        assert stepper.kernel_launches() == 14
        for k, seed in enumerate((1, 2)):
            args, r = _batch(B, seed=seed)
            le, _, pe = train_step(m_e, o_e, args, r, max_grad_norm=1e9)
            lg, _, pg = stepper(args, r)
            torch.cuda.synchronize()
            # every atomic sum of these batches has at most two addends, so the steps leave the same parameters in both models
            # and the second replay is held to check 2's tolerances like the first
            eager = (pe, le, {n: getattr(m_e, n).grad for n in _Net.NAMES})
            graph = (pg, lg, {n: getattr(m_g, n).grad for n in _Net.NAMES})
            _compare(graph, eager)
