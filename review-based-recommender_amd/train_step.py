"""The trainer's optimisation step (trainer/train_deepconn_pp.py:161-168, train_narre.py:163-169,
train_dual_att.py:157-163), reproduced above the module boundary so bench.py and the parity
tests drive the HIP modules exactly as the reference trainers drive theirs:

    optimizer.zero_grad(); y = model(*batch); loss = MSELoss()(y, ratings); loss.backward()
    [data-parallel: all-reduce the gradients]
    clip_grad_norm_(model.parameters(), max_grad_norm); optimizer.step()

Nothing here calls .item(): the step stays asynchronous on the HIP stream (the reference's two
loss.item() calls per step, :171-172, are logging, not part of the math).
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as RF

LR = 2e-3            # default_deepconn_pp.json:24
MAX_GRAD_NORM = 5.0  # default_deepconn_pp.json:27


def make_optimizer(model: nn.Module, lr: float = LR, fused: bool | None = None,
                   capturable: bool = False, hip_clip_adam: bool = False) -> torch.optim.Optimizer:
    """torch.optim.Adam(model.parameters(), lr=args.lr)  (train_deepconn_pp.py:135).

    `fused=None` picks torch's single-kernel ("fused") Adam implementation when every parameter lives on
    a HIP device and the default multi-kernel one otherwise; both compute the same update.
    `capturable=True` keeps the step counter on the device so the update can be recorded into a hipGraph
    (GraphedTrainStep).  `hip_clip_adam=True` returns HipClipAdam instead: same update, with the trainer's
    clip_grad_norm_ folded into the optimizer pass (train_step() then calls its clip_and_step)."""
    params = list(model.parameters())
    if hip_clip_adam:      # clip + Adam as two HIP launches (HipClipAdam below); always graph-capturable
        return HipClipAdam(params, lr=lr)
    if fused is None:
        fused = len(params) > 0 and all(p.is_cuda for p in params)
    if fused:
        return torch.optim.Adam(params, lr=lr, fused=True, capturable=capturable)
    return torch.optim.Adam(params, lr=lr, capturable=capturable)


class HipClipAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr)  +  the clip_grad_norm_ in front of its step  (train_deepconn_pp.py:135,166-167)
    as two HIP launches over all parameter tensors (csrc/clip_adam.hip): torch's sequence is ~10 kernels and three
    full passes over the gradients, dominated by the 60 MB word table.

    Same update rule and state names as torch.optim.Adam (amsgrad / weight_decay / maximize unsupported, as the
    reference trainers never set them); `state_dict()` interchanges with it.  The step counter lives on the device,
    so `clip_and_step` can be recorded into a hipGraph.  Parameters must be contiguous fp32 HIP tensors.

    Step counts are per parameter, as torch.optim.Adam's: a parameter counts the steps on which it had a gradient.  The
    tensors of one launch pair share ONE device counter, so only tensors that have stepped together since their state was
    created (or that a checkpoint loaded with equal counts) go into one pair.  When every parameter has a gradient on every
    step -- the trainers' case -- that is one pair and one counter, as recorded by GraphedTrainStep.  A parameter whose first
    gradient arrives later starts a counter of its own at 0 (its first update uses t = 1 whatever the others' count is), and
    a parameter that sits a step out keeps its count while the others take a copy of the counter and move on; either way
    the step then takes one launch pair per distinct count, and with more than one pair the norm and the clipping are
    torch's clip_grad_norm_ (device-side) in front of unclipped pairs.  load_state_dict reads the loaded counts once (a
    host synchronisation) to put equal counts of a parameter group on one counter."""

    MAX_TENSORS = 64      # RBR_OPT_MAX_TENSORS

    ROW_GRAD_MIN_ROWS = 4096      # tables at least this tall take their gradient in compact row form

    def __init__(self, params, lr: float = LR, betas=(0.9, 0.999), eps: float = 1e-8, row_grads: bool = True):
        """row_grads: embedding tables among the parameters (2-D, >= ROW_GRAD_MIN_ROWS rows, row length % 4 == 0) receive the
        gradient of a token-product conv as the rows of the batch's tokens (functional.RowGradient) instead of a dense
        [V, D] tensor whose other rows are zeros -- but only for a backward that runs inside this optimizer's row_grad_scope()
        (train_step() and GraphedTrainStep open it around the forward + backward of a step THIS optimizer will finish): `.grad`
        of such a table then stays None after backward -- call materialize_grads() to see the dense gradient -- and the clip +
        Adam launches neither read nor re-write the zero rows.  Same parameters and state as with the dense gradient, bit for
        bit.  Outside the scope (a hand-written loop, another optimizer on the same model, an external clip_grad_norm_) every
        backward leaves the ordinary dense .grad."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._ws = None
        self._gnorm = None
        self._row_grads = {}          # parameter -> functional.RowGradient of the last backward
        self._row_tables = []
        self._row_scope = 0           # > 0: inside row_grad_scope() -- the only time wants_row_grad() says yes
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            row_grads = False         # a data-parallel exchange reads every gradient as a dense .grad
        if os.environ.get("RBR_ROW_GRADS", "1") == "0":
            row_grads = False
        if row_grads:
            for g in self.param_groups:
                for p in g["params"]:
                    if p.is_cuda and p.dim() == 2 and p.shape[0] >= self.ROW_GRAD_MIN_ROWS and p.shape[1] % 4 == 0 \
                            and p.dtype == torch.float32 and p.numel() < (1 << 32):
                        RF.set_row_grad_sink(p, self)
                        self._row_tables.append(p)

    # ---- functional.set_row_grad_sink protocol
    def wants_row_grad(self, table) -> bool:
        return self._row_scope > 0 and any(table.data_ptr() == p.data_ptr() for p in self._row_tables)

    @contextlib.contextmanager
    def row_grad_scope(self):
        """with opt.row_grad_scope(): forward; loss.backward() -- the caller's promise that THIS optimizer's clip_and_step() /
        step() is what consumes the gradients of that backward: its tables then receive their gradient in compact row form.
        (The registry in functional holds the optimizer weakly and asks wants_row_grad() per backward, so an optimizer that
        merely exists -- beside torch's Adam on the same model, or after its last step -- changes nothing.)"""
        self._row_scope += 1
        try:
            yield self
        finally:
            self._row_scope -= 1

    def put_row_grad(self, table, rg) -> None:
        p = next(q for q in self._row_tables if q.data_ptr() == table.data_ptr())
        old = self._row_grads.pop(p, None)
        if old is not None:               # a second backward before the step: accumulate the ordinary way
            dense = old.to_dense()
            p.grad = dense if p.grad is None else p.grad + dense
        self._row_grads[p] = rg

    def put_exchanged_rows(self, table, rg) -> bool:
        """A data-parallel exchange (distributed.TapExchange, owner mode) hands over the AVERAGED gradient of `table` in row form:
        the next clip_and_step reads it through rg's token -> row map.  False: not a table this optimizer can take that way."""
        p = next((q for g in self.param_groups for q in g["params"] if q.data_ptr() == table.data_ptr()), None)
        if p is None or p.dim() != 2 or p.shape[1] % 4 != 0 or p.dtype != torch.float32 or not p.is_cuda \
                or os.environ.get("RBR_ROW_GRADS", "1") == "0":
            return False
        self._row_grads.clear()           # one row-form table per launch pair
        self._row_grads[p] = rg
        p.grad = None
        return True

    def close(self) -> None:
        """Unregisters the row-gradient hand-off (the tables get dense gradients again)."""
        for p in self._row_tables:
            RF.set_row_grad_sink(p, None)
        self._row_tables = []
        self.materialize_grads()

    @torch.no_grad()
    def materialize_grads(self) -> None:
        """Turns every pending compact row gradient into the dense `.grad` nn.Embedding's backward would have left (after a
        clipping step: the clipped gradient, as clip_grad_norm_ leaves it)."""
        for p, rg in list(self._row_grads.items()):
            dense = rg.to_dense()
            p.grad = dense if p.grad is None else p.grad + dense
        self._row_grads.clear()

    def zero_grad(self, set_to_none: bool = True):
        self._row_grads.clear()
        super().zero_grad(set_to_none=set_to_none)

    def _counter_of(self, p):
        st = self.state.get(p)
        return st["step"] if st else None

    def _shared_counter(self, ps):
        """The device step counter of one launch pair.  `ps` hold one counter already, or have no state yet: their state is
        created around a fresh counter at 0 (torch.optim.Adam's lazy state: the count starts with the first gradient).  A counter
        that tensors outside `ps` hold as well -- they have no gradient on this step, or lie beyond the 64 tensors of a pair --
        must not advance for them: `ps` move on with a copy."""
        step = self._counter_of(ps[0])
        if step is None:
            step = torch.zeros((), dtype=torch.float32, device=ps[0].device)
            for p in ps:
                st = self.state[p]
                st["step"] = step
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            return step
        mine = {id(p) for p in ps}
        if any(st.get("step") is step and id(q) not in mine for q, st in self.state.items()):
            step = step.clone()
            for p in ps:
                self.state[p]["step"] = step
        return step

    @torch.no_grad()
    def clip_and_step(self, max_grad_norm: float | None = None) -> torch.Tensor:
        """Clips the gradients of ALL parameter groups to a total 2-norm of `max_grad_norm` (None: no clipping),
        applies the Adam update, leaves the clipped gradients in .grad and returns the norm before clipping."""
        import ctypes as C
        from . import _lib
        L_ = _lib.lib()
        for p in [q for q in self._row_grads if q.grad is not None]:      # mixed: a dense gradient exists too -> dense path
            p.grad = p.grad + self._row_grads.pop(p).to_dense()
        todo = [(g, p) for g in self.param_groups for p in g["params"] if p.grad is not None or p in self._row_grads]
        if not todo:
            raise RuntimeError("HipClipAdam.clip_and_step: no gradients")
        dev = todo[0][1].device
        if self._ws is None or self._ws.device != dev:
            self._ws = torch.empty(L_.rbr_clip_adam_ws_floats(), dtype=torch.float32, device=dev)
            self._gnorm = torch.zeros((), dtype=torch.float32, device=dev)
        st = _lib.current_stream()
        # one launch pair per parameter group, per step counter (the tensors of a pair share one: the class docstring) and per 64
        # tensors; the common case (17 tensors, one group, always stepping together) is one pair.
        # With several pairs the norm must still be global: a first sweep with lr = 0 would be wasteful, so more than
        # one pair is only allowed without clipping.
        batches = []
        for g in self.param_groups:
            by_counter = {}               # id of the counter (None: no state yet) -> its tensors, in parameter order
            for gg, p in todo:
                if gg is g:
                    c = self._counter_of(p)
                    by_counter.setdefault(None if c is None else id(c), []).append(p)
            for ps in by_counter.values():
                for k in range(0, len(ps), self.MAX_TENSORS):
                    batches.append((g, ps[k:k + self.MAX_TENSORS]))
        if self._row_grads and (len(batches) > 1 or len(self._row_grads) > 1):
            self.materialize_grads()          # one compact table per launch pair: anything else takes the dense path
        if len(batches) > 1 and max_grad_norm is not None:
            # the fused clip needs every gradient in ONE launch pair; beyond 64 tensors (or with several parameter groups) the
            # norm and the in-place scaling are torch's clip_grad_norm_ (same maths, device-side, capturable) and the launch
            # pairs below run without clipping
            gn = nn.utils.clip_grad_norm_([p for _, p in todo], max_grad_norm)
            self._gnorm.copy_(gn)
            max_grad_norm = None
        elif len(batches) > 1:            # no pair sees every gradient: the returned norm is torch's as well
            self._gnorm.copy_(torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for _, p in todo]))))
        for g, ps in batches:
            step = self._shared_counter(ps)
            states = [self.state[p] for p in ps]
            grads = [p.grad for p in ps]          # None for the table whose gradient is in row form
            for p, gr in zip(ps, grads):
                if not (p.is_contiguous() and (gr is None or gr.is_contiguous())):
                    raise RuntimeError("HipClipAdam needs contiguous parameters and gradients")
            numel = (C.c_int64 * len(ps))(*[p.numel() for p in ps])
            b1, b2 = g["betas"]
            ev = _lib.TIMER.record("clip_adam_step")
            args = (len(ps), _lib.ptr_array(ps, torch.float32, "param"), _lib.ptr_array(grads, torch.float32, "grad"),
                    _lib.ptr_array([s_["exp_avg"] for s_ in states], torch.float32, "exp_avg"),
                    _lib.ptr_array([s_["exp_avg_sq"] for s_ in states], torch.float32, "exp_avg_sq"),
                    numel, float(max_grad_norm) if max_grad_norm is not None else 0.0,
                    float(g["lr"]), float(b1), float(b2), float(g["eps"]), _lib.dev_ptr(step, torch.float32, "step"),
                    _lib.dev_ptr(self._gnorm, torch.float32, "gnorm") if len(batches) == 1 else None,
                    _lib.dev_ptr(self._ws, torch.float32, "ws"))
            rowp = [k for k, p in enumerate(ps) if p in self._row_grads]
            if rowp:
                rg = self._row_grads[ps[rowp[0]]]
                # the kernel leaves the rows as they are and the clip coefficient beside them: to_dense() applies it
                if rg.coef is None:
                    rg.coef = torch.empty((), dtype=torch.float32, device=dev)
                crg = _lib.RowGrad(rowp[0], rg.V, rg.D, rg.row_of_token_ptr, rg.rows.data_ptr(), rg.sq.data_ptr(), rg.sq.numel(),
                                   rg.coef.data_ptr())
                _lib.check(L_.rbr_clip_adam_step_rows(*args, C.byref(crg), st), "rbr_clip_adam_step_rows")
            else:
                _lib.check(L_.rbr_clip_adam_step(*args, st), "rbr_clip_adam_step")
            if ev is not None:
                ev.record()
        return self._gnorm

    @torch.no_grad()
    def step(self, closure=None):
        """Plain Adam step (no clipping), for callers that clip separately: `loss.backward(); clip_grad_norm_(...); opt.step()`
        sees every gradient as a dense .grad, because a backward outside row_grad_scope() never produces the row form.  Should
        rows be pending all the same (the caller opened the scope and then clipped by hand), they are made dense here first --
        late for that clip, which is why the scope is train_step()'s business and not a default."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step(None)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch.optim.Adam checkpoints hold a step per parameter (a CPU float / int, or a tensor each): equal counts of a group
        # go onto one device counter, so that the group is one launch pair again; reading them is a host synchronisation
        for g in self.param_groups:
            shared = {}
            for p in g["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    key = (float(st["step"]), st["exp_avg"].device)
                    if key not in shared:
                        shared[key] = torch.as_tensor(key[0], dtype=torch.float32, device=key[1])
                    st["step"] = shared[key]


def train_step(model: nn.Module, optimizer: torch.optim.Optimizer, batch, ratings: torch.Tensor,
               max_grad_norm: float = MAX_GRAD_NORM, grad_sync=None, objective=None):
    """One step.  `batch` is the tuple passed to model(*batch); models returning a tuple
    (NARRE: pred, u_att, i_att) contribute their first element.  `grad_sync(model)` is the
    data-parallel gradient all-reduce hook (None on one GPU).  Returns (loss, gnorm, pred) tensors.
    `objective` (None: the trainers' MSELoss against `ratings`): a callable pred -> scalar loss that replaces it, e.g.
    BprObjective; `ratings` is then not looked at and `pred` has as many rows as the objective's feed made of the batch."""
    optimizer.zero_grad()
    if objective is None:
        pred, loss = _forward_loss_backward(model, batch, ratings, optimizer if grad_sync is None else None)
    else:
        pred, loss = _forward_objective_backward(model, batch, objective, optimizer if grad_sync is None else None)
    if grad_sync is not None:
        if isinstance(optimizer, HipClipAdam):
            optimizer.materialize_grads()        # the all-reduce wants every gradient as a dense .grad
        grad_sync(model)
    gnorm = clip_and_step(model, optimizer, max_grad_norm)
    return loss.detach(), gnorm, pred.detach()


def _forward_loss_backward(model: nn.Module, batch, ratings: torch.Tensor, optimizer=None):
    """y = model(*batch); loss = MSELoss()(y, ratings); loss.backward()  (train_deepconn_pp.py:162-165).  The target is
    announced to the forward (functional.fused_loss): a model whose last launch can compute the loss takes it along.
    `optimizer`: the optimizer whose step follows this backward; a HipClipAdam then takes its tables' gradients in compact row
    form (its row_grad_scope() is open for exactly this forward + backward)."""
    scope = optimizer.row_grad_scope() if isinstance(optimizer, HipClipAdam) else contextlib.nullcontext()
    fusable = ratings.is_cuda and ratings.dtype == torch.float32
    with scope:
        # (after_backward: the loss is read only once the backward below has been issued, so the forward may leave it to it)
        with (RF.fused_loss(ratings, after_backward=True) if fusable else contextlib.nullcontext()) as req:
            out = model(*batch)
            pred = out[0] if isinstance(out, tuple) else out
            loss = req.loss_for(pred) if req is not None else None
        if loss is not None:
            loss.backward(RF.unit_scalar(pred.device))
            return pred, loss
        return pred, _loss_and_backward(pred, ratings)


def _forward_objective_backward(model: nn.Module, batch, objective, optimizer=None):
    """y = model(*batch); loss = objective(y); loss.backward() -- no MSE target is announced to the forward (the model's head runs
    un-fused), and the root gradient is the cached unit scalar, which functional.bpr_loss answers without a launch."""
    scope = optimizer.row_grad_scope() if isinstance(optimizer, HipClipAdam) else contextlib.nullcontext()
    with scope:
        if hasattr(objective, "forward_loss"):      # an objective over the towers' latents runs the model's forward itself
            pred, loss = objective.forward_loss(model, batch)
        else:
            out = model(*batch)
            pred = out[0] if isinstance(out, tuple) else out
            loss = objective(pred)
        loss.backward(RF.unit_scalar(pred.device) if pred.is_cuda else None)
    return pred, loss


class BprObjective:
    """loss = functional.bpr_loss(pred, feed.n_neg, feed.valid) for a step fed through `feed` (a data.NegativeFeed): pred's rows
    are the feed's expanded pairs -- the B observed pairs, then n_neg slabs of their sampled negatives -- and the loss is the mean
    of -log sigmoid(pred_pos - pred_neg) over the negatives the sampler could draw.  Pass it as `objective` to train_step /
    GraphedTrainStep together with the feed."""

    def __init__(self, feed):
        self.feed = feed

    def __call__(self, pred: torch.Tensor) -> torch.Tensor:
        n_neg = self.feed.n_neg
        if pred.dim() != 1 or pred.shape[0] % (1 + n_neg):
            raise RuntimeError(f"BprObjective: pred {tuple(pred.shape)} is not (1 + {n_neg}) * B scores")
        return RF.bpr_loss(pred, n_neg, self.feed.buffers(pred.shape[0] // (1 + n_neg))[2])


class AhnBprObjective:
    """BprObjective for AHN, with the forward_loss(model, batch) protocol: `batch` is the feed's expanded batch -- AHN's ten
    arguments for (1 + n_neg) * B rows -- and the scores come from model.forward_groups(*batch, groups=1 + n_neg), which encodes
    every user once (from the observed pair's rows: the AHN BPR rule stated there) and runs the pair-dependent tail as one HIP
    op; the loss is functional.bpr_loss over the feed's valid flags, as in BprObjective.  The step stays eager."""

    def __init__(self, feed):
        if not hasattr(feed, "n_neg") or not hasattr(feed, "buffers"):
            raise ValueError("AhnBprObjective takes a data.NegativeFeed (n_neg, the valid flags of its last draw)")
        self.feed = feed

    def forward_loss(self, model, batch):
        if not hasattr(model, "forward_groups"):
            raise ValueError(f"AhnBprObjective needs a model with forward_groups(); {type(model).__name__} has none")
        n_neg = self.feed.n_neg
        rows = batch[0].shape[0]
        if rows % (1 + n_neg):
            raise RuntimeError(f"AhnBprObjective: a batch of {rows} rows is not (1 + {n_neg}) * B pairs")
        pred = model.forward_groups(*batch, groups=1 + n_neg)[0]
        return pred, RF.bpr_loss(pred, n_neg, self.feed.buffers(rows // (1 + n_neg))[2])


class InBatchSoftmaxObjective:
    """The in-batch softmax ranking objective for a step fed through `feed` (a data.InBatchFeed): the towers' latent rows of the
    B observed pairs (model.pair_latents), then functional.pair_softmax_loss over ALL B x B pairs -- every user's negatives are
    the batch's other items, less the pad id, the row's own item again and the items the user has rated (feed.seen) -- scored
    by the model's own head (score_mode_and_params(): FM with the head's dropout drawn in the kernel, or D-ATT's dot) at
    `temperature`.  `logq` (f32 [n_items] on the device, or None): the log sampling probability of every item, subtracted from
    its column's logit (the sampled-softmax correction for popular items).  forward_loss(model, batch) -> (pos, loss) with
    pos [B] the observed pairs' scores; pass the objective as `objective` to train_step / GraphedTrainStep together with the feed.
    user_bias and g_bias receive an exactly zero gradient (a per-user constant cancels in a softmax over items)."""

    def __init__(self, model, feed, temperature: float = 1.0, logq=None):
        for name in ("pair_latents", "score_mode_and_params"):
            if not hasattr(model, name):
                raise ValueError(f"InBatchSoftmaxObjective needs a two-tower model with {name}(); {type(model).__name__} has none")
        if not hasattr(feed, "seen") or not hasattr(feed, "item_lo") or not hasattr(feed, "_last"):
            raise ValueError("InBatchSoftmaxObjective takes a data.InBatchFeed (the batch's ids, the seen CSR, item_lo)")
        temperature = float(temperature)
        if not (temperature > 0.0 and temperature < float("inf")):
            raise ValueError(f"temperature must be positive and finite, got {temperature}")
        self.feed, self.temperature = feed, temperature
        self.logq = None if logq is None else logq.detach().to(torch.float32).contiguous().view(-1, 1)

    def forward_loss(self, model, batch):
        feed = self.feed
        if feed._last is None:
            raise RuntimeError("InBatchSoftmaxObjective: the feed has gathered no batch yet (feed.inputs / feed.gather come first)")
        u_ids, i_ids = feed.u_ids, feed.i_ids
        ul, il = model.pair_latents(*batch)
        if ul.shape[0] != u_ids.shape[0]:
            raise RuntimeError(f"InBatchSoftmaxObjective: the batch has {ul.shape[0]} pairs, the feed's last gather {u_ids.shape[0]}")
        mode, h, g, ub, ib = model.score_mode_and_params()
        row_bias = col_bias = logq = None
        p_drop = 0.0
        u_idx, i_idx = u_ids, i_ids
        if getattr(model, "validate_ids", True) and (ub is not None or ib is not None or self.logq is not None):
            # ids as indices: range-checked like every other lookup of the model (one launch for both); a caller that has
            # validated its split and switched the model's check off (the trainer) spares this launch as well
            u_idx, i_idx = RF.sanitize_ids([(u_ids, ub.shape[0] if ub is not None else (1 << 62), 0),
                                            (i_ids, ib.shape[0] if ib is not None else self.logq.shape[0], 0)])
        if mode == "fm":
            fm = model.fm
            if fm.training and torch.is_grad_enabled():
                p_drop = float(fm.dropout.p)
            if ub is not None:
                row_bias = RF.embedding(ub, u_idx, fm.user_padding_idx).view(-1) + g
                col_bias = RF.embedding(ib, i_idx, fm.item_padding_idx).view(-1)
            else:
                row_bias = g.expand(ul.shape[0])
        if self.logq is not None:
            logq = RF.embedding(self.logq, i_idx, None).view(-1)
        drop = None
        if p_drop >= 1.0:
            drop, p_drop = torch.zeros(ul.shape[0], ul.shape[0], ul.shape[1], dtype=torch.float32, device=ul.device), 0.0
        loss, pos = RF.pair_softmax_loss(ul, il, u_ids, i_ids, mode, h=h, row_bias=row_bias, col_bias=col_bias, drop=drop,
                                         seen=feed.seen, item_lo=feed.item_lo, logq=logq, temperature=self.temperature, p_drop=p_drop)
        return pos, loss


def _loss_and_backward(pred: torch.Tensor, ratings: torch.Tensor) -> torch.Tensor:
    """loss = MSELoss()(pred, ratings); loss.backward()  (train_deepconn_pp.py:164-165)."""
    if pred.is_cuda and pred.dtype == torch.float32 and ratings.dtype == torch.float32 and pred.shape == ratings.shape:
        # one launch for the loss AND its gradient; the root gradient is a cached device scalar (no fill per step)
        loss = RF.mse_loss(pred, ratings)
        loss.backward(RF.unit_scalar(pred.device))
    else:
        loss = F.mse_loss(pred, ratings)
        loss.backward()
    return loss


def clip_and_step(model: nn.Module, optimizer: torch.optim.Optimizer, max_grad_norm: float) -> torch.Tensor:
    """clip_grad_norm_(model.parameters(), max_grad_norm); optimizer.step()  (train_deepconn_pp.py:166-167).
    Returns the total gradient norm before clipping."""
    if isinstance(optimizer, HipClipAdam):
        return optimizer.clip_and_step(max_grad_norm)
    gnorm = nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
    optimizer.step()
    return gnorm


def _flat_layout(tensors, align: int = 256):
    """Byte offsets of `tensors` laid out one after another in one block; neighbours (2k, 2k+1) of equal shape and dtype
    are packed back to back (no padding between them) so functional.stack_rows() sees one [2n, ...] tensor.  Last entry:
    total bytes."""
    offs, o, k = [], 0, 0
    while k < len(tensors):
        a = tensors[k]
        b = tensors[k + 1] if k + 1 < len(tensors) else None
        o = (o + align - 1) // align * align
        offs.append(o)
        o += a.numel() * a.element_size()
        if b is not None and a.shape == b.shape and a.dtype == b.dtype and a.dim() >= 1:
            offs.append(o)
            o += b.numel() * b.element_size()
            k += 2
        else:
            k += 1
    offs.append((o + align - 1) // align * align)
    return offs


def _flat_views(flat: torch.Tensor, layout, like):
    return [flat[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for o, t in zip(layout, like)]


class _InputBlock:
    """`tensors` in ONE block: `flat` (uint8, _flat_layout) and `views` of it with the tensors' shapes and dtypes, initialised from
    them -- so a loader hands a batch over with a single copy, and the two towers' inputs are neighbours that the models stack
    as a view.  `mismatch`: the error text for a packed block of another layout."""
    __slots__ = ("layout", "flat", "views", "mismatch")

    def __init__(self, tensors, device, mismatch: str):
        tensors = list(tensors)
        self.layout, self.mismatch = _flat_layout(tensors), mismatch
        self.flat = torch.empty(self.layout[-1], dtype=torch.uint8, device=device)
        self.views = tuple(_flat_views(self.flat, self.layout, tensors))
        for v, src in zip(self.views, tensors):
            v.copy_(src)

    def matches(self, batch) -> bool:
        """True when `batch` has the views' shapes and dtypes."""
        return len(batch) == len(self.views) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(batch, self.views))

    def pack(self, tensors, device=None) -> torch.Tensor:
        """`tensors` as one block of this layout, on the block's device (or on `device`)."""
        tensors = list(tensors)
        blob = torch.empty(self.flat.shape, dtype=torch.uint8, device=device or self.flat.device)
        for v, src in zip(_flat_views(blob, self.layout, tensors), tensors):
            v.copy_(src)
        return blob

    def load(self, tensors=None, packed: torch.Tensor | None = None, pack_on_host: bool = False) -> None:
        """Copies into the block on the current stream: `packed` (pack()'s blob) with one copy; `tensors` (one per view, None: leave
        that view) with one copy per tensor that is not already its view -- or, with pack_on_host and all of them in host memory,
        packed there and sent with ONE host-to-device copy."""
        if packed is not None:
            if packed.shape != self.flat.shape or packed.dtype != torch.uint8:
                raise RuntimeError(self.mismatch)
            self.flat.copy_(packed, non_blocking=True)
        if tensors is None:
            return
        if pack_on_host and all(t is not None and not t.is_cuda for t in tensors):
            self.flat.copy_(self.pack(tensors, "cpu"), non_blocking=True)
            return
        for dst, src in zip(self.views, tensors):
            if src is not None and dst is not src:
                dst.copy_(src, non_blocking=True)


def _lib_mod():
    from . import _lib
    return _lib


def _capture_stream(dev) -> torch.cuda.Stream:
    """A stream to record a graph on, with the library's per-stream state (functional.prepare_stream_state) already in place."""
    cs = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(cs):
        RF.prepare_stream_state(dev)
    torch.cuda.synchronize(dev)
    return cs


class GraphedForward:
    """model(*batch) under torch.no_grad(), recorded once into a hipGraph and replayed: the eval / serving forward of a
    fixed batch shape (the trainers' validation loops, trainer/train_deepconn_pp.py:171-196: ~25 short kernels whose eager
    launches leave the GPU waiting on Python).  The model's train/eval mode at construction is what the graph holds -- put
    the model in eval() first.  __call__ copies a batch of the same shapes into the static input block (one copy when it was
    pack()ed) and replays; the returned prediction tensor is static: overwritten by the next replay.

    `feed` (a data.DeviceDocCache, or a data.ReviewFeed for the review split; from_ids()): the batch is (u_ids, i_ids) and the
    graph starts with the gather of their documents into the model's input block (with_ids=False: documents only, D-ATT's
    forward)."""

    def __init__(self, model: nn.Module, batch, warmup: int = 2, capture_error_mode: str = "global", feed=None,
                 with_ids: bool = True):
        batch = list(batch)
        if not batch or not batch[0].is_cuda:
            raise RuntimeError("GraphedForward needs HIP tensors")
        self.model = model
        self._feed, self._with_ids = feed, with_ids
        mismatch = "packed batch does not match the forward's input layout (use GraphedForward.pack)"
        # `_staged` is the block a caller's batch is copied into: the model's inputs, or with a feed the (u_ids, i_ids) block
        self._staged = block = _InputBlock(batch, batch[0].device, mismatch)
        self.ids = None
        if feed is not None:
            self.ids = block.views
            block = _InputBlock(feed.empty_inputs(batch[0].shape[0], with_ids), batch[0].device, mismatch)
        self.batch = block.views
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():      # warm-up off the default stream (allocator, lazy module state)
            for _ in range(warmup):
                self._prologue()
                model(*self.batch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        self._capture_stream = _capture_stream(batch[0].device)
        self._kept_ws = []           # forward workspaces the graph keeps the addresses of (functional.kept_ws_owner)
        with torch.no_grad(), _lib_mod().capture_guard(self._capture_stream), RF.kept_ws_owner(self._kept_ws), \
                torch.cuda.graph(self.graph, stream=self._capture_stream, capture_error_mode=capture_error_mode):
            self._prologue()
            out = model(*self.batch)
        self.pred = out[0] if isinstance(out, tuple) else out

    @classmethod
    def from_ids(cls, model: nn.Module, cache, u_ids: torch.Tensor, i_ids: torch.Tensor, with_ids: bool = True, **kw):
        """The id-fed forward: replays gather (cache.gather) + model; __call__((u_ids, i_ids))."""
        return cls(model, (u_ids, i_ids), feed=cache, with_ids=with_ids, **kw)

    def _prologue(self):
        if self._feed is not None:
            self._feed.gather(self.ids[0], self.ids[1], out=self.batch)

    def matches(self, batch) -> bool:
        """True when `batch` has the shapes and dtypes the graph was recorded with (a ragged last batch does not)."""
        return self._staged.matches(batch)

    def pack(self, batch) -> torch.Tensor:
        return self._staged.pack(batch)

    def __call__(self, batch=None, packed: torch.Tensor | None = None) -> torch.Tensor:
        self._staged.load(packed=packed)
        if batch is not None:
            if not self.matches(batch):
                raise RuntimeError("batch shapes differ from the recorded forward's (run ragged batches eagerly)")
            self._staged.load(batch)
        self.graph.replay()
        return self.pred


def _count_kernel_nodes(graph: torch.cuda.CUDAGraph) -> int:
    """hipGraphGetNodes + hipGraphNodeGetType over the captured hipGraph_t (kernel nodes only: type 0)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    g = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(g, None, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (C.c_void_p * max(1, n.value))()
    if hip.hipGraphGetNodes(g, nodes, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    kernels = 0
    for k in range(n.value):
        ty = C.c_int(-1)
        if hip.hipGraphNodeGetType(C.c_void_p(nodes[k]), C.byref(ty)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        kernels += int(ty.value == 0)          # hipGraphNodeTypeKernel
    return kernels


class _StepSlot:
    """One input slot of a GraphedTrainStep -- `block`: the model's inputs, `staged`: the block a loader writes (the same one, or
    with a feed the id block) -- and the graph(s) recorded over it."""
    __slots__ = ("block", "staged", "batch", "ratings", "ids", "g_fwd_bwd", "g_update", "static_grads", "loss", "gnorm", "pred")


class GraphedTrainStep:
    """train_step() recorded once into a hipGraph and replayed: the step is ~70 short kernels (0.8 ms of GPU
    work at the cfg2 shape), so launching them one by one from Python leaves the GPU waiting on the host.

    Everything data-dependent in the HIP path (distinct-token list, work lists, argmax windows) lives in device
    memory and every launch has a shape-only grid, so a recorded step is valid for any batch of the same shape:
    __call__ copies the new batch into the static input buffers and replays.  With a data-parallel
    `grad_sync` the step is recorded as two graphs (zero_grad+forward+backward | clip+Adam) sharing one memory
    pool, and the RCCL all-reduce runs eagerly between them.

    `slots` > 1 records the step once per INPUT SLOT: each slot has its own input block, so a loader stages batch
    i + 1 into slot (i + 1) % slots (one host-to-device copy, `stage` / `slot_inputs`) while slot i % slots is replayed,
    and the step itself starts with no device-to-device copy of its inputs (`__call__(slot=k)`).  Parameters,
    optimizer state and the optimizer's own buffers are shared by the slots; every slot keeps its own graph memory.

    The optimizer must have been built with make_optimizer(..., capturable=True).

    `feed` (a data.DeviceDocCache, or a data.ReviewFeed for the review split; from_ids()): the id-fed step.  `batch` is then (u_ids, i_ids); a slot stages only
    (u_ids, i_ids, ratings) -- one small block, `stage` / `slot_inputs` -- and its graph starts with the gather of the
    documents into the slot's document block (cache.gather: documents, masks and checked ids for DeepCoNN++; documents
    only with with_ids=False, D-ATT), followed by the unchanged step.

    `objective` (None: the MSE step): train_step's `objective`, e.g. BprObjective(feed) with `feed` a data.NegativeFeed -- the graph
    then starts with the negative sampler, the staged ratings are not looked at and `pred` has the feed's expanded rows."""

    def __init__(self, model: nn.Module, optimizer: torch.optim.Optimizer, batch, ratings: torch.Tensor,
                 max_grad_norm: float = MAX_GRAD_NORM, grad_sync=None, warmup: int = 3, capture_error_mode: str | None = None,
                 slots: int = 1, keep_graph: bool = False, feed=None, with_ids: bool = True, objective=None):
        if not ratings.is_cuda:
            raise RuntimeError("GraphedTrainStep needs HIP tensors")
        if slots < 1:
            raise ValueError("slots must be >= 1")
        if objective is not None and grad_sync is not None:
            raise ValueError("a recorded step with an objective is not available with grad_sync (data-parallel training keeps "
                             "the MSE step)")
        self.objective = objective
        self.model, self.optimizer, self.grad_sync, self.max_grad_norm = model, optimizer, grad_sync, max_grad_norm
        self._keep_graph = bool(keep_graph)      # keeps the hipGraph_t behind the executable: kernel_launches() can count its nodes
        self._feed, self._with_ids = feed, with_ids
        self._slots = []
        for _ in range(slots):
            # what a loader stages -- the batch and its ratings -- lives in ONE block; with a feed that is (u_ids, i_ids, ratings),
            # and the documents are gathered on the device into a block of their own
            sl = _StepSlot()
            sl.staged = sl.block = _InputBlock(list(batch) + [ratings], ratings.device, "packed batch does not match the step's "
                                               "input layout (use GraphedTrainStep.pack)" if feed is None else
                                               "packed ids do not match the step's id block (use GraphedTrainStep.pack)")
            sl.batch, sl.ratings, sl.ids = sl.staged.views[:-1], sl.staged.views[-1], None
            if feed is not None:
                sl.ids = sl.batch
                sl.block = _InputBlock(feed.empty_inputs(batch[0].shape[0], with_ids), ratings.device, sl.staged.mismatch)
                sl.batch = sl.block.views
            sl.g_update = sl.static_grads = None
            self._slots.append(sl)
        first = self._slots[0]
        # the warm-up steps below must not count as training: parameters and Adam state are put back in place
        # (same storage -- the recorded graph keeps their addresses) once the graph exists
        saved_params = [p.detach().clone() for p in model.parameters()]
        saved_state = {p: {k: v.clone() for k, v in optimizer.state[p].items() if torch.is_tensor(v)}
                       for group in optimizer.param_groups for p in group["params"] if p in optimizer.state}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):      # warm-up off the default stream: allocator, lazy optimizer state, occupancy queries
            for _ in range(warmup):
                self._prologue(first)
                train_step(model, optimizer, first.batch, first.ratings, max_grad_norm, grad_sync, objective)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # with a process group alive, RCCL's watchdog thread polls events while we record: only this thread's calls
        # may be policed by the capture ("thread_local"), as torch recommends for captures next to NCCL work
        mode = capture_error_mode or ("thread_local" if grad_sync is not None else "global")
        self._capture_stream = _capture_stream(ratings.device)
        cs = self._capture_stream
        self._kept_ws = []           # forward workspaces the graphs keep the addresses of (functional.kept_ws_owner)
        for sl in self._slots:
            if sl is not first:      # every recording takes its own kept workspaces: one more set on the capture stream
                with torch.cuda.stream(cs):
                    RF.prepare_stream_state(ratings.device)
                torch.cuda.synchronize(ratings.device)
            optimizer.zero_grad(set_to_none=True)
            sl.g_fwd_bwd = torch.cuda.CUDAGraph(keep_graph=True) if self._keep_graph else torch.cuda.CUDAGraph()
            if grad_sync is None:
                with _lib_mod().capture_guard(cs), RF.kept_ws_owner(self._kept_ws), \
                        torch.cuda.graph(sl.g_fwd_bwd, stream=cs, capture_error_mode=mode):
                    self._prologue(sl)
                    sl.loss, sl.gnorm, sl.pred = train_step(model, optimizer, sl.batch, sl.ratings, max_grad_norm,
                                                            objective=objective)
                sl.static_grads = [(p, p.grad) for p in model.parameters()]
            else:
                with _lib_mod().capture_guard(cs), RF.kept_ws_owner(self._kept_ws), \
                        torch.cuda.graph(sl.g_fwd_bwd, stream=cs, capture_error_mode=mode):
                    self._prologue(sl)
                    optimizer.zero_grad()
                    pred, loss = _forward_loss_backward(model, sl.batch, sl.ratings)
                    sl.loss, sl.pred = loss.detach(), pred.detach()
                    if isinstance(optimizer, HipClipAdam):
                        optimizer.materialize_grads()
                grad_sync(model)
                sl.static_grads = [(p, p.grad) for p in model.parameters()]
                sl.g_update = torch.cuda.CUDAGraph(keep_graph=True) if self._keep_graph else torch.cuda.CUDAGraph()
                with _lib_mod().capture_guard(cs), torch.cuda.graph(sl.g_update, pool=sl.g_fwd_bwd.pool(), stream=cs, capture_error_mode=mode):
                    sl.gnorm = clip_and_step(model, optimizer, max_grad_norm)
        with torch.no_grad():
            for p, v in zip(model.parameters(), saved_params):
                p.copy_(v)
            for group in optimizer.param_groups:
                for p in group["params"]:
                    for k, v in optimizer.state.get(p, {}).items():
                        if torch.is_tensor(v):
                            old = saved_state.get(p, {}).get(k)
                            v.copy_(old) if old is not None else v.zero_()
        if self._slots[-1].static_grads is not None:
            for p, g in first.static_grads:
                p.grad = g

    @classmethod
    def from_ids(cls, model: nn.Module, optimizer: torch.optim.Optimizer, cache, u_ids: torch.Tensor, i_ids: torch.Tensor,
                 ratings: torch.Tensor, max_grad_norm: float = MAX_GRAD_NORM, grad_sync=None, with_ids: bool = True, **kw):
        """The id-fed step over `cache` (data.DeviceDocCache): each replay gathers the staged ids' documents, then steps.
        with_ids=False: the model takes (u_docs, i_docs) only (D-ATT)."""
        return cls(model, optimizer, (u_ids, i_ids), ratings, max_grad_norm, grad_sync, feed=cache, with_ids=with_ids, **kw)

    def _prologue(self, sl) -> None:
        """What a slot's graph runs in front of the step: the id feed's gather (nothing without a feed)."""
        if self._feed is not None:
            self._feed.gather(sl.ids[0], sl.ids[1], out=sl.batch)

    # slot 0 under the names the one-slot step has always had
    batch = property(lambda self: self._slots[0].batch)
    ratings = property(lambda self: self._slots[0].ratings)
    loss = property(lambda self: self._slots[0].loss)
    gnorm = property(lambda self: self._slots[0].gnorm)
    pred = property(lambda self: self._slots[0].pred)
    g_fwd_bwd = property(lambda self: self._slots[0].g_fwd_bwd)
    g_update = property(lambda self: self._slots[0].g_update)
    _flat = property(lambda self: self._slots[0].block.flat)

    @property
    def slots(self) -> int:
        return len(self._slots)

    def kernel_launches(self, slot: int = 0):
        """Kernel nodes of the recorded step (slot `slot`: forward + backward [+ the update graph of a data-parallel step]): what
        one replay launches.  Needs keep_graph=True at construction; None when the runtime does not hand the graph out."""
        sl = self._slots[slot]
        try:
            return sum(_count_kernel_nodes(g) for g in (sl.g_fwd_bwd, sl.g_update) if g is not None)
        except Exception:
            return None

    def slot_inputs(self, slot: int = 0):
        """(batch views, ratings view, the whole block as uint8) of input slot `slot`: what a loader writes into.  With an id
        feed: ((u_ids, i_ids) views, ratings view, the id block) -- slot_batch() has the gathered documents."""
        st = self._slots[slot].staged
        return st.views[:-1], st.views[-1], st.flat

    def slot_batch(self, slot: int = 0):
        """The model's input views of slot `slot` (with an id feed: what the recorded gather writes)."""
        return self._slots[slot].batch

    def pack(self, batch, ratings: torch.Tensor) -> torch.Tensor:
        """`batch` + `ratings` as one block in the layout of the step's input buffers (what a loader would stage on the
        device); hand it to __call__(packed=...).  With an id feed `batch` is (u_ids, i_ids) and the block is the id block."""
        return self._slots[0].staged.pack(list(batch) + [ratings])

    def stage(self, slot: int, batch=None, ratings: torch.Tensor | None = None, packed: torch.Tensor | None = None) -> None:
        """Copies a batch into input slot `slot` on the current stream (no replay).  With an id feed `batch` is (u_ids, i_ids):
        host tensors together with host ratings go over in ONE host-to-device copy of the id block."""
        st = self._slots[slot].staged
        tensors = None
        if batch is not None or ratings is not None:
            tensors = (list(batch) if batch is not None else [None] * (len(st.views) - 1)) + [ratings]
        st.load(tensors, packed, pack_on_host=self._feed is not None)

    def __call__(self, batch=None, ratings: torch.Tensor | None = None, packed: torch.Tensor | None = None, slot: int = 0):
        """Runs one step on `batch` / `packed` (None: the batch already in the slot's input block).  Returns the slot's
        static (loss, gnorm, pred) tensors -- overwritten by the next replay of that slot."""
        sl = self._slots[slot]
        if batch is not None or ratings is not None or packed is not None:
            self.stage(slot, batch, ratings, packed)
        sl.g_fwd_bwd.replay()
        if sl.static_grads is not None:
            # the graphs read and write the gradient tensors they were recorded with; an eager step in between (a ragged
            # last batch) re-points p.grad elsewhere, so hand the recorded tensors back before anything looks at p.grad
            for p, g in sl.static_grads:
                p.grad = g
        if sl.g_update is not None:
            tap = getattr(self.grad_sync, "tap", None)
            if tap is not None:
                tap.mark_replayed()          # the replayed backward refilled the tap buffers (distributed.TapExchange)
            self.grad_sync(self.model)
            sl.g_update.replay()
        return sl.loss, sl.gnorm, sl.pred
