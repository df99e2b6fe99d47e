"""The --optimizer choices (model/plt.py:150-161) on one flat parameter/gradient buffer: each rule is one HIP launch per
step (AdamW, the default, and sgd / radam / adabelief / adabound) or three (adamp, novograd: per-tensor reductions), plus
the device step-counter increment.

All parameters are re-pointed at views of a single fp32 buffer and their ``.grad`` at views of a second one,
so (a) the optimizer step is a single streaming kernel over the parameter, gradient and state arrays, (b) the
data-parallel reducer (xview2_amd.dist) all-reduces contiguous slices without packing copies.

``FlatEMA`` keeps an exponential moving average of that parameter buffer (one more launch per step) that validation,
``best.ckpt`` and evaluation can be taken from.

Gradient accumulation (``FlatOptimizer.accumulate``): the backward kernels overwrite their slot, so the sum over a group of
micro-batches is kept in a third flat buffer by one streaming launch per micro-batch, in micro-batch order; ``step`` adds it
into the gradient buffer and folds the group's 1 / m into the rule's gradient scale.
"""
import contextlib

import torch

from . import ops


class FlatOptimizer:
    """The flat buffers, the gradient slots the HIP backward kernels write into, the device-resident lr / step counter
    and the checkpoint surface shared by every rule.  A rule names its flat fp32 state arrays in STATE (allocated here,
    zero-initialised, saved under those names) and launches its kernels in _launch."""
    STATE = ()

    def __init__(self, params, lr, weight_decay=0.0):
        seen, plist = set(), []
        for p in params:
            if p.requires_grad and id(p) not in seen:      # FusedUNet registers every stage twice
                seen.add(id(p))
                plist.append(p)
        self.params = plist
        dev = plist[0].device
        sizes = [p.numel() for p in plist]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += (n + 3) // 4 * 4                      # keep every view 16-byte aligned
        self.offsets, self.total = offs, total
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        for name in self.STATE:
            setattr(self, name, torch.zeros(total, dtype=torch.float32, device=dev))
        with torch.no_grad():
            for p, o in zip(plist, offs):
                view = self.flat_p[o:o + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = None
                # the HIP backward kernels write a parameter's gradient straight into its slice of flat_g
                # (ops.grad_slot): autograd then adopts that view as .grad without an accumulation kernel
                p._xv2_slot = (self, o)
                p._xv2_epoch = -1
        ops.clear_pack_cache()         # the parameters just moved to new storage
        self.epoch = 0
        self.lr, self.weight_decay = lr, weight_decay
        self.step_count = 0
        self.param_groups = [{"lr": lr, "params": plist}]  # what utils/scheduler.py NoamLR touches
        # device-resident copies for hipGraph capture (see xview2_amd.graph.GraphedStep)
        self.capturable = dev.type == "cuda"   # always the device-state kernel on the GPU: one code path, graph-safe
        self.lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev) if dev.type == "cuda" else None
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev) if dev.type == "cuda" else None
        self._lr_on_dev = lr
        self.guard = None                  # the gradient guard's device record (set_guard)
        # gradient accumulation (accumulate): the running sum of a group's micro-batch gradients, flat_g's layout, allocated by
        # the first accumulate() and never saved; `pending` counts the micro-batches it holds; buckets_closed: the reducer has
        # already added it into every bucket of flat_g (dist.GradReducer), so step() must not do it again
        self.flat_acc, self.pending, self.buckets_closed = None, 0, False

    # ------------------------------------------------------------------ gradient accumulation
    def accumulate(self):
        """after backward() of a micro-batch that does NOT end its group, in place of step(): the micro-batch's gradient goes
        into flat_acc (include/xv2.h xv2_grad_accumulate: a copy for the group's first, one rounded addition per element
        afterwards), so the sum runs in micro-batch order.  zero_grad() stays the per-micro-batch call; the step() after the
        group's last backward() adds flat_acc into flat_g and divides by the group's size through the rule's gradient scale."""
        if not self.capturable:
            raise RuntimeError("gradient accumulation runs on the GPU only (HIP kernels; there is no CPU fallback)")
        from ._capi import call
        ops.join_wgrad_stream()
        self._gather_foreign_grads()       # shared weights' second contributions and torch-side gradients are in flat_g first
        if self.flat_acc is None:
            self.flat_acc = torch.empty_like(self.flat_g)
        call("xv2_grad_accumulate", self.flat_acc, self.flat_g, self.total, 0 if self.pending == 0 else 1)
        self.pending += 1

    def _close_group(self, grad_scale):
        """step() with micro-batches pending: every element of flat_g gets flat_acc added exactly once (here, unless the
        reducer did it bucket by bucket before its collectives); returns the scale with the group's 1 / m folded in, divided
        on the host in double like the reducer's 1 / world"""
        if self.pending == 0:
            return grad_scale
        if not self.buckets_closed:
            from ._capi import call
            call("xv2_grad_accumulate", self.flat_acc, self.flat_g, self.total, 2)
        scale = float(grad_scale / (self.pending + 1))
        self.pending, self.buckets_closed = 0, False
        return scale

    # ------------------------------------------------------------------ gradient guard
    def set_guard(self, max_norm=0.0, skip_nonfinite=False):
        """clip the global gradient norm to `max_norm` (0: no clipping; torch.nn.utils.clip_grad_norm_'s arithmetic) and /
        or skip a step whose gradient holds an Inf or NaN: two launches over flat_g in front of the rule (include/xv2.h
        xv2_grad_guard), decided and applied on the device - nothing syncs, and a captured step keeps it.  The record and
        the workspace are allocated once; a later call changes the settings and keeps the counters."""
        max_norm = float(max_norm)
        if not (0.0 <= max_norm < float("inf")):
            raise ValueError("max_norm = %r: must be finite and >= 0 (0: no clipping)" % max_norm)
        if not self.capturable:
            raise RuntimeError("the gradient guard runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if self.guard is None:
            from ._capi import query
            dev = self.flat_g.device
            self.guard = torch.zeros(8, dtype=torch.int64, device=dev)           # 64 bytes, layout in include/xv2.h
            self._guard_ws = torch.zeros(query("xv2_grad_guard_workspace", self.total) // 8, dtype=torch.float64, device=dev)
        self._guard_cfg = (max_norm, int(bool(skip_nonfinite)))

    def _guard_pass(self, grad_scale):
        """the norm pass over the (reduced, gathered) gradient, then the record named for the rule's entry point: call
        right before _launch"""
        if self.guard is None:
            return
        from ._capi import _func, call
        call("xv2_grad_guard", self.flat_g, self.total, float(grad_scale), self._guard_cfg[0], self._guard_cfg[1],
             self._guard_ws, self.guard)
        _func("xv2_optim_guard_ctx")(self.guard.data_ptr())

    def guard_stats(self):
        """the guard's record as a dict (the last step's norm / coef / skip, the cumulative counters, the largest finite
        norm).  Reading it synchronises with the device: the caller chooses when."""
        if self.guard is None:
            raise RuntimeError("no gradient guard is set (set_guard)")
        rec = self.guard.cpu()
        f, i = rec.view(torch.float32), rec.view(torch.int32)
        return {"norm": float(f[0]), "coef": float(f[1]), "skip": int(i[2]), "skipped_in_a_row": int(i[3]),
                "steps": int(rec[2]), "clipped": int(rec[3]), "skipped": int(rec[4]), "norm_max": float(f[10])}

    def zero_grad(self):
        ops.begin_step()               # (a backward pass that raised leaves its side-stream bookkeeping behind)
        self.flat_g.zero_()            # one memset; parameters that get no gradient this step stay at zero
        self.epoch += 1
        for p in self.params:
            p.grad = None

    def _gather_foreign_grads(self):
        """gradients that did not come from a HIP backward kernel (torch-side ops) are copied into their slice"""
        base = self.flat_g.data_ptr()
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is not None and g.data_ptr() != base + 4 * o:
                self.flat_g[o:o + p.numel()].view_as(p).copy_(g)
                p.grad = self.flat_g[o:o + p.numel()].view_as(p)

    def sync_lr(self):
        """push the host-side learning rate to the device copy (call OUTSIDE a captured region)"""
        lr = self.param_groups[0]["lr"]
        if self.lr_dev is not None and lr != self._lr_on_dev:
            self.lr_dev.fill_(lr)
            self._lr_on_dev = lr

    def step(self, grad_scale=1.0):
        """one update; grad_scale multiplies the gradient first (the reducer's 1/world).  With micro-batches pending
        (accumulate) it first closes their group: the guard and the rule see the group's sum once, scaled by 1 / m"""
        ops.join_wgrad_stream()      # weight-gradient kernels run on a side stream (ops.ASYNC_WGRAD)
        self._gather_foreign_grads()
        grad_scale = self._close_group(grad_scale)
        self.step_count += 1
        if not self.capturable:
            raise RuntimeError("%s steps on the GPU only (HIP kernels; there is no CPU fallback)" % type(self).__name__)
        self.sync_lr()
        self._guard_pass(grad_scale)
        self._launch(float(grad_scale))
        ops.weights_changed()
        ops.repack_all()       # the packed conv-weight layouts, refreshed in one launch

    def _launch(self, grad_scale):
        raise NotImplementedError

    def _extra_state(self):
        """state beyond the step, the flat STATE arrays and the lr (per-rule tensors / hyperparameters)"""
        return {}

    def _load_extra_state(self, sd):
        pass

    def state_dict(self):
        # under a guard the device counter is the truth: the host's count runs ahead after a skipped step, and a resumed
        # run must continue the bias corrections where the device stands (this read synchronises)
        sd = {"step": self.step_count if self.guard is None else int(self.step_dev.item())}
        sd.update((name, getattr(self, name)) for name in self.STATE)
        sd.update(self._extra_state())
        sd["lr"] = self.param_groups[0]["lr"]
        return sd

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        for name in self.STATE:
            getattr(self, name).copy_(sd[name])
        self._load_extra_state(sd)
        self.param_groups[0]["lr"] = sd["lr"]
        if self.step_dev is not None:
            # the GPU kernels take their bias corrections from the device-resident counter
            self.step_dev.fill_(int(sd["step"]))
            self.sync_lr()


class FlatAdamW(FlatOptimizer):
    """model/plt.py:154 torch.optim.AdamW (and model/plt.py:153 apex FusedAdam, whose default adam_w_mode is the same
    decoupled-decay update): one launch of xv2_adamw_step_dev"""
    STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, lr, weight_decay)
        self.betas, self.eps = betas, eps

    def step(self, grad_scale=1.0):
        ops.join_wgrad_stream()      # weight-gradient kernels run on a side stream (ops.ASYNC_WGRAD)
        self._gather_foreign_grads()
        grad_scale = self._close_group(grad_scale)
        self.step_count += 1
        lr = self.param_groups[0]["lr"]
        if self.capturable:
            from ._capi import call
            self.sync_lr()
            self._guard_pass(grad_scale)
            call("xv2_adamw_step_dev", self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.flat_p.numel(),
                 self.lr_dev, float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                 self.step_dev, float(grad_scale))
            ops.weights_changed()
            ops.repack_all()       # the packed conv-weight layouts, refreshed in one launch
            return
        ops.adamw_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, lr, self.betas[0], self.betas[1],
                       self.eps, self.weight_decay, self.step_count, grad_scale)
        ops.weights_changed()


class _FlatRule(FlatOptimizer):
    """a rule of xv2_flat_step_dev: one elementwise launch over the flat buffer and up to two state arrays"""
    RULE = None
    betas, eps, momentum, final_lr, gamma = (0.9, 0.999), 1e-8, 0.0, 0.1, 1e-3

    def _state_args(self):
        return [getattr(self, name) for name in self.STATE] + [None] * (2 - len(self.STATE))

    def _launch(self, grad_scale):
        from ._capi import call
        call("xv2_flat_step_dev", self.RULE, self.flat_p, self.flat_g, *self._state_args(), self.flat_p.numel(),
             self.lr_dev, self.step_dev, float(self.betas[0]), float(self.betas[1]), float(self.eps),
             float(self.weight_decay), float(self.momentum), float(getattr(self, "base_lr", 0.0)), float(self.final_lr),
             float(self.gamma), grad_scale)


class FlatSGD(_FlatRule):
    """model/plt.py:152 apex FusedSGD(lr, momentum): dampening 0, no Nesterov, no weight decay (the reference passes
    none, so --weight_decay does not reach it).  The momentum buffer starts as the first gradient."""

    def __init__(self, params, lr=3e-4, momentum=0.0):
        self.STATE = ("momentum_buffer",) if momentum != 0.0 else ()
        super().__init__(params, lr, 0.0)
        self.momentum = momentum
        self.RULE = 1 if momentum != 0.0 else 0


class FlatRAdam(_FlatRule):
    """model/plt.py:155 torch_optimizer RAdam(lr, weight_decay): decoupled decay p *= 1 - lr * wd, the rectified Adam
    step once rho_t >= 5, the bias-corrected momentum step before"""
    RULE = 2
    STATE = ("exp_avg", "exp_avg_sq")


class FlatAdaBelief(_FlatRule):
    """model/plt.py:156 torch_optimizer AdaBelief(lr, weight_decay): eps 1e-3 (the package's default), L2 decay added to
    the gradient, eps accumulated into the variance state"""
    RULE = 3
    STATE = ("exp_avg", "exp_avg_var")
    eps = 1e-3


class FlatAdaBound(_FlatRule):
    """model/plt.py:157 torch_optimizer AdaBound(lr, weight_decay): final_lr 0.1, gamma 1e-3, L2 decay; the bounds follow
    the learning rate relative to base_lr (the rate at construction)"""
    RULE = 4
    STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=3e-4, weight_decay=0.0):
        super().__init__(params, lr, weight_decay)
        self.base_lr = lr

    def _extra_state(self):
        return {"base_lr": self.base_lr}

    def _load_extra_state(self, sd):
        self.base_lr = sd["base_lr"]


class _FlatSegmented(FlatOptimizer):
    """rules with per-tensor / per-output-channel sums: the segment table of include/xv2.h (rows = dim-0 slices of a
    tensor with >= 2 dims, else the whole tensor) and the scratch, built once here"""
    betas, eps = (0.9, 0.999), 1e-8

    def __init__(self, params, lr, weight_decay):
        super().__init__(params, lr, weight_decay)
        rows, tens = [], []
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            n = p.numel()
            nr = p.shape[0] if p.dim() >= 2 and n > 0 else 1
            ln = n // nr
            tens.append((len(rows), nr, n, int(p.dim() >= 2)))
            rows.extend((o + r * ln, ln, i) for r in range(nr))
        dev = self.flat_p.device
        self.rows = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.tensors = torch.tensor(tens, dtype=torch.int64, device=dev)
        self.partials = torch.zeros(len(rows), 4, dtype=torch.float32, device=dev)


class FlatAdamP(_FlatSegmented):
    """model/plt.py:158 torch_optimizer AdamP(lr, weight_decay): delta 0.1, wd_ratio 0.1.  `decision` holds the view the
    last step projected each tensor with (0 none, 1 channel, 2 layer)."""
    STATE = ("exp_avg", "exp_avg_sq")
    delta, wd_ratio = 0.1, 0.1

    def __init__(self, params, lr=3e-4, weight_decay=0.0):
        super().__init__(params, lr, weight_decay)
        dev = self.flat_p.device
        self.decision = torch.zeros(len(self.params), dtype=torch.int32, device=dev)
        self.aux = torch.zeros(len(self.params), 2, dtype=torch.float32, device=dev)

    def _launch(self, grad_scale):
        from ._capi import call
        call("xv2_adamp_step_dev", self.rows, self.rows.shape[0], self.tensors, len(self.params), self.flat_p,
             self.flat_g, self.exp_avg, self.exp_avg_sq, self.partials, self.decision, self.aux, self.lr_dev,
             self.step_dev, float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
             float(self.delta), float(self.wd_ratio), grad_scale)


class FlatNovoGrad(_FlatSegmented):
    """model/plt.py:159 apex FusedNovoGrad(lr, weight_decay): grad averaging and bias correction on, decay outside the
    moment, L2 norms; exp_avg_norm is the per-tensor blended gradient norm (the first step's norm at step 1)"""
    STATE = ("exp_avg",)

    def __init__(self, params, lr=3e-4, weight_decay=0.0):
        super().__init__(params, lr, weight_decay)
        self.exp_avg_norm = torch.zeros(len(self.params), dtype=torch.float32, device=self.flat_p.device)

    def _extra_state(self):
        return {"exp_avg_norm": self.exp_avg_norm}

    def _load_extra_state(self, sd):
        self.exp_avg_norm.copy_(sd["exp_avg_norm"])

    def _launch(self, grad_scale):
        from ._capi import call
        call("xv2_novograd_step_dev", self.rows, self.rows.shape[0], self.tensors, len(self.params), self.flat_p,
             self.flat_g, self.exp_avg, self.exp_avg_norm, self.partials, self.lr_dev, self.step_dev,
             float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay), grad_scale)


class FlatEMA:
    """Exponential moving average of a FlatOptimizer's parameter buffer (include/xv2.h xv2_ema_update_dev): `ema` has
    flat_p's layout, padding included, and starts as a copy of it; `count_dev` counts the updates on the device.  Under
    --precision 16 flat_p holds the fp32 master weights, so the average is one of fp32 masters.

    The average covers the trainable parameters only.  Buffers (the BatchNorm running statistics, num_batches_tracked)
    are already averages of their own: the model computes with its live buffers inside applied(), and
    model_state_dict() passes them on as they are.

    decay d, warmup: the effective decay of update t (from 0) is min(d, (1 + t) / (10 + t)), so that the first updates
    are not dominated by the initial weights; warmup=False uses d throughout."""

    def __init__(self, optimizer, decay, warmup=True):
        if not isinstance(optimizer, FlatOptimizer):
            raise TypeError("FlatEMA averages the flat buffer of a FlatOptimizer, not %s" % type(optimizer).__name__)
        decay = float(decay)
        if not (0.0 <= decay < 1.0):
            raise ValueError("decay = %r: must lie in [0, 1)" % decay)
        if not optimizer.capturable:
            raise RuntimeError("FlatEMA updates on the GPU only (HIP kernels; there is no CPU fallback)")
        self.optimizer, self.decay, self.warmup = optimizer, decay, bool(warmup)
        self.ema = optimizer.flat_p.clone()
        self.count_dev = torch.zeros(1, dtype=torch.int32, device=self.ema.device)
        self._applied = False

    def update(self):
        """one call on the current stream, right after optimizer.step(...): the optimizer's guard record rides along, so
        a skipped step leaves the average and the counter alone"""
        if self._applied:
            raise RuntimeError("FlatEMA.update() inside applied(): the parameters hold the average itself")
        from ._capi import call
        o = self.optimizer
        call("xv2_ema_update_dev", self.ema, o.flat_p, o.total, self.decay, int(self.warmup), self.count_dev, o.guard)

    @torch.no_grad()
    def _exchange(self):
        """the contents of flat_p and ema change places (the parameters stay the same views), then the invalidation the
        optimizer's step uses: every cached layout of the old weights is stale"""
        o = self.optimizer
        tmp = o.flat_p.clone()
        o.flat_p.copy_(self.ema)
        self.ema.copy_(tmp)
        self._applied = not self._applied
        ops.weights_changed()
        ops.repack_all()

    @contextlib.contextmanager
    def applied(self):
        """inside, the model computes with the averaged weights through the ordinary HIP path; on the way out (also when
        the body raised) the exchange is undone and training continues as if the context had never been entered"""
        if self._applied:
            raise RuntimeError("FlatEMA.applied() is already entered")
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def _slices(self, model):
        """(name, tensor, offset or None) per state_dict entry: the offset into the flat buffer of every tensor that lives
        in flat_p, by address - which covers the names FusedUNet registers twice"""
        o = self.optimizer
        base, end = o.flat_p.data_ptr(), o.flat_p.data_ptr() + 4 * o.total
        for k, v in model.state_dict().items():
            inside = v.dtype == torch.float32 and v.numel() > 0 and v.device == o.flat_p.device and base <= v.data_ptr() < end
            yield k, v, (v.data_ptr() - base) // 4 if inside else None

    def model_state_dict(self, model):
        """the model's state_dict() with every tensor that lives in flat_p replaced by its slice of the average (views,
        as state_dict()'s own).  Trainable parameters only: buffers (BatchNorm running statistics, num_batches_tracked)
        are taken as they are - they are averages of their own already."""
        src = self.optimizer.flat_p if self._applied else self.ema
        return {k: (v if off is None else src[off:off + v.numel()].view(v.shape)) for k, v, off in self._slices(model)}

    def state_dict(self):
        """{"decay", "warmup", "updates"}; `updates` is read from the device (this synchronises)"""
        return {"decay": self.decay, "warmup": self.warmup, "updates": int(self.count_dev.item())}

    @torch.no_grad()
    def load_state_dict(self, sd, ema_state_dict=None, model=None):
        """restores the device counter and, given an EMA state dict (model_state_dict's product) and the model, the
        buffer by parameter name.  decay and warmup stay what this object was built with."""
        if self._applied:
            raise RuntimeError("FlatEMA.load_state_dict() inside applied()")
        self.count_dev.fill_(int(sd["updates"]))
        if ema_state_dict is None:
            return
        if model is None:
            raise ValueError("FlatEMA.load_state_dict: the buffer is restored by parameter name and needs the model")
        for k, v, off in self._slices(model):
            if off is not None:
                self.ema[off:off + v.numel()].view(v.shape).copy_(ema_state_dict[k])


def make_flat_optimizer(name, params, lr, weight_decay=0.0, momentum=0.0):
    """the flat optimizer of one --optimizer choice, with the hyperparameters model/plt.py:150-161 passes"""
    name = name.lower()
    if name == "sgd":
        return FlatSGD(params, lr=lr, momentum=momentum)
    if name in ("adam", "adamw"):
        return FlatAdamW(params, lr=lr, weight_decay=weight_decay)
    rules = {"radam": FlatRAdam, "adabelief": FlatAdaBelief, "adabound": FlatAdaBound, "adamp": FlatAdamP,
             "novograd": FlatNovoGrad}
    if name not in rules:
        raise ValueError("unknown optimizer %r (choices: sgd, adam, adamw, %s)" % (name, ", ".join(rules)))
    return rules[name](params, lr=lr, weight_decay=weight_decay)
