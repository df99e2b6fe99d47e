"""Minimal trainer with the part of the PyTorch-Lightning 1.0 ``Trainer`` contract that the reference's main.py uses
(main.py:96-122): fit / test, one process per GPU with SyncBatchNorm when gpus > 1, per-step LR scheduler, validation
every epoch driving ``f1_score`` checkpointing (ModelCheckpoint(monitor="f1_score", mode="max", save_last=True)),
resume.  Checkpoints keep PL's layout ``{"state_dict": ..., "hyper_parameters": {"args": ...}, "epoch": ...}`` with the
reference's key names (``model.unet.enc_l1.0.weight`` ...), so files move between the two code bases.
``precision=16`` (the reference's fp16 AMP) selects XV2_MATH_BF16_STORE: bf16 activations in HBM, bf16 MFMA with fp32
accumulation, fp32 BatchNorm statistics and master weights."""
import gc
import os

import torch

from . import dist as xdist
from .optim import FlatEMA, FlatOptimizer


def _mark_last(loader, wanted):
    """(index, batch, this is the epoch's last batch) - known from len(loader), or by looking one batch ahead where there is
    no len; not wanted (no accumulation): plain enumeration, the mark stays False"""
    if not wanted:
        for i, batch in enumerate(loader):
            yield i, batch, False
        return
    try:
        n = len(loader)
    except TypeError:
        n = None
    if n is not None:
        for i, batch in enumerate(loader):
            yield i, batch, i == n - 1
        return
    it = iter(loader)
    try:
        ahead = next(it)
    except StopIteration:
        return
    i = 0
    for nxt in it:
        yield i, ahead, False
        ahead, i = nxt, i + 1
    yield i, ahead, True


class Trainer:
    def __init__(self, gpus=1, precision=32, max_epochs=1, min_epochs=None, sync_batchnorm=False, accelerator=None,
                 default_root_dir=".", resume_from_checkpoint=None, checkpoint_callback=True, callbacks=None,
                 benchmark=True, deterministic=False, num_sanity_val_steps=0, logger=False, log_every=0,
                 gradient_clip_val=0.0, skip_nonfinite=False, ema_decay=0.0, accumulate_grad_batches=1):
        self.gpus, self.max_epochs, self.root = gpus, max_epochs, default_root_dir
        # PL's gradient_clip_val (global-norm clipping, 0 = off) and the step skipping of its native-AMP GradScaler: the flat
        # optimizer's gradient guard (optim.FlatOptimizer.set_guard).  guard_log: one dict per epoch when a guard is set.
        self.gradient_clip_val, self.skip_nonfinite = float(gradient_clip_val), bool(skip_nonfinite)
        self.guard_log = []
        # > 0: an exponential moving average of the weights (optim.FlatEMA), updated after every optimizer step; validation, the
        # score that selects best.ckpt and the checkpoints' ema_state_dict are taken from it.  0: off, nothing changes.
        self.ema_decay, self.ema = float(ema_decay), None
        # PL's accumulate_grad_batches: K consecutive batches of an epoch form a group whose mean gradient takes ONE optimizer
        # step (optim.FlatOptimizer.accumulate); the epoch's last group may be short and steps with the mean of what it holds.
        # No group spans an epoch, validation or a checkpoint.  1: off, nothing changes.
        k = accumulate_grad_batches
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError("accumulate_grad_batches = %r: must be an integer >= 1" % (k,))
        self.accumulate_grad_batches = k
        self.sync_batchnorm, self.resume = sync_batchnorm, resume_from_checkpoint
        self.checkpointing = bool(checkpoint_callback)
        self.log_every = log_every
        from . import ops
        # the reference's --precision 16 is fp16 autocast (activations and convolutions in half precision, fp32
        # accumulate, fp32 BN statistics / master weights); here the 16-bit type is bf16 (no loss scaling needed)
        ops.MATH_MODE = ops.MATH_BF16 if precision == 16 else ops.fp32_math()
        ops.set_storage_dtype(torch.bfloat16 if precision == 16 else None)
        self.rank, self.local_rank, self.world = xdist.init_from_env()
        self.device = torch.device("cuda", self.local_rank)
        torch.cuda.set_device(self.device)
        self.best_score = None
        self.global_step = 0

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, model, path, epoch, optimizer=None):
        if self.rank != 0:
            return
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        ckpt = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "hyper_parameters": {"args": model.args}, "epoch": epoch, "global_step": self.global_step}
        if isinstance(optimizer, FlatOptimizer):
            ckpt["optimizer_states"] = [{k: (v.cpu() if torch.is_tensor(v) else v)
                                         for k, v in optimizer.state_dict().items()}]
        if self.ema is not None:
            # state_dict stays the live weights (resume continues from them); the averaged ones ride next to it
            ckpt["ema_state_dict"] = {k: v.detach().cpu() for k, v in self.ema.model_state_dict(model).items()}
            ckpt["ema"] = self.ema.state_dict()
        torch.save(ckpt, path)

    # ------------------------------------------------------------------ fit
    def fit(self, model, datamodule):
        model.to(self.device)
        start_epoch, ckpt = 0, None
        # the loader (dataset index, worker pool, sampler) is built once; its length is this rank's steps per epoch
        train_loader = datamodule.train_dataloader()
        K = self.accumulate_grad_batches
        try:
            model.steps_per_epoch_hint = -(-len(train_loader) // K)      # optimizer steps: the schedule's warm-up epochs stay epochs
        except TypeError:
            model.steps_per_epoch_hint = None
        opt_cfg = model.configure_optimizers()
        if isinstance(opt_cfg, dict):
            optimizer, scheduler = opt_cfg["optimizer"], opt_cfg["lr_scheduler"]["scheduler"]
        else:
            optimizer, scheduler = opt_cfg, None
        if self.resume and os.path.exists(self.resume):
            ckpt = torch.load(self.resume, map_location="cpu", weights_only=False)
            model.load_state_dict(ckpt["state_dict"])
            start_epoch = ckpt.get("epoch", -1) + 1
            self.global_step = ckpt.get("global_step", 0)
            if isinstance(optimizer, FlatOptimizer) and ckpt.get("optimizer_states"):
                st = ckpt["optimizer_states"][0]
                optimizer.load_state_dict({k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in st.items()})
            if scheduler is not None:
                # NoamLR counts from 1 (its constructor steps once): after n optimizer steps it stands at n + 1
                scheduler.step(self.global_step + 1)
                if isinstance(optimizer, FlatOptimizer):
                    optimizer.sync_lr()
        flat = isinstance(optimizer, FlatOptimizer)
        guarded = self.gradient_clip_val > 0.0 or self.skip_nonfinite
        if guarded:
            if not flat:
                raise RuntimeError("gradient_clip_val / skip_nonfinite need a flat optimizer (xview2_amd.optim)")
            optimizer.set_guard(self.gradient_clip_val, self.skip_nonfinite)
        if K > 1 and not flat:
            raise RuntimeError("accumulate_grad_batches = %d needs a flat optimizer (xview2_amd.optim)" % K)
        self.ema = None
        if self.ema_decay > 0.0:
            if not flat:
                raise RuntimeError("ema_decay needs a flat optimizer (xview2_amd.optim)")
            # (after a resume has loaded the weights: without an average in the file it starts from them, counter 0)
            self.ema = FlatEMA(optimizer, self.ema_decay)
            if ckpt is not None and "ema" in ckpt and "ema_state_dict" in ckpt:
                self.ema.load_state_dict(ckpt["ema"], ckpt["ema_state_dict"], model)
        ckpt = None
        seen = {"steps": 0, "clipped": 0, "skipped": 0}
        reducer = xdist.GradReducer(optimizer, sync_bn=self.sync_batchnorm or self.world > 1) if flat else None
        frozen = False
        for epoch in range(start_epoch, self.max_epochs):
            model.current_epoch = epoch
            model.train()
            if hasattr(train_loader, "set_epoch"):
                train_loader.set_epoch(epoch)        # DistributedSampler reshuffles per epoch (PL's ddp does this)
            for i, batch, last in _mark_last(train_loader, K > 1):
                closes = K == 1 or last or (i + 1) % K == 0       # this batch ends its group: the optimizer steps
                optimizer.zero_grad()
                if reducer:
                    reducer.prepare(sync=closes)
                loss = model.training_step(batch, i)
                loss.backward()
                if not closes:
                    optimizer.accumulate()
                    continue
                if flat:
                    optimizer.step(reducer.finish())
                    if self.ema is not None:
                        self.ema.update()
                else:
                    optimizer.step()
                if scheduler is not None:
                    scheduler.step()
                self.global_step += 1
                if not frozen:
                    # everything alive after the first step (modules, parameters, packed layouts, the loader's index) is there for the
                    # whole run: park it in the permanent generation so that the cyclic collector's full passes walk only what the
                    # steps create - a full pass over the model's object graph is 10 - 30 ms, more than a bf16 step (bench.quiet_gc)
                    gc.collect()
                    gc.freeze()
                    frozen = True
                if self.log_every and self.rank == 0 and self.global_step % self.log_every == 0:
                    print("epoch %d step %d loss %.5f" % (epoch, self.global_step, float(loss)))
            if flat and optimizer.pending:
                # (a loader that yields fewer batches than its len never shows its last one: no group may outlive the epoch)
                raise RuntimeError("epoch %d ended with %d micro-batches of an open accumulation group: the loader yielded fewer "
                                   "batches than its len()" % (epoch, optimizer.pending))
            xdist.check_peer_exchange()          # one-shot SyncBatchNorm exchange: a timed-out exchange is an error, per epoch
            if guarded:
                self._report_guard(model, optimizer, epoch, seen)
            if self.ema is not None:
                model.epoch_extras = dict(getattr(model, "epoch_extras", None) or {}, ema=True)
                with self.ema.applied():         # f1 / val_loss and the score that selects best.ckpt: the averaged weights'
                    score = self.validate(model, datamodule)
            else:
                score = self.validate(model, datamodule)
            if guarded or self.ema is not None:
                model.epoch_extras = None
            if self.checkpointing:
                ckdir = os.path.join(self.root, "checkpoints")
                self.save_checkpoint(model, os.path.join(ckdir, "last.ckpt"), epoch, optimizer)
                if score is not None and (self.best_score is None or score >= self.best_score):
                    self.best_score = score
                    self.save_checkpoint(model, os.path.join(ckdir, "best.ckpt"), epoch, optimizer)
            if self.world > 1:
                # rank 0 alone wrote the checkpoints: the others wait here instead of inside the next epoch's first SyncBatchNorm
                # exchange (a collective would wait anyway; the one-shot peer exchange has a bounded wait - ADVICE r04)
                import torch.distributed as tdist
                tdist.barrier()
        if self.world > 1:
            xdist.reset_peer_exchange()          # unmap the peers' exchange buffers, free this rank's own
        if frozen:
            gc.unfreeze()
        return model

    def _report_guard(self, model, optimizer, epoch, seen):
        """end of an epoch, where validation synchronises anyway: this epoch's share of the guard's counters, handed to the
        model for the epoch's record (lightning.Model.validation_epoch_end).  Every rank took the same decisions on the same
        reduced gradient, so every rank raises together when the epoch trained nothing."""
        st = optimizer.guard_stats()
        steps, clipped, skipped = (st[k] - seen[k] for k in ("steps", "clipped", "skipped"))
        seen.update((k, st[k]) for k in seen)
        rec = {"grad_norm_max": st["norm_max"], "clipped_steps": clipped, "skipped_steps": skipped}
        self.guard_log.append(dict(rec, epoch=epoch, steps=steps, total=st))
        model.epoch_extras = rec
        if self.rank == 0:
            print("epoch %d gradient guard: largest norm %.6g, %d of %d steps clipped, %d skipped (non-finite gradient)"
                  % (epoch, st["norm_max"], clipped, steps, skipped))
        if steps > 0 and skipped == steps:
            raise RuntimeError("every step of epoch %d was skipped for a non-finite gradient (%d of %d): training is dead"
                               % (epoch, skipped, steps))

    @torch.no_grad()
    def validate(self, model, datamodule):
        model.eval()
        model.on_validation_epoch_start()
        outs = [model.validation_step(b, i) for i, b in enumerate(datamodule.val_dataloader())]
        model.validation_epoch_end(outs)
        score = getattr(model, "logged", {}).get("f1_score")
        return None if score is None else float(score)

    @torch.no_grad()
    def test(self, model, test_dataloaders=None):
        model.to(self.device).eval()
        model.on_test_epoch_start()
        for i, b in enumerate(test_dataloaders):
            model.test_step(b, i)
        model.test_epoch_end(None)
