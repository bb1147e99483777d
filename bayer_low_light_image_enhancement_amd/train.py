"""Training step on the HIP path (SURVEY.md section 8 f3 / BASELINE configs[4]).

Mirrors the reference's loop body (train.py:132-145; RawFomer_WFB_FFAB/train.py:124 for the L1 loss):

    pred = model(inp); loss = criterion(pred, gt); optimizer.zero_grad(); loss.backward(); optimizer.step()

(``Trainer(clamp_pred=True)`` puts the reference's ``pred = torch.clamp(pred, 0, 1)`` of train.py:139 in front of the criterion;
the default evaluates the criterion on the raw prediction) with torch.autograd replaced by the library's explicit adjoint schedule (``rf_train_step``) and ``nn.DataParallel``
(train.py:108-111) by one process per GPU: every rank runs its own images, the flat gradient buffer is all-reduced in
fixed-size buckets (RCCL with the ``nccl`` backend, ``gloo`` in the CPU tests), then ``rf_adam_step`` updates the flat
parameter buffer.  PyTorch provides device memory, streams and the collective; no torch op computes anything.
``Trainer(max_grad_norm=..., skip_nonfinite=True)`` replaces that last call by the guarded step (``rf_grad_stats`` +
``rf_adam_step_guarded``): the reference's ``GradScaler.step`` / ``clip_grad_norm_`` pair, decided on the device.

Around the step, ``fit`` is the reference's epoch loop (train.py:113-175): ``warmup_cosine_lr`` restates the learning rate its
``GradualWarmupScheduler`` + ``CosineAnnealingLR`` pair leaves in the optimiser, batches come from a device-resident set
(``data.PatchSampler``), validation is the uint8 PSNR of the evaluation harness, the best checkpoint has the reference's
``{'epoch', 'state_dict', 'optimizer'}`` layout and the log its line format.
"""
from __future__ import annotations

import math
import os
import random
import time
from typing import Optional

import numpy as np
import torch

from . import _lib
from .model import RawFormer

LOSS_L1, LOSS_CHARBONNIER = 0, 1


def bucket_bounds(n: int, bucket_floats: int):
    """Contiguous [lo, hi) slices of a flat buffer of ``n`` floats, ``bucket_floats`` each (last one shorter)."""
    return [(lo, min(n, lo + bucket_floats)) for lo in range(0, n, bucket_floats)]


def allreduce_flat(flat: torch.Tensor, group=None, bucket_floats: int = 1 << 20):
    """Sum ``flat`` over the ranks in buckets (async, waited at the end).  9.9 MB of RawFormer-S gradients = 3 buckets of
    4 MiB: large enough for xGMI links, small enough that the first bucket is on the wire while the others queue."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    works = [dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True) for lo, hi in bucket_bounds(flat.numel(), bucket_floats)]
    for w in works:
        w.wait()


class OverlappedReducer:
    """All-reduce of the flat gradient buffer OVERLAPPED with the backward pass (the reference reduces inside backward through
    ``nn.DataParallel``, train.py:108-111).  ``rf_train_step`` announces ranges of the flat buffer whose gradients are final, from
    the end of the buffer towards its start (``rf_set_grad_ready``); ``ready`` coalesces them into buckets of at least
    ``bucket_floats`` and starts each bucket's asynchronous all-reduce at once -- with the ``nccl`` backend (RCCL) the collective
    is ordered behind the kernels already enqueued on the current stream and runs beside the rest of the backward pass; ``wait``
    waits for all of them; ``finish`` checks that the whole buffer was announced, then waits.  ``begin`` waits too: a new round
    never starts while the previous one may still write into the buffer.  Works on any tensor / backend (the CPU tests drive it
    with ``gloo``)."""

    def __init__(self, flat: torch.Tensor, group=None, bucket_floats: int = 1 << 20):
        self.flat, self.group, self.bucket_floats = flat, group, int(bucket_floats)
        self.works, self.buckets = [], []
        self.hi = self.lo = flat.numel()

    def begin(self) -> None:
        self.wait()
        self.buckets = []
        self.hi = self.lo = self.flat.numel()

    def ready(self, offset: int, count: int) -> None:
        import torch.distributed as dist
        if offset + count != self.lo:
            raise RuntimeError(f"gradient ranges must arrive contiguously from the end: got [{offset}, {offset + count}), expected to end at {self.lo}")
        self.lo = offset
        if self.hi - self.lo >= self.bucket_floats or self.lo == 0:
            if self.hi > self.lo:
                self.buckets.append((self.lo, self.hi))
                self.works.append(dist.all_reduce(self.flat[self.lo:self.hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            self.hi = self.lo

    def finish(self) -> None:
        if self.lo != 0:
            raise RuntimeError(f"gradient ranges stopped at float {self.lo}: the step did not announce the whole buffer")
        self.wait()

    def wait(self) -> None:
        """Wait for the all-reduces started so far (none: nothing to do)."""
        for w in self.works:
            w.wait()
        self.works = []


class Trainer:
    """Owns the flat parameter / gradient / moment buffers of a ``RawFormer`` and runs training steps on them.

    ``max_grad_norm`` and ``skip_nonfinite`` switch on the GUARDED optimiser step (``rf_grad_stats`` +
    ``rf_adam_step_guarded``), the reference loops' ``GradScaler.step`` (training.py:233,251-253: no step is applied when a
    gradient holds an inf or a NaN) and ``torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)``.  Norm, clip coefficient,
    the decision to skip and the step count behind Adam's bias corrections are computed and kept ON THE DEVICE: a guarded
    ``step`` reads nothing back and copies nothing to the device.  A skipped step leaves parameters and moments bit for bit as
    they were and does not count as a step.  Clipping is applied on the way into the update: ``grads`` / ``grad_of`` keep the
    unclipped gradient.  The decision is taken on the ALL-REDUCED buffer, which every rank holds bit for bit the same (one
    collective result, the same kernels in the same fixed summation order), with ``grad_scale = 1 / world``: the ranks decide
    alike and their weights cannot drift apart.  With both arguments left at their defaults ``optimizer_step`` is the plain
    ``rf_adam_step`` and ``step_no`` a host integer."""

    def __init__(self, model: RawFormer, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False, loss: str = "l1", charbonnier_eps: float = 1e-3, group=None, overlap_allreduce: bool = True,
                 bucket_floats: int = 1 << 20, clamp_pred: bool = False, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False):
        if model.variant not in ("plain", "flca"):
            raise RuntimeError(f"Trainer: the adjoint schedule exists for variants 'plain' and 'flca', not {model.variant!r}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("Trainer needs the model on a ROCm device: there is no CPU path in this package")
        self.model, self.group = model, group
        self.lr, self.betas, self.eps, self.wd, self.decoupled = float(lr), betas, float(eps), float(weight_decay), bool(decoupled)
        self.loss_mode = {"l1": LOSS_L1, "charbonnier": LOSS_CHARBONNIER}[loss]
        self.loss_eps = float(charbonnier_eps)
        self.clamp_pred = bool(clamp_pred)       # the criterion sees clamp(pred, 0, 1): train.py:139
        self.state = model._state_for(dev)
        self.n = _lib.size("rf_flat_param_floats", self.state.handle)
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=dev)
        params = dict(model.named_parameters())
        self.slices = {}
        with torch.no_grad():
            for i, k in enumerate(model._param_names):
                off = _lib.size("rf_flat_offset", self.state.handle, i)
                p = params[k]
                view = self.flat[off: off + p.numel()].view(p.shape)
                view.copy_(p)
                p.data = view                       # the module's parameters ARE the flat buffer from now on
                self.slices[k] = (off, p.numel())
        self.grads = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self._step_no = 0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        if self.guarded:
            # the registry's parameters as segments of the flat buffer (offsets 16-byte aligned, gaps of up to 3 floats that belong
            # to no segment); tables and counters go to the device once, here
            self._segments = sorted((off, cnt, k) for k, (off, cnt) in self.slices.items())
            nseg = len(self._segments)
            self.opt_state = torch.zeros(_lib.size("rf_optim_state_bytes", nseg, self.n), dtype=torch.uint8, device=dev)
            as_size_t = _lib.C.c_size_t * nseg
            _lib.launch("rf_optim_init", self.flat, as_size_t(*[s[0] for s in self._segments]), as_size_t(*[s[1] for s in self._segments]),
                        nseg, self.n, self.opt_state, self.opt_state.numel())
            self._grad_scale = 1.0
        self.workspace: Optional[torch.Tensor] = None
        self.loss_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        # gradient all-reduce started range by range from inside rf_train_step (several ranks only)
        self.overlap = bool(overlap_allreduce)
        self.overlap_always = overlap_allreduce == "always"      # also with a world of one (tests of the RCCL stream ordering)
        self.reducer = OverlappedReducer(self.grads, group, bucket_floats)
        self._reduced = False
        self._ready_cb = _lib.GRAD_READY_FN(lambda user, off, cnt, stream: self.reducer.ready(int(off), int(cnt)))   # kept alive with the Trainer
        model.invalidate_packed()

    def grad_of(self, key: str) -> torch.Tensor:
        """View of ``key``'s gradient in ``self.grads``: this rank's local gradient on the serial path (until ``optimizer_step``
        all-reduces it), the sum over the ranks after an overlapped step.  An all-reduce still in flight is waited first."""
        self.reducer.wait()
        off, n = self.slices[key]
        return self.grads[off: off + n].view(dict(self.model.named_parameters())[key].shape)

    def forward_backward(self, x: torch.Tensor, gt: torch.Tensor, want_pred: bool = False, loss_out: Optional[torch.Tensor] = None):
        """Loss (device scalar; written into ``loss_out``, one float32 on the device, when given) and, in ``self.grads``, this
        rank's gradient of the mean loss over ITS images."""
        x, gt = x.detach().float().contiguous(), gt.detach().float().contiguous()
        b, c, h, w = x.shape
        if c != 1 or h % 16 or w % 64:
            raise RuntimeError(f"training step: mosaic [B,1,H,W] with H % 16 == 0 and W % 64 == 0, got {tuple(x.shape)}")
        if tuple(gt.shape) != (b, self.model.out_channels, h, w):
            raise RuntimeError(f"ground truth must be {(b, self.model.out_channels, h, w)}, got {tuple(gt.shape)}")
        H, W = h // 2, w // 2
        with torch.cuda.device(x.device):
            self.model._sync_params(self.state, x.device, pack=False)   # the (flat-buffer) pointers, once: rf_train_step reads raw weights
            need = _lib.size("rf_train_workspace_bytes", self.state.handle, b, H, W)
            if self.workspace is None or self.workspace.numel() < need:
                self.workspace = None
                self.workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
            pred = torch.empty_like(gt) if want_pred else None
            import torch.distributed as dist
            overlapped = self.overlap and dist.is_initialized() and (dist.get_world_size(self.group) > 1 or self.overlap_always)
            _lib.call("rf_set_grad_ready", self.state.handle, self._ready_cb if overlapped else _lib.GRAD_READY_FN(), None)
            self.reducer.begin()                # waits for a previous round's all-reduces: they write into self.grads
            _lib.call("rf_set_loss_clamp", self.state.handle, int(self.clamp_pred))
            loss_dev = self.loss_dev if loss_out is None else loss_out
            if loss_dev.dtype != torch.float32 or loss_dev.numel() != 1 or loss_dev.device != x.device:
                raise RuntimeError("loss_out must be one float32 on the input's device")
            _lib.launch("rf_train_step", x, self.state.handle, x, gt, self.grads, loss_dev, pred, self.workspace, self.workspace.numel(),
                        b, H, W, self.loss_mode, self.loss_eps)
            self._reduced = overlapped          # the buckets are on the wire (or done); optimizer_step waits for them
        return (loss_dev, pred) if want_pred else loss_dev

    def optimizer_step(self):
        import torch.distributed as dist
        world = dist.get_world_size(self.group) if dist.is_initialized() else 1
        if self._reduced:
            self.reducer.finish()
            self._reduced = False
        else:
            allreduce_flat(self.grads, self.group)
        if self.guarded:
            # statistics -> control -> Adam on the current stream, behind the all-reduce it has just been made to wait for
            nseg, nbytes = len(self._segments), self.opt_state.numel()
            self._grad_scale = 1.0 / world
            _lib.launch("rf_grad_stats", self.flat, self.grads, self.n, nseg, self.opt_state, nbytes)
            _lib.launch("rf_adam_step_guarded", self.flat, self.flat, self.grads, self.m, self.v, self.n, self.lr, self.betas[0], self.betas[1],
                        self.eps, self.wd, int(self.decoupled), self._grad_scale, math.inf if self.max_grad_norm is None else self.max_grad_norm,
                        int(self.skip_nonfinite), nseg, self.opt_state, nbytes)
        else:
            self._step_no += 1
            _lib.launch("rf_adam_step", self.flat, self.flat, self.grads, self.m, self.v, self.n, self.lr, self.betas[0], self.betas[1], self.eps,
                        self.wd, int(self.decoupled), self._step_no, 1.0 / world)
        self.model.invalidate_packed()          # the weights moved: packed copies are stale

    @property
    def step_no(self) -> int:
        """Optimiser steps applied so far.  Default mode: a host integer.  Guarded mode: the device's ``steps_applied`` (skipped
        steps do not count), read with one SYNCHRONISING copy.  Setting it (``load_optimizer_state_dict`` does) also sets the
        device counter, on the current stream."""
        return int(self._control()["steps_applied"]) if self.guarded else self._step_no

    @step_no.setter
    def step_no(self, value: int) -> None:
        self._step_no = int(value)
        if self.guarded:
            _lib.launch("rf_optim_set_steps", self.flat, self.opt_state, self.opt_state.numel(), self._step_no)

    def _control(self, raw: Optional[bytes] = None):
        """``rf_optim_control`` as a numpy record; read from the device (synchronising) unless its bytes are given."""
        if raw is None:
            raw = self.opt_state[:_lib.OPTIM_CONTROL_BYTES].cpu().numpy().tobytes()
        return np.frombuffer(raw, dtype=np.dtype(_lib.OPTIM_CONTROL))[0]

    def _need_guarded(self, what: str) -> None:
        if not self.guarded:
            raise RuntimeError(f"{what}: this Trainer runs the plain optimiser step; pass max_grad_norm and / or skip_nonfinite=True")

    def optimizer_stats(self, raw: Optional[bytes] = None) -> dict:
        """Guarded mode: the counters and the last step's decision, read from the device with one SYNCHRONISING copy:
        ``steps_applied``, ``steps_skipped``, ``grad_norm`` (float64 norm of the all-reduced gradient times 1 / world, before
        clipping), ``clip_coef`` (``min(1, max_grad_norm / (grad_norm + 1e-6))``, 1 without clipping), ``nonfinite`` (inf / NaN
        elements of the gradient)."""
        self._need_guarded("optimizer_stats")
        c = self._control(raw)
        return {"steps_applied": int(c["steps_applied"]), "steps_skipped": int(c["steps_skipped"]), "grad_norm": float(c["grad_norm"]),
                "clip_coef": float(c["clip_coef"]), "nonfinite": int(c["nonfinite"])}

    def grad_norms(self) -> dict:
        """Guarded mode: ``{parameter name: (norm, non-finite count)}`` of the last step's gradient, the per-parameter NaN monitor the
        reference keeps commented out (RawFomer_WFB_FFAB/train.py:185-188).  Norms are float64, scaled like ``grad_norm``.  One
        SYNCHRONISING copy."""
        self._need_guarded("grad_norms")
        lo, nseg = _lib.OPTIM_CONTROL_BYTES, len(self._segments)
        seg = np.frombuffer(self.opt_state[lo: lo + 16 * nseg].cpu().numpy().tobytes(), dtype=np.dtype(_lib.OPTIM_SEGMENT))
        return {k: (self._grad_scale * math.sqrt(float(seg[i]["sumsq"])), int(seg[i]["nonfinite"])) for i, (_, _, k) in enumerate(self._segments)}

    def step(self, x: torch.Tensor, gt: torch.Tensor, loss_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        loss = self.forward_backward(x, gt, loss_out=loss_out)
        self.optimizer_step()
        return loss

    def optimizer_state_dict(self) -> dict:
        """``torch.optim.Adam(model.parameters()).state_dict()`` of this trainer: ``state[i] = {step, exp_avg, exp_avg_sq}`` in
        ``model.parameters()`` order (host copies of the parameter's slices of the flat moment buffers) and one parameter group."""
        step = torch.tensor(float(self.step_no))
        state = {}
        for i, (k, p) in enumerate(self.model.named_parameters()):
            off, n = self.slices[k]
            state[i] = {"step": step.clone(), "exp_avg": self.m[off: off + n].view(p.shape).cpu(), "exp_avg_sq": self.v[off: off + n].view(p.shape).cpu()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": self.decoupled,
                 "params": list(range(len(state)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """Resume from ``optimizer_state_dict()`` or from a real ``torch.optim.Adam.state_dict()`` over the same model."""
        names = [k for k, _ in self.model.named_parameters()]
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(names):
            raise RuntimeError(f"optimizer state: expected one parameter group of {len(names)} tensors")
        if groups[0].get("amsgrad"):
            raise RuntimeError("optimizer state: amsgrad has no counterpart in rf_adam_step")
        g = groups[0]
        self.lr, self.betas, self.eps, self.wd = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"])
        self.decoupled = bool(g.get("decoupled_weight_decay", self.decoupled))
        state, steps = sd["state"], set()
        self.m.zero_()
        self.v.zero_()
        for i, pid in enumerate(g["params"]):
            st = state.get(pid)
            if st is None:                     # torch creates a tensor's state at its first step
                continue
            off, n = self.slices[names[i]]
            for buf, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq")):
                t = st[key]
                if t.numel() != n:
                    raise RuntimeError(f"optimizer state: {key} of '{names[i]}' has {t.numel()} elements, expected {n}")
                buf[off: off + n].copy_(t.reshape(-1))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise RuntimeError(f"optimizer state: the tensors disagree on the step count ({sorted(steps)})")
        self.step_no = steps.pop() if steps else 0


def warmup_cosine_lr(epoch: int, base_lr: float = 1e-4, epochs: int = 3000, warmup: int = 20, eta_min: float = 1e-5) -> float:
    """The learning rate the reference's optimiser holds DURING epoch ``epoch`` (train.py:113-115, ``scheduler.step()`` at the
    end of every epoch, :147): ``CosineAnnealingLR(optimizer, epochs, eta_min)`` behind ``GradualWarmupScheduler(multiplier=1,
    total_epoch=warmup)``.  What that pair does, not a textbook schedule:

    * epochs 0..warmup ramp ``base_lr * epoch / warmup``: epoch 0 trains at 0.0 and epoch ``warmup`` at ``base_lr``;
    * epoch ``warmup + 1`` is the hand-over: the cosine scheduler, which has never stepped, is asked for its value at ITS epoch 0
      and applies its recursive update ``(1 + cos(pi t / T)) / (1 + cos(pi (t - 1) / T))`` with t = 0 to the rate in the
      optimiser, ``base_lr``: the rate rises ABOVE ``base_lr``, by the factor ``2 / (1 + cos(pi / T))`` on its part over ``eta_min``;
    * the next epoch undoes that (``base_lr`` again) and from there the recursion telescopes: epoch ``e`` has
      ``eta_min + (base_lr - eta_min) (1 + cos(pi t / T)) / (1 + cos(pi / T))`` with ``t = e - warmup - 1``: the cosine runs from
      its own epoch 0 over ``T = epochs`` (not ``epochs - warmup``), one epoch late and scaled by that factor, so the last epoch
      is still well above ``eta_min``.

    The values were read from the real optimiser (tests/golden/lr_schedule.json); the reference's recursion and this closed form
    differ by rounding only."""
    if epoch <= warmup:
        return base_lr * (float(epoch) / warmup)
    t = epoch - warmup - 1
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * t / epochs)) / (1.0 + math.cos(math.pi / epochs))


def validate(model: RawFormer, val_sampler) -> float:
    """Mean uint8 PSNR (data range 255) of the whole validation frames, one frame at a time (train.py:150-164)."""
    from . import harness
    was_training = model.training
    model.eval()
    psnr_val_rgb = []
    try:
        with torch.no_grad():
            for idx in range(len(val_sampler.dataset)):
                x, gt = val_sampler.whole([idx])
                psnr_val_rgb.extend(float(v) for v in harness.psnr_u8(harness.to_uint8_hwc(gt), harness.to_uint8_hwc(model(x))))
    finally:
        model.train(was_training)
    return float(np.mean(psnr_val_rgb))


def fit(trainer: Trainer, sampler, val_sampler, epochs: int, batch_size: int, out_dir: str, start_epoch: int = 0, shuffle_seed=None, *,
        base_lr: Optional[float] = None, warmup: int = 20, eta_min: float = 1e-5, log_name: str = "train_log.txt"):
    """The reference's epoch loop (train.py:127-176) on ``Trainer.step``.  Epochs ``start_epoch .. epochs`` INCLUSIVE, as there
    (``range(start_epoch, epochs + 1)``).  Per epoch: the learning rate of ``warmup_cosine_lr`` (``base_lr``: the trainer's rate
    at the call), one pass over a shuffled index list in batches of ``batch_size`` (the last one shorter, ``DataLoader``'s
    default), the sum of the batch losses read from the device ONCE, validation (``validate``), ``model_best.pth`` =
    ``{'epoch', 'state_dict', 'optimizer'}`` in ``out_dir`` on a new best PSNR (:165-172; host tensors) and one line of :175's
    format appended to ``out_dir/log_name``.  No progress bar, no image writing.  To resume, load a checkpoint's ``state_dict``
    into the model and its ``optimizer`` with ``Trainer.load_optimizer_state_dict``, then pass ``start_epoch = epoch + 1``.
    Returns one dict per epoch: ``epoch``, ``lr``, ``loss``, ``psnr``, ``best_psnr``, ``best_epoch``; with a guarded trainer
    (``Trainer(max_grad_norm=..., skip_nonfinite=...)``) also ``skipped``, the steps of this epoch that were not applied, and
    ``grad_norm``, the gradient norm of its last step -- the control block is read in the epoch's one host read.  The loss of a
    skipped step still enters the epoch's sum, as in the reference, so one NaN batch makes that epoch's logged loss NaN while
    the weights stay clean."""
    model = trainer.model
    os.makedirs(out_dir, exist_ok=True)
    base_lr = trainer.lr if base_lr is None else float(base_lr)
    order_rng = random.Random(shuffle_seed)
    n = len(sampler.dataset)
    steps = (n + batch_size - 1) // batch_size
    losses = torch.zeros(steps, dtype=torch.float32, device=trainer.flat.device)
    best_psnr, best_epoch, history = 0, 0, []
    skipped_before = trainer.optimizer_stats()["steps_skipped"] if trainer.guarded else 0      # one read before the first epoch
    with open(os.path.join(out_dir, log_name), "a") as log_f:
        for epoch in range(start_epoch, epochs + 1):
            start_time = time.time()
            model.train()
            trainer.lr = warmup_cosine_lr(epoch, base_lr, epochs, warmup, eta_min)
            order = list(range(n))
            order_rng.shuffle(order)
            for k in range(steps):
                x, gt = sampler.batch(order[k * batch_size: (k + 1) * batch_size])
                trainer.step(x, gt, loss_out=losses[k: k + 1])
            epoch_loss = 0
            if trainer.guarded:                      # the control block rides along in the epoch's one host read
                ctl_bytes = trainer.opt_state[:_lib.OPTIM_CONTROL_BYTES]
                host = torch.cat([losses.view(torch.uint8), ctl_bytes]).cpu()
                epoch_losses = host[:4 * steps].view(torch.float32).tolist()
                stats = trainer.optimizer_stats(host[4 * steps:].numpy().tobytes())
            else:
                epoch_losses, stats = losses.cpu().tolist(), None
            for v in epoch_losses:                   # the epoch's one host read; added in step order, as `+= loss.item()`
                epoch_loss += v
            avg_psnr = validate(model, val_sampler)
            if avg_psnr > best_psnr:
                best_psnr, best_epoch = avg_psnr, epoch
                torch.save({"epoch": epoch, "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                            "optimizer": trainer.optimizer_state_dict()}, os.path.join(out_dir, "model_best.pth"))
            epoch_time = time.time() - start_time
            log_f.write(f"Epoch {epoch}/{epochs} | Time: {epoch_time:.2f}s | Loss: {epoch_loss:.4f} | Avg PSNR: {avg_psnr:.4f} | Best PSNR: {best_psnr:.4f} (Epoch {best_epoch})\n")
            log_f.flush()
            history.append({"epoch": epoch, "lr": trainer.lr, "loss": epoch_loss, "psnr": avg_psnr, "best_psnr": best_psnr, "best_epoch": best_epoch})
            if stats is not None:
                history[-1].update(skipped=stats["steps_skipped"] - skipped_before, grad_norm=stats["grad_norm"])
                skipped_before = stats["steps_skipped"]
    return history
