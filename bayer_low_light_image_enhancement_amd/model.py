"""Drop-in ``RawFormer(nn.Module)`` whose ``forward`` runs on hand-written gfx950 kernels.

Interface kept from the reference:

* constructor ``RawFormer(inp_channels=1, out_channels=3, dim=48, num_heads=[8,8,8,8],
  ffn_expansion_factor=2)`` -- RawFomer_WFB_FFAB/model.py:448,
  FrequencyawareLumaChromaAttentionRAWFormer.py:296 (root ``model.py:111`` spells the same
  arguments ``in_ch, out_ch, dim, heads, ffn_exp``; those keywords are accepted too);
* ``state_dict()`` / ``load_state_dict(strict=True)`` with the reference's key names (the
  ``module.`` prefix left by ``nn.DataParallel`` is stripped, test.py:90);
* ``forward(x[B,1,2H,2W]) -> [B,3,2H,2W]`` float32, input not modified (test.py:116).

``variant='flca'`` is the wiring of FrequencyawareLumaChromaAttentionRAWFormer.py:284-370;
``variant='truecolor'`` is ``TrueColorRawFormer`` (BayerTORGBColorMultiLvl.py:387-462: learned Bayer
front end, colour-aware pyramid FLCA, ``exp(log_temperature)`` attention, colour-correction head;
``flca_levels`` as in its constructor); ``variant='plain'`` replaces the FLCA
branch by the 3x3 conv branch of RawFomer_WFB_FFAB/model.py:393-412 (``branch_lrelu=True``)
or model.py:94-108 (``False``) and, with ``clamp_io=True``, adds the I/O clamps of
RawFomer_WFB_FFAB/model.py:475,508.  ``variant='multilvl'`` is the ``RawFormer`` of
MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:313-416 (``FLCA_Pyramid`` branches with ``flca_levels`` pyramid
levels, per-channel colour anchor and luminance nudge on the output); forward and evaluation only.
``variant='wfb'`` is the whole ``RawFormer`` of RawFomer_WFB_FFAB/model.py:437-508: the plain stage wiring (conv branch with
LeakyReLU, I/O clamps) around a ``WMB`` block per stage (LayerNorm, Haar DWT, ``Illumination_Estimator`` + ``FFAB`` on the LL band,
``WM`` / Mamba on the high bands, IWT, gated ``FeedForward`` with BatchNorm); eval mode, forward and evaluation only.

The module owns ordinary ``nn.Parameter`` objects; the HIP library borrows their device
pointers.  There is no PyTorch fallback: on a CPU tensor ``forward`` raises.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib

_ROOT_STAGE_ALIASES = (
    ("transformer.norm1.norm.", "Transformer.norm1.body."),
    ("transformer.norm2.norm.", "Transformer.norm2.body."),
    ("transformer.attn.scale", "Transformer.attn.temperature"),
    ("transformer.attn.qkv.0.", "Transformer.attn.qkv."),
    ("transformer.attn.qkv.1.", "Transformer.attn.qkv_dwconv."),
    ("transformer.attn.proj.", "Transformer.attn.project_out."),
    ("transformer.ffn.net.0.", "Transformer.ffn.pointwise1."),
    ("transformer.ffn.net.1.", "Transformer.ffn.depthwise."),
    ("transformer.ffn.net.3.", "Transformer.ffn.pointwise2."),
    ("reduce.", "channel_reduce."),
    ("out.0.", "Conv_out."),
    ("conv.", "conv."),
)


def canonical_key(key: str) -> str:
    """Map a checkpoint key to this module's naming: strips ``module.`` (test.py:90) and
    translates the root ``model.py`` layout to the
    RawFomer_WFB_FFAB / FrequencyawareLumaChroma layout."""
    if key.startswith("module."):
        key = key[len("module."):]
    head, _, rest = key.partition(".")
    stage = None
    if head == "embed":
        return "embedding." + rest
    if head == "output" and rest.startswith("0."):
        return "conv_out." + rest[2:]
    if head == "encoder":
        i, _, rest = rest.partition(".")
        stage = f"conv_tran{int(i) + 1}."
    elif head == "bottleneck":
        stage = "conv_tran4."
    elif head == "decoder":
        i, _, rest = rest.partition(".")
        stage = f"conv_tran{int(i) + 5}."
    elif head == "downsamples":
        i, _, rest = rest.partition(".")
        return f"down{int(i) + 1}.body.0." + rest[len("net.0."):] if rest.startswith("net.0.") else key
    elif head == "upsamples":
        i, _, rest = rest.partition(".")
        return f"up{int(i) + 1}." + rest
    if stage is None:
        return key
    for a, b in _ROOT_STAGE_ALIASES:
        if rest.startswith(a):
            return stage + b + rest[len(a):]
    return stage + rest


_VARIANTS = {"flca": _lib.RF_VARIANT_FLCA, "plain": _lib.RF_VARIANT_PLAIN, "truecolor": _lib.RF_VARIANT_TRUECOLOR,
             "multilvl": _lib.RF_VARIANT_MULTILVL, "wfb": _lib.RF_VARIANT_WFB}


class _Node(nn.Module):
    """Name-only container so parameters get the reference's dotted state_dict keys."""

    def forward(self, *a, **k):  # pragma: no cover - never called
        raise RuntimeError("container module; call RawFormer.forward")


class _DeviceState:
    def __init__(self):
        self.handle = C.c_void_p()
        self.signature = None
        self.ptrs = None          # data_ptr of every parameter as registered with the handle
        self.packed: Optional[torch.Tensor] = None
        self.workspace: Optional[torch.Tensor] = None


class RawFormer(nn.Module):
    def __init__(self, inp_channels: int = 1, out_channels: int = 3, dim: int = 48,
                 num_heads: Sequence[int] = (8, 8, 8, 8), ffn_expansion_factor: int = 2, *,
                 variant: str = "flca", branch_lrelu: bool = True, clamp_io: Optional[bool] = None, flca_levels: int = 2,
                 in_ch: Optional[int] = None, out_ch: Optional[int] = None,
                 heads: Optional[Sequence[int]] = None, ffn_exp: Optional[int] = None):
        super().__init__()
        inp_channels = in_ch if in_ch is not None else inp_channels
        out_channels = out_ch if out_ch is not None else out_channels
        num_heads = list(heads if heads is not None else num_heads)
        ffn_expansion_factor = ffn_exp if ffn_exp is not None else ffn_expansion_factor
        if variant not in _VARIANTS:
            raise ValueError(f"variant must be 'flca', 'plain', 'truecolor', 'multilvl' or 'wfb', got {variant!r}")
        if len(num_heads) != 4:
            raise ValueError("num_heads must have 4 entries")
        if variant == "wfb":
            # the reference model clamps its input and output and applies the LeakyReLU unconditionally (model.py:428,475,508)
            if clamp_io is False or not branch_lrelu:
                raise ValueError("variant='wfb' always applies the input / output clamps and the LeakyReLU on the conv branch: "
                                 "clamp_io=False and branch_lrelu=False are not available")
            if int(ffn_expansion_factor) != ffn_expansion_factor:
                raise ValueError(f"variant='wfb': ffn_expansion_factor must be a whole number, got {ffn_expansion_factor!r}")
            clamp_io = True
        clamp_io = bool(clamp_io)
        self.dim, self.inp_channels, self.out_channels = int(dim), int(inp_channels), int(out_channels)
        self.num_heads, self.ffn_expansion_factor = [int(h) for h in num_heads], int(ffn_expansion_factor)
        self.variant, self.branch_lrelu, self.clamp_io = variant, bool(branch_lrelu), bool(clamp_io)
        self.flca_levels = int(flca_levels)

        cfg = self._config()
        lib = _lib.load()
        probe = C.c_void_p()
        _lib.call("rf_create", C.byref(cfg), C.byref(probe))
        try:
            # _param_names: every tensor the handle borrows (parameters and, for 'wfb', the BatchNorm statistics, which are
            # module buffers); entries the reference registers and its forward never reads stay out of it
            self._param_names: List[str] = []
            self._buffer_names: List[str] = []
            name, shape, ndim, flags = C.c_char_p(), (C.c_int64 * 4)(), C.c_int(), C.c_int()
            for i in range(lib.rf_param_count(probe)):
                _lib.call("rf_param_info", probe, i, C.byref(name), C.byref(shape), C.byref(ndim))
                _lib.call("rf_param_flags", probe, i, C.byref(flags))
                key, shp = name.value.decode(), tuple(shape[: ndim.value])
                if flags.value & _lib.RF_PARAM_BUFFER:
                    self._param_names.append(key)
                    self._buffer_names.append(key)
                    self._register_buffer(key, torch.ones(shp) if key.endswith("running_var") else torch.zeros(shp))
                    if key.endswith("running_var"):      # nn.BatchNorm2d's third buffer follows it in the state_dict
                        self._register_buffer(key[: -len("running_var")] + "num_batches_tracked", torch.tensor(0, dtype=torch.int64))
                    continue
                if not flags.value & _lib.RF_PARAM_UNUSED:
                    self._param_names.append(key)
                self._register(key, nn.Parameter(torch.empty(shp, dtype=torch.float32)))
        finally:
            lib.rf_destroy(probe)
        if variant in ("flca", "truecolor", "multilvl"):
            # fixed buffers the reference keeps in its state_dict (values are constants in the kernels)
            if variant in ("flca", "multilvl"):
                for k, v in (("r_w", 0.299), ("g_w", 0.587), ("b_w", 0.114)):
                    self._register_buffer("luma_chroma." + k, torch.tensor(v, dtype=torch.float32))
            else:
                self._register_buffer("bayer_processor.y_weights", torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float32))
            hv = torch.tensor([1.0, 1.0]) / math.sqrt(2.0)
            gv = torch.tensor([1.0, -1.0]) / math.sqrt(2.0)
            filt = torch.stack([torch.outer(hv, hv), torch.outer(hv, gv), torch.outer(gv, hv), torch.outer(gv, gv)]).unsqueeze(1)
            for i in range(1, 8):
                self._register_buffer(f"conv_tran{i}.FLCA.dwt.filt", filt.clone())
            if variant == "multilvl":
                self._register_buffer("haar.filt", filt.clone())
        self.reset_parameters()
        self._rt: Dict[int, _DeviceState] = {}
        self._rt_lock = threading.Lock()
        self._rt_owner = id(self)   # shallow copies (module.__dict__ copies) share _rt; only the owner frees the handles

    # ------------------------------------------------------------------ construction helpers
    def _config(self) -> _lib.RfConfig:
        return _lib.RfConfig(self.dim, (C.c_int32 * 4)(*self.num_heads), self.inp_channels, self.out_channels,
                             self.ffn_expansion_factor,
                             _VARIANTS[self.variant],
                             int(self.branch_lrelu), int(self.clamp_io), self.flca_levels)

    def _node(self, path: List[str]) -> nn.Module:
        mod: nn.Module = self
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, _Node())
            mod = mod._modules[part]
        return mod

    def _register(self, key: str, p: nn.Parameter) -> None:
        *path, leaf = key.split(".")
        self._node(path).register_parameter(leaf, p)

    def _register_buffer(self, key: str, t: torch.Tensor) -> None:
        *path, leaf = key.split(".")
        self._node(path).register_buffer(leaf, t)

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """PyTorch's default initialisers (what the reference's ``__init__`` leaves behind)."""
        params = dict(self.named_parameters())
        for key, p in params.items():
            leaf = key.rsplit(".", 1)[-1]
            if leaf in ("alpha", "beta", "gamma", "temperature"):
                p.fill_(1.0)
            elif leaf == "log_temperature":                    # TrueColorRawFormer's own initial values
                p.zero_()                                      # (BayerTORGBColorMultiLvl.py:78-83, 144, 331)
            elif leaf == "wb_gains":
                p.copy_(torch.tensor([1.8, 1.0, 1.0, 1.6]))
            elif leaf == "color_matrix":
                p.copy_(torch.eye(3, 4))
            elif leaf == "gamma_param":
                p.fill_(2.2)
            elif leaf == "A_log":                              # mamba_ssm's initial values: A = 1 .. d_state per row, D = 1
                p.copy_(torch.log(torch.arange(1, p.shape[1] + 1, dtype=torch.float32)).repeat(p.shape[0], 1))
            elif leaf == "D":
                p.fill_(1.0)
            elif key.endswith((".bn.bias", ".ln.bias")):       # BatchNorm2d / nn.LayerNorm shifts
                p.zero_()
            elif p.dim() == 1:
                if leaf == "weight":
                    p.fill_(1.0)                      # LayerNorm scale
                elif "norm" in key:
                    p.zero_()                          # LayerNorm shift
                else:                                  # conv bias: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                    w = params[key[: -len("bias")] + "weight"]
                    fan_in = w[0].numel()              # also what torch uses for ConvTranspose2d [Cin,Cout,2,2]
                    bound = 1.0 / math.sqrt(max(fan_in, 1))
                    p.uniform_(-bound, bound)
            else:
                nn.init.kaiming_uniform_(p, a=math.sqrt(5))

    # ------------------------------------------------------------------ state_dict compatibility
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix == "":
            for k in list(state_dict.keys()):
                ck = canonical_key(k)
                if ck != k:
                    state_dict[ck] = state_dict.pop(k)
            # temperature may arrive as [1,heads,1,1] (root model.py `scale`)
            for k, v in list(state_dict.items()):
                if k.endswith("attn.temperature") and v.dim() == 4:
                    state_dict[k] = v.reshape(v.shape[1], 1, 1)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ------------------------------------------------------------------ runtime
    def _state_for(self, device: torch.device) -> _DeviceState:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._rt_lock:
            st = self._rt.get(idx)
            if st is None:
                st = _DeviceState()
                cfg = self._config()
                _lib.call("rf_create", C.byref(cfg), C.byref(st.handle))
                self._rt[idx] = st
        return st

    def _state_with_workspace(self, device: torch.device, b: int, H: int, W: int, sync: bool = True) -> _DeviceState:
        """The device state with a workspace large enough for ``(b, H, W)``: kept while it is, dropped before a larger one is
        allocated.  ``sync``: register (and repack) the parameters first; ``forward_window`` leaves that to ``_run``."""
        st = self._state_for(device)
        if sync:
            self._sync_params(st, device)
        need = _lib.size("rf_workspace_bytes", st.handle, b, H, W)
        if st.workspace is None or st.workspace.numel() < need:
            st.workspace = None
            st.workspace = torch.empty(need, dtype=torch.uint8, device=device)
        return st

    @staticmethod
    def _refuse_host_tensor(t: torch.Tensor) -> None:
        if t.device.type != "cuda":
            raise RuntimeError("RawFormer (HIP) needs a ROCm device tensor: there is no CPU path in this package "
                               f"(input is on {t.device})")

    def invalidate_packed(self) -> None:
        """Force the next ``forward`` to re-register and repack the weights.

        The repack check compares ``(data_ptr, _version)`` of every parameter.  ``_version`` does not move for writes
        through ``p.data`` (``p.data.copy_()`` / ``p.data.add_()``: EMA weight swaps, manual initialisation), so after such
        a write call this method -- ``load_state_dict``, ``.to()``, optimiser steps and ``torch.no_grad()`` in-place
        updates are detected without it."""
        for st in self._rt.values():
            st.signature = None

    # The runtime state (library handles, packed weights, workspace, lock) is per process and per device: it is dropped
    # by copy.deepcopy / pickle / torch.save(model) and rebuilt lazily by the first forward of the copy.
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_rt"] = {}
        state["_rt_lock"] = None
        state["_rt_owner"] = None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._rt = {}
        self._rt_lock = threading.Lock()
        self._rt_owner = id(self)

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return new

    def _sync_params(self, st: _DeviceState, device: torch.device, pack: bool = True) -> None:
        """Register the parameter pointers with the handle and (``pack=True``, the inference forward) repack the weights when
        any of them changed.  ``pack=False`` is the training step's call: ``rf_train_step`` reads the raw weights, so it only
        needs the pointers -- registered once as long as they do not move -- and leaves the packed copies stale (the next
        inference forward repacks: ``signature`` stays ``None``)."""
        params = dict(self.named_parameters())
        if self._buffer_names:      # 'wfb': the BatchNorm running statistics take part in the fold, so also in the signature
            buffers = dict(self.named_buffers())
            params.update({k: buffers[k] for k in self._buffer_names if k in buffers})
        if len(params) < len(self._param_names):
            # nn.DataParallel replicas carry their weights as plain tensors, not Parameters (train.py:108-111 is the
            # reference's only multi-device construct); this package shards across PROCESSES instead (tiling.py)
            raise RuntimeError("RawFormer (HIP) cannot run as an nn.DataParallel replica: use one process per GPU "
                               "(bayer_low_light_image_enhancement_amd.tiling / torch.distributed)")
        sig = tuple((p.data_ptr(), p._version) for p in (params[k] for k in self._param_names))
        ptrs = tuple(s[0] for s in sig)
        if sig == st.signature or (not pack and ptrs == st.ptrs):
            return
        for k in self._param_names:
            p = params[k]
            if p.device != device:
                raise RuntimeError(f"parameter {k} is on {p.device} but the input is on {device}; call model.to(device)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"parameter {k} must be contiguous float32")
            shape = (C.c_int64 * max(p.dim(), 1))(*p.shape)
            _lib.call("rf_set_param", st.handle, k.encode(), p.data_ptr(), shape, p.dim())
        st.ptrs = ptrs
        if not pack:
            st.signature = None
            return
        need = _lib.size("rf_packed_bytes", st.handle)
        if st.packed is None or st.packed.numel() < need or st.packed.device != device:
            st.packed = torch.empty(need, dtype=torch.uint8, device=device)
        _lib.launch("rf_pack_params", st.packed, st.handle, st.packed, need)
        st.signature = sig

    def _run(self, x: torch.Tensor, packed_input: bool) -> torch.Tensor:
        self._refuse_host_tensor(x)
        if x.dim() != 4:
            raise RuntimeError(f"expected a 4-D input [B,C,H,W], got {tuple(x.shape)}")
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("RawFormer.forward (HIP) is the inference path and builds no autograd graph: call model.eval() or wrap "
                               "in torch.no_grad(); to train use bayer_low_light_image_enhancement_amd.train.Trainer(model).step(x, gt) "
                               "(rf_train_step: forward, loss, explicit backward, Adam / AdamW)")
        self._refuse_training_mode()
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        b, c, h, w = x.shape
        if packed_input:
            if c != 4 * self.inp_channels:
                raise RuntimeError(f"expected {4 * self.inp_channels} packed channels, got {c}")
            H, W = h, w
        else:
            if c != self.inp_channels:
                raise RuntimeError(f"Given a mosaic with {c} channels, expected {self.inp_channels}")
            if h % 2 or w % 2:
                raise RuntimeError(f"mosaic size {h}x{w} must be even")
            H, W = h // 2, w // 2
        if H % 8 or W % 8:
            raise RuntimeError(f"mosaic size must be divisible by 16 (three 2x down-samplings after the Bayer pack); "
                               f"got {2 * H}x{2 * W}")
        st = self._state_with_workspace(x.device, b, H, W)
        out = torch.empty((b, self.out_channels, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        _lib.launch("rf_forward", x, st.handle, x, out, st.workspace, st.workspace.numel(), b, H, W, packed_input)
        return out

    def _refuse_training_mode(self) -> None:
        if self.variant == "wfb" and self.training:
            raise RuntimeError("RawFormer(variant='wfb') is inference only: in training mode its BatchNorm layers are a different "
                               "function (batch statistics); call model.eval()")

    def forward_window(self, x: torch.Tensor, y_lo: int, y_hi: int, total_rows: int, group=None, *,
                       x_lo: int = 0, x_hi: int = 0, total_cols: Optional[int] = None) -> torch.Tensor:
        """Forward of one rank's WINDOW of a spatially sharded frame (``tiling.forward_full_frame_exact``; C ABI
        ``rf_set_shard``).  ``x``: the window of the mosaic ``[B,1,2Hl,2Wl]``, the same shape on every rank of ``group``;
        ``[y_lo, y_hi)``: this rank's interior rows inside the window and ``total_rows`` the frame's height, in PACKED rows
        (mosaic rows / 2, multiples of 8).  The channel attention's Gram statistics and FLCA's squeeze-excite pooling are
        taken over interior rows and all-reduced over ``group`` (RCCL with the ``nccl`` backend), so interior rows of the
        result equal the whole-frame forward up to summation order when the window reaches ``tiling.HALO_ROWS`` rows beyond
        the interior (or the frame border).  Rows outside the interior are meaningless.

        With ``total_cols`` the window is one of a rows x columns grid (``rf_set_shard_grid``): the interior is also cut to
        columns ``[x_lo, x_hi)`` of the window, ``total_cols`` is the frame's packed width, ``x_lo`` a multiple of 32 and
        ``x_hi`` a multiple of 32 or the window's width (``tiling.plan_grid_shards``)."""
        import torch.distributed as dist

        if self.variant not in ("flca", "plain"):
            raise RuntimeError(f"forward_window: variants 'flca' and 'plain' only, not {self.variant!r}")
        lib = _lib.load()
        failure: List[BaseException] = []

        def allreduce(_user, buf, n, op, _stream):
            try:
                ws = self._state_for(x.device).workspace
                off = buf - ws.data_ptr()
                if off < 0 or off % 4 or off + 4 * n > ws.numel():
                    raise RuntimeError("all-reduce buffer outside the workspace")
                view = ws[off: off + 4 * n].view(torch.float32)
                dist.all_reduce(view, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)      # ordered on torch's current stream = `stream`
            except BaseException as e:  # noqa: BLE001 - a ctypes callback cannot raise; re-raised below
                failure.append(e)

        cb = _lib.ALLREDUCE_FN(allreduce)
        with torch.cuda.device(x.device):
            # the workspace must exist (and not move) before the callback sees pointers into it
            st = self._state_with_workspace(x.device, x.shape[0], x.shape[2] // 2, x.shape[3] // 2, sync=False)
            if total_cols is None:
                if x_lo or x_hi:
                    raise ValueError("forward_window: x_lo / x_hi need total_cols")
                _lib.call("rf_set_shard", st.handle, int(y_lo), int(y_hi), int(total_rows), cb, None)
            else:
                _lib.call("rf_set_shard_grid", st.handle, int(y_lo), int(y_hi), int(total_rows), int(x_lo), int(x_hi), int(total_cols), cb, None)
            try:
                out = self._run(x, packed_input=False)
            finally:
                lib.rf_set_shard(st.handle, 0, 0, 0, _lib.ALLREDUCE_FN(0), None)      # unchecked: must not mask _run's own exception
        if failure:
            raise failure[0]
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Mosaic ``[B, inp_channels, 2H, 2W]`` -> ``[B, out_channels, 2H, 2W]`` (test.py:116)."""
        return self._run(x, packed_input=False)

    def forward_packed(self, x4: torch.Tensor) -> torch.Tensor:
        """Packed RGGB ``[B, 4, H, W]`` (the ``downshuffle`` already applied) -> ``[B, 3, 2H, 2W]``."""
        return self._run(x4, packed_input=True)

    def forward_stage(self, stage: int, x: torch.Tensor, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ``conv_tran<stage>`` (``Conv_Transformer``) exactly as ``forward`` schedules it.  ``x``: the stage input
        ``[B, dim*2^l, H>>l, W>>l]``; ``packed``: the packed frame ``[B,4,H,W]`` the branch's guidance is derived from
        (``variant='flca'``, ``'multilvl'`` and ``'truecolor'``, whose front end -- ``EnhancedBayerProcessor`` with the model's
        own parameters -- runs on it first; for ``'plain'`` and ``'wfb'`` pass ``None`` and H, W are taken from ``x``)."""
        self._refuse_host_tensor(x)
        self._refuse_training_mode()
        lvl = stage - 1 if stage <= 4 else 7 - stage
        x = x.detach().float().contiguous()
        b, c, hh, ww = x.shape
        if c != self.dim << lvl:
            raise RuntimeError(f"stage {stage} expects {self.dim << lvl} channels, got {c}")
        H, W = hh << lvl, ww << lvl
        if packed is not None:
            packed = packed.detach().float().contiguous()
            if tuple(packed.shape) != (b, 4, H, W):
                raise RuntimeError(f"packed frame must be {(b, 4, H, W)}, got {tuple(packed.shape)}")
        st = self._state_with_workspace(x.device, b, H, W)
        out = torch.empty_like(x)
        _lib.launch("rf_forward_stage", x, st.handle, stage, x, packed, out, st.workspace, st.workspace.numel(), b, H, W)
        return out

    def tc_guidance(self, packed: torch.Tensor, level: int):
        """``variant='truecolor'``: the front end on a packed frame ``[B,4,H,W]`` exactly as ``forward`` runs it, and the seven
        guidance planes an ``EnhancedFLCA`` block sees at U-Net level ``level`` (0..3).  Returns ``(y [B,1,H,W], crcb [B,2,H,W],
        rgb [B,3,H,W], guide [B,7,H>>level,W>>level])``: ``EnhancedBayerProcessor``'s outputs (BayerTORGBColorMultiLvl.py:100-134)
        and ``[y, cr, cb, R, G, y_low, y_high]`` (:255-275)."""
        self._refuse_host_tensor(packed)
        if self.variant != "truecolor":
            raise RuntimeError(f"tc_guidance: variant 'truecolor' only, not {self.variant!r}")
        packed = packed.detach().float().contiguous()
        if packed.dim() != 4 or packed.shape[1] != 4:
            raise RuntimeError(f"expected a packed frame [B,4,H,W], got {tuple(packed.shape)}")
        b, _, H, W = packed.shape
        st = self._state_with_workspace(packed.device, b, H, W)
        new = lambda c, hh, ww: torch.empty((b, c, hh, ww), dtype=torch.float32, device=packed.device)      # noqa: E731
        y, crcb, rgb, guide = new(1, H, W), new(2, H, W), new(3, H, W), new(7, H >> max(level, 0), W >> max(level, 0))
        _lib.launch("rf_tc_guidance", packed, st.handle, packed, int(level), y, crcb, rgb, guide, st.workspace, st.workspace.numel(), b, H, W)
        return y, crcb, rgb, guide

    def _ml_call(self, who: str, frame: torch.Tensor, H: int, W: int):
        """``variant='multilvl'`` diagnostics: the device state with parameters in place and a workspace for ``(B, H, W)``."""
        self._refuse_host_tensor(frame)
        if self.variant != "multilvl":
            raise RuntimeError(f"{who}: variant 'multilvl' only, not {self.variant!r}")
        return self._state_with_workspace(frame.device, frame.shape[0], H, W)

    def ml_guidance(self, packed: torch.Tensor, level: int):
        """``variant='multilvl'``: the guidance an ``FLCA_Pyramid`` block sees at U-Net level ``level`` (0..3) of a packed frame
        ``[B,4,H,W]``, exactly as ``forward`` computes it.  Returns ``(guide [B,2L+2,H>>level,W>>level], means [B,8])``: the planes
        ``[y_low_0, y_high_0, .., y_low_{L-1}, y_high_{L-1}, cr, cb]`` (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:143-145,
        :168-169; L = ``flca_levels``) and the table the kernels read their pooled gates from: ``means[:, 2l]``, ``means[:, 2l+1]`` the
        means of ``y_low_l``, ``y_high_l`` at this size (:151-152), ``means[:, 6]`` that of ``sqrt(cr^2 + cb^2 + eps)`` (:171-172)."""
        packed = packed.detach().float().contiguous()
        if packed.dim() != 4 or packed.shape[1] != 4:
            raise RuntimeError(f"expected a packed frame [B,4,H,W], got {tuple(packed.shape)}")
        b, _, H, W = packed.shape
        st = self._ml_call("ml_guidance", packed, H, W)
        guide = torch.empty((b, 2 * self.flca_levels + 2, H >> max(level, 0), W >> max(level, 0)), dtype=torch.float32, device=packed.device)
        means = torch.zeros((b, 8), dtype=torch.float32, device=packed.device)
        _lib.launch("rf_ml_guidance", packed, st.handle, packed, int(level), guide, means, st.workspace, st.workspace.numel(), b, H, W)
        return guide, means

    def ml_tail(self, image: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """``variant='multilvl'``: the colour anchor and the luminance nudge of ``RawFormer.forward``
        (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:403-414) applied to ``image`` [B,3,2H,2W] for the model input ``x``, a
        mosaic ``[B,1,2H,2W]`` or a packed frame ``[B,4,H,W]``, as ``forward`` applies them to its own output.  A new tensor."""
        x = x.detach().float().contiguous()
        if x.dim() != 4 or x.shape[1] not in (1, 4):
            raise RuntimeError(f"expected a mosaic [B,1,2H,2W] or a packed frame [B,4,H,W], got {tuple(x.shape)}")
        packed_input = x.shape[1] == 4
        b = x.shape[0]
        H, W = (x.shape[2], x.shape[3]) if packed_input else (x.shape[2] // 2, x.shape[3] // 2)
        if tuple(image.shape) != (b, 3, 2 * H, 2 * W) or image.device != x.device:
            raise RuntimeError(f"image must be {(b, 3, 2 * H, 2 * W)} on {x.device}, got {tuple(image.shape)} on {image.device}")
        out = image.detach().float().clone(memory_format=torch.contiguous_format)
        st = self._ml_call("ml_tail", x, H, W)
        _lib.launch("rf_ml_tail", x, st.handle, out, x, packed_input, st.workspace, st.workspace.numel(), b, H, W)
        return out

    def workspace_bytes(self, batch: int, H: int, W: int) -> int:
        probe = C.c_void_p()
        cfg = self._config()
        _lib.call("rf_create", C.byref(cfg), C.byref(probe))
        try:
            return _lib.size("rf_workspace_bytes", probe, batch, H, W)
        finally:
            _lib.load().rf_destroy(probe)

    def __del__(self):
        try:
            if getattr(self, "_rt_owner", None) != id(self):
                return
            lib = _lib.load()
            for st in getattr(self, "_rt", {}).values():
                if st.handle:
                    lib.rf_destroy(st.handle)
                    st.handle = C.c_void_p()
        except Exception:
            pass
