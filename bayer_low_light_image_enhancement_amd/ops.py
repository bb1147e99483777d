"""Operator-level Python surface over the C ABI (same kernels the whole forward uses).

Function names and argument meaning follow the reference's Python
(``downshuffle``, ``dwt_init`` / ``iwt_init``, ``CustomDWT`` / ``CustomIDWT``, ``HaarDWT``,
``LayerNorm``, ``Attention`` ...), so the parity tests read like calls into the reference.
Tensors must be float32, contiguous, on a ROCm device; torch is only the allocator and the
stream provider here.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor is on {t.device}; the RawFormer HIP path has no CPU implementation")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _opt(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    return None if t is None else _chk(t, name)


def _out(out: Optional[torch.Tensor], like: torch.Tensor, who: str, shape=None, name: str = "out") -> torch.Tensor:
    """The tensor an operator writes: a new one of ``shape`` (default: ``like``'s) beside ``like``, a checked float32 tensor, or
    the caller's own, checked."""
    if out is None:
        return torch.empty_like(like) if shape is None else like.new_empty(shape)
    shape = tuple(like.shape) if shape is None else tuple(shape)
    if tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != torch.float32 or out.device != like.device:
        raise RuntimeError(f"{who}: `{name}` must be a contiguous float32 tensor of shape {shape} on {like.device}")
    return out


def downshuffle(x: torch.Tensor, r: int = 2) -> torch.Tensor:
    """``downshuffle(var, 2)`` (RawFomer_WFB_FFAB/model.py:287-298): [B,C,2h,2w] -> [B,4C,h,w]."""
    if r != 2:
        raise ValueError("only r=2 is used by RawFormer")
    x = _chk(x, "x")
    b, c, h2, w2 = x.shape
    if h2 % 2 or w2 % 2:
        raise RuntimeError(f"downshuffle: spatial size {h2}x{w2} not divisible by 2")
    out = torch.empty((b, 4 * c, h2 // 2, w2 // 2), dtype=x.dtype, device=x.device)
    _lib.launch("rf_pixel_unshuffle2", x, x, out, b, c, h2 // 2, w2 // 2)
    return out


def pixel_shuffle(x: torch.Tensor, r: int = 2) -> torch.Tensor:
    """``nn.PixelShuffle(2)`` (RawFomer_WFB_FFAB/model.py:471,507): [B,4C,h,w] -> [B,C,2h,2w]."""
    if r != 2:
        raise ValueError("only r=2 is used by RawFormer")
    x = _chk(x, "x")
    b, c4, h, w = x.shape
    if c4 % 4:
        raise RuntimeError(f"pixel_shuffle: {c4} channels not divisible by 4")
    out = torch.empty((b, c4 // 4, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    _lib.launch("rf_pixel_shuffle2", x, x, out, b, c4 // 4, h, w)
    return out


def dwt_init(x: torch.Tensor) -> torch.Tensor:
    """``dwt_init`` / ``DWT`` (RawFomer_WFB_FFAB/blocks.py:102-115): [B,C,2h,2w] -> [4B,C,h,w]."""
    x = _chk(x, "x")
    b, c, h2, w2 = x.shape
    if h2 % 2 or w2 % 2:
        raise RuntimeError(f"dwt_init: spatial size {h2}x{w2} not divisible by 2")
    out = torch.empty((4 * b, c, h2 // 2, w2 // 2), dtype=x.dtype, device=x.device)
    _lib.launch("rf_dwt_haar", x, x, out, b, c, h2 // 2, w2 // 2)
    return out


def iwt_init(x: torch.Tensor) -> torch.Tensor:
    """``iwt_init`` / ``IWT`` (RawFomer_WFB_FFAB/blocks.py:119-136): [4B,C,h,w] -> [B,C,2h,2w]."""
    x = _chk(x, "x")
    b4, c, h, w = x.shape
    if b4 % 4:
        raise RuntimeError(f"iwt_init: batch {b4} not divisible by 4")
    out = torch.empty((b4 // 4, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    _lib.launch("rf_idwt_haar", x, x, out, b4 // 4, c, h, w)
    return out


def _k16(kernel: Sequence[Sequence[float]]):
    flat = [float(v) for row in kernel for v in row]
    if len(flat) != 16:
        raise ValueError("kernel must be 4x4")
    return (C.c_float * 16)(*flat)


DEFAULT_KERNEL = ((1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1))  # README.md:98-103


def custom_dwt(x: torch.Tensor, kernel=DEFAULT_KERNEL, norm: bool = True) -> torch.Tensor:
    """``CustomDWT(kernel, norm=norm)(x)`` (README.md:92-117): [B,C,2h,2w] -> [B,4C,h,w]."""
    x = _chk(x, "x")
    b, c, h2, w2 = x.shape
    if h2 % 2 or w2 % 2:
        raise RuntimeError(f"CustomDWT: spatial size {h2}x{w2} not divisible by 2")
    out = torch.empty((b, 4 * c, h2 // 2, w2 // 2), dtype=x.dtype, device=x.device)
    _lib.launch("rf_dwt_custom", x, x, out, _k16(kernel), int(norm), b, c, h2 // 2, w2 // 2)
    return out


def custom_idwt(x: torch.Tensor, kernel=DEFAULT_KERNEL, norm: bool = True) -> torch.Tensor:
    """``CustomIDWT(kernel, norm=norm)(x)`` (README.md:120-144): [B,4C,h,w] -> [B,C,2h,2w]."""
    x = _chk(x, "x")
    b, c4, h, w = x.shape
    if c4 % 4:
        raise RuntimeError(f"CustomIDWT: {c4} channels not divisible by 4")
    out = torch.empty((b, c4 // 4, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    _lib.launch("rf_idwt_custom", x, x, out, _k16(kernel), int(norm), b, c4 // 4, h, w)
    return out


def haar_dwt(x: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """``HaarDWT()(x)`` (FrequencyawareLumaChromaAttentionRAWFormer.py:39-73): LL, (LH, HL, HH)."""
    x = _chk(x, "x")
    b, c, h, w = x.shape
    out = torch.empty((4, b, c, (h + 1) // 2, (w + 1) // 2), dtype=x.dtype, device=x.device)
    _lib.launch("rf_haar_dwt", x, x, out, b, c, h, w)
    return out[0], (out[1], out[2], out[3])


def layernorm2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5) -> torch.Tensor:
    """``LayerNorm(dim)(x)`` on NCHW (FrequencyawareLumaChromaAttentionRAWFormer.py:180-187);
    ``bias=None`` is ``BiasFree_LayerNorm`` (RawFomer_WFB_FFAB/model.py:89-103)."""
    x, weight, bias = _chk(x, "x"), _chk(weight, "weight"), _opt(bias, "bias")
    b, c, h, w = x.shape
    if weight.numel() != c:
        raise RuntimeError(f"LayerNorm: weight has {weight.numel()} elements, input has {c} channels")
    out = torch.empty_like(x)
    _lib.launch("rf_layernorm2d", x, x, out, weight, bias, float(eps), b, c, h, w)
    return out


def conv1x1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
            x2: Optional[torch.Tensor] = None, ln_weight: Optional[torch.Tensor] = None,
            ln_bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nn.Conv2d(Cin, Cout, 1)``; optional fused LayerNorm prologue, ``torch.cat([x, x2], 1)``
    input and residual add."""
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    b, c1, h, w = x.shape
    c2 = 0
    if x2 is not None:
        x2 = _chk(x2, "x2")
        c2 = x2.shape[1]
    cout = weight.shape[0]
    if weight.numel() != cout * (c1 + c2):
        raise RuntimeError(f"conv1x1: weight {tuple(weight.shape)} does not match {c1 + c2} input channels")
    scratch = _lib.scratch("rf_conv1x1_scratch_bytes", x, c1 + c2, cout)
    out = torch.empty((b, cout, h, w), dtype=x.dtype, device=x.device)
    args = [_opt(t, "arg") for t in (bias, ln_weight, ln_bias, residual)]
    _lib.launch("rf_conv1x1", x, x, x2, out, weight, *args, scratch, b, c1, c2, cout, h, w)
    return out


def dwconv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, gelu: bool = False) -> torch.Tensor:
    """``nn.Conv2d(C, C, 3, padding=1, groups=C)`` (+ exact GELU)."""
    x, weight, bias = _chk(x, "x"), _chk(weight, "weight"), _opt(bias, "bias")
    b, c, h, w = x.shape
    if weight.numel() != c * 9:
        raise RuntimeError(f"dwconv3x3: weight {tuple(weight.shape)} does not match {c} channels")
    out = torch.empty_like(x)
    _lib.launch("rf_dwconv3x3", x, x, out, weight, bias, int(gelu), b, c, h, w)
    return out


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
            store: str = "plain") -> torch.Tensor:
    """``nn.Conv2d(Cin, Cout, 3, padding=1)``; ``act='lrelu'`` adds LeakyReLU(0.2), ``'relu'`` ReLU;
    ``store='unshuffle'`` = Downsample (a8), ``'shuffle'`` = conv_out + PixelShuffle (a10)."""
    x, weight, bias = _chk(x, "x"), _chk(weight, "weight"), _opt(bias, "bias")
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (cin, 3, 3):
        raise RuntimeError(f"conv3x3: weight {tuple(weight.shape)} does not match {cin} input channels")
    mode = {"plain": 0, "unshuffle": 1, "shuffle": 2}[store]
    shape = {0: (b, cout, h, w), 1: (b, cout * 4, h // 2, w // 2), 2: (b, cout // 4, 2 * h, 2 * w)}[mode]
    scratch = _lib.scratch("rf_conv3x3_scratch_bytes", x, cin, cout)
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _lib.launch("rf_conv3x3", x, x, out, weight, bias, scratch, {"none": 0, "lrelu": 1, "relu": 2}[act], mode, b, cin, cout, h, w)
    return out


def conv_transpose2x2(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nn.ConvTranspose2d(Cin, Cout, 2, stride=2)`` (RawFomer_WFB_FFAB/model.py:461)."""
    x, weight, bias = _chk(x, "x"), _chk(weight, "weight"), _opt(bias, "bias")
    b, cin, h, w = x.shape
    if weight.shape[0] != cin or tuple(weight.shape[2:]) != (2, 2):
        raise RuntimeError(f"ConvTranspose2d: weight {tuple(weight.shape)} does not match {cin} input channels")
    cout = weight.shape[1]
    scratch = _lib.scratch("rf_convT2x2_scratch_bytes", x, cin, cout)
    out = torch.empty((b, cout, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
    _lib.launch("rf_convT2x2", x, x, out, weight, bias, scratch, b, cin, cout, h, w)
    return out


def channel_attention(x: torch.Tensor, qkv_w, qkv_b, dw_w, dw_b, temperature, proj_w, proj_b, heads: int) -> torch.Tensor:
    """``Attention(dim, heads, bias=True)(x)`` (FrequencyawareLumaChromaAttentionRAWFormer.py:212-235)."""
    x = _chk(x, "x")
    ts = [_opt(t, "param") for t in (qkv_w, qkv_b, dw_w, dw_b, temperature, proj_w, proj_b)]
    b, c, h, w = x.shape
    if c % heads:
        raise RuntimeError(f"Attention: {c} channels not divisible by {heads} heads")
    scratch = _lib.scratch("rf_chan_attn_scratch_bytes", x, b, c, heads, h, w)
    out = torch.empty_like(x)
    _lib.launch("rf_chan_attn", x, x, out, *ts, scratch, b, c, heads, h, w)
    return out


def _guidance(x4: torch.Tensor, size: Optional[Tuple[int, int]], who: str):
    """``rf_flca_guidance`` on the packed frame ``x4`` at feature size ``size`` (``None``: the frame's own): the four planes and
    the scratch area, at whose head the kernels keep the base planes ``y, cr, cb`` (include/rawformer_hip.h)."""
    x4 = _chk(x4, "x4")
    b, c, h, w = x4.shape
    if c != 4:
        raise RuntimeError(f"{who} expects packed RGGB [B,4,H,W]")
    scratch = _lib.scratch("rf_guidance_scratch_bytes", x4, b, h, w)
    oh, ow = (h, w) if size is None else (size[0], size[1])
    out = torch.empty((b, 4, oh, ow), dtype=x4.dtype, device=x4.device)
    _lib.launch("rf_flca_guidance", x4, x4, out, scratch, b, h, w, oh, ow)
    return out, scratch


def flca_guidance(x4: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """Guidance planes ``[y_low, y_high, cr, cb]`` an FLCA block sees at feature size ``size``
    (``BayerLumaChroma`` + ``HaarDWT`` + bilinear ``F.interpolate``,
    FrequencyawareLumaChromaAttentionRAWFormer.py:79-97,138-149)."""
    return _guidance(x4, size, "flca_guidance")[0]


def bayer_luma_chroma(x4: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``BayerLumaChroma()(x4)`` -> ``(y, cr, cb)``, each ``[B,1,H,W]``
    (FrequencyawareLumaChromaAttentionRAWFormer.py:79-97): the base planes the guidance kernels keep at the head of their
    scratch area (include/rawformer_hip.h, rf_flca_guidance)."""
    scratch = _guidance(x4, None, "bayer_luma_chroma")[1]
    b, _, h, w = x4.shape
    planes = scratch[: 3 * b * h * w * 4].view(torch.float32).reshape(3, b, 1, h, w)
    return planes[0].clone(), planes[1].clone(), planes[2].clone()


def conv_ffn(x: torch.Tensor, pw1_w, pw1_b, dw_w, dw_b, pw2_w, pw2_b) -> torch.Tensor:
    """``conv_ffn(dim, expansion)(x)`` = 1x1 -> depthwise 3x3 -> GELU -> 1x1
    (FrequencyawareLumaChromaAttentionRAWFormer.py:190-209, RawFomer_WFB_FFAB/model.py:319-336), as the three kernels
    the forward launches for it at U-Net levels 1-3 (level 0 runs it inside the fused FFN kernel together with
    LayerNorm and the residual: ``transformer_block``)."""
    return conv1x1(dwconv3x3(conv1x1(x, pw1_w, pw1_b), dw_w, dw_b, gelu=True), pw2_w, pw2_b)


_TB_KEYS = ("norm1.body.weight", "norm1.body.bias", "attn.temperature", "attn.qkv.weight", "attn.qkv.bias",
            "attn.qkv_dwconv.weight", "attn.qkv_dwconv.bias", "attn.project_out.weight", "attn.project_out.bias",
            "norm2.body.weight", "norm2.body.bias", "ffn.pointwise1.weight", "ffn.pointwise1.bias",
            "ffn.depthwise.weight", "ffn.depthwise.bias", "ffn.pointwise2.weight", "ffn.pointwise2.bias")


def transformer_block(x: torch.Tensor, params, heads: int, ffn_expansion_factor: int = 2, prefix: str = "", interior=None) -> torch.Tensor:
    """``TransformerBlock(dim, heads, ffn_expansion_factor, bias=True)(x)``
    (FrequencyawareLumaChromaAttentionRAWFormer.py:238-254).  ``params`` maps the block's
    state_dict keys (``norm1.body.weight`` ...) to device tensors.  Same schedule as the whole
    forward, i.e. the fused gfx950 kernels where the shape allows.  ``interior = (y_lo, y_hi, x_lo, x_hi)``: ``x`` is one window
    of a sharded frame and only that part of it enters the attention's Gram statistics (``rf_transformer_block_window``)."""
    x = _chk(x, "x")
    b, c, h, w = x.shape
    ts = [_chk(params[prefix + k], k) for k in _TB_KEYS]
    scratch = _lib.scratch("rf_transformer_block_scratch_bytes", x, b, c, heads, ffn_expansion_factor, h, w)
    out = torch.empty_like(x)
    if interior is None:
        _lib.launch("rf_transformer_block", x, x, out, ts, scratch, b, c, heads, ffn_expansion_factor, h, w)
    else:
        _lib.launch("rf_transformer_block_window", x, x, out, ts, scratch, b, c, heads, ffn_expansion_factor, h, w, *(int(v) for v in interior))
    return out


_FLCA_KEYS = ("alpha", "beta", "gamma", "low_attn.0.weight", "high_attn.0.weight", "chroma_attn.0.weight",
              "se.1.weight", "se.1.bias", "se.3.weight", "se.3.bias")


def flca(feat: torch.Tensor, x4: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """``FLCA(channels)(feat, *BayerLumaChroma()(x4))`` (FrequencyawareLumaChromaAttentionRAWFormer.py:103-162):
    guidance from the packed RGGB frame ``x4``, spatial gates, squeeze-excite."""
    feat = _chk(feat, "feat")
    b, c, h, w = feat.shape
    guide = flca_guidance(x4, (h, w))
    ts = [_chk(params[prefix + k].reshape(-1) if params[prefix + k].dim() == 0 else params[prefix + k], k) for k in _FLCA_KEYS]
    scratch = _lib.scratch("rf_flca_scratch_bytes", feat, b, c, h, w)
    out = torch.empty_like(feat)
    _lib.launch("rf_flca", feat, feat, guide, out, ts, scratch, b, c, h, w)
    return out


def token_attention(qkv: torch.Tensor, heads: int, scale: Optional[float] = None) -> torch.Tensor:
    """``softmax(q k^T * scale) v`` per (image, head) with tokens = pixels (Attenblock.py:212-217), flash style:
    ``qkv`` is ``[B, 3*heads*d, H, W]`` (q, k, v thirds, channel = head*d + i), the result ``[B, heads*d, H, W]``."""
    qkv = _chk(qkv, "qkv")
    b, c3, h, w = qkv.shape
    if c3 % (3 * heads):
        raise RuntimeError(f"token_attention: {c3} channels are not 3 x {heads} heads x d")
    inner = c3 // 3
    d, n = inner // heads, h * w
    if not 1 <= d <= 32:                                  # rf_token_attn's own check, ahead of the default scale d ** -0.5
        raise RuntimeError(f"token_attention: head dimension {d} not in 1..32")
    out = torch.empty((b, inner, h, w), dtype=qkv.dtype, device=qkv.device)
    q = qkv.data_ptr()
    _lib.launch("rf_token_attn", qkv, q, q + 4 * inner * n, q + 8 * inner * n, out, 3 * inner * n, inner * n, b, heads, d, n,
                float(d ** -0.5 if scale is None else scale))
    return out


def luma_film(qkv: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, luma: Optional[torch.Tensor] = None,
              alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FiLM ``gamma * t + beta`` on the q, k, v thirds of ``qkv`` and the query bias
    ``alpha * centered(avg_pool3(1 - luma))`` (Attenblock.py:193-210)."""
    qkv, gamma, beta = _chk(qkv, "qkv"), _chk(gamma, "gamma"), _chk(beta, "beta")
    b, c3, h, w = qkv.shape
    inner = c3 // 3
    if tuple(gamma.shape) != (b, inner, h, w) or tuple(beta.shape) != (b, inner, h, w):
        raise RuntimeError(f"luma_film: gamma/beta {tuple(gamma.shape)} do not match {(b, inner, h, w)}")
    if luma is not None:
        luma = _chk(luma, "luma")
        if tuple(luma.shape) != (b, 1, h, w):
            raise RuntimeError(f"luma_film: luma {tuple(luma.shape)} must be {(b, 1, h, w)}")
        alpha = _chk(alpha, "alpha")
    scratch = _lib.scratch("rf_luma_film_scratch_bytes", qkv, b, h, w)
    out = torch.empty_like(qkv)
    _lib.launch("rf_luma_film", qkv, qkv, gamma, beta, inner * h * w, luma, alpha, out, scratch, b, inner, h, w)
    return out


def _luma_attention(x, luma, params, prefix, heads, ln_weight=None, ln_bias=None, residual=None):
    """The schedule of ``LuminanceAwareMHSA`` on the state_dict keys under ``prefix``; a LayerNorm (``ln_*``) rides in the prologue
    of the ``to_qkv`` GEMM, ``residual`` in the epilogue of ``proj``."""
    p = lambda k: params[prefix + k]  # noqa: E731
    qkv = conv1x1(x, p("to_qkv.weight"), params.get(prefix + "to_qkv.bias"), ln_weight=ln_weight, ln_bias=ln_bias)
    hcond = conv3x3(luma, p("luma_cond.net.0.weight"), p("luma_cond.net.0.bias"), act="relu")
    hcond = conv3x3(hcond, p("luma_cond.net.2.weight"), p("luma_cond.net.2.bias"), act="relu")
    gamma = conv1x1(hcond, p("luma_cond.gamma.weight"), p("luma_cond.gamma.bias"))
    beta = conv1x1(hcond, p("luma_cond.beta.weight"), p("luma_cond.beta.bias"))
    alpha = params.get(prefix + "alpha")
    qkv = luma_film(qkv, gamma, beta, luma if alpha is not None else None, None if alpha is None else alpha.reshape(1))
    return conv1x1(token_attention(qkv, heads), p("proj.weight"), params.get(prefix + "proj.bias"), residual=residual)


def luminance_aware_mhsa(x: torch.Tensor, luma: torch.Tensor, params, heads: int = 8, prefix: str = "") -> torch.Tensor:
    """``LuminanceAwareMHSA.forward(x, luma)`` (Attenblock.py:161-220) from its state_dict ``params``
    (``to_qkv``, ``proj``, ``luma_cond.net.{0,2}``, ``luma_cond.{gamma,beta}``, ``alpha``): 1x1 GEMM, two 3x3
    convs + ReLU, two 1x1 GEMMs, FiLM + luma bias, flash token attention, 1x1 GEMM."""
    return _luma_attention(x, luma, params, prefix, heads)


def dwgate3x3(x: torch.Tensor, wa: torch.Tensor, ba: Optional[torch.Tensor], wb: torch.Tensor, bb: Optional[torch.Tensor]) -> torch.Tensor:
    """``gelu(g) * a + gelu(a) * g`` with ``a = dw3x3(x; wa, ba)``, ``g = dw3x3(x; wb, bb)`` in one pass
    (middle of the WFB ``FeedForward``, RawFomer_WFB_FFAB/model.py:55-59 with the rep-conv branch fused)."""
    x, wa, wb = _chk(x, "x"), _chk(wa, "wa"), _chk(wb, "wb")
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    _lib.launch("rf_dwgate3x3", x, x, out, wa, _opt(ba, "ba"), wb, _opt(bb, "bb"), b, c, h, w)
    return out


def dwconv5x5(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nn.Conv2d(C, C, 5, padding=2, groups=C)`` (Illumination_Estimator.depth_conv, model.py:182-183)."""
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    b, c, h, w = x.shape
    if tuple(weight.shape) != (c, 1, 5, 5):
        raise RuntimeError(f"dwconv5x5: weight {tuple(weight.shape)} does not match {c} channels")
    out = torch.empty_like(x)
    _lib.launch("rf_dwconv5x5", x, x, out, weight, _opt(bias, "bias"), b, c, h, w)
    return out


def fuse_rep_convs(params, prefix: str = "", eps: float = 1e-5):
    """``FeedForward.fuse()`` (RawFomer_WFB_FFAB/model.py:27-40, 66-87) on a state_dict: the depthwise 3x3 + BN,
    the depthwise 1x1 + BN and the identity as ONE depthwise 3x3 weight and bias (weight preparation, host side)."""
    def bn_fold(name):
        s = params[prefix + name + ".bn.weight"] / torch.sqrt(params[prefix + name + ".bn.running_var"] + eps)
        wgt = params[prefix + name + ".c.weight"] * s[:, None, None, None]
        return wgt, params[prefix + name + ".bn.bias"] - params[prefix + name + ".bn.running_mean"] * s
    w1, b1 = bn_fold("rep_conv1")
    w2, b2 = bn_fold("rep_conv2")
    ident = torch.zeros_like(w1)
    ident[:, :, 1, 1] = 1.0
    return (w1 + torch.nn.functional.pad(w2, [1, 1, 1, 1]) + ident).contiguous(), (b1 + b2).contiguous()


def wfb_feed_forward(x: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """Eval-mode ``FeedForward.forward`` (RawFomer_WFB_FFAB/model.py:42-62): 1x1, fused gate pass, 1x1 + identity."""
    p = lambda k: params.get(prefix + k)  # noqa: E731
    wa, ba = fuse_rep_convs(params, prefix)
    hid = conv1x1(x, p("project_in.weight"), p("project_in.bias"))
    gated = dwgate3x3(hid, wa, ba, p("dwconv.weight"), p("dwconv.bias"))
    return conv1x1(gated, p("project_out.weight"), p("project_out.bias"), residual=x)


def illumination_estimator(img: torch.Tensor, params, prefix: str = "") -> Tuple[torch.Tensor, torch.Tensor]:
    """``Illumination_Estimator.forward`` (RawFomer_WFB_FFAB/model.py:186-200) -> (illu_fea, illu_map).  The channel
    mean that the reference concatenates folds into conv1's weights: W [img ; mean] = (W_img + w_mean / C) img."""
    img = _chk(img, "img")
    b, c, h, w = img.shape
    w1 = params[prefix + "conv1.weight"]
    if w1.shape[1] != c + 1:
        raise RuntimeError(f"illumination_estimator: conv1 expects {w1.shape[1]} = C + 1 channels, image has {c}")
    pad = (-c) % 4                                        # the GEMM kernels take channel counts in multiples of 4
    wf = torch.cat([w1[:, :c] + w1[:, c:] / c, w1.new_zeros(w1.shape[0], pad, 1, 1)], dim=1).contiguous()
    xin = torch.cat([img, img.new_zeros(b, pad, h, w)], dim=1) if pad else img
    x1 = conv1x1(xin, wf, params.get(prefix + "conv1.bias"))
    fea = dwconv5x5(x1, params[prefix + "depth_conv.weight"], params.get(prefix + "depth_conv.bias"))
    return fea, conv1x1(fea, params[prefix + "conv2.weight"], params.get(prefix + "conv2.bias"))


def upsample_cat_reduce(x: torch.Tensor, skip: torch.Tensor, up_w: torch.Tensor, up_b: Optional[torch.Tensor],
                        cr_w: torch.Tensor, cr_b: Optional[torch.Tensor]) -> torch.Tensor:
    """Decoder step ``channel_reduce(cat[up(x), skip])`` (RawFomer_WFB_FFAB/model.py:494-503) as one kernel on composed
    weights: ``x`` [B,2C,h,w], ``skip`` [B,C,2h,2w] -> [B,C,2h,2w]."""
    x, skip, up_w, cr_w = _chk(x, "x"), _chk(skip, "skip"), _chk(up_w, "up_w"), _chk(cr_w, "cr_w")
    b, c2, h, w = x.shape
    c = c2 // 2
    if tuple(skip.shape) != (b, c, 2 * h, 2 * w) or tuple(up_w.shape) != (c2, c, 2, 2) or tuple(cr_w.shape) != (c, c2, 1, 1):
        raise RuntimeError("upsample_cat_reduce: shapes do not describe ConvTranspose2d(2C,C,2,2) + cat + Conv2d(2C,C,1)")
    scratch = _lib.scratch("rf_upcat_scratch_bytes", x, c)
    out = torch.empty_like(skip)
    _lib.launch("rf_upcat", x, x, skip, out, up_w, _opt(up_b, "up_b"), cr_w, _opt(cr_b, "cr_b"), scratch, b, c, h, w)
    return out


def atten_transformer_block(x: torch.Tensor, luma: torch.Tensor, params, heads: int = 8, prefix: str = "") -> torch.Tensor:
    """``Attenblock.TransformerBlock.forward(x, luma=luma)`` (Attenblock.py:225-236): ``x + attn(LN1(x))`` then
    ``x + ffn(LN2(x))`` with ``LuminanceAwareMHSA`` and ``ConvFFN``.  Both LayerNorms ride in the prologue of the 1x1
    GEMM that consumes them, both residuals in the epilogue of the 1x1 GEMM that produces the branch."""
    p = lambda k: params.get(prefix + k)  # noqa: E731
    x1 = _luma_attention(x, luma, params, prefix + "attn.", heads, p("norm1.body.weight"), p("norm1.body.bias"), residual=x)
    f = prefix + "ffn."
    hid = conv1x1(x1, params[f + "pointwise1.weight"], params.get(f + "pointwise1.bias"), ln_weight=p("norm2.body.weight"), ln_bias=p("norm2.body.bias"))
    hid = dwconv3x3(hid, params[f + "depthwise.weight"], params.get(f + "depthwise.bias"), gelu=True)
    return conv1x1(hid, params[f + "pointwise2.weight"], params.get(f + "pointwise2.bias"), residual=x1)


def bayer_luma(mosaic: torch.Tensor, pattern: str = "rggb") -> torch.Tensor:
    """``BayerLuma(pattern)(mosaic)`` (Attenblock.py:79-138): ``[B,1,H,W]`` mosaic -> normalised luma ``[B,1,H,W]``."""
    mosaic = _chk(mosaic, "mosaic")
    b, c, h, w = mosaic.shape
    if c != 1:
        raise RuntimeError("bayer_luma expects a one-channel mosaic")
    pat = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3}[pattern.lower()]
    scratch = _lib.scratch("rf_bayer_luma_scratch_bytes", mosaic, b, h, w)
    out = torch.empty_like(mosaic)
    _lib.launch("rf_bayer_luma", mosaic, mosaic, out, scratch, b, h, w, pat)
    return out


# ------------------------------------------------------------------------------------------ FFAB / FEB (f2)
_FEB_KEYS = ("fpre.weight", "fpre.bias", "process1.0.weight", "process1.0.bias", "process1.2.weight", "process1.2.bias",
             "process2.0.weight", "process2.0.bias", "process2.2.weight", "process2.2.bias")
_PB_KEYS = tuple("frequency_process." + k for k in _FEB_KEYS) + ("cat.weight", "cat.bias")
_FFAB_KEYS = (("conv0.0.weight", "conv0.0.bias") + tuple("conv0.1." + k for k in _PB_KEYS)
              + tuple(f"conv{i}." + k for i in (1, 2, 3) for k in _PB_KEYS)
              + tuple(f"{n}.0." + k for n in ("conv4",) for k in _PB_KEYS) + ("conv4.1.weight", "conv4.1.bias")
              + tuple("conv5.0." + k for k in _PB_KEYS) + ("conv5.1.weight", "conv5.1.bias")
              + tuple("convout.0." + k for k in _PB_KEYS) + ("convout.1.weight", "convout.1.bias"))


def rfft2_polar(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``f = torch.fft.rfft2(x, norm='ortho'); (f.abs() + 1e-6, f.angle())`` (FEB, RawFomer_WFB_FFAB/blocks.py:27-29)."""
    x = _chk(x, "x")
    b, c, h, w = x.shape
    scratch = _lib.scratch("rf_rfft2_polar_scratch_bytes", x, b * c, h, w)
    mag = torch.empty((b, c, h, w // 2 + 1), dtype=x.dtype, device=x.device)
    pha = torch.empty_like(mag)
    _lib.launch("rf_rfft2_polar", x, x, mag, pha, scratch, b * c, h, w)
    return mag, pha


def polar_irfft2(mag: torch.Tensor, pha: torch.Tensor, width: int) -> torch.Tensor:
    """``torch.fft.irfft2(torch.complex(mag * cos(pha), mag * sin(pha)), s=(h, width), norm='ortho')`` (blocks.py:32-35)."""
    mag, pha = _chk(mag, "mag"), _chk(pha, "pha")
    b, c, h, wf = mag.shape
    if wf != width // 2 + 1:
        raise RuntimeError(f"half spectrum of width {wf} does not belong to an output width of {width}")
    scratch = _lib.scratch("rf_rfft2_polar_scratch_bytes", mag, b * c, h, width)
    out = torch.empty((b, c, h, width), dtype=mag.dtype, device=mag.device)
    _lib.launch("rf_polar_irfft2", mag, mag, pha, out, scratch, b * c, h, width)
    return out


def feb(x: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """``FEB(nc)(x)`` (RawFomer_WFB_FFAB/blocks.py:11-39)."""
    x = _chk(x, "x")
    b, c, h, w = x.shape
    ts = [_chk(params[prefix + k], k) for k in _FEB_KEYS]
    scratch = _lib.scratch("rf_feb_scratch_bytes", x, b, c, h, w)
    out = torch.empty_like(x)
    _lib.launch("rf_feb", x, x, out, ts, scratch, b, c, h, w)
    return out


def ffab(x: torch.Tensor, params, prefix: str = "", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``FFAB(nc)(x)`` (RawFomer_WFB_FFAB/blocks.py:59-92): seven ProcessBlocks (FEB + 1x1 + residual), dense concatenations.
    ``out``: an existing contiguous tensor (or leading slice of one) of x's shape to write into -- lets a caller place the result
    where the next operator reads it instead of concatenating afterwards."""
    x = _chk(x, "x")
    b, c, h, w = x.shape
    ts = [_chk(params[prefix + k], k) for k in _FFAB_KEYS]
    scratch = _lib.scratch("rf_ffab_scratch_bytes", x, b, c, h, w)
    out = _out(out, x, "ffab")
    _lib.launch("rf_ffab", x, x, out, ts, scratch, b, c, h, w)
    return out


def _affine_clamp_add(y: torch.Tensor, t: torch.Tensor, scale: float, shift: float, lo: float, hi: float) -> torch.Tensor:
    """``t + clamp(scale * y + shift, lo, hi)`` (``rf_affine_clamp_add``) as a new tensor."""
    out = torch.empty_like(t)
    _lib.launch("rf_affine_clamp_add", t, y, t, out, t.numel(), scale, shift, lo, hi)
    return out


def wmb_ll_branch(x: torch.Tensor, params, prefix: str = "", high=None) -> torch.Tensor:
    """The wavelet branch of ``WMB.forward`` (RawFomer_WFB_FFAB/model.py:215-243) with the Mamba module ``mb`` (``mamba_ssm``:
    absent offline, parity unpinned) replaced by ``high`` (a callable on the ``[3B,C,h/2,w/2]`` high bands; identity when
    ``None``):  ``t = 2 LN(x) - 1;  LL, hi = DWT(t);  LL = FFAB(illu(LL)[0]);  t + clamp((IWT(cat(LL, high(hi))) + 1) / 2, 0, 1)``.
    ``2 LN(x) - 1`` is the LayerNorm kernel with weight ``2 w`` and bias ``2 b - 1``."""
    x = _chk(x, "x")
    n = x.shape[0]
    t = layernorm2d(x, 2.0 * params[prefix + "norm1.body.weight"], 2.0 * params[prefix + "norm1.body.bias"] - 1.0)
    d = dwt_init(t)
    fea, _ = illumination_estimator(d[:n], params, prefix + "illu.")      # d[:n] = the LL band: a contiguous leading slice, no copy
    if high is not None:
        d[n:].copy_(high(d[n:]))                                         # the caller's module (Mamba in the reference) on the high bands
    ffab(fea, params, prefix + "ffab.", out=d[:n])                        # LL band replaced in place: IWT reads [LL ; high] as it lies
    return _affine_clamp_add(iwt_init(d), t, 0.5, 0.5, 0.0, 1.0)


# ------------------------------------------------------------------------------------------ Mamba / WM / WMB
_MAMBA_KEYS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
               "out_proj.weight")
_WM_KEYS = (("convb.0.weight", "convb.0.bias", "convb.2.weight", "convb.2.bias", "ln.weight", "ln.bias")
            + tuple("model1." + k for k in _MAMBA_KEYS) + ("smooth.weight", "smooth.bias"))


def mamba_param_shapes(d_model: int, d_state: int = 32, d_conv: int = 4, expand: int = 2):
    """state_dict names and shapes of ``mamba_ssm.modules.mamba_simple.Mamba(d_model, d_state, d_conv, expand)`` with the
    module's defaults (``dt_rank='auto'`` = ceil(d_model / 16), no projection biases, conv1d bias)."""
    di, r = expand * d_model, -(-d_model // 16)
    return {"in_proj.weight": (2 * di, d_model), "conv1d.weight": (di, 1, d_conv), "conv1d.bias": (di,),
            "x_proj.weight": (r + 2 * d_state, di), "dt_proj.weight": (di, r), "dt_proj.bias": (di,),
            "A_log": (di, d_state), "D": (di,), "out_proj.weight": (d_model, di)}


def _shaped(params, prefix, keys, shapes, what):
    """The tensors ``params[prefix + k]`` for ``k`` in ``keys``, each checked; against ``shapes[k]`` where that is given: a shape, or
    an ``int`` for an element count.  A key ``None`` (a pointer the operator takes as null) gives ``None``."""
    ts = []
    for k in keys:
        if k is None:
            ts.append(None)
            continue
        t = _chk(params[prefix + k], prefix + k)
        want = shapes.get(k)
        if isinstance(want, int):
            if t.numel() != want:
                raise RuntimeError(f"{what}: {prefix + k} has {t.numel()} elements, expected {want}")
        elif want is not None and tuple(t.shape) != tuple(want):
            raise RuntimeError(f"{what}: {prefix + k} has shape {tuple(t.shape)}, expected {tuple(want)}")
        ts.append(t)
    return ts


def mamba(u: torch.Tensor, params, prefix: str = "", d_state: int = 32, d_conv: int = 4, expand: int = 2,
          channel_major: bool = False) -> torch.Tensor:
    """``Mamba(d_model, d_state, d_conv, expand)(u)`` (mamba_ssm, as RawFomer_WFB_FFAB/model.py:146-152 builds it), inference:
    ``u`` and the result are ``[B, L, d_model]``, or ``[B, d_model, L]`` with ``channel_major=True`` (the layout of the other
    operators here).  ``params`` maps the module's state_dict keys (``mamba_param_shapes``) to device tensors."""
    u = _chk(u, "u")
    if u.dim() != 3:
        raise RuntimeError(f"mamba: expected a 3-D tensor, got {tuple(u.shape)}")
    b, l, d = (u.shape[0], u.shape[2], u.shape[1]) if channel_major else tuple(u.shape)
    ts = _shaped(params, prefix, _MAMBA_KEYS, mamba_param_shapes(d, d_state, d_conv, expand), "mamba")
    ws = _lib.scratch("rf_mamba_workspace_bytes", u, b, l, d, d_state, d_conv, expand)
    out = torch.empty_like(u)
    _lib.launch("rf_mamba_forward", u, u, out, ts, ws, ws.numel(), b, l, d, d_state, d_conv, expand, int(channel_major))
    return out


def mamba_backward(u: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", d_state: int = 32, d_conv: int = 4, expand: int = 2,
                   channel_major: bool = False, grads=None):
    """The gradient of ``mamba``: ``(grad_u, grads)`` for ``grad_out`` = dL/d ``mamba(u, params)``, in ``u``'s layout.  ``grads`` maps
    the module's state_dict keys (``prefix`` included) to the parameter gradients, with the shapes of ``mamba_param_shapes``
    (``conv1d.weight``: ``[Di, 1, 4]``).  Passing the ``grads`` of an earlier call ADDS to its tensors (a training step sums
    several modules' calls); ``grad_u`` is always a new tensor.  The forward intermediates are recomputed: nothing is kept from
    a ``mamba`` call, and ``u`` and ``grad_out`` are not written."""
    u, grad_out = _chk(u, "u"), _chk(grad_out, "grad_out")
    if u.dim() != 3 or tuple(grad_out.shape) != tuple(u.shape):
        raise RuntimeError(f"mamba_backward: expected 3-D u and grad_out of one shape, got {tuple(u.shape)} and {tuple(grad_out.shape)}")
    b, l, d = (u.shape[0], u.shape[2], u.shape[1]) if channel_major else tuple(u.shape)
    return _backward("mamba", _MAMBA_KEYS, mamba_param_shapes(d, d_state, d_conv, expand), u, params, grad_out, prefix, grads,
                     (b, l, d, d_state, d_conv, expand), (int(channel_major),))


def wm_param_shapes(c: int):
    """Names and shapes of the 17 tensors ``wm`` reads, in the order of the C ABI's pointer array."""
    shapes = {"convb.0.weight": (2 * c, c, 3, 3), "convb.0.bias": (2 * c,), "convb.2.weight": (c, 2 * c, 3, 3), "convb.2.bias": (c,),
              "ln.weight": (c,), "ln.bias": (c,)}
    shapes.update({"model1." + k: v for k, v in mamba_param_shapes(c).items()})
    shapes.update({"smooth.weight": (c, c, 3, 3), "smooth.bias": (c,)})
    return shapes


def wm(x: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """``WM(c)(x)`` (RawFomer_WFB_FFAB/model.py:138-172) on ``[n, c, h, w]``: ``convb`` + residual, LayerNorm over the runs of ``c``
    floats of the NCHW memory (the reference's raw ``reshape(b, -1, c)``), ``model1`` = ``Mamba(c, 32, 4, 2)``, ``smooth``.  Reads
    ``convb.0/2.*``, ``ln.*``, ``model1.*``, ``smooth.*``; ``model2`` is constructed by the reference but never called."""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    ts = _shaped(params, prefix, _WM_KEYS, wm_param_shapes(c), "wm")
    ws = _lib.scratch("rf_wm_workspace_bytes", x, n, c, h, w)
    out = torch.empty_like(x)
    _lib.launch("rf_wm_forward", x, x, out, ts, ws, ws.numel(), n, c, h, w)
    return out


def wm_backward(x: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", grads=None):
    """The gradient of ``wm``: ``(grad_x, grads)`` for ``grad_out`` = dL/d ``wm(x, params)``.  ``grads`` maps the 17 keys ``wm`` reads
    (``prefix`` included) to gradients of the parameters' shapes (``wm_param_shapes``; ``model1.conv1d.weight``: ``[Di, 1, 4]``);
    ``model2`` and ``softmax`` are never called by the reference and have none.  Passing the ``grads`` of an earlier call ADDS to its
    tensors; ``grad_x`` is always a new tensor.  The forward intermediates are recomputed: nothing is kept from a ``wm`` call, and
    ``x``, ``grad_out`` and ``params`` are not written."""
    return _block_backward("wm", _WM_KEYS, wm_param_shapes, x, params, grad_out, prefix, grads)


def feb_param_shapes(nc: int):
    """Names and shapes of the 10 tensors ``feb`` reads, in the order of the C ABI's pointer array."""
    return {k: ((nc, nc, 1, 1) if k.endswith("weight") else (nc,)) for k in _FEB_KEYS}


def ffab_param_shapes(nc: int):
    """Names and shapes of the 92 tensors ``ffab`` reads, in the order of the C ABI's pointer array: the four ``nc`` ProcessBlocks,
    then ``conv4`` / ``conv5`` / ``convout``, each a ``2 nc`` ProcessBlock and a 1x1 back to ``nc``."""
    shapes = {}
    for k in _FFAB_KEYS:
        head = k.split(".")[0]
        if head in ("conv4", "conv5", "convout"):
            c = 2 * nc
            shapes[k] = ((nc, c, 1, 1) if k.endswith("weight") else (nc,)) if k.split(".")[1] == "1" else ((c, c, 1, 1) if k.endswith("weight") else (c,))
        else:
            shapes[k] = (nc, nc, 1, 1) if k.endswith("weight") else (nc,)
    return shapes


def rfft2_polar_backward(x: torch.Tensor, grad_mag: torch.Tensor, grad_pha: torch.Tensor) -> torch.Tensor:
    """The gradient of ``rfft2_polar``: ``grad_x`` for ``grad_mag`` = dL/d ``mag`` and ``grad_pha`` = dL/d ``pha``.  The spectrum of
    ``x`` is recomputed; where it is exactly 0 both maps pass no gradient (torch's ``abs`` / ``angle`` backward)."""
    x, grad_mag, grad_pha = _chk(x, "x"), _chk(grad_mag, "grad_mag"), _chk(grad_pha, "grad_pha")
    if x.dim() != 4:
        raise RuntimeError(f"rfft2_polar_backward: expected a 4-D x, got {tuple(x.shape)}")
    b, c, h, w = x.shape
    if tuple(grad_mag.shape) != (b, c, h, w // 2 + 1) or tuple(grad_pha.shape) != tuple(grad_mag.shape):
        raise RuntimeError(f"rfft2_polar_backward: grad_mag / grad_pha must be {(b, c, h, w // 2 + 1)}, got {tuple(grad_mag.shape)} and "
                           f"{tuple(grad_pha.shape)}")
    scratch = _lib.scratch("rf_rfft2_polar_backward_scratch_bytes", x, b * c, h, w)
    grad_x = torch.empty_like(x)
    _lib.launch("rf_rfft2_polar_backward", x, x, grad_mag, grad_pha, grad_x, scratch, b * c, h, w)
    return grad_x


def polar_irfft2_backward(mag: torch.Tensor, pha: torch.Tensor, grad_out: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The gradient of ``polar_irfft2``: ``(grad_mag, grad_pha)`` for ``grad_out`` = dL/d ``polar_irfft2(mag, pha, grad_out.shape[-1])``."""
    mag, pha, grad_out = _chk(mag, "mag"), _chk(pha, "pha"), _chk(grad_out, "grad_out")
    if grad_out.dim() != 4:
        raise RuntimeError(f"polar_irfft2_backward: expected a 4-D grad_out, got {tuple(grad_out.shape)}")
    b, c, h, w = grad_out.shape
    if tuple(mag.shape) != (b, c, h, w // 2 + 1) or tuple(pha.shape) != tuple(mag.shape):
        raise RuntimeError(f"polar_irfft2_backward: mag / pha must be {(b, c, h, w // 2 + 1)}, got {tuple(mag.shape)} and {tuple(pha.shape)}")
    scratch = _lib.scratch("rf_polar_irfft2_backward_scratch_bytes", mag, b * c, h, w)
    grad_mag, grad_pha = torch.empty_like(mag), torch.empty_like(mag)
    _lib.launch("rf_polar_irfft2_backward", mag, mag, pha, grad_out, grad_mag, grad_pha, scratch, b * c, h, w)
    return grad_mag, grad_pha


def _grads(grads, prefix, keys, shapes, like, who, zeros=()):
    """The parameter gradients a backward operator writes, as ``(grads, its tensors in the order of keys, accumulate)``: new ones
    of ``shapes`` beside ``like``, a checked tensor (``zeros``: the keys the operator may leave unwritten), or the caller's own, which the
    operator adds to in place: they must be contiguous and of ``shapes``."""
    accumulate = grads is not None
    if grads is None:
        grads = {prefix + k: (like.new_zeros if k in zeros else like.new_empty)(tuple(shapes[k])) for k in keys}
    gs = _shaped(grads, prefix, keys, shapes, f"{who} (grads)")
    if any(t is not grads[prefix + k] for k, t in zip(keys, gs)):
        raise RuntimeError(f"{who}: the tensors of grads must be contiguous (they are written in place)")
    return grads, gs, int(accumulate)


def _backward(name, keys, shapes, x, params, grad_out, prefix, grads, geometry, trailing=(), buffers=(), extra=()):
    """What the ``*_backward`` wrappers share, ``x`` and ``grad_out`` checked by the caller: ``params`` and ``grads`` against
    ``shapes``, the workspace ``rf_<name>_backward_workspace_bytes(*geometry)`` asks for, and the call
    ``rf_<name>_backward(x, *extra, grad_out, grad_x, params, grads, workspace, bytes, *geometry, *trailing, accumulate, stream)``.
    ``buffers``: keys of ``shapes`` that the operator reads behind its parameters and that have no gradient.  ``extra``: checked
    tensors the operator reads beside ``x`` and that have no gradient either."""
    read = _shaped(params, prefix, tuple(keys) + tuple(buffers), shapes, f"{name}_backward")
    grads, gs, accumulate = _grads(grads, prefix, keys, shapes, x, f"{name}_backward")
    ws = _lib.scratch(f"rf_{name}_backward_workspace_bytes", x, *geometry)
    grad_x = torch.empty_like(x)
    _lib.launch(f"rf_{name}_backward", x, x, *extra, grad_out, grad_x, read, gs, ws, ws.numel(), *geometry, *trailing, accumulate)
    return grad_x, grads


def _block_backward(name, keys, shapes_of, x, params, grad_out, prefix, grads):
    x, grad_out = _chk(x, "x"), _chk(grad_out, "grad_out")
    if x.dim() != 4 or tuple(grad_out.shape) != tuple(x.shape):
        raise RuntimeError(f"{name}_backward: expected 4-D x and grad_out of one shape, got {tuple(x.shape)} and {tuple(grad_out.shape)}")
    return _backward(name, keys, shapes_of(x.shape[1]), x, params, grad_out, prefix, grads, tuple(x.shape))


def feb_backward(x: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", grads=None):
    """The gradient of ``feb``: ``(grad_x, grads)`` for ``grad_out`` = dL/d ``feb(x, params)``.  ``grads`` maps the 10 keys ``feb`` reads
    (``prefix`` included) to gradients of the parameters' shapes (``feb_param_shapes``).  Passing the ``grads`` of an earlier call ADDS
    to its tensors; ``grad_x`` is always a new tensor.  The forward intermediates are recomputed: nothing is kept from a ``feb``
    call, and ``x``, ``grad_out`` and ``params`` are not written.  The three clamps follow ``torch.clamp``'s backward (the gradient
    passes where ``lo <= v <= hi`` at the value before the clamp)."""
    return _block_backward("feb", _FEB_KEYS, feb_param_shapes, x, params, grad_out, prefix, grads)


def ffab_backward(x: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", grads=None):
    """The gradient of ``ffab``: ``(grad_x, grads)`` for ``grad_out`` = dL/d ``ffab(x, params)``, with ``feb_backward``'s contract and
    the 92 keys of ``ffab_param_shapes``."""
    return _block_backward("ffab", _FFAB_KEYS, ffab_param_shapes, x, params, grad_out, prefix, grads)


_WFB_FF_KEYS = ("project_in.weight", "project_in.bias", "dwconv.weight", "dwconv.bias", "project_out.weight", "project_out.bias",
                "rep_conv1.c.weight", "rep_conv1.bn.weight", "rep_conv1.bn.bias", "rep_conv2.c.weight", "rep_conv2.bn.weight", "rep_conv2.bn.bias")
_WFB_FF_BUFFERS = ("rep_conv1.bn.running_mean", "rep_conv1.bn.running_var", "rep_conv2.bn.running_mean", "rep_conv2.bn.running_var")


def wfb_ff_param_shapes(dim: int, hidden: int):
    """Names and shapes of the 12 parameters of the WFB ``FeedForward`` and, behind them, of the 4 BatchNorm buffers the operators
    below read or update, in the order of the C ABI's pointer array.  The gradients are those of the first 12."""
    shapes = {"project_in.weight": (hidden, dim, 1, 1), "project_in.bias": (hidden,), "dwconv.weight": (hidden, 1, 3, 3), "dwconv.bias": (hidden,),
              "project_out.weight": (dim, hidden, 1, 1), "project_out.bias": (dim,)}
    for name, k in (("rep_conv1", 3), ("rep_conv2", 1)):
        shapes.update({f"{name}.c.weight": (hidden, 1, k, k), f"{name}.bn.weight": (hidden,), f"{name}.bn.bias": (hidden,)})
    shapes.update({k: (hidden,) for k in _WFB_FF_BUFFERS})
    return shapes


def _wfb_ff_geometry(x, params, prefix, who):
    x = _chk(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"{who}: expected a 4-D x, got {tuple(x.shape)}")
    b, dim, h, w = x.shape
    return x, (b, dim, params[prefix + "project_in.weight"].shape[0], h, w)


def wfb_feed_forward_train(x: torch.Tensor, params, prefix: str = "", eps: float = 1e-5, momentum: float = 0.1,
                           update_running_stats: bool = True, batch_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``FeedForward.forward`` under ``train()`` (RawFomer_WFB_FFAB/model.py:42-62): the two ``Conv2d_BN`` branches normalise with
    the statistics of the batch (mean and biased variance over ``(B, h, w)``), which ``wfb_feed_forward``'s eval-mode fold cannot
    express.  With ``update_running_stats`` the four ``running_mean`` / ``running_var`` tensors of ``params`` are updated IN PLACE as
    ``nn.BatchNorm2d`` does (momentum, unbiased variance; they must be contiguous float32 device tensors), and
    ``num_batches_tracked`` is incremented where ``params`` holds it.  ``batch_stats``: a contiguous float32 ``[4, hidden]`` tensor that
    receives ``mu1, v1, mu2, v2``.  Refused where torch raises: fewer than two values per channel."""
    x, geo = _wfb_ff_geometry(x, params, prefix, "wfb_feed_forward_train")
    hidden = geo[2]
    shapes = wfb_ff_param_shapes(geo[1], hidden)
    ts = _shaped(params, prefix, _WFB_FF_KEYS + _WFB_FF_BUFFERS, shapes, "wfb_feed_forward_train")
    if update_running_stats and any(t.data_ptr() != params[prefix + k].data_ptr() for k, t in zip(_WFB_FF_BUFFERS, ts[len(_WFB_FF_KEYS):])):
        raise RuntimeError("wfb_feed_forward_train: the running statistics must be contiguous (they are updated in place)")
    batch_stats = _out(batch_stats, x, "wfb_feed_forward_train", (4, hidden), "batch_stats")
    ws = _lib.scratch("rf_wfb_ffn_train_workspace_bytes", x, *geo)
    out = torch.empty_like(x)
    _lib.launch("rf_wfb_ffn_train_forward", x, x, out, ts, batch_stats, ws, ws.numel(), *geo, float(eps), float(momentum),
                int(update_running_stats))
    if update_running_stats:
        for name in ("rep_conv1", "rep_conv2"):
            nbt = params.get(f"{prefix}{name}.bn.num_batches_tracked")
            if nbt is not None:
                nbt += 1
    return out


def wfb_feed_forward_backward(x: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", grads=None, training: bool = True,
                              eps: float = 1e-5):
    """The gradient of ``wfb_feed_forward_train`` (``training=True``: through the batch statistics) or of the eval-mode
    ``wfb_feed_forward`` (``training=False``: the running statistics are constants): ``(grad_x, grads)`` for ``grad_out`` = dL/d out.
    ``grads`` maps the 12 parameter keys of ``wfb_ff_param_shapes`` (``prefix`` included) to gradients of the parameters' shapes.
    Passing the ``grads`` of an earlier call ADDS to its tensors; ``grad_x`` is always a new tensor.  The forward intermediates and
    the batch statistics are recomputed: nothing is kept from a forward call, and ``x``, ``grad_out`` and ``params`` are not written."""
    x, geo = _wfb_ff_geometry(x, params, prefix, "wfb_feed_forward_backward")
    grad_out = _chk(grad_out, "grad_out")
    if tuple(grad_out.shape) != tuple(x.shape):
        raise RuntimeError(f"wfb_feed_forward_backward: expected x and grad_out of one shape, got {tuple(x.shape)} and {tuple(grad_out.shape)}")
    return _backward("wfb_ffn", _WFB_FF_KEYS, wfb_ff_param_shapes(geo[1], geo[2]), x, params, grad_out, prefix, grads, geo,
                     (int(training), float(eps)), _WFB_FF_BUFFERS)


def _wmb(x, params, prefix, ffn):
    """``WMB.forward`` with ``ffn(y, params, prefix)`` as its FeedForward: the wavelet branch with ``mb`` = ``WM`` on the three high
    bands, then ``x + ffn(norm2(x))``."""
    t = wmb_ll_branch(x, params, prefix, high=lambda hi: wm(hi, params, prefix + "mb."))
    y = layernorm2d(t, params[prefix + "norm2.body.weight"], params.get(prefix + "norm2.body.bias"))
    hid = ffn(y, params, prefix + "ffn.")                       # ffn(y) + y: the operator carries FeedForward's own identity
    return _affine_clamp_add(hid, t, 1.0, 0.0, float("-inf"), float("inf"))     # t + hid (an unbounded clamp is the identity)


def wmb(x: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """``WMB(dim)(x)`` (RawFomer_WFB_FFAB/model.py:203-245), eval mode: the wavelet branch with ``mb`` = ``WM`` on the three high
    bands, then ``x + ffn(norm2(x))``."""
    return _wmb(x, params, prefix, wfb_feed_forward)


def wmb_train(x: torch.Tensor, params, prefix: str = "", eps: float = 1e-5, momentum: float = 0.1,
              update_running_stats: bool = True) -> torch.Tensor:
    """``WMB(dim)(x)`` under ``train()``: ``wmb`` with ``wfb_feed_forward_train`` in place of the folded eval-mode FeedForward, the
    block's only module that train() changes (its two BatchNorms normalise with the statistics of the batch).  With
    ``update_running_stats`` the four ``ffn.rep_conv*.bn.running_*`` tensors of ``params`` are updated IN PLACE, as that operator
    does; ``eps`` and ``momentum`` are the BatchNorms'."""
    return _wmb(x, params, prefix,
                lambda y, p, pre: wfb_feed_forward_train(y, p, pre, eps=eps, momentum=momentum, update_running_stats=update_running_stats))


_WMB_BUFFERS = tuple("ffn." + k for k in _WFB_FF_BUFFERS)


def wmb_param_shapes(c: int, hidden: int):
    """Names and shapes of the 131 parameters of ``WMB(c)`` in ``state_dict`` order -- ``norm1.body.*``, ``illu.*``, ``ffab.*``,
    ``norm2.body.*``, ``ffn.*``, ``mb.*`` (the 17 ``wm`` reads) -- and, behind them, of ffn's 4 BatchNorm buffers: the order of the C
    ABI's pointer array.  ``hidden`` = ``ffn.project_in``'s output channels.  The gradients are those of the first 131."""
    ff = wfb_ff_param_shapes(c, hidden)
    shapes = {"norm1.body.weight": (c,), "norm1.body.bias": (c,)}
    shapes.update({"illu.conv1.weight": (c, c + 1, 1, 1), "illu.conv1.bias": (c,), "illu.depth_conv.weight": (c, 1, 5, 5),
                   "illu.depth_conv.bias": (c,), "illu.conv2.weight": (c, c, 1, 1), "illu.conv2.bias": (c,)})
    shapes.update({"ffab." + k: v for k, v in ffab_param_shapes(c).items()})
    shapes.update({"norm2.body.weight": (c,), "norm2.body.bias": (c,)})
    shapes.update({"ffn." + k: ff[k] for k in _WFB_FF_KEYS})
    shapes.update({"mb." + k: v for k, v in wm_param_shapes(c).items()})
    shapes.update({"ffn." + k: ff[k] for k in _WFB_FF_BUFFERS})
    return shapes


def wmb_backward(x: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", grads=None, training: bool = True, eps: float = 1e-5):
    """The gradient of ``wmb_train`` (``training=True``) or of ``wmb`` (``training=False``: ffn's running statistics are constants):
    ``(grad_x, grads)`` for ``grad_out`` = dL/d out, with ``feb_backward``'s contract and the 131 parameter keys of ``wmb_param_shapes``.
    One schedule over the block's operators on one workspace (csrc/rf_wmb_block_bwd.hip): the forward is recomputed, then
    ``wfb_feed_forward_backward``, ``layernorm2d_backward`` (``residual = grad_out``), ``wmb_back_backward``, ``ffab_backward``,
    ``illumination_estimator_backward``, ``wm_backward`` and ``wmb_front_backward`` (``grad_scale=2``) run in that order, and the result has
    the bits of that composition.  ``illu.conv2.*`` feed only ``illu_map``, which ``WMB.forward`` discards: their gradients are zeros in a
    new ``grads`` and untouched in a passed one.  ``eps`` is the BatchNorms'; the running statistics are read (``training=False``),
    never written.  Needs C % 4 == 0 in 4 .. 512, hidden % 4 == 0, an even height, a width in multiples of 4 and band sides
    (h / 2, w / 2) of 2 .. 4096, at most 2048 when no power of two."""
    x, grad_out = _chk(x, "x"), _chk(grad_out, "grad_out")
    if x.dim() != 4 or tuple(grad_out.shape) != tuple(x.shape):
        raise RuntimeError(f"wmb_backward: expected 4-D x and grad_out of one shape, got {tuple(x.shape)} and {tuple(grad_out.shape)}")
    b, c, h, w = x.shape
    hidden = params[prefix + "ffn.project_in.weight"].shape[0]
    shapes = wmb_param_shapes(c, hidden)
    keys = tuple(k for k in shapes if k not in _WMB_BUFFERS)
    return _backward("wmb", keys, shapes, x, params, grad_out, prefix, grads, (b, c, hidden, h, w), (int(training), float(eps)), _WMB_BUFFERS)


# ------------------------------------------------------------------------------------------ the fused passes of the WFB handle's WMB block
def wmb_front(x: torch.Tensor, weight2: torch.Tensor, bias2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``t = LayerNorm_c(x) * weight2 + bias2`` per pixel and ``dwt_init(t)`` in one pass (csrc/rf_wmb.hip); with ``weight2 = 2 w``,
    ``bias2 = 2 b - 1`` that is ``data_transform(norm1(x))`` and its four bands (WMB.forward, model.py:221-225).
    ``x`` [B,C,2h,2w] with 2w % 4 == 0 -> (t [B,C,2h,2w], bands [4B,C,h,w])."""
    x, weight2, bias2 = _chk(x, "x"), _chk(weight2, "weight2"), _chk(bias2, "bias2")
    b, c, h2, w2 = x.shape
    if h2 % 2 or w2 % 4 or weight2.numel() != c or bias2.numel() != c:
        raise RuntimeError(f"wmb_front: needs an even height, a width in multiples of 4 and {c} LayerNorm weights (got {h2}x{w2})")
    t, bands = torch.empty_like(x), torch.empty((4 * b, c, h2 // 2, w2 // 2), dtype=x.dtype, device=x.device)
    _lib.launch("rf_wmb_front", x, x, t, bands, weight2, bias2, b, c, h2 // 2, w2 // 2)
    return t, bands


def wmb_back(bands: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """``t + clamp((iwt_init(bands) + 1) / 2, 0, 1)`` in one pass (WMB.forward, model.py:239-243)."""
    bands, t = _chk(bands, "bands"), _chk(t, "t")
    b4, c, h, w = bands.shape
    if b4 % 4 or w % 2 or tuple(t.shape) != (b4 // 4, c, 2 * h, 2 * w):
        raise RuntimeError(f"wmb_back: bands {tuple(bands.shape)} and t {tuple(t.shape)} do not belong together (band width must be even)")
    out = torch.empty_like(t)
    _lib.launch("rf_wmb_back", t, bands, t, out, b4 // 4, c, h, w)
    return out


def _grad_pair(grads, like, who):
    """``(pair, accumulate)`` for a ``(grad_weight, grad_bias)`` pair: a new one, or the caller's own, which the call adds to."""
    shapes = {"weight": like.shape, "bias": like.shape}
    named = None if grads is None else dict(zip(shapes, grads, strict=True))
    _, gs, accumulate = _grads(named, "", tuple(shapes), shapes, like, who)
    return (tuple(gs) if grads is None else grads), accumulate


def wmb_front_backward(x: torch.Tensor, weight2: torch.Tensor, bias2: torch.Tensor, grad_t: torch.Tensor, grad_bands: torch.Tensor,
                       grad_scale: float = 1.0, grads=None):
    """The gradient of ``wmb_front``: ``(grad_x, (grad_weight2, grad_bias2))`` for ``grad_t`` = dL/d ``t`` and ``grad_bands`` = dL/d ``bands``.
    One pass: ``g = grad_t + iwt_init(grad_bands)`` (``dwt_init``'s transpose) stays in registers and goes through the LayerNorm
    adjoint.  ``grad_scale`` multiplies the two parameter gradients: a block that passes ``weight2 = 2 w`` gets the gradient of ``w``
    with ``grad_scale=2``.  Passing the ``grads`` pair of an earlier call ADDS to its tensors; ``grad_x`` is always a new tensor.
    ``bias2`` does not enter the gradient and is only checked."""
    x, weight2, bias2 = _chk(x, "x"), _chk(weight2, "weight2"), _chk(bias2, "bias2")
    grad_t, grad_bands = _chk(grad_t, "grad_t"), _chk(grad_bands, "grad_bands")
    b, c, h2, w2 = x.shape
    if (h2 % 2 or w2 % 4 or weight2.numel() != c or bias2.numel() != c or tuple(grad_t.shape) != tuple(x.shape)
            or tuple(grad_bands.shape) != (4 * b, c, h2 // 2, w2 // 2)):
        raise RuntimeError(f"wmb_front_backward: x {tuple(x.shape)}, grad_t {tuple(grad_t.shape)}, grad_bands {tuple(grad_bands.shape)}: needs an "
                           f"even height, a width in multiples of 4, {c} LayerNorm weights and the shapes wmb_front returns")
    pair, acc = _grad_pair(grads, weight2, "wmb_front_backward")
    gw, gb = pair
    geo = (b, c, h2 // 2, w2 // 2)
    ws = _lib.scratch("rf_wmb_front_backward_workspace_bytes", x, *geo)
    grad_x = torch.empty_like(x)
    _lib.launch("rf_wmb_front_backward", x, x, grad_t, grad_x, grad_bands, weight2, gw, gb, ws, ws.numel(), *geo, float(grad_scale), acc)
    return grad_x, pair


def wmb_back_backward(bands: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """The gradient of ``wmb_back`` with respect to ``bands`` (the one with respect to ``t`` is ``grad_out`` itself):
    ``dwt_init(m * grad_out / 2)`` with ``m = 1`` where the value before the clamp lies in [0, 1], as ``torch.clamp``'s backward."""
    bands, grad_out = _chk(bands, "bands"), _chk(grad_out, "grad_out")
    b4, c, h, w = bands.shape
    if b4 % 4 or w % 2 or tuple(grad_out.shape) != (b4 // 4, c, 2 * h, 2 * w):
        raise RuntimeError(f"wmb_back_backward: bands {tuple(bands.shape)} and grad_out {tuple(grad_out.shape)} do not belong together "
                           "(band width must be even)")
    grad_bands = torch.empty_like(bands)
    _lib.launch("rf_wmb_back_backward", bands, bands, grad_out, grad_bands, b4 // 4, c, h, w)
    return grad_bands


def dwconv5x5_backward(x: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, grads=None):
    """The gradient of ``dwconv5x5``: ``(grad_x, grads)`` with ``grads = {"weight": [C,1,5,5], "bias": [C]}``.  Passing the ``grads`` of
    an earlier call ADDS to its tensors; ``grad_x`` is always a new tensor."""
    x, weight, grad_out = _chk(x, "x"), _chk(weight, "weight"), _chk(grad_out, "grad_out")
    b, c, h, w = x.shape
    if tuple(weight.shape) != (c, 1, 5, 5) or tuple(grad_out.shape) != tuple(x.shape):
        raise RuntimeError(f"dwconv5x5_backward: weight {tuple(weight.shape)} / grad_out {tuple(grad_out.shape)} do not match x {tuple(x.shape)}")
    shapes = {"weight": (c, 1, 5, 5), "bias": (c,)}
    grads, gs, acc = _grads(grads, "", tuple(shapes), shapes, x, "dwconv5x5_backward")
    ws = _lib.scratch("rf_dwconv5x5_backward_workspace_bytes", x, b, c, h, w)
    grad_x = torch.empty_like(x)
    _lib.launch("rf_dwconv5x5_backward", x, x, grad_out, grad_x, weight, *gs, ws, ws.numel(), b, c, h, w, acc)
    return grad_x, grads


_ILLU_KEYS = ("conv1.weight", "conv1.bias", "depth_conv.weight", "depth_conv.bias", "conv2.weight", "conv2.bias")


def illumination_estimator_backward(img: torch.Tensor, params, grad_fea: torch.Tensor, grad_map: Optional[torch.Tensor] = None,
                                    prefix: str = "", grads=None):
    """The gradient of ``illumination_estimator``: ``(grad_img, grads)`` for ``grad_fea`` = dL/d ``illu_fea`` and, optionally, ``grad_map``
    = dL/d ``illu_map``; ``grads`` holds the six keys ``conv1.*``, ``depth_conv.*``, ``conv2.*`` (``prefix`` included).  ``x1`` is
    recomputed, ``illu_fea`` only when ``grad_map`` is given.  Without ``grad_map`` (``WMB.forward`` discards ``illu_map``) the two
    ``conv2.*`` gradients are zeros in a new ``grads`` and untouched in a passed one.  Passing the ``grads`` of an earlier call ADDS to
    its tensors; ``grad_img`` is always a new tensor.  All three channel counts must be multiples of 4 in 4 .. 512."""
    img, grad_fea = _chk(img, "img"), _chk(grad_fea, "grad_fea")
    b, c, h, w = img.shape
    cm, co = params[prefix + "conv1.weight"].shape[0], params[prefix + "conv2.weight"].shape[0]
    shapes = {"conv1.weight": (cm, c + 1, 1, 1), "conv1.bias": (cm,), "depth_conv.weight": (cm, 1, 5, 5), "depth_conv.bias": (cm,),
              "conv2.weight": (co, cm, 1, 1), "conv2.bias": (co,)}
    ts = _shaped(params, prefix, _ILLU_KEYS, shapes, "illumination_estimator_backward")
    if tuple(grad_fea.shape) != (b, cm, h, w):
        raise RuntimeError(f"illumination_estimator_backward: grad_fea {tuple(grad_fea.shape)}, expected {(b, cm, h, w)}")
    if grad_map is not None:
        grad_map = _chk(grad_map, "grad_map")
        if tuple(grad_map.shape) != (b, co, h, w):
            raise RuntimeError(f"illumination_estimator_backward: grad_map {tuple(grad_map.shape)}, expected {(b, co, h, w)}")
    grads, gs, acc = _grads(grads, prefix, _ILLU_KEYS, shapes, img, "illumination_estimator_backward",
                            zeros=() if grad_map is not None else ("conv2.weight", "conv2.bias"))
    geo = (b, c, cm, co, h, w)
    ws = _lib.scratch("rf_illumination_estimator_backward_workspace_bytes", img, *geo, int(grad_map is not None))
    grad_img = torch.empty_like(img)
    _lib.launch("rf_illumination_estimator_backward", img, img, grad_fea, grad_map, grad_img, ts, gs, ws, ws.numel(), *geo, acc)
    return grad_img, grads


def layernorm2d_backward(x: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, residual: Optional[torch.Tensor] = None,
                         eps: float = 1e-5, grads=None):
    """The gradient of ``layernorm2d`` (with bias): ``(grad_x, grads)`` with ``grads = {"weight": [C], "bias": [C]}``; ``residual`` is
    added to ``grad_x`` (``grad_u = grad_out + LN^T(grad_v)`` of a pre-norm block in one pass).  Passing the ``grads`` of an earlier
    call ADDS to its tensors; ``grad_x`` is always a new tensor."""
    x, weight, grad_out = _chk(x, "x"), _chk(weight, "weight"), _chk(grad_out, "grad_out")
    b, c, h, w = x.shape
    if weight.numel() != c or tuple(grad_out.shape) != tuple(x.shape) or (residual is not None and tuple(residual.shape) != tuple(x.shape)):
        raise RuntimeError(f"layernorm2d_backward: x {tuple(x.shape)}, grad_out {tuple(grad_out.shape)}: equal shapes and {c} weights are needed")
    residual = _opt(residual, "residual")
    shapes = {"weight": (c,), "bias": (c,)}
    grads, gs, acc = _grads(grads, "", tuple(shapes), shapes, x, "layernorm2d_backward")
    ws = _lib.scratch("rf_layernorm2d_backward_workspace_bytes", x, b, c, h, w)
    grad_x = torch.empty_like(x)
    _lib.launch("rf_layernorm2d_backward", x, x, grad_out, grad_x, weight, *gs, residual, ws, ws.numel(), b, c, h, w, float(eps), acc)
    return grad_x, grads


def wmb_ffn_tail(t: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``t + y + LayerNorm_c(t)``: the end of ``x + ffn(norm2(x))`` with ``y = project_out(..)``, FeedForward's identity
    ``norm2(x)`` recomputed per pixel instead of stored (model.py:58-65, 244)."""
    t, y, weight, bias = _chk(t, "t"), _chk(y, "y"), _chk(weight, "weight"), _chk(bias, "bias")
    b, c, h, w = t.shape
    if w % 4 or tuple(y.shape) != tuple(t.shape) or weight.numel() != c or bias.numel() != c:
        raise RuntimeError(f"wmb_ffn_tail: t {tuple(t.shape)}, y {tuple(y.shape)}: equal shapes and a width in multiples of 4 are needed")
    out = torch.empty_like(t)
    _lib.launch("rf_wmb_ffn_sum", t, t, y, out, weight, bias, b, c, h, w)
    return out


# ------------------------------------------------------------------------------------------ the TrueColor variant's kernels one by one
def tc_spatial(feat: torch.Tensor, guide: torch.Tensor, params, prefix: str = "", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The spatial gate of ``EnhancedFLCA.forward`` (BayerTORGBColorMultiLvl.py:277-283) given the seven guidance planes
    ``guide`` [B,7,h,w] at the feature size: ``feat * (1 + sigmoid(color_attention(guide[:, 0:5])) + tanh(sigmoid(low_attn(guide[:, 5:6]))
    + tanh(high_attn(guide[:, 6:7]))))``.  ``params``: the block's ``state_dict`` (``color_attention.0.*``, ``low_attn.0.*``,
    ``high_attn.0.*``).  ``out``: where to write (default: a new tensor)."""
    feat, guide = _chk(feat, "feat"), _chk(guide, "guide")
    b, c, h, w = feat.shape
    if tuple(guide.shape) != (b, 7, h, w):
        raise RuntimeError(f"tc_spatial: guide must be {(b, 7, h, w)}, got {tuple(guide.shape)}")
    shapes = {"color_attention.0.weight": (c, 5, 3, 3), "color_attention.0.bias": (c,), "low_attn.0.weight": (c, 1, 3, 3),
              "low_attn.0.bias": (c,), "high_attn.0.weight": (c, 1, 3, 3), "high_attn.0.bias": (c,)}
    prm = _shaped(params, prefix, tuple(shapes), shapes, "tc_spatial")
    out = _out(out, feat, "tc_spatial")
    _lib.launch("rf_tc_spatial", feat, feat, guide, *prm, out, b, c, h, w)
    return out


def tc_nblk(h: int, w: int) -> int:
    """Blocks per image of ``tc_residual``'s pooling sums: 1024 consecutive pixels each where ``w % 4 == 0``, else 256."""
    n = _lib.load().rf_tc_nblk(int(h), int(w))     # a count, or a negative status: neither of _lib's two size conventions
    _lib.check(min(n, 0), "rf_tc_nblk")
    return n


def tc_residual(xs: torch.Tensor, r: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x2 = xs + 0.2 tanh(r)`` (EnhancedFLCA.forward, BayerTORGBColorMultiLvl.py:285-288; ``r = res_proj(xs)``) and the
    squeeze-excite pooling sums ``partial`` [B, tc_nblk(h, w), C]: entry ``[b, k, c]`` is the sum of ``x2[b, c]`` over block ``k`` of
    the flattened plane.  ``out`` may be ``xs`` itself (the forward writes in place)."""
    xs, r = _chk(xs, "xs"), _chk(r, "r")
    b, c, h, w = xs.shape
    if tuple(r.shape) != tuple(xs.shape):
        raise RuntimeError(f"tc_residual: xs {tuple(xs.shape)} and r {tuple(r.shape)} differ")
    out = _out(out, xs, "tc_residual")
    if c > 512:
        raise RuntimeError(f"tc_residual: C={c} > 512 not supported")
    partial = torch.empty((b, tc_nblk(h, w), c), dtype=torch.float32, device=xs.device)
    _lib.launch("rf_tc_residual", xs, xs, r, out, partial, b, c, h, w)
    return out, partial


def tc_color_head(x: torch.Tensor, params, prefix: str = "") -> torch.Tensor:
    """``CameraAwareColorCorrection()(x)`` (BayerTORGBColorMultiLvl.py:160-176) on ``x`` [B,3,...]: clamp, ``pow(1 / gamma)``, the
    3 -> 64 -> 3 colour transform, the per-channel tone curve, clamp.  ``params``: the module's ``state_dict``.  A new tensor."""
    x = _chk(x, "x")
    if x.dim() < 3 or x.shape[1] != 3:
        raise RuntimeError(f"tc_color_head: expected [B,3,...], got {tuple(x.shape)}")
    counts = {"gamma_param": 1, "color_transform.0.weight": 192, "color_transform.0.bias": 64, "color_transform.2.weight": 192,
              "color_transform.2.bias": 3, "tone_curve.0.weight": 32, "tone_curve.0.bias": 32, "tone_curve.2.weight": 32,
              "tone_curve.2.bias": 1}
    prm = _shaped(params, prefix, tuple(counts), counts, "tc_color_head")      # element counts, not shapes
    out = x.clone()
    _lib.launch("rf_tc_color_head", x, out, *prm, x.shape[0], x[0, 0].numel())
    return out


def tc_pyramid(src: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One level of ``EnhancedFLCA._pyramid_y`` (BayerTORGBColorMultiLvl.py:236-247) on planes ``src`` [B,1,h,w]: the Haar LL band and
    the high-band magnitude ``sqrt(LH^2 + HL^2 + HH^2 + 1e-8)``, each [B,1,ceil(h/2),ceil(w/2)]; an odd side is reflect-padded."""
    src = _chk(src, "src")
    if src.dim() != 4 or src.shape[1] != 1:
        raise RuntimeError(f"tc_pyramid: expected [B,1,h,w], got {tuple(src.shape)}")
    b, _, h, w = src.shape
    ll = torch.empty((b, 1, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=src.device)
    mag = torch.empty_like(ll)
    _lib.launch("rf_tc_pyramid", src, src, ll, mag, b, h, w)
    return ll, mag


# ------------------------------------------------------------------------------------------ the multi-level variant's kernels one by one
def _ml_step_params(params, prefix: str, step: int, levels: int, c: int, who: str):
    """The weights of one residual step of ``FLCA_Pyramid`` from the block's ``state_dict``: ``(w_a, w_b, gate_w, gate_b)``."""
    if step == levels:
        keys = ("chroma_attn.0.weight", None, "chroma_gate.weight", "chroma_gate.bias")
        shapes = {"chroma_attn.0.weight": (c, 2, 3, 3), "chroma_gate.weight": (1, 1, 1, 1), "chroma_gate.bias": (1,)}
    else:
        keys = (f"low_attn.{step}.0.weight", f"high_attn.{step}.0.weight", f"freq_gate_head.{step}.weight", f"freq_gate_head.{step}.bias")
        shapes = dict(zip(keys, ((c, 1, 3, 3), (c, 1, 3, 3), (2, 2, 1, 1), (2,))))
    return _shaped(params, prefix, keys, shapes, who)


def _ml_step_inputs(x, guide, means, step, levels, who):
    x, guide, means = _chk(x, "x"), _chk(guide, "guide"), _chk(means, "means")
    if x.dim() != 4:
        raise RuntimeError(f"{who}: expected x [B,C,h,w], got {tuple(x.shape)}")
    b, c, h, w = x.shape
    step, levels = int(step), int(levels)
    if not 1 <= levels <= 3 or not 0 <= step <= levels:
        raise RuntimeError(f"{who}: levels={levels} must be 1..3 and step={step} 0..levels")
    if tuple(guide.shape) != (b, 2 * levels + 2, h, w):
        raise RuntimeError(f"{who}: guide must be {(b, 2 * levels + 2, h, w)}, got {tuple(guide.shape)}")
    if tuple(means.shape) != (b, 8):
        raise RuntimeError(f"{who}: means must be {(b, 8)}, got {tuple(means.shape)}")
    return x, guide, means, step, levels


def ml_modulate(x: torch.Tensor, guide: torch.Tensor, means: torch.Tensor, step: int, levels: int, params, prefix: str = "",
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gated spatial attention of one step of ``FLCA_Pyramid.forward`` (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py
    :147-162, :170-173) applied to ``x`` [B,C,h,w].  ``guide`` [B,2 levels+2,h,w] and ``means`` [B,8] as ``RawFormer.ml_guidance``
    returns them; ``step`` < ``levels`` is that pyramid level, ``step == levels`` the chroma form.  ``params``: the block's
    ``state_dict``.  ``out``: where to write (default: a new tensor)."""
    x, guide, means, step, levels = _ml_step_inputs(x, guide, means, step, levels, "ml_modulate")
    b, c, h, w = x.shape
    prm = _ml_step_params(params, prefix, step, levels, c, "ml_modulate")
    out = _out(out, x, "ml_modulate")
    _lib.launch("rf_ml_modulate", x, x, guide, means, step, levels, *prm, out, b, c, h, w)
    return out


def ml_step_fused(x: torch.Tensor, guide: torch.Tensor, means: torch.Tensor, step: int, levels: int, params, prefix: str = "",
                  out: Optional[torch.Tensor] = None, sums: bool = False):
    """One whole residual step of ``FLCA_Pyramid.forward`` in one kernel: ``x + 0.2 tanh(res_proj(ml_modulate(x, ...)))`` for
    C = 16, 32, 48 or 64, ``w % 4 == 0`` and ``h * w % 64 == 0`` (anything else raises).  Arguments as ``ml_modulate``; ``params``
    also holds ``res_proj.0.*`` and ``res_proj.2.*``.  ``out`` may be ``x``.  With ``sums`` returns ``(out, partial)``, ``partial``
    [B, tc_nblk(h, w), C] the sums of ``out`` over each block of 1024 consecutive pixels (``tc_residual``'s layout)."""
    x, guide, means, step, levels = _ml_step_inputs(x, guide, means, step, levels, "ml_step_fused")
    b, c, h, w = x.shape
    prm = _ml_step_params(params, prefix, step, levels, c, "ml_step_fused")
    res = {"res_proj.0.weight": (c, c, 1, 1), "res_proj.0.bias": (c,), "res_proj.2.weight": (c, c, 1, 1), "res_proj.2.bias": (c,)}
    prm += _shaped(params, prefix, tuple(res), res, "ml_step_fused")
    out = _out(out, x, "ml_step_fused")
    # the library refuses an unsupported shape before it reads `partial`: one block of 1024 pixels is the most any shape needs there
    partial = torch.empty((b, -(-h * w // 1024), c), dtype=torch.float32, device=x.device) if sums else None
    _lib.launch("rf_ml_step_fused", x, x, guide, means, step, levels, *prm, out, partial, b, c, h, w)
    return (out, partial) if sums else out


def ml_residual(x: torch.Tensor, r: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x + 0.2 tanh(r)`` (FLCA_Pyramid.forward, :162-165; ``r = res_proj(x * attention)``), tensors of any one shape.  ``out`` may
    be ``x`` itself (the forward writes in place)."""
    x, r = _chk(x, "x"), _chk(r, "r")
    if tuple(r.shape) != tuple(x.shape):
        raise RuntimeError(f"ml_residual: x {tuple(x.shape)} and r {tuple(r.shape)} differ")
    if x.numel() == 0:
        raise RuntimeError("ml_residual: empty tensor")
    out = _out(out, x, "ml_residual")
    b, c, h, w = x.shape if x.dim() == 4 else (1, 1, 1, x.numel())
    _lib.launch("rf_ml_residual", x, x, r, out, b, c, h, w)
    return out


# ------------------------------------------------------------------------------------------ FLCA_Pyramid as an operator, and its gradient
def flca_pyramid_param_shapes(c: int, levels: int = 2):
    """Names and shapes of the 4 ``levels`` + 11 tensors ``flca_pyramid`` reads, in the order of the reference's ``state_dict`` (=
    the C ABI's pointer array).  The squeeze-excite hidden width is ``max(8, c // 8)``."""
    hid = max(8, c // 8)
    shapes = {f"low_attn.{l}.0.weight": (c, 1, 3, 3) for l in range(levels)}
    shapes.update({f"high_attn.{l}.0.weight": (c, 1, 3, 3) for l in range(levels)})
    for l in range(levels):
        shapes.update({f"freq_gate_head.{l}.weight": (2, 2, 1, 1), f"freq_gate_head.{l}.bias": (2,)})
    shapes.update({"chroma_attn.0.weight": (c, 2, 3, 3), "chroma_gate.weight": (1, 1, 1, 1), "chroma_gate.bias": (1,),
                   "se.1.weight": (hid, c, 1, 1), "se.1.bias": (hid,), "se.3.weight": (c, hid, 1, 1), "se.3.bias": (c,),
                   "res_proj.0.weight": (c, c, 1, 1), "res_proj.0.bias": (c,), "res_proj.2.weight": (c, c, 1, 1), "res_proj.2.bias": (c,)})
    return shapes


def _flca_pyramid_inputs(feat, x4, levels, who):
    feat, x4 = _chk(feat, "feat"), _chk(x4, "x4")
    if feat.dim() != 4 or x4.dim() != 4 or x4.shape[1] != 4 or x4.shape[0] != feat.shape[0]:
        raise RuntimeError(f"{who}: expected feat [B,C,h,w] and packed RGGB x4 [B,4,H,W], got {tuple(feat.shape)} and {tuple(x4.shape)}")
    b, c, h, w = feat.shape
    return feat, x4, (b, c, h, w, x4.shape[2], x4.shape[3], int(levels))


def flca_pyramid(feat: torch.Tensor, x4: torch.Tensor, params, prefix: str = "", levels: int = 2) -> torch.Tensor:
    """``FLCA_Pyramid(channels, levels)(feat, *BayerLumaChroma()(x4))`` (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py
    :86-183): the guidance pyramid from the packed RGGB frame ``x4`` [B,4,H,W] resized to ``feat``'s size, ``levels`` + 1 gated
    residual steps through one ``res_proj``, squeeze-excite.  ``params``: the block's ``state_dict`` (``flca_pyramid_param_shapes``).
    1 <= C <= 512, ``levels`` 1..3, H and W multiples of 8, any feature size; anything else raises with the library's message."""
    feat, x4, geometry = _flca_pyramid_inputs(feat, x4, levels, "flca_pyramid")
    ws = _lib.scratch("rf_flca_pyramid_workspace_bytes", feat, *geometry)
    shapes = flca_pyramid_param_shapes(feat.shape[1], geometry[-1])
    ts = _shaped(params, prefix, tuple(shapes), shapes, "flca_pyramid")
    out = torch.empty_like(feat)
    _lib.launch("rf_flca_pyramid_forward", feat, feat, x4, out, ts, ws, ws.numel(), *geometry)
    return out


def flca_pyramid_backward(feat: torch.Tensor, x4: torch.Tensor, params, grad_out: torch.Tensor, prefix: str = "", levels: int = 2,
                          grads=None):
    """The gradient of ``flca_pyramid``: ``(grad_feat, grads)`` for ``grad_out`` = dL/d ``flca_pyramid(feat, x4, params)``.  ``grads``
    maps the 4 ``levels`` + 11 keys (``prefix`` included) to gradients of the parameters' shapes; ``x4`` and the guidance carry no
    gradient.  Passing the ``grads`` of an earlier call ADDS to its tensors; ``grad_feat`` is always a new tensor.  The forward
    intermediates are recomputed: nothing is kept from a ``flca_pyramid`` call, and ``feat``, ``x4``, ``grad_out`` and ``params``
    are not written."""
    feat, x4, geometry = _flca_pyramid_inputs(feat, x4, levels, "flca_pyramid_backward")
    grad_out = _chk(grad_out, "grad_out")
    if tuple(grad_out.shape) != tuple(feat.shape):
        raise RuntimeError(f"flca_pyramid_backward: feat {tuple(feat.shape)} and grad_out {tuple(grad_out.shape)} differ")
    _lib.size("rf_flca_pyramid_backward_workspace_bytes", *geometry)      # an unsupported geometry raises here, with the library's message
    shapes = flca_pyramid_param_shapes(feat.shape[1], geometry[-1])
    return _backward("flca_pyramid", tuple(shapes), shapes, feat, params, grad_out, prefix, grads, geometry, extra=(x4,))


def ml_tail_backward(grad_out: torch.Tensor) -> torch.Tensor:
    """The adjoint of the multi-level variant's output corrections (``RawFormer.ml_tail``; MultiLvlFrequencyawareLumaChromaAttention
    RAWFormer.py:270-288, :403-414) with respect to the image: ``grad_image`` [B,3,h2,w2] for ``grad_out`` = dL/d (corrected image).
    The map is affine in the image with constant coefficients, so nothing else is read."""
    grad_out = _chk(grad_out, "grad_out")
    if grad_out.dim() != 4 or grad_out.shape[1] != 3:
        raise RuntimeError(f"ml_tail_backward: expected grad_out [B,3,h2,w2], got {tuple(grad_out.shape)}")
    b, _, h2, w2 = grad_out.shape
    ws = _lib.scratch("rf_ml_corrections_backward_workspace_bytes", grad_out, b, h2, w2)
    grad_image = torch.empty_like(grad_out)
    _lib.launch("rf_ml_corrections_backward", grad_out, grad_out, grad_image, ws, ws.numel(), b, h2, w2)
    return grad_image
