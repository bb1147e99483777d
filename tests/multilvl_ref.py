"""CPU restatement of ``RawFormer(variant='multilvl')`` in plain torch, written from the mathematics (DESIGN.md section 4,
"multi-level FLCA"): the oracle for shapes that have no fixture.  The shared pieces (TransformerBlock, Haar step, bilinear
resize, Bayer luma / chroma, U-Net resampling) are the operator restatements of ``oracle/rawformer_ref.py``.

Works in the dtype of its inputs, so a float64 state_dict and input give a float64 forward."""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import rawformer_ref as R


def pyramid(y: Tensor, levels: int, eps: float = 1e-8) -> Tuple[List[Tensor], List[Tensor]]:
    """``LL_l`` and ``sqrt(LH^2 + HL^2 + HH^2 + eps)`` of every Haar level of ``y``."""
    lows, highs, cur = [], [], y
    for _ in range(levels):
        ll, (lh, hl, hh) = R.haar_dwt(cur)
        lows.append(ll)
        highs.append(torch.sqrt(lh * lh + hl * hl + hh * hh + eps))
        cur = ll
    return lows, highs


def res_step(x: Tensor, spatial: Tensor, p: Dict[str, Tensor], pre: str) -> Tensor:
    """``x + 0.2 tanh(res_proj(x * spatial))`` with res_proj = 1x1, ReLU, 1x1."""
    t = torch.relu(F.conv2d(x * spatial, p[pre + "res_proj.0.weight"], p[pre + "res_proj.0.bias"]))
    return x + 0.2 * torch.tanh(F.conv2d(t, p[pre + "res_proj.2.weight"], p[pre + "res_proj.2.bias"]))


def step_gate(a: Tensor, b: Tensor, p: Dict[str, Tensor], pre: str, step: int, levels: int, eps: float = 1e-8) -> Tensor:
    """The gated spatial attention of residual step ``step`` of FLCA_Pyramid from its two planes at the feature size:
    ``step < levels``: (y_low, y_high) of pyramid level ``step`` -> ``g0 sigmoid(conv3(y_low)) + g1 tanh(conv3(y_high))`` with
    ``(g0, g1) = sigmoid(freq_gate_head(mean y_low, mean y_high))``; ``step == levels``: (cr, cb) ->
    ``sigmoid(chroma_gate(mean sqrt(cr^2 + cb^2 + eps))) sigmoid(conv3([cr, cb]))``.  The means are those of the planes given."""
    if step == levels:
        a_chr = torch.sigmoid(F.conv2d(torch.cat([a, b], dim=1), p[pre + "chroma_attn.0.weight"], padding=1))
        mag = torch.sqrt(a * a + b * b + eps).mean(dim=(2, 3), keepdim=True)
        return torch.sigmoid(F.conv2d(mag, p[pre + "chroma_gate.weight"], p[pre + "chroma_gate.bias"])) * a_chr
    a_low = torch.sigmoid(F.conv2d(a, p[f"{pre}low_attn.{step}.0.weight"], padding=1))
    a_high = torch.tanh(F.conv2d(b, p[f"{pre}high_attn.{step}.0.weight"], padding=1))
    pooled = torch.cat([a.mean(dim=(2, 3), keepdim=True), b.mean(dim=(2, 3), keepdim=True)], dim=1)      # means at THIS size
    gates = torch.sigmoid(F.conv2d(pooled, p[f"{pre}freq_gate_head.{step}.weight"], p[f"{pre}freq_gate_head.{step}.bias"]))
    return gates[:, 0:1] * a_low + gates[:, 1:2] * a_high


def flca_pyramid(feat: Tensor, guide, p: Dict[str, Tensor], pre: str, levels: int, eps: float = 1e-8) -> Tensor:
    y, cr, cb = guide
    size = feat.shape[-2:]
    lows, highs = pyramid(y, levels, eps)
    x = feat
    for l in range(levels):
        x = res_step(x, step_gate(R.bilinear_resize(lows[l], size), R.bilinear_resize(highs[l], size), p, pre, l, levels, eps), p, pre)
    x = res_step(x, step_gate(R.bilinear_resize(cr, size), R.bilinear_resize(cb, size), p, pre, levels, levels, eps), p, pre)
    pooled = x.mean(dim=(2, 3), keepdim=True)
    hid = torch.relu(F.conv2d(pooled, p[pre + "se.1.weight"], p[pre + "se.1.bias"]))
    return x * torch.sigmoid(F.conv2d(hid, p[pre + "se.3.weight"], p[pre + "se.3.bias"]))


def stage(x: Tensor, guide, p: Dict[str, Tensor], pre: str, heads: int, levels: int = 2) -> Tensor:
    """One ``conv_tran<i>``: lrelu(Conv_out(channel_reduce(cat[FLCA(x), Transformer(x)])))."""
    branch = flca_pyramid(x, guide, p, pre + "FLCA.", levels)
    trans = R.transformer_block(x, p, pre + "Transformer.", heads)
    t = F.conv2d(torch.cat([branch, trans], dim=1), p[pre + "channel_reduce.weight"], p[pre + "channel_reduce.bias"])
    return F.leaky_relu(F.conv2d(t, p[pre + "Conv_out.weight"], p[pre + "Conv_out.bias"], padding=1), 0.2)


def corrections(out: Tensor, x4: Tensor, y: Tensor, resize=R.bilinear_resize, anchor_level: int = 2) -> Tensor:
    """Colour anchor ``out += 0.12 (in_mean - out_mean)`` then the nudge ``out += 0.03 (up(LL2) - luma(out))``.  ``resize`` and
    ``anchor_level`` are the model's (bilinear, align_corners=False; LL2); tests that inject a defect pass others."""
    rgb = torch.cat([x4[:, 0:1], 0.5 * (x4[:, 1:2] + x4[:, 2:3]), x4[:, 3:4]], dim=1)
    in_mean = resize(rgb, out.shape[-2:]).mean(dim=(2, 3), keepdim=True)
    out = out + 0.12 * (in_mean - out.mean(dim=(2, 3), keepdim=True))
    ll2 = pyramid(y, anchor_level)[0][anchor_level - 1]
    out_y = 0.299 * out[:, 0:1] + 0.587 * out[:, 1:2] + 0.114 * out[:, 2:3]
    return out + 0.03 * (resize(ll2, out.shape[-2:]) - out_y)


def forward(p: Dict[str, Tensor], x: Tensor, dim: int, heads=(8, 8, 8, 8), levels: int = 2, packed: bool = False) -> Tensor:
    """Mosaic ``[B,1,2H,2W]`` (or packed ``[B,4,H,W]``) -> ``[B,3,2H,2W]``."""
    x4 = x if packed else R.pixel_unshuffle2(x)
    guide = R.bayer_luma_chroma(x4)
    t = F.conv2d(x4, p["embedding.weight"], p["embedding.bias"], padding=1)
    e1 = stage(t, guide, p, "conv_tran1.", heads[0], levels)
    e2 = stage(R.downsample(e1, p["down1.0.weight"]), guide, p, "conv_tran2.", heads[1], levels)
    e3 = stage(R.downsample(e2, p["down2.0.weight"]), guide, p, "conv_tran3.", heads[2], levels)
    e4 = stage(R.downsample(e3, p["down3.0.weight"]), guide, p, "conv_tran4.", heads[3], levels)

    def up(t_in, skip, i):
        u = R.conv_transpose2x2(t_in, p[f"up{i}.weight"], p[f"up{i}.bias"])
        return F.conv2d(torch.cat([u, skip], dim=1), p[f"channel_reduce{i}.weight"], p[f"channel_reduce{i}.bias"])

    d3 = stage(up(e4, e3, 1), guide, p, "conv_tran5.", heads[2], levels)
    d2 = stage(up(d3, e2, 2), guide, p, "conv_tran6.", heads[1], levels)
    d1 = stage(up(d2, e1, 3), guide, p, "conv_tran7.", heads[0], levels)
    out = R.pixel_shuffle2(F.leaky_relu(F.conv2d(d1, p["conv_out.weight"], p["conv_out.bias"], padding=1), 0.2))
    return corrections(out, x4, guide[0])
