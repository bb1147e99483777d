"""Plain-torch restatements of the operators behind csrc/rf_tokattn.hip, rf_wfb.hip and rf_upcat.hip:

    token_attention      softmax(q k^T scale) v per (image, head), tokens = pixels           (Attenblock.py:190-191, 212-217)
    luma_film            gamma t + beta on q, k, v; q += alpha (avgpool3(1 - luma) - mean)   (Attenblock.py:193-210)
    bayer_luma           the four taps of BayerLuma's mask kernels, luma, per-image (luma - min) / (max - min + 1e-6)
    dwgate3x3            gelu(g) a + gelu(a) g with a, g two depthwise 3x3 of one input      (RawFomer_WFB_FFAB/model.py:55-59)
    dwconv5x5            depthwise 5x5, padding 2                                            (model.py:182-183)
    upsample_cat_reduce  ConvTranspose2d(2C, C, 2, 2), cat with the skip, Conv2d(2C, C, 1)   (model.py:494-503), the two-step form

Everything computes in the dtype (and on the device) of its inputs: float64 in, float64 out.  The depthwise filters are sums of
shifted slices times weights and the GELU is written with ``torch.erf``, so they use no convolution library call.

``defect`` evaluates the same operator with one deliberate error, each exactly what one branch of the kernel would get wrong, for
tests that have to show that their bound would see it:

    token_attention   drop_tail_keys      the keys from 64 (N // 64) on are ignored (the partial last block is skipped)
                      pad_keys            the keys are padded to a multiple of 64 with copies of key N - 1 (the clamped loads of the
                                          partial block without the -inf mask)
                      drop_tail_channels  the score uses the channels below 4 (d // 4) only (the last k-set is dropped)
                      padded_scale        (4 ceil(d / 4)) ** -0.5 in place of the scale
                      v_rows_16           rows of v from 16 on read as zero (the second 16-row tile of DT = 2 is missing)
    luma_film         bias_on_k           the query bias is added to k as well
                      exclude_pad         the pool divides by the number of taps inside the image
                      mean_head           the mean is taken over the first 65536 pixels only (one trip of luma_mean_kernel's loop)
    bayer_luma        swap_rb, no_eps (the 1e-6 omitted), range_head (min and max from the first 262144 pixels only: one trip of
                      the normaliser's loop over 1024 blocks)
    dwgate3x3         no_right (column x0 + 4 of every 4-pixel group reads zero), no_row_above (row y0 - 1 of every 4-row group reads
                      zero), no_ba.  Swapping the two filters cannot show: the gate gelu(g) a + gelu(a) g is symmetric in a and g.
    dwconv5x5         no_outer_halo (columns x0 - 2 and x0 + 5 of every 4-pixel group read zero), transposed_taps, no_bias
    upsample_cat_reduce  no_up_bias_term (b' = bR without Wr[:, :C] bU), swap_ij (Wu[k][m][j][i]), drop_tail_chunk (x channels from
                      16 (2C // 16) on and skip channels from 8 (C // 8) on are dropped: the partial last chunk of either phase)
    feed_forward      fold_identity (the rep-conv fold left at the identity: x1 = x);  illumination_estimator  no_mean_fold
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import rawformer_ref as R

DEFECTS = {
    "token_attention": ("drop_tail_keys", "pad_keys", "drop_tail_channels", "padded_scale", "v_rows_16"),
    "luma_film": ("bias_on_k", "exclude_pad", "mean_head"),
    "bayer_luma": ("swap_rb", "no_eps", "range_head"),
    "dwgate3x3": ("no_right", "no_row_above", "no_ba"),
    "dwconv5x5": ("no_outer_halo", "transposed_taps", "no_bias"),
    "upsample_cat_reduce": ("no_up_bias_term", "swap_ij", "drop_tail_chunk"),
    "feed_forward": ("fold_identity",),
    "illumination_estimator": ("no_mean_fold",),
}


def _known(op, defect):
    if defect is not None and defect not in DEFECTS[op]:
        raise ValueError(f"{op}: unknown defect {defect!r}")


def token_attention(qkv, heads, scale=None, defect=None):
    """``qkv`` [B, 3 heads d, h, w] (q, k, v thirds, channel = head d + i) -> [B, heads d, h, w]."""
    _known("token_attention", defect)
    b, c3, h, w = qkv.shape
    inner = c3 // 3
    d, n = inner // heads, h * w
    q, k, v = (t.reshape(b, heads, d, n).transpose(2, 3) for t in qkv.chunk(3, dim=1))          # b heads N d
    scale = d ** -0.5 if scale is None else scale
    qs, ks = q, k
    if defect == "drop_tail_channels":
        qs, ks = q[..., :4 * (d // 4)], k[..., :4 * (d // 4)]
    if defect == "padded_scale":
        scale = (4 * math.ceil(d / 4)) ** -0.5
    if defect == "v_rows_16":
        v = torch.cat((v[..., :16], torch.zeros_like(v[..., 16:])), dim=-1)
    if defect == "drop_tail_keys":
        ks, v = ks[:, :, :64 * (n // 64)], v[:, :, :64 * (n // 64)]
    if defect == "pad_keys":
        extra = (-n) % 64
        ks = torch.cat((ks, ks[:, :, -1:].expand(-1, -1, extra, -1)), dim=2)
        v = torch.cat((v, v[:, :, -1:].expand(-1, -1, extra, -1)), dim=2)
    attn = torch.softmax(torch.matmul(qs, ks.transpose(2, 3)) * scale, dim=-1)
    return torch.matmul(attn, v).transpose(2, 3).reshape(b, inner, h, w)


def luma_film(qkv, gamma, beta, luma, alpha, defect=None):
    _known("luma_film", defect)
    q, k, v = qkv.chunk(3, dim=1)
    q, k, v = gamma * q + beta, gamma * k + beta, gamma * v + beta
    if luma is not None:
        inv = F.avg_pool2d(1.0 - luma, 3, padding=1, stride=1, count_include_pad=defect != "exclude_pad")
        flat = inv.flatten(2)
        mean = (flat[..., :65536] if defect == "mean_head" else flat).mean(dim=-1)
        bias = alpha * (inv - mean[..., None, None])
        q = q + bias
        if defect == "bias_on_k":
            k = k + bias
    return torch.cat((q, k, v), dim=1)


def bayer_luma(mosaic, pattern="rggb", defect=None):
    """Tap (0, 0) = in[y-1][x-1], (0, 1) = in[y-1][x], (1, 0) = in[y][x-1], (1, 1) = in[y][x] of the zero-padded mosaic; a pattern
    names the colour of each tap in that order, the two greens average."""
    _known("bayer_luma", defect)
    hh, ww = mosaic.shape[-2:]
    p = F.pad(mosaic, (1, 0, 1, 0))
    taps = (p[..., :hh, :ww], p[..., :hh, 1:], p[..., 1:, :ww], p[..., 1:, 1:])
    rgb = {"r": 0.0, "g": 0.0, "b": 0.0}
    for t, c in zip(taps, pattern.lower()):
        rgb[c] = rgb[c] + (0.5 * t if c == "g" else t)
    r, b = (rgb["b"], rgb["r"]) if defect == "swap_rb" else (rgb["r"], rgb["b"])
    luma = (r * 0.299 + rgb["g"] * 0.587) + b * 0.114
    flat = luma.flatten(2)
    stat = flat[..., :262144] if defect == "range_head" else flat
    lo, hi = stat.amin(dim=-1)[..., None, None], stat.amax(dim=-1)[..., None, None]
    return (luma - lo) / (hi - lo + (0.0 if defect == "no_eps" else 1e-6))


def _depthwise(x, w, b, dead=None):
    """sum_taps w[c][ky][kx] x[y + ky - r][x + kx - r] + b[c] over the zero-padded planes, as shifted slices.  ``dead(dy, dx)``
    gives the output pixels ([h, w] mask) at which that tap reads zero instead, or None."""
    k = w.shape[-1]
    r = k // 2
    hh, ww = x.shape[-2:]
    xp = F.pad(x, (r, r, r, r))
    out = torch.zeros_like(x) if b is None else torch.zeros_like(x) + b.view(1, -1, 1, 1)
    for ky in range(k):
        for kx in range(k):
            term = xp[..., ky:ky + hh, kx:kx + ww]
            mask = dead(ky - r, kx - r) if dead else None
            if mask is not None:
                term = term * (~mask).to(x.dtype)
            out.addcmul_(term, w[:, 0, ky, kx].view(1, -1, 1, 1))      # one pass over the planes per tap
    return out


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def dwgate3x3(x, wa, ba, wb, bb, defect=None):
    _known("dwgate3x3", defect)
    hh, ww = x.shape[-2:]
    ys, xs = torch.arange(hh, device=x.device)[:, None], torch.arange(ww, device=x.device)[None, :]
    dead = None
    if defect == "no_right":
        dead = lambda dy, dx: ((xs % 4 == 3) & (ys >= 0)) if dx == 1 else None  # noqa: E731
    if defect == "no_row_above":
        dead = lambda dy, dx: ((ys % 4 == 0) & (xs >= 0)) if dy == -1 else None  # noqa: E731
    a = _depthwise(x, wa, None if defect == "no_ba" else ba, dead)
    g = _depthwise(x, wb, bb, dead)
    return _gelu(g) * a + _gelu(a) * g


def dwconv5x5(x, w, b, defect=None):
    _known("dwconv5x5", defect)
    hh, ww = x.shape[-2:]
    ys, xs = torch.arange(hh, device=x.device)[:, None], torch.arange(ww, device=x.device)[None, :]
    dead = None
    if defect == "no_outer_halo":
        dead = lambda dy, dx: ((xs % 4 == 0) & (ys >= 0)) if dx == -2 else ((xs % 4 == 3) & (ys >= 0)) if dx == 2 else None  # noqa: E731
    if defect == "transposed_taps":
        w = w.transpose(-1, -2)
    return _depthwise(x, w, None if defect == "no_bias" else b, dead)


def upsample_cat_reduce(x, skip, up_w, up_b, cr_w, cr_b, defect=None):
    """``x`` [B, 2C, h, w], ``skip`` [B, C, 2h, 2w], ``up_w`` [2C, C, 2, 2], ``cr_w`` [C, 2C, 1, 1] -> [B, C, 2h, 2w]."""
    _known("upsample_cat_reduce", defect)
    c = skip.shape[1]
    if defect == "swap_ij":
        up_w = up_w.transpose(-1, -2)
    if defect == "drop_tail_chunk":
        kx, ks = 16 * (2 * c // 16), 8 * (c // 8)
        x = torch.cat((x[:, :kx], torch.zeros_like(x[:, kx:])), dim=1)
        skip = torch.cat((skip[:, :ks], torch.zeros_like(skip[:, ks:])), dim=1)
    up = R.conv_transpose2x2(x, up_w, None if defect == "no_up_bias_term" else up_b)
    out = torch.einsum("ok,bkyx->boyx", cr_w[:, :, 0, 0], torch.cat((up, skip), dim=1))
    return out if cr_b is None else out + cr_b.view(1, -1, 1, 1)


def feed_forward(x, p, defect=None):
    """Eval-mode FeedForward (model.py:53-62) on the state_dict ``p``, un-fused (``R.wfb_feed_forward``)."""
    _known("feed_forward", defect)
    if defect is None:
        return R.wfb_feed_forward(x, p, "")
    hid = F.conv2d(x, p["project_in.weight"], p.get("project_in.bias"))
    x2 = F.conv2d(hid, p["dwconv.weight"], p.get("dwconv.bias"), padding=1, groups=hid.shape[1])
    return F.conv2d(F.gelu(x2) * hid + F.gelu(hid) * x2, p["project_out.weight"], p.get("project_out.bias")) + x


def illumination_estimator(img, p, defect=None):
    """Illumination_Estimator (model.py:186-200) for any channel count: conv1 takes [img ; mean_c(img)]."""
    _known("illumination_estimator", defect)
    mean = img.mean(dim=1, keepdim=True)
    inp = torch.cat([img, torch.zeros_like(mean) if defect == "no_mean_fold" else mean], dim=1)
    x1 = F.conv2d(inp, p["conv1.weight"], p["conv1.bias"])
    fea = F.conv2d(x1, p["depth_conv.weight"], p["depth_conv.bias"], padding=2, groups=x1.shape[1])
    return fea, F.conv2d(fea, p["conv2.weight"], p["conv2.bias"])
