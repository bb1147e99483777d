"""Plain-torch restatements of the operators of the base RawFormer block (variants 'flca' and 'plain'), for
tests/test_base_kernels.py:

    channel_attention    Attention(dim, heads): 1x1 -> depthwise 3x3 -> normalised c x c softmax per head -> 1x1
    bayer_luma_chroma    y = luma / max(per-image max, 1e-6), cr = R - y, cb = B - y
    flca_guidance        [resize(LL), resize(sqrt(LH^2 + HL^2 + HH^2 + 1e-8)), resize(cr), resize(cb)], bilinear
    flca                 the three spatial gates on the guidance planes, the pooled mean, the squeeze-excite gate
    layernorm2d          per-pixel LayerNorm over the channels, with and without bias
    dwconv3x3            depthwise 3x3, padding 1 (+ exact GELU)
    conv_ffn             1x1 -> depthwise 3x3 -> GELU -> 1x1
    transformer_block    x1 = x + attention(LN1 x); out = x1 + conv_ffn(LN2 x1)

Everything computes in the dtype of its inputs: float64 in, float64 out.  The 1x1 convolutions are einsums, the depthwise
filters sums of shifted slices, the GELU is written with ``torch.erf``: no convolution library call.  Without a defect each
function is oracle/rawformer_ref.py's, to 1e-12 relative in float64 (test_restatements_match_the_oracle); dwconv3x3, which the
oracle has only inside conv_ffn, is pinned to torch.nn.functional.conv2d and gelu as well.

``defect`` evaluates the same operator with one deliberate error, each what one branch of a kernel would get wrong, for the
tests that have to show that their bound would see it:

    channel_attention  no_clamp            q / |q| and k / |k| without the 1e-12 clamp of the norm
                       clamp_squared       the clamp applied to |q|^2: sqrt(max(|q|^2, 1e-12))
                       head0_temperature   the temperature of head 0 for every head
                       softmax_over_i      the softmax runs over the query index
                       full_cxc            one C x C softmax over all channels (the heads are not block-diagonal)
                       drop_last_slab      the Gram sums and the norms leave out the pixels of the last slab: of gram_plan's slabs
                                           (``gram_slabs``) or, where attn_mid_kernel runs, of attn_mid_plan's (``mid_slabs``)
                       drop_tail_64        ... leave out the pixels from 64 (P // 64) on (the partial last step of a slab)
                       k_norm_from_q       |k_j|^2 is read from the q tile: |q_j|^2 of the same head
                       no_proj_bias        project_out without its bias
                       replicate_pad       the depthwise 3x3 pads with the edge pixel, not with zero
    guidance           no_luma_eps         y = luma / max without the 1e-6 clamp
                       no_mag_eps          the Haar magnitude without the 1e-8 under the root
                       g1_only             G = G1, not (G1 + G2) / 2
                       swap_cr_cb          the chroma planes exchanged
                       batch_max           the luma maximum over the whole batch
                       align_corners       F.interpolate(align_corners=True)
                       no_far_clamp        the second bilinear neighbour is not clamped at the far edge: it reads the next row's
                                           first pixel (columns) or zero (below the last row)
                       ll_no_half          LL = a + b + c + d, without the 0.5
    flca               replicate_pad       the 3x3 gates pad the guidance planes with the edge pixel
                       no_group_left       the tap left of every lane group (4 pixels at w % 4 == 0, else 2) reads zero
                       no_group_right      the tap right of every lane group reads zero
                       tanh_sigmoid        the high-band gate is a sigmoid, the low-band gate a tanh
                       swap_chroma_taps    the cr taps meet the cb plane and the reverse
                       last_block_unpooled the pooled mean leaves out the last pixel block (``flca_block`` pixels; still / P)
                       mean_padded         the pooled sum is divided by nblk x the block size
                       no_relu             the squeeze-excite hidden layer has no ReLU
                       no_se3_bias         se.3 without its bias
    layernorm2d        unbiased_var        variance / (C - 1)
                       eps_outside         1 / (sqrt(var) + eps)
    dwconv3x3          replicate_pad, no_bias, tanh_gelu (the tanh approximation in place of erf),
                       no_group_left (the tap left of every 4-pixel group reads zero), no_row_above (the row above every
                       group of ``rows`` output rows reads zero)
    conv_ffn           tanh_gelu, no_seam_row / no_seam_col: the depthwise filter reads zero above every 4-row tile / left of every
                       64-column tile (the halo of a 4 x 64 tile of the fused kernels)
    transformer_block  unbiased_var, eps_outside (both LayerNorms), ln2_of_x (LN2 is fed x, not x1), no_ffn_residual,
                       tanh_gelu, no_seam_row, no_seam_col
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

DEFECTS = {
    "channel_attention": ("no_clamp", "clamp_squared", "head0_temperature", "softmax_over_i", "full_cxc", "drop_last_slab",
                          "drop_tail_64", "k_norm_from_q", "no_proj_bias", "replicate_pad"),
    "guidance": ("no_luma_eps", "no_mag_eps", "g1_only", "swap_cr_cb", "batch_max", "align_corners", "no_far_clamp", "ll_no_half"),
    "flca": ("replicate_pad", "no_group_left", "no_group_right", "tanh_sigmoid", "swap_chroma_taps", "last_block_unpooled",
             "mean_padded", "no_relu", "no_se3_bias"),
    "layernorm2d": ("unbiased_var", "eps_outside"),
    "dwconv3x3": ("replicate_pad", "no_bias", "tanh_gelu", "no_group_left", "no_row_above"),
    "conv_ffn": ("tanh_gelu", "no_seam_row", "no_seam_col"),
    "transformer_block": ("unbiased_var", "eps_outside", "ln2_of_x", "no_ffn_residual", "tanh_gelu", "no_seam_row", "no_seam_col"),
}


def _known(op, defect):
    if defect is not None and defect not in DEFECTS[op]:
        raise ValueError(f"{op}: unknown defect {defect!r}")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- the plans, restated
def gram_slabs(p):
    """(nslab, slab) of gram_plan (csrc/rf_attn.hip) for P pixels."""
    target = min(max(p // 16, 1024), 8192)
    ns = max(1, min(cdiv(p, target), cdiv(p, 256)))
    slab = cdiv(cdiv(p, ns), 256) * 256
    return cdiv(p, slab), slab


def mid_slabs(h, w):
    """(nslab, tiles per slab, tiles) of attn_mid_plan (csrc/rf_attn_mid.hip): tiles of 4 x 64 pixels."""
    ntiles = cdiv(w, 64) * cdiv(h, 4)
    per = min(max(ntiles // 64, 1), 8)
    return cdiv(ntiles, per), per, ntiles


def attn_path(c, heads, h, w):
    """'mid' where ops.channel_attention runs attn_mid_kernel (attn_mid_supported), else 'gram'."""
    hs = c // heads
    return "mid" if c in (64, 128) and w % 4 == 0 and hs <= 16 and 16 % hs == 0 else "gram"


def band_of(tq, c, hs):
    """(first k tile, k tiles) that the 16-channel q tile ``tq`` needs at C channels in heads of ``hs`` (band_of, csrc/rf_attn.hip)."""
    lo, hi = 16 * tq, min(16 * tq + 15, c - 1)
    klo, khi = (lo // hs) * hs, (hi // hs + 1) * hs - 1
    return klo // 16, khi // 16 - klo // 16 + 1


def gram_tiles(c, heads):
    """Per q tile of gram_kernel: (first k tile, k tiles, whether the tile may take the fast loop: every row of it and of its band
    below C; the loop also needs float4 loads and a slab length that is a multiple of 64)."""
    out = []
    for tq in range(cdiv(c, 16)):
        tklo, nb = band_of(tq, c, c // heads)
        out.append((tklo, nb, 16 * tq + 16 <= c and 16 * (tklo + nb) <= c))
    return out


def layernorm_kernel(c, p):
    """The kernel launch_layernorm2d (csrc/rf_pointwise.hip) picks under the one census name: 'reg', 'vec4' or 'scalar'."""
    if p % 4:
        return "scalar"
    return "reg" if c in (16, 32, 48, 64, 96, 128, 192, 256, 384, 512) else "vec4"


def fold_rs(hs):
    """RS of attn_fold_kernel for head size ``hs``: the threads that share one value's sum over the slabs."""
    return min(max(256 // (hs * hs + 2 * hs), 1), 16)


def flca_block(w):
    """Pixels per block of the FLCA spatial kernels (flca_nblk, csrc/rf_flca.hip)."""
    return 1024 if w % 4 == 0 else 512 if w % 2 == 0 else 256


# ---------------------------------------------------------------------------------------------- pieces
def conv1x1(x, w, b=None):
    out = torch.einsum("ok,bkyx->boyx", w.reshape(w.shape[0], -1), x)
    return out if b is None else out + b.view(1, -1, 1, 1)


def _depthwise3(x, w, b, pad="zero", dead=None):
    """sum_taps w[c][ky][kx] x[y + ky - 1][x + kx - 1] + b[c].  ``dead(dy, dx)``: the output pixels ([h, w] mask) at which that
    tap reads zero instead, or None."""
    hh, ww = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate") if pad == "replicate" else F.pad(x, (1, 1, 1, 1))
    out = torch.zeros_like(x) if b is None else torch.zeros_like(x) + b.view(1, -1, 1, 1)
    for ky in range(3):
        for kx in range(3):
            term = xp[..., ky:ky + hh, kx:kx + ww]
            mask = dead(ky - 1, kx - 1) if dead else None
            if mask is not None:
                term = term * (~mask).to(x.dtype)
            out = out + term * w[:, 0, ky, kx].view(1, -1, 1, 1)
    return out


def _grid(x):
    hh, ww = x.shape[-2:]
    return torch.arange(hh, device=x.device)[:, None], torch.arange(ww, device=x.device)[None, :]


def gelu(v, tanh=False):
    if tanh:
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


# ---------------------------------------------------------------------------------------------- channel attention
def channel_attention(x, qkv_w, qkv_b, dw_w, dw_b, temperature, proj_w, proj_b, heads, defect=None, parts=False):
    """``parts``: also the dict of q, k ([b, heads, c, P]), the squared row norms, the logits and the attention map."""
    _known("channel_attention", defect)
    b, cc, h, w = x.shape
    hs, p = cc // heads, h * w
    qkv = _depthwise3(conv1x1(x, qkv_w, qkv_b), dw_w, dw_b, pad="replicate" if defect == "replicate_pad" else "zero")
    q, k, v = qkv.reshape(b, 3, heads, hs, p).unbind(dim=1)
    keep = torch.ones(p, dtype=torch.bool)
    if defect == "drop_last_slab":
        if attn_path(cc, heads, h, w) == "gram":
            ns, slab = gram_slabs(p)
            keep[slab * (ns - 1):] = False
        else:
            ns, per, _ = mid_slabs(h, w)
            ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
            tile = (xs // 64) * cdiv(h, 4) + ys // 4                      # numbered down the columns
            keep = (tile < per * (ns - 1)).reshape(p)
    if defect == "drop_tail_64":
        keep[64 * (p // 64):] = False
    keep = keep.to(x.device)
    qs, ks = q * keep.to(x.dtype), k * keep.to(x.dtype)
    nq, nk = (qs * qs).sum(dim=-1), (ks * ks).sum(dim=-1)                 # [b, heads, c]
    if defect == "k_norm_from_q":
        nk = nq
    gram = torch.einsum("bhin,bhjn->bhij", qs, ks)

    def inv_norm(n2):
        if defect == "no_clamp":
            return 1.0 / n2.sqrt()
        if defect == "clamp_squared":
            return 1.0 / n2.clamp_min(1e-12).sqrt()
        return 1.0 / n2.sqrt().clamp_min(1e-12)

    t = temperature.reshape(1, heads, 1, 1).to(x.dtype)
    if defect == "head0_temperature":
        t = t[:, :1].expand(1, heads, 1, 1)
    logits = gram * inv_norm(nq)[..., :, None] * inv_norm(nk)[..., None, :] * t
    if defect == "full_cxc":
        qn = (qs * inv_norm(nq)[..., None]).reshape(b, cc, p)
        kn = (ks * inv_norm(nk)[..., None]).reshape(b, cc, p)
        full = torch.einsum("bin,bjn->bij", qn, kn) * t.expand(1, heads, hs, 1).reshape(1, cc, 1)
        out = torch.einsum("bij,bjn->bin", torch.softmax(full, dim=-1), v.reshape(b, cc, p))
        attn = None
    else:
        attn = torch.softmax(logits, dim=-2 if defect == "softmax_over_i" else -1)
        out = torch.einsum("bhij,bhjn->bhin", attn, v)
    out = conv1x1(out.reshape(b, cc, h, w), proj_w, None if defect == "no_proj_bias" else proj_b)
    if parts:
        return out, {"q": q, "k": k, "nq": nq, "nk": nk, "logits": logits, "attn": attn}
    return out


# ---------------------------------------------------------------------------------------------- guidance
def bayer_luma_chroma(x4, defect=None):
    _known("guidance", defect)
    r, b = x4[:, 0:1], x4[:, 3:4]
    g = x4[:, 1:2] if defect == "g1_only" else 0.5 * (x4[:, 1:2] + x4[:, 2:3])
    y = 0.299 * r + 0.587 * g + 0.114 * b
    top = y.amax(dim=(1, 2, 3), keepdim=True) if defect != "batch_max" else y.amax().reshape(1, 1, 1, 1)
    y = y / (top if defect == "no_luma_eps" else top.clamp_min(1e-6))
    cr, cb = r - y, b - y
    return (y, cb, cr) if defect == "swap_cr_cb" else (y, cr, cb)


def bilinear_resize(x, size, defect=None):
    """F.interpolate(mode='bilinear', align_corners=False), written out; the weights are computed in ``x.dtype``."""
    def axis(n_in, n_out):
        i = torch.arange(n_out, dtype=x.dtype, device=x.device)
        if defect == "align_corners":
            src = i * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            src = ((i + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
        i0 = src.floor().to(torch.int64).clamp_max(n_in - 1)
        i1 = i0 + 1 if defect == "no_far_clamp" else (i0 + 1).clamp_max(n_in - 1)
        return i0, i1, src - i0.to(x.dtype)

    hh, ww = x.shape[-2:]
    y0, y1, ly = axis(hh, size[0])
    x0, x1, lx = axis(ww, size[1])
    if defect == "no_far_clamp":          # flat memory: column w of row y is column 0 of row y + 1; below the last row, zero
        flat = torch.cat((x.flatten(2), x.new_zeros(*x.shape[:2], ww + 1)), dim=-1)
        at = lambda yy, xx: flat[..., (yy[:, None] * ww + xx[None, :]).reshape(-1)].reshape(*x.shape[:2], len(yy), len(xx))  # noqa: E731
    else:
        at = lambda yy, xx: x[:, :, yy][:, :, :, xx]  # noqa: E731
    top = at(y0, x0) * (1 - lx) + at(y0, x1) * lx
    bot = at(y1, x0) * (1 - lx) + at(y1, x1) * lx
    return top * (1 - ly).view(1, 1, -1, 1) + bot * ly.view(1, 1, -1, 1)


def flca_guidance(x4, size, defect=None):
    """[B, 4, H, W] packed RGGB (H, W even) -> the four guidance planes at ``size``."""
    _known("guidance", defect)
    y, cr, cb = bayer_luma_chroma(x4, defect)
    a, b, c, d = y[:, :, 0::2, 0::2], y[:, :, 0::2, 1::2], y[:, :, 1::2, 0::2], y[:, :, 1::2, 1::2]
    ll = (a + b + c + d) * (1.0 if defect == "ll_no_half" else 0.5)
    lh, hl, hh = (a - b + c - d) * 0.5, (a + b - c - d) * 0.5, (a - b - c + d) * 0.5
    mag = torch.sqrt(lh * lh + hl * hl + hh * hh + (0.0 if defect == "no_mag_eps" else 1e-8))
    return torch.cat([bilinear_resize(t, size, defect) for t in (ll, mag, cr, cb)], dim=1)


# ---------------------------------------------------------------------------------------------- FLCA
def flca(feat, guide, p, defect=None, parts=False):
    """``guide`` [B, 4, h, w] = flca_guidance at the feature size; ``p``: alpha, beta, gamma, low_attn.0.weight,
    high_attn.0.weight, chroma_attn.0.weight, se.1.weight, se.1.bias, se.3.weight, se.3.bias."""
    _known("flca", defect)
    hh, ww = feat.shape[-2:]
    n, c = hh * ww, feat.shape[1]
    ys, xs = _grid(feat)
    grp = 4 if ww % 4 == 0 else 2
    dead = None
    if defect == "no_group_left":
        dead = lambda dy, dx: ((xs % grp == 0) & (ys >= 0)) if dx == -1 else None  # noqa: E731
    if defect == "no_group_right":
        dead = lambda dy, dx: ((xs % grp == grp - 1) & (ys >= 0)) if dx == 1 else None  # noqa: E731
    pad = "replicate" if defect == "replicate_pad" else "zero"

    def gate(plane, w):          # one guidance plane [B, 1, h, w] against [C, 1, 3, 3]: [B, C, h, w]
        pp = F.pad(plane, (1, 1, 1, 1), mode="replicate") if pad == "replicate" else F.pad(plane, (1, 1, 1, 1))
        taps = []
        for ky in range(3):
            for kx in range(3):
                term = pp[:, 0, ky:ky + hh, kx:kx + ww]
                mask = dead(ky - 1, kx - 1) if dead else None
                taps.append(term if mask is None else term * (~mask).to(plane.dtype))
        return torch.einsum("ct,btyx->bcyx", w.reshape(c, 9), torch.stack(taps, dim=1))

    wc = p["chroma_attn.0.weight"]
    if defect == "swap_chroma_taps":
        wc = wc.flip(1)
    s_low, s_high = gate(guide[:, 0:1], p["low_attn.0.weight"]), gate(guide[:, 1:2], p["high_attn.0.weight"])
    s_chr = gate(guide[:, 2:3], wc[:, 0:1]) + gate(guide[:, 3:4], wc[:, 1:2])
    lo, hi = (torch.tanh, torch.sigmoid) if defect == "tanh_sigmoid" else (torch.sigmoid, torch.tanh)
    x = feat * (1 + p["alpha"] * lo(s_low) + p["beta"] * hi(s_high) + p["gamma"] * torch.sigmoid(s_chr))
    blk = flca_block(ww)
    flat = x.flatten(2)
    if defect == "last_block_unpooled":
        flat = flat[..., :blk * (cdiv(n, blk) - 1)]
    pooled = flat.sum(dim=-1) / (blk * cdiv(n, blk) if defect == "mean_padded" else n)          # [B, C]
    hid = pooled @ p["se.1.weight"].reshape(-1, c).t() + p["se.1.bias"]
    if defect != "no_relu":
        hid = torch.relu(hid)
    ch = hid @ p["se.3.weight"].reshape(c, -1).t()
    if defect != "no_se3_bias":
        ch = ch + p["se.3.bias"]
    out = x * torch.sigmoid(ch)[:, :, None, None]
    if parts:
        return out, {"s_low": s_low, "s_high": s_high, "s_chr": s_chr, "pooled": pooled, "hid": hid}
    return out


# ---------------------------------------------------------------------------------------------- LayerNorm, depthwise, FFN, block
def layernorm2d(x, weight, bias, eps=1e-5, defect=None):
    _known("layernorm2d", defect)
    mu = x.mean(dim=1, keepdim=True)
    d = x - mu
    var = (d * d).sum(dim=1, keepdim=True) / (x.shape[1] - 1 if defect == "unbiased_var" else x.shape[1])
    rs = 1.0 / (var.sqrt() + eps) if defect == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    w = weight.view(1, -1, 1, 1)
    if bias is None:                      # BiasFree: the mean stays in the numerator
        return x * rs * w
    return d * rs * w + bias.view(1, -1, 1, 1)


def dwconv3x3(x, weight, bias, gelu_act=False, defect=None, rows=4):
    _known("dwconv3x3", defect)
    ys, xs = _grid(x)
    dead = None
    if defect == "no_group_left":
        dead = lambda dy, dx: ((xs % 4 == 0) & (ys >= 0)) if dx == -1 else None  # noqa: E731
    if defect == "no_row_above":
        dead = lambda dy, dx: ((ys % rows == 0) & (xs >= 0)) if dy == -1 else None  # noqa: E731
    out = _depthwise3(x, weight, None if defect == "no_bias" else bias, "replicate" if defect == "replicate_pad" else "zero", dead)
    return gelu(out, tanh=defect == "tanh_gelu") if gelu_act else out


def conv_ffn(x, pw1_w, pw1_b, dw_w, dw_b, pw2_w, pw2_b, defect=None, parts=False):
    _known("conv_ffn", defect)
    t = conv1x1(x, pw1_w, pw1_b)
    ys, xs = _grid(x)
    dead = None
    if defect == "no_seam_row":
        dead = lambda dy, dx: ((ys % 4 == 0) & (xs >= 0)) if dy == -1 else None  # noqa: E731
    if defect == "no_seam_col":
        dead = lambda dy, dx: ((xs % 64 == 0) & (ys >= 0)) if dx == -1 else None  # noqa: E731
    pre = _depthwise3(t, dw_w, dw_b, "zero", dead)
    out = conv1x1(gelu(pre, tanh=defect == "tanh_gelu"), pw2_w, pw2_b)
    return (out, {"pre": pre}) if parts else out


def transformer_block(x, p, heads, defect=None, parts=False):
    _known("transformer_block", defect)
    ln = defect if defect in ("unbiased_var", "eps_outside") else None
    ffn = defect if defect in DEFECTS["conv_ffn"] else None
    a = layernorm2d(x, p["norm1.body.weight"], p["norm1.body.bias"], defect=ln)
    x1 = x + channel_attention(a, p["attn.qkv.weight"], p["attn.qkv.bias"], p["attn.qkv_dwconv.weight"], p["attn.qkv_dwconv.bias"],
                               p["attn.temperature"], p["attn.project_out.weight"], p["attn.project_out.bias"], heads)
    f = layernorm2d(x if defect == "ln2_of_x" else x1, p["norm2.body.weight"], p["norm2.body.bias"], defect=ln)
    y, extra = conv_ffn(f, p["ffn.pointwise1.weight"], p["ffn.pointwise1.bias"], p["ffn.depthwise.weight"], p["ffn.depthwise.bias"],
                        p["ffn.pointwise2.weight"], p["ffn.pointwise2.bias"], defect=ffn, parts=True)
    out = y if defect == "no_ffn_residual" else x1 + y
    return (out, extra) if parts else out
