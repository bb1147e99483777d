"""Evaluation-harness mirror of the reference's test loop (test.py:17-40 and 106-143).

``test.py`` post-processes every prediction on the host: ``clamp(0,1) * 255`` truncated to uint8,
Bayer-order channel fix-ups, PSNR / SSIM from scikit-image, JPEG + CSV.  Here the conversion, the
PSNR reduction and the SSIM run on the device with exact integer arithmetic (``csrc/rf_harness.hip``,
``csrc/rf_ssim.hip``); the channel fix-ups keep the reference's function names and semantics;
``evaluate_loader`` is the loop and ``write_metrics_csv`` its ``test_metrics.csv`` (no JPEG writing).

SSIM is scikit-image's definition (7x7 uniform window, K1 = 0.01, K2 = 0.03, data range 255, sample
covariance, mean over the fully covered window positions, channel-wise mean).  scikit-image itself is
not available where this project is built and tested, so SSIM parity is NOT pinned against
scikit-image: ``ssim_u8_device`` is tested against two independent float64 restatements of that
definition -- ``ssim_u8`` below (scipy ``uniform_filter``) and the integral-image restatement in
``tests/test_ssim.py`` (exact integer window sums).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib


def correct_bayer_channels(rgb, pattern: str = "RGGB"):
    """Channel order fix-up per Bayer pattern (test.py:17-29); works on numpy arrays and tensors (HWC)."""
    pattern = pattern.upper()
    if pattern == "BGGR":
        rgb = rgb[..., [2, 1, 0]]
    elif pattern == "GBRG":
        rgb = rgb[..., [1, 0, 2]]
    elif pattern == "GRBG":
        rgb = rgb[..., [0, 2, 1]]
    return rgb


def to_uint8_hwc(pred: torch.Tensor) -> torch.Tensor:
    """``(clamp(pred,0,1)[b].cpu().numpy().transpose(1,2,0) * 255).astype(np.uint8)`` for every image
    (test.py:117-118): float32 ``[B,C,H,W]`` on the device -> uint8 ``[B,H,W,C]`` on the device."""
    if pred.device.type != "cuda" or pred.dtype != torch.float32 or pred.dim() != 4:
        raise RuntimeError("to_uint8_hwc expects a float32 [B,C,H,W] ROCm tensor")
    pred = pred.contiguous()
    b, c, h, w = pred.shape
    out = torch.empty((b, h, w, c), dtype=torch.uint8, device=pred.device)
    _lib.launch("rf_to_uint8_hwc", pred, pred, out, b, c, h, w)
    return out


def channel_means_u8(img: torch.Tensor) -> torch.Tensor:
    """Exact per-channel means of uint8 ``[B,H,W,C]`` images (float64 ``[B,C]`` on the host)."""
    img = img.contiguous()
    b, h, w, c = img.shape
    sums = torch.empty((b, c), dtype=torch.int64, device=img.device)
    _lib.launch("rf_u8_channel_sums", img, img, sums, b, c, h * w)
    return sums.cpu().double() / float(h * w)


def auto_correct_rb(rgb: torch.Tensor) -> torch.Tensor:
    """Swap R and B when the red channel is darker than the blue one (test.py:31-40), per image."""
    means = channel_means_u8(rgb)
    out = rgb.clone()
    for i in range(rgb.shape[0]):
        if means[i, 0] < means[i, 2]:
            out[i] = rgb[i][..., [2, 1, 0]]
    return out


def psnr_u8(a: torch.Tensor, b: torch.Tensor) -> np.ndarray:
    """``skimage.metrics.peak_signal_noise_ratio`` on uint8 images (data_range 255, test.py:123):
    ``10 log10(255^2 / mean((a-b)^2))`` per image, the squared error summed exactly in uint64."""
    if a.shape != b.shape or a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise RuntimeError("psnr_u8 expects two uint8 tensors of the same shape")
    a, b = a.contiguous(), b.contiguous()
    n = a[0].numel()
    sse = torch.empty((a.shape[0],), dtype=torch.int64, device=a.device)
    _lib.launch("rf_u8_sse", a, a, b, sse, a.shape[0], n)
    mse = sse.cpu().numpy().astype(np.float64) / float(n)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 / mse)


def ssim_u8(a: np.ndarray, b: np.ndarray) -> float:
    """``structural_similarity(a, b, channel_axis=-1)`` restated from scikit-image's definition for one
    uint8 HWC image pair (host, float64).  PARITY UNPINNED: scikit-image is absent offline."""
    from scipy.ndimage import uniform_filter

    win, k1, k2, rng = 7, 0.01, 0.03, 255.0
    npx = win * win
    cov_norm = npx / (npx - 1.0)
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    pad = (win - 1) // 2
    vals = []
    for ch in range(a.shape[-1]):
        x, y = a[..., ch].astype(np.float64), b[..., ch].astype(np.float64)
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        vals.append(s[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


def ssim_u8_channel_means(a: torch.Tensor, b: torch.Tensor) -> np.ndarray:
    """Per-image, per-channel SSIM means of uint8 ``[B,H,W,C]`` device tensors (float64 ``[B,C]`` on the host): the window
    sums are exact integers and the per-position values are added in a fixed order, so the result is bitwise reproducible
    and the same for an image alone or in a batch (``csrc/rf_ssim.hip``)."""
    if a.shape != b.shape or a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() != 4:
        raise RuntimeError("ssim_u8_device expects two uint8 [B,H,W,C] tensors of the same shape")
    if a.device.type != "cuda" or b.device != a.device:
        raise RuntimeError("ssim_u8_device runs on the ROCm device only (ssim_u8 is the host restatement)")
    a, b = a.contiguous(), b.contiguous()
    n, h, w, c = a.shape
    scratch = _lib.scratch("rf_u8_ssim_scratch_bytes", a, n, c, h, w)
    sums = torch.empty((n, c), dtype=torch.float64, device=a.device)
    _lib.launch("rf_u8_ssim", a, a, b, sums, scratch, n, c, h, w)
    return sums.cpu().numpy() / float((h - 6) * (w - 6))


def ssim_u8_device(a: torch.Tensor, b: torch.Tensor) -> np.ndarray:
    """``structural_similarity(a[i], b[i], channel_axis=-1)`` (test.py:124) for every image of two uint8 ``[B,H,W,C]`` device
    tensors: float64 per image, the mean of ``ssim_u8_channel_means`` over the channels."""
    return ssim_u8_channel_means(a, b).mean(axis=1)


def evaluate(pred: torch.Tensor, gt: torch.Tensor, bayer_pattern: str = "RGGB", with_ssim: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The body of test.py's loop (test.py:110-124) for a batch: uint8 conversion, Bayer fix-ups on both
    images, PSNR (and optionally SSIM, on the device).  ``pred``/``gt`` are float32 ``[B,3,H,W]`` device tensors."""
    p8 = auto_correct_rb(correct_bayer_channels(to_uint8_hwc(torch.clamp(pred, 0, 1)), bayer_pattern).contiguous())
    g8 = auto_correct_rb(correct_bayer_channels(to_uint8_hwc(gt), bayer_pattern).contiguous())
    psnr = psnr_u8(p8, g8)
    ssim = ssim_u8_device(p8, g8) if with_ssim else np.array([])
    return psnr, ssim


def evaluate_loader(model, batches, bayer_pattern: str = "RGGB") -> Dict[str, object]:
    """test.py:106-137 without the image writing: for every ``(inp, gt)`` batch the forward under ``no_grad`` and the loop body
    (``evaluate`` with SSIM) for each of its images.  Returns the per-image lists ``psnr`` and ``ssim`` in loader order and
    their means ``psnr_average`` / ``ssim_average`` (test.py:136-137)."""
    psnr_val_rgb, ssim_val_rgb = [], []
    dev = next(model.parameters()).device
    with torch.no_grad():
        for inp, gt in batches:
            psnr, ssim = evaluate(model(inp.to(dev)), gt.to(dev), bayer_pattern, with_ssim=True)
            psnr_val_rgb.extend(float(v) for v in psnr)
            ssim_val_rgb.extend(float(v) for v in ssim)
    return {"psnr": psnr_val_rgb, "ssim": ssim_val_rgb,
            "psnr_average": float(np.mean(psnr_val_rgb)), "ssim_average": float(np.mean(ssim_val_rgb))}


def write_metrics_csv(path, psnr, ssim) -> None:
    """``test_metrics.csv`` as test.py:141-143 writes it: one ``PSNR,SSIM`` row per image, four decimals."""
    np.savetxt(path, np.column_stack((psnr, ssim)), delimiter=',', fmt='%.4f')


_SID_MODES = {"loader": 0, "rgbg": 0, "rggb": 1, "unshuffle": 1, "mosaic": 2}


def pack_raw(raw: torch.Tensor, black_level: int, white_level: int, ratio: float = 1.0, layout: str = "loader") -> torch.Tensor:
    """SID front-end on the device (correctdataloader.py:58-72 ``pack_raw``, :86 ``* ratio``, :103 ``min(., 1)``).

    ``raw``: uint16 (or int16-viewed) Bayer frames ``[B, 2h, 2w]`` on the GPU; ``black_level`` =
    ``min(raw.black_level_per_channel)``.  ``layout``: ``"loader"`` = the reference loader's channel order
    (sites (0,0) (0,1) (1,1) (1,0)), ``"rggb"`` = ``pixel_unshuffle`` order, ``"mosaic"`` = normalised
    ``[B,1,2h,2w]`` mosaic (the input of ``RawFormer.forward``)."""
    if not raw.is_cuda:
        raise RuntimeError("pack_raw: the SID front-end runs on the ROCm device only (no CPU fallback)")
    if raw.dtype not in (torch.uint16, torch.int16):
        raise TypeError(f"pack_raw: expected a uint16 Bayer frame, got {raw.dtype}")
    if raw.dim() == 2:
        raw = raw.unsqueeze(0)
    raw = raw.contiguous()
    B, H2, W2 = raw.shape
    if H2 % 2 or W2 % 8:
        raise ValueError(f"pack_raw: mosaic {H2}x{W2} must have an even height and a width that is a multiple of 8")
    mode = _SID_MODES[layout]
    h, w = H2 // 2, W2 // 2
    out = torch.empty((B, 1, H2, W2) if mode == 2 else (B, 4, h, w), dtype=torch.float32, device=raw.device)
    _lib.launch("rf_sid_pack", raw, raw, out, B, h, w, int(black_level), int(white_level), float(ratio), mode)
    return out
