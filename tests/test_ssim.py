"""Device SSIM of the evaluation harness (test.py:124, ``structural_similarity(a, b, channel_axis=-1)`` on uint8 HWC images).

The reference here is ``exact_ssim`` below, an independent restatement of scikit-image's definition: int64 integral images give
the five 7x7 window sums exactly, the quotient is evaluated in float64 from those integers, and ``math.fsum`` takes the mean.
``harness.ssim_u8`` (scipy ``uniform_filter``, float64 throughout) is the second restatement.  scikit-image itself is not
available where this suite runs, so neither the device path nor the two restatements are pinned against it.

Tolerance of the device path against ``exact_ssim``, per channel mean, N = (h-6)(w-6):  (N + 16) 2^-53.  Every per-position
value lies in [-1, 1] and is fewer than 16 float64 roundings away from exact integers on either side (four factors, two
products, one quotient); a sum of N such terms in any order errs by at most (N-1) units of 2^-53 on the mean.

CPU: the ABI (exported, declared, bound; argument errors without a launch) and the CSV writer.  GPU: everything else.
"""
import ctypes as C
import io
import math
import os
import re

import numpy as np
import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib, harness, synth
from oracle import harness_ref as H

WIN, NPX = 7, 49
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def _window_sums(v):
    """7x7 window sums of an int64 [H,W] plane at the fully covered positions, through an integral image (exact)."""
    ii = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
    ii[1:, 1:] = v.cumsum(0).cumsum(1)
    return ii[WIN:, WIN:] - ii[:-WIN, WIN:] - ii[WIN:, :-WIN] + ii[:-WIN, :-WIN]


def exact_ssim(a, b):
    """Per-channel SSIM means (float64 [C]) of two uint8 HWC images."""
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c].astype(np.int64), b[..., c].astype(np.int64)
        sx, sy, sxx, syy, sxy = (_window_sums(v) for v in (x, y, x * x, y * y, x * y))
        n = NPX
        num = (2 * sx * sy + C1 * n * n) * (2 * (n * sxy - sx * sy) + C2 * n * (n - 1))
        den = (sx * sx + sy * sy + C1 * n * n) * (n * sxx - sx * sx + n * syy - sy * sy + C2 * n * (n - 1))
        s = (num / den).ravel()
        out.append(math.fsum(s) / s.size)
    return np.array(out)


def tol(h, w):
    return ((h - 6) * (w - 6) + 16) * 2.0 ** -53


def synth_pair(h, w, c, seed=5):
    """uint8 HWC pair from the smooth synthetic scenes (the pair test_harness.py uses, cropped / tiled to c channels)."""
    p = H.to_uint8_hwc(np.clip(synth.smooth_rgb(seed, 1, h, w)[0] * 1.2 - 0.1, 0, 1))
    g = H.to_uint8_hwc(synth.smooth_rgb(seed + 4, 1, h, w)[0])
    idx = [i % 3 for i in range(c)]
    return np.ascontiguousarray(p[..., idx]), np.ascontiguousarray(g[..., idx])


def random_pair(h, w, c, seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8), rng.integers(0, 256, (h, w, c), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_restatements_agree_on_the_host():
    for a, b in (synth_pair(33, 47, 3), random_pair(8, 200, 3), random_pair(7, 7, 3)):
        assert abs(float(np.mean(exact_ssim(a, b))) - harness.ssim_u8(a, b)) < 1e-12


def test_ssim_abi_is_exported_declared_and_bound():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(cases.REPO, "include", "rawformer_hip.h")).read(), flags=re.S)
    for name in ("rf_u8_ssim", "rf_u8_ssim_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in rawformer_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"


def test_ssim_argument_errors_return_invalid_without_a_launch():
    lib = _lib.load()
    sz = C.c_size_t()
    fake = C.c_void_p(1 << 12)      # aligned, never dereferenced: the shape checks come first and nothing is launched
    assert lib.rf_u8_ssim_scratch_bytes(2, 3, 96, 160, C.byref(sz)) == 0 and sz.value > 0 and sz.value % 8 == 0
    one = sz.value
    assert lib.rf_u8_ssim_scratch_bytes(4, 3, 96, 160, C.byref(sz)) == 0 and sz.value == 2 * one
    for b, c, h, w, word in ((1, 3, 6, 160, b"window"), (1, 3, 96, 6, b"window"), (1, 0, 96, 160, b"channels"), (1, 5, 96, 160, b"channels"),
                             (0, 3, 96, 160, b"batch"), (65536, 3, 96, 160, b"batch")):
        assert lib.rf_u8_ssim_scratch_bytes(b, c, h, w, C.byref(sz)) == -22, (b, c, h, w)
        assert word in lib.rf_last_error()
        assert lib.rf_u8_ssim(fake, fake, fake, fake, b, c, h, w, None) == -22, (b, c, h, w)
        assert word in lib.rf_last_error()
    assert lib.rf_u8_ssim(fake, fake, None, fake, 1, 3, 96, 160, None) == -22       # null output


def test_write_metrics_csv_is_the_reference_file(tmp_path):
    psnr = [31.123456, 28.5, float("inf"), 40.00004]
    ssim = [0.912345, 0.5, 1.0, 0.99995]
    path = tmp_path / "test_metrics.csv"
    harness.write_metrics_csv(str(path), psnr, ssim)
    ref = io.BytesIO()
    np.savetxt(ref, np.column_stack((psnr, ssim)), delimiter=',', fmt='%.4f')       # test.py:141-143
    assert path.read_bytes() == ref.getvalue()
    harness.write_metrics_csv(str(path), np.array(psnr[:1]), np.array(ssim[:1]))    # arrays, one image
    assert path.read_bytes() == b"31.1235,0.9123\n"


# ------------------------------------------------------------------------------------------------------------------ GPU

def device_means(a, b, device):
    ta, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in (a, b))
    if ta.dim() == 3:
        ta, tb = ta[None], tb[None]
    return harness.ssim_u8_channel_means(ta, tb)


SHAPES = [(7, 7, 3), (8, 200, 3), (33, 47, 3), (96, 160, 3), (64, 80, 1), (64, 80, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synth", "random"])
@pytest.mark.parametrize("h,w,c", SHAPES)
def test_device_ssim_is_exact(device, h, w, c, kind):
    a, b = synth_pair(h, w, c) if kind == "synth" else random_pair(h, w, c)
    got = device_means(a, b, device)
    assert got.shape == (1, c) and got.dtype == np.float64
    want = exact_ssim(a, b)
    err = np.abs(got[0] - want)
    print(f"{kind} {h}x{w}x{c}: max |device - exact| = {err.max():.3e} (bound {tol(h, w):.3e})")
    assert (err <= tol(h, w)).all(), (got[0], want)
    per_image = harness.ssim_u8_device(torch.from_numpy(a)[None].to(device), torch.from_numpy(b)[None].to(device))
    print(f"    |device - ssim_u8| = {abs(per_image[0] - harness.ssim_u8(a, b)):.3e}")
    assert abs(per_image[0] - harness.ssim_u8(a, b)) < 1e-9


@pytest.mark.gpu
def test_device_ssim_two_channels_and_unaligned_views(device):
    """C = 2, and images whose first byte is not on a dword: image i of a batch with an odd image size."""
    a, b = random_pair(19, 31, 2, seed=3)
    assert (np.abs(device_means(a, b, device)[0] - exact_ssim(a, b)) <= tol(19, 31)).all()
    rng = np.random.default_rng(11)
    A, B = rng.integers(0, 256, (3, 9, 13, 3), dtype=np.uint8), rng.integers(0, 256, (3, 9, 13, 3), dtype=np.uint8)   # 351 bytes per image
    got = device_means(A, B, device)
    for i in range(3):
        assert (np.abs(got[i] - exact_ssim(A[i], B[i])) <= tol(9, 13)).all()
    ta, tb = torch.from_numpy(A).to(device), torch.from_numpy(B).to(device)
    alone = harness.ssim_u8_channel_means(ta[1:2], tb[1:2])      # a view starting 351 bytes into the buffer
    assert np.array_equal(alone[0], got[1])


@pytest.mark.gpu
def test_device_ssim_known_values(device):
    a, _ = random_pair(33, 47, 3)
    assert np.array_equal(device_means(a, a, device), np.ones((1, 3)))                     # ssim(x, x) == 1 exactly
    s, _ = synth_pair(96, 160, 3)
    assert np.array_equal(device_means(s, s, device), np.ones((1, 3)))
    white, black = np.full((40, 52, 3), 255, np.uint8), np.zeros((40, 52, 3), np.uint8)
    got = device_means(white, black, device)
    want = C1 / (255.0 ** 2 + C1)
    assert abs(want - 9.99900009999e-05) < 1e-15
    assert (np.abs(got - want) <= tol(40, 52)).all(), got


@pytest.mark.gpu
def test_device_ssim_is_bitwise_reproducible_and_batch_independent(device):
    rng = np.random.default_rng(21)
    A = rng.integers(0, 256, (5, 70, 345, 3), dtype=np.uint8)                # two segments across, two bands down
    B = np.clip(A.astype(np.int16) + rng.integers(-20, 21, A.shape), 0, 255).astype(np.uint8)
    ta, tb = torch.from_numpy(A).to(device), torch.from_numpy(B).to(device)
    first = harness.ssim_u8_channel_means(ta, tb)
    for _ in range(9):
        assert np.array_equal(harness.ssim_u8_channel_means(ta, tb), first)
    for i in range(5):
        alone = harness.ssim_u8_channel_means(ta[i:i + 1].clone(), tb[i:i + 1].clone())
        assert np.array_equal(alone[0], first[i]), i
        assert (np.abs(first[i] - exact_ssim(A[i], B[i])) <= tol(70, 345)).all()


@pytest.mark.gpu
def test_device_ssim_full_sid_frame(device):
    h, w = 2848, 4256
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    got = device_means(a, b, device)[0]
    want = exact_ssim(a, b)
    err = np.abs(got - want)
    print(f"full frame: device {got}, max |device - exact| = {err.max():.3e} (bound {tol(h, w):.3e})")
    assert (err <= tol(h, w)).all(), (got, want)


@pytest.mark.gpu
def test_evaluate_reports_device_ssim(device):
    pred = torch.from_numpy(synth.smooth_rgb(5, 3, 96, 160) * 1.2 - 0.1).to(device)
    gt = torch.from_numpy(synth.smooth_rgb(9, 3, 96, 160)).to(device)
    psnr, ssim = harness.evaluate(pred, gt, "RGGB", with_ssim=True)
    psnr_only, none = harness.evaluate(pred, gt, "RGGB")
    assert np.array_equal(psnr, psnr_only) and none.size == 0
    assert ssim.shape == (3,) and ssim.dtype == np.float64
    for i in range(3):
        p8 = H.auto_correct_rb(H.correct_bayer_channels(H.to_uint8_hwc(np.clip(pred[i].cpu().numpy(), 0, 1)), "RGGB"))
        g8 = H.auto_correct_rb(H.correct_bayer_channels(H.to_uint8_hwc(gt[i].cpu().numpy()), "RGGB"))
        assert abs(psnr[i] - H.psnr_u8(p8, g8)) < 1e-9
        assert abs(ssim[i] - float(np.mean(exact_ssim(p8, g8)))) <= tol(96, 160)
        assert abs(ssim[i] - harness.ssim_u8(p8, g8)) < 1e-9


@pytest.mark.gpu
def test_evaluate_loader_reproduces_per_image_evaluate(device, tmp_path):
    from bayer_low_light_image_enhancement_amd import RawFormer
    m = RawFormer(dim=16)
    m.load_state_dict({**m.state_dict(), **cases.model_state(16, 21)}, strict=True)
    m = m.to(device).eval()
    batches = [(torch.from_numpy(synth.bayer_mosaic(21 + 2 * k, 2, 64, 64)), torch.from_numpy(synth.smooth_rgb(40 + 2 * k, 2, 64, 64)))
               for k in range(2)]
    res = harness.evaluate_loader(m, batches, "RGGB")
    psnr, ssim = [], []
    with torch.no_grad():
        for inp, gt in batches:
            out = m(inp.to(device))
            for i in range(inp.shape[0]):                       # test.py's loader has batch size 1: image by image
                p, s = harness.evaluate(out[i:i + 1], gt[i:i + 1].to(device), "RGGB", with_ssim=True)
                psnr.append(float(p[0]))
                ssim.append(float(s[0]))
    assert len(res["psnr"]) == 4 and len(res["ssim"]) == 4
    assert res["psnr"] == psnr and res["ssim"] == ssim          # integer SSE, fixed-order SSIM sums: the same bits image by image
    assert res["psnr_average"] == float(np.mean(res["psnr"])) and res["ssim_average"] == float(np.mean(res["ssim"]))
    assert all(0.0 < v <= 1.0 for v in res["ssim"]) and all(np.isfinite(res["psnr"]))
    harness.write_metrics_csv(str(tmp_path / "test_metrics.csv"), res["psnr"], res["ssim"])
    rows = np.loadtxt(str(tmp_path / "test_metrics.csv"), delimiter=",")
    assert rows.shape == (4, 2) and np.abs(rows[:, 1] - np.array(res["ssim"])).max() <= 5e-5
