"""The hand-written rfft2 / irfft2 (rf_fft.hip; ops.rfft2_polar, ops.polar_irfft2) over its whole advertised range: radix-2 lines
up to 4096, direct-DFT lines up to 2048, more row groups and column tiles than the capped grids (the persistent loops' second
trip), odd heights, the 2 x 2 plane.  tests/test_ffab.py holds the small planes pinned to the reference's own outputs.

Cases: ``cases.FFT_LINE_CASES``, (planes, h, w) each.  The regime every case is there for -- radix 2 or direct per axis, L, TC, trips
per workgroup, LDS bytes -- is read from the library (rf_fft_plan, the plan both launchers launch from) by a CPU test, not copied.

Reference.  Forward: ``torch.fft.rfft2(x.double(), norm='ortho')`` on the CPU.  Inverse, written out so that it does not depend on
what the host's FFT does with a half spectrum that is not Hermitian: ifft along the height of mag e^{i pha} in complex128, the
imaginary parts of columns 0 and w/2 set to zero, irfft(n=w) along the width, both norm='ortho'.  Inputs: ``cases.rnd`` with fixed
seeds; forward uniform in +-1, inverse magnitudes in [0, 2] and phases in +-3 (tests/test_ffab.py).

Bound (the scheme of tests/test_mamba.py and tests/test_wfb_model.py): e64 = max|hip - ref_f64| <= 8 e32 + 2e-6 max|ref_f64|, e32 =
max|ref_f32 - ref_f64| with ref_f32 the same reference computed in float32 on the CPU.  Forward, on two quantities: mag - 1e-6
against |F|, and the complex value (mag - 1e-6) e^{i pha} against F; the phase is never compared as an angle (tests/test_ffab.py says
why).  Every output must be finite.  A float32 emulation of the kernel's direct DFT (sequential accumulation, the kernel's
rounded twiddle argument 2 k / n) lies at 0.40 of the bound at 712 x 1072 and 0.24 at 90 x 2046: the bound admits a correct kernel.

Real bins: the bins (0 | h/2, 0 | w/2) -- for an odd h only the two at y = 0 -- are real by symmetry; their phase must be exactly 0
or float32 pi, agree with the sign of the float64 real part wherever |Re| exceeds the bound, and for power-of-two planes equal the
float32 reference's phase bit for bit.

Measured on the MI355X (``-s`` prints every case; the table is in DESIGN.md section 2), worst e64 / bound per path: radix 2 0.086
forward (2 x 4096 x 64) and 0.048 inverse; direct DFT 0.509 forward (1 x 2047 x 6) and 0.298 inverse; 712 x 1072: 0.425 and 0.278.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from cases import FFT_LINE_CASES, fft_plan, rnd
from bayer_low_light_image_enhancement_amd import _lib

RATIO, FLOOR = 8.0, 2e-6          # tests/test_mamba.py
LDS_LIMIT = 65536                 # dynamic LDS a launch may ask for without opting in to more
PI32 = float(np.float32(np.pi))


def bound(ref32, ref64):
    e32 = float((ref32 - ref64).abs().max())
    return RATIO * e32 + FLOOR * float(ref64.abs().max()), e32


def report(tag, what, got, ref64, ref32):
    """Print e64 and its share of the bound, then assert it."""
    b, e32 = bound(ref32, ref64)
    e64 = float((got - ref64).abs().max())
    msg = f"[{tag}] {what}: e64 {e64:.3e} e32 {e32:.3e} max|ref| {float(ref64.abs().max()):.3e} | bound {b:.3e} ({e64 / b:.3f} of it)"
    print(msg)
    assert e64 <= b, msg
    return b


def irfft2_polar_ref(mag, pha, w):
    """The inverse reference of the module docstring in the precision of its arguments."""
    z = torch.fft.ifft(torch.complex(mag * torch.cos(pha), mag * torch.sin(pha)), dim=-2, norm="ortho")
    z = torch.view_as_real(z).clone()
    z[..., 0, 1] = 0
    z[..., w // 2, 1] = 0
    return torch.fft.irfft(torch.view_as_complex(z), n=w, dim=-1, norm="ortho")


# ------------------------------------------------------------------------------------------ CPU: the plan
@pytest.mark.parametrize("tag", list(FFT_LINE_CASES))
def test_case_reaches_its_regime(tag):
    (planes, h, w), want = FFT_LINE_CASES[tag]
    p = fft_plan(planes, h, w)
    assert {k: p[k] for k in want} == want, (tag, p)
    wf, rows = w // 2 + 1, planes * h
    groups, units = -(-rows // p["L"]), planes * -(-wf // p["TC"])
    assert p["grid"] == (min(groups, 4096), min(units, 4096))
    assert p["trips"] == (-(-groups // p["grid"][0]), -(-units // p["grid"][1]))
    for n, l2 in ((w, p["log2w"]), (h, p["log2h"])):
        assert (l2 >= 0 and 1 << l2 == n) or (l2 == -1 and n & (n - 1) and n <= 2048), (n, l2)
    # a line, and for the direct DFT its output line, of every row / column of the group in LDS, below what a launch may ask for
    assert all(8 * p["L" if a == 0 else "TC"] * n * (2 if l2 < 0 else 1) <= p["lds"][a] <= LDS_LIMIT
               for a, (n, l2) in enumerate(((w, p["log2w"]), (h, p["log2h"])))), p


def test_cases_cover_what_they_are_named_for():
    plans = {t: (s, fft_plan(*s)) for t, (s, _) in FFT_LINE_CASES.items()}
    lds = [p["lds"] for _, p in plans.values()]
    assert plans["r2_row4096"][1]["lds"][0] == max(a for a, _ in lds) and plans["r2_col4096"][1]["lds"][1] == max(b for _, b in lds)
    (_, _, w), p = plans["r2_row4096"]
    assert (w // 2 + 1) % p["TC"] == 1, "the last column tile holds one column"
    (n, h, _), p = plans["row_trip2"]
    assert p["L"] == 1 and p["grid"][0] < n * h < 2 * p["grid"][0], "some workgroups take two lines and some one"
    (n, h, w), p = plans["col_trip2"]
    assert p["TC"] == 1 and p["grid"][1] < n * (w // 2 + 1) < 2 * p["grid"][1]
    (n, h, _), p = plans["ragged_trip2"]
    assert (n * h) % p["L"] == 1 and -(-n * h // p["L"]) > p["grid"][0], "the last group, one live line, belongs to a second trip"
    assert {(p["log2h"] >= 0, p["log2w"] >= 0) for _, p in plans.values()} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(h % 2 == 1 and p["log2h"] < 0 for (_, h, _), p in plans.values()) and (3, 2, 2) in [s for s, _ in plans.values()]
    assert max(h for (_, h, _), p in plans.values() if p["log2h"] < 0) == 2047, "the longest direct column (odd: 2048 is radix 2)"
    assert max(w for (_, _, w), p in plans.values() if p["log2w"] < 0) == 2046, "the longest direct row"


REFUSED = ((8, 7, "width 7 "), (1, 8, "length 1 "), (8, 4098, "length 4098 "), (8, 2050, "length 2050 "), (2049, 8, "length 2049 "))


@pytest.mark.parametrize("h,w,names", REFUSED)
def test_refused_before_any_launch(h, w, names):
    """Fake pointers: a launch would not come back with -22."""
    lib = _lib.load()
    fake = C.c_void_p(1 << 12)
    for rc in (lib.rf_fft_plan(1, h, w, (C.c_int * 10)()), lib.rf_rfft2_polar(fake, fake, fake, fake, 1, h, w, None),
               lib.rf_polar_irfft2(fake, fake, fake, fake, 1, h, w, None)):
        assert rc == -22 and names.encode() in lib.rf_last_error(), (rc, lib.rf_last_error())


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(FFT_LINE_CASES))
def test_forward(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    (planes, h, w), _ = FFT_LINE_CASES[tag]
    x = rnd(f"fftl.{tag}.x", (1, planes, h, w), seed=81)
    mag, pha = ops.rfft2_polar(x.to(device))
    mag, pha = mag.cpu(), pha.cpu()
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(pha).all())
    f64, f32 = torch.fft.rfft2(x.double(), norm="ortho"), torch.fft.rfft2(x, norm="ortho")
    m = mag.double() - 1e-6
    report(tag, "|F|", m, f64.abs(), f32.abs().double())
    b = report(tag, "F", torch.polar(m, pha.double()), f64, f32.to(torch.complex128))
    for y in {0, h // 2} if h % 2 == 0 else {0}:
        for xx in {0, w // 2}:
            got, re = pha[..., y, xx], f64.real[..., y, xx]
            assert bool(((got == 0) | (got == PI32)).all()), (tag, y, xx, got)
            clear = re.abs() > b
            assert torch.equal(got[clear] == PI32, re[clear] < 0), (tag, y, xx)
            if h & (h - 1) == 0 and w & (w - 1) == 0:
                assert torch.equal(got, torch.angle(f32)[..., y, xx]), (tag, y, xx)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(FFT_LINE_CASES))
def test_inverse(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    (planes, h, w), _ = FFT_LINE_CASES[tag]
    shape = (1, planes, h, w // 2 + 1)
    mag, pha = rnd(f"fftl.{tag}.mag", shape, 0.0, 2.0, seed=82), rnd(f"fftl.{tag}.pha", shape, -3.0, 3.0, seed=83)
    out = ops.polar_irfft2(mag.to(device), pha.to(device), w).cpu()
    assert bool(torch.isfinite(out).all())
    report(tag, "irfft2", out.double(), irfft2_polar_ref(mag.double(), pha.double(), w), irfft2_polar_ref(mag, pha, w).double())
