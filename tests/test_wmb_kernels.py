"""The three fused passes of the WFB handle's WMB block (csrc/rf_wmb.hip) through their thin entry points ops.wmb_front /
ops.wmb_back / ops.wmb_ffn_tail, against float64.

Shapes [B, C, H, W] (full resolution): C = 16 / 48 / 256; W = 4 (one lane per row pair), widths that are no multiple of a
workgroup's strip (20, 12, 40), and 2 x 16 x 36 x 40 = 360 row-pair items: more than one 256-lane workgroup.
Tolerance 2e-5 max-abs, the operator tolerance of DESIGN.md section 2; the front kernel's bands must equal ops.dwt_init of its
own t bit for bit (dwt_init's expression order).
"""
import ctypes as C

import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

TOL = 2e-5
SHAPES = ((2, 16, 6, 4), (1, 48, 10, 20), (1, 256, 4, 12), (2, 16, 36, 40))


def inputs(shape):
    b, c, h, w = shape
    x = cases.rnd(f"wmbk.x.{shape}", shape, -2.0, 2.0, seed=90)
    gw, gb = cases.rnd(f"wmbk.w.{c}", (c,), 0.8, 1.2, seed=90), cases.rnd(f"wmbk.b.{c}", (c,), -0.3, 0.3, seed=90)
    return x, gw, gb


def test_entry_points_refuse_bad_shapes_before_any_launch():
    lib = _lib.load()
    fake = C.c_void_p(1 << 12)
    assert lib.rf_wmb_front(fake, fake, fake, fake, fake, 1, 16, 4, 3, None) == -22 and b"multiple of 4" in lib.rf_last_error()
    assert lib.rf_wmb_front(fake, fake, fake, fake, fake, 1, 1024, 4, 4, None) == -22 and b"512" in lib.rf_last_error()
    assert lib.rf_wmb_back(fake, fake, C.c_void_p(4), 1, 16, 4, 4, None) == -22 and b"aligned" in lib.rf_last_error()
    assert lib.rf_wmb_ffn_sum(fake, fake, fake, fake, fake, 1, 16, 4, 6, None) == -22 and b"multiple of 4" in lib.rf_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_front(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    x, gw, gb = inputs(shape)
    w2, b2 = (2.0 * gw).contiguous(), (2.0 * gb - 1.0).contiguous()
    t, bands = ops.wmb_front(x.to(device), w2.to(device), b2.to(device))
    assert torch.equal(bands, ops.dwt_init(t)), "the bands are not dwt_init of the kernel's own t"
    want = 2.0 * R.layernorm2d(x.double(), gw.double(), gb.double()) - 1.0
    err = float((t.cpu().double() - want).abs().max())
    print(f"front {shape}: t max-abs {err:.3e}")
    assert err <= TOL
    assert float((bands.cpu().double() - R.dwt_init(want)).abs().max()) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_back(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w = shape
    t = cases.rnd(f"wmbk.t.{shape}", shape, -3.0, 3.0, seed=91)
    bands = cases.rnd(f"wmbk.bands.{shape}", (4 * b, c, h // 2, w // 2), -1.5, 1.5, seed=91)      # IWT in +-3: both clamp ends are reached
    out = ops.wmb_back(bands.to(device), t.to(device))
    inner = (R.iwt_init(bands.double()) + 1.0) / 2.0
    assert float((inner < 0).double().mean()) > 0.05 and float((inner > 1).double().mean()) > 0.05
    err = float((out.cpu().double() - (t.double() + inner.clamp(0.0, 1.0))).abs().max())
    print(f"back {shape}: max-abs {err:.3e}")
    assert err <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_ffn_tail(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    t, gw, gb = inputs(shape)
    y = cases.rnd(f"wmbk.y.{shape}", shape, -2.0, 2.0, seed=92)
    out = ops.wmb_ffn_tail(t.to(device), y.to(device), gw.to(device), gb.to(device))
    want = t.double() + y.double() + R.layernorm2d(t.double(), gw.double(), gb.double())
    err = float((out.cpu().double() - want).abs().max())
    print(f"ffn_tail {shape}: max-abs {err:.3e}")
    assert err <= TOL
