"""The kernels of csrc/rf_truecolor.hip one by one, against the oracle (oracle/rawformer_ref.py) in float64 on the test's own inputs:

  front end + guidance   RawFormer.tc_guidance (rf_tc_guidance): tc_front / tc_normalise / tc_pyramid / tc_add / tc_guide_level
  tc_pyramid             ops.tc_pyramid, odd sides included (the reflect branch, which no model shape reaches)
  tc_spatial             ops.tc_spatial, float4 and scalar forms, channel-group borders, second workgroups
  tc_residual            ops.tc_residual: x2 and the squeeze-excite pooling sums, block by block (also multilvl's last step)
  tc_color_head          ops.tc_color_head: clamp ends, pow near 0, the grid cap
  stage                  RawFormer.forward_stage, stages 1 and 4

Tolerances.  Operators: TOL = 2e-5 max-abs, relative to max(1, max|want|) of the compared tensor.  Stage:
5e-5, the stage bound of tests/test_multilvl.py and tests/test_gpu_model.py.  Bit-equality checks have none.  No case needed the
float32-floor rule of test_truecolor.test_oracle_matches_the_reference.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cases
from bayer_low_light_image_enhancement_amd import RawFormer, _lib, synth
from oracle import rawformer_ref as R

TOL = 2e-5
STAGE_TOL = 5e-5
DIM = 16
PLANES = ("y", "cr", "cb", "R", "G", "y_low", "y_high")
BP = "bayer_processor."
_SD, _MODEL = {}, {}


# ------------------------------------------------------------------------------------------------ shared inputs
def state(levels=2):
    """Synthetic weights by name, as ``state()`` of tests/test_truecolor.py makes them (dim 16)."""
    if levels not in _SD:
        sd = RawFormer(dim=DIM, variant="truecolor", flca_levels=levels).state_dict()
        synth.fill_state_dict(sd, 4000 + DIM)
        _SD[levels] = sd
    return {k: v.clone() for k, v in _SD[levels].items()}


def f64(sd):
    return {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}


def model(device, levels=2, sd=None):
    """The dim-16 model with the synthetic weights (built once per pyramid depth), or a fresh one with ``sd``."""
    if sd is not None:
        m = RawFormer(dim=DIM, variant="truecolor", flca_levels=levels)
        m.load_state_dict(sd, strict=True)
        return m.to(device).eval()
    if (levels, str(device)) not in _MODEL:
        _MODEL[levels, str(device)] = model(device, levels, state(levels))
    return _MODEL[levels, str(device)]


def err_of(got, want):
    """max-abs error relative to max(1, max|want|)."""
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def raw_luma(x4, sd):
    """The luma before its normalisation, [B,1,H,W]: the first lines of R.enhanced_bayer_processor (white balance, colour matrix,
    BT.709 weights), for the coverage assertions on the frame maximum."""
    wb = x4 * (F.softplus(sd[BP + "wb_gains"]) + 1e-6).view(1, 4, 1, 1)
    rgb = torch.cat([wb[:, 0:1], 0.5 * (wb[:, 1:2] + wb[:, 2:3]), wb[:, 3:4]], dim=1)
    m = sd[BP + "color_matrix"]
    lin = torch.einsum("bchw,oc->bohw", rgb, m[:, :3]) + m[:, 3].view(1, 3, 1, 1)
    return (lin * torch.tensor([0.2126, 0.7152, 0.0722]).view(1, 3, 1, 1)).sum(dim=1, keepdim=True)


FRAMES = {"b2_16x24": (2, 16, 24), "b1_8x40": (1, 8, 40)}      # 8 x 40: level widths 40, 20, 10, 5 and a single row at level 3


def frame(tag):
    b, h, w = FRAMES[tag]
    return cases.rnd(f"tck.packed.{tag}", (b, 4, h, w), 0.0, 1.0, seed=95)


def negative_case():
    """A colour-matrix bias column of -2: image 0 (a frame in [0, 0.5]) has a negative luma everywhere, image 1 (in [0, 4]) has not."""
    sd = state()
    sd[BP + "color_matrix"][:, 3] = -2.0
    x4 = cases.rnd("tck.packed.neg", (2, 4, 16, 24), 0.0, 0.5, seed=96)
    x4[1] *= 8.0
    return sd, x4


SPATIAL_SHAPES = ((2, 16, 6, 8),        # float4 form, half a channel group
                  (1, 48, 5, 7),        # scalar form, C no multiple of 32
                  (1, 33, 4, 12),       # a one-channel last group
                  (2, 64, 36, 32),      # 1152 pixels: a second float4 workgroup with a partial tail
                  (1, 16, 19, 15))      # 285 pixels: a second scalar workgroup
RESIDUAL_SHAPES = SPATIAL_SHAPES + ((1, 512, 2, 4),       # the C limit
                                    (1, 300, 3, 5))       # the `c += 256` tail of the final loop


def flca_spec(c):
    return {"color_attention.0.weight": (c, 5, 3, 3), "color_attention.0.bias": (c,), "low_attn.0.weight": (c, 1, 3, 3),
            "low_attn.0.bias": (c,), "high_attn.0.weight": (c, 1, 3, 3), "high_attn.0.bias": (c,)}


def spatial_inputs(shape, guide_scale=1.0):
    b, c, h, w = shape
    feat = cases.rnd(f"tck.feat.{shape}", shape, -2.0, 2.0, seed=97)
    guide = cases.rnd(f"tck.guide.{shape}", (b, 7, h, w), -1.0, 1.0, seed=97) * guide_scale
    return feat, guide, cases.params(flca_spec(c), seed=4100 + c)


def spatial_sums(guide, p):
    """The three pre-activation convolution sums of R.enhanced_flca's first lines, float64."""
    g, p = guide.double(), f64(p)
    return (F.conv2d(g[:, 0:5], p["color_attention.0.weight"], p["color_attention.0.bias"], padding=1),
            F.conv2d(g[:, 5:6], p["low_attn.0.weight"], p["low_attn.0.bias"], padding=1),
            F.conv2d(g[:, 6:7], p["high_attn.0.weight"], p["high_attn.0.bias"], padding=1))


def spatial_want(feat, guide, p):
    col, low, high = spatial_sums(guide, p)
    return feat.double() * (1.0 + torch.sigmoid(col) + torch.tanh(torch.sigmoid(low) + torch.tanh(high)))


SATURATION_SCALE = 1000.0      # the sums of the unit-range guide have a spread of about 0.5

# colour head: B = 2; launch_tc_color_head caps its grid at max(4096 / B, 64) workgroups of 256 pixels per image
COLOR_B = 2
COLOR_CAP_PIXELS = max(4096 // COLOR_B, 64) * 256
COLOR_P = (5, 256, 1030, COLOR_CAP_PIXELS + 261)        # the last: every workgroup takes a second trip, the last 261 pixels' worth
CC = "color_correction."


def color_inputs(p_count):
    """Uniform in [-0.25, 1.25]; image 0 starts with the exact values 0, 1 and 1e-6; image 1 holds a block of values in [0, 1e-4]."""
    x = cases.rnd(f"tck.color.{p_count}", (COLOR_B, 3, p_count), -0.25, 1.25, seed=98)
    x[0, :, 0], x[0, :, 1], x[0, :, 2] = 0.0, 1.0, 1e-6
    n = min(64, p_count - 3)
    x[1, :, 3:3 + n] = cases.rnd(f"tck.color.tiny.{p_count}", (3, n), 0.0, 1e-4, seed=98)
    return x


def color_params(big_gamma):
    sd = {k: v for k, v in state().items() if k.startswith(CC)}
    if big_gamma:
        sd[CC + "gamma_param"].fill_(25.0)      # softplus takes its x > 20 branch: gamma = 25
    return sd


def color_want(x, sd):
    """R.camera_color_correction in float64, in pieces of 64k pixels (the function is per pixel)."""
    p = f64(sd)
    return torch.cat([R.camera_color_correction(part.double().unsqueeze(2), p, CC).squeeze(2) for part in x.split(1 << 16, dim=2)], dim=2)


# ------------------------------------------------------------------------------------------------ no GPU
def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake, off4 = C.c_void_p(1 << 12), C.c_void_p((1 << 12) + 4)
    err = lib.rf_last_error
    assert lib.rf_tc_spatial(fake, None, fake, fake, fake, fake, fake, fake, fake, 1, 16, 4, 4, None) == -22 and b"null" in err()
    assert lib.rf_tc_spatial(*[fake] * 9, 1, 513, 4, 4, None) == -22 and b"512" in err()
    assert lib.rf_tc_spatial(*[fake] * 9, 0, 16, 4, 4, None) == -22 and b"positive" in err()
    assert lib.rf_tc_spatial(*[fake] * 8, C.c_void_p((1 << 12) + 2), 1, 16, 4, 4, None) == -22 and b"aligned" in err()
    assert lib.rf_tc_residual(fake, fake, fake, fake, 1, 513, 2, 4, None) == -22 and b"512" in err()
    assert lib.rf_tc_residual(fake, fake, off4, fake, 1, 16, 2, 4, None) == -22 and b"16-byte aligned" in err()
    assert lib.rf_tc_residual(fake, fake, fake, None, 1, 16, 2, 4, None) == -22 and b"null" in err()
    assert lib.rf_tc_residual(fake, fake, fake, fake, 1, 16, 0, 4, None) == -22 and b"positive" in err()
    assert lib.rf_tc_nblk(0, 4) == -22
    assert (lib.rf_tc_nblk(36, 32), lib.rf_tc_nblk(19, 15), lib.rf_tc_nblk(2, 4), lib.rf_tc_nblk(32, 32)) == (2, 2, 1, 1)
    assert lib.rf_tc_color_head(*[fake] * 5, None, *[fake] * 4, 1, 16, None) == -22 and b"null" in err()
    assert lib.rf_tc_color_head(*[fake] * 10, 0, 16, None) == -22 and b"B=0" in err()
    assert lib.rf_tc_color_head(*[fake] * 10, 1, 0, None) == -22 and b"P=0" in err()
    assert lib.rf_tc_pyramid(fake, fake, fake, 1, 1, 8, None) == -22 and b"pyramid" in err()
    assert lib.rf_tc_pyramid(fake, None, fake, 1, 8, 8, None) == -22 and b"null" in err()
    assert lib.rf_tc_pyramid(fake, fake, fake, 0, 8, 8, None) == -22 and b"B=0" in err()

    def handle(variant):
        cfg = _lib.RfConfig(DIM, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, 2, variant, 1, 0, 2)
        h = C.c_void_p()
        assert lib.rf_create(C.byref(cfg), C.byref(h)) == 0
        return h
    tc, flca = handle(_lib.RF_VARIANT_TRUECOLOR), handle(_lib.RF_VARIANT_FLCA)
    try:
        args = (fake, fake, fake, fake, fake, 1 << 30, 1, 16, 24, None)       # y, crcb, rgb, guide, workspace, bytes, B, H, W, stream
        assert lib.rf_tc_guidance(tc, None, 0, *args) == -22 and b"null" in err()
        assert lib.rf_tc_guidance(flca, fake, 0, *args) == -22 and b"TrueColor" in err()
        assert lib.rf_tc_guidance(tc, fake, 4, *args) == -22 and b"level" in err()
        assert lib.rf_tc_guidance(tc, fake, 0, fake, fake, fake, fake, fake, 1 << 30, 1, 12, 24, None) == -22 and b"multiples of 8" in err()
        assert lib.rf_tc_guidance(tc, fake, 0, *args) == -2 and b"not packed" in err()
        # the stage of this variant derives its guidance from the packed frame
        assert lib.rf_forward_stage(tc, 1, fake, None, fake, fake, 1 << 30, 1, 16, 24, None) == -22 and b"packed frame" in err()
        assert lib.rf_forward_stage(tc, 1, fake, fake, fake, fake, 1 << 30, 1, 16, 24, None) == -2 and b"not packed" in err()
    finally:
        lib.rf_destroy(tc)
        lib.rf_destroy(flca)


def test_negative_luma_inputs_reach_both_atomics():
    """atomic_max_float takes atomicMin on the bit pattern for negative values: image 0's luma must be negative everywhere, so
    that its maximum is found there and the eps clamp applies; image 1's maximum must be positive."""
    sd, x4 = negative_case()
    assert float(x4[0].min()) >= 0.0 and float(x4[0].max()) <= 1.0
    raw = raw_luma(x4.double(), f64(sd))
    assert float(raw[0].max()) < 0.0 < float(raw[1].max())
    assert float(raw[1].min()) < 0.0                # both atomics inside one image too
    y = R.enhanced_bayer_processor(x4.double(), f64(sd), BP)[0]
    assert float(y[0].abs().max()) > 1e6            # image 0 is divided by eps


def test_saturation_inputs_reach_beyond_100():
    feat, guide, p = spatial_inputs(SPATIAL_SHAPES[0], SATURATION_SCALE)
    for name, s in zip(("color", "low", "high"), spatial_sums(guide, p)):
        assert float(s.min()) < -100.0 and float(s.max()) > 100.0, name


@pytest.mark.parametrize("p_count", COLOR_P)
def test_color_head_inputs_reach_both_clamp_ends(p_count):
    x = color_inputs(p_count)
    assert float((x < 0).double().mean()) > 0.05 and float((x > 1).double().mean()) > 0.05
    assert float(x[0, 0, 0]) == 0.0 and float(x[0, 1, 1]) == 1.0 and float(x[0, 2, 2]) == float(torch.tensor(1e-6))
    tiny = x[1, :, 3:3 + min(64, p_count - 3)]
    assert float(tiny.min()) >= 0.0 and float(tiny.max()) <= 1e-4
    if p_count == COLOR_P[-1]:
        assert p_count > COLOR_CAP_PIXELS and (p_count + 255) // 256 > max(4096 // COLOR_B, 64)      # the cap binds


def test_color_head_large_gamma_takes_softplus_linear_branch():
    assert float(color_params(True)[CC + "gamma_param"]) > 20.0 > float(color_params(False)[CC + "gamma_param"])


# ------------------------------------------------------------------------------------------------ front end and guidance
@pytest.mark.gpu
@pytest.mark.parametrize("levels", (1, 2, 3))
@pytest.mark.parametrize("tag", list(FRAMES))
def test_front_and_guidance(device, tag, levels):
    """EnhancedBayerProcessor's four outputs and the seven guidance planes at every U-Net level, for every pyramid depth the
    constructor admits."""
    b, h, w = FRAMES[tag]
    x4, sd = frame(tag), f64(state(levels))
    want = R.enhanced_bayer_processor(x4.double(), sd, BP)
    m = model(device, levels)
    worst = {}
    for lvl in range(4):
        y, crcb, rgb, guide = m.tc_guidance(x4.to(device), lvl)
        got = {"y": y, "cr": crcb[:, 0:1], "cb": crcb[:, 1:2], "rgb": rgb}
        for name, ref in zip(("y", "cr", "cb", "rgb"), want):
            e = err_of(got[name], ref)
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= TOL, f"{name} (call for level {lvl}): {e:.3e}"
        g = R.enhanced_flca_guidance(*want, (h >> lvl, w >> lvl), levels)
        assert guide.shape == g.shape
        for i, name in enumerate(PLANES):
            e = err_of(guide[:, i], g[:, i])
            worst[f"guide.{name}"] = max(worst.get(f"guide.{name}", 0.0), e)
            assert e <= TOL, f"guidance plane {name} at level {lvl} ({h >> lvl} x {w >> lvl}), {levels} pyramid level(s): {e:.3e}"
    print(f"front {tag} levels={levels}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.gpu
def test_frame_maximum_is_per_image(device):
    """Image 1 is image 0 scaled by 0.25: each is normalised by its own maximum."""
    x4 = cases.rnd("tck.packed.scaled", (2, 4, 16, 24), 0.0, 1.0, seed=95)
    x4[1] = 0.25 * x4[0]
    want = R.enhanced_bayer_processor(x4.double(), f64(state()), BP)[0]
    y = model(device).tc_guidance(x4.to(device), 0)[0].cpu()
    e = err_of(y, want)
    print(f"per-image maximum: y {e:.3e}, max(y) = {[float(v) for v in y.amax(dim=(1, 2, 3))]}")
    assert e <= TOL
    assert float((y.amax(dim=(1, 2, 3)) - 1.0).abs().max()) <= TOL and float((want.amax(dim=(1, 2, 3)) - 1.0).abs().max()) < 1e-12


@pytest.mark.gpu
def test_negative_luma_maximum(device):
    """Image 0's luma is negative everywhere (test_negative_luma_inputs_reach_both_atomics): its maximum goes through the
    atomicMin form and then the eps clamp, so y is of order 1e6 there; image 1 takes its true, positive maximum."""
    sd, x4 = negative_case()
    want = R.enhanced_bayer_processor(x4.double(), f64(sd), BP)[0]
    y = model(device, sd=sd).tc_guidance(x4.to(device), 0)[0].cpu()
    assert bool(torch.isfinite(y).all())
    for i in range(2):
        e = err_of(y[i], want[i])
        print(f"negative luma, image {i}: y {e:.3e} of max|want| {float(want[i].abs().max()):.3e}")
        assert e <= TOL, f"image {i}"


@pytest.mark.gpu
def test_zero_frame(device):
    sd = state()
    sd[BP + "color_matrix"][:, 3] = 0.0
    x4 = torch.zeros((2, 4, 16, 24))
    y = model(device, sd=sd).tc_guidance(x4.to(device), 0)[0].cpu()
    assert bool(torch.isfinite(y).all()) and bool((y == 0).all())


# ------------------------------------------------------------------------------------------------ tc_pyramid
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", ((2, 2), (2, 3), (3, 2), (5, 7), (8, 8), (33, 18), (40, 52)))
def test_pyramid(device, h, w):
    """Odd sides take the reflect branch (source index n -> n - 2); 40 x 52 has 520 outputs, so a second workgroup."""
    from bayer_low_light_image_enhancement_amd import ops
    src = cases.rnd(f"tck.pyr.{h}x{w}", (3, 1, h, w), -1.0, 1.0, seed=99)
    ll, mag = ops.tc_pyramid(src.to(device))
    wll, (lh, hl, hh) = R.haar_dwt(src.double())
    wmag = torch.sqrt(lh * lh + hl * hl + hh * hh + 1e-8)
    assert ll.shape == wll.shape and mag.shape == wmag.shape
    e = (err_of(ll, wll), err_of(mag, wmag))
    print(f"pyramid {h}x{w}: LL {e[0]:.3e}, magnitude {e[1]:.3e}")
    assert max(e) <= TOL


# ------------------------------------------------------------------------------------------------ tc_spatial
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SPATIAL_SHAPES)
def test_spatial(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    feat, guide, p = spatial_inputs(shape)
    out = ops.tc_spatial(feat.to(device), guide.to(device), {k: v.to(device) for k, v in p.items()})
    e = err_of(out, spatial_want(feat, guide, p))
    print(f"spatial {shape}: {e:.3e}")
    assert e <= TOL


@pytest.mark.gpu
def test_spatial_saturated(device):
    """Convolution sums beyond +-100 (test_saturation_inputs_reach_beyond_100): sigmoid and tanh sit at their limits, exp overflows
    on one side; the output stays finite and at the float64 value."""
    from bayer_low_light_image_enhancement_amd import ops
    feat, guide, p = spatial_inputs(SPATIAL_SHAPES[0], SATURATION_SCALE)
    out = ops.tc_spatial(feat.to(device), guide.to(device), {k: v.to(device) for k, v in p.items()})
    assert bool(torch.isfinite(out).all())
    e = err_of(out, spatial_want(feat, guide, p))
    print(f"spatial saturated: {e:.3e}")
    assert e <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in SPATIAL_SHAPES if s[1] % 32])
def test_spatial_stays_inside_its_channels(device, shape):
    """A workgroup owns up to 32 channels; the last group of an image ends at C.  Every operand sits at the head of a longer
    buffer (32 more channels' worth), the output's tail holds a sentinel: it must be untouched, and the result the same bits as
    the plain call's."""
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w = shape
    feat, guide, p = spatial_inputs(shape)
    sentinel = 12345.0

    def headed(t, per_channel):
        buf = torch.full((t.numel() + 32 * per_channel,), sentinel, dtype=torch.float32, device=device)
        buf[: t.numel()] = t.reshape(-1).to(device)
        return buf, buf[: t.numel()].view(t.shape)
    pd = {k: headed(v, v[0].numel())[1] for k, v in p.items()}
    xbuf, xs = headed(torch.zeros(shape), h * w)
    ops.tc_spatial(headed(feat, h * w)[1], guide.to(device), pd, out=xs)
    assert bool((xbuf[xs.numel():] == sentinel).all()), "written past the last channel"
    assert torch.equal(xs, ops.tc_spatial(feat.to(device), guide.to(device), {k: v.to(device) for k, v in p.items()}))


# ------------------------------------------------------------------------------------------------ tc_residual
@pytest.mark.gpu
@pytest.mark.parametrize("shape", RESIDUAL_SHAPES)
def test_residual(device, shape):
    """x2, the pooling sums per image and channel, and every block's own sum (1024 consecutive pixels where w % 4 == 0, else 256);
    two calls give the same bits, and so does writing x2 over xs as the forward does."""
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w = shape
    xs = cases.rnd(f"tck.xs.{shape}", shape, -2.0, 2.0, seed=100)
    r = cases.rnd(f"tck.r.{shape}", shape, -50.0, 50.0, seed=100)
    x2, partial = ops.tc_residual(xs.to(device), r.to(device))
    want = xs.double() + 0.2 * torch.tanh(r.double())
    blk = 1024 if w % 4 == 0 else 256
    nblk = -(-h * w // blk)
    assert ops.tc_nblk(h, w) == nblk and tuple(partial.shape) == (b, nblk, c)
    wblocks = F.pad(want.reshape(b, c, h * w), (0, nblk * blk - h * w)).reshape(b, c, nblk, blk).sum(dim=3).permute(0, 2, 1)
    e = (err_of(x2, want), err_of(partial.sum(dim=1), want.sum(dim=(2, 3))), err_of(partial, wblocks))
    print(f"residual {shape}: x2 {e[0]:.3e}, channel sums {e[1]:.3e}, block sums {e[2]:.3e}")
    assert e[0] <= TOL, "x2"
    assert e[1] <= TOL, "channel sums"
    assert e[2] <= TOL, "block sums"
    again, partial_again = ops.tc_residual(xs.to(device), r.to(device))
    assert torch.equal(x2, again) and torch.equal(partial, partial_again), "two calls differ"
    inplace = xs.to(device)
    over, partial_over = ops.tc_residual(inplace, r.to(device), out=inplace)
    assert over.data_ptr() == inplace.data_ptr() and torch.equal(over, x2) and torch.equal(partial_over, partial), "in place differs"


@pytest.mark.gpu
def test_residual_refuses_more_than_512_channels(device):
    from bayer_low_light_image_enhancement_amd import ops
    x = torch.zeros((1, 513, 2, 4), device=device)
    with pytest.raises(RuntimeError, match="512"):
        ops.tc_residual(x, x)
    out = torch.empty_like(x)
    part = torch.empty((1, 1, 513), device=device)
    rc = _lib.load().rf_tc_residual(*[C.c_void_p(t.data_ptr()) for t in (x, x, out, part)], 1, 513, 2, 4, None)
    assert rc == -22 and b"512" in _lib.load().rf_last_error()


# ------------------------------------------------------------------------------------------------ tc_color_head
@pytest.mark.gpu
@pytest.mark.parametrize("big_gamma", (False, True))
@pytest.mark.parametrize("p_count", COLOR_P)
def test_color_head(device, p_count, big_gamma):
    """Inputs past both clamp ends, the exact values 0, 1 and 1e-6 and a block in [0, 1e-4] (pow's steep end); gamma from the
    synthetic weights and gamma = 25 (softplus's linear branch; 1 / gamma = 0.04).  The last size takes the grid-stride loop's
    second trip (test_color_head_inputs_reach_both_clamp_ends)."""
    from bayer_low_light_image_enhancement_amd import ops
    x, sd = color_inputs(p_count), color_params(big_gamma)
    out = ops.tc_color_head(x.to(device), {k: v.to(device) for k, v in sd.items()}, CC).cpu()
    want = color_want(x, sd)
    e = err_of(out, want)
    print(f"color head P={p_count} gamma_param={float(sd[CC + 'gamma_param']):.3f}: {e:.3e}, range [{float(out.min())}, {float(out.max())}]")
    assert e <= TOL
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


# ------------------------------------------------------------------------------------------------ one stage
@pytest.mark.gpu
@pytest.mark.parametrize("stage", (1, 4))
def test_forward_stage(device, stage):
    """One EnhancedConv_Transformer at U-Net level 0 (stage 1: C = 16 at 32 x 48) and level 3 (stage 4: C = 128 at 4 x 6) of a
    32 x 48 packed frame, B = 2: front end, guidance at that level, block, branch (spatial gate, res_proj, residual, squeeze-excite
    fold), channel_reduce, Conv_out."""
    lvl = stage - 1
    sd = f64(state())
    x4 = R.pixel_unshuffle2(torch.from_numpy(synth.bayer_mosaic(99, 2, 64, 96)))
    xin = torch.from_numpy(synth.uniform(100 + stage, "tck.stage.x", (2, DIM << lvl, 32 >> lvl, 48 >> lvl), -1.0, 1.0))
    with torch.no_grad():
        ref = R.truecolor_stage(xin.double(), R.enhanced_bayer_processor(x4.double(), sd, BP), sd, f"conv_tran{stage}.", 8)
        out = model(device).forward_stage(stage, xin.to(device), x4.to(device)).cpu()
    e = float((out.double() - ref).abs().max())
    print(f"stage {stage}: max-abs error {e:.3e} (max|ref| {float(ref.abs().max()):.3f})")
    assert e <= STAGE_TOL
