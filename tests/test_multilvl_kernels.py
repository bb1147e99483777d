"""The kernels of csrc/rf_multilvl.hip one by one, against float64 on the CPU from the test's own inputs (tests/multilvl_ref.py,
oracle/rawformer_ref.py):

  ml_guide_level, ml_means   RawFormer.ml_guidance (rf_ml_guidance): every plane by name and every used mean, all depths and levels
  ml_modulate<1|4, *>        ops.ml_modulate: float4 and scalar forms, channel-group tails, second workgroups, every step of every depth
  ml_residual<1|4>           ops.ml_residual: vector and scalar forms, in place
  ml_step_fused<C, *>        ops.ml_step_fused: C = 16, 32, 48, 64, both forms, the pooling sums block by block
  ml_tail_sums/delta/apply   RawFormer.ml_tail (rf_ml_tail): past both grid caps, on a non-constant image
  stage, model               RawFormer.forward_stage and forward at dim 16 / 24 / 48 and depth 1 / 2

Tolerances.  Operators: TOL = 2e-5 max-abs, relative to max(1, max|want|) of the compared tensor.  Stage and
model: 5e-5, the bound of tests/test_multilvl.py.  Bit-equality checks have none.  No case needed the float32-floor rule: the
restatement's own float32-against-float64 error on the three model cases is 1.6e-6 .. 2.0e-6, below the 1.2e-5 where it would apply.

The grid caps the large cases are sized by (csrc/rf_multilvl.hip): kMlGuideBlocks = 256 workgroups per image for ml_guide_level_kernel
(line 27; launch_ml_guide_level), kMlTailBlocks = 1024 for ml_tail_sums_kernel (line 28; launch_ml_tail), 4096 for ml_tail_apply_kernel
(`if (gx > 4096)` in launch_ml_tail).  test_cases_reach_the_branches_they_are_named_for restates the launch arithmetic.
"""
import ctypes as C
import gc

import pytest
import torch
import torch.nn.functional as F

import cases
import multilvl_ref as M
from bayer_low_light_image_enhancement_amd import RawFormer, _lib, synth
from oracle import rawformer_ref as R

TOL = 2e-5
STAGE_TOL = 5e-5
DIM = 16
GUIDE_CAP, TAIL_SUMS_CAP, TAIL_APPLY_CAP = 256, 1024, 4096      # workgroups per image, see the module docstring
_SD, _MODEL = {}, {}


# ------------------------------------------------------------------------------------------------ shared inputs
def state(dim=DIM, levels=2):
    """Synthetic weights by name, as ``state()`` of tests/test_multilvl.py makes them."""
    if (dim, levels) not in _SD:
        sd = RawFormer(dim=dim, variant="multilvl", flca_levels=levels).state_dict()
        synth.fill_state_dict(sd, 5000 + dim)
        _SD[dim, levels] = sd
    return {k: v.clone() for k, v in _SD[dim, levels].items()}


def f64(sd):
    return {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}


def model(device, dim=DIM, levels=2, fresh=False):
    """The model with the synthetic weights, built once per configuration; ``fresh``: one of the caller's own, whose workspace goes
    with it."""
    if fresh:
        m = RawFormer(dim=dim, variant="multilvl", flca_levels=levels)
        m.load_state_dict(state(dim, levels), strict=True)
        return m.to(device).eval()
    if (dim, levels, str(device)) not in _MODEL:
        _MODEL[dim, levels, str(device)] = model(device, dim, levels, fresh=True)
    return _MODEL[dim, levels, str(device)]


def err_of(got, want):
    """max-abs error relative to max(1, max|want|)."""
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def on(device, p):
    return {k: v.to(device) for k, v in p.items()}


# ---- guidance
FRAMES = {"b2_16x24": (2, 16, 24), "b1_8x40": (1, 8, 40)}      # 8 x 40: level widths 40, 20, 10, 5 and a single row at level 3
BIG_GUIDE = (1, 264, 256)      # 67 584 pixels at level 0: workgroups 0..7 of the 256 take a second trip


def frame(tag):
    b, h, w = FRAMES[tag]
    return cases.rnd(f"mlk.packed.{tag}", (b, 4, h, w), 0.0, 1.0, seed=195)


def big_guide_frame():
    """Uniform in [0, 0.25] but for the last 8 rows, which lie in [0.75, 1]: exactly the pixels of the second trip."""
    b, h, w = BIG_GUIDE
    x4 = cases.rnd("mlk.packed.big", (b, 4, h, w), 0.0, 0.25, seed=196)
    x4[:, :, h - 8:] += 0.75
    return x4


def plane_names(levels):
    return [n for l in range(levels) for n in (f"y_low_{l}", f"y_high_{l}")] + ["cr", "cb"]


def guidance_ref(x4, levels, lvl, resize=R.bilinear_resize, shift=0):
    """float64: the 2 L + 2 planes by name at U-Net level ``lvl`` and the means the gates use (``chroma`` = that of
    sqrt(cr^2 + cb^2 + 1e-8)).  ``resize`` and ``shift`` (pyramid level l + shift in place of l) are for the defect test."""
    x4 = x4.double()
    y, cr, cb = R.bayer_luma_chroma(x4)
    lows, highs = M.pyramid(y, levels + shift)
    size = (x4.shape[2] >> lvl, x4.shape[3] >> lvl)
    planes = {}
    for l in range(levels):
        planes[f"y_low_{l}"], planes[f"y_high_{l}"] = resize(lows[l + shift], size), resize(highs[l + shift], size)
    planes["cr"], planes["cb"] = resize(cr, size), resize(cb, size)
    means = {n: v.mean(dim=(1, 2, 3)) for n, v in planes.items() if n.startswith("y_")}
    means["chroma"] = torch.sqrt(planes["cr"] ** 2 + planes["cb"] ** 2 + 1e-8).mean(dim=(1, 2, 3))
    return planes, means


def means_entry(name):
    """Where the kernels keep a mean in the [B, 8] table: 2 l and 2 l + 1 for pyramid level l, 6 for the chroma magnitude."""
    if name == "chroma":
        return 6
    return 2 * int(name.rsplit("_", 1)[1]) + (1 if "high" in name else 0)


def check_guidance(guide, means, planes, wmeans, levels, what):
    worst = 0.0
    assert guide.shape[1] == 2 * levels + 2 and tuple(means.shape) == (guide.shape[0], 8)
    for i, name in enumerate(plane_names(levels)):
        e = err_of(guide[:, i:i + 1], planes[name])
        worst = max(worst, e)
        assert e <= TOL, f"{what}: plane {name}: {e:.3e}"
    for name, want in wmeans.items():
        e = err_of(means[:, means_entry(name)], want)
        worst = max(worst, e)
        assert e <= TOL, f"{what}: mean of {name}: {e:.3e}"
    return worst


# ---- the residual steps
MOD_SHAPES = ((2, 16, 6, 8),        # float4 form, half a channel group
              (1, 48, 5, 7),        # scalar form, C no multiple of 32
              (1, 33, 4, 12),       # a one-channel last group
              (2, 64, 36, 32),      # 1152 pixels: a second float4 workgroup, mostly idle
              (1, 16, 19, 15))      # 285 pixels: a second scalar workgroup
STEP_HW = ((8, 8),                  # 64 pixels: one trip per wave
           (16, 12),                # 192 pixels: a wave's 16 pixels straddle two rows
           (36, 32),                # 1152 pixels: a second workgroup owning 128 pixels
           (2, 1056))               # three workgroups inside one row pair
STEP_B, STEP_LEVELS = 2, 2          # the level step tested is pyramid level 1: planes 2, 3 and means 2, 3; the chroma step planes 4, 5
SATURATION_SCALE, GATE_SCALE = 1000.0, 100.0
JUNK = 1.0e3                        # in every means entry the step under test must not read


def block_spec(c, levels):
    s = {"chroma_attn.0.weight": (c, 2, 3, 3), "chroma_gate.weight": (1, 1, 1, 1), "chroma_gate.bias": (1,),
         "res_proj.0.weight": (c, c, 1, 1), "res_proj.0.bias": (c,), "res_proj.2.weight": (c, c, 1, 1), "res_proj.2.bias": (c,)}
    for l in range(levels):
        s.update({f"low_attn.{l}.0.weight": (c, 1, 3, 3), f"high_attn.{l}.0.weight": (c, 1, 3, 3),
                  f"freq_gate_head.{l}.weight": (2, 2, 1, 1), f"freq_gate_head.{l}.bias": (2,)})
    return s


def means_table(guide, step, levels):
    """The [B, 8] table for one step from the float64 means of its two planes (what ml_means leaves), JUNK everywhere else."""
    t = torch.full((guide.shape[0], 8), JUNK, dtype=torch.float64)
    a, b = guide[:, 2 * step].double(), guide[:, 2 * step + 1].double()
    if step == levels:
        t[:, 6] = torch.sqrt(a * a + b * b + 1e-8).mean(dim=(1, 2))
    else:
        t[:, 2 * step], t[:, 2 * step + 1] = a.mean(dim=(1, 2)), b.mean(dim=(1, 2))
    return t.float()


def step_inputs(shape, levels, saturated=False):
    b, c, h, w = shape
    x = cases.rnd(f"mlk.x.{shape}", shape, -2.0, 2.0, seed=197)
    guide = cases.rnd(f"mlk.guide.{shape}.{levels}", (b, 2 * levels + 2, h, w), -1.0, 1.0, seed=197)
    p = cases.params(block_spec(c, levels), seed=5100 + c)
    if saturated:
        guide = guide * SATURATION_SCALE
        for k in p:
            if "gate" in k:
                p[k] = p[k] * GATE_SCALE
        p["chroma_gate.weight"] = p["chroma_gate.weight"].abs()      # the magnitude's mean is positive: an open gate, not x * 0
    return x, guide, p


def gate_want(guide, p, step, levels):
    g = guide.double()
    return M.step_gate(g[:, 2 * step:2 * step + 1], g[:, 2 * step + 1:2 * step + 2], f64(p), "", step, levels)


def gate_arguments(guide, p, step, levels):
    """float64 arguments of every sigmoid / tanh of one step: (gate head, convolution sums)."""
    g, p = guide.double(), f64(p)
    a, b = g[:, 2 * step:2 * step + 1], g[:, 2 * step + 1:2 * step + 2]
    if step == levels:
        mag = torch.sqrt(a * a + b * b + 1e-8).mean(dim=(2, 3), keepdim=True)
        return (F.conv2d(mag, p["chroma_gate.weight"], p["chroma_gate.bias"]).flatten(),
                F.conv2d(torch.cat([a, b], dim=1), p["chroma_attn.0.weight"], padding=1).flatten())
    pooled = torch.cat([a.mean(dim=(2, 3), keepdim=True), b.mean(dim=(2, 3), keepdim=True)], dim=1)
    return (F.conv2d(pooled, p[f"freq_gate_head.{step}.weight"], p[f"freq_gate_head.{step}.bias"]).flatten(),
            torch.cat([F.conv2d(a, p[f"low_attn.{step}.0.weight"], padding=1).flatten(),
                       F.conv2d(b, p[f"high_attn.{step}.0.weight"], padding=1).flatten()]))


def block_sums(want, blk=1024):
    b, c, h, w = want.shape
    nblk = -(-h * w // blk)
    return F.pad(want.reshape(b, c, h * w), (0, nblk * blk - h * w)).reshape(b, c, nblk, blk).sum(dim=3).permute(0, 2, 1)


# With r in +-1e-4 the increment 0.2 tanh(r) is at most 2e-5 = TOL, so TOL on the sum would pass a kernel that ignores r.  The increment
# out - x is therefore held to INC_TOL = 1e-6, from the float32 formats alone: the final sum (|out| < 4) rounds by at most 2^-23 =
# 1.2e-7; tanh as 1 - 2 rcp(1 + exp(2 r)) is five float32 operations on values of at most 2 (exp, add, rcp, multiply, subtract), each
# within 2^-23 absolutely, so 6e-7 in all, 1.2e-7 after the factor 0.2; 2.4e-7 in all, and 4 x that is INC_TOL.
INC_TOL = 1e-6
RESIDUAL_COUNTS = (35, 1024 * 3 + 4, 4 * 257)      # scalar by count | four float4 workgroups, the last with one live lane | two, one lane


# ---- tail
TAIL_FRAMES = {"16x24": (16, 24), "512x520": (512, 520), "1024x1032": (1024, 1032)}      # packed H, W
TAIL_STEP_ROWS = 16      # image rows at the bottom lifted by TAIL_STEP: they hold every pixel past the first trip of both caps
TAIL_STEP = 1.0


def tail_inputs(tag):
    """Image uniform in [-1, 2] plus an offset per channel, its last 16 rows lifted by 1; a mosaic in [0, 0.5] whose last 16 rows
    (8 packed rows) are lifted by 0.5 and whose G2 sites are halved, so that G1 alone is not the green mean."""
    H, W = TAIL_FRAMES[tag]
    img = torch.from_numpy(synth.uniform(198, f"mlk.tail.img.{tag}", (1, 3, 2 * H, 2 * W), -1.0, 2.0))
    img += torch.tensor([0.3, -0.2, 0.5]).view(1, 3, 1, 1)
    img[:, :, -TAIL_STEP_ROWS:] += TAIL_STEP
    x = torch.from_numpy(synth.uniform(199, f"mlk.tail.x.{tag}", (1, 1, 2 * H, 2 * W), 0.0, 0.5))
    x[:, :, -TAIL_STEP_ROWS:] += 0.5
    x[:, :, 1::2, 0::2] *= 0.5
    return img, x


def tail_want(img, x4, **kw):
    return M.corrections(img.double(), x4.double(), R.bayer_luma_chroma(x4.double())[0], **kw)


# ---- model: tag -> (dim, depth, mosaic batch, height, width, seed, launches of ml_step_fused / ml_modulate / tc_residual / ml_residual)
MODEL_CASES = {
    # 4 guidance planes, the LL2 anchor still present.  Fused at level 0 only (16 x 24 = 384 pixels; 8 x 12 = 96 is no multiple of 64)
    "d16_l1_b1_32x48": (16, 1, 1, 32, 48, 191, (2 * 2, 5 * 2, 5, 5 * 1)),
    # the default width: fused C = 48 at level 0 (stages 1, 7), composed C = 96 / 192 / 384
    "d48_l2_b2_64x96": (48, 2, 2, 64, 96, 192, (2 * 3, 5 * 3, 5, 5 * 2)),
    # composed C = 24 at level 0 (a channel group shorter than 32), fused C = 48 at level 1 (stages 2, 6)
    "d24_l2_b1_64x64": (24, 2, 1, 64, 64, 193, (2 * 3, 5 * 3, 5, 5 * 2)),
}
LAUNCH_NAMES = ("ml_step_fused_kernel", "ml_modulate_kernel", "tc_residual_kernel", "ml_residual_kernel")


def fused_supported(c, h, w):
    """ml_step_fused_supported (csrc/rf_multilvl.hip) restated."""
    return c % 16 == 0 and c <= 64 and w % 4 == 0 and (h * w) % 64 == 0


# ------------------------------------------------------------------------------------------------ no GPU
def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake, off2 = C.c_void_p(1 << 12), C.c_void_p((1 << 12) + 2)
    err = lib.rf_last_error
    mod = lambda **kw: lib.rf_ml_modulate(*[kw.get(k, fake) for k in ("x", "guide", "means")], kw.get("step", 0), kw.get("levels", 2),      # noqa: E731
                                          *[kw.get(k, fake) for k in ("w_a", "w_b", "gate_w", "gate_b", "out")], kw.get("B", 1), kw.get("C", 16),
                                          kw.get("h", 4), kw.get("w", 4), None)
    assert mod(guide=None) == -22 and b"null" in err()
    assert mod(w_b=None) == -22 and b"null" in err()                      # the level form needs high_attn
    assert mod(out=off2) == -22 and b"aligned" in err()
    assert mod(B=65536) == -22 and b"65535" in err()
    assert mod(B=0) == -22 and b"positive" in err()
    assert mod(C=513) == -22 and b"512" in err()
    assert mod(step=3) == -22 and b"step=3" in err()
    assert mod(step=-1) == -22 and b"step=-1" in err()
    assert mod(levels=4, step=4) == -22 and b"levels=4" in err()
    assert mod(levels=0) == -22 and b"levels=0" in err()
    step = lambda **kw: lib.rf_ml_step_fused(*[kw.get(k, fake) for k in ("x", "guide", "means")], kw.get("step", 0), kw.get("levels", 2),      # noqa: E731
                                             *[kw.get(k, fake) for k in ("w_a", "w_b", "gate_w", "gate_b", "w0", "b0", "w2", "b2", "out")],
                                             kw.get("partial", None), kw.get("B", 1), kw.get("C", 16), kw.get("h", 8), kw.get("w", 8), None)
    assert step(b2=None) == -22 and b"null" in err()
    assert step(partial=off2) == -22 and b"aligned" in err()
    assert step(B=65536) == -22 and b"65535" in err()
    assert step(step=3) == -22 and b"step=3" in err()
    for kw in (dict(C=24), dict(C=80), dict(w=6, h=32), dict(h=3, w=4)):
        assert step(**kw) == -22 and b"the fused step needs" in err(), kw
    assert lib.rf_ml_residual(fake, None, fake, 1, 1, 1, 8, None) == -22 and b"null" in err()
    assert lib.rf_ml_residual(fake, fake, off2, 1, 1, 1, 8, None) == -22 and b"aligned" in err()
    assert lib.rf_ml_residual(fake, fake, fake, 1, 1, 0, 8, None) == -22 and b"positive" in err()
    assert lib.rf_ml_residual(fake, fake, fake, 65535, 512, 4096, 4096, None) == -22 and b"2^38" in err()

    def handle(variant):
        cfg = _lib.RfConfig(DIM, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, 2, variant, 1, 0, 2)
        h = C.c_void_p()
        assert lib.rf_create(C.byref(cfg), C.byref(h)) == 0
        return h
    ml, flca = handle(_lib.RF_VARIANT_MULTILVL), handle(_lib.RF_VARIANT_FLCA)
    try:
        args = (fake, fake, fake, 1 << 30, 1, 16, 24, None)       # guide, means, workspace, bytes, B, H, W, stream
        assert lib.rf_ml_guidance(ml, None, 0, *args) == -22 and b"null" in err()
        assert lib.rf_ml_guidance(flca, fake, 0, *args) == -22 and b"multi-level" in err()
        assert lib.rf_ml_guidance(ml, fake, 4, *args) == -22 and b"level" in err()
        assert lib.rf_ml_guidance(ml, fake, 0, fake, fake, fake, 1 << 30, 1, 12, 24, None) == -22 and b"multiples of 8" in err()
        assert lib.rf_ml_guidance(ml, fake, 0, *args) == -2 and b"not packed" in err()
        targs = (fake, 1 << 30, 1, 16, 24, None)                  # workspace, bytes, B, H, W, stream
        assert lib.rf_ml_tail(ml, None, fake, 0, *targs) == -22 and b"null" in err()
        assert lib.rf_ml_tail(flca, fake, fake, 0, *targs) == -22 and b"multi-level" in err()
        assert lib.rf_ml_tail(ml, fake, fake, 0, fake, 1 << 30, 65536, 16, 24, None) == -22
        assert lib.rf_ml_tail(ml, fake, fake, 0, *targs) == -2 and b"not packed" in err()
    finally:
        lib.rf_destroy(ml)
        lib.rf_destroy(flca)


def test_cases_reach_the_branches_they_are_named_for():
    """The launch arithmetic of csrc/rf_multilvl.hip restated, from the shapes alone."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    # ml_guide_level_kernel: min(cdiv(pf, 256), 256) workgroups of 256 pixels; ml_means_kernel: 64 lanes over the partials
    b, h, w = BIG_GUIDE
    pf = h * w
    assert cdiv(pf, 256) > GUIDE_CAP and pf - GUIDE_CAP * 256 == 8 * w == 2048      # the last 8 rows = workgroups 0..7, second trip
    assert GUIDE_CAP // 64 == 4                                                      # ml_means: 4 trips per lane
    for tag, (b, h, w) in FRAMES.items():
        assert cdiv(h * w, 256) <= GUIDE_CAP and cdiv(h * w, 256) == 2               # two workgroups at level 0, the last partly live
    assert (FRAMES["b1_8x40"][1] >> 3, FRAMES["b1_8x40"][2] >> 3) == (1, 5)         # LL3 of 8 x 40 and its level 3: one row

    # ml_modulate_kernel: float4 form = cdiv(P, 1024) x cdiv(C, 32) workgroups of 256 lanes x 4 pixels; scalar = cdiv(P, 256)
    reach = {}
    for b, c, h, w in MOD_SHAPES:
        vec = w % 4 == 0
        wg = cdiv(h * w, 1024 if vec else 256)
        live_last = cdiv(h * w - (wg - 1) * (1024 if vec else 256), 4 if vec else 1)
        reach[b, c, h, w] = (vec, wg, live_last, cdiv(c, 32), c - 32 * (cdiv(c, 32) - 1))
    assert reach[2, 16, 6, 8] == (True, 1, 12, 1, 16)          # half a channel group: c_hi = C clips
    assert reach[1, 48, 5, 7] == (False, 1, 35, 2, 16)
    assert reach[1, 33, 4, 12] == (True, 1, 12, 2, 1)          # a one-channel last group
    assert reach[2, 64, 36, 32] == (True, 2, 32, 2, 32)        # the second float4 workgroup has 32 live lanes of 256
    assert reach[1, 16, 19, 15] == (False, 2, 29, 1, 16)       # the second scalar workgroup has 29

    # ml_residual_kernel: float4 form where n % 4 == 0 (and 16-byte alignment): cdiv(n / 4, 256) workgroups, else cdiv(n, 256)
    assert RESIDUAL_COUNTS[0] % 4 and [n % 4 for n in RESIDUAL_COUNTS[1:]] == [0, 0]
    assert [(cdiv(n // 4, 256), n // 4 % 256) for n in RESIDUAL_COUNTS[1:]] == [(4, 1), (2, 1)]
    assert cdiv(RESIDUAL_COUNTS[2], 256) == 5 and RESIDUAL_COUNTS[2] % 256 == 4      # the same count in the scalar form (offset view)

    # ml_step_fused_kernel: a workgroup owns 1024 consecutive pixels, a wave 16 of every 64
    got = []
    for h, w in STEP_HW:
        assert all(fused_supported(c, h, w) for c in (16, 32, 48, 64))
        p = h * w
        trips_last = cdiv(p - (cdiv(p, 1024) - 1) * 1024, 64)
        got.append((cdiv(p, 1024), trips_last, any((16 * g) // w != (16 * g + 15) // w for g in range(p // 16))))
    assert got == [(1, 1, True), (1, 3, True), (2, 2, False), (3, 1, False)]      # workgroups, trips per wave in the last, a group over two rows
    assert divmod(15, STEP_HW[1][1]) == (1, 3)                     # 16 x 12: the first group of 16 ends at x = 3 of row 1, away from any border of 4
    assert STEP_HW[3][0] == 2 and 1024 < STEP_HW[3][1] < 2048      # workgroup 1 starts and ends inside a row
    assert not any(fused_supported(c, h, w) for c, h, w in ((24, 8, 8), (80, 8, 8), (16, 32, 6), (16, 3, 4)))

    # ml_tail_sums_kernel: min(cdiv(P4 / 4, 256), 1024) workgroups over P4 / 4 float4s per channel and over H W packed pixels;
    # ml_tail_apply_kernel: min(cdiv(P4 / 4, 256), 4096) over P4 / 4
    trips = {}
    for tag, (H, W) in TAIL_FRAMES.items():
        q = 4 * H * W // 4
        trips[tag] = (cdiv(q, min(cdiv(q, 256), TAIL_SUMS_CAP) * 256), cdiv(H * W, min(cdiv(q, 256), TAIL_SUMS_CAP) * 256),
                      cdiv(q, min(cdiv(q, 256), TAIL_APPLY_CAP) * 256))
    assert trips == {"16x24": (1, 1, 1), "512x520": (2, 2, 1), "1024x1032": (5, 5, 2)}      # sums: float4s, packed pixels; apply
    assert TAIL_SUMS_CAP // 64 == 16 and cdiv(16 * 24, 256) == 2      # ml_tail_delta's 64 lanes: 16 trips over 1024 partials, one over 2
    for tag in ("512x520", "1024x1032"):      # the lifted rows hold every output pixel past the first trip of the cap the case is named for
        H, W = TAIL_FRAMES[tag]
        cap = TAIL_SUMS_CAP if tag == "512x520" else TAIL_APPLY_CAP
        assert 0 < 4 * H * W - cap * 256 * 4 <= TAIL_STEP_ROWS * 2 * W
    H, W = TAIL_FRAMES["512x520"]             # and the lifted mosaic rows every packed pixel past ml_tail_sums's
    assert 0 < H * W - TAIL_SUMS_CAP * 256 <= (TAIL_STEP_ROWS // 2) * W

    # model cases: which U-Net levels take the fused step
    for tag, (dim, depth, b, hm, wm, seed, counts) in MODEL_CASES.items():
        fused = [fused_supported(dim << l, hm // 2 >> l, wm // 2 >> l) for l in range(4)]
        stages_fused = sum(fused[:3]) * 2 + fused[3]
        assert stages_fused == 2 and counts == (stages_fused * (depth + 1), (7 - stages_fused) * (depth + 1), 7 - stages_fused,
                                                 (7 - stages_fused) * depth), tag
    assert [fused_supported(48 << l, 32 >> l, 48 >> l) for l in range(4)] == [True, False, False, False]
    assert [fused_supported(24 << l, 32 >> l, 32 >> l) for l in range(4)] == [False, True, False, False]
    assert RawFormer(variant="multilvl").dim == 48


def test_saturation_inputs_reach_beyond_100():
    """Guide x 1000 and gate heads x 100: every gate-head argument lies beyond +-100, the convolution sums reach far beyond on both
    sides (four in five of them beyond +-100; the rest check the unsaturated form under the same call)."""
    for shape in (MOD_SHAPES[0], (STEP_B, 48) + STEP_HW[1]):
        for step in (1, STEP_LEVELS):      # the steps of the saturated GPU tests
            x, guide, p = step_inputs(shape, STEP_LEVELS, saturated=True)
            head, sums = gate_arguments(guide, p, step, STEP_LEVELS)
            assert float(head.abs().min()) > 100.0, (shape, step, head)
            assert float(sums.min()) < -1000.0 and float(sums.max()) > 1000.0
            assert float((sums.abs() > 100.0).double().mean()) > 0.8
            gates = torch.sigmoid(head)      # at 0 or 1; a step whose gates are all shut would compare zeros
            print(f"{shape} step {step}: gates {[round(float(v), 3) for v in gates]}")
            assert float(gates.reshape(shape[0], -1).amax(dim=1).min()) > 0.999, "an image with every gate shut"


def test_big_guidance_frame_shows_a_dropped_trip():
    """float64: the sum over the first 65 536 pixels alone (a grid-stride loop that stops after one trip) misses every mean by more
    than 10 x the bound."""
    planes, means = guidance_ref(big_guide_frame(), 3, 0)
    first = GUIDE_CAP * 256
    pf = BIG_GUIDE[1] * BIG_GUIDE[2]
    for name, want in means.items():
        v = torch.sqrt(planes["cr"] ** 2 + planes["cb"] ** 2 + 1e-8) if name == "chroma" else planes[name]
        dropped = v.reshape(1, -1)[:, :first].sum(dim=1) / pf
        assert float((dropped - want).abs().max()) / max(1.0, float(want.abs().max())) > 10 * TOL, name


def test_large_tail_frames_show_a_dropped_trip():
    """float64: without the pixels past the first trip of ml_tail_sums (1024 workgroups x 256 float4s) out_mean and in_mean move the
    result by more than 10 x the bound; the pixels past ml_tail_apply's first trip are changed by more than that, so leaving them
    as they were shows too."""
    for tag in ("512x520", "1024x1032"):
        H, W = TAIL_FRAMES[tag]
        img, x = tail_inputs(tag)
        img, x4 = img.double(), R.pixel_unshuffle2(x).double()
        first = TAIL_SUMS_CAP * 256 * 4
        want = tail_want(img, x4)
        scale = max(1.0, float(want.abs().max()))      # err_of's
        flat = img.reshape(3, -1)
        moved = 0.12 * (flat.mean(dim=1) - flat[:, :first].sum(dim=1) / flat.shape[1]).abs() / scale
        assert float(moved.min()) > 10 * TOL, (tag, moved)
        rgb = torch.cat([x4[:, 0:1], 0.5 * (x4[:, 1:2] + x4[:, 2:3]), x4[:, 3:4]], dim=1).reshape(3, -1)
        moved_in = 0.12 * (rgb.mean(dim=1) - rgb[:, :TAIL_SUMS_CAP * 256].sum(dim=1) / rgb.shape[1]).abs() / scale
        assert float(moved_in.min()) > 10 * TOL, (tag, moved_in)
        if tag == "1024x1032":
            past = (want - img).reshape(3, -1)[:, TAIL_APPLY_CAP * 256 * 4:]
            assert past.shape[1] > 0 and float(past.abs().max()) / scale > 10 * TOL


# defects of the float64 restatement, per kernel family: name -> the error it causes on the cases above, relative as err_of
def guidance_defects():
    out = {}
    for tag in FRAMES:
        for levels, lvl in ((2, 1), (3, 3), (1, 2)):
            x4 = frame(tag)
            planes, means = guidance_ref(x4, levels, lvl)
            out.setdefault("low and high plane swapped", []).append(err_of(planes["y_high_0"], planes["y_low_0"]))
            out.setdefault("cr and cb swapped", []).append(err_of(planes["cb"], planes["cr"]))
            ac = guidance_ref(x4, levels, lvl, resize=lambda t, size: F.interpolate(t, size=size, mode="bilinear", align_corners=True))
            out.setdefault("align_corners=True sampling", []).append(max(err_of(ac[0][n], planes[n]) for n in planes))
            if min(x4.shape[2:]) >> levels >= 2:      # one more Haar level exists (not below the single row of 8 x 40 at depth 3)
                up = guidance_ref(x4, levels, lvl, shift=1)
                out.setdefault("pyramid level l+1 used for level l", []).append(max(err_of(up[0][n], planes[n]) for n in planes if n.startswith("y_")))
            if lvl >= 2:      # at levels 0 and 1 the bilinear resize keeps the mean of a y plane; the chroma magnitude's moves at 1, 2, 3
                full = guidance_ref(x4, levels, 0)[1]
                out.setdefault("means taken at the guidance size instead of the stage size", []).append(err_of(full["chroma"], means["chroma"]))
    return {k: min(v) for k, v in out.items()}      # per case what the plane and mean checks see at most, over the cases the least


def step_defects():
    out = {}
    for shape in (MOD_SHAPES[0], MOD_SHAPES[2], (STEP_B, 48) + STEP_HW[1]):
        x, guide, p = step_inputs(shape, STEP_LEVELS)
        g = guide.double()
        lvl = gate_want(guide, p, 1, STEP_LEVELS)
        chroma = gate_want(guide, p, STEP_LEVELS, STEP_LEVELS)
        xd = x.double()
        res = shape[1] == 48

        def moved(gate, ref):
            if res:      # through the whole residual step
                return err_of(M.res_step(xd, gate, f64(p), ""), M.res_step(xd, ref, f64(p), ""))
            return err_of(xd * gate, xd * ref)
        out.setdefault("low and high plane swapped", []).append(moved(M.step_gate(g[:, 3:4], g[:, 2:3], f64(p), "", 1, STEP_LEVELS), lvl))
        out.setdefault("pyramid level l+1 used for level l", []).append(moved(M.step_gate(g[:, 2:3], g[:, 3:4], f64(p), "", 0, STEP_LEVELS),
                                                                              gate_want(guide, p, 0, STEP_LEVELS)))
        q = dict(p)
        q["freq_gate_head.1.weight"], q["freq_gate_head.1.bias"] = p["freq_gate_head.1.weight"].flip(0), p["freq_gate_head.1.bias"].flip(0)
        out.setdefault("gate rows g0 / g1 swapped", []).append(moved(gate_want(guide, q, 1, STEP_LEVELS), lvl))
        q = dict(p)
        q["chroma_attn.0.weight"] = p["chroma_attn.0.weight"].flip(1)
        out.setdefault("chroma weight halves swapped", []).append(moved(gate_want(guide, q, STEP_LEVELS, STEP_LEVELS), chroma))
        out.setdefault("cr and cb swapped", []).append(moved(M.step_gate(g[:, 5:6], g[:, 4:5], f64(p), "", STEP_LEVELS, STEP_LEVELS), chroma))
    return {k: min(v) for k, v in out.items()}


def sums_defects():
    """One group of 16 pixels (a wave's step) left out of a block's sum, on every step_fused shape."""
    worst = []
    for h, w in STEP_HW:
        x, guide, p = step_inputs((STEP_B, 48, h, w), STEP_LEVELS)
        want = M.res_step(x.double(), gate_want(guide, p, STEP_LEVELS, STEP_LEVELS), f64(p), "")
        full = block_sums(want)
        flat = want.reshape(STEP_B, 48, -1)
        for g0 in (0, h * w - 16):      # the first group of the first block, the last of the last
            less = full.clone()
            less[:, g0 // 1024] -= flat[:, :, g0:g0 + 16].sum(dim=2)
            worst.append(max(err_of(less, full), err_of(less.sum(dim=1) / (h * w), full.sum(dim=1) / (h * w))))      # what the two checks see
    return {"one 16-pixel group missing from a block sum": min(worst)}


def tail_defects():
    img, x = tail_inputs("16x24")
    x4 = R.pixel_unshuffle2(x)
    want = tail_want(img, x4)
    g1 = x4.clone()
    g1[:, 2] = g1[:, 1]      # (G1 + G2) / 2 -> G1
    y = R.bayer_luma_chroma(x4.double())[0]
    ac = M.corrections(img.double(), x4.double(), y, resize=lambda t, size: F.interpolate(t, size=size, mode="bilinear", align_corners=True))
    return {"in_mean G taken as G1 alone": err_of(M.corrections(img.double(), g1.double(), y), want),
            "align_corners=True sampling": err_of(ac, want),
            "pyramid level l+1 used for level l": err_of(M.corrections(img.double(), x4.double(), y, anchor_level=3), want)}


DEFECT_FAMILIES = {"guidance": guidance_defects, "modulate / step_fused": step_defects, "step_fused sums": sums_defects, "tail": tail_defects}
DEFECTS = ("low and high plane swapped", "cr and cb swapped", "gate rows g0 / g1 swapped", "chroma weight halves swapped",
           "means taken at the guidance size instead of the stage size", "align_corners=True sampling",
           "one 16-pixel group missing from a block sum", "in_mean G taken as G1 alone", "pyramid level l+1 used for level l")


def test_bound_sees_every_defect():
    """Each plausible defect, applied to the float64 restatement, moves the result on the cases of this file by at least 4 x the
    operator bound (the smallest move over the cases of a family is what counts)."""
    seen = set()
    for family, fn in DEFECT_FAMILIES.items():
        for name, moved in fn().items():
            print(f"{family}: {name}: moves the result by {moved:.3e} = {moved / TOL:.0f} x the bound")
            assert moved >= 4 * TOL, (family, name, moved)
            seen.add(name)
    assert seen == set(DEFECTS)


# ------------------------------------------------------------------------------------------------ guidance
@pytest.mark.gpu
@pytest.mark.parametrize("levels", (1, 2, 3))
@pytest.mark.parametrize("tag", list(FRAMES))
def test_guidance(device, tag, levels):
    """Every plane by name and every used mean at every U-Net level.  Depth 1 has 4 planes; at depth 3 the LL3 of 8 x 40 is one row
    high (bilerp's y1 = y0 clamp), and so is its level 3."""
    x4 = frame(tag)
    m = model(device, levels=levels)
    worst = 0.0
    for lvl in range(4):
        guide, means = m.ml_guidance(x4.to(device), lvl)
        planes, wmeans = guidance_ref(x4, levels, lvl)
        assert tuple(guide.shape) == (x4.shape[0], 2 * levels + 2, x4.shape[2] >> lvl, x4.shape[3] >> lvl)
        worst = max(worst, check_guidance(guide, means, planes, wmeans, levels, f"{tag} depth {levels} level {lvl}"))
    print(f"guidance {tag} depth {levels}: worst {worst:.3e}")


@pytest.mark.gpu
def test_guidance_past_the_grid_cap(device):
    """264 x 256 at level 0: 264 workgroups' worth of pixels on a grid of 256, so workgroups 0..7 take a second trip over the bright
    last rows (test_big_guidance_frame_shows_a_dropped_trip), and ml_means sums 256 partials per plane in 4 trips."""
    x4 = big_guide_frame()
    guide, means = model(device, levels=3).ml_guidance(x4.to(device), 0)
    planes, wmeans = guidance_ref(x4, 3, 0)
    print(f"guidance 264x256: worst {check_guidance(guide, means, planes, wmeans, 3, '264x256'):.3e}")


@pytest.mark.gpu
def test_guidance_is_per_image(device):
    """Image 1 is image 0 scaled by 0.25: each luma is normalised by its own maximum, so the y planes agree and the chroma planes
    do not; strides between images are those of the planes."""
    x4 = frame("b2_16x24")
    x4[1] = 0.25 * x4[0]
    guide, means = model(device).ml_guidance(x4.to(device), 1)
    planes, wmeans = guidance_ref(x4, 2, 1)
    assert float((planes["y_low_0"][0] - planes["y_low_0"][1]).abs().max()) < 1e-12 < float((planes["cr"][0] - planes["cr"][1]).abs().max())
    print(f"guidance per image: worst {check_guidance(guide, means, planes, wmeans, 2, 'scaled copy'):.3e}")
    assert err_of(guide[1, :4], guide[0, :4].cpu()) <= TOL


# ------------------------------------------------------------------------------------------------ ml_modulate
@pytest.mark.gpu
@pytest.mark.parametrize("shape", MOD_SHAPES)
def test_modulate(device, shape):
    """Every step of every depth: level step l reads planes 2 l, 2 l + 1 and means 2 l, 2 l + 1, the chroma step planes 2 L, 2 L + 1,
    mean 6 and the two halves of chroma_attn.  Every other means entry holds JUNK."""
    from bayer_low_light_image_enhancement_amd import ops
    worst = 0.0
    for levels in (1, 2, 3):
        x, guide, p = step_inputs(shape, levels)
        xd, gd, pd = x.to(device), guide.to(device), on(device, p)
        for step in range(levels + 1):
            out = ops.ml_modulate(xd, gd, means_table(guide, step, levels).to(device), step, levels, pd)
            e = err_of(out, x.double() * gate_want(guide, p, step, levels))
            worst = max(worst, e)
            assert e <= TOL, f"depth {levels} step {step}: {e:.3e}"
    print(f"modulate {shape}: worst {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("step", (1, 2))
def test_modulate_saturated(device, step):
    """Arguments beyond +-100 (test_saturation_inputs_reach_beyond_100): __expf overflows on one side and the result rests on
    rcp(inf) = 0; finite, and at the float64 limits."""
    from bayer_low_light_image_enhancement_amd import ops
    x, guide, p = step_inputs(MOD_SHAPES[0], STEP_LEVELS, saturated=True)
    out = ops.ml_modulate(x.to(device), guide.to(device), means_table(guide, step, STEP_LEVELS).to(device), step, STEP_LEVELS, on(device, p))
    assert bool(torch.isfinite(out).all())
    e = err_of(out, x.double() * gate_want(guide, p, step, STEP_LEVELS))
    print(f"modulate saturated step {step}: {e:.3e}")
    assert e <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in MOD_SHAPES if s[1] % 32])
def test_modulate_stays_inside_its_channels(device, shape):
    """A workgroup owns up to 32 channels; the last group ends at C.  x, the weights and the output sit at the head of longer
    buffers (32 more channels' worth) filled with a sentinel: the output's tail must be untouched and the bits those of the plain
    call, for the level and the chroma form."""
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w = shape
    x, guide, p = step_inputs(shape, STEP_LEVELS)
    sentinel = 12345.0

    def headed(t, per_channel):
        buf = torch.full((t.numel() + 32 * per_channel,), sentinel, dtype=torch.float32, device=device)
        buf[: t.numel()] = t.reshape(-1).to(device)
        return buf, buf[: t.numel()].view(t.shape)
    pd = {k: headed(v, v[0].numel())[1] for k, v in p.items()}
    for step in (1, 2):
        mt = means_table(guide, step, STEP_LEVELS).to(device)
        obuf, out = headed(torch.zeros(shape), h * w)
        ops.ml_modulate(headed(x, h * w)[1], guide.to(device), mt, step, STEP_LEVELS, pd, out=out)
        assert bool((obuf[out.numel():] == sentinel).all()), "written past the last channel"
        assert torch.equal(out, ops.ml_modulate(x.to(device), guide.to(device), mt, step, STEP_LEVELS, on(device, p)))


@pytest.mark.gpu
def test_modulate_scalar_form_by_alignment(device):
    """w % 4 == 0 but x and out start 4 bytes past a 16-byte boundary: launch_ml_modulate's alignment test sends the call to the
    scalar form.  Same values as the float4 call within the bound, and nothing written outside the view."""
    from bayer_low_light_image_enhancement_amd import ops
    shape = MOD_SHAPES[3]
    x, guide, p = step_inputs(shape, STEP_LEVELS)
    n = x.numel()
    xbuf = torch.zeros(n + 1, device=device)
    obuf = torch.full((n + 2,), 777.0, device=device)
    xv, ov = xbuf[1:].view(shape), obuf[1:n + 1].view(shape)
    xv.copy_(x)
    assert xv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4 and xv.is_contiguous()
    mt = means_table(guide, 1, STEP_LEVELS).to(device)
    ops.ml_modulate(xv, guide.to(device), mt, 1, STEP_LEVELS, on(device, p), out=ov)
    e = err_of(ov, x.double() * gate_want(guide, p, 1, STEP_LEVELS))
    print(f"modulate, offset view: {e:.3e}")
    assert e <= TOL and float(obuf[0]) == 777.0 and float(obuf[-1]) == 777.0


# ------------------------------------------------------------------------------------------------ ml_residual
@pytest.mark.gpu
@pytest.mark.parametrize("scale", (50.0, 1e-4))
@pytest.mark.parametrize("n", RESIDUAL_COUNTS)
def test_residual(device, n, scale):
    """x + 0.2 tanh(r) with r in +-50 (tanh saturated) and +-1e-4 (its linear end); the float4 form where n % 4 == 0, else the scalar
    one; in place and twice give the same bits."""
    from bayer_low_light_image_enhancement_amd import ops
    x = cases.rnd(f"mlk.res.x.{n}", (n,), -2.0, 2.0, seed=200)
    r = cases.rnd(f"mlk.res.r.{n}", (n,), -scale, scale, seed=200)
    want = x.double() + 0.2 * torch.tanh(r.double())
    out = ops.ml_residual(x.to(device), r.to(device))
    e = err_of(out, want)
    inc = float(((out.cpu().double() - x.double()) - 0.2 * torch.tanh(r.double())).abs().max())
    print(f"residual n={n} r in +-{scale}: {e:.3e}, increment {inc:.3e}")
    assert e <= TOL
    assert inc <= INC_TOL
    assert torch.equal(out, ops.ml_residual(x.to(device), r.to(device))), "two calls differ"
    inplace = x.to(device)
    over = ops.ml_residual(inplace, r.to(device), out=inplace)
    assert over.data_ptr() == inplace.data_ptr() and torch.equal(over, out), "in place differs"


@pytest.mark.gpu
def test_residual_scalar_form_by_alignment(device):
    """4 x 257 elements 4 bytes past a 16-byte boundary: the scalar form, five workgroups, nothing written outside the view."""
    from bayer_low_light_image_enhancement_amd import ops
    n = RESIDUAL_COUNTS[2]
    x = cases.rnd(f"mlk.res.x.{n}", (n,), -2.0, 2.0, seed=200)
    r = cases.rnd(f"mlk.res.r.{n}", (n,), -50.0, 50.0, seed=200)
    xbuf, rbuf, obuf = torch.zeros(n + 1, device=device), torch.zeros(n + 1, device=device), torch.full((n + 2,), 777.0, device=device)
    xbuf[1:], rbuf[1:] = x.to(device), r.to(device)
    assert xbuf[1:].data_ptr() % 16 == 4
    out = ops.ml_residual(xbuf[1:], rbuf[1:], out=obuf[1:n + 1])
    e = err_of(out, x.double() + 0.2 * torch.tanh(r.double()))
    print(f"residual, offset view: {e:.3e}")
    assert e <= TOL and float(obuf[0]) == 777.0 and float(obuf[-1]) == 777.0
    assert torch.equal(out, ops.ml_residual(x.to(device), r.to(device)))      # the same float operations per element in both forms


# ------------------------------------------------------------------------------------------------ ml_step_fused
@pytest.mark.gpu
@pytest.mark.parametrize("hw", STEP_HW)
@pytest.mark.parametrize("c", (16, 32, 48, 64))
def test_step_fused(device, c, hw):
    """One whole residual step for the level form (pyramid level 1) and the chroma form, with and without the pooling sums: out
    against res_step, the sums block by block (1024 consecutive pixels) and as channel means; in place and twice the same bits."""
    from bayer_low_light_image_enhancement_amd import ops
    shape = (STEP_B, c) + hw
    x, guide, p = step_inputs(shape, STEP_LEVELS)
    xd, gd, pd = x.to(device), guide.to(device), on(device, p)
    P = hw[0] * hw[1]
    for step in (1, STEP_LEVELS):
        mt = means_table(guide, step, STEP_LEVELS).to(device)
        want = M.res_step(x.double(), gate_want(guide, p, step, STEP_LEVELS), f64(p), "")
        plain = ops.ml_step_fused(xd, gd, mt, step, STEP_LEVELS, pd)
        out, partial = ops.ml_step_fused(xd, gd, mt, step, STEP_LEVELS, pd, sums=True)
        assert tuple(partial.shape) == (STEP_B, ops.tc_nblk(*hw), c) and ops.tc_nblk(*hw) == -(-P // 1024)
        e = (err_of(out, want), err_of(partial, block_sums(want)), err_of(partial.sum(dim=1) / P, want.mean(dim=(2, 3))))
        print(f"step_fused C={c} {hw} step {step}: out {e[0]:.3e}, block sums {e[1]:.3e}, channel means {e[2]:.3e}")
        assert e[0] <= TOL, "out"
        assert e[1] <= TOL, "block sums"
        assert e[2] <= TOL, "channel means"
        assert torch.equal(plain, out), "the sums changed the result"
        again, partial_again = ops.ml_step_fused(xd, gd, mt, step, STEP_LEVELS, pd, sums=True)
        assert torch.equal(out, again) and torch.equal(partial, partial_again), "two calls differ"
        inplace = x.to(device)
        over, partial_over = ops.ml_step_fused(inplace, gd, mt, step, STEP_LEVELS, pd, out=inplace, sums=True)
        assert over.data_ptr() == inplace.data_ptr() and torch.equal(over, out) and torch.equal(partial_over, partial), "in place differs"


@pytest.mark.gpu
@pytest.mark.parametrize("step", (1, 2))
def test_step_fused_saturated(device, step):
    from bayer_low_light_image_enhancement_amd import ops
    shape = (STEP_B, 48) + STEP_HW[1]
    x, guide, p = step_inputs(shape, STEP_LEVELS, saturated=True)
    out = ops.ml_step_fused(x.to(device), guide.to(device), means_table(guide, step, STEP_LEVELS).to(device), step, STEP_LEVELS, on(device, p))
    assert bool(torch.isfinite(out).all())
    e = err_of(out, M.res_step(x.double(), gate_want(guide, p, step, STEP_LEVELS), f64(p), ""))
    print(f"step_fused saturated step {step}: {e:.3e}")
    assert e <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((1, 24, 8, 8), (1, 80, 8, 8), (1, 16, 32, 6), (1, 16, 3, 4)))
def test_step_fused_refuses_what_it_cannot_run(device, shape):
    """C = 24 or 80, w % 4 != 0, h * w % 64 != 0: a RuntimeError with the library's message, and no kernel runs."""
    from bayer_low_light_image_enhancement_amd import ops
    x, guide, p = step_inputs(shape, STEP_LEVELS)
    xd, gd, pd, mt = x.to(device), guide.to(device), on(device, p), means_table(guide, 1, STEP_LEVELS).to(device)

    def attempt():
        with pytest.raises(RuntimeError, match="the fused step needs C = 16, 32, 48 or 64"):
            ops.ml_step_fused(xd, gd, mt, 1, STEP_LEVELS, pd, sums=True)
    _, n = cases.launches(attempt)
    assert not n, n


@pytest.mark.gpu
def test_step_fused_against_composed_on_the_same_inputs(device):
    """ops.ml_modulate -> float64 1x1 / ReLU / 1x1 on the host -> ops.ml_residual, and ops.ml_step_fused: both within the bound of
    the float64 step."""
    from bayer_low_light_image_enhancement_amd import ops
    shape = (STEP_B, 32) + STEP_HW[1]
    x, guide, p = step_inputs(shape, STEP_LEVELS)
    xd, gd, pd, p64 = x.to(device), guide.to(device), on(device, p), f64(p)
    for step in (0, STEP_LEVELS):
        mt = means_table(guide, step, STEP_LEVELS).to(device)
        want = M.res_step(x.double(), gate_want(guide, p, step, STEP_LEVELS), p64, "")
        mod = ops.ml_modulate(xd, gd, mt, step, STEP_LEVELS, pd).cpu().double()
        t = torch.relu(F.conv2d(mod, p64["res_proj.0.weight"], p64["res_proj.0.bias"]))
        r = F.conv2d(t, p64["res_proj.2.weight"], p64["res_proj.2.bias"]).float()
        composed = ops.ml_residual(xd, r.to(device))
        fused = ops.ml_step_fused(xd, gd, mt, step, STEP_LEVELS, pd)
        e = (err_of(composed, want), err_of(fused, want), err_of(fused, composed.cpu()))
        print(f"step {step}: composed {e[0]:.3e}, fused {e[1]:.3e}, fused against composed {e[2]:.3e}")
        assert max(e[:2]) <= TOL


# ------------------------------------------------------------------------------------------------ tail
def run_tail(device, tag, packed_too=False, levels=2, fresh=False):
    img, x = tail_inputs(tag)
    x4 = R.pixel_unshuffle2(x).contiguous()
    m = model(device, levels=levels, fresh=fresh)
    keep = img.to(device)
    out = m.ml_tail(keep, x.to(device))
    assert out.data_ptr() != keep.data_ptr() and torch.equal(keep.cpu(), img), "the caller's image was written"
    if packed_too:
        assert torch.equal(out, m.ml_tail(keep, x4.to(device))), "mosaic and packed input differ"
    got = out.cpu()
    del out, keep
    e = err_of(got, tail_want(img, x4))
    print(f"tail {tag} depth {levels}: {e:.3e}")
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("levels", (1, 2, 3))
def test_tail_small(device, levels):
    """Packed 16 x 24, on an image that is no constant; the mosaic and the packed input give the same bits.  The anchor is LL2 at
    every depth: at depth 1 the pyramid is built one level past what the guidance uses."""
    assert run_tail(device, "16x24", packed_too=True, levels=levels) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("512x520", "1024x1032"))
def test_tail_past_the_grid_caps(device, tag):
    """512 x 520: 266 240 float4s per channel on ml_tail_sums's 1024 workgroups (a second trip, also over the packed pixels).
    1024 x 1032: 1 056 768 on ml_tail_apply's 4096 (a second trip; five in ml_tail_sums).  The image's last rows sit at another
    level, so a trip left out shows (test_large_tail_frames_show_a_dropped_trip).  The workspace of the larger frame is about 1 GB:
    the model is the test's own and takes it along when it goes."""
    try:
        assert run_tail(device, tag, fresh=True) <= TOL
    finally:
        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ model and stage
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_forward(device, tag):
    dim, depth, b, hm, wm, seed, counts = MODEL_CASES[tag]
    x = torch.from_numpy(synth.bayer_mosaic(seed, b, hm, wm))
    with torch.no_grad():
        ref = M.forward(f64(state(dim, depth)), x.double(), dim, levels=depth)
        out, n = cases.launches(lambda: model(device, dim, depth)(x.to(device)))
    e = float((out.cpu().double() - ref).abs().max())
    print(f"{tag}: max-abs error {e:.3e} (max|ref| {float(ref.abs().max()):.3f}); launches {[n.get(k) for k in LAUNCH_NAMES]}")
    assert tuple(n.get(k, 0) for k in LAUNCH_NAMES) == counts
    assert e <= STAGE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("stage", (1, 2))
def test_forward_stage_dim24(device, stage):
    """dim 24 on a 32 x 32 packed frame: stage 1 composes its steps at C = 24 (a channel group of 24), stage 2 runs the fused step
    at C = 48 (16 x 16)."""
    dim, lvl = 24, stage - 1
    sd = f64(state(dim))
    x4 = R.pixel_unshuffle2(torch.from_numpy(synth.bayer_mosaic(194, 2, 64, 64)))
    xin = torch.from_numpy(synth.uniform(200 + stage, "mlk.stage.x", (2, dim << lvl, 32 >> lvl, 32 >> lvl), -1.0, 1.0))
    with torch.no_grad():
        ref = M.stage(xin.double(), R.bayer_luma_chroma(x4.double()), sd, f"conv_tran{stage}.", 8)
        out, n = cases.launches(lambda: model(device, dim).forward_stage(stage, xin.to(device), x4.to(device)))
    e = float((out.cpu().double() - ref).abs().max())
    print(f"dim 24 stage {stage}: max-abs error {e:.3e}; launches {[n.get(k) for k in LAUNCH_NAMES]}")
    assert tuple(n.get(k, 0) for k in LAUNCH_NAMES) == ((0, 3, 1, 2) if stage == 1 else (3, 0, 0, 0))
    assert e <= STAGE_TOL
