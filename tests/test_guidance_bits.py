"""The bits of the forward guidance and gate kernels of csrc/rf_flca.hip, csrc/rf_truecolor.hip and csrc/rf_multilvl.hip, and the
workspace sizes of the two variants, against tests/golden/guidance_parent.json: recorded on an MI355X with
tools/record_guidance_golden.py at the commit before these kernels were put on the shared device pieces of csrc/rf_guidance.h.
That change keeps every sum and every fmaf chain in its order: no bit may move, and there is no tolerance.  ``record`` is that of
tests/test_train_bits.py; the inputs come from ``cases.rnd`` / ``cases.params`` and the builders of tests/test_truecolor_kernels.py
and tests/test_multilvl_kernels.py.  The smallest shapes that reach each form:

=====================  ==============================================================================================================
guidance               ops.flca_guidance + ops.bayer_luma_chroma, packed (2, 4, 16, 24) to 16 x 24, 8 x 12, 2 x 3: guide_luma /
                       guide_haar / guide_level, two images (per-image maximum), down- and same-size resize
flca_c24_6x7           ops.flca on a packed 16 x 24 frame: the scalar flca_spatial_kernel (odd width), C no multiple of 32
flca_c40_6x10          ... and the PX = 2 vector form (PX = 4: the two ops.flca cases of tests/test_flca_pyramid_bits.py)
tc_guidance.<f>.l<L>   RawFormer(variant='truecolor').tc_guidance, frames of test_truecolor_kernels.FRAMES, pyramid depth L, U-Net
                       levels 0 and 3: tc_front, tc_normalise, tc_pyramid, tc_guide_level; widths 40, 20, 10, 5
tc_forward_mosaic      the mosaic form of the front end, through ``forward`` on a 32 x 48 mosaic
tc_pyramid             ops.tc_pyramid on 5 x 7 (reflect at both odd sides) and 6 x 8 planes
tc_gate.<shape>        ops.tc_spatial and ops.tc_residual at SPATIAL_SHAPES: PX = 4 and 1, half a channel group, more than one group
tc_color_head          ops.tc_color_head, P = 300
ml_guidance.l<L>       RawFormer(variant='multilvl').ml_guidance, packed (2, 4, 16, 24), U-Net levels 0 and 2: guidance_base, the
                       pyramid, ml_guide_level, ml_means
ml_modulate.<shape>    ops.ml_modulate, depth 2, steps 0, 1 (level form) and 2 (chroma form): PX = 4 / 1, channel-group tail, three groups
ml_step.c<C>.<hw>      ops.ml_step_fused, level step 1 and the chroma step, with and without ``partial``: every instantiation; at
                       16 x 68 a workgroup's second 1024-pixel block
ml_residual            ops.ml_residual, n = 1024 (float4 form) and 1023 (scalar form)
ml_tail                RawFormer.ml_tail on a 32 x 48 mosaic and on its packed form: both branches of packed_at in ml_tail_sums
=====================  ==============================================================================================================

Sizes: ``rf_workspace_bytes`` of a dim-16 ``truecolor`` and ``multilvl`` handle, depths 1, 2, 3, at (B, H, W) = (1, 16, 24) and
(2, 64, 64), compared without a device (the library loads without one).
"""
import ctypes as C
import json
import os

import pytest
import torch

import cases
import test_multilvl_kernels as ML
import test_truecolor_kernels as TC
from test_train_bits import record

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guidance_parent.json")
SEED = 6400
MOD_SHAPES = ((1, 16, 8, 8), (2, 40, 6, 7), (1, 72, 4, 12))
STEP_HW = ((8, 8), (16, 68))
WS_FRAMES = ((1, 16, 24), (2, 64, 64))


def tag_of(shape):
    return "x".join(str(v) for v in shape)


def host(**arrays):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in arrays.items()}


def packed_frame():
    return cases.rnd("gbits.packed", (2, 4, 16, 24), 0.0, 1.0, seed=SEED)


def run_guidance(device):
    from bayer_low_light_image_enhancement_amd import ops
    x4 = packed_frame().to(device)
    y, cr, cb = ops.bayer_luma_chroma(x4)
    return host(y=y, cr=cr, cb=cb, **{f"guide_{h}x{w}": ops.flca_guidance(x4, (h, w)) for h, w in ((16, 24), (8, 12), (2, 3))})


def run_flca(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    c = shape[1]
    p = {k: v.to(device) for k, v in cases.params(cases.flca_spec(c), seed=SEED + c).items()}
    feat = cases.rnd(f"gbits.flca.feat.{shape}", shape, seed=SEED)
    return host(out=ops.flca(feat.to(device), packed_frame()[:1].contiguous().to(device), p))


def run_tc_guidance(device, frame, levels):
    m, x4 = TC.model(device, levels), TC.frame(frame).to(device)
    y, crcb, rgb, g0 = m.tc_guidance(x4, 0)
    return host(y=y, crcb=crcb, rgb=rgb, guide0=g0, guide3=m.tc_guidance(x4, 3)[3])


def run_tc_forward_mosaic(device):
    from bayer_low_light_image_enhancement_amd import synth
    x = torch.from_numpy(synth.bayer_mosaic(SEED, 1, 32, 48))
    with torch.no_grad():
        return host(out=TC.model(device)(x.to(device)))


def run_tc_pyramid(device):
    from bayer_low_light_image_enhancement_amd import ops
    out = {}
    for h, w in ((5, 7), (6, 8)):
        ll, mag = ops.tc_pyramid(cases.rnd(f"gbits.pyr.{h}x{w}", (2, 1, h, w), seed=SEED).to(device))
        out.update({f"ll_{h}x{w}": ll, f"mag_{h}x{w}": mag})
    return host(**out)


def run_tc_gate(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    feat, guide, p = TC.spatial_inputs(shape)
    xs = ops.tc_spatial(feat.to(device), guide.to(device), {k: v.to(device) for k, v in p.items()})
    r = cases.rnd(f"gbits.tc.r.{shape}", shape, -3.0, 3.0, seed=SEED)
    x2, partial = ops.tc_residual(xs, r.to(device))
    return host(xs=xs, x2=x2, partial=partial)


def run_tc_color_head(device):
    from bayer_low_light_image_enhancement_amd import ops
    sd = TC.color_params(False)
    return host(out=ops.tc_color_head(TC.color_inputs(300).to(device), {k: v.to(device) for k, v in sd.items()}, TC.CC))


def run_ml_guidance(device, levels):
    m, x4 = ML.model(device, levels=levels), ML.frame("b2_16x24").to(device)
    g0, m0 = m.ml_guidance(x4, 0)
    g2, m2 = m.ml_guidance(x4, 2)
    used = [k for l in range(levels) for k in (2 * l, 2 * l + 1)] + [6]      # the other entries of the table are never written
    return host(guide0=g0, means0=m0[:, used], guide2=g2, means2=m2[:, used])


def run_ml_modulate(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    x, guide, p = ML.step_inputs(shape, 2)
    xd, gd, pd = x.to(device), guide.to(device), ML.on(device, p)
    return host(**{f"step{s}": ops.ml_modulate(xd, gd, ML.means_table(guide, s, 2).to(device), s, 2, pd) for s in range(3)})


def run_ml_step(device, c, hw):
    from bayer_low_light_image_enhancement_amd import ops
    x, guide, p = ML.step_inputs((2 if hw == (8, 8) else 1, c) + hw, 2)
    xd, gd, pd = x.to(device), guide.to(device), ML.on(device, p)
    out = {}
    for name, step in (("level", 1), ("chroma", 2)):
        mt = ML.means_table(guide, step, 2).to(device)
        out[name + "_plain"] = ops.ml_step_fused(xd, gd, mt, step, 2, pd)
        out[name], out[name + "_partial"] = ops.ml_step_fused(xd, gd, mt, step, 2, pd, sums=True)
    return host(**out)


def run_ml_residual(device):
    from bayer_low_light_image_enhancement_amd import ops
    out = {}
    for n in (1024, 1023):
        x, r = cases.rnd(f"gbits.res.x.{n}", (n,), -2.0, 2.0, seed=SEED), cases.rnd(f"gbits.res.r.{n}", (n,), -3.0, 3.0, seed=SEED)
        out[f"n{n}"] = ops.ml_residual(x.to(device), r.to(device))
    return host(**out)


def run_ml_tail(device):
    from oracle import rawformer_ref as R
    img, x = ML.tail_inputs("16x24")
    m = ML.model(device)
    return host(mosaic=m.ml_tail(img.to(device), x.to(device)), packed=m.ml_tail(img.to(device), R.pixel_unshuffle2(x).contiguous().to(device)))


RUNNERS = {"guidance": run_guidance,
           "flca_c24_6x7": lambda d: run_flca(d, (1, 24, 6, 7)), "flca_c40_6x10": lambda d: run_flca(d, (1, 40, 6, 10)),
           **{f"tc_guidance.{f}.l{l}": (lambda d, f=f, l=l: run_tc_guidance(d, f, l)) for f in TC.FRAMES for l in (1, 2, 3)},
           "tc_forward_mosaic": run_tc_forward_mosaic, "tc_pyramid": run_tc_pyramid,
           **{f"tc_gate.{tag_of(s)}": (lambda d, s=s: run_tc_gate(d, s)) for s in TC.SPATIAL_SHAPES},
           "tc_color_head": run_tc_color_head,
           **{f"ml_guidance.l{l}": (lambda d, l=l: run_ml_guidance(d, l)) for l in (1, 2, 3)},
           **{f"ml_modulate.{tag_of(s)}": (lambda d, s=s: run_ml_modulate(d, s)) for s in MOD_SHAPES},
           **{f"ml_step.c{c}.{tag_of(hw)}": (lambda d, c=c, hw=hw: run_ml_step(d, c, hw)) for c in (16, 32, 48, 64) for hw in STEP_HW},
           "ml_residual": run_ml_residual, "ml_tail": run_ml_tail}
CASE_IDS = list(RUNNERS)


def run_case(tag, device):
    """name -> array of everything the case digests."""
    return RUNNERS[tag](device)


def workspace_bytes():
    """'<variant>.l<depth>' -> rf_workspace_bytes at every WS_FRAMES entry; needs the library, no device."""
    from bayer_low_light_image_enhancement_amd import _lib
    lib = _lib.load()
    out = {}
    for name, variant in (("truecolor", _lib.RF_VARIANT_TRUECOLOR), ("multilvl", _lib.RF_VARIANT_MULTILVL)):
        for levels in (1, 2, 3):
            cfg = _lib.RfConfig(16, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, 2, variant, 1, 0, levels)
            h, sz = C.c_void_p(), C.c_size_t()
            _lib.check(lib.rf_create(C.byref(cfg), C.byref(h)), "rf_create")
            try:
                sizes = []
                for b, hh, ww in WS_FRAMES:
                    _lib.check(lib.rf_workspace_bytes(h, b, hh, ww, C.byref(sz)), "rf_workspace_bytes")
                    sizes.append(int(sz.value))
            finally:
                lib.rf_destroy(h)
            out[f"{name}.l{levels}"] = sizes
    return out


def test_cases_reach_the_forms_they_are_named_for():
    """The launch arithmetic of the three files restated, from the shapes alone."""
    assert 7 % 2 == 1 and 10 % 4 == 2 and (6 * 10) % 2 == 0 and 24 % 32 and 40 % 32      # ops.flca: scalar | PX = 2; channel tails
    assert [s[3] % 4 == 0 for s in TC.SPATIAL_SHAPES] == [True, False, True, True, False]
    assert [s[3] % 4 == 0 for s in MOD_SHAPES] == [True, False, True] and [-(-s[1] // 32) for s in MOD_SHAPES] == [1, 2, 3]
    for h, w in STEP_HW:
        assert all(ML.fused_supported(c, h, w) for c in (16, 32, 48, 64))
    assert 16 * 68 > 1024                                                                  # a second block of 64 pixels
    assert 1024 % 4 == 0 and 1023 % 4


def test_workspace_sizes_of_the_parent():
    with open(FIXTURE) as f:
        want = json.load(f)["workspace_bytes"]
    got = workspace_bytes()
    assert len(got) == 6 and set(got) == set(want)
    for tag in got:
        assert 0 < got[tag][0] < got[tag][1], (tag, got[tag])
        assert got[tag] == want[tag], f"[{tag}] workspace bytes at {WS_FRAMES} now {got[tag]}, recorded {want[tag]}"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASE_IDS)
def test_bits_of_the_parent(device, tag):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][tag]
    got = record(run_case(tag, device))
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k]["shape"] == want[k]["shape"], (tag, k)
        assert got[k]["sha256"] == want[k]["sha256"], f"[{tag}] {k}: bits moved; samples now {got[k]['samples']}, recorded {want[k]['samples']}"
