"""ops.flca_pyramid_backward and ops.ml_tail_backward (csrc/rf_flca_pyramid_bwd.hip) against float64 autograd of the restatement
tests/multilvl_ref.py.

Block.  Loss: ``<multilvl_ref.flca_pyramid(feat, guide, p), g>`` with a fixed random ``g``; truth = ``torch.autograd.grad`` in float64
with respect to ``feat`` and the 4 L + 11 parameter tensors (tests/flca_pyramid_grad_ref.py), e32 = the same computation in
float32.  Inputs: ``flca_pyramid_grad_ref.inputs(tag)``; seed = 6100 + the case's place in the table.

Cases (B, C, h, w, levels, H, W), each the smallest shape that reaches its branch:

==============================  ====================================================================================================
one_pixel (1,8,1,1,1,8,8)       P = 1: every tap but the centre is outside; plain weight-gradient path; hidden = 8 = C
base (2,16,16,16,2,16,16)       fused forward step; w % 4 == 0: the MFMA tap kernel; P % 4 == 0: gram2 weight gradients; sums over 2 images
odd (1,24,5,7,2,8,8)            scalar forms of every kernel; a channel tile of 8 after one of 16; P % 4 != 0
w_mod4_2 (2,16,6,10,2,16,24)    w % 4 == 2 with P % 4 == 0: the scalar tap kernel beside the float4 pointwise kernels and gram2
levels1 (1,16,8,8,1,8,8)        L = 1
levels3 (1,32,8,12,3,16,24)     L = 3: four steps share res_proj; P = 96: the composed forward at C = 32
c48 (1,48,8,8,2,16,16)          fused forward at C = 48; three channel tiles
deep (2,128,2,2,2,16,16)        U-Net level 3: guidance shrunk 8 x; composed forward; the scalar tap kernel over eight channel tiles
c512 (1,512,2,4,2,16,32)        largest C; hidden = 64; two passes of 256 threads over the channels in pyr_se_kernel
blocks (3,16,40,64,2,40,64)     P = 2560: five pixel slabs per image in the MFMA tap kernel (five rows per gate sum), three pooling blocks,
                                two pyr_dch blocks
up (1,16,24,16,2,8,8)           feature larger than the guidance (bilinear upsampling)
slabs_odd (1,8,23,23,1,8,8)     P = 529: two slabs, of 320 and 209 pixels, in the scalar tap kernel; three pooling blocks of 256
==============================  ====================================================================================================

(The last is this file's addition to the issue's table: the second slab of the scalar tap kernel.  No kernel of the block has a
grid cap: the pointwise kernels launch one thread per 4 or 1 elements, the tap kernels one workgroup per slab and tile.)

Bound, per gradient tensor (the scheme of tests/test_mamba.py, whose RATIO and FLOOR are imported): e64 = max|hip - ref_f64| <=
8 e32 + 2e-6 S with S = max|ref_f64|.  No exception is made for any tensor.  ``-s`` prints e64 / bound for every tensor of every
case; DESIGN.md section 4, "FLCA_Pyramid backward", holds the table measured on the MI355X.

Condition on the bound: before comparing, every case shows on the CPU that each defect of flca_pyramid_grad_ref.DEFECTS moves at
least one gradient tensor by >= 100 x that tensor's bound, and that no reference gradient tensor is identically zero.

Tail.  Loss ``<multilvl_ref.corrections(out, x4, y), g>``, truth = float64 autograd with respect to ``out``; ``out``, ``g``, ``x4`` uniform
in [0, 1] (a ``g`` whose channel means were near zero would hide ``anchor_mean_constant``).  The gradient does not depend on ``out``
or ``x4``: the map is affine.  Frames h2 x w2 (image size), by the launch arithmetic of rf_ml_corrections_backward (sums: at most 256
workgroups per image, apply: at most 1024, each of 256 lanes x 4 pixels where w2 % 4 == 0, else x 1):

==================  ================================================================================================================
16x16 (B = 2)       packed 8 x 8; one workgroup; the sum over the partials is per image
16x80               packed 8 x 40
6x10                w2 % 4 != 0: the scalar forms
512x520             266 240 pixels = 260 workgroups' worth on the 256 of the sums kernel: workgroups 0 .. 3 take a second trip
1024x1032           1 056 768 pixels = 1032 workgroups' worth on the 1024 of the apply kernel (five trips in the sums kernel)
514x518             scalar forms past both caps: 266 252 pixels on 256 and on 1024 workgroups of 256 pixels
==================  ================================================================================================================

The same bound; the three defects of flca_pyramid_grad_ref.TAIL_DEFECTS move the gradient by >= 100 x it on every frame.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import cases
import flca_pyramid_grad_ref as G
import multilvl_ref as M
from bayer_low_light_image_enhancement_amd import _lib, ops
from oracle import rawformer_ref as R
from test_mamba import FLOOR, RATIO

CASES = G.CASES
TAIL_FRAMES = {"16x16": (2, 16, 16), "16x80": (1, 16, 80), "6x10": (1, 6, 10), "512x520": (1, 512, 520), "1024x1032": (1, 1024, 1032),
               "514x518": (1, 514, 518)}      # B, h2, w2
TAIL_SUMS_CAP, TAIL_APPLY_CAP = 256, 1024      # kTailSumBlocks, kTailApplyBlocks (csrc/rf_flca_pyramid_bwd.hip)
TAIL_SEED = 6200


def names_of(tag):
    return ("feat",) + tuple(G.param_shapes(CASES[tag][1], CASES[tag][4]))


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Inputs, the float64 and float32 gradients, the bounds and what each defect moves: computed once, shared, never changed."""
    feat, x4, p, g = G.inputs(tag)
    L = CASES[tag][4]
    names = names_of(tag)
    guide64, p64 = R.bayer_luma_chroma(x4.double()), {k: v.double() for k, v in p.items()}
    ref64 = G.gradients(feat.double(), guide64, p64, g.double(), L)
    ref32 = G.gradients(feat, R.bayer_luma_chroma(x4), p, g, L)
    assert tuple(ref64) == names and all(ref64[k].dtype == torch.float64 and ref32[k].dtype == torch.float32 for k in names)
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in names}
    mx = {k: float(ref64[k].abs().max()) for k in names}
    bound = {k: RATIO * e32[k] + FLOOR * mx[k] for k in names}
    moved = {}
    for d in G.DEFECTS:
        bad = G.gradients(feat.double(), guide64, p64, g.double(), L, defect=d)
        moved[d] = {k: float((bad[k] - ref64[k]).abs().max()) for k in names}
    return {"feat": feat, "x4": x4, "p": p, "g": g, "levels": L, "ref64": ref64, "e32": e32, "max": mx, "bound": bound, "moved": moved}


def assert_bound_sees_defects(tag):
    c = reference(tag)
    for k, v in c["max"].items():
        assert math.isfinite(v) and v > 0.0, f"[{tag}] the reference gradient {k} is identically zero or not finite"
    for d, moved in c["moved"].items():
        ratio = {k: moved[k] / c["bound"][k] for k in moved}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {moved[best]:.3e} against the "
                                      f"bound {c['bound'][best]:.3e}): the case cannot see it")


@functools.lru_cache(maxsize=None)
def tail_reference(tag):
    b, h2, w2 = TAIL_FRAMES[tag]
    out = cases.rnd(f"pyr.tail.out.{tag}", (b, 3, h2, w2), 0.0, 1.0, seed=TAIL_SEED)
    g = cases.rnd(f"pyr.tail.g.{tag}", (b, 3, h2, w2), 0.0, 1.0, seed=TAIL_SEED)
    x4 = cases.rnd(f"pyr.tail.x4.{tag}", (b, 4, 8, 8), 0.0, 1.0, seed=TAIL_SEED)      # (the gradient does not depend on it: any frame serves)
    ref64 = G.tail_gradient(out.double(), x4.double(), g.double())
    e32 = float((G.tail_gradient(out, x4, g).double() - ref64).abs().max())
    bound = RATIO * e32 + FLOOR * float(ref64.abs().max())
    return {"out": out, "g": g, "x4": x4, "ref64": ref64, "e32": e32, "bound": bound}


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["one_pixel", "odd", "levels3", "up"])
def test_copy_with_detach_points_is_the_restatement(tag):
    c = reference(tag)
    guide, p64 = R.bayer_luma_chroma(c["x4"].double()), {k: v.double() for k, v in c["p"].items()}
    with torch.no_grad():
        want = M.flca_pyramid(c["feat"].double(), guide, p64, "", c["levels"])
        for d in (None,) + G.DEFECTS:                      # a detach point changes the gradient, never the value
            got = G.flca_pyramid(c["feat"].double(), guide, p64, "", c["levels"], d)
            assert float((got - want).abs().max()) <= 1e-12, (tag, d)
        y = guide[0]
        out = cases.rnd("pyr.tail.value", (1, 3) + tuple(2 * s for s in c["x4"].shape[2:]), 0.0, 1.0, seed=TAIL_SEED).double()
        for d in (None,) + G.TAIL_DEFECTS:
            assert float((G.corrections(out, c["x4"].double(), y, d) - M.corrections(out, c["x4"].double(), y)).abs().max()) <= 1e-12, (tag, d)


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_cannot_hide_the_defects(tag):
    assert_bound_sees_defects(tag)


@pytest.mark.parametrize("tag", ["16x16", "16x80", "6x10"])
def test_tail_bound_cannot_hide_the_defects_and_the_closed_form_is_the_adjoint(tag):
    c = tail_reference(tag)
    g = c["g"].double()
    w = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64).view(1, 3, 1, 1)
    g1 = g - 0.03 * w * g.sum(dim=1, keepdim=True)
    closed = g1 - 0.12 * g1.mean(dim=(2, 3), keepdim=True)
    assert float((closed - c["ref64"]).abs().max()) <= 1e-14                 # the formula of the kernels, no input but g
    assert float(c["g"].mean(dim=(0, 2, 3)).min()) > 0.3                       # channel means away from zero
    for d in G.TAIL_DEFECTS:
        moved = float((G.tail_gradient(c["out"].double(), c["x4"].double(), g, d) - c["ref64"]).abs().max())
        print(f"tail {tag}: bound {c['bound']:.3e}, {d} moves the gradient by {moved / c['bound']:.0f} x it")
        assert moved >= 100.0 * c["bound"], (tag, d, moved, c["bound"])


def test_cases_reach_the_branches_they_are_named_for():
    """The launch arithmetic of csrc/rf_flca_pyramid_bwd.hip restated, from the shapes alone."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    shp = CASES
    P = {t: s[2] * s[3] for t, s in shp.items()}
    # tap kernel: MFMA form where w % 4 == 0, else scalar; pointwise kernels and wgrad1x1 (gram2): float4 / gram where P % 4 == 0
    assert [t for t in shp if shp[t][3] % 4 != 0] == ["one_pixel", "odd", "w_mod4_2", "deep", "slabs_odd"]
    assert [t for t in shp if P[t] % 4 != 0] == ["one_pixel", "odd", "slabs_odd"]
    assert shp["w_mod4_2"][3] % 4 == 2 and P["w_mod4_2"] % 4 == 0 and shp["deep"][3] == 2 and P["deep"] == 4
    # 16-channel tiles: a partial last tile, several tiles
    assert [cdiv(shp[t][1], 16) for t in ("one_pixel", "odd", "c48", "deep", "c512")] == [1, 2, 3, 8, 32] and shp["odd"][1] % 16 == 8
    assert shp["one_pixel"][1] == 8 == max(8, shp["one_pixel"][1] // 8) and max(8, shp["c512"][1] // 8) == 64 and shp["c512"][1] > 256

    def slabs(b, p, tiles):      # pyr_slabs: pixels per slab (a multiple of 64, 512 or more where the image has them), slabs per image
        per = min(cdiv(1024, b * tiles), cdiv(p, 512))
        px = cdiv(cdiv(p, per), 64) * 64
        return px, cdiv(p, px)
    per_image = {t: slabs(s[0], P[t], cdiv(s[1], 16)) for t, s in shp.items()}
    assert [t for t in shp if per_image[t][1] > 1] == ["blocks", "slabs_odd"]
    assert per_image["blocks"] == (512, 5) and per_image["slabs_odd"] == (320, 2) and P["slabs_odd"] - 320 == 209
    assert per_image["base"] == (256, 1) and 256 // 64 == 4                                # one slab: 4 trips of 16 pixels per wave
    assert slabs(4, 256 * 256, 2) == (512, 128) and slabs(4, 32 * 32, 16) == (512, 2)      # the stage shapes DESIGN.md times: 1024 and 128 workgroups
    # pyr_dch_kernel: min(16, cdiv(P, 2048)) blocks per image and channel; pooling blocks: tc_nblk
    assert {t: min(16, cdiv(P[t], 2048)) for t in ("base", "blocks")} == {"base": 1, "blocks": 2}
    assert cdiv(P["blocks"], 1024) == 3 and cdiv(P["slabs_odd"], 256) == 3
    assert [shp[t][4] for t in ("levels1", "base", "levels3")] == [1, 2, 3] and shp["base"][0] == 2 and shp["blocks"][0] == 3
    # the tail: workgroups' worth of pixels against the two caps
    trips = {}
    for tag, (b, h2, w2) in TAIL_FRAMES.items():
        px = 4 if w2 % 4 == 0 else 1
        n = cdiv(h2 * w2 // px, 256)
        trips[tag] = (px, cdiv(n, min(n, TAIL_SUMS_CAP)), cdiv(n, min(n, TAIL_APPLY_CAP)))
    assert trips == {"16x16": (4, 1, 1), "16x80": (4, 1, 1), "6x10": (1, 1, 1), "512x520": (4, 2, 1), "1024x1032": (4, 5, 2), "514x518": (1, 5, 2)}
    assert cdiv(512 * 520 // 4, 256) == TAIL_SUMS_CAP + 4 and cdiv(1024 * 1032 // 4, 256) == TAIL_APPLY_CAP + 8


def test_host_checks_refuse_unsupported_shapes_before_any_launch():
    lib = _lib.load()
    b, c, h, w, H, W, L = good = (2, 16, 6, 10, 16, 24, 2)
    need = lib.rf_flca_pyramid_backward_workspace_bytes(*good)
    assert need > lib.rf_flca_pyramid_workspace_bytes(*good) > 0
    # never dereferenced: the checks come first.  Every buffer has an address of its own, of its true size, clear of the others
    n, plane, frame = 4 * L + 11, 4 * b * c * h * w, 4 * b * 4 * H * W
    tensors = [4 * math.prod(s) for s in ops.flca_pyramid_param_shapes(c, L).values()]
    at = cases.fake_addresses([plane] * 3 + [frame, need] + 2 * tensors)
    feat, g, dx, x4, ws = (C.c_void_p(v) for v in at[:5])
    prm, grd = (C.c_void_p * n)(*at[5:5 + n]), (C.c_void_p * n)(*at[5 + n:])
    call, err = lib.rf_flca_pyramid_backward, lib.rf_last_error
    for bad, word in (((b, c, h, w, H, W, 0), b"levels=0"), ((b, c, h, w, H, W, 4), b"levels=4"), ((b, 513, h, w, H, W, L), b"C=513"),
                      ((b, c, h, w, 12, W, L), b"multiples of 8"), ((b, c, h, w, H, 28, L), b"multiples of 8"), ((0, c, h, w, H, W, L), b"positive"),
                      ((b, c, h, 0, H, W, L), b"positive")):
        assert lib.rf_flca_pyramid_backward_workspace_bytes(*bad) == -22
        assert err().startswith(b"rf_flca_pyramid_backward_workspace_bytes: ") and word in err(), err()
        assert call(feat, x4, g, dx, prm, grd, ws, 1 << 40, *bad, 0, None) == -22
        assert err().startswith(b"rf_flca_pyramid_backward: ") and word in err(), err()
    for shape in CASES.values():                                                    # every case's geometry is accepted
        bb, cc, hh, ww, LL, HH, WW = shape
        assert lib.rf_flca_pyramid_backward_workspace_bytes(bb, cc, hh, ww, HH, WW, LL) > 0
    assert call(feat, x4, g, dx, prm, grd, ws, need - 1, *good, 0, None) == -12
    assert err().startswith(b"rf_flca_pyramid_backward: workspace")
    for args in ((None, x4, g, dx), (feat, x4, None, dx), (feat, x4, g, None)):
        assert call(*args, prm, grd, ws, 1 << 40, *good, 0, None) == -22 and err().startswith(b"rf_flca_pyramid_backward: ")
    assert call(feat, None, g, dx, prm, grd, ws, 1 << 40, *good, 0, None) == -22 and b"buffer 0 is null" in err()      # the packed frame
    holed = (C.c_void_p * n)(*prm)
    holed[7] = None
    assert call(feat, x4, g, dx, holed, grd, ws, 1 << 40, *good, 0, None) == -22 and b"7 is null" in err()
    assert call(feat, x4, g, C.c_void_p(dx.value + 4), prm, grd, ws, 1 << 40, *good, 0, None) == -22 and b"aligned" in err()

    def refused_as_alias(*args):
        assert call(*args, 1 << 40, *good, 0, None) == -22
        assert err().startswith(b"rf_flca_pyramid_backward: ") and b"alias" in err(), err()

    inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
    refused_as_alias(feat, x4, g, feat, prm, grd, ws)                 # grad_feat on feat
    refused_as_alias(feat, x4, g, inside(feat, 64), prm, grd, ws)     # ... inside feat
    refused_as_alias(feat, x4, g, g, prm, grd, ws)                    # ... on grad_out
    refused_as_alias(feat, x4, g, inside(x4, 256), prm, grd, ws)      # ... inside the packed frame, which is read
    refused_as_alias(feat, x4, g, dx, prm, grd, inside(x4, 16))       # the workspace over the packed frame
    refused_as_alias(feat, x4, g, dx, prm, grd, inside(dx, 64))       # ... over grad_feat
    for i, target in ((3, prm[5]), (0, dx.value), (2, grd[7]), (1, ws.value + 1024), (n - 1, g.value + 32), (8, x4.value + 128)):
        bad_grd = (C.c_void_p * n)(*grd)
        bad_grd[i] = target                                           # a gradient on a parameter, grad_feat, another gradient, the workspace, ...
        refused_as_alias(feat, x4, g, dx, prm, bad_grd, ws)
    assert call(feat, x4, inside(feat, 16), dx, prm, grd, ws, need - 1, *good, 0, None) == -12      # inputs may overlap: refused for the workspace alone

    # the tail
    tail, tneed = lib.rf_ml_corrections_backward, lib.rf_ml_corrections_backward_workspace_bytes(2, 16, 16)
    assert tneed > 0 and tneed % 16 == 0 and lib.rf_ml_corrections_backward_workspace_bytes(4, 16, 16) >= tneed
    ta = cases.fake_addresses([4 * 2 * 3 * 256] * 2 + [tneed])
    tg, to, tw = (C.c_void_p(v) for v in ta)
    for bad in ((0, 16, 16), (2, 0, 16), (65536, 16, 16), (1, 1 << 16, 1 << 15)):
        assert lib.rf_ml_corrections_backward_workspace_bytes(*bad) == -22 and err().startswith(b"rf_ml_corrections_backward_workspace_bytes: ")
        assert tail(tg, to, tw, 1 << 40, *bad, None) == -22 and err().startswith(b"rf_ml_corrections_backward: ")
    assert tail(None, to, tw, tneed, 2, 16, 16, None) == -22 and b"non-null" in err()
    assert tail(tg, inside(to, 8), tw, tneed, 2, 16, 16, None) == -22 and b"aligned" in err()
    assert tail(tg, to, tw, tneed - 1, 2, 16, 16, None) == -12 and err().startswith(b"rf_ml_corrections_backward: workspace")
    assert tail(tg, tg, tw, tneed, 2, 16, 16, None) == -22 and b"alias" in err()
    assert tail(tg, to, inside(to, 16), tneed, 2, 16, 16, None) == -22 and b"alias" in err()


# ------------------------------------------------------------------------------------------ GPU
def run(device, tag):
    c = reference(tag)
    return c, {k: v.to(device) for k, v in c["p"].items()}, c["feat"].to(device), c["x4"].to(device), c["g"].to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_float64_autograd(device, tag):
    assert_bound_sees_defects(tag)
    c, p, feat, x4, g = run(device, tag)
    names, L = names_of(tag), c["levels"]
    dx, grads = ops.flca_pyramid_backward(feat, x4, p, g, levels=L)
    dx2, grads2 = ops.flca_pyramid_backward(feat, x4, p, g, levels=L)
    torch.cuda.synchronize()
    assert torch.equal(feat.cpu(), c["feat"]) and torch.equal(x4.cpu(), c["x4"]) and torch.equal(g.cpu(), c["g"]), f"[{tag}] an input was written"
    assert all(torch.equal(p[k].cpu(), c["p"][k]) for k in p), f"[{tag}] a parameter was written"
    got, again = {"feat": dx, **grads}, {"feat": dx2, **grads2}
    assert set(got) == set(names) and dx.data_ptr() != feat.data_ptr()
    failed = []
    for k in names:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (tag, k)
        assert torch.equal(got[k], again[k]), f"[{tag}] {k}: two runs differ"
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        msg = (f"[{tag}] {k:26s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} S {c['max'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / c['bound'][k]:.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["base", "odd", "levels3"])      # gram2's accumulation, the plain kernel's, four steps into res_proj
def test_passing_grads_accumulates(device, tag):
    c, p, feat, x4, g = run(device, tag)
    dx, grads = ops.flca_pyramid_backward(feat, x4, p, g, levels=c["levels"])
    once = {k: v.clone() for k, v in grads.items()}
    dx2, same = ops.flca_pyramid_backward(feat, x4, p, g, levels=c["levels"], grads=grads)
    assert same is grads and set(grads) == set(names_of(tag)[1:])
    assert torch.equal(dx, dx2) and dx.data_ptr() != dx2.data_ptr(), "grad_feat is a new tensor, overwritten, never accumulated"
    for k in grads:
        assert torch.equal(grads[k], 2.0 * once[k]), k


@pytest.mark.gpu
def test_prefix_and_a_wrong_shape(device):
    c, p, feat, x4, g = run(device, "levels1")
    pre = "conv_tran3.FLCA."
    dx, grads = ops.flca_pyramid_backward(feat, x4, {pre + k: v for k, v in p.items()}, g, prefix=pre, levels=1)
    want_dx, want = ops.flca_pyramid_backward(feat, x4, p, g, levels=1)
    assert torch.equal(dx, want_dx) and all(torch.equal(grads[pre + k], want[k]) for k in want)
    with pytest.raises(RuntimeError, match="levels=4"):
        ops.flca_pyramid_backward(feat, x4, p, g, levels=4)
    with pytest.raises(RuntimeError, match="differ"):
        ops.flca_pyramid_backward(feat, x4, p, g[:, :8], levels=1)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(TAIL_FRAMES))
def test_tail_matches_float64_autograd(device, tag):
    c = tail_reference(tag)
    g = c["g"].to(device)
    got = ops.ml_tail_backward(g)
    again = ops.ml_tail_backward(g)
    assert torch.equal(g.cpu(), c["g"]), "grad_out was written"
    assert torch.equal(got, again), "two calls differ"
    e64 = float((got.cpu().double() - c["ref64"]).abs().max())
    print(f"[tail {tag}] e64 {e64:.3e} e32 {c['e32']:.3e} | bound {c['bound']:.3e} ({e64 / c['bound']:.3f} of it)")
    assert e64 <= c["bound"]
