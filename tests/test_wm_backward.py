"""ops.wm_backward (csrc/rf_wm_bwd.hip) against float64 autograd of the restatement tests/mamba_ref.py.

Loss: ``<mamba_ref.wm(x, p), g>`` with a fixed random ``g``; truth = ``torch.autograd.grad`` in float64 with respect to ``x`` and the
17 parameter tensors (tests/wm_grad_ref.py), e32 = the same computation in float32.  Parameters: ``test_mamba.wm_params`` with the
per-case delta range; inputs ``cases.rnd("wm_bwd.<tag>.x" / ".g")``; seed = 4500 + the case's place in the table.

Cases (n, c, h, w), each the smallest shape that reaches its branch; Lc = rf_mamba_chunk_len():

======================  ============================================================================================================
one_pixel (1,4,1,1)     one token, the smallest c, the plain weight-gradient kernel
base (3,16,8,8)         gram2<9> with one A tile; L % c == 0
w_mod4_2 (2,16,6,10)    w % 4 == 2: the plain weight-gradient kernel; L = 60: rows straddle channel planes
odd (1,24,5,7)          L = 35: Mamba's scalar-row path; partial 32-wide tiles in the LayerNorm adjoint (c = 24, 35 rows)
chunks (3,32,16,24)     L = 384: three scan chunks, 12 row groups per image
c64 (1,64,16,16)        Di = 128: two channel tiles; two A tiles in gram2<9>
c256_w2 (3,256,2,2)     level-3 channels of RawFormer-S, Cin = 512, rows of 256 floats, the plain weight-gradient kernel
c256_w4 (1,256,4,4)     the same through gram2<9>
c512 (1,512,2,4)        the largest c the forward accepts: rows of 512 floats, all 8 register slots of the row pass
c32_L130 (1,32,10,13)   L = 130: a second chunk of two tokens
======================  ============================================================================================================

Bound, per gradient tensor (the scheme of tests/test_mamba.py, whose RATIO and FLOOR are imported): e64 = max|hip - ref_f64| <=
8 e32 + 2e-6 S with S = max|ref_f64|.  One exception: where L % c == 0 every token lies inside one channel plane, LayerNorm
removes a per-row constant, and d convb.2.bias is zero in exact arithmetic (float64 autograd: about 1e-14; float32: about 3e-6 of
cancellation noise).  For that tensor in those cases S = max over channels of sum_{n,h,w} |g_r|, the sum of the absolute
summands, with g_r from ``autograd.grad`` with respect to the intermediate r.  (base, chunks, c64.  In c256_w4, L = 16 < c, a token
is 16 whole channel planes: the sum over a plane does not cancel and the tensor keeps the plain bound, the smaller of the two.)
In one_pixel d model1.A_log is exactly 0
(h_{-1} = 0): its bound is 0 and the operator returns exact zeros.  ``-s`` prints e64 / bound for every tensor of every case;
DESIGN.md section 4, "WM backward", holds the table measured on the MI355X.

Measured on the MI355X: the largest e64 / bound per case is 0.17 .. 0.62 (c256_w4: 0.375, model1.dt_proj.weight).  c256_w4 is the
case that needs the input-channel split the backward gives its small 3x3 convolution launches: with one accumulator over all
9 x 512 products per output the convolution kernel alone was at 4.7e-6 max|out| there and model1.conv1d.bias at 1.035 of its bound
(DESIGN.md has the account).

Condition on the bound: before comparing, each case shows on the CPU that each defect of wm_grad_ref.DEFECTS that applies to it
(``tokens_as_permute``: L > 1; ``cut_adjoint``: L > Lc; the others: all) moves at least one gradient tensor by >= 100 x that
tensor's bound.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
import mamba_grad_ref as MG
import mamba_ref as M
import wm_grad_ref as G
from bayer_low_light_image_enhancement_amd import _lib, ops
from test_mamba import FLOOR, RATIO, lc, wm_params

SEED = 4500
NAMES = ("x",) + G.KEYS
# id: (shape, delta range), in the order that fixes the seeds
CASES = {
    "one_pixel": ((1, 4, 1, 1), (0.05, 0.5)),
    "base": ((3, 16, 8, 8), (0.01, 0.2)),
    "w_mod4_2": ((2, 16, 6, 10), (0.01, 0.2)),
    "odd": ((1, 24, 5, 7), (0.01, 0.2)),
    "chunks": ((3, 32, 16, 24), (0.005, 0.1)),
    "c64": ((1, 64, 16, 16), (0.005, 0.1)),
    "c256_w2": ((3, 256, 2, 2), (0.05, 0.5)),
    "c256_w4": ((1, 256, 4, 4), (0.05, 0.5)),
    "c512": ((1, 512, 2, 4), (0.05, 0.5)),
    "c32_L130": ((1, 32, 10, 13), (0.005, 0.1)),
}
B2 = "convb.2.bias"


def defects_of(shape, n):
    L = shape[2] * shape[3]
    out = ["no_skip", "relu_passthrough", "ln_no_projection"]
    if L > 1:
        out.append("tokens_as_permute")
    if L > n:
        out.append("cut_adjoint")
    return out


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Inputs, parameters, the float64 and float32 gradients, the bounds and what each defect moves: computed once, shared, never
    changed."""
    shape, (dlo, dhi) = CASES[tag]
    n = lc()
    seed = SEED + list(CASES).index(tag)
    p = wm_params(shape[1], seed, dlo, dhi)
    x = cases.rnd(f"wm_bwd.{tag}.x", shape, seed=seed)
    g = cases.rnd(f"wm_bwd.{tag}.g", shape, seed=seed)
    p64 = {k: v.double() for k, v in p.items()}
    ref64, gr64 = G.gradients(x.double(), p64, g.double())
    ref32, _ = G.gradients(x, p, g)
    assert all(ref64[k].dtype == torch.float64 and ref32[k].dtype == torch.float32 for k in NAMES)
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in NAMES}
    mx = {k: float(ref64[k].abs().max()) for k in NAMES}
    scale = dict(mx)
    if (shape[2] * shape[3]) % shape[1] == 0:                # d convb.2.bias is a sum that cancels to 0: module docstring
        scale[B2] = float(gr64.abs().sum(dim=(0, 2, 3)).max())
    bound = {k: RATIO * e32[k] + FLOOR * scale[k] for k in NAMES}
    moved = {}
    for d in defects_of(shape, n):
        bad, _ = G.gradients(x.double(), p64, g.double(), defect=d, chunk=n)
        moved[d] = {k: float((bad[k] - ref64[k]).abs().max()) for k in NAMES}
    return {"x": x, "g": g, "p": p, "ref64": ref64, "e32": e32, "max": mx, "scale": scale, "bound": bound, "moved": moved}


def assert_bound_sees_defects(tag):
    c = reference(tag)
    assert all(math.isfinite(c["max"][k]) for k in NAMES) and c["max"]["x"] > 0
    for d, moved in c["moved"].items():
        # (dA_log of one_pixel is exactly 0, h_{-1} being 0: its bound is 0 and nothing moves it)
        ratio = {k: moved[k] / c["bound"][k] for k in NAMES if c["bound"][k] > 0}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {moved[best]:.3e} against the "
                                      f"bound {c['bound'][best]:.3e}): the case cannot see it")


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["w_mod4_2", "odd", "c32_L130"])
def test_copy_with_detach_points_is_the_restatement(tag):
    c = reference(tag)
    p64 = {k: v.double() for k, v in c["p"].items()}
    with torch.no_grad():
        want = M.wm(c["x"].double(), p64)
        for d in (None,) + G.DEFECTS:                      # a detach point changes the gradient, never the value
            got = G.wm(c["x"].double(), p64, "", d, lc())
            assert float((got - want).abs().max()) <= 1e-12, (tag, d)


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_cannot_hide_the_defects(tag):
    assert_bound_sees_defects(tag)


def test_cases_reach_the_branches_they_are_named_for():
    n = lc()
    shp = {t: CASES[t][0] for t in CASES}
    L = {t: s[2] * s[3] for t, s in shp.items()}
    assert [t for t in CASES if shp[t][3] % 4 != 0] == ["one_pixel", "w_mod4_2", "odd", "c256_w2", "c32_L130"]      # the plain weight gradient
    assert shp["w_mod4_2"][3] % 4 == 2 and shp["c256_w2"][3] % 4 == 2
    assert [t for t in CASES if L[t] % 4 != 0] == ["one_pixel", "odd", "c32_L130"]                                  # Mamba's scalar-row GEMMs
    assert [t for t in CASES if L[t] % shp[t][1] == 0] == ["base", "chunks", "c64"]                                 # d convb.2.bias cancels
    assert [t for t in CASES if L[t] > n] == ["chunks", "c64", "c32_L130"] == [t for t in CASES if "cut_adjoint" in reference(t)["moved"]]
    assert L["chunks"] == 3 * n and L["c32_L130"] == n + 2 and L["one_pixel"] == 1
    assert L["w_mod4_2"] % shp["w_mod4_2"][1] != 0 and L["odd"] % 32 != 0 and shp["odd"][1] % 32 != 0
    assert 2 * shp["c64"][1] > MG.TILE and shp["c512"][1] == 512 and 2 * shp["c256_w2"][1] == 512
    r = reference("one_pixel")
    assert r["bound"]["model1.A_log"] == 0.0 and r["max"]["model1.A_log"] == 0.0
    for t in CASES:                                         # the exception of the bound: the sum cancels, its summands do not
        r = reference(t)
        if L[t] % shp[t][1] == 0:
            assert r["max"][B2] <= 1e-10 * r["scale"][B2] and r["scale"][B2] > 0, (t, r["max"][B2], r["scale"][B2])
        else:                                               # (c256_w4: a token is 16 whole planes, a plane's sum does not cancel)
            assert r["scale"][B2] == r["max"][B2] > 1e-3, (t, r["max"][B2])


def test_host_checks_refuse_unsupported_shapes_before_any_launch():
    lib = _lib.load()
    good = (6, 32, 16, 24)
    need = lib.rf_wm_backward_workspace_bytes(*good)
    assert need >= lib.rf_wm_workspace_bytes(*good) > 0
    # never dereferenced: the checks come first.  Every buffer has an address of its own, of its true size, clear of the others
    n, plane, a = 17, 4 * math.prod(good), good
    tensors = [4 * math.prod(s) for s in ops.wm_param_shapes(good[1]).values()]
    at = cases.fake_addresses([plane] * 3 + [need] + 2 * tensors)
    x, g, dx, ws = (C.c_void_p(v) for v in at[:4])
    prm, grd = (C.c_void_p * n)(*at[4:4 + n]), (C.c_void_p * n)(*at[4 + n:])
    call = lib.rf_wm_backward
    for bad, word in (((6, 18, 16, 24), b"c 18"), ((6, 516, 16, 24), b"c 516"), ((0, 32, 16, 24), b"n 0"), ((6, 32, 0, 24), b"0 x 24")):
        assert lib.rf_wm_backward_workspace_bytes(*bad) < 0
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_wm_backward_workspace_bytes: ") and word in msg, msg
        assert lib.rf_wm_backward(x, g, dx, prm, grd, ws, 1 << 40, *bad, 0, None) == -22
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_wm_backward: ") and word in msg, msg
    for ok in ((1, 4, 1, 1), (2, 16, 6, 10), (1, 512, 2, 4), (1, 24, 5, 7)):      # every shape the forward accepts
        assert lib.rf_wm_backward_workspace_bytes(*ok) >= lib.rf_wm_workspace_bytes(*ok) > 0
    assert lib.rf_wm_backward(x, g, dx, prm, grd, ws, need - 1, *good, 0, None) == -12
    assert lib.rf_last_error().startswith(b"rf_wm_backward: workspace")
    for trio in ((x, x, dx), (x, g, x), (x, g, g)):
        assert lib.rf_wm_backward(*trio, prm, grd, ws, 1 << 40, *good, 0, None) == -22
        assert lib.rf_last_error().startswith(b"rf_wm_backward: ") and b"alias" in lib.rf_last_error()
    assert lib.rf_wm_backward(x, g, None, prm, grd, ws, 1 << 40, *good, 0, None) == -22
    assert lib.rf_last_error().startswith(b"rf_wm_backward: ")
    assert lib.rf_wm_backward(x, g, C.c_void_p(dx.value + 4), prm, grd, ws, 1 << 40, *good, 0, None) == -22
    assert lib.rf_last_error().startswith(b"rf_wm_backward: ") and b"aligned" in lib.rf_last_error()

    def refused_as_alias(*args):
        assert call(*args, 1 << 40, *a, 0, None) == -22
        assert lib.rf_last_error().startswith(b"rf_wm_backward: ") and b"alias" in lib.rf_last_error(), lib.rf_last_error()

    inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
    refused_as_alias(x, g, inside(g, 4096), prm, grd, ws)         # grad_in inside grad_out
    refused_as_alias(x, g, dx, prm, grd, inside(x, 16))           # the workspace over in
    refused_as_alias(x, g, dx, prm, grd, inside(dx, 64))          # ... over grad_in
    refused_as_alias(x, g, dx, prm, grd, C.c_void_p(prm[n - 1] - 256))      # ... over a parameter
    for i, target in ((3, prm[5]), (0, dx.value), (2, grd[7]), (1, ws.value + 1024), (n - 1, g.value + 32), (4, grd[5] - 16)):
        bad_grd = (C.c_void_p * n)(*grd)
        bad_grd[i] = target                                       # a gradient on a parameter, grad_in, another gradient, the workspace, ...
        refused_as_alias(x, g, dx, prm, bad_grd, ws)
    assert call(x, inside(x, 16), dx, prm, grd, ws, need - 1, *a, 0, None) == -12      # inputs may overlap: refused for the workspace alone


# ------------------------------------------------------------------------------------------ GPU
def run(device, tag):
    c = reference(tag)
    p = {k: v.to(device) for k, v in c["p"].items()}
    return c, p, c["x"].to(device), c["g"].to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_float64_autograd(device, tag):
    assert_bound_sees_defects(tag)
    c, p, x, g = run(device, tag)
    keep_x, keep_g, keep_p = x.clone(), g.clone(), {k: v.clone() for k, v in p.items()}
    dx, grads = ops.wm_backward(x, p, g)
    dx2, grads2 = ops.wm_backward(x, p, g)
    torch.cuda.synchronize()
    assert torch.equal(x, keep_x) and torch.equal(g, keep_g), f"[{tag}] an input was written"
    assert all(torch.equal(p[k], keep_p[k]) for k in p), f"[{tag}] a parameter was written"
    got = {"x": dx, **grads}
    again = {"x": dx2, **grads2}
    assert set(got) == set(NAMES)
    failed = []
    for k in NAMES:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (tag, k)
        assert torch.equal(got[k], again[k]), f"[{tag}] {k}: two runs differ"
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        msg = (f"[{tag}] {k:24s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} S {c['scale'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / max(c['bound'][k], 1e-300):.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["base", "w_mod4_2"])          # launch_gram2's accumulation and the plain kernel's
def test_passing_grads_accumulates(device, tag):
    c, p, x, g = run(device, tag)
    dx, grads = ops.wm_backward(x, p, g)
    once = {k: v.clone() for k, v in grads.items()}
    dx2, same = ops.wm_backward(x, p, g, grads=grads)
    assert same is grads and set(grads) == set(G.KEYS)
    assert torch.equal(dx, dx2), "grad_x is overwritten, never accumulated"
    for k in G.KEYS:
        assert torch.equal(grads[k], 2.0 * once[k]), k


@pytest.mark.gpu
def test_mamba_part_is_mamba_backward(device):
    """With convb = 0 and smooth = the identity (the configuration of test_wm_tokens_are_runs_of_c_floats) wm(x) = Mamba(LN(tokens)),
    so the nine model1 gradients of wm_backward are those of ops.mamba_backward on (tok, g), tok = LayerNorm of the runs of c
    floats computed by torch, stored channel-major.  Compared within the float64 bound of this configuration (8 e32 + 2e-6 max|ref|
    per tensor), not bit for bit: on the MI355X no tensor was torch.equal, because torch's LayerNorm rounds differently from
    tok_transpose_kernel<true> and g passes through smooth's Winograd transform, which is not exact for the identity either.  The
    differences were 0.05 .. 0.12 of the bound."""
    c, p, x, g = run(device, "chunks")
    n, ch, h, w = x.shape
    for k in ("convb.0.weight", "convb.0.bias", "convb.2.weight", "convb.2.bias", "smooth.bias", "smooth.weight"):
        p[k] = torch.zeros_like(p[k])
    p["smooth.weight"][torch.arange(ch), torch.arange(ch), 1, 1] = 1.0
    tok = torch.nn.functional.layer_norm(x.reshape(n, h * w, ch), (ch,), p["ln.weight"], p["ln.bias"], 1e-5)
    pm = {k: p["model1." + k] for k in MG.KEYS}
    _, want = ops.mamba_backward(tok.transpose(1, 2).contiguous(), pm, g.reshape(n, ch, h * w), channel_major=True)
    _, grads = ops.wm_backward(x, p, g)
    # the float64 gradients of this configuration, for the bound of a comparison that is not bit for bit
    p64 = {k: v.double().cpu() for k, v in pm.items()}
    tok64 = torch.nn.functional.layer_norm(c["x"].double().reshape(n, h * w, ch), (ch,), p["ln.weight"].double().cpu(),
                                           p["ln.bias"].double().cpu(), 1e-5)
    g_tok = c["g"].reshape(n, ch, h * w).transpose(1, 2)
    ref64 = MG.gradients(tok64, p64, g_tok.double())
    ref32 = MG.gradients(tok64.float(), {k: v.float() for k, v in p64.items()}, g_tok)
    failed = []
    for k in MG.KEYS:
        bound = RATIO * float((ref32[k].double() - ref64[k]).abs().max()) + FLOOR * float(ref64[k].abs().max())
        a, b = grads["model1." + k].cpu().double(), want[k].cpu().double()
        diff = float((a - b).abs().max())
        msg = (f"{k:16s} equal {torch.equal(grads['model1.' + k], want[k])} | wm - mamba {diff:.3e}, wm - f64 {float((a - ref64[k]).abs().max()):.3e}, "
               f"bound {bound:.3e}")
        print(msg)
        if not (diff <= bound and float((a - ref64[k]).abs().max()) <= bound):
            failed.append(msg)
    assert not failed, "\n".join(failed)
