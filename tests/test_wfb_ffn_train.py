"""ops.wfb_feed_forward_train / ops.wfb_feed_forward_backward (csrc/rf_wfb_train.hip) against float64 autograd of the restatement
tests/wfb_ffn_grad_ref.py, which tests/golden/wfb_ffn_train.npz pins to the reference's own ``FeedForward`` in ``.train()``.

Loss: ``<y, g>`` with a fixed random ``g``; truth = the float64 restatement and ``torch.autograd.grad`` of it with respect to ``x`` and
the 12 parameters; e32 = the same computation in float32.  Inputs: ``wfb_ffn_grad_ref.inputs(tag)`` (``cases.params`` /
``cases.rnd``; BatchNorm weights of either sign, running_var in [0.5, 1.5], |rep_conv2.c.weight| in [0.5, 1), x in +-4, +-1 in
``shifted``); seed = 4700 + the case's place in the table.

Cases (B, dim, hidden, h, w), each the smallest shape that reaches its branch:

========================  ==========================================================================================================
two_px (1,4,8,1,2)        N = 2, the smallest training batch; scalar row paths
base (2,16,32,8,8)        float4 row paths; gram2 weight gradients
w_mod4_2 (2,16,40,6,10)   w % 4 == 2: the plain weight-gradient kernels, scalar row ends
odd (1,24,60,5,7)         odd sizes, partial 4 x 4 stencil tiles
ff48 (1,48,120,10,14)     the hidden width of the ``ff48`` golden case (cases.WFB_FF_CASES)
slabs (2,4,8,8,516)       2 x 129 = 258 tiles of 4 x 4 pixels: rf_wfb_ffn_nblk = 2 slabs per image and channel, and two images.
                          The smallest such plane with float4 rows and more than one row of tiles (8 x 512 has 256 tiles: one slab)
c256 (1,256,512,4,4)      level-3 channels of RawFormer-S, several channel tiles in the GEMMs
shifted (2,16,32,8,12)    project_in.bias = 8: every channel of u2 has |mean| >= 10 std, so E[u^2] - E[u]^2 in float32 loses v2
                          (asserted below from the float32 restatement's own hid).  u1 does NOT reach 10 std: the zero padding of
                          the 3x3 gives its border pixels other tap sums, so its std is of the order of its mean
========================  ==========================================================================================================

Bound, per tensor (``y``, the four batch statistics, the four updated running statistics, ``grad_x``, the 12 gradients): the scheme
of tests/test_mamba.py, whose RATIO and FLOOR are imported: e64 = max|hip - ref_f64| <= 8 e32 + 2e-6 S, S = max|ref_f64|.  One
exception, fixed in advance: d rep_conv2.c.weight in training mode.  BN(w2 hid) does not depend on the size of w2 except through
eps, so the exact gradient is of order eps while its summands are not; for that tensor alone S = max over channels of
sum |du2 hid| from the float64 reference.  The CPU test asserts max|ref_f64| <= 1e-3 S for it in every case but two_px: with N = 2,
uh = +-sqrt(v / (v + eps)) whatever the data, so du2 itself, not only its sum, carries the factor eps / (v + eps): summands and sum
shrink together, and their ratio is 1e-2 there (from the one channel whose v2 = 7e-5 is a few eps); the tensor keeps the same S.
For the same reason d rep_conv1.c.weight of two_px is small (1.9e-3) next to its neighbours; it keeps the plain bound.  No other
tensor cancels: every other tensor of every case has max|ref_f64| > 0 and is compared with the plain bound.  ``-s`` prints e64 / bound for every tensor of every case; DESIGN.md section 4,
"WFB FeedForward, training mode", holds the table measured on the MI355X: the largest e64 / bound per case is 0.09 .. 0.32
(two_px: d rep_conv1.c.weight; odd: v2); d rep_conv2.c.weight is at 0.008 .. 0.13 of its bound, v2 of ``shifted`` at 0.03.

Condition on the bound, shown on the CPU and asserted again at the head of each GPU test: each of wfb_ffn_grad_ref.GRAD_DEFECTS moves
at least one gradient tensor of every case by >= 100 x that tensor's bound, and ``biased_running`` moves a running variance by
>= 100 x its bound in every case but ``slabs`` (N = 8256: N / (N - 1) - 1 = 1.2e-4; 22 x and 11 x there): both of them in two_px, base,
w_mod4_2, odd, ff48 and c256, rep_conv1's in ``shifted`` (rep_conv2's by about 60 x: its variance is small at x in +-1).
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import cases
import wfb_ffn_grad_ref as G
from bayer_low_light_image_enhancement_amd import _lib, ops
from test_mamba import FLOOR, RATIO

CASES = {t: s for t, (s, _) in G.CASES.items()}
FWD = ("y",) + G.STATS + G.BUFFERS
NAMES = FWD + ("x",) + G.KEYS
RV = ("rep_conv1.bn.running_var", "rep_conv2.bn.running_var")
EVAL_CASES = ("base", "w_mod4_2", "c256")
NBT = ("rep_conv1.bn.num_batches_tracked", "rep_conv2.bn.num_batches_tracked")


@functools.lru_cache(maxsize=None)
def reference(tag, training=True):
    """Inputs, parameters, the float64 and float32 results, the bounds and what each defect moves: computed once, shared, never
    changed."""
    x, g, p = G.inputs(tag)
    p64 = {k: v.double() for k, v in p.items()}
    ref64, s_w2 = G.gradients(x.double(), p64, g.double(), training)
    ref32, _ = G.gradients(x, p, g, training)
    assert all(ref64[k].dtype == torch.float64 and ref32[k].dtype == torch.float32 for k in NAMES)
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in NAMES}
    mx = {k: float(ref64[k].abs().max()) for k in NAMES}
    scale = dict(mx)
    if training:                                             # d rep_conv2.c.weight is a sum that cancels: module docstring
        scale[G.W2] = s_w2
    bound = {k: RATIO * e32[k] + FLOOR * scale[k] for k in NAMES}
    moved = {}
    for d in G.DEFECTS if training else ():
        bad, _ = G.gradients(x.double(), p64, g.double(), defect=d)
        moved[d] = {k: float((bad[k] - ref64[k]).abs().max()) for k in NAMES}
    return {"x": x, "g": g, "p": p, "ref64": ref64, "ref32": ref32, "e32": e32, "max": mx, "scale": scale, "bound": bound, "moved": moved}


def assert_bound_sees_defects(tag):
    c = reference(tag)
    assert all(math.isfinite(c["max"][k]) and c["bound"][k] > 0 for k in NAMES)
    for d in G.GRAD_DEFECTS:
        ratio = {k: c["moved"][d][k] / c["bound"][k] for k in ("x",) + G.KEYS}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {c['moved'][d][best]:.3e} against the "
                                      f"bound {c['bound'][best]:.3e}): the case cannot see it")
        assert all(c["moved"][d][k] == 0.0 for k in FWD), (tag, d)      # a detach point changes the gradient, never the value
    ratio = {k: c["moved"]["biased_running"][k] / c["bound"][k] for k in RV}
    if tag == "shifted":                                     # rep_conv2's variance is small there (x in +-1, |w2| < 1): about 60 x
        assert max(ratio.values()) >= 100.0 and min(ratio.values()) >= 50.0, (tag, ratio)
    elif tag != "slabs":
        assert min(ratio.values()) >= 100.0, (tag, ratio)
    else:
        assert 10.0 <= min(ratio.values()) and max(ratio.values()) < 100.0, (tag, ratio)


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["base", "odd"])
def test_restatement_is_the_reference_module_in_train_mode(tag):
    """The float64 restatement against the reference's own FeedForward.train() (the fixture) to 1e-12 relative; the reference's
    own float32 run stays inside the bound the HIP operators get."""
    fix = cases.golden("wfb_ffn_train")
    c = reference(tag)
    for k in NAMES:
        key = "grad." + k if k in ("x",) + G.KEYS else k
        if k in G.STATS:                                  # the module does not expose its batch statistics
            continue
        want = torch.from_numpy(fix[f"{tag}.f64.{key}"])
        assert want.dtype == torch.float64 and tuple(want.shape) == tuple(c["ref64"][k].shape), (tag, k)
        diff = float((c["ref64"][k] - want).abs().max())
        assert diff <= 1e-12 * c["scale"][k], (tag, k, diff, c["scale"][k])
        ref32 = torch.from_numpy(fix[f"{tag}.f32.{key}"])
        assert ref32.dtype == torch.float32
        assert float((ref32.double() - c["ref64"][k]).abs().max()) <= c["bound"][k], (tag, k)
    for k in NBT:
        assert int(fix[f"{tag}.f64.{k}"]) == 1 and int(fix[f"{tag}.f32.{k}"]) == 1


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_cannot_hide_the_defects(tag):
    assert_bound_sees_defects(tag)


def test_cases_reach_the_branches_they_are_named_for():
    nblk = _lib.load().rf_wfb_ffn_nblk
    n = {t: s[0] * s[3] * s[4] for t, s in CASES.items()}
    assert n["two_px"] == 2 and CASES["two_px"][4] % 4 != 0
    assert [t for t in CASES if CASES[t][4] % 4 == 0] == ["base", "slabs", "c256", "shifted"]                 # float4 rows
    assert [t for t in CASES if (CASES[t][3] * CASES[t][4]) % 4 == 0] == ["base", "w_mod4_2", "ff48", "slabs", "c256", "shifted"]     # gram2<1>
    assert CASES["w_mod4_2"][4] % 4 == 2 and CASES["ff48"][4] % 4 == 2
    assert CASES["odd"][3] % 2 == 1 and CASES["odd"][4] % 2 == 1 and CASES["odd"][3] % 4 and CASES["odd"][4] % 4
    ff48 = next(c for c in cases.WFB_FF_CASES if c[0] == "ff48")
    assert CASES["ff48"][1:3] == (ff48[1], int(ff48[1] * ff48[2])) and CASES["ff48"][3:] == tuple(ff48[4:])
    assert CASES["c256"][1:3] == (256, 512)
    # slabs: more than one workgroup partial per image and channel, and several images; the planes one step smaller have one
    h, w = CASES["slabs"][3:]
    assert [nblk(*s[3:]) for s in CASES.values()] == [1, 1, 1, 1, 1, 2, 1, 1] and CASES["slabs"][0] == 2
    assert ((h + 3) // 4) * ((w + 3) // 4) == 258 and nblk(h, w - 4) == 1 and nblk(h - 4, w) == 1 and w % 4 == 0
    assert nblk(1024, 1024) == 32 and nblk(0, 4) == -22
    # shifted: |mean| >= 10 std in every channel of u2, and the one-pass float32 variance E[u^2] - E[u]^2 misses v2's bound there
    c = reference("shifted")
    assert bool((c["p"]["project_in.bias"] == G.SHIFT).all())
    with torch.no_grad():
        _, _, _, (hid, u2) = G.forward(c["x"], c["p"])
    assert u2.dtype == torch.float32
    mu2, v2 = c["ref64"]["mu2"], c["ref64"]["v2"]
    assert float((mu2.abs() / v2.sqrt()).min()) >= 10.0
    naive = (u2 * u2).mean(dim=(0, 2, 3)) - u2.mean(dim=(0, 2, 3)) ** 2
    assert float((naive.double() - v2).abs().max()) > c["bound"]["v2"], "the shifted case cannot see a cancelling variance"
    u1 = F.conv2d(hid, c["p"]["rep_conv1.c.weight"], None, padding=1, groups=hid.shape[1])
    assert float((c["ref64"]["mu1"].abs() / c["ref64"]["v1"].sqrt()).median()) < 10.0 and u1.shape == u2.shape      # (module docstring)
    # the exception of the bound is real: the sum cancels, its summands do not; nothing else cancels
    for t in CASES:
        r = reference(t)
        for k in NAMES:
            assert r["max"][k] > 0.0, (t, k)
            if k != G.W2:
                assert r["scale"][k] == r["max"][k]
        if t == "two_px":                                    # N = 2: du2 shrinks with its sum (module docstring)
            assert 1e-3 * r["scale"][G.W2] < r["max"][G.W2] <= 2e-2 * r["scale"][G.W2] and float(r["ref64"]["v2"].min()) < 1e-4
        else:
            assert r["max"][G.W2] <= 1e-3 * r["scale"][G.W2], (t, r["max"][G.W2], r["scale"][G.W2])
    for t in EVAL_CASES:                                     # in eval mode the statistics are constants: no cancellation, the plain bound
        r = reference(t, False)
        assert r["scale"][G.W2] == r["max"][G.W2] > 1e-3


def fake_call_args(good):
    b, dim, hidden, h, w = good
    lib = _lib.load()
    need_f, need_b = lib.rf_wfb_ffn_train_workspace_bytes(*good), lib.rf_wfb_ffn_backward_workspace_bytes(*good)
    assert need_f > 0 and need_b > need_f
    shapes = ops.wfb_ff_param_shapes(dim, hidden)
    assert list(shapes) == list(G.KEYS + G.BUFFERS)
    tensors = [4 * math.prod(s) for s in shapes.values()]
    plane = 4 * b * dim * h * w
    at = cases.fake_addresses([plane] * 3 + [max(need_f, need_b), 16 * hidden] + tensors + tensors[:12])
    return lib, need_f, need_b, at


def test_forward_host_checks_refuse_before_any_launch():
    good = (2, 16, 32, 8, 8)
    lib, need, _, at = fake_call_args(good)
    # never dereferenced: the checks come first.  Every buffer has an address of its own, of its true size, clear of the others
    x, _, out, ws, stats = (C.c_void_p(v) for v in at[:5])
    prm = (C.c_void_p * 16)(*at[5:21])
    call, err = lib.rf_wfb_ffn_train_forward, lib.rf_last_error
    rest = (1e-5, 0.1, 1, None)
    for bad, word in (((2, 18, 32, 8, 8), b"dim 18"), ((2, 16, 34, 8, 8), b"hidden 34"), ((0, 16, 32, 8, 8), b"B 0"), ((2, 16, 32, 0, 8), b"0 x 8"),
                      ((2, 16, 32, 8, -1), b"8 x -1"), ((1, 16, 32, 1, 1), b"B h w = 1")):
        assert lib.rf_wfb_ffn_train_workspace_bytes(*bad) == -22
        assert err().startswith(b"rf_wfb_ffn_train_workspace_bytes: ") and word in err(), err()
        assert call(x, out, prm, stats, ws, 1 << 40, *bad, *rest) == -22
        assert err().startswith(b"rf_wfb_ffn_train_forward: ") and word in err(), err()
    assert lib.rf_wfb_ffn_train_workspace_bytes(1, 4, 8, 1, 2) > 0
    assert call(x, out, prm, stats, ws, need - 1, *good, *rest) == -12
    assert err().startswith(b"rf_wfb_ffn_train_forward: workspace")
    for args in ((None, out, prm, stats, ws), (x, None, prm, stats, ws), (x, out, None, stats, ws), (x, out, prm, None, ws), (x, out, prm, stats, None),
                 (x, C.c_void_p(out.value + 4), prm, stats, ws), (x, out, prm, C.c_void_p(stats.value + 8), ws)):
        assert call(*args, 1 << 40, *good, *rest) == -22
        assert err().startswith(b"rf_wfb_ffn_train_forward: ") and b"aligned" in err()
    null_prm = (C.c_void_p * 16)(*prm)
    null_prm[13] = None
    assert call(x, out, null_prm, stats, ws, 1 << 40, *good, *rest) == -22 and b"13 is null" in err()

    def refused_as_alias(*args, update=1):
        assert call(*args, 1 << 40, *good, 1e-5, 0.1, update, None) == -22
        assert err().startswith(b"rf_wfb_ffn_train_forward: ") and b"alias" in err(), err()

    inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
    refused_as_alias(x, x, prm, stats, ws)                        # out on in
    refused_as_alias(x, inside(x, 64), prm, stats, ws)
    refused_as_alias(x, out, prm, inside(out, 16), ws)            # batch_stats inside out
    refused_as_alias(x, out, prm, stats, inside(x, 16))           # the workspace over in
    refused_as_alias(x, out, prm, stats, C.c_void_p(prm[3] - 256))      # ... over a parameter
    for i, target in ((12, prm[7]), (13, x.value + 32), (14, prm[15]), (15, ws.value + 4096), (12, stats.value)):
        bad = (C.c_void_p * 16)(*prm)
        bad[i] = target                                           # an updated buffer on a parameter, in, another buffer, the workspace, batch_stats
        refused_as_alias(x, out, bad, stats, ws)
    shared = (C.c_void_p * 16)(*prm)
    shared[12] = prm[7]                                           # without the update the buffers are inputs, and inputs may overlap
    assert call(x, out, shared, stats, ws, need - 1, *good, 1e-5, 0.1, 0, None) == -12
    refused_as_alias(x, out, prm, stats, C.c_void_p(prm[14] - 64), update=0)      # ... but nothing may be written over them


def test_backward_host_checks_refuse_before_any_launch():
    good = (2, 16, 32, 8, 8)
    lib, _, need, at = fake_call_args(good)
    x, g, dx, ws = (C.c_void_p(v) for v in at[:4])
    prm, grd = (C.c_void_p * 16)(*at[5:21]), (C.c_void_p * 12)(*at[21:33])
    call, err = lib.rf_wfb_ffn_backward, lib.rf_last_error
    for bad, word in (((2, 18, 32, 8, 8), b"dim 18"), ((2, 16, 34, 8, 8), b"hidden 34"), ((0, 16, 32, 8, 8), b"B 0"), ((2, 16, 32, 0, 8), b"0 x 8")):
        assert lib.rf_wfb_ffn_backward_workspace_bytes(*bad) == -22
        assert err().startswith(b"rf_wfb_ffn_backward_workspace_bytes: ") and word in err(), err()
        for training in (0, 1):
            assert call(x, g, dx, prm, grd, ws, 1 << 40, *bad, training, 1e-5, 0, None) == -22
            assert err().startswith(b"rf_wfb_ffn_backward: ") and word in err(), err()
    one = (1, 16, 32, 1, 1)                                       # one value per channel: the eval-mode gradient exists, the training-mode one does not
    assert lib.rf_wfb_ffn_backward_workspace_bytes(*one) > 0
    assert call(x, g, dx, prm, grd, ws, 1 << 40, *one, 1, 1e-5, 0, None) == -22 and b"B h w = 1" in err()
    assert call(x, g, dx, prm, grd, ws, 16, *one, 0, 1e-5, 0, None) == -12
    assert call(x, g, dx, prm, grd, ws, need - 1, *good, 1, 1e-5, 0, None) == -12
    assert err().startswith(b"rf_wfb_ffn_backward: workspace")
    assert call(x, g, None, prm, grd, ws, 1 << 40, *good, 1, 1e-5, 0, None) == -22 and err().startswith(b"rf_wfb_ffn_backward: ")
    assert call(x, g, C.c_void_p(dx.value + 4), prm, grd, ws, 1 << 40, *good, 1, 1e-5, 0, None) == -22 and b"aligned" in err()
    null_prm = (C.c_void_p * 16)(*prm)
    null_prm[14] = None
    assert call(x, g, dx, null_prm, grd, ws, 1 << 40, *good, 0, 1e-5, 0, None) == -22 and b"buffer 2 is null" in err()

    def refused_as_alias(*args):
        for training in (0, 1):
            assert call(*args, 1 << 40, *good, training, 1e-5, 0, None) == -22
            assert err().startswith(b"rf_wfb_ffn_backward: ") and b"alias" in err(), err()

    inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
    for trio in ((x, g, x), (x, g, g), (x, g, inside(g, 1024))):
        refused_as_alias(*trio, prm, grd, ws)
    refused_as_alias(x, g, dx, prm, grd, inside(x, 16))           # the workspace over in
    refused_as_alias(x, g, dx, prm, grd, inside(dx, 64))          # ... over grad_in
    refused_as_alias(x, g, dx, prm, grd, C.c_void_p(prm[15] - 256))      # ... over a running statistic
    for i, target in ((3, prm[5]), (0, dx.value), (2, grd[7]), (1, ws.value + 1024), (11, g.value + 32), (4, grd[5] - 16), (6, prm[13]), (9, prm[12] + 64)):
        bad = (C.c_void_p * 12)(*grd)
        bad[i] = target                                           # a gradient on a parameter, grad_in, another gradient, the workspace, a buffer, ...
        refused_as_alias(x, g, dx, prm, bad, ws)
    assert call(x, inside(x, 16), dx, prm, grd, ws, need - 1, *good, 1, 1e-5, 0, None) == -12


# ------------------------------------------------------------------------------------------ GPU
def on_device(c, device):
    p = {k: v.to(device) for k, v in c["p"].items()}
    p.update({k: torch.zeros((), dtype=torch.int64, device=device) for k in NBT})
    return p, c["x"].to(device), c["g"].to(device)


def compare(tag, c, got, names, failed):
    for k in names:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (tag, k)
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        msg = (f"[{tag}] {k:28s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} S {c['scale'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / c['bound'][k]:.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_float64_autograd(device, tag):
    assert_bound_sees_defects(tag)
    c = reference(tag)
    hidden = CASES[tag][2]
    failed = []
    # forward: the output, the batch statistics, the updated running statistics
    runs = []
    for _ in range(2):
        p, x, g = on_device(c, device)
        stats = torch.empty((4, hidden), device=device)
        y = ops.wfb_feed_forward_train(x, p, batch_stats=stats)
        assert all(int(p[k]) == 1 for k in NBT)
        runs.append({"y": y, **{k: stats[i] for i, k in enumerate(G.STATS)}, **{k: p[k] for k in G.BUFFERS}})
        assert torch.equal(x, c["x"].to(device)) and all(torch.equal(p[k], c["p"][k].to(device)) for k in G.KEYS), f"[{tag}] the forward wrote an input"
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in FWD), f"[{tag}] two forward runs differ"
    compare(tag, c, runs[0], FWD, failed)
    p, x, g = on_device(c, device)
    y = ops.wfb_feed_forward_train(x, p, update_running_stats=False)
    assert torch.equal(y, runs[0]["y"])
    assert all(torch.equal(p[k], c["p"][k].to(device)) for k in G.BUFFERS) and all(int(p[k]) == 0 for k in NBT), f"[{tag}] a buffer was written"
    # backward
    keep = {k: v.clone() for k, v in p.items()}
    dx, grads = ops.wfb_feed_forward_backward(x, p, g)
    dx2, grads2 = ops.wfb_feed_forward_backward(x, p, g)
    torch.cuda.synchronize()
    assert torch.equal(x, c["x"].to(device)) and torch.equal(g, c["g"].to(device)), f"[{tag}] an input was written"
    assert all(torch.equal(p[k], keep[k]) for k in p), f"[{tag}] a parameter or buffer was written"
    got, again = {"x": dx, **grads}, {"x": dx2, **grads2}
    assert set(got) == {"x"} | set(G.KEYS)
    assert all(torch.equal(got[k], again[k]) for k in got), f"[{tag}] two backward runs differ"
    compare(tag, c, got, ("x",) + G.KEYS, failed)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", EVAL_CASES)
def test_eval_mode_backward_matches_float64_autograd(device, tag):
    c = reference(tag, False)
    p, x, g = on_device(c, device)
    keep = {k: v.clone() for k, v in p.items()}
    dx, grads = ops.wfb_feed_forward_backward(x, p, g, training=False)
    dx2, grads2 = ops.wfb_feed_forward_backward(x, p, g, training=False)
    assert all(torch.equal(p[k], keep[k]) for k in p)
    got, again = {"x": dx, **grads}, {"x": dx2, **grads2}
    assert all(torch.equal(got[k], again[k]) for k in got), f"[{tag}] two runs differ"
    failed = []
    compare(tag, c, got, ("x",) + G.KEYS, failed)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["base", "w_mod4_2"])          # launch_gram2's accumulation and the plain kernels'
@pytest.mark.parametrize("training", [True, False])
def test_passing_grads_accumulates(device, tag, training):
    p, x, g = on_device(reference(tag), device)
    dx, grads = ops.wfb_feed_forward_backward(x, p, g, training=training)
    once = {k: v.clone() for k, v in grads.items()}
    dx2, same = ops.wfb_feed_forward_backward(x, p, g, grads=grads, training=training)
    assert same is grads and set(grads) == set(G.KEYS)
    assert torch.equal(dx, dx2), "grad_x is overwritten, never accumulated"
    for k in G.KEYS:
        assert torch.equal(grads[k], 2.0 * once[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["base", "odd"])
def test_eval_forward_on_the_batch_statistics_is_the_training_forward(device, tag):
    """With batch_stats copied into the running buffers, the eval-mode ops.wfb_feed_forward (the host's fold, dwgate_kernel) computes
    the function the training-mode forward computed: the two agree, and both meet float64, within the case's bound on y."""
    c = reference(tag)
    p, x, _ = on_device(c, device)
    stats = torch.empty((4, CASES[tag][2]), device=device)
    y = ops.wfb_feed_forward_train(x, p, update_running_stats=False, batch_stats=stats)
    for i, k in enumerate(G.BUFFERS):
        p[k] = stats[i].clone()
    y_eval = ops.wfb_feed_forward(x, p)
    d_train = float((y_eval - y).abs().max())
    d_ref = float((y_eval.cpu().double() - c["ref64"]["y"]).abs().max())
    print(f"[{tag}] eval on batch statistics: against the training forward {d_train:.3e}, against float64 {d_ref:.3e}, bound {c['bound']['y']:.3e}")
    assert d_train <= c["bound"]["y"] and d_ref <= c["bound"]["y"]
