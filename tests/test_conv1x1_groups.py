"""The bf16x3 1x1 GEMM without LayerNorm when its output groups share the input they fetch (conv1x1_b3_kernel<NCO, false, true>,
rf_gemm1x1.hip): two output groups per 512-thread workgroup, the pairs of a pixel tile 8 workgroup ids apart.

launch_conv1x1 takes that form only for launches that still give every CU a workgroup, so the small shapes here reach it through
the diagnostic twin: RF_B3_PAIR=1 takes the paired form at any size, RF_B3_PAIR=0 never does, RF_NO_B3=1 runs the f32 MFMA kernels.
One worker process per form computes every case once; the tests share the three results.  One large case goes through the
shipped library's own dispatch.  Every call is bracketed by the library's profiler, whose key names the form the launch took
(conv1x1_b3_kernel<NCO, false, true> is the paired one): bit-equal results alone could not tell whether the switch was honoured.

Tolerance: that of tests/test_gpu_ops.py::test_conv1x1 (max-abs 2e-5, same input ranges, weights / sqrt(K)) against the float64
product; the paired and the unpaired form must agree bit for bit (same k order, same six-term chains, same epilogue).

A third source exists only behind run_stage, whose C3 is the FFN's hidden width (a multiple of 32): the whole-model case runs
K = [C ; C ; 2C] at C = 128 and 256 with per-image weights.  The ragged last K block that a last source of 40 channels gives
(channel loads clamped to the source's last channel against zero weight pieces, in both halves of a pair) runs with two sources:
(C1, C2) = (128, 40) and (64, 104), K = 168 = 5 blocks of 32 and one of 8.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from cases import rnd
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

TOL = 2e-5   # tests/test_gpu_ops.py: TOL of test_conv1x1

# (C1, C2, Cout): output tiles NT = Cout / 16 -> tiles per group NCO -> groups
SHAPES = [(128, 0, 128),    # NT 8, NCO 4: two groups = one pair
          (128, 0, 256),    # NT 16, NCO 4: four groups = two pairs, 8 ids apart
          (128, 0, 160),    # NT 10, NCO 6: two groups, the second ragged (4 tiles of 6)
          (128, 0, 224),    # NT 14, NCO 6: three groups (6, 6, 2): odd count, the last pair's second half idle
          (128, 0, 512),    # NT 32, NCO 4: eight groups = four pairs
          (64, 64, 128),    # two sources, cut at a multiple of 32 channels
          (128, 40, 128),   # K = 168: the last K block holds 8 channels of the second source, the other 24 are clamped loads
          (64, 104, 256)]   # the same tail behind a second source that spans four K blocks; four groups
# (B, h, w): one full pixel tile; 400 pixels (second tile: one full, one partial and two dead waves); 11 tiles (a whole chunk of 8
# units and a tail of 3); three images (the flat grid crosses image boundaries inside a chunk)
FRAMES = [(1, 16, 16), (3, 16, 16), (1, 20, 20), (3, 20, 20), (1, 44, 64)]
MODEL_SEED, MODEL_SHAPE = 77, (2, 256, 128)      # the model of test_composed_stage_tail_agrees_with_the_two_gemm_form
LARGE = (128, 0, 128, 3, 148, 148)               # 86 pixel tiles x 3 images = 258 units >= 256: paired by launch_conv1x1 itself


def inputs(c1, c2, cout, b, h, w):
    k = c1 + c2
    x = rnd("g.x", (b, c1, h, w))
    x2 = rnd("g.x2", (b, c2, h, w)) if c2 else None
    wt = rnd("g.w", (cout, k, 1, 1), -1, 1) / np.sqrt(k)
    return x, x2, wt, rnd("g.b", (cout,)), rnd("g.res", (b, cout, h, w))


def tag(c1, c2, cout, b, h, w, res):
    return f"k{c1}_{c2}_o{cout}_b{b}_{h}x{w}_{'res' if res else 'bias'}"


WORKER = r'''
import ctypes, json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cases, test_conv1x1_groups as T
from bayer_low_light_image_enhancement_amd import _lib, ops, RawFormer, synth
dev = torch.device("cuda:0")
out, keys = {}, {}
def gemm_keys(fn):      # (result, profiler keys of the GEMM kernels the call launched)
    torch.cuda.synchronize()
    _lib.load().rf_profile_begin()
    y = fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(_lib.load().rf_profile_end(buf, len(buf)), "rf_profile_end")
    return y, sorted({r["kernel"] for r in json.loads(buf.value.decode()) if r["kernel"].startswith("conv1x1_")})
for c1, c2, cout in T.SHAPES:
    for b, h, w in T.FRAMES:
        x, x2, wt, bias, res = (None if t is None else t.to(dev) for t in T.inputs(c1, c2, cout, b, h, w))
        for r in (None, res):
            y, k = gemm_keys(lambda: ops.conv1x1(x, wt, bias if r is None else None, x2=x2, residual=r))
            keys[T.tag(c1, c2, cout, b, h, w, r is not None)] = k
            again = ops.conv1x1(x, wt, bias if r is None else None, x2=x2, residual=r)
            assert torch.equal(y, again), ("two calls differ", c1, c2, cout, b, h, w)
            out[T.tag(c1, c2, cout, b, h, w, r is not None)] = y.cpu().numpy()
if sys.argv[3] == "model":
    m = RawFormer(dim=32, variant="flca")
    m.load_state_dict({**m.state_dict(), **cases.model_state(32, T.MODEL_SEED, "flca")}, strict=True)
    m = m.to(dev).eval()
    x = torch.from_numpy(synth.bayer_mosaic(T.MODEL_SEED, *T.MODEL_SHAPE)).to(dev)
    with torch.no_grad():
        y, keys["model"] = gemm_keys(lambda: m(x))
        out["model"] = y.cpu().numpy()
    c1, c2, cout, b, h, w = T.LARGE
    x, x2, wt, bias, res = (None if t is None else t.to(dev) for t in T.inputs(*T.LARGE))
    y, keys["large"] = gemm_keys(lambda: ops.conv1x1(x, wt, None, residual=res))
    out["large"] = y.cpu().numpy()
np.savez(sys.argv[2], keys=np.array(json.dumps(keys)), **out)
'''


@pytest.fixture(scope="module")
def forms(device, tmp_path_factory):
    """Every case on the paired form, the unpaired form and the f32 kernels of the diagnostic twin."""
    from bayer_low_light_image_enhancement_amd import build
    diag = build.build_diag_library()
    tmp = tmp_path_factory.mktemp("conv1x1_groups")
    res = {}
    for name, env, what in (("pair", {"RF_B3_PAIR": "1"}, "model"), ("single", {"RF_B3_PAIR": "0"}, "model"), ("f32", {"RF_NO_B3": "1"}, "ops")):
        path = str(tmp / f"{name}.npz")
        r = subprocess.run([sys.executable, "-c", WORKER, cases.REPO, path, what], env=dict(os.environ, RF_LIB_PATH=diag, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        z = np.load(path)
        res[name] = {k: z[k] for k in z.files if k != "keys"}
        res[name]["keys"] = json.loads(str(z["keys"]))
    return res


def paired(keys):
    return [k for k in keys if k.startswith("conv1x1_b3_kernel<") and k.endswith(", false, true>")]


def unpaired(keys):
    return [k for k in keys if k.startswith("conv1x1_b3_kernel<") and not k.endswith(", false, true>")]


def err(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("c1,c2,cout", SHAPES)
def test_paired_form_against_float64_the_f32_kernels_and_the_unpaired_form(forms, c1, c2, cout):
    for b, h, w in FRAMES:
        x, x2, wt, bias, res = inputs(c1, c2, cout, b, h, w)
        xin = x if x2 is None else torch.cat([x, x2], 1)
        prod = torch.einsum("ok,bkp->bop", wt.double().reshape(cout, c1 + c2), xin.double().reshape(b, c1 + c2, h * w)).reshape(b, cout, h, w)
        for with_res in (False, True):
            ref = (prod + (res.double() if with_res else bias.double().reshape(1, cout, 1, 1))).numpy()
            t = tag(c1, c2, cout, b, h, w, with_res)
            pair, single, f32 = forms["pair"][t], forms["single"][t], forms["f32"][t]
            kp, ks, kf = (forms[n]["keys"][t] for n in ("pair", "single", "f32"))
            nco = 6 if cout in (160, 224) else 4
            assert kp == [f"conv1x1_b3_kernel<{nco}, false, true>"], (t, kp)       # the switch took the paired kernel ...
            assert len(ks) == 1 and unpaired(ks) == ks, (t, ks)                      # ... and the unpaired one
            assert not [k for k in kf if "b3" in k], (t, kf)                           # f32 MFMA kernels only
            e = {"pair vs float64": err(pair, ref), "unpaired vs float64": err(single, ref), "pair vs f32 kernels": err(pair, f32)}
            print(t, e)
            assert e["pair vs float64"] <= TOL, (t, e)
            assert e["pair vs f32 kernels"] <= TOL, (t, e)
            assert np.array_equal(pair, single), (t, "paired and unpaired forms differ", err(pair, single))


@pytest.mark.gpu
def test_whole_model_with_per_image_weights_and_three_sources(forms):
    """FLCA model, dim 32, two images with different gates: the attention apply (K = Cout = C, residual, per-image folded weights)
    and the composed stage tail (three sources [xs ; x1 ; g], per-image weights) at C = 128 (two groups) and C = 256 (four).
    A wrong image offset in either half of a pair moves whole output groups of image 1 away from the unpaired form's."""
    from bayer_low_light_image_enhancement_amd import synth
    pair, single = forms["pair"], forms["single"]
    assert paired(pair["keys"]["model"]) == ["conv1x1_b3_kernel<4, false, true>"], pair["keys"]["model"]
    assert not paired(single["keys"]["model"]) and unpaired(single["keys"]["model"]), single["keys"]["model"]
    assert np.array_equal(pair["model"], single["model"]), err(pair["model"], single["model"])
    sd = cases.model_state(32, MODEL_SEED, "flca")
    with torch.no_grad():
        ref = R.rawformer_forward(sd, torch.from_numpy(synth.bayer_mosaic(MODEL_SEED, *MODEL_SHAPE)), R.RawFormerConfig(dim=32, variant="flca", branch_lrelu=True)).numpy()
    e = err(pair["model"], ref)
    print("model, paired form vs oracle", e)
    assert e <= TOL, e


@pytest.mark.gpu
def test_large_launch_takes_the_paired_form_by_itself(forms, device):
    """258 units of two groups: the shipped library's dispatch pairs them.  Same bits as the diagnostic twin's two forms."""
    import ctypes
    from bayer_low_light_image_enhancement_amd import ops
    c1, c2, cout, b, h, w = LARGE
    x, _, wt, _, res = inputs(*LARGE)
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.rf_profile_begin()
    y = ops.conv1x1(x.to(device), wt.to(device), None, residual=res.to(device)).cpu().numpy()
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(lib.rf_profile_end(buf, len(buf)), "rf_profile_end")
    assert "conv1x1_b3_kernel<4, false, true>" in [r["kernel"] for r in json.loads(buf.value.decode())]
    assert paired(forms["pair"]["keys"]["large"]) and not paired(forms["single"]["keys"]["large"])
    ref = (torch.einsum("ok,bkp->bop", wt.double().reshape(cout, c1), x.double().reshape(b, c1, h * w)).reshape(b, cout, h, w) + res.double()).numpy()
    print("large", err(y, ref))
    assert err(y, ref) <= TOL
    assert np.array_equal(y, forms["pair"]["large"]) and np.array_equal(y, forms["single"]["large"])


@pytest.mark.parametrize("ngroups", [1, 2, 3, 4, 6, 8])
def test_group_map_is_one_to_one_and_keeps_a_units_groups_eight_ids_apart(ngroups):
    """Host function, no GPU.  Ids [0, units * ngroups) alone cannot put the groups of every unit on one id % 8 (one unit, two
    groups: ids 0 and 1), so the grid is whole chunks of 8 units and the ids of the missing units carry no work."""
    lib = _lib.load()
    for units in range(1, 41):
        n, u, g = C.c_int(), C.c_int(), C.c_int()
        assert lib.rf_conv1x1_group_grid(units, ngroups, C.byref(n)) == 0
        assert n.value == (units + 7) // 8 * 8 * ngroups and n.value - units * ngroups <= 7 * ngroups
        ids = {}
        for i in range(n.value):
            assert lib.rf_conv1x1_group_map(units, ngroups, i, C.byref(u), C.byref(g)) == 0
            if u.value < 0:
                assert g.value < 0
                continue
            assert 0 <= u.value < units and 0 <= g.value < ngroups
            assert (u.value, g.value) not in ids, "two ids for one (unit, group)"
            ids[(u.value, g.value)] = i
        assert len(ids) == units * ngroups                       # onto: every pair has its id
        for unit in range(units):
            mine = [ids[(unit, k)] for k in range(ngroups)]
            assert len({i % 8 for i in mine}) == 1               # one XCD
            assert all(b - a == 8 for a, b in zip(mine, mine[1:]))   # neighbours in that XCD's dispatch order
        assert lib.rf_conv1x1_group_map(units, ngroups, n.value, C.byref(u), C.byref(g)) == -22
