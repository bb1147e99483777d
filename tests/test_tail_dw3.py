"""The composed stage tail with the FFN's depthwise 3x3 + GELU inside the GEMM (conv1x1_b3_dw3_kernel, rf_gemm1x1_dw3.hip): where
plan_conv1x1 takes that form, run_stage launches no dwconv3x3 for the stage and the GEMM over [xs ; x1 ; hidden] stencils and
activates the hidden source as it reads it.  The diagnostic twin's RF_TAIL_DW=1 takes the form at any launch size the kernel
supports, RF_TAIL_DW=0 never; the shipped library takes it from 512 pixel tiles up (cfg2 level 1).

The two forms run the same fmaf chains in the same order, so their outputs are compared bit for bit."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

NEW_KEY = "conv1x1_b3_kernel<4, false, dw3>"

# Both forms in ONE child on the diagnostic twin (plan_conv1x1 reads the switch at every call): per form a profiled forward of the
# whole batch, whose launch census goes with the result, and for the new form one of image 0 alone
CODE = r'''
import json, os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cases
from bayer_low_light_image_enhancement_amd import RawFormer, synth
dev = torch.device("cuda:0")
variant, dim, seed, b, hm, wm = sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8])
kw = dict(variant=variant) if variant == "flca" else dict(variant="plain", branch_lrelu=True)
m = RawFormer(dim=dim, **kw)
m.load_state_dict({**m.state_dict(), **cases.model_state(dim, seed, variant)}, strict=True)
m = m.to(dev).eval()
x = torch.from_numpy(synth.bayer_mosaic(seed, b, hm, wm)).to(dev)
out = {}
with torch.no_grad():
    for form in "10":
        os.environ["RF_TAIL_DW"] = form
        y, census = cases.census(lambda: m(x).cpu().numpy())
        out["y" + form] = y
        out["census" + form] = np.array(json.dumps({k: v[0] for k, v in census.items()}))
        if form == "1":
            out["alone"] = m(x[:1].contiguous()).cpu().numpy()
np.savez(sys.argv[2], **out)
'''

SEED = 93
# (variant, dim, B, mosaic rows, mosaic columns).  dim 32: level 1 is C = 64 at 8 x 128 -- two tile rows and two tile columns of
# 4 x 64, so the image border on all four sides and a seam in both directions -- and the two images carry different gates.
# dim 64: level 0 is C = 64 at 16 x 128 and takes the form; level 1 (C = 128) has two output groups and must not.
CASES = {"flca_d32": ("flca", 32, 2, 32, 512), "plain_d32": ("plain", 32, 2, 32, 512), "flca_d64": ("flca", 64, 1, 32, 256)}
STAGES = 2      # stages of the affected level: its encoder and its decoder stage


def both_forms(tmp_path, case):
    from bayer_low_light_image_enhancement_amd import build
    variant, dim, *shape = CASES[case]
    out = str(tmp_path / "forms.npz")
    e = dict(os.environ)
    e.update({"RF_LIB_PATH": build.build_diag_library()})
    r = subprocess.run([sys.executable, "-c", CODE, cases.REPO, out, variant, str(dim), str(SEED), *map(str, shape)], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    return z["y1"], z["alone"], json.loads(str(z["census1"])), z["y0"], json.loads(str(z["census0"]))


def oracle(case):
    from bayer_low_light_image_enhancement_amd import synth
    variant, dim, *shape = CASES[case]
    sd = cases.model_state(dim, SEED, variant)
    cfg = R.RawFormerConfig(dim=dim, variant=variant, branch_lrelu=True)
    with torch.no_grad():
        return R.rawformer_forward(sd, torch.from_numpy(synth.bayer_mosaic(SEED, *shape)), cfg).numpy()


def err(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def dw_launches(census):
    return sum(n for k, n in census.items() if k.startswith("dwconv3x3"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_stencil_inside_the_tail_gemm(device, tmp_path, case):
    y1, alone1, c1, y0, c0 = both_forms(tmp_path, case)
    ref = oracle(case)
    e = {"on the fly vs oracle": err(y1, ref), "two kernels vs oracle": err(y0, ref), "on the fly vs two kernels": err(y1, y0)}
    print(case, e, {k: v for k, v in c1.items() if k == NEW_KEY or k.startswith("dwconv3x3")},
          {k: v for k, v in c0.items() if k.startswith("dwconv3x3")})
    # the switch did something: the depthwise launches of the affected stages are gone and the new kernel ran in their place ...
    assert NEW_KEY not in c0 and c1.get(NEW_KEY) == STAGES, (c0, c1)
    assert dw_launches(c0) - dw_launches(c1) == STAGES, (c0, c1)
    # ... at that level only: every other GEMM of the stage tails kept its kernel
    gemm = {k for c in (c0, c1) for k in c if k.startswith("conv1x1_") and k != NEW_KEY}
    moved = {k: c0.get(k, 0) - c1.get(k, 0) for k in gemm if c0.get(k, 0) != c1.get(k, 0)}
    assert list(moved.values()) == [STAGES] and next(iter(moved)).startswith("conv1x1_b3_kernel<"), (moved, c0, c1)
    assert np.array_equal(y1, y0), e                      # the same chains in the same order
    assert e["on the fly vs oracle"] <= 2e-5 and e["two kernels vs oracle"] <= 2e-5, e
    assert np.array_equal(y1[:1], alone1), err(y1[:1], alone1)


def plan(b, c, hc, h, w):
    """rf_conv1x1_dw3_plan: (key, grid, block, takes the form), or None where the three-source GEMM has no plan at all."""
    key, grid, block, fly = C.create_string_buffer(64), (C.c_int * 3)(), C.c_int(), C.c_int()
    if _lib.load().rf_conv1x1_dw3_plan(b, c, hc, h, w, key, len(key), grid, C.byref(block), C.byref(fly)) != 0:
        return None
    return key.value.decode(), tuple(grid), block.value, bool(fly.value)


def test_plan_rule():
    """The shipped library: the form is taken by one output group of four tiles on 4 x 64 workgroups from 512 pixel tiles up."""
    assert plan(8, 64, 128, 256, 256) == (NEW_KEY, (256, 8, 1), 256, True)                # cfg2 level 1: 2048 tiles
    assert plan(8, 128, 256, 128, 128) == ("conv1x1_b3_kernel<4, false, true>", (512, 1, 1), 512, False)      # cfg2 level 2: two groups, paired
    assert plan(2, 64, 128, 256, 256)[3] and not plan(1, 64, 128, 256, 256)[3]           # 512 tiles | 256 (frame1 level 1)
    assert not plan(8, 64, 128, 256, 72)[3] and not plan(8, 64, 128, 254, 256)[3]          # w % 64, h % 4
    assert not plan(8, 32, 64, 512, 512)[3] and not plan(8, 96, 192, 256, 256)[3]          # Cout = 32 (two tiles), 96 (six)
    assert plan(8, 64, 256, 256, 256)[3] and not plan(8, 64, 288, 256, 256)[3]             # hidden <= 256: its taps sit in LDS
    # no shape of the launch-census fixture reaches it (tests/golden/forward_launches.json stays what it is)
    for tag, (variant, dim, kw, b, hh, ww, stage) in cases.LAUNCH_CASES.items():
        for lvl in range(4):
            c = dim << lvl
            p = plan(b, c, c * kw.get("ffn_expansion_factor", 2), hh >> lvl, ww >> lvl)
            assert p is None or not p[3], (tag, lvl, p)
