"""The stage tail inside the fused FFN kernel (level 0, C = 32): ffn_fused_kernel<32, true> writes
channel_reduce(cat(branch, x1 + ffn(x1))) = Wa' xs + Wb x1 + (Wb W2) g + (Wb b2 + b_cr) itself, so run_stage launches no
channel_reduce GEMM there.  The diagnostic twin's RF_NO_COMPOSE=1 runs the two-kernel form (fused FFN, then the GEMM)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

# one forward of the whole batch, and one of image 0 alone
CODE = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cases
from bayer_low_light_image_enhancement_amd import RawFormer, synth
dev = torch.device("cuda:0")
variant, seed, b, hm, wm = sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
kw = dict(variant=variant) if variant == "flca" else dict(variant="plain", branch_lrelu=True)
m = RawFormer(dim=32, **kw)
m.load_state_dict({**m.state_dict(), **cases.model_state(32, seed, variant)}, strict=True)
m = m.to(dev).eval()
x = torch.from_numpy(synth.bayer_mosaic(seed, b, hm, wm)).to(dev)
with torch.no_grad():
    y = m(x).cpu().numpy()
    alone = m(x[:1].contiguous()).cpu().numpy()
np.savez(sys.argv[2], y=y, alone=alone)
'''

SEED = 91
LARGE = (2, 272, 1040)    # level 0 is 136 x 520: 34 x 9 = 306 tiles > 256 workgroups per image, last tile column 8 px wide
SMALL = (1, 32, 48)       # level 0 is 16 x 24: one partial tile


def forward(tmp_path, tag, variant, shape, env):
    out = str(tmp_path / f"{tag}.npz")
    e = dict(os.environ)
    e.pop("RF_LIB_PATH", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CODE, cases.REPO, out, variant, str(SEED), *map(str, shape)], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def both_forms(tmp_path, variant, shape):
    from bayer_low_light_image_enhancement_amd import build
    diag = build.build_diag_library()
    return (forward(tmp_path, "fused", variant, shape, {}),
            forward(tmp_path, "two", variant, shape, {"RF_LIB_PATH": diag, "RF_NO_COMPOSE": "1"}))


def oracle(variant, shape):
    from bayer_low_light_image_enhancement_amd import synth
    sd = cases.model_state(32, SEED, variant)
    cfg = R.RawFormerConfig(dim=32, variant=variant, branch_lrelu=True)
    with torch.no_grad():
        return R.rawformer_forward(sd, torch.from_numpy(synth.bayer_mosaic(SEED, *shape)), cfg).numpy()


def err(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def check_forms(fused, two, ref):
    e = {"fused vs oracle": err(fused, ref), "two-kernel vs oracle": err(two, ref), "fused vs two-kernel": err(fused, two)}
    print(e)
    assert e["fused vs oracle"] <= 2e-5, e
    assert e["two-kernel vs oracle"] <= 2e-5, e
    assert e["fused vs two-kernel"] <= 1e-5, e
    assert not np.array_equal(fused, two), "the switch changed nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flca", "plain"])
def test_fused_tail_on_a_ragged_multi_tile_frame(device, tmp_path, variant):
    """Mosaic 2 x 272 x 1040: some persistent workgroups run two tiles, the last tile column is 8 pixels wide and the two images
    carry different squeeze-excite gates.  Both forms against the oracle and against each other; image 0 of the batch is
    bit-identical to image 0 run alone (per-image weights; no state crosses images or depends on the tile-to-workgroup map)."""
    fused, two = both_forms(tmp_path, variant, LARGE)
    check_forms(fused["y"], two["y"], oracle(variant, LARGE))
    assert np.array_equal(fused["y"][:1], fused["alone"]), err(fused["y"][:1], fused["alone"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flca", "plain"])
def test_fused_tail_on_a_single_partial_tile(device, tmp_path, variant):
    """Mosaic 1 x 32 x 48: level 0 is 16 x 24, every tile is 24 < 64 pixels wide."""
    fused, two = both_forms(tmp_path, variant, SMALL)
    check_forms(fused["y"], two["y"], oracle(variant, SMALL))
    assert np.array_equal(fused["y"], fused["alone"])


@pytest.mark.parametrize("variant,dim", [("flca", 32), ("plain", 32), ("flca", 16)])
def test_workspace_plan_still_covers_the_fold_slot(variant, dim):
    """The kernel reads [Wa' | Wb | Wb W2] (packed 1x1 form, K = 4C) from the workspace slot of the channel_reduce fold, which the
    plan sizes for the widest level (K = 2 * 8 dim, Cout = 8 dim): 16 x what the tail level needs.  The plan's size is therefore
    what it was (test_abi.py pins the numbers); here: it is positive and grows with the batch at the shapes of this file, and no
    entry point was added to the ABI for the tail."""
    lib = _lib.load()
    cfg = _lib.RfConfig(dim, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, 2, {"flca": _lib.RF_VARIANT_FLCA, "plain": _lib.RF_VARIANT_PLAIN}[variant], 1, 0)
    h = C.c_void_p()
    assert lib.rf_create(C.byref(cfg), C.byref(h)) == 0
    try:
        one, two = C.c_size_t(), C.c_size_t()
        for hh, ww in ((136, 520), (16, 24)):
            assert lib.rf_workspace_bytes(h, 1, hh, ww, C.byref(one)) == 0 and one.value > 0
            assert lib.rf_workspace_bytes(h, 2, hh, ww, C.byref(two)) == 0 and two.value > one.value
            tail_level = {32: 0, 16: 1}[dim]
            c_tail, c_top = dim << tail_level, dim << 3
            need = (4 * c_tail // 4) * (c_tail // 16) * 64      # packed1x1_floats(2C + hidden, C), hidden = 2C
            slot = (2 * c_top // 4) * (c_top // 16) * 64        # packed1x1_floats(2 * 8 dim, 8 dim)
            assert need <= slot
    finally:
        lib.rf_destroy(h)
    # rf_ml_tail is the multi-level variant's output tail (colour anchor and luminance nudge on the image), not the stage tail
    assert not [n for n in _lib.SIGNATURES if "tail" in n and n != "rf_ml_tail"]
