"""The attention projection inside the fused FFN kernel (level 0, C = 32, frames above 256 tiles of 4 x 64): the third form of
ffn_fused_kernel forms x1 = x + W_fold,b v + b_proj per halo'd tile instead of reading it, so run_stage launches no projection
GEMM there and x1 never reaches HBM.  The diagnostic twin's RF_NO_FUSE_PROJ=1 runs the two-launch form (projection GEMM, then
ffn_fused_kernel<32, true>) at any size.  Follows test_stage_tail_fused.py: a subprocess per form, the oracle on the CPU.

The census cases: the rule is cdiv(w, 64) * cdiv(h, 4) > 256 at level 0 (fused_ffn_proj_rule, the tall attention front's size
class).  Mosaic 2 x 272 x 1040 has 9 x 34 = 306 tiles at level 0 and is therefore ABOVE the rule, not below it: it must record the
new form like the large case.  The frame that stays on the two-launch path here is mosaic 2 x 224 x 1040 (9 x 28 = 252 tiles,
the same 8-pixel last tile column)."""
import functools

import numpy as np
import pytest
import torch

import cases
from test_stage_tail_fused import SEED, err, forward, oracle

LARGE = (2, 528, 656)     # level 0 is 264 x 328: 6 x 66 = 396 tiles, last tile column 8 px wide, persistent workgroups run several
ABOVE = (2, 272, 1040)    # level 0 is 136 x 520: 9 x 34 = 306 tiles > 256
BELOW = (2, 224, 1040)    # level 0 is 112 x 520: 9 x 28 = 252 tiles <= 256
NEW = "ffn_fused_kernel<32, true, proj>"
TAIL = "ffn_fused_kernel<32, true>"
PROJ_GEMM = "conv1x1_res_kernel<8, false, 2, true>"


def fold_row(co):
    """rf_common.h fold_row_perm32: the row of the permuted b3 fold that holds output channel co."""
    return 16 * ((co >> 2) & 1) + 4 * (co >> 3) + (co & 3)


def test_fold_row_permutation_matches_the_two_lane_maps():
    """Row 16 t + 4 a + r <-> channel 8 a + 4 t + r is a bijection on 0..31, and it is the one that needs no shuffle: the MFMA
    leaves lane (j, kq) with output rows 16 t + 4 kq + r in acc[t][.][r], ln_step_b3 wants channel 8 kq + s in xh[s], and
    proj_step_b3 adds acc[t][.][r] to xh[4 t + r]."""
    rows = {}
    for t in range(2):
        for a in range(4):
            for r in range(4):
                rows[16 * t + 4 * a + r] = 8 * a + 4 * t + r
    assert sorted(rows) == list(range(32)) and sorted(rows.values()) == list(range(32))
    assert all(fold_row(ch) == row for row, ch in rows.items())
    for kq in range(4):
        held = sorted(rows[16 * t + 4 * kq + r] for t in range(2) for r in range(4))      # what the MFMA leaves in lane (., kq)
        assert held == [8 * kq + s for s in range(8)]                                      # what ln_step_b3 reads there
        for t in range(2):
            for r in range(4):
                assert rows[16 * t + 4 * kq + r] == 8 * kq + (4 * t + r)                   # ... at xh[4 t + r]


@functools.lru_cache(maxsize=None)
def reference(variant):
    return oracle(variant, LARGE)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flca", "plain"])
def test_fused_projection_on_a_ragged_multi_tile_frame(device, tmp_path, variant):
    """Mosaic 2 x 528 x 656: 396 tiles per image, persistent workgroups run several, the last tile column is 8 pixels wide and
    the two images carry different attention folds and squeeze-excite gates.  Both forms against the oracle and against each
    other (test_stage_tail_fused.py's bounds: the same kernels at the same value scale); image 0 of the batch is bit-identical
    to image 0 run alone."""
    from bayer_low_light_image_enhancement_amd import build
    diag = build.build_diag_library()
    new = forward(tmp_path, "proj", variant, LARGE, {})
    two = forward(tmp_path, "two", variant, LARGE, {"RF_LIB_PATH": diag, "RF_NO_FUSE_PROJ": "1"})
    ref = reference(variant)
    e = {"new vs oracle": err(new["y"], ref), "two-launch vs oracle": err(two["y"], ref), "new vs two-launch": err(new["y"], two["y"])}
    print(e)
    assert e["new vs oracle"] <= 2e-5, e
    assert e["two-launch vs oracle"] <= 2e-5, e
    assert e["new vs two-launch"] <= 1e-5, e
    assert not np.array_equal(new["y"], two["y"]), "the switch changed nothing"
    assert np.array_equal(new["y"][:1], new["alone"]), err(new["y"][:1], new["alone"])


def launches_of(device, variant, shape):
    from bayer_low_light_image_enhancement_amd import RawFormer, synth
    kw = dict(variant=variant) if variant == "flca" else dict(variant="plain", branch_lrelu=True)
    m = RawFormer(dim=32, **kw)
    m.load_state_dict({**m.state_dict(), **cases.model_state(32, SEED, variant)}, strict=True)
    m = m.to(device).eval()
    x = torch.from_numpy(synth.bayer_mosaic(SEED, *shape)).to(device)
    with torch.no_grad():
        m(x)                                   # parameters packed, workspace allocated
        return cases.launches(lambda: m(x))[1]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flca", "plain"])
def test_census_follows_the_rule(device, variant):
    """Above the rule a forward records the new kernel at stages 1 and 7 and neither the tail form nor the projection GEMM's
    instantiation; below it, the parent's launches."""
    for shape in (LARGE, ABOVE):
        got = launches_of(device, variant, shape)
        assert (got.get(NEW, 0), got.get(TAIL, 0), got.get(PROJ_GEMM, 0)) == (2, 0, 0), (shape, sorted(got.items()))
    got = launches_of(device, variant, BELOW)
    assert (got.get(NEW, 0), got.get(TAIL, 0), got.get(PROJ_GEMM, 0)) == (0, 2, 2), (BELOW, sorted(got.items()))
