"""conv1x1_b3_ln_kernel (rf_gemm1x1.hip) where a workgroup walks MORE than one pixel tile, through ops.conv1x1.

The kernel is persistent over the 64-pixel tiles of an image and carries loads across the tile boundary: the next tile's input,
and either the first ring steps of the next tile's weights or (K = 64 with one chunk of output tiles per wave) all of the wave's
weights for the life of the workgroup.  The cases of cases.CONV1X1_CASES give every workgroup ONE tile, so they never take the
second trip.  Each shape here is the smallest that reaches the state named; it follows from plan_conv1x1 (grid x =
min(slots / B, P / 64) with 512 resident workgroups at K <= 128 and 256 at K = 256), and the test asserts the plan it counts on.

Inputs as in cases.conv1x1_case: x scaled by 2 and shifted by 0.7, gamma in [0.5, 1.5], weights / sqrt(K).  Tolerance: the 2e-5
max-abs against the float64 composition that tests/test_conv1x1_plan.py applies to this family on these ranges.
"""
import functools

import numpy as np
import pytest
import torch

import cases
from test_conv1x1_plan import TOL, plan

# tag -> (K, Cout, B, h, w, key, grid at B, chunks of output tiles per wave, most tiles a workgroup takes)
CASES = {
    # one chunk per wave at K = 64: the weights stay in registers; 72 tiles on 64 workgroups per image
    "k64_o192_two_tiles": (64, 192, 8, 72, 64, "conv1x1_b3_ln_kernel<2, 3>", (64, 8, 1), 1, 2),
    "k64_o128_two_tiles": (64, 128, 8, 72, 64, "conv1x1_b3_ln_kernel<2, 2>", (64, 8, 1), 1, 2),
    # the same with a ragged last tile: P = 4624 = 72 * 64 + 16 (P % 64 != 0, P % 4 == 0), 73 tiles
    "k64_o192_ragged": (64, 192, 8, 68, 68, "conv1x1_b3_ln_kernel<2, 3>", (64, 8, 1), 1, 2),
    "k64_o128_ragged": (64, 128, 8, 68, 68, "conv1x1_b3_ln_kernel<2, 2>", (64, 8, 1), 1, 2),
    # two chunks per wave: the ring is refilled for the next chunk and, behind the last one, for the next tile
    "k128_o384_two_chunks": (128, 384, 8, 72, 64, "conv1x1_b3_ln_kernel<4, 3>", (64, 8, 1), 2, 2),
    "k128_o256_two_chunks": (128, 256, 8, 72, 64, "conv1x1_b3_ln_kernel<4, 2>", (64, 8, 1), 2, 2),
    "k64_o256_two_chunks": (64, 256, 8, 72, 64, "conv1x1_b3_ln_kernel<2, 2>", (64, 8, 1), 2, 2),
    # K = 256: 36 tiles on 32 workgroups per image; three and two chunks of four tiles
    "k256_o768_three_chunks": (256, 768, 8, 48, 48, "conv1x1_b3_ln_kernel<8, 4>", (32, 8, 1), 3, 2),
    "k256_o512_two_chunks": (256, 512, 8, 48, 48, "conv1x1_b3_ln_kernel<8, 4>", (32, 8, 1), 2, 2),
    # small launches split their output channels over blockIdx.z (the shapes of b3ln_*_zsplit): one chunk per wave, one tile
    "k128_o256_zsplit": (128, 256, 1, 16, 16, "conv1x1_b3_ln_kernel<4, 2>", (4, 1, 2), 1, 1),
    "k256_o384_zsplit": (256, 384, 1, 16, 16, "conv1x1_b3_ln_kernel<8, 3>", (4, 1, 2), 1, 1),
}


@functools.lru_cache(maxsize=None)
def inputs(tag):
    k, cout, b, h, w = CASES[tag][:5]
    return {"x": cases.rnd("p.x", (b, k, h, w)) * 2.0 + 0.7, "w": cases.rnd("p.w", (cout, k, 1, 1)) / np.sqrt(k), "bias": cases.rnd("p.b", (cout,)),
            "ln_w": cases.rnd("p.lw", (k,), 0.5, 1.5), "ln_b": cases.rnd("p.lb", (k,))}


@functools.lru_cache(maxsize=None)
def reference(tag):
    """float64 composition (``reference`` of tests/test_conv1x1_plan.py for a LayerNorm case), computed once per case."""
    k, cout, b, h, w = CASES[tag][:5]
    t = inputs(tag)
    x = t["x"].double()
    mu, var = x.mean(1, keepdim=True), x.var(1, keepdim=True, unbiased=False)
    x = (x - mu) / torch.sqrt(var + 1e-5) * t["ln_w"].double().reshape(1, -1, 1, 1) + t["ln_b"].double().reshape(1, -1, 1, 1)
    y = torch.einsum("ok,bkp->bop", t["w"].double().reshape(cout, k), x.reshape(b, k, h * w)).reshape(b, cout, h, w)
    return y + t["bias"].double().reshape(1, cout, 1, 1)


@pytest.mark.parametrize("tag", list(CASES))
def test_the_plan_puts_the_case_where_it_says(tag):
    k, cout, b, h, w, key, grid, chunks, trips = CASES[tag]
    got_key, got_grid = plan(k, 0, cout, b, h, w, "ln")[:2]
    assert (got_key, got_grid) == (key, grid)
    nco = int(key[-2])
    assert cout // 64 // grid[2] == chunks * nco, "output tiles per wave = chunks x NCO"
    tiles = (h * w + 63) // 64
    assert (tiles + grid[0] - 1) // grid[0] == trips, "most pixel tiles of a workgroup"
    if b > 1:       # the same image alone: every workgroup takes one tile
        assert plan(k, 0, cout, 1, h, w, "ln")[1][0] == tiles


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_persistent_trips_compute_what_single_trips_compute(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    k, cout, b, h, w, key = CASES[tag][:6]
    d = {n: v.to(device) for n, v in inputs(tag).items()}

    def run(x):
        return ops.conv1x1(x, d["w"], d["bias"], ln_weight=d["ln_w"], ln_bias=d["ln_b"])

    y, census = cases.census(lambda: run(d["x"]))
    assert [n for n in census if n.startswith("conv1x1_")] == [plan(k, 0, cout, b, h, w, "ln")[0]] == [key]
    e = float((y.cpu().double() - reference(tag)).abs().max())
    print(tag, "max-abs error against float64:", e)
    assert e <= TOL, (tag, e)
    assert torch.equal(run(d["x"]), y), "two runs differ"
    if b > 1:       # a tile's result does not depend on which trip of the persistent loop computed it
        assert torch.equal(run(d["x"][:1].contiguous()), y[:1]), "image 0 of the batch differs from the same image run alone"
