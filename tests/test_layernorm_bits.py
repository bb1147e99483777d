"""The bits of every kernel with a per-pixel LayerNorm over channels or the exact Haar pair (csrc/rf_layernorm.h, haar_analysis /
haar_synthesis of csrc/rf_common.h, tok_row_stats of csrc/rf_mamba.h) against tests/golden/layernorm_parent.json: recorded on an
MI355X with tools/record_layernorm_golden.py at the commit before the kernels were put on those pieces.  Such a change keeps every
sum in its order: no bit may move, and there is no tolerance.  ``record`` is that of tests/test_train_bits.py, the inputs come from
``cases.rnd`` and the builders of the tests named below.  The smallest shapes that reach each form:

======================  =============================================================================================================
ln.c<C>                 ops.layernorm2d, (1, C, 2, 4) with bias at each of the ten channel counts of the register-resident kernel
ln.nobias.<shape>       ... without bias (the mean stays in the numerator): (1, 16, 2, 4) register-resident, (1, 24, 5, 7) generic
ln.walk4 / ln.walk1     (1, 24, 3, 4): layernorm2d_kernel<4>; (1, 24, 5, 7): <1>
ln.trips                (64, 16, 92, 92): 2116 groups of 4 pixels on a grid capped at 32 workgroups of 64 groups: a second, partial trip
lnb.<case>[.res]        ops.layernorm2d_backward at wmb_grad_ref.LN_CASES, with and without ``residual``: ln_bwd_reg_kernel (C = 16)
                        and ln_bwd_kernel + ln_wgrad_kernel (C = 24)
lnb.c<C>                ... (1, C, 2, 4) per channel count of the table
lnb.accumulate          (2, 16, 8, 8) once more into the ``grads`` of the first call
lnb.trips               (64, 16, 68, 64): 1088 groups on 16 workgroups of 64: a second trip
wmb.<shape>             ops.wmb_front / wmb_back / wmb_ffn_tail at test_wmb_kernels.SHAPES
front_bwd.<case>        ops.wmb_front_backward at every row of wmb_grad_ref.BAND_CASES (``trips`` included), grad_scale 2, then once more
                        into the returned ``grads``
back_bwd.<case>         ops.wmb_back_backward at wmb_grad_ref.BACK_CASES
wm.<case>               ops.wm and ops.wm_backward at one_pixel, odd (c = 24, L = 35: no multiples of 32), c512 and c32_L130 of
                        tests/test_wm_backward.py: tok_transpose_kernel<true> and wm_ln_bwd_kernel; the gradients in key order
haar.init               ops.dwt_init / ops.iwt_init, (1, 3, 6, 8) for the vector form and (1, 3, 6, 6) for the scalar form
haar.custom             the non-exact branch, which must not move either: ops.custom_dwt / custom_idwt at the same two shapes (CustomDWT
                        refuses odd sizes) and ops.haar_dwt at (1, 3, 5, 7), the reflect padding
======================  =============================================================================================================
"""
import json
import os

import pytest
import torch

import cases
import test_wm_backward as WB
import test_wmb_kernels as WK
import wmb_grad_ref as G
from test_mamba import wm_params
from test_train_bits import record

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layernorm_parent.json")
SEED = 7100
TABLE = (16, 32, 48, 64, 96, 128, 192, 256, 384, 512)      # C = CPL * KS of the register-resident kernels
WM_TAGS = ("one_pixel", "odd", "c512", "c32_L130")
LN_TRIPS, LNB_TRIPS = (64, 16, 92, 92), (64, 16, 68, 64)


def tag_of(shape):
    return "x".join(str(v) for v in shape)


def host(**arrays):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in arrays.items()}


def ln_inputs(shape, what="ln"):
    c = shape[1]
    return (cases.rnd(f"lnbits.{what}.x.{shape}", shape, -2.0, 2.0, seed=SEED), cases.rnd(f"lnbits.{what}.w.{c}", (c,), 0.5, 1.5, seed=SEED),
            cases.rnd(f"lnbits.{what}.b.{c}", (c,), -0.5, 0.5, seed=SEED))


def run_ln(device, shape, bias=True):
    from bayer_low_light_image_enhancement_amd import ops
    x, w, b = ln_inputs(shape)
    return host(out=ops.layernorm2d(x.to(device), w.to(device), b.to(device) if bias else None))


def lnb_out(gx, g):
    return {"x": gx, "weight": g["weight"], "bias": g["bias"]}


def run_lnb_case(device, tag, residual):
    from bayer_low_light_image_enhancement_amd import ops
    i = {k: v.to(device) for k, v in G.ln_inputs(tag).items()}
    return host(**lnb_out(*ops.layernorm2d_backward(i["x"], i["weight"], i["grad_out"], residual=i["residual"] if residual else None)))


def run_lnb_shape(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    x, w, _ = ln_inputs(shape, "lnb")
    g = cases.rnd(f"lnbits.lnb.g.{shape}", shape, seed=SEED)
    return host(**lnb_out(*ops.layernorm2d_backward(x.to(device), w.to(device), g.to(device))))


def run_lnb_accumulate(device):
    from bayer_low_light_image_enhancement_amd import ops
    i = {k: v.to(device) for k, v in G.ln_inputs("base").items()}
    _, grads = ops.layernorm2d_backward(i["x"], i["weight"], i["grad_out"])
    gx, same = ops.layernorm2d_backward(i["x"], i["weight"], i["grad_out"], grads=grads)
    assert same is grads
    return host(**lnb_out(gx, grads))


def run_wmb(device, shape):
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w = shape
    x, gw, gb = WK.inputs(shape)
    t, bands = ops.wmb_front(x.to(device), (2.0 * gw).contiguous().to(device), (2.0 * gb - 1.0).contiguous().to(device))
    tb = cases.rnd(f"wmbk.t.{shape}", shape, -3.0, 3.0, seed=91)
    bb = cases.rnd(f"wmbk.bands.{shape}", (4 * b, c, h // 2, w // 2), -1.5, 1.5, seed=91)
    y = cases.rnd(f"wmbk.y.{shape}", shape, -2.0, 2.0, seed=92)
    return host(t=t, bands=bands, back=ops.wmb_back(bb.to(device), tb.to(device)),
                tail=ops.wmb_ffn_tail(x.to(device), y.to(device), gw.to(device), gb.to(device)))


def run_front_bwd(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    d = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in G.front_inputs(tag).items()}
    call = lambda grads: ops.wmb_front_backward(d["x"], d["weight2"], d["bias2"], d["grad_t"], d["grad_bands"], grad_scale=G.GRAD_SCALE, grads=grads)  # noqa: E731
    gx, pair = call(None)
    first = host(x=gx, weight2=pair[0], bias2=pair[1])
    gx2, same = call(pair)
    assert same is pair
    return {**first, **{k + "_twice": v for k, v in host(x=gx2, weight2=pair[0], bias2=pair[1]).items()}}


def run_back_bwd(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    i = G.back_inputs(tag)
    return host(bands=ops.wmb_back_backward(i["bands"].to(device), i["grad_out"].to(device)))


def run_wm(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    shape, (dlo, dhi) = WB.CASES[tag]
    seed = WB.SEED + list(WB.CASES).index(tag)
    p = {k: v.to(device) for k, v in wm_params(shape[1], seed, dlo, dhi).items()}
    x, g = cases.rnd(f"wm_bwd.{tag}.x", shape, seed=seed).to(device), cases.rnd(f"wm_bwd.{tag}.g", shape, seed=seed).to(device)
    dx, grads = ops.wm_backward(x, p, g)
    return host(out=ops.wm(x, p), x=dx, **{f"g{n:02d}.{k}": grads[k] for n, k in enumerate(grads)})


def run_haar_init(device):
    from bayer_low_light_image_enhancement_amd import ops
    out = {}
    for shape in ((1, 3, 6, 8), (1, 3, 6, 6)):
        b, c, h, w = shape
        x = cases.rnd(f"lnbits.haar.x.{shape}", shape, -2.0, 2.0, seed=SEED)
        bands = cases.rnd(f"lnbits.haar.bands.{shape}", (4 * b, c, h // 2, w // 2), -2.0, 2.0, seed=SEED)
        out.update({f"dwt_{tag_of(shape)}": ops.dwt_init(x.to(device)), f"iwt_{tag_of(shape)}": ops.iwt_init(bands.to(device))})
    return host(**out)


def run_haar_custom(device):
    """CustomDWT refuses odd sizes, so the pair runs at the two even shapes of haar.init; HaarDWT pads (1, 3, 5, 7) by reflection."""
    from bayer_low_light_image_enhancement_amd import ops
    out = {}
    for shape in ((1, 3, 6, 8), (1, 3, 6, 6)):
        bands = ops.custom_dwt(cases.rnd(f"lnbits.haar.custom.x.{shape}", shape, -2.0, 2.0, seed=SEED).to(device))
        out.update({f"dwt_{tag_of(shape)}": bands, f"idwt_{tag_of(shape)}": ops.custom_idwt(bands)})
    ll, (lh, hl, hh) = ops.haar_dwt(cases.rnd("lnbits.haar.custom.odd", (1, 3, 5, 7), -2.0, 2.0, seed=SEED).to(device))
    return host(ll=ll, lh=lh, hl=hl, hh=hh, **out)


RUNNERS = {**{f"ln.c{c}": (lambda d, c=c: run_ln(d, (1, c, 2, 4))) for c in TABLE},
           "ln.nobias.1x16x2x4": lambda d: run_ln(d, (1, 16, 2, 4), bias=False), "ln.nobias.1x24x5x7": lambda d: run_ln(d, (1, 24, 5, 7), bias=False),
           "ln.walk4": lambda d: run_ln(d, (1, 24, 3, 4)), "ln.walk1": lambda d: run_ln(d, (1, 24, 5, 7)), "ln.trips": lambda d: run_ln(d, LN_TRIPS),
           **{f"lnb.{t}{'.res' if r else ''}": (lambda d, t=t, r=r: run_lnb_case(d, t, r)) for t in G.LN_CASES for r in (False, True)},
           **{f"lnb.c{c}": (lambda d, c=c: run_lnb_shape(d, (1, c, 2, 4))) for c in TABLE},
           "lnb.accumulate": run_lnb_accumulate, "lnb.trips": lambda d: run_lnb_shape(d, LNB_TRIPS),
           **{f"wmb.{tag_of(s)}": (lambda d, s=s: run_wmb(d, s)) for s in WK.SHAPES},
           **{f"front_bwd.{t}": (lambda d, t=t: run_front_bwd(d, t)) for t in G.BAND_CASES},
           **{f"back_bwd.{t}": (lambda d, t=t: run_back_bwd(d, t)) for t in G.BACK_CASES},
           **{f"wm.{t}": (lambda d, t=t: run_wm(d, t)) for t in WM_TAGS},
           "haar.init": run_haar_init, "haar.custom": run_haar_custom}
CASE_IDS = list(RUNNERS)


def run_case(tag, device):
    """name -> array of everything the case digests."""
    return RUNNERS[tag](device)


def test_cases_reach_the_forms_they_are_named_for():
    """The launch arithmetic of launch_layernorm2d and launch_ln_bwd restated, from the shapes alone."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    for shape, wg_per_cu in ((LN_TRIPS, 8), (LNB_TRIPS, 4)):
        b, c, h, w = shape
        groups, per_wg, grid = h * w // 4, 4 * (64 // 4), cdiv(256 * wg_per_cu, b)      # C = 16: KS = 4, 16 groups per wave
        assert c == 16 and (h * w) % 4 == 0 and cdiv(groups, per_wg) > grid and grid * per_wg < groups < 2 * grid * per_wg
    assert (LN_TRIPS[2] * LN_TRIPS[3] // 4) % 64                                              # ... a partial last trip
    assert 24 not in TABLE and (3 * 4) % 4 == 0 and (5 * 7) % 4                                # the generic kernel, VEC = 4 | 1
    assert [s[1] for s in G.LN_CASES.values()] == [16, 24]
    assert WB.CASES["odd"][0][1] % 32 and (WB.CASES["odd"][0][2] * WB.CASES["odd"][0][3]) % 32
    assert 8 % 4 == 0 and 6 % 4                                                                 # dwt_init / iwt_init: vector | scalar


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
