"""Plain-torch restatements, for autograd, of the four pieces of ``WMB.forward`` (RawFomer_WFB_FFAB/model.py:215-245) whose gradients
csrc/rf_wmb_bwd.hip computes, and of ``layernorm2d``.  dtype-generic: every tensor takes the dtype of its input.

    front          t = layernorm2d(x; weight2, bias2),  bands = dwt_init(t)                  oracle.rawformer_ref.layernorm2d / dwt_init
    back           u = t + clamp((iwt_init(bands) + 1) / 2, 0, 1)                            ``iwt`` below
    dwconv5x5      F.conv2d(x, weight, bias, padding=2, groups=C)
    illumination   oracle.rawformer_ref.illumination_estimator (pinned by tests/golden/wfb_extras.npz)

``oracle.rawformer_ref.iwt_init`` builds a float32 result whatever its input, so ``iwt`` restates it for any dtype; the test module
shows that the two agree bit for bit in float32.

Every ``*_grads`` function returns the gradients of ``<f(inputs), cotangents>`` by ``torch.autograd.grad``.  ``defect=`` names a wrong
gradient that a bound must be able to see:

    front          ln_no_projection   the two mean terms of the LayerNorm adjoint missing (statistics treated as constants)
                   bands_dropped      grad_bands ignored
                   hl_lh_swapped      the HL and LH slices of grad_bands exchanged
    back           no_mask            the clamp's mask missing
                   no_half            the factor 1/2 of (v + 1) / 2 missing
                   hl_lh_swapped      the HL and LH slices of the result exchanged
    dwconv5x5      taps_unflipped     the data gradient taken with the forward's taps
                   no_padding_mask    pixels outside the plane read as the nearest edge pixel instead of zero
    illumination   no_mean_fold       grad_img without the path through the channel mean
                   no_mean_column     d conv1.weight[:, C] left at zero
                   map_ignored        grad_map ignored
"""
import torch
import torch.nn.functional as F

import cases
from oracle import rawformer_ref as R

SEED = 4700

# (B, C, h, w) of the BAND; the full-resolution tensors are [B, C, 2h, 2w].  tests/test_wmb_pieces_backward.py says what each is for.
BAND_CASES = {
    "one_item": (1, 4, 1, 2),
    "base": (2, 16, 4, 4),
    "odd": (1, 24, 3, 6),
    "blocks": (2, 4, 17, 32),
    "c512": (1, 512, 1, 2),
    "masked": (1, 6, 1, 2),
    "c48": (1, 48, 1, 2),
    "c128": (1, 128, 1, 2),
    "trips": (64, 4, 33, 64),
}
# the back pass has no branch that `trips` reaches, and 2 M draws cannot keep 1e-5 away from the clamp's two edges
BACK_CASES = {t: s for t, s in BAND_CASES.items() if t != "trips"}
# (B, C, Cm, Co, h, w); dwconv5x5 runs on [B, Cm, h, w]
ILLU_CASES = {
    "one_px": (1, 4, 4, 4, 1, 1),
    "small": (1, 4, 4, 4, 2, 3),
    "base": (2, 16, 16, 16, 8, 8),
    "w_mod4_2": (2, 16, 16, 16, 6, 10),
    "mixed": (1, 8, 12, 4, 5, 7),
    "c256": (1, 256, 256, 256, 4, 4),
    "slabs": (2, 4, 4, 4, 8, 516),
}
LN_CASES = {"base": (2, 16, 8, 8), "odd": (1, 24, 5, 7)}
ILLU_KEYS = ("conv1.weight", "conv1.bias", "depth_conv.weight", "depth_conv.bias", "conv2.weight", "conv2.bias")
GRAD_SCALE = 2.0      # what a block passes with weight2 = 2 norm1.weight

FRONT_DEFECTS = ("ln_no_projection", "bands_dropped", "hl_lh_swapped")
BACK_DEFECTS = ("no_mask", "no_half", "hl_lh_swapped")
DW5_DEFECTS = ("taps_unflipped", "no_padding_mask")
ILLU_DEFECTS = ("no_mean_fold", "no_mean_column", "map_ignored")


def seed_of(table, tag):
    return SEED + 16 * list(table).index(tag)


def iwt(x):
    """``iwt_init`` (RawFomer_WFB_FFAB/blocks.py:119-136) in the dtype of ``x``."""
    n = x.shape[0] // 4
    ll, hl, lh, hh = (x[i * n:(i + 1) * n] / 2 for i in range(4))
    out = x.new_zeros((n, x.shape[1], x.shape[2] * 2, x.shape[3] * 2))
    out[:, :, 0::2, 0::2] = ll - hl - lh + hh
    out[:, :, 1::2, 0::2] = ll - hl + lh - hh
    out[:, :, 0::2, 1::2] = ll + hl - lh - hh
    out[:, :, 1::2, 1::2] = ll + hl + lh + hh
    return out


def swap_hl_lh(bands):
    n = bands.shape[0] // 4
    return torch.cat((bands[:n], bands[2 * n:3 * n], bands[n:2 * n], bands[3 * n:]), dim=0)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------- front
def front_inputs(tag):
    """``x, weight2, bias2, grad_t, grad_bands`` in float32: x in +-2, weight2 = 2 w with w in [0.5, 1.5) and alternating signs."""
    b, c, h, w = BAND_CASES[tag]
    s = seed_of(BAND_CASES, tag)
    sign = 1.0 - 2.0 * (torch.arange(c) % 2).float()
    return {"x": cases.rnd(f"front.{tag}.x", (b, c, 2 * h, 2 * w), -2.0, 2.0, seed=s),
            "weight2": 2.0 * sign * cases.rnd(f"front.{tag}.w", (c,), 0.5, 1.5, seed=s),
            "bias2": 2.0 * cases.rnd(f"front.{tag}.b", (c,), seed=s) - 1.0,
            "grad_t": cases.rnd(f"front.{tag}.gt", (b, c, 2 * h, 2 * w), seed=s),
            "grad_bands": cases.rnd(f"front.{tag}.gb", (4 * b, c, h, w), seed=s)}


def front_forward(x, weight2, bias2, eps=1e-5):
    t = R.layernorm2d(x, weight2, bias2, eps)
    return t, R.dwt_init(t)


def front_grads(i, defect=None):
    """``{"x", "weight2", "bias2"}``: the gradients of ``<t, grad_t> + <bands, grad_bands>``, the parameter gradients times GRAD_SCALE."""
    assert defect is None or defect in FRONT_DEFECTS, defect
    x, w2, b2 = _leaf(i["x"]), _leaf(i["weight2"]), _leaf(i["bias2"])
    if defect == "ln_no_projection":
        mu = x.mean(dim=1, keepdim=True).detach()
        var = ((x - mu) ** 2).mean(dim=1, keepdim=True).detach()
        t = (x - mu) / torch.sqrt(var + 1e-5) * w2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)
        bands = R.dwt_init(t)
    else:
        t, bands = front_forward(x, w2, b2)
    gb = swap_hl_lh(i["grad_bands"]) if defect == "hl_lh_swapped" else i["grad_bands"]
    loss = (t * i["grad_t"]).sum()
    if defect != "bands_dropped":
        loss = loss + (bands * gb).sum()
    gx, gw, gbias = torch.autograd.grad(loss, [x, w2, b2])
    return {"x": gx, "weight2": GRAD_SCALE * gw, "bias2": GRAD_SCALE * gbias}


# ---------------------------------------------------------------------------------------------- back
def back_preclamp(bands):
    return (iwt(bands) + 1) / 2


def back_condition(bands):
    """What the clamp condition asks of a draw, in float64 and against the float32 restatement: the fractions cut low and high, the
    smallest distance of a value before the clamp from 0 or 1, and whether float32 puts every element on float64's side."""
    v64, v32 = back_preclamp(bands.double()), back_preclamp(bands)
    low, high = v64 < 0, v64 > 1
    same = bool(((v32 < 0) == low).all() and ((v32 > 1) == high).all())
    return float(low.double().mean()), float(high.double().mean()), float(torch.minimum(v64.abs(), (v64 - 1).abs()).min()), same


def back_condition_holds(bands):
    low, high, gap, same = back_condition(bands)
    return low >= 0.1 and high >= 0.1 and gap > 1e-5 and same


def back_inputs(tag):
    """``bands, grad_out, tries``: bands uniform in (-2, 2), the first of at most 16 seeds ``seed_of(tag) + k`` whose draw meets
    ``back_condition_holds``."""
    b, c, h, w = BAND_CASES[tag]
    s = seed_of(BAND_CASES, tag)
    for k in range(16):
        bands = cases.rnd(f"back.{tag}.bands", (4 * b, c, h, w), -2.0, 2.0, seed=s + k)
        if back_condition_holds(bands):
            return {"bands": bands, "grad_out": cases.rnd(f"back.{tag}.g", (b, c, 2 * h, 2 * w), seed=s), "tries": k + 1}
    raise AssertionError(f"back.{tag}: none of 16 seeds meets the clamp condition")


def back_grads(i, defect=None):
    """``{"bands"}``: the gradient of ``<clamp((iwt_init(bands) + 1) / 2, 0, 1), grad_out>`` (t adds grad_out itself and is left out)."""
    assert defect is None or defect in BACK_DEFECTS, defect
    bands = _leaf(i["bands"])
    v = iwt(bands) + 1 if defect == "no_half" else back_preclamp(bands)
    u = v if defect == "no_mask" else (v.clamp(0, 2) if defect == "no_half" else v.clamp(0, 1))      # no_half keeps the mask's set
    (g,) = torch.autograd.grad((u * i["grad_out"]).sum(), [bands])
    return {"bands": swap_hl_lh(g) if defect == "hl_lh_swapped" else g}


# ---------------------------------------------------------------------------------------------- depthwise 5x5
def dw5_inputs(tag):
    b, _, c, _, h, w = ILLU_CASES[tag]
    s = seed_of(ILLU_CASES, tag)
    return {"x": cases.rnd(f"dw5.{tag}.x", (b, c, h, w), seed=s), "weight": cases.rnd(f"dw5.{tag}.w", (c, 1, 5, 5), seed=s) / 5.0,
            "bias": cases.rnd(f"dw5.{tag}.b", (c,), seed=s), "grad_out": cases.rnd(f"dw5.{tag}.g", (b, c, h, w), seed=s)}


def dw5_grads(i, defect=None):
    """``{"x", "weight", "bias"}`` of ``<dwconv5x5(x), grad_out>``."""
    assert defect is None or defect in DW5_DEFECTS, defect
    x, wgt, bias = _leaf(i["x"]), _leaf(i["weight"]), _leaf(i["bias"])
    c = x.shape[1]
    if defect == "no_padding_mask":
        y = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), wgt, bias, groups=c)
    else:
        y = F.conv2d(x, wgt, bias, padding=2, groups=c)
    gx, gw, gb = torch.autograd.grad((y * i["grad_out"]).sum(), [x, wgt, bias])
    if defect == "taps_unflipped":
        gx = F.conv2d(i["grad_out"], i["weight"], None, padding=2, groups=c)
    return {"x": gx, "weight": gw, "bias": gb}


# ---------------------------------------------------------------------------------------------- Illumination_Estimator
def illu_inputs(tag):
    """``img, grad_fea, grad_map`` and the six parameters: weights uniform in +-1 / sqrt(fan-in), biases in +-1."""
    b, c, cm, co, h, w = ILLU_CASES[tag]
    s = seed_of(ILLU_CASES, tag)
    shapes = {"conv1.weight": (cm, c + 1, 1, 1), "conv1.bias": (cm,), "depth_conv.weight": (cm, 1, 5, 5), "depth_conv.bias": (cm,),
              "conv2.weight": (co, cm, 1, 1), "conv2.bias": (co,)}
    p = {}
    for k, shp in shapes.items():
        fan = shp[1] * shp[2] * shp[3] if len(shp) == 4 else 1
        p[k] = cases.rnd(f"illu.{tag}.{k}", shp, seed=s) / fan ** 0.5
    return {"img": cases.rnd(f"illu.{tag}.img", (b, c, h, w), seed=s), "grad_fea": cases.rnd(f"illu.{tag}.gf", (b, cm, h, w), seed=s),
            "grad_map": cases.rnd(f"illu.{tag}.gm", (b, co, h, w), seed=s), "p": p}


def illu_grads(i, with_map, defect=None):
    """``{"img"} + ILLU_KEYS``: the gradients of ``<illu_fea, grad_fea>`` (``with_map``: ``+ <illu_map, grad_map>``)."""
    assert defect is None or defect in ILLU_DEFECTS, defect
    assert defect != "map_ignored" or with_map
    img = _leaf(i["img"])
    p = {k: _leaf(v) for k, v in i["p"].items()}
    if defect == "no_mean_fold":
        inp = torch.cat([img, img.mean(dim=1, keepdim=True).detach()], dim=1)
        x1 = F.conv2d(inp, p["conv1.weight"], p["conv1.bias"])
        fea = F.conv2d(x1, p["depth_conv.weight"], p["depth_conv.bias"], padding=2, groups=x1.shape[1])
        out = fea, F.conv2d(fea, p["conv2.weight"], p["conv2.bias"])
    else:
        out = R.illumination_estimator(img, p, "")
    loss = (out[0] * i["grad_fea"]).sum()
    if with_map and defect != "map_ignored":
        loss = loss + (out[1] * i["grad_map"]).sum()
    else:
        loss = loss + 0.0 * out[1].sum()                     # conv2's gradients: exact zeros
    got = torch.autograd.grad(loss, [img] + [p[k] for k in ILLU_KEYS])
    res = {"img": got[0], **dict(zip(ILLU_KEYS, got[1:]))}
    if defect == "no_mean_column":
        res["conv1.weight"] = res["conv1.weight"].clone()
        res["conv1.weight"][:, -1] = 0
    return res


# ---------------------------------------------------------------------------------------------- LayerNorm
def ln_inputs(tag):
    b, c, h, w = LN_CASES[tag]
    s = seed_of(LN_CASES, tag)
    return {"x": cases.rnd(f"ln.{tag}.x", (b, c, h, w), -2.0, 2.0, seed=s), "weight": cases.rnd(f"ln.{tag}.w", (c,), 0.5, 1.5, seed=s),
            "bias": cases.rnd(f"ln.{tag}.b", (c,), seed=s), "grad_out": cases.rnd(f"ln.{tag}.g", (b, c, h, w), seed=s),
            "residual": cases.rnd(f"ln.{tag}.r", (b, c, h, w), seed=s)}


def ln_grads(i, with_residual):
    """``{"x", "weight", "bias"}`` of ``<layernorm2d(x), grad_out>``; ``with_residual`` adds ``residual`` to the gradient of x."""
    x, wgt, bias = _leaf(i["x"]), _leaf(i["weight"]), _leaf(i["bias"])
    gx, gw, gb = torch.autograd.grad((R.layernorm2d(x, wgt, bias) * i["grad_out"]).sum(), [x, wgt, bias])
    return {"x": gx + i["residual"] if with_residual else gx, "weight": gw, "bias": gb}


def as_dtype(i, dtype):
    """The inputs of a case in ``dtype`` (nested parameter dictionaries included; other entries pass through)."""
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) else as_dtype(v, dtype) if isinstance(v, dict) else v) for k, v in i.items()}
