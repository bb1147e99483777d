"""Shared description of the golden per-operator cases.

``oracle/make_golden.py`` ran the REFERENCE's classes on these inputs/parameters (all
regenerated from ``synth`` by name) and stored the reference outputs in
``tests/golden/per_op.npz``.  The CPU tests check the oracle against those outputs; the GPU
tests check the HIP path against both.
"""
from __future__ import annotations

import glob
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from bayer_low_light_image_enhancement_amd import synth  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
SEED = 11


class _Parts(dict):
    """The arrays of a fixture stored in parts, with the ``files`` list an ``np.load`` result has."""

    @property
    def files(self):
        return list(self)


def golden(name: str):
    """``tests/golden/<name>.npz``, or the union of ``<name>.part<i>.npz`` for a fixture stored in parts (every committed file
    stays below 1 MiB; oracle/make_golden.py ``save`` splits)."""
    path = os.path.join(GOLDEN, name + ".npz")
    if os.path.exists(path):
        return np.load(path)
    parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")))
    if not parts:
        raise FileNotFoundError(path)
    out = _Parts()
    for p in parts:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def rnd(name, shape, lo=-1.0, hi=1.0, seed=SEED):
    return torch.from_numpy(synth.uniform(seed, name, shape, lo, hi))


def params(spec, seed=SEED, prefix=""):
    """spec: {name: shape}; values exactly as ``synth.fill_state_dict`` gave the reference module."""
    return {prefix + k: torch.from_numpy(synth.param_values(seed, k, s)).reshape(s) for k, s in spec.items()}


def attention_spec(c):
    return {"temperature": (8, 1, 1), "qkv.weight": (3 * c, c, 1, 1), "qkv.bias": (3 * c,),
            "qkv_dwconv.weight": (3 * c, 1, 3, 3), "qkv_dwconv.bias": (3 * c,),
            "project_out.weight": (c, c, 1, 1), "project_out.bias": (c,)}


def ffn_spec(c):
    return {"pointwise1.weight": (2 * c, c, 1, 1), "pointwise1.bias": (2 * c,),
            "depthwise.weight": (2 * c, 1, 3, 3), "depthwise.bias": (2 * c,),
            "pointwise2.weight": (c, 2 * c, 1, 1), "pointwise2.bias": (c,)}


def transformer_spec(c):
    s = {"norm1.body.weight": (c,), "norm1.body.bias": (c,)}
    s.update({"attn." + k: v for k, v in attention_spec(c).items()})
    s.update({"norm2.body.weight": (c,), "norm2.body.bias": (c,)})
    s.update({"ffn." + k: v for k, v in ffn_spec(c).items()})
    return s


def flca_spec(c):
    hid = max(8, c // 8)
    return {"alpha": (), "beta": (), "gamma": (), "low_attn.0.weight": (c, 1, 3, 3),
            "high_attn.0.weight": (c, 1, 3, 3), "chroma_attn.0.weight": (c, 2, 3, 3),
            "se.1.weight": (hid, c, 1, 1), "se.1.bias": (hid,), "se.3.weight": (c, hid, 1, 1), "se.3.bias": (c,)}


def conv_transformer_flca_spec(c):
    s = {"FLCA." + k: v for k, v in flca_spec(c).items()}
    s.update({"Transformer." + k: v for k, v in transformer_spec(c).items()})
    s.update({"channel_reduce.weight": (c, 2 * c, 1, 1), "channel_reduce.bias": (c,),
              "Conv_out.weight": (c, c, 3, 3), "Conv_out.bias": (c,)})
    return s


ATTN_CASES = ((16, (16, 24)), (32, (16, 16)), (48, (8, 12)))
FLCA_CASES = ((16, (32, 48)), (32, (16, 24)), (64, (8, 12)), (128, (4, 6)))
LN_CASES = ((16, (16, 24)), (48, (8, 8)))

MODEL_CASES = (("d16_b2_32x32", 16, 2, 32, 32, 21), ("d16_b1_32x48", 16, 1, 32, 48, 22),
               ("d32_b2_64x64", 32, 2, 64, 64, 23), ("d48_b1_32x32", 48, 1, 32, 32, 24))


def model_state(dim, seed, variant="flca"):
    """Deterministic canonical state_dict for a whole model (what make_golden gave the reference)."""
    from oracle import rawformer_ref as R
    cfg = R.RawFormerConfig(dim=dim, variant=variant)
    shapes = R.param_shapes(cfg)
    return {k: torch.from_numpy(synth.param_values(seed, k, s)).reshape(s) for k, s in shapes.items()}


# a16: Attenblock.LuminanceAwareMHSA cases of tests/golden/attenblock.npz: (tag, dim, heads, B, h, w)
ATTEN_CASES = (("d4", 32, 8, 2, 16, 16), ("d6", 48, 8, 1, 12, 20), ("d16", 64, 4, 1, 8, 24), ("d32", 64, 2, 1, 16, 16))


def atten_spec(dim, heads):
    inner = heads * (dim // heads)
    hid = max(16, inner // 2)
    return {"alpha": (), "to_qkv.weight": (3 * inner, dim, 1, 1), "to_qkv.bias": (3 * inner,),
            "proj.weight": (dim, inner, 1, 1), "proj.bias": (dim,),
            "luma_cond.net.0.weight": (hid, 1, 3, 3), "luma_cond.net.0.bias": (hid,),
            "luma_cond.net.2.weight": (hid, hid, 3, 3), "luma_cond.net.2.bias": (hid,),
            "luma_cond.gamma.weight": (inner, hid, 1, 1), "luma_cond.gamma.bias": (inner,),
            "luma_cond.beta.weight": (inner, hid, 1, 1), "luma_cond.beta.bias": (inner,)}


def atten_inputs(tag, dim, heads, b, h, w):
    x = rnd(f"atten.{tag}.x", (b, dim, h, w), seed=41)
    luma = rnd(f"atten.{tag}.luma", (b, 1, h, w), 0.0, 1.0, seed=42)
    return x, luma, params(atten_spec(dim, heads), seed=700 + dim + heads)


# a17: WFB extras of tests/golden/wfb_extras.npz
WFB_FF_CASES = (("ff32", 32, 2.0, 2, 16, 24), ("ff48", 48, 2.5, 1, 10, 14))     # tag, dim, expansion, B, h, w
WFB_IE_CASES = (("ie32", 32, 2, 16, 24), ("ie40", 40, 1, 9, 14))                # tag, middle channels, B, h, w


def wfb_ff_spec(dim, fac):
    hid = int(dim * fac)
    s = {"project_in.weight": (hid, dim, 1, 1), "project_in.bias": (hid,), "dwconv.weight": (hid, 1, 3, 3), "dwconv.bias": (hid,),
         "project_out.weight": (dim, hid, 1, 1), "project_out.bias": (dim,)}
    for name, k in (("rep_conv1", 3), ("rep_conv2", 1)):
        s[f"{name}.c.weight"] = (hid, 1, k, k)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{name}.bn.{leaf}"] = (hid,)
    return s


def wfb_ie_spec(mid):
    return {"conv1.weight": (mid, 4, 1, 1), "conv1.bias": (mid,), "depth_conv.weight": (mid, 1, 5, 5), "depth_conv.bias": (mid,),
            "conv2.weight": (3, mid, 1, 1), "conv2.bias": (3,)}


def atten_tb_spec(dim, heads):
    s = {"norm1.body.weight": (dim,), "norm1.body.bias": (dim,), "norm2.body.weight": (dim,), "norm2.body.bias": (dim,)}
    s.update({"attn." + k: v for k, v in atten_spec(dim, heads).items()})
    s.update({"ffn." + k: v for k, v in ffn_spec(dim).items()})
    return s


def atten_tb_inputs(tag, dim, heads, b, h, w):
    x = rnd(f"atten.tb.{tag}.x", (b, dim, h, w), seed=43)
    luma = rnd(f"atten.tb.{tag}.luma", (b, 1, h, w), 0.0, 1.0, seed=44)
    return x, luma, params(atten_tb_spec(dim, heads), seed=750 + dim)


# ---- handle layout and launch census: tools/make_handle_layout.py records, test_handle_layout.py / test_forward_launches.py compare
VARIANT_IDS = {"flca": 0, "plain": 1, "truecolor": 2, "multilvl": 3, "wfb": 4}
# tag: (variant, dim, ffn_expansion, branch_lrelu, clamp_io, flca_levels); heads 8 at every level, 3 output channels
HANDLE_CONFIGS = {
    "flca_d32": ("flca", 32, 2, 1, 0, 0), "flca_d48": ("flca", 48, 2, 1, 0, 0),
    "plain_d16_lrelu0": ("plain", 16, 2, 0, 0, 0), "plain_d16_lrelu1": ("plain", 16, 2, 1, 0, 0), "plain_d32_clamp": ("plain", 32, 2, 1, 1, 0),
    "truecolor_d32_l2": ("truecolor", 32, 2, 1, 0, 2), "truecolor_d32_l3": ("truecolor", 32, 2, 1, 0, 3),
    **{f"multilvl_d{d}_l{l}": ("multilvl", d, 2, 1, 0, l) for d in (16, 32) for l in (0, 1, 3)},
    **{f"wfb_d{d}_f{f}": ("wfb", d, f, 1, 1, 0) for d in (16, 32) for f in (2, 3)},
}
LAYOUT_FRAMES = ((1, 32, 32), (2, 64, 96), (1, 40, 72), (8, 512, 512), (1, 712, 1064))      # B, packed H, W


def handle_params(tag):
    """``(name, shape, flags)`` of every registered tensor of HANDLE_CONFIGS[tag], in registry order, and the handle's plans:
    rf_packed_bytes and, per LAYOUT_FRAMES entry, rf_workspace_bytes or its (negative) error code.  No device is needed."""
    import ctypes as C
    from bayer_low_light_image_enhancement_amd import _lib
    variant, dim, ffn, lrelu, clamp, levels = HANDLE_CONFIGS[tag]
    lib = _lib.load()
    cfg = _lib.RfConfig(dim, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, ffn, VARIANT_IDS[variant], lrelu, clamp, levels)
    h = C.c_void_p()
    _lib.check(lib.rf_create(C.byref(cfg), C.byref(h)), "rf_create")
    try:
        name, shape, ndim, flags, sz = C.c_char_p(), (C.c_int64 * 4)(), C.c_int(), C.c_int(), C.c_size_t()
        rows = []
        for i in range(lib.rf_param_count(h)):
            _lib.check(lib.rf_param_info(h, i, C.byref(name), C.byref(shape), C.byref(ndim)), "rf_param_info")
            _lib.check(lib.rf_param_flags(h, i, C.byref(flags)), "rf_param_flags")
            rows.append((name.value.decode(), list(shape[: ndim.value]), flags.value))
        _lib.check(lib.rf_packed_bytes(h, C.byref(sz)), "rf_packed_bytes")
        plans = {"packed_bytes": sz.value, "workspace_bytes": []}
        for b, hh, ww in LAYOUT_FRAMES:
            rc = lib.rf_workspace_bytes(h, b, hh, ww, C.byref(sz))
            plans["workspace_bytes"].append(sz.value if rc == 0 else rc)
    finally:
        lib.rf_destroy(h)
    return rows, plans


def params_digest(rows):
    import hashlib
    return hashlib.sha256("\n".join(f"{n} {s} {f}" for n, s, f in rows).encode()).hexdigest()


def census(fn):
    """``fn()`` between rf_profile_begin and rf_profile_end: its result and ``{kernel: [launches, flops, bytes]}``, the library's
    per-launch brackets summed by kernel class (the times left out)."""
    import ctypes
    import json
    from bayer_low_light_image_enhancement_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.rf_profile_begin()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        buf = ctypes.create_string_buffer(1 << 16)
        _lib.check(lib.rf_profile_end(buf, len(buf)), "rf_profile_end")
    return out, {r["kernel"]: [r["launches"], r["flops"], r["bytes"]] for r in json.loads(buf.value.decode())}


def launches(fn):
    """Kernel launches of ``fn()`` by kernel class, from the library's own per-launch brackets."""
    out, c = census(fn)
    return out, {k: v[0] for k, v in c.items()}


# Launch census cases: tag -> (variant, dim, constructor keywords, B, packed H, W, stage or None = the whole forward).  Small
# frames; between them every decision of the host schedule takes both values (the kernel named is what shows it in the census):
#   fuse_tail   dim 32 level 0 / dim 16 level 1 at a width % 4 == 0 (ffn_fused tail) | every other level
#   compose     C % 32 == 0 off the fused FFN (dim 32 levels 1-3) | dim 16 level 0, and level 3 of 40 x 72 (5 x 9 pixels, not % 4)
#   fuse_up     level-3 width 4 (packed width 32: upcat_kernel) | 9 (packed width 72: the ConvTranspose2d GEMM + channel_reduce)
#   ks_floats   > 0 (every small frame) | 0: 1032 x 1024, whose level 3 has more than 16384 pixels
#   ml_step_fused_supported   C <= 64 (levels 0-1) | levels 2-3;   conv1x1_ln_single_pass   C <= 64 or 128 / 256 | dim 24 levels 2-3 (C = 96, 192)
LAUNCH_CASES = {
    "flca_d16_b2_32x32": ("flca", 16, {}, 2, 32, 32, None),
    "flca_d32_b2_64x64": ("flca", 32, {}, 2, 64, 64, None),
    "flca_d32_b1_40x72": ("flca", 32, {}, 1, 40, 72, None),
    "plain_d16_b1_32x48": ("plain", 16, {"branch_lrelu": False}, 1, 32, 48, None),
    "plain_d32_b1_32x32": ("plain", 32, {"clamp_io": True}, 1, 32, 32, None),
    "plain_d16_b1_1032x1024": ("plain", 16, {}, 1, 1032, 1024, None),
    "truecolor_d32_b1_32x32": ("truecolor", 32, {}, 1, 32, 32, None),
    "truecolor_d32_l3_b1_40x72": ("truecolor", 32, {"flca_levels": 3}, 1, 40, 72, None),
    "multilvl_d16_b2_32x48": ("multilvl", 16, {}, 2, 32, 48, None),
    "multilvl_d32_l3_b1_40x72": ("multilvl", 32, {"flca_levels": 3}, 1, 40, 72, None),
    "wfb_d16_b1_32x32": ("wfb", 16, {}, 1, 32, 32, None),
    "wfb_d32_f3_b2_64x96": ("wfb", 32, {"ffn_expansion_factor": 3}, 2, 64, 96, None),
    "wfb_d24_b1_32x32": ("wfb", 24, {}, 1, 32, 32, None),
    **{f"{v}_d{d}_stage{s}": (v, d, {}, 1, 32, 32, s) for v, d in (("flca", 32), ("plain", 16), ("multilvl", 16), ("wfb", 16)) for s in (1, 4)},
}
_LAUNCH_MODELS = {}


def launch_case(tag, device):
    """The model (PyTorch's default initialisers under a fixed seed, built once per configuration) and a closure that runs the
    case's one call on fixed random inputs."""
    from bayer_low_light_image_enhancement_amd import RawFormer
    variant, dim, kw, b, hh, ww, stage = LAUNCH_CASES[tag]
    key = (variant, dim, tuple(sorted(kw.items())))
    if key not in _LAUNCH_MODELS:
        torch.manual_seed(1234)
        _LAUNCH_MODELS[key] = RawFormer(dim=dim, variant=variant, **kw).to(device).eval()
    m = _LAUNCH_MODELS[key]
    g = torch.Generator().manual_seed(len(tag) + 7 * b + hh + ww)
    if stage is None:
        x = torch.rand((b, 1, 2 * hh, 2 * ww), generator=g).to(device)
        return m, lambda: m(x)
    lvl = stage - 1
    x = (2 * torch.rand((b, dim << lvl, hh >> lvl, ww >> lvl), generator=g) - 1).to(device)
    packed = torch.rand((b, 4, hh, ww), generator=g).to(device) if variant in ("flca", "multilvl") else None
    return m, lambda: m.forward_stage(stage, x, packed)


# ---- 1x1 GEMM selection: tools/make_conv1x1_keys.py records, test_conv1x1_plan.py compares.
# tag -> (C1, C2, Cout, B, h, w, flags); flags: "ln" LayerNorm prologue, "res" residual (no bias), "T" ConvTranspose2d(C1, Cout, 2, 2)
# through ops.conv_transpose2x2 (GEMM rows 4 Cout, no bf16x3 weights).  Derived from the ladders of plan_conv1x1 (rf_gemm1x1.hip),
# in its order, at the smallest frame that reaches each instantiation (K = C1 + C2, NT = Cout / 16, units = pixel tiles x images):
#   scalar      P % 4 != 0 | a residual with Cout % 16 != 0
#   b3_ln       LayerNorm, K = 64 / 128 / 256 (KB = 2 / 4 / 8), Cout % 64 == 0, no residual; NCO 4 at K = 256 and Cout % 256 == 0,
#               else 3 at Cout % 192 == 0, else 2; the blockIdx.z split at fewer than 128 workgroups and more than one chunk per wave
#   b3          K >= 128 otherwise: NCO 6 at NT % 6 == 0, 2 below 256 workgroups at an even NT, else 4; LayerNorm (K = 512, or K = 128
#               with a residual) only at 4; paired from units x pairs >= 256
#   res         K <= 64, or K <= 128 without LayerNorm and residual: KS = 4, 8, 12, 16, 24, 32; RT 2 with a residual, 4 at KS 12 / 16
#               without LayerNorm and Cout >= 48; one case with two output groups (K = 64 -> 256)
#   stream      the rest (K = 96 with LayerNorm or a residual, K = 132): NCO 4 | 8 where 8 tiles fill the 512 slots no worse (129 units, NT 16)
CONV1X1_CASES = {
    "scalar_p35": (24, 0, 80, 1, 5, 7, "res"),
    "scalar_cout24_res": (16, 0, 24, 1, 8, 8, "res"),
    **{f"res_k{k}_o{o}{'_' + f.replace(' ', '_') if f else ''}": (k, 0, o, 1, 16, 16, f)
       for k, o in ((16, 32), (32, 48)) for f in ("", "ln", "res", "ln res")},
    **{f"res_k{k}_o{o}{'_' + f.replace(' ', '_') if f else ''}": (k, 0, o, 2, 12, 20, f)
       for k, o, fs in ((48, 64, ("", "ln", "res", "ln res")), (48, 32, ("res",)), (64, 48, ("", "ln", "res", "ln res")), (64, 32, ("res",)))
       for f in fs},
    "res_k32_32_o48_res": (32, 32, 48, 1, 16, 16, "res"),
    "res_k64_o256_two_groups": (64, 0, 256, 1, 16, 16, ""),
    "res_k96_o48": (96, 0, 48, 1, 16, 16, ""),
    "res_k112_o48": (112, 0, 48, 1, 16, 16, ""),
    "stream_k96_o96_res": (96, 0, 96, 1, 16, 16, "res"),
    "stream_k96_o96_ln": (96, 0, 96, 1, 16, 16, "ln"),
    "stream_k132_o64": (132, 0, 64, 1, 8, 8, ""),
    "stream8_k96_o256_res": (96, 0, 256, 1, 129, 256, "res"),
    "stream8_k96_o256_ln": (96, 0, 256, 1, 129, 256, "ln"),
    "b3_k128_o128": (128, 0, 128, 1, 16, 16, ""),
    "b3_k128_o80": (128, 0, 80, 1, 16, 16, ""),
    "b3_k64_64_o80_res": (64, 64, 80, 1, 12, 20, "res"),
    "b3_k128_o96_res": (128, 0, 96, 1, 16, 16, "res"),
    "b3_k512_o64_ln": (512, 0, 64, 1, 8, 8, "ln"),
    "b3_k128_o64_ln_res": (128, 0, 64, 1, 16, 16, "ln res"),
    "b3_pair_k128_o512": (128, 0, 512, 1, 128, 128, ""),
    "b3_pair_k128_o768": (128, 0, 768, 1, 128, 128, ""),
    "b3ln_k64_o128": (64, 0, 128, 1, 16, 16, "ln"),
    "b3ln_k64_o192": (64, 0, 192, 1, 9, 20, "ln"),
    "b3ln_k128_o256_zsplit": (128, 0, 256, 1, 16, 16, "ln"),
    "b3ln_k128_o256_b8_no_split": (128, 0, 256, 8, 32, 32, "ln"),
    "b3ln_k128_o192": (128, 0, 192, 1, 16, 16, "ln"),
    "b3ln_k256_o128": (256, 0, 128, 1, 16, 16, "ln"),
    "b3ln_k256_o384_zsplit": (256, 0, 384, 1, 16, 16, "ln"),
    "b3ln_k256_o256": (256, 0, 256, 1, 12, 20, "ln"),
    "convT_k32_o16": (32, 0, 16, 2, 8, 8, "T"),
    "convT_k128_o64": (128, 0, 64, 1, 8, 8, "T"),
    "convT_k256_o128": (256, 0, 128, 1, 4, 6, "T"),
}


def conv1x1_case(tag):
    """Inputs of CONV1X1_CASES[tag] (ranges and weight scaling of test_conv1x1_groups.inputs; the LayerNorm input and affine of
    test_gpu_ops.test_conv1x1) and ``run(ops, device)``, the case's one call."""
    c1, c2, cout, b, h, w, flags = CONV1X1_CASES[tag]
    k = c1 + c2
    t = {"x": rnd("g.x", (b, c1, h, w)), "bias": rnd("g.b", (cout,))}
    if "T" in flags:
        t["w"] = rnd("g.w", (k, cout, 2, 2)) / np.sqrt(k)
    else:
        t["w"] = rnd("g.w", (cout, k, 1, 1)) / np.sqrt(k)
    if c2:
        t["x2"] = rnd("g.x2", (b, c2, h, w))
    if "ln" in flags:
        t["x"] = t["x"] * 2.0 + 0.7
        t["ln_w"], t["ln_b"] = rnd("g.lw", (k,), 0.5, 1.5), rnd("g.lb", (k,))
    if "res" in flags:
        t["res"] = rnd("g.res", (b, cout, h, w))

    def run(ops, device):
        d = {n: v.to(device) for n, v in t.items()}
        if "T" in flags:
            return ops.conv_transpose2x2(d["x"], d["w"], d["bias"])
        return ops.conv1x1(d["x"], d["w"], None if "res" in flags else d["bias"], x2=d.get("x2"), ln_weight=d.get("ln_w"),
                           ln_bias=d.get("ln_b"), residual=d.get("res"))
    return t, run


# ---- 3x3 convolution selection: tools/make_conv3x3_keys.py records, test_conv3x3_plan.py compares.
# tag -> (B, Cin, Cout, h, w, store), through ops.conv3x3 with bias and LeakyReLU.  Derived from the ladder of plan_conv3x3
# (rf_conv3x3.hip), in its order, at the smallest frame that reaches each instantiation <NCO, LOG2_RW, RPW, NWV>.  NT = ceil(Cout / 16)
# output tiles; NCO = 4, or at NT % 4 != 0: 3 at NT % 3 == 0, else 2 at an even NT, else 1 at NT == 1, else 4.
#   small       w > 32, h >= 8 and fewer than 128 workgroups of the wide form: <N, 0, 1, 4>, NCO halved (3 -> 1) while 4 x 64 tiles x
#               groups < 192.  NCO stays 4 / 3 / 2 only on one tall frame (192 tiles of 4 rows, under 128 of 8 or 16)
#   <1,0,1,16>  NCO 1, w > 32, h >= 16; 128 workgroups = 8 frames of 16 tiles.  Level-0 form (", false, 3") at Cin <= 32, w % 4 == 0
#   <2,0,2,8>   NCO 2, w > 32, h >= 16; its level-0 form likewise.  <N,0,1,8>: NCO 3 / 4 at h >= 8, NCO 1 / 2 at 8 <= h < 16 (128 frames
#               of one workgroup: the small rule counts 16-row tiles for them)
#   <N,L,1,4>   the rest: w > 32 and h < 8 (L = 0), 16 < w <= 32 (L = 1), w <= 16 (L = 2)
# The input-channel split needs scratch that ops.conv3x3 does not pass: CONV3X3_SPLIT_STAGES pins it through forward_stage.
CONV3X3_CASES = {
    "small_n4_tall": (1, 8, 64, 768, 64, "plain"),
    "small_n3_tall": (1, 12, 48, 766, 64, "unshuffle"),
    "small_n2_tall": (1, 8, 32, 768, 62, "plain"),                # w % 4 != 0: scalar stores
    "small_n4_to_n2": (1, 8, 64, 400, 64, "shuffle"),
    "small_n4_to_n1": (1, 20, 64, 16, 64, "plain"),
    "small_n3_to_n1": (1, 8, 48, 30, 70, "unshuffle"),            # ragged last tile in both directions
    "small_n1": (1, 8, 16, 8, 33, "plain"),
    "w16_n1": (8, 40, 16, 256, 64, "plain"),                      # exactly 128 workgroups
    "w16_n1_ragged": (8, 44, 12, 250, 38, "shuffle"),             # Cin ends inside a chunk, w % 4 != 0
    "w16_n1_l0": (8, 32, 16, 256, 64, "plain"),
    "w16_n1_l0_ragged": (8, 20, 12, 250, 36, "unshuffle"),
    "rpw2_n2": (8, 40, 32, 256, 64, "plain"),
    "rpw2_n2_ragged": (8, 36, 32, 242, 34, "unshuffle"),
    "rpw2_n2_l0": (8, 32, 32, 256, 64, "shuffle"),
    "rpw2_n2_l0_ragged": (8, 20, 32, 250, 36, "plain"),
    "wide8_n4": (16, 8, 64, 64, 64, "plain"),                     # exactly 128 workgroups
    "wide8_n4_two_tiles": (4, 12, 64, 200, 200, "unshuffle"),     # 400 tiles on 200 workgroups: the persistent loop, ragged both ways
    "wide8_n4_nt5": (16, 8, 80, 60, 62, "shuffle"),               # two groups, the second with one live tile of four
    "wide8_n3": (16, 12, 48, 60, 62, "plain"),
    "wide8_n1": (128, 8, 12, 9, 34, "plain"),
    "wide8_n2": (128, 8, 32, 12, 36, "unshuffle"),
    **{f"rw0_n{n}": (1, 8, 16 * n, 7, 66, "plain") for n in (1, 2, 3, 4)},
    "rw1_n1": (2, 20, 16, 9, 21, "plain"), "rw1_n2": (2, 20, 32, 9, 32, "plain"),
    "rw1_n3": (2, 20, 48, 10, 22, "unshuffle"), "rw1_n4": (2, 20, 64, 9, 24, "shuffle"),
    "rw2_n1": (2, 20, 16, 17, 13, "plain"), "rw2_n2": (2, 20, 32, 17, 16, "plain"),
    "rw2_n3": (2, 20, 48, 17, 15, "shuffle"), "rw2_n4": (2, 20, 64, 33, 9, "plain"),
    "rw2_n4_unshuffle": (1, 8, 60, 18, 16, "unshuffle"),
}
# LAUNCH_CASES whose level-3 convolutions (128 / 256 channels on one 4 x 4 frame) run with their input channels split,
# <4, 2, 1, 4, true>, which forward_launches.json records under the key of the unsplit kernel
CONV3X3_SPLIT_STAGES = ("plain_d16_stage4", "flca_d32_stage4")


def conv3x3_case(tag):
    """Inputs of CONV3X3_CASES[tag] (ranges and weight scaling of test_conv3x3_level0.inputs) and ``run(ops, device)``, the case's
    one call."""
    b, cin, cout, h, w, store = CONV3X3_CASES[tag]
    t = {"x": rnd(f"c3l0.x.{tag}", (b, cin, h, w)), "w": rnd(f"c3l0.w.{tag}", (cout, cin, 3, 3)) / np.sqrt(cin * 9 / 3),
         "bias": rnd(f"c3l0.b.{tag}", (cout,))}

    def run(ops, device):
        return ops.conv3x3(t["x"].to(device), t["w"].to(device), t["bias"].to(device), act="lrelu", store=store)
    return t, run


# ---- FFT lines: test_fft_lines.py. tag -> ((planes, h, w), the regime the case is there for, as rf_fft_plan states it:
# log2 w / log2 h (-1: direct DFT), L rows per row workgroup, TC columns per column workgroup, most trips of a row / of a column
# workgroup through its persistent loop).  The shapes follow the plan's constants (rf_fft.hip, plan_fft: a line budget of 2048 values
# per workgroup, TC <= 16, grids capped at 4096, lines <= 4096, direct lines <= 2048); if those change, these change with them.
FFT_LINE_CASES = {
    # long radix-2 lines: 12 stages and the largest LDS request; wf = 2049 = 128 * 16 + 1, so the last column tile holds one column
    "r2_row4096": ((2, 64, 4096), dict(log2w=12, log2h=6, L=1, TC=16, trips=(1, 1))),
    "r2_col4096": ((2, 4096, 64), dict(log2w=6, log2h=12, L=32, TC=1, trips=(1, 1))),
    "r2_512x1024": ((1, 512, 1024), dict(log2w=10, log2h=9, L=2, TC=4, trips=(1, 1))),
    # long direct lines: the LL band of a padded SID frame (packed 1424 x 2144); the longest direct row; the longest direct column, odd
    "direct_712x1072": ((1, 712, 1072), dict(log2w=-1, log2h=-1, L=1, TC=2, trips=(1, 1))),
    "direct_row2046": ((1, 90, 2046), dict(log2w=-1, log2h=-1, L=1, TC=16, trips=(1, 1))),
    "direct_col2047": ((1, 2047, 6), dict(log2w=-1, log2h=-1, L=341, TC=1, trips=(1, 1))),
    "mixed_256x288": ((1, 256, 288), dict(log2w=-1, log2h=8, L=7, TC=8, trips=(1, 1))),
    # second trips: 5120 row groups on a grid of 4096 (some workgroups take two lines, some one); 460 * 9 = 4140 column tiles on a
    # grid of 4096; 16 405 rows in groups of 4, so that the last group (of the second trip) has one live line, with direct columns
    "row_trip2": ((5, 1024, 2048), dict(log2w=11, log2h=10, L=1, TC=2, trips=(2, 1))),
    "col_trip2": ((460, 2048, 16), dict(log2w=4, log2h=11, L=128, TC=1, trips=(2, 2))),
    "ragged_trip2": ((17, 965, 512), dict(log2w=9, log2h=-1, L=4, TC=2, trips=(2, 1))),
    # small edges: all four bins real; an odd height of 3 (no 2 y == h bins); odd direct height; a height of 2 under the longest row
    "edge_2x2": ((3, 2, 2), dict(log2w=1, log2h=1, L=1024, TC=16, trips=(1, 1))),
    "edge_3x4": ((2, 3, 4), dict(log2w=2, log2h=-1, L=512, TC=16, trips=(1, 1))),
    "edge_15x22": ((1, 15, 22), dict(log2w=-1, log2h=-1, L=93, TC=16, trips=(1, 1))),
    "edge_2x4096": ((1, 2, 4096), dict(log2w=12, log2h=1, L=1, TC=16, trips=(1, 1))),
}


def fft_plan(planes, h, w):
    """rf_fft_plan as a dict (include/rawformer_hip.h); raises RuntimeError with the library's message for refused sizes."""
    import ctypes as C
    from bayer_low_light_image_enhancement_amd import _lib
    out = (C.c_int * 10)()
    _lib.check(_lib.load().rf_fft_plan(planes, h, w, out), "rf_fft_plan")
    l2w, l2h, L, tc, gx, gy, trips_r, trips_c, lds_r, lds_c = out
    return dict(log2w=l2w, log2h=l2h, L=L, TC=tc, grid=(gx, gy), trips=(trips_r, trips_c), lds=(lds_r, lds_c))


def fake_addresses(nbytes):
    """One fake device address per byte size: page aligned, in the order given, a free page between neighbours.  For the host-side
    refusal tests, whose calls are turned away before anything is dereferenced but compare the byte ranges of their arguments."""
    out, at = [], 1 << 30
    for n in nbytes:
        out.append(at)
        at += (n + 4095) // 4096 * 4096 + 4096
    return out
