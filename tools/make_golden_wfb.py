#!/usr/bin/env python3
"""Fixtures of ``RawFormer(variant='wfb')`` by RUNNING the reference's own ``RawFomer_WFB_FFAB/model.py`` ``RawFormer`` on the CPU
(nothing of it is copied), in ``.eval()`` with non-trivial BatchNorm statistics:

* ``tests/golden/wfb.npz``: the reference's float32 outputs of the whole-model cases, their float64 checksums, and per case the
  reference's own float32-against-float64 error (the float32 floor);
* ``tests/golden/wfb_state_dict_keys.json``: the reference's ``state_dict`` keys, shapes and dtypes at dim 16;
* ``tests/golden/PINNING_wfb.txt``: what the fixture pins and what it does not, the floors and the bounds derived from them.

``mamba_ssm`` is not installed, so ``mamba_ssm.Mamba`` is bound to a module here whose parameters have the names and shapes of
``ops.mamba_param_shapes`` and whose forward is ``tests/mamba_ref.mamba``: the fixture pins the reference's WIRING with the
RESTATED Mamba, not parity with the package.  ``ptflops`` and ``timm`` (imported, never used on this path) are inert stubs.

Weights are ``tests/wfb_ref.synth_state`` values by name, inputs ``synth`` mosaics: both sides regenerate them.

Usage:  python tools/make_golden_wfb.py [--reference DIR]
"""
import argparse
import importlib.util
import json
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

from bayer_low_light_image_enhancement_amd import ops, synth  # noqa: E402
from oracle import make_golden as G  # noqa: E402
import mamba_ref  # noqa: E402
import wfb_ref  # noqa: E402

# tag, dim, batch, mosaic height, width, input seed: the smallest power-of-two sizes the model admits (packed 32 x 32).  The seeds
# are the first whose frames keep every FFT bin of every FEB at least 8 float32 perturbations away from the branch cut of `angle`
# (wfb_ref.branch_cut_margins, printed below): closer than that a float32 forward has no single answer.
CASES = (("wfb_d16_b1_64x64", 16, 1, 64, 64, 77), ("wfb_d16_b2_64x128", 16, 2, 64, 128, 95))
WEIGHT_SEED = 6000      # + dim


class Mamba(nn.Module):
    """Stand-in for ``mamba_ssm.Mamba``: the parameters of ``ops.mamba_param_shapes``, the forward of ``mamba_ref.mamba``."""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2):
        super().__init__()
        for key, shape in ops.mamba_param_shapes(d_model, d_state, d_conv, expand).items():
            *path, leaf = key.split(".")
            mod = self
            for part in path:
                if part not in mod._modules:
                    mod.add_module(part, nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(shape)))

    def forward(self, u):
        return mamba_ref.mamba(u, dict(self.state_dict()), "")


def import_reference(ref_dir):
    G.stub("ptflops", get_model_complexity_info=None)
    G.stub("timm")
    G.stub("timm.models")
    G.stub("timm.models.vision_transformer", VisionTransformer=object, _cfg=None)
    G.stub("timm.models.registry", register_model=lambda f: f)
    G.stub("timm.models.layers", trunc_normal_=None, DropPath=None, to_2tuple=None)
    G.stub("mamba_ssm", Mamba=Mamba)
    wfb_dir = os.path.join(ref_dir, "RawFomer_WFB_FFAB")
    sys.path.insert(0, wfb_dir)      # its `import blocks`
    spec = importlib.util.spec_from_file_location("wfb_reference_model", os.path.join(wfb_dir, "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(ref, dim):
    m = ref.RawFormer(dim=dim).eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(wfb_ref.synth_state(shapes, WEIGHT_SEED + dim), strict=True)
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF, help="directory of the reference project")
    args = ap.parse_args()
    ref = import_reference(args.reference)
    pin = ["wfb fixtures (tools/make_golden_wfb.py): the reference's RawFomer_WFB_FFAB RawFormer on the CPU, eval mode, torch " + torch.__version__,
           "",
           "What is pinned: the reference's WIRING -- the U-Net, Conv_Transformer, WMB (LayerNorm, DWT, Illumination_Estimator, FFAB, WM, IWT),",
           "FeedForward with its BatchNorms on running statistics (running_mean of either sign, running_var in [0.5, 2]) -- executed by the",
           "reference's own classes, with mamba_ssm.Mamba bound to a module that evaluates the RESTATED Mamba of tests/mamba_ref.py.",
           "What is NOT pinned: parity with the mamba_ssm package (not installed), and therefore also the order of the keys under",
           "mb.model1. / mb.model2. inside the state_dict: their names and shapes are those of ops.mamba_param_shapes and the tests",
           "compare them as a set.", ""]
    out = {}
    for tag, dim, b, hh, ww, seed in CASES:
        m = build(ref, dim)
        x = G.t(synth.bayer_mosaic(seed, b, hh, ww))
        sd = G.sd_of(m)
        with torch.no_grad():
            y = m(x)
            mine = wfb_ref.forward(sd, x)
            y64 = m.double()(x.double())
            mine64 = wfb_ref.forward({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}, x.double())
            m.float()
        assert not m.training and y64.dtype == torch.float64
        floor, d32, d64 = G.maxabs(y.double(), y64), G.maxabs(y, mine), G.maxabs(y64, mine64)
        margin, where = wfb_ref.branch_cut_margins(lambda p, xx: wfb_ref.forward(p, xx), sd, x)
        pin.append(f"{tag}: dim {dim}, mosaic {b}x{hh}x{ww}: reference f32 vs f64 (the float32 floor) {floor:.3e}; tests/wfb_ref.py vs reference "
                   f"f32 {d32:.3e}, f64 vs f64 {d64:.3e}; output mean {float(y.mean()):.4f}, max {float(y.max()):.4f}, "
                   f"clamped to 0: {float((y == 0).float().mean()):.3f}, to 1: {float((y == 1).float().mean()):.3f}; "
                   f"nearest FFT bin to the branch cut of angle: {margin:.1f} float32 perturbations ({where[0]} at {where[1]}x{where[2]})")
        assert margin >= 8.0, margin
        assert d64 < 1e-9, d64      # float64 against float64: the two differ by summation order alone
        out[f"{tag}.out"], out[f"{tag}.floor"] = y, torch.tensor(floor, dtype=torch.float64)
        out[f"{tag}.checksum_fp64"] = torch.tensor(float(y64.sum()), dtype=torch.float64)
    G.save("wfb", **out)
    keys = {"16": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in ref.RawFormer(dim=16).state_dict().items()]}
    with open(os.path.join(G.GOLD, "wfb_state_dict_keys.json"), "w") as f:
        json.dump(keys, f)
    pin += ["", "tests/test_wfb_model.py, CPU: wfb_ref in float32 against wfb.npz within 4 x the case's floor above (two CPU implementations of one",
            "float32 forward differ by summation order; 4 x is the rule of PINNING_multilvl.txt).",
            "GPU: truth is wfb_ref in float64 and the bound e64 <= 8 e32 + 2e-6 max|ref| (tests/test_mamba.py); against wfb.npz the whole-model",
            "tolerance 5e-5 of DESIGN.md section 2.",
            "", "Conditioning: FEB's angle() jumps by 2 pi where a bin with a negative real part has a zero imaginary part, and the phase feeds a 1x1",
            "MLP.  A frame that puts a bin within float32's perturbation of that cut has two float32 answers (mosaic seed 71 at 1x64x64 is one:",
            "conv_tran7 ... ffab.conv4.0, |Im F| / |F| = 3.1e-7, and the MI355X forward lands on the other side of it, 3.2e-3 from float64).",
            "Every case here and in the tests keeps 8 perturbations of distance -- the factor the GPU bound grants over e32 -- checked from",
            "the float32 and float64 restatements alone (test_cases_stay_clear_of_the_phase_branch_cut)."]
    with open(os.path.join(G.GOLD, "PINNING_wfb.txt"), "w") as f:
        f.write("\n".join(pin) + "\n")
    print("\n".join(pin))


if __name__ == "__main__":
    main()
