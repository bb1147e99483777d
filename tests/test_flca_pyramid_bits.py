"""The bits of ``ops.flca_pyramid`` / ``ops.flca_pyramid_backward`` and of two ``ops.flca`` forwards, and the two workspace sizes of
the pyramid, against tests/golden/flca_pyramid_parent.json: recorded on an MI355X with tools/record_flca_pyramid_golden.py at the
commit before the FLCA adjoints were made to share their tap-contraction step, their ``dch`` kernel and their squeeze-excite MLP
(csrc/rf_flca_adjoint.h).  That change keeps every sum and every fmaf chain in its order: no bit may move, and there is no
tolerance.  ``record`` / ``digest`` are those of tests/test_train_bits.py, whose two FLCA cases cover the base backward.

Pyramid cases: rows of ``flca_pyramid_grad_ref.CASES`` with ``inputs(tag)``; per case the output of ``ops.flca_pyramid``, ``grad_feat``
("feat") and every parameter gradient of ``ops.flca_pyramid_backward``.  What each is here for:

==========  ==============================================================================================================
base        the MFMA tap kernel, the fused forward
odd         every scalar form; channel tiles of 16 and 8
w_mod4_2    the scalar tap kernel beside the float4 kernels
levels3     four steps, both CHROMA forms
c512        two passes over the channels in the squeeze-excite kernel, hidden = 64
blocks      five slabs per image, two ``dch`` blocks
deep        eight channel tiles
==========  ==============================================================================================================

``ops.flca`` forward cases, for flca_se_kernel (inputs from ``cases.rnd`` / ``cases.params`` with the seeds below):

===============  =========================================================================================================
flca_c16_16x16   (2, 16, 16, 16), packed 16 x 16: sixteen slices of the column sum side by side (nsl = 16)
flca_c512_2x4    (1, 512, 2, 4), packed 16 x 32: two passes over the channels (c0 = 0, 256), one slice each
===============  =========================================================================================================

Sizes: ``rf_flca_pyramid_workspace_bytes`` and ``rf_flca_pyramid_backward_workspace_bytes`` of all 12 rows of ``CASES``, compared
without a device (the library loads without one).
"""
import json
import os

import pytest
import torch

import cases
import flca_pyramid_grad_ref as G
from test_train_bits import record

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flca_pyramid_parent.json")
PYR_CASES = ["base", "odd", "w_mod4_2", "levels3", "c512", "blocks", "deep"]
# id: (B, C, h, w, H, W, seed)
FLCA_CASES = {"flca_c16_16x16": (2, 16, 16, 16, 16, 16, 6300), "flca_c512_2x4": (1, 512, 2, 4, 16, 32, 6301)}
CASE_IDS = PYR_CASES + list(FLCA_CASES)


def run_pyramid_case(tag, device):
    from bayer_low_light_image_enhancement_amd import ops
    feat, x4, p, g = G.inputs(tag)
    levels = G.CASES[tag][4]
    p = {k: v.to(device) for k, v in p.items()}
    feat, x4, g = feat.to(device), x4.to(device), g.to(device)
    out = ops.flca_pyramid(feat, x4, p, levels=levels)
    dx, grads = ops.flca_pyramid_backward(feat, x4, p, g, levels=levels)
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy(), "feat": dx.cpu().numpy(), **{k: v.cpu().numpy() for k, v in grads.items()}}


def run_flca_case(tag, device):
    from bayer_low_light_image_enhancement_amd import ops
    b, c, h, w, H, W, seed = FLCA_CASES[tag]
    assert (c > 256) == (tag == "flca_c512_2x4") and 256 // min(c, 256) == (1 if c > 256 else 16)
    p = {k: v.to(device) for k, v in cases.params(cases.flca_spec(c), seed=seed).items()}
    feat = cases.rnd(f"pyr_bits.{tag}.feat", (b, c, h, w), seed=seed).to(device)
    x4 = cases.rnd(f"pyr_bits.{tag}.x4", (b, 4, H, W), 0.0, 1.0, seed=seed).to(device)
    out = ops.flca(feat, x4, p)
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy()}


def run_case(tag, device):
    """name -> array of everything the case digests."""
    return run_flca_case(tag, device) if tag in FLCA_CASES else run_pyramid_case(tag, device)


def workspace_bytes():
    """tag -> [forward, backward] workspace bytes of every row of CASES; needs the library, no device."""
    from bayer_low_light_image_enhancement_amd import _lib
    lib = _lib.load()
    return {tag: [int(lib.rf_flca_pyramid_workspace_bytes(b, c, h, w, H, W, L)), int(lib.rf_flca_pyramid_backward_workspace_bytes(b, c, h, w, H, W, L))]
            for tag, (b, c, h, w, L, H, W) in G.CASES.items()}


def test_workspace_sizes_of_the_parent():
    with open(FIXTURE) as f:
        want = json.load(f)["workspace_bytes"]
    got = workspace_bytes()
    assert len(got) == 12 and set(got) == set(want)
    for tag in got:
        assert 0 < got[tag][0] < got[tag][1], (tag, got[tag])
        assert got[tag] == want[tag], f"[{tag}] workspace bytes (forward, backward) now {got[tag]}, recorded {want[tag]}"


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
