"""GPU: the bits of one ``rf_train_step`` (loss, prediction, the whole flat gradient buffer) and of two backward operators,
against the digests of tests/golden/train_step_parent.json, recorded on an MI355X with tools/record_train_step_golden.py at the
commit before the training kernels were cleaned up (unreachable adjoint paths deleted, one block reduction, the FLCA backward
in its own file).  Those changes keep every sum in its order: no bit may move, and there is no tolerance.

Training cases: rows of tests/test_train_shapes.py::CASES, built by the builder of tests/test_train_clamp.py with the same
seeds.  What each is here for:

==============================  ===========================================================================================
d24_flca_charb_ffn4_pool        generic LayerNorm path (C = 24: ln_bwd_kernel / ln_wgrad_kernel, the residual copied by the
                                EW_COPY pass), split_halves under FLCA, a partial FLCA pooling block, Charbonnier, masked
                                level 3
d24_plain_charb_b3              B = 3, the split two-source contraction, the plain branch
d16_plain_l1_ffn4_nonsquare     LeakyReLU on the branch (EW_LRELU_GRAD) and the L1 loss
d16_flca_l1_slabs_b1            several slabs per image in gram2 and in the fused FLCA kernel
d24_plain_charb_b3_24x32_io     the ``clamp_io`` case of tests/test_train_clamp.py under the clamped criterion (EW_CLAMP01)
==============================  ===========================================================================================

Operator cases, for kernels the training step does not reach:

==============================  ===========================================================================================
mamba_three_chunks              ops.mamba_backward at (3, 3 Lc + 5, 32) of tests/test_mamba_backward.py: a sequence length
                                that is no multiple of 4, chan_sum_kernel's scalar branch
wfb_ffn_w_mod4_2                ops.wfb_feed_forward_backward at (2, 16, 40, 6, 10) of tests/test_wfb_ffn_train.py: a width
                                that is no multiple of 4, dw_wgrad_kernel<1>
==============================  ===========================================================================================
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_parent.json")
SAMPLES = 8
# id, row of test_train_shapes.CASES, clamp_io, clamped criterion, seed (None: the row's)
TRAIN_CASES = [
    ("d24_flca_charb_ffn4_pool", "d24_flca_charb_ffn4_pool", False, False, None),
    ("d24_plain_charb_b3", "d24_plain_charb_b3", False, False, None),
    ("d16_plain_l1_ffn4_nonsquare", "d16_plain_l1_ffn4_nonsquare", False, False, None),
    ("d16_flca_l1_slabs_b1", "d16_flca_l1_slabs_b1", False, False, None),
    ("d24_plain_charb_b3_24x32_io", "d24_plain_charb_b3_24x32", True, True, 404),
]
OP_CASES = ["mamba_three_chunks", "wfb_ffn_w_mod4_2"]
CASE_IDS = [c[0] for c in TRAIN_CASES] + OP_CASES


def run_train_case(case, device):
    """{"loss", "pred", "grads"} of one training step, as numpy arrays."""
    from test_train_clamp import _inputs, _trainer
    tag, base, clamp_io, clamp_pred, seed = case
    cfg, sd, x, gt, loss = _inputs(base, clamp_io, seed)
    tr = _trainer(device, base, clamp_io, clamp_pred, sd)
    loss_dev, pred = tr.forward_backward(x.to(device), gt.to(device), want_pred=True)
    torch.cuda.synchronize()
    return {"loss": loss_dev.cpu().numpy(), "pred": pred.cpu().numpy(), "grads": tr.grads.cpu().numpy()}


def run_mamba_case(device):
    from bayer_low_light_image_enhancement_amd import ops
    import test_mamba_backward as T
    from test_mamba import lc, mamba_params
    tag = "three_chunks"
    shape_of, (dlo, dhi) = T.CASES[tag]
    shape, seed = shape_of(lc()), T.SEED + T.SEEDS[tag]
    assert shape[1] % 4 != 0
    p = {k: v.to(device) for k, v in mamba_params(shape[2], seed, dlo, dhi).items()}
    u = cases.rnd(f"mamba_bwd.{tag}.u", shape, seed=seed).to(device)
    g = cases.rnd(f"mamba_bwd.{tag}.g", shape, seed=seed).to(device)
    du, grads = ops.mamba_backward(u, p, g)
    torch.cuda.synchronize()
    return {"u": du.cpu().numpy(), **{k: v.cpu().numpy() for k, v in grads.items()}}


def run_wfb_ffn_case(device):
    from bayer_low_light_image_enhancement_amd import ops
    import wfb_ffn_grad_ref as G
    from test_wfb_ffn_train import NBT
    tag = "w_mod4_2"
    assert G.CASES[tag][0][4] % 4 != 0
    x, g, p = G.inputs(tag)
    p = {k: v.to(device) for k, v in p.items()}
    p.update({k: torch.zeros((), dtype=torch.int64, device=device) for k in NBT})
    dx, grads = ops.wfb_feed_forward_backward(x.to(device), p, g.to(device))
    torch.cuda.synchronize()
    return {"x": dx.cpu().numpy(), **{k: v.cpu().numpy() for k, v in grads.items()}}


def run_case(tag, device):
    """name -> array of everything the case digests."""
    if tag == "mamba_three_chunks":
        return run_mamba_case(device)
    if tag == "wfb_ffn_w_mod4_2":
        return run_wfb_ffn_case(device)
    return run_train_case(next(c for c in TRAIN_CASES if c[0] == tag), device)


def sample_index(n):
    return [int(i) for i in np.linspace(0, n - 1, min(SAMPLES, n)).astype(np.int64)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").tobytes()).hexdigest()


def record(arrays):
    """What the fixture keeps of a case: per array its shape, the SHA-256 of its bytes (little-endian float32) and a few values
    as hex floats, for diagnosis."""
    out = {}
    for k, a in arrays.items():
        flat = np.asarray(a).reshape(-1)
        out[k] = {"shape": list(np.asarray(a).shape), "sha256": digest(a), "samples": [float(flat[i]).hex() for i in sample_index(flat.size)]}
    return out


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
