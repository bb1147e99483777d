"""GPU: ops.channel_attention at the shapes where attn_mid_kernel<64|128> and attn_fold_kernel change path, against
(i) the digests of tests/golden/attn_mid_parent.json, recorded on an MI355X with tools/record_attn_mid_golden.py at the commit
before the per-step bookkeeping of attn_mid_kernel was cut and the passes of attn_fold_kernel were made to run side by side:
neither change may move a bit (same partial layout, same order of every sum), and
(ii) the CPU oracle, at the tolerance of test_gpu_ops.py::test_channel_attention_oracle.

The plan arithmetic is attn_mid_plan's: per = ntiles / 64 clamped to 1..8 over tiles of 4 x 64 px numbered down the columns,
nslab = ceil(ntiles / per), and rgroups = 3 when nslab * B < 256.

  C   B  h x w       reaches
  64  1  6 x 72      4 tiles, ragged in both directions, rgroups = 3
  64  4  130 x 256   132 tiles, per = 2, 264 workgroups -> rgroups = 1; sliding row window; slab 16 holds tiles 32 and 33, the
                     last tile of column 0 and the first of column 1 (full restage); ragged last tile row
  64  1  130 x 256   the same plan with rgroups = 3
  128 2  10 x 136    9 tiles, per = 1, ragged; fold at c = 16 (RS = 1, two passes)
  128 4  260 x 128   130 tiles, per = 2, rgroups = 1; slab 32 holds tiles 64 and 65 and crosses a column
  256 1  8 x 8       the gram_kernel path; fold at c = 32 (five passes)
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

HEADS = 8
SEED = 20240917
CASES = [(64, 1, 6, 72), (64, 4, 130, 256), (64, 1, 130, 256), (128, 2, 10, 136), (128, 4, 260, 128), (256, 1, 8, 8)]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_mid_parent.json")
SAMPLES = 8


def case_id(case):
    return "C{}_B{}_{}x{}".format(*case)


def make_inputs(case):
    """x and the seven parameters of Attention(C, heads), from a CPU generator seeded by the case alone: conv weights uniform
    with variance 1 / fan_in, biases in +-0.1, temperature in [0.5, 2) -- the magnitudes of synth.param_values."""
    c, b, h, w = case
    gen = torch.Generator(device="cpu")
    gen.manual_seed(SEED + 1000003 * c + 10007 * b + 101 * h + w)

    def u(shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float32)

    def conv(shape):
        bound = (3.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        return u(shape, -bound, bound)

    x = u((b, c, h, w), -1.0, 1.0)
    ps = [conv((3 * c, c, 1, 1)), u((3 * c,), -0.1, 0.1), conv((3 * c, 1, 3, 3)), u((3 * c,), -0.1, 0.1),
          u((HEADS, 1, 1), 0.5, 2.0), conv((c, c, 1, 1)), u((c,), -0.1, 0.1)]
    return x, ps


def run_case(case, device):
    from bayer_low_light_image_enhancement_amd import ops
    x, ps = make_inputs(case)
    out = ops.channel_attention(x.to(device), *[p.to(device) for p in ps], HEADS)
    return out.cpu().contiguous().numpy()


def sample_index(n):
    return [int(i) for i in np.linspace(0, n - 1, SAMPLES).astype(np.int64)]


def digest(out):
    return hashlib.sha256(np.ascontiguousarray(out, dtype="<f4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def outputs(device):
    return {case: run_case(case, device) for case in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits_of_the_parent(outputs, case):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][case_id(case)]
    out = outputs[case]
    assert list(out.shape) == want["shape"]
    flat = out.reshape(-1)
    got = [float(flat[i]).hex() for i in sample_index(flat.size)]
    assert digest(out) == want["sha256"], f"output bits moved; samples now {got}, recorded {want['samples']}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle(outputs, case):
    from oracle import rawformer_ref as R
    from test_gpu_ops import close
    x, ps = make_inputs(case)
    close(outputs[case], R.channel_attention(x, *ps, HEADS))
