#!/usr/bin/env python3
"""``tests/golden/wfb_ffn_train.npz``: the reference's own ``RawFomer_WFB_FFAB/model.py`` ``FeedForward`` RUN in ``.train()`` on the
CPU (nothing of it is copied), in float64 and in float32, on two cases of tests/wfb_ffn_grad_ref.py (``base`` and ``odd``).

Per case and dtype (``<tag>.f64.`` / ``<tag>.f32.``): the output ``y``; the autograd gradients of ``<y, g>`` with respect to ``x``
(``grad.x``) and the 12 parameters (``grad.<state_dict key>``); the four running statistics and ``num_batches_tracked`` of both
BatchNorms after the call.  Inputs and weights are ``wfb_ffn_grad_ref.inputs(tag)``: both sides regenerate them.
tests/test_wfb_ffn_train.py holds the restatement against the float64 half to 1e-12.

Usage:  python tools/make_golden_wfb_ffn_train.py [--reference DIR]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.dont_write_bytecode = True

from oracle import make_golden as G  # noqa: E402
from make_golden_wfb import import_reference  # noqa: E402
import wfb_ffn_grad_ref as R  # noqa: E402

TAGS = ("base", "odd")
NBT = ("rep_conv1.bn.num_batches_tracked", "rep_conv2.bn.num_batches_tracked")


def run(ref, tag, dtype):
    x, g, p = R.inputs(tag)
    (_, dim, hidden, _, _), _ = R.CASES[tag]
    m = ref.FeedForward(dim, hidden / dim, True)
    state = {k: v.clone() for k, v in p.items()}
    state.update({k: torch.zeros((), dtype=torch.int64) for k in NBT})
    m.load_state_dict(state, strict=True)
    m = m.to(dtype).train()
    x = x.to(dtype).requires_grad_(True)
    y = m(x)
    assert m.training and y.dtype == dtype
    named = dict(m.named_parameters())
    assert set(named) == set(R.KEYS)
    grads = torch.autograd.grad((y * g.to(dtype)).sum(), [x] + [named[k] for k in R.KEYS])
    out = {"y": y.detach(), "grad.x": grads[0]}
    out.update({"grad." + k: t for k, t in zip(R.KEYS, grads[1:])})
    after = m.state_dict()
    out.update({k: after[k].detach().clone() for k in R.BUFFERS + NBT})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF, help="directory of the reference project")
    args = ap.parse_args()
    ref = import_reference(args.reference)
    out = {}
    for tag in TAGS:
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            res = run(ref, tag, dtype)
            out.update({f"{tag}.{name}.{k}": v for k, v in res.items()})
        floor = max(G.maxabs(out[f"{tag}.f32.{k}"].double(), out[f"{tag}.f64.{k}"]) / float(out[f"{tag}.f64.{k}"].abs().max())
                    for k in ["y", "grad.x"] + ["grad." + k for k in R.KEYS if k != R.W2])
        print(f"{tag}: reference f32 against f64, largest max|diff| / max|f64| over y and the gradients (d {R.W2} apart): {floor:.3e}")
    G.save("wfb_ffn_train", **out)


if __name__ == "__main__":
    main()
