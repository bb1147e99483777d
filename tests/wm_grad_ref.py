"""Gradients of the WM block for tests/test_wm_backward.py: ``torch.autograd.grad`` of the loss ``<wm(x, p), g>`` with respect to
``x`` and the 17 parameter tensors.

``wm`` is ``mamba_ref.wm`` (the same operations in the same order: without a defect it equals it to 1e-12 in float64, which the
test asserts) built on ``mamba_grad_ref.mamba``, with detach points, so that autograd yields the gradients a backward with one
deliberate error would produce -- the forward VALUE is the same with every defect:

``"no_skip"``            ``+ x.detach()``: the residual carries no gradient
``"relu_passthrough"``   ``a + (relu(a) - a).detach()``: ReLU's derivative taken as 1
``"ln_no_projection"``   mean and variance detached: the two projection terms of the LayerNorm adjoint are dropped
``"tokens_as_permute"``  the value of ``tok``, with the gradient routed through ``LN(t.reshape(n, c, L).permute(0, 2, 1))`` as if a
                         token were a pixel's channel vector (the same thing at L = 1, where it does not apply)
``"cut_adjoint"``        mamba_grad_ref's: the adjoint of the scan does not cross a chunk boundary
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import mamba_grad_ref as G
import mamba_ref as M

KEYS = (("convb.0.weight", "convb.0.bias", "convb.2.weight", "convb.2.bias", "ln.weight", "ln.bias")
        + tuple("model1." + k for k in G.KEYS) + ("smooth.weight", "smooth.bias"))
DEFECTS = ("no_skip", "relu_passthrough", "ln_no_projection", "tokens_as_permute", "cut_adjoint")
EPS = 1e-5


def wm(x, p, pre: str = "", defect: str | None = None, chunk: int = 0, keep: dict | None = None):
    """``keep``: receives the intermediate ``r`` (the LayerNorm input as [n, c, h, w]) so that a caller can differentiate by it."""
    assert defect is None or defect in DEFECTS, defect
    n, c, h, w = x.shape
    a = F.conv2d(x, p[pre + "convb.0.weight"], p[pre + "convb.0.bias"], padding=1)
    t = F.relu(a)
    if defect == "relu_passthrough":
        t = a + (t - a).detach()
    t = F.conv2d(t, p[pre + "convb.2.weight"], p[pre + "convb.2.bias"], padding=1) + (x.detach() if defect == "no_skip" else x)
    if keep is not None:
        keep["r"] = t
    lw, lb = p[pre + "ln.weight"], p[pre + "ln.bias"]
    rows = M.wm_tokens(t)
    if defect == "ln_no_projection":
        mean = rows.mean(-1, keepdim=True).detach()
        var = rows.var(-1, unbiased=False, keepdim=True).detach()
        tok = (rows - mean) / torch.sqrt(var + EPS) * lw + lb
    else:
        tok = F.layer_norm(rows, (c,), lw, lb, EPS)
        if defect == "tokens_as_permute":
            alt = F.layer_norm(t.reshape(n, c, h * w).permute(0, 2, 1), (c,), lw, lb, EPS)
            tok = alt + (tok - alt).detach()
    y = G.mamba(tok, p, pre + "model1.", "cut_adjoint" if defect == "cut_adjoint" else None, chunk)
    y = y.permute(0, 2, 1).reshape(n, c, h, w)
    return F.conv2d(y, p[pre + "smooth.weight"], p[pre + "smooth.bias"], padding=1)


def gradients(x, p, g, defect: str | None = None, chunk: int = 0):
    """``({"x": dL/dx, name: dL/dp[name]}, dL/dr)`` of ``L = <wm(x, p), g>`` in the dtype of the inputs."""
    x = x.detach().clone().requires_grad_(True)
    q = {k: p[k].detach().clone().requires_grad_(True) for k in KEYS}
    keep = {}
    loss = (wm(x, q, "", defect, chunk, keep) * g).sum()
    got = torch.autograd.grad(loss, [x] + [q[k] for k in KEYS] + [keep["r"]])
    return dict(zip(("x",) + KEYS, (t.detach() for t in got[:-1]))), got[-1].detach()
