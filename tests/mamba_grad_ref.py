"""Gradients of the Mamba module for tests/test_mamba_backward.py: ``torch.autograd.grad`` of the loss ``<mamba(u, p), g>`` with
respect to ``u`` and the nine parameter tensors.

``mamba`` is a copy of ``mamba_ref.mamba`` (the same operations in the same order: without a defect it equals it to 1e-12 in
float64, which the test asserts) with detach points, so that autograd yields the gradients a backward with one deliberate error
would produce -- the forward VALUE is the same with every defect:

``"cut_adjoint"``        ``h = h.detach()`` at every multiple of ``chunk`` tokens: the adjoint does not cross a chunk boundary
``"straight_softplus"``  ``delta = pre + (softplus(pre) - pre).detach()``: softplus' derivative taken as 1
``"dead_gate"``          ``silu(z).detach()``: no gradient through the gate
``"first_tile_bc"``      ``Bm``, ``Cm`` detached where they feed the channels from 64 on: the sum of dBm / dCm over the channel
                         tiles keeps its first tile only
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

KEYS = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
        "out_proj.weight")
DEFECTS = ("cut_adjoint", "straight_softplus", "dead_gate", "first_tile_bc")
TILE = 64


def mamba(u, p, pre: str = "", defect: str | None = None, chunk: int = 0):
    assert defect is None or defect in DEFECTS, defect
    l = u.shape[1]
    di = p[pre + "D"].shape[0]
    n = p[pre + "A_log"].shape[1]
    k = p[pre + "conv1d.weight"].shape[2]
    r = p[pre + "dt_proj.weight"].shape[1]
    xz = u @ p[pre + "in_proj.weight"].t()
    x, z = xz[..., :di], xz[..., di:]
    xp = F.pad(x, (0, 0, k - 1, 0))
    xc = p[pre + "conv1d.bias"] + sum(p[pre + "conv1d.weight"][:, 0, j] * xp[:, j:j + l] for j in range(k))
    xc = F.silu(xc)
    dbc = xc @ p[pre + "x_proj.weight"].t()
    dt, bm, cm = dbc[..., :r], dbc[..., r:r + n], dbc[..., r + n:]
    pre_act = dt @ p[pre + "dt_proj.weight"].t() + p[pre + "dt_proj.bias"]
    delta = F.softplus(pre_act)
    if defect == "straight_softplus":
        delta = pre_act + (delta - pre_act).detach()
    A = -torch.exp(p[pre + "A_log"])
    bm_d, cm_d = bm[:, :, None, :], cm[:, :, None, :]                 # [B, L, 1 -> Di, N]
    if defect == "first_tile_bc":
        far = (torch.arange(di) >= TILE)[None, None, :, None]
        bm_d, cm_d = torch.where(far, bm_d.detach(), bm_d), torch.where(far, cm_d.detach(), cm_d)
    h = delta.new_zeros(u.shape[0], di, n)
    hs = []
    for t in range(l):
        if defect == "cut_adjoint" and t and t % chunk == 0:
            h = h.detach()
        dl = delta[:, t]
        h = torch.exp(dl[:, :, None] * A) * h + (dl * xc[:, t])[:, :, None] * bm_d[:, t]
        hs.append(h)
    h = torch.stack(hs, dim=1)
    y = (h * cm_d).sum(-1) + p[pre + "D"] * xc
    gate = F.silu(z)
    if defect == "dead_gate":
        gate = gate.detach()
    return (y * gate) @ p[pre + "out_proj.weight"].t()


def gradients(u, p, g, defect: str | None = None, chunk: int = 0):
    """``{"u": dL/du, name: dL/dp[name]}`` of ``L = <mamba(u, p), g>`` in the dtype of the inputs."""
    u = u.detach().clone().requires_grad_(True)
    q = {k: p[k].detach().clone().requires_grad_(True) for k in KEYS}
    loss = (mamba(u, q, "", defect, chunk) * g).sum()
    got = torch.autograd.grad(loss, [u] + [q[k] for k in KEYS])
    return dict(zip(("u",) + KEYS, (t.detach() for t in got)))
