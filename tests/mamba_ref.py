"""Plain-torch restatement of the Mamba forward, the WM block and the complete WMB block of the WFB variant
(RawFomer_WFB_FFAB/model.py:138-172, 203-245), written from the equations of the module
``mamba_ssm.modules.mamba_simple.Mamba(d_model, d_state, d_conv, expand)`` with its defaults (dt_rank = ceil(d_model / 16),
no projection biases, conv1d bias):

    [x ; z]      = in_proj(u)
    x_t          = silu(conv1d.bias + sum_k conv1d.weight[:, 0, k] x_{t-(K-1)+k})         x_s = 0 for s < 0
    [dt; Bm; Cm] = x_proj(x_t)
    delta_t      = softplus(dt_proj.weight dt_t + dt_proj.bias)
    h_t[d, n]    = exp(delta_t[d] A[d, n]) h_{t-1}[d, n] + delta_t[d] Bm_t[n] x_t[d]      A = -exp(A_log), h_{-1} = 0
    y_t[d]       = sum_n Cm_t[n] h_t[d, n] + D[d] x_t[d]
    out_t        = out_proj(y_t silu(z_t))

Everything works in the dtype of its inputs (float64 in, float64 out); the recurrence is an explicit loop over t.  The package
itself is absent here, so parity with IT is unpinned; what these functions pin is the arithmetic above.

``defect`` evaluates the same forward with one deliberate error, for tests that have to show their bound would see it:
``"zero_state"`` (the state is zeroed at every multiple of ``chunk`` tokens, i.e. every chunk starts from nothing),
``"shift_taps"`` (the convolution taps reach one token further back) and ``"no_dt_bias"`` (dt_proj.bias dropped).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import rawformer_ref as R


def scan_states(delta, A, Bm, x, zero_every: int = 0):
    """h_t for every t as ``[B, L, Di, N]``: delta, x ``[B, L, Di]``, A ``[Di, N]``, Bm ``[B, L, N]``.  The loop over t."""
    b, l, di = delta.shape
    h = delta.new_zeros(b, di, A.shape[1])
    out = []
    for t in range(l):
        if zero_every and t % zero_every == 0:
            h = torch.zeros_like(h)
        dl = delta[:, t]
        h = torch.exp(dl[:, :, None] * A) * h + (dl * x[:, t])[:, :, None] * Bm[:, t][:, None, :]
        out.append(h)
    return torch.stack(out, dim=1)


def mamba(u, p, pre: str = "", defect: str | None = None, chunk: int = 0):
    """Mamba.forward on ``u [B, L, D]`` from the module's state_dict entries ``p[pre + name]``."""
    l = u.shape[1]
    di = p[pre + "D"].shape[0]
    n = p[pre + "A_log"].shape[1]
    k = p[pre + "conv1d.weight"].shape[2]
    r = p[pre + "dt_proj.weight"].shape[1]
    xz = u @ p[pre + "in_proj.weight"].t()
    x, z = xz[..., :di], xz[..., di:]
    back = k - 1 + (1 if defect == "shift_taps" else 0)
    xp = F.pad(x, (0, 0, back, 0))                                   # zeros in front of token 0: causal
    xc = p[pre + "conv1d.bias"] + sum(p[pre + "conv1d.weight"][:, 0, j] * xp[:, j:j + l] for j in range(k))
    xc = F.silu(xc)
    dbc = xc @ p[pre + "x_proj.weight"].t()
    dt, bm, cm = dbc[..., :r], dbc[..., r:r + n], dbc[..., r + n:]
    pre_act = dt @ p[pre + "dt_proj.weight"].t()
    if defect != "no_dt_bias":
        pre_act = pre_act + p[pre + "dt_proj.bias"]
    delta = F.softplus(pre_act)                                      # torch softplus: the identity above 20
    h = scan_states(delta, -torch.exp(p[pre + "A_log"]), bm, xc, zero_every=chunk if defect == "zero_state" else 0)
    y = (h * cm[:, :, None, :]).sum(-1) + p[pre + "D"] * xc
    return (y * F.silu(z)) @ p[pre + "out_proj.weight"].t()


def wm_tokens(x):
    """The tokens WM hands to Mamba (model.py:168): ``x.reshape(n, -1, c)`` of the contiguous NCHW tensor -- token i is the run
    ``flat[i c : (i + 1) c]`` of an image's memory, not a permutation of its axes."""
    n, c = x.shape[:2]
    return x.contiguous().reshape(n, -1, c)


def wm(x, p, pre: str = "", defect: str | None = None, chunk: int = 0):
    """WM.forward (model.py:165-172); ``model2`` and ``softmax`` are constructed by the reference and never called."""
    n, c, h, w = x.shape
    t = F.relu(F.conv2d(x, p[pre + "convb.0.weight"], p[pre + "convb.0.bias"], padding=1))
    t = F.conv2d(t, p[pre + "convb.2.weight"], p[pre + "convb.2.bias"], padding=1) + x
    tok = F.layer_norm(wm_tokens(t), (c,), p[pre + "ln.weight"], p[pre + "ln.bias"], 1e-5)
    y = mamba(tok, p, pre + "model1.", defect, chunk).permute(0, 2, 1).reshape(n, c, h, w)
    return F.conv2d(y, p[pre + "smooth.weight"], p[pre + "smooth.bias"], padding=1)


def wmb(x, p, pre: str = "", defect: str | None = None, chunk: int = 0):
    """WMB.forward (model.py:215-245), eval mode: the wavelet branch with ``mb`` = WM on the high bands, then
    ``x + ffn(norm2(x))`` (FeedForward adds its own input once more, model.py:59-65)."""
    t = R.wmb_ll_branch(x, p, pre, high=lambda hi: wm(hi, p, pre + "mb.", defect, chunk))
    y = R.layernorm2d(t, p[pre + "norm2.body.weight"], p[pre + "norm2.body.bias"])
    return t + R.wfb_feed_forward(y, p, pre + "ffn.")
