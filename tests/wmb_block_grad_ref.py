"""The whole WMB block (RawFomer_WFB_FFAB/model.py:203-245) restated for autograd, eval and training mode, for
tests/test_wmb_backward.py: ``torch.autograd.grad`` of the loss ``<wmb(x, p), g>`` with respect to ``x`` and the block's 131 parameters.

``wmb`` is ``mamba_ref.wmb`` (the same operations in the same order) built from the restatements the pieces were tested against --
``R.layernorm2d`` / ``R.dwt_init``, ``wfb_ref.illu_fea``, ``ffab_grad_ref.ffab`` (the symmetric bins exact), ``wm_grad_ref.wm``,
``wmb_grad_ref.iwt`` and ``wfb_ffn_grad_ref.forward`` (``training=True``: the batch-statistics FeedForward; ``False``: the running
statistics) -- plain torch in the dtype of its inputs.  Two places where ``mamba_ref.wmb`` itself is not float64, and what the value test
does about them:

* ``R.iwt_init`` returns float32 whatever it is given (as blocks.py:126 does), so ``mamba_ref.wmb`` rounds the wavelet branch to float32
  once.  ``wmb(..., iwt=R.iwt_init)`` takes the same step and then equals it to 1e-12; the gradients use ``wmb_grad_ref.iwt``, which is
  ``R.iwt_init`` bit for bit in float32 (tests/test_wmb_pieces_backward.py) and float64 in float64.
* ``R.ffab`` leaves the CPU transform's rounding noise in the imaginary part of the bins that are real by symmetry, so ``angle`` of a
  negative real bin is +pi or -pi at random where a band side is no power of two (``R.feb``'s docstring).  ``ffab_grad_ref.ffab`` sets
  those imaginary parts to 0, as the HIP transform and ``wfb_ref.wmb`` do; for power-of-two sides it is the same function.

``defect`` names a wiring error of the block's backward schedule.  Every one is a detach point or a term ``k v + ((1 - k) v).detach()``:
the forward VALUE never changes, only the gradient autograd returns, which is the gradient that schedule would produce:

``ll_hi_swapped``       the gradient of the LL' slot goes to the first high band (HL') and HL's to LL': the two leading slices of
                        ``grad_[LL' ; hi']`` exchanged (a slice offset taken from the wrong end)
``no_t_skip``           ``u = t.detach() + clamp(..)``: ``grad_t = grad_u`` dropped from the front adjoint
``no_ln2_residual``     ``out = u.detach() + ffn(LN2(u))``: ``grad_out`` not added to ``LN2^T(grad_v)``
``ffn_identity_twice``  FeedForward's own identity ``+ v`` counted twice
``illu_skipped``        ``grad_LL = grad_fea``: the Illumination_Estimator's adjoint taken as the identity
``no_mask``             the back clamp lets every gradient through
``norm1_scale_1``       ``grad_scale`` taken as 1: the two norm1 gradients are those of ``weight2 = 2 w``, i.e. halved

``ffab_grad_ref.TAPS`` (while recording) also receives the two kinks outside FFAB: WM's ReLU input ``mb.convb.0`` (edge 0) and the value
before the back clamp ``back`` (edges 0 and 1).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import ffab_grad_ref as FG
import wfb_ffn_grad_ref as FF
import wfb_ref as W
import wm_grad_ref as WG
import wmb_grad_ref as PG
from bayer_low_light_image_enhancement_amd import ops
from oracle import rawformer_ref as R

DEFECTS = ("ll_hi_swapped", "no_t_skip", "no_ln2_residual", "ffn_identity_twice", "illu_skipped", "no_mask", "norm1_scale_1")
BUFFERS = tuple("ffn." + k for k in FF.BUFFERS)
B2 = "mb.convb.2.bias"


def keys(c, hidden):
    """The 131 parameter names in the order of the C ABI's pointer array."""
    return tuple(k for k in ops.wmb_param_shapes(c, hidden) if k not in BUFFERS)


def wmb(x, p, pre: str = "", training: bool = False, defect: str | None = None, chunk: int = 0, keep: dict | None = None, iwt=PG.iwt,
        eps: float = 1e-5, momentum: float = 0.1):
    """WMB.forward.  ``keep`` receives ``r`` (WM's LayerNorm input, for the bound of d convb.2.bias), ``v`` = LN2(u) and, in training
    mode, ``running``: the four running statistics after the call."""
    assert defect is None or defect in DEFECTS, defect
    keep = {} if keep is None else keep
    n = x.shape[0]
    w1, b1 = p[pre + "norm1.body.weight"], p[pre + "norm1.body.bias"]
    if defect == "norm1_scale_1":
        w1, b1 = FG.scale_grad(w1, 0.5), FG.scale_grad(b1, 0.5)
    t = 2.0 * R.layernorm2d(x, w1, b1) - 1.0
    d = R.dwt_init(t)
    ll, hi = d[:n], d[n:]
    fea = W.illu_fea(ll, p, pre + "illu.")
    if defect == "illu_skipped":
        fea = ll + (fea - ll).detach()
    ll = FG.ffab(fea, p, pre + "ffab.")
    if FG.TAPS is not None:
        FG.tap(pre + "mb.convb.0", F.conv2d(hi, p[pre + "mb.convb.0.weight"], p[pre + "mb.convb.0.bias"], padding=1), (0.0,))
    hi = WG.wm(hi, p, pre + "mb.", None, chunk, keep)
    bands = torch.cat((ll, hi), dim=0)
    if defect == "ll_hi_swapped":
        alt = torch.cat((hi[:n], ll, hi[n:]), dim=0)
        bands = alt + (bands - alt).detach()
    s = (iwt(bands) + 1.0) / 2.0
    FG.tap(pre + "back", s, (0.0, 1.0))
    c = s.clamp(0.0, 1.0)
    if defect == "no_mask":
        c = s + (c - s).detach()
    u = (t.detach() if defect == "no_t_skip" else t) + c
    v = R.layernorm2d(u, p[pre + "norm2.body.weight"], p[pre + "norm2.body.bias"])
    keep["v"] = v
    y, _, running, _ = FF.forward(v, p, pre + "ffn.", training, eps, momentum)
    keep["running"] = running
    if defect == "ffn_identity_twice":
        y = y + (v - v.detach())
    return (u.detach() if defect == "no_ln2_residual" else u) + y


def gradients(x, p, g, training: bool = True, defect: str | None = None, chunk: int = 0):
    """``({"x": dL/dx, name: dL/dp[name] for the 131 names}, dL/dr)`` of ``L = <wmb(x, p), g>`` in the dtype of the inputs; ``r`` is WM's
    LayerNorm input.  ``illu.conv2.*`` do not reach the output: their gradients are exact zeros."""
    names = keys(x.shape[1], p["ffn.project_in.weight"].shape[0])
    x = x.detach().clone().requires_grad_(True)
    q = {k: (v.detach().clone().requires_grad_(True) if k in names else v) for k, v in p.items()}
    keep = {}
    loss = (wmb(x, q, "", training, defect, chunk, keep) * g).sum()
    got = torch.autograd.grad(loss, [x] + [q[k] for k in names] + [keep["r"]], allow_unused=True)
    out = {}
    for k, t, like in zip(("x",) + names, got[:-1], [x] + [q[k] for k in names]):
        assert t is not None or k.startswith("illu.conv2.") or (defect == "illu_skipped" and k.startswith("illu.")), k
        out[k] = (torch.zeros_like(like) if t is None else t).detach()
    return out, got[-1].detach()


def margin_of(v32, v64, edges):
    """ffab_grad_ref.kink_margin's formula for one tap: min over the elements and edges of |v64 - edge| / max(|v32 - v64|, 2^-24 |v64|)."""
    pert = torch.maximum((v32.double() - v64).abs(), v64.abs() * 2.0 ** -24).clamp_min(1e-300)
    return min(float(((v64 - e).abs() / pert).min()) for e in edges)


def conditioning(x32, p32, training):
    """``{"cut": (margin, where), "kink": (margin, tap), "relu": margin, "clamp": margin, "masks": bool, "cut_low", "cut_high"}``: the
    branch-cut margin of every FEB (wfb_ref.branch_cut_margins); ffab_grad_ref.kink_margin, its one documented departure included,
    over EVERY tap of the block (FFAB's LeakyReLU and clamp taps, WM's ReLU input, the back clamp's two edges), the float32 and
    float64 recordings both starting from the block's float32 input; the same formula at WM's ReLU input and at the back clamp alone;
    whether float32 and float64 put every tapped value on the same side of every edge; and the fractions the back clamp cuts."""
    block = lambda xx, pp, pre: wmb(xx, pp, pre, training)      # noqa: E731
    kink, which, _ = FG.kink_margin(block, x32, p32)
    out = {"cut": W.branch_cut_margins(lambda pp, xx: W.wmb(xx, pp, ""), p32, x32), "kink": (kink, which), "masks": True}
    t32, t64 = FG.record(block, x32, p32), FG.record(block, x32.double(), {k: v.double() for k, v in p32.items()})
    for (name, v32, edges), (_, v64, _) in zip(t32, t64):
        for e in edges:
            out["masks"] &= bool(((v32 < e) == (v64 < e)).all() and ((v32 > e) == (v64 > e)).all())
        if name == "mb.convb.0":
            out["relu"] = margin_of(v32, v64, edges)
        elif name == "back":
            out["clamp"] = margin_of(v32, v64, edges)
            out["cut_low"], out["cut_high"] = float((v64 < 0).double().mean()), float((v64 > 1).double().mean())
    return out
