"""Gradients of FEB / ProcessBlock / FFAB for tests/test_ffab_backward.py: a differentiable restatement of ``oracle.rawformer_ref.feb``
(with the symmetric bins exact) and of ``wfb_ref.ffab``, plain torch, any dtype, and ``torch.autograd.grad`` of the loss
``<op(x, p), g>`` with respect to ``x`` and every parameter.

``R.feb(..., exact_symmetric_bins=True)`` writes the four bins that are real by symmetry in place, which autograd refuses; here the
imaginary part of the spectrum is multiplied by a 0/1 mask of those bins instead (``sym_mask``).  The value is the same.

``defect`` evaluates the same forward with one deliberate error in the GRADIENT (the value never changes: every defect is a detach
point or a term ``v * k + (v * (1 - k)).detach()``, which has the value ``v`` and ``k`` times its gradient):

``no_phase_grad``      ``angle`` detached: no gradient through the phase of the spectrum
``irfft_undoubled``    the gradient into ``irfft2`` halved on the interior spectrum columns (1 .. w/2 - 1): the adjoint of ``irfft2``
                       taken as a plain ``rfft2``
``rfft_as_irfft``      the gradient out of ``rfft2`` doubled on the interior columns: the adjoint of ``rfft2`` taken as ``irfft2``
``clamp_passthrough``  the output clamp lets every gradient through
``sym_bins_leak``      the imaginary gradient of the symmetric bins not dropped

``TAPS`` (a list, or None) records every value with a kink downstream: ``(name, tensor, edges)`` for the LeakyReLU inputs (edge 0)
and the three clamps (+-10; 0 and 1e4) -- ``kink_margin`` compares a float32 and a float64 recording.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

DEFECTS = ("no_phase_grad", "irfft_undoubled", "rfft_as_irfft", "clamp_passthrough", "sym_bins_leak")
FEB_KEYS = ("fpre.weight", "fpre.bias", "process1.0.weight", "process1.0.bias", "process1.2.weight", "process1.2.bias",
            "process2.0.weight", "process2.0.bias", "process2.2.weight", "process2.2.bias")

TAPS = None


def tap(name, v, edges):
    if TAPS is not None:
        TAPS.append((name, v.detach(), edges))


def sym_mask(h, w, like):
    """1 everywhere, 0 at the bins (0 | h/2, 0 | w/2) of an [h, w/2 + 1] half spectrum (h/2 only for an even h)."""
    m = torch.ones(h, w // 2 + 1, dtype=like.dtype, device=like.device)
    for yy in ({0, h // 2} if h % 2 == 0 else {0}):
        for xx in {0, w // 2}:
            m[yy, xx] = 0.0
    return m


def interior(w, like, k):
    """k on the columns 1 .. w/2 - 1 of a half spectrum, 1 on columns 0 and w/2."""
    c = torch.ones(w // 2 + 1, dtype=like.dtype, device=like.device)
    c[1:w // 2] = k
    return c


def scale_grad(v, k):
    """The value v with k times its gradient (k: a real tensor that broadcasts)."""
    return v * k + (v * (1.0 - k)).detach()


def spectrum(y, defect=None):
    """rfft2 (ortho) with the symmetric bins' imaginary part exactly 0."""
    h, w = y.shape[-2:]
    f = torch.fft.rfft2(y, norm="ortho")
    if defect == "rfft_as_irfft":
        f = torch.complex(scale_grad(f.real, interior(w, y, 2.0)), scale_grad(f.imag, interior(w, y, 2.0)))
    m = sym_mask(h, w, y)
    im = f.imag * m
    if defect == "sym_bins_leak":
        im = im + (f.imag - f.imag.detach()) * (1.0 - m)
    return torch.complex(f.real, im)


def polar(f, defect=None):
    pha = torch.angle(f)
    return f.abs() + 1e-6, (pha.detach() if defect == "no_phase_grad" else pha)


def inverse(mag, pha, h, w, defect=None):
    """irfft2 (ortho, s = (h, w)) of mag e^{i pha}."""
    re, im = mag * torch.cos(pha), mag * torch.sin(pha)
    if defect == "irfft_undoubled":
        re, im = scale_grad(re, interior(w, mag, 0.5)), scale_grad(im, interior(w, mag, 0.5))
    return torch.fft.irfft2(torch.complex(re, im), s=(h, w), norm="ortho")


def feb(x, p, pre="", defect=None):
    h, w = x.shape[-2:]
    tap(pre + "x", x, (-10.0, 10.0))
    xc = x.clamp(-10.0, 10.0)
    mag, pha = polar(spectrum(F.conv2d(xc, p[pre + "fpre.weight"], p[pre + "fpre.bias"]), defect), defect)

    def mlp(t, name):
        u = F.conv2d(t, p[pre + name + ".0.weight"], p[pre + name + ".0.bias"])
        tap(pre + name + ".0", u, (0.0,))
        return F.conv2d(F.leaky_relu(u, 0.1), p[pre + name + ".2.weight"], p[pre + name + ".2.bias"])

    a = mlp(mag, "process1")
    tap(pre + "process1.2", a, (0.0, 1e4))
    s = inverse(a.clamp(0.0, 1e4), mlp(pha, "process2"), h, w, defect) + xc
    tap(pre + "sum", s, (-10.0, 10.0))
    out = s.clamp(-10.0, 10.0)
    return s + (out - s).detach() if defect == "clamp_passthrough" else out


def process_block(x, p, pre, defect=None):
    return F.conv2d(feb(x, p, pre + "frequency_process.", defect), p[pre + "cat.weight"], p[pre + "cat.bias"]) + x


def ffab(x, p, pre="", defect=None):
    x = process_block(F.conv2d(x, p[pre + "conv0.0.weight"], p[pre + "conv0.0.bias"]), p, pre + "conv0.1.", defect)
    x1 = process_block(x, p, pre + "conv1.", defect)
    x2 = process_block(x1, p, pre + "conv2.", defect)
    x3 = process_block(x2, p, pre + "conv3.", defect)

    def tail(a, b, name):
        t = process_block(torch.cat((a, b), dim=1), p, pre + name + ".0.", defect)
        return F.conv2d(t, p[pre + name + ".1.weight"], p[pre + name + ".1.bias"])

    x4 = tail(x2, x3, "conv4")
    x5 = tail(x1, x4, "conv5")
    return tail(x, x5, "convout")


def gradients(op, x, p, g, defect=None):
    """{"x": dL/dx, key: dL/dp[key]} of L = <op(x, p, "", defect), g>, in the dtype of the inputs."""
    x = x.detach().clone().requires_grad_(True)
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    loss = (op(x, q, "", defect) * g).sum()
    keys = list(q)
    grads = torch.autograd.grad(loss, [x] + [q[k] for k in keys], allow_unused=True)
    out = {"x": grads[0] if grads[0] is not None else torch.zeros_like(x)}
    out.update({k: (v if v is not None else torch.zeros_like(q[k])) for k, v in zip(keys, grads[1:])})
    return {k: v.detach() for k, v in out.items()}


def record(op, x, p):
    """The taps of one forward."""
    global TAPS
    TAPS = []
    try:
        with torch.no_grad():
            op(x, p, "")
        return TAPS
    finally:
        TAPS = None


def kink_margin(op, x32, p32):
    """``min |v64 - edge| / max(|v32 - v64|, 2^-24 |v64|)`` over every tapped value and each of its edges: the distance of a case to
    the nearest kink of the block (LeakyReLU at 0, the clamps' ends) in units of the float32 perturbation observed at that very
    value.  Returns (margin, name of the tap, on_edge).

    One departure from that formula, which would give 0 there: a pre-clamp sum of the output clamp is counted in ``on_edge`` (a
    dict tap name -> count) and left out of the minimum where ALL of this holds, in float32 and in float64 alike:
    the sum equals +-10 bit for bit; the FEB's input at that pixel lies outside [-10, 10] on that side; and the magnitude MLP of that
    (image, channel) is <= 0 at every bin, so that m = clamp(a, 0, 1e4) is 0 on the whole plane.  Then the inverse transform of the
    plane is exactly 0 in any arithmetic and the sum is the clamped input itself: it sits on the edge by construction, not by
    rounding, and ``torch.clamp``'s backward passes the gradient on the closed interval in every precision.  (That the plane stays
    <= 0 is the ``process1.2`` tap's own margin.)  A sum on the edge for any other reason stays in the minimum and makes it 0."""
    t32 = record(op, x32, p32)
    t64 = record(op, x32.double(), {k: v.double() for k, v in p32.items()})
    by_name = {name: (v32, v64) for (name, v32, _), (_, v64, _) in zip(t32, t64)}
    worst, where, on_edge = float("inf"), None, {}
    for (name, v32, edges), (_, v64, _) in zip(t32, t64):
        pert = torch.maximum((v32.double() - v64).abs(), v64.abs() * 2.0 ** -24)
        for e in edges:
            exact = torch.zeros_like(v64, dtype=torch.bool)
            if name.endswith("sum"):
                pre = name[:-len("sum")]
                dead = torch.ones(v64.shape[:2], dtype=torch.bool)
                for a in by_name[pre + "process1.2"]:
                    dead &= (a <= 0).flatten(2).all(dim=2)
                outside = torch.ones_like(exact)
                for xin in by_name[pre + "x"]:
                    outside &= (xin >= e) if e > 0 else (xin <= e)
                exact = (v64 == e) & (v32.double() == e) & outside & dead[:, :, None, None]
            if bool(exact.any()):
                on_edge[name] = on_edge.get(name, 0) + int(exact.sum())
            r = ((v64 - e).abs() / pert.clamp_min(1e-300))[~exact]
            if r.numel() and float(r.min()) < worst:
                worst, where = float(r.min()), f"{name} at {e:g}"
    return worst, where, on_edge
