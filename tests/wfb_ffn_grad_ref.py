"""Plain-torch restatement of the WFB ``FeedForward`` (RawFomer_WFB_FFAB/model.py:42-62) in training and in eval mode, for autograd.

dtype-generic: every tensor takes the dtype of ``x``.  With ``hid = project_in(x)``::

    u1 = dw3x3(hid; rep_conv1.c.weight)      u2 = rep_conv2.c.weight (.) hid
    training: mu_i, v_i = mean and BIASED variance of u_i over (B, h, w);   eval: running_mean / running_var
    uh_i = (u_i - mu_i) / sqrt(v_i + eps)
    a = hid + g1 uh1 + b1 + g2 uh2 + b2      g = dw3x3(hid; dwconv.weight) + dwconv.bias
    y = project_out(gelu(g) a + gelu(a) g) + x

and ``nn.BatchNorm2d``'s side effect in training mode: ``running <- (1 - momentum) running + momentum new`` with the UNBIASED variance.

``defect=`` names a wrong gradient (or, ``biased_running``, a wrong update) that a bound must be able to see.  The gradient defects
are detach points: they change the gradient and never the value.
"""
import torch
import torch.nn.functional as F

import cases

KEYS = ("project_in.weight", "project_in.bias", "dwconv.weight", "dwconv.bias", "project_out.weight", "project_out.bias",
        "rep_conv1.c.weight", "rep_conv1.bn.weight", "rep_conv1.bn.bias", "rep_conv2.c.weight", "rep_conv2.bn.weight", "rep_conv2.bn.bias")
BUFFERS = ("rep_conv1.bn.running_mean", "rep_conv1.bn.running_var", "rep_conv2.bn.running_mean", "rep_conv2.bn.running_var")
STATS = ("mu1", "v1", "mu2", "v2")
W2 = "rep_conv2.c.weight"
# stats_detached: mu, v constants (the eval formula for du);  no_var_term: the uh dg / N term dropped (v a constant);
# gate_one_term: only gelu(g) a differentiated;  no_skip: the hid identity missing from dhid
GRAD_DEFECTS = ("stats_detached", "no_var_term", "gate_one_term", "no_skip")
DEFECTS = GRAD_DEFECTS + ("biased_running",)      # biased_running: the running variance updated without N / (N - 1)

SEED = 4700
# tag: ((B, dim, hidden, h, w), amplitude of x), in the order that fixes the seeds.  tests/test_wfb_ffn_train.py says what each is for.
CASES = {
    "two_px": ((1, 4, 8, 1, 2), 4.0),
    "base": ((2, 16, 32, 8, 8), 4.0),
    "w_mod4_2": ((2, 16, 40, 6, 10), 4.0),
    "odd": ((1, 24, 60, 5, 7), 4.0),
    "ff48": ((1, 48, 120, 10, 14), 4.0),
    "slabs": ((2, 4, 8, 8, 516), 4.0),
    "c256": ((1, 256, 512, 4, 4), 4.0),
    "shifted": ((2, 16, 32, 8, 12), 1.0),
}
SHIFT = 8.0      # project_in.bias of `shifted`


def inputs(tag):
    """``(x, g, p)`` of a case in float32: ``x`` uniform in +-amplitude and the cotangent ``g`` in +-1 from ``cases.rnd``; the 12
    parameters and 4 buffers from ``cases.params`` (running_var in [0.5, 1.5]), the two BatchNorm weights given alternating signs
    (period 2 and 4), ``rep_conv2.c.weight`` kept away from 0 (0.5 <= |w2| < 1: BN(w2 hid) is independent of the size of w2 only
    while w2^2 var(hid) >> eps), ``project_in.bias`` = SHIFT in ``shifted``."""
    (b, dim, hidden, h, w), amp = CASES[tag]
    seed = SEED + list(CASES).index(tag)
    p = cases.params(cases.wfb_ff_spec(dim, hidden / dim), seed=seed)
    assert set(p) == set(KEYS + BUFFERS) and p["project_in.weight"].shape[0] == hidden
    c = torch.arange(hidden)
    p["rep_conv1.bn.weight"] = p["rep_conv1.bn.weight"] * (1.0 - 2.0 * (c % 2)).float()
    p["rep_conv2.bn.weight"] = p["rep_conv2.bn.weight"] * (1.0 - 2.0 * ((c // 2) % 2)).float()
    w2 = p[W2]
    p[W2] = torch.where(w2 < 0, -1.0, 1.0) * (0.5 + 0.25 * w2.abs())
    assert float(p[W2].abs().max()) < 1.0
    if tag == "shifted":
        p["project_in.bias"] = torch.full((hidden,), SHIFT)
    x = cases.rnd(f"wfb_ffn.{tag}.x", (b, dim, h, w), -amp, amp, seed=seed)
    g = cases.rnd(f"wfb_ffn.{tag}.g", (b, dim, h, w), seed=seed)
    return x, g, p


def forward(x, p, prefix="", training=True, eps=1e-5, momentum=0.1, defect=None):
    """``(y, stats, running, (hid, u2))``: the output, ``{mu1, v1, mu2, v2}`` as used, the four running statistics AFTER the call
    (those of ``p`` in eval mode) and two intermediates (``u2`` for the gradient with respect to it)."""
    assert defect is None or defect in DEFECTS, defect
    q = lambda k: p[prefix + k]      # noqa: E731
    c = q("project_in.weight").shape[0]
    hid = F.conv2d(x, q("project_in.weight"), q("project_in.bias"))
    u = [F.conv2d(hid, q("rep_conv1.c.weight"), None, padding=1, groups=c), F.conv2d(hid, q(W2), None, groups=c)]
    n = x.shape[0] * x.shape[2] * x.shape[3]
    a = hid.detach() if defect == "no_skip" else hid
    stats, running = {}, {}
    for i, name in enumerate(("rep_conv1", "rep_conv2")):
        rm, rv = q(f"{name}.bn.running_mean"), q(f"{name}.bn.running_var")
        if training:
            mu = u[i].mean(dim=(0, 2, 3))
            v = ((u[i] - mu[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
            unbiased = v if defect == "biased_running" else v * (n / (n - 1))
            running[f"{name}.bn.running_mean"] = ((1 - momentum) * rm + momentum * mu).detach()
            running[f"{name}.bn.running_var"] = ((1 - momentum) * rv + momentum * unbiased).detach()
            if defect == "stats_detached":
                mu, v = mu.detach(), v.detach()
            elif defect == "no_var_term":
                v = v.detach()
        else:
            mu, v = rm, rv
            running[f"{name}.bn.running_mean"], running[f"{name}.bn.running_var"] = rm, rv
        stats[f"mu{i + 1}"], stats[f"v{i + 1}"] = mu.detach(), v.detach()
        uh = (u[i] - mu[None, :, None, None]) / torch.sqrt(v + eps)[None, :, None, None]
        a = a + q(f"{name}.bn.weight")[None, :, None, None] * uh + q(f"{name}.bn.bias")[None, :, None, None]
    g = F.conv2d(hid, q("dwconv.weight"), q("dwconv.bias"), padding=1, groups=c)
    second = F.gelu(a) * g
    m = F.gelu(g) * a + (second.detach() if defect == "gate_one_term" else second)
    return F.conv2d(m, q("project_out.weight"), q("project_out.bias")) + x, stats, running, (hid, u[1])


def gradients(x, p, g, training=True, eps=1e-5, momentum=0.1, defect=None):
    """Everything the operators return, by autograd of ``<y, g>``: ``{"y", "x" (the gradient), the 12 KEYS (gradients), mu1 .. v2, the
    four BUFFERS after the call}`` and, second, ``max over channels of sum |du2 hid|``: the sum of the absolute summands of
    d rep_conv2.c.weight (du2 = the gradient with respect to u2, and u2 = w2 hid)."""
    x = x.detach().clone().requires_grad_(True)
    p = {k: (v.detach().clone().requires_grad_(True) if k in KEYS else v) for k, v in p.items()}
    y, stats, running, (hid, u2) = forward(x, p, "", training, eps, momentum, defect)
    got = torch.autograd.grad((y * g).sum(), [x] + [p[k] for k in KEYS] + [u2])
    out = {"y": y.detach(), "x": got[0]}
    out.update({k: t for k, t in zip(KEYS, got[1:])})
    out.update(stats)
    out.update({k: running[k].detach() for k in BUFFERS})
    return out, float((got[-1] * hid.detach()).abs().sum(dim=(0, 2, 3)).max())
