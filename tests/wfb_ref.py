"""Plain-torch restatement of the whole WFB RawFormer (RawFomer_WFB_FFAB/model.py:437-508), eval mode: the wiring of
``oracle.rawformer_ref.rawformer_forward`` (plain variant, ``branch_lrelu``, ``clamp_io``) with the ``WMB`` block of
``tests/mamba_ref.py`` as each stage's ``Transformer``.  Everything works in the dtype of its inputs (float64 in, float64 out).

``FFAB`` is restated here rather than taken from ``R.ffab`` because its ``FEB`` must run with ``exact_symmetric_bins=True``: the
CPU FFT leaves rounding noise of either sign in the imaginary part of the bins that are real by symmetry when a size is no power
of two, and ``angle`` of a negative real bin then is +pi or -pi at random (``R.feb``'s docstring).

``defect`` evaluates the same forward with one deliberate error, for tests that have to show their bound would see it: the three
of ``mamba_ref`` (``"zero_state"``, ``"shift_taps"``, ``"no_dt_bias"``; ``chunk`` = the scan's chunk length) and
``"bn_identity"`` (the BatchNorms of ``ffn.rep_conv1/2`` taken as the identity, i.e. not folded) and ``"no_mean_fold"``
(``illu.conv1``'s channel-mean column dropped).

``synth_state`` builds the deterministic weights the fixtures and the tests share.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import mamba_ref as M
from bayer_low_light_image_enhancement_amd import synth
from oracle import rawformer_ref as R

MAMBA_DEFECTS = ("zero_state", "shift_taps", "no_dt_bias")
DEFECTS = MAMBA_DEFECTS + ("bn_identity", "no_mean_fold")


SPECTRA = None      # a list: every FEB appends (its prefix, rfft2 of its input) -- see branch_cut_margins


def process_block(x, p, pre):
    if SPECTRA is not None:
        q = pre + "frequency_process."
        SPECTRA.append((q, torch.fft.rfft2(F.conv2d(x.clamp(-10.0, 10.0), p[q + "fpre.weight"], p[q + "fpre.bias"]), norm="ortho")))
    return F.conv2d(R.feb(x, p, pre + "frequency_process.", exact_symmetric_bins=True), p[pre + "cat.weight"], p[pre + "cat.bias"]) + x


def branch_cut_margins(run, p32, x32):
    """How well a case is conditioned with respect to FEB's one discontinuity.  ``angle`` jumps by 2 pi where a bin with a negative
    real part has a zero imaginary part, and the phase feeds a 1x1 MLP that is not 2 pi periodic: an input that puts a bin closer to
    that cut than float32 arithmetic resolves has no float32 answer (either side is one).  For every FEB of ``run(p, x)`` and every
    bin with a negative real part (the bins that are real by symmetry excluded: they are exact), this returns
    ``min over bins of |Im F_64| / |Im F_32 - Im F_64|``: the distance to the cut in units of the float32 perturbation observed at
    that very bin, and the bin's description.  From the float32 and float64 restatements alone."""
    global SPECTRA
    spectra = []
    for p, x in ((p32, x32), ({k: (v.double() if v.dtype.is_floating_point else v) for k, v in p32.items()}, x32.double())):
        SPECTRA = []
        try:
            with torch.no_grad():
                run(p, x)
        finally:
            spectra.append(SPECTRA)
            SPECTRA = None
    worst, where = float("inf"), None
    for (pre, f32), (_, f64) in zip(*spectra):
        h, wf = f64.shape[-2:]
        mask = torch.ones(h, wf, dtype=torch.bool)
        for yy in {0, h // 2} if h % 2 == 0 else {0}:
            for xx in {0, wf - 1}:
                mask[yy, xx] = False
        neg = (f64.real < 0) & mask
        if not bool(neg.any()):
            continue
        # the perturbation of a bin, floored by float32's resolution of the bin's own magnitude
        pert = torch.maximum((f32.imag.double() - f64.imag).abs(), f64.abs() * 2.0 ** -24)[neg]
        ratio = f64.imag.abs()[neg] / pert
        if float(ratio.min()) < worst:
            worst, where = float(ratio.min()), (pre, h, 2 * (wf - 1))
    return worst, where


def ffab(x, p, pre):
    """FFAB.forward (blocks.py:83-92), as ``R.ffab`` with the symmetric bins exact."""
    x = process_block(F.conv2d(x, p[pre + "conv0.0.weight"], p[pre + "conv0.0.bias"]), p, pre + "conv0.1.")
    x1 = process_block(x, p, pre + "conv1.")
    x2 = process_block(x1, p, pre + "conv2.")
    x3 = process_block(x2, p, pre + "conv3.")

    def tail(a, b, name):
        t = process_block(torch.cat((a, b), dim=1), p, pre + name + ".0.")
        return F.conv2d(t, p[pre + name + ".1.weight"], p[pre + name + ".1.bias"])

    x4 = tail(x2, x3, "conv4")
    x5 = tail(x1, x4, "conv5")
    return tail(x, x5, "convout")


def illu_fea(img, p, pre, defect=None):
    """Illumination_Estimator.forward (model.py:186-200) up to ``illu_fea``; WMB.forward discards ``illu_map`` (conv2)."""
    if defect == "no_mean_fold":
        x1 = F.conv2d(img, p[pre + "conv1.weight"][:, :-1], p[pre + "conv1.bias"])
    else:
        x1 = F.conv2d(torch.cat([img, img.mean(dim=1, keepdim=True)], dim=1), p[pre + "conv1.weight"], p[pre + "conv1.bias"])
    return F.conv2d(x1, p[pre + "depth_conv.weight"], p[pre + "depth_conv.bias"], padding=2, groups=x1.shape[1])


def feed_forward(x, p, pre, defect=None):
    """FeedForward.forward (model.py:58-65), BatchNorm on its running statistics."""
    if defect != "bn_identity":
        return R.wfb_feed_forward(x, p, pre)
    hid = F.conv2d(x, p[pre + "project_in.weight"], p[pre + "project_in.bias"])
    c = hid.shape[1]
    x1 = hid + F.conv2d(hid, p[pre + "rep_conv1.c.weight"], None, padding=1, groups=c) + F.conv2d(hid, p[pre + "rep_conv2.c.weight"], None, groups=c)
    x2 = F.conv2d(hid, p[pre + "dwconv.weight"], p[pre + "dwconv.bias"], padding=1, groups=c)
    return F.conv2d(F.gelu(x2) * x1 + F.gelu(x1) * x2, p[pre + "project_out.weight"], p[pre + "project_out.bias"]) + x


def wmb(x, p, pre, defect=None, chunk=0):
    """WMB.forward (model.py:215-245)."""
    n = x.shape[0]
    t = 2.0 * R.layernorm2d(x, p[pre + "norm1.body.weight"], p[pre + "norm1.body.bias"]) - 1.0
    d = R.dwt_init(t)
    ll = ffab(illu_fea(d[:n], p, pre + "illu.", defect), p, pre + "ffab.")
    hi = M.wm(d[n:], p, pre + "mb.", defect if defect in MAMBA_DEFECTS else None, chunk)
    t = t + ((R.iwt_init(torch.cat((ll, hi), dim=0)) + 1.0) / 2.0).clamp(0.0, 1.0)
    return t + feed_forward(R.layernorm2d(t, p[pre + "norm2.body.weight"], p[pre + "norm2.body.bias"]), p, pre + "ffn.", defect)


def stage(x, p, i, defect=None, chunk=0):
    """Conv_Transformer.forward (model.py:427-433) of ``conv_tran<i>``."""
    pre = f"conv_tran{i}."
    conv = F.leaky_relu(F.conv2d(x, p[pre + "conv.weight"], p[pre + "conv.bias"], padding=1), 0.2)
    t = F.conv2d(torch.cat([conv, wmb(x, p, pre + "Transformer.", defect, chunk)], dim=1), p[pre + "channel_reduce.weight"], p[pre + "channel_reduce.bias"])
    return F.leaky_relu(F.conv2d(t, p[pre + "Conv_out.weight"], p[pre + "Conv_out.bias"], padding=1), 0.2)


def forward(p, x, packed=False, defect=None, chunk=0):
    """RawFormer.forward (model.py:473-508): mosaic ``[B,1,2H,2W]`` (or the packed frame with ``packed``) -> ``[B,3,2H,2W]``."""
    x = x.clamp(0.0, 1.0)
    x4 = x if packed else R.pixel_unshuffle2(x)
    t = F.conv2d(x4, p["embedding.weight"], p["embedding.bias"], padding=1)
    e1 = stage(t, p, 1, defect, chunk)
    e2 = stage(R.downsample(e1, p["down1.body.0.weight"]), p, 2, defect, chunk)
    e3 = stage(R.downsample(e2, p["down2.body.0.weight"]), p, 3, defect, chunk)
    e4 = stage(R.downsample(e3, p["down3.body.0.weight"]), p, 4, defect, chunk)

    def up(t_in, skip, i):
        u = R.conv_transpose2x2(t_in, p[f"up{i}.weight"], p[f"up{i}.bias"])
        return F.conv2d(torch.cat([u, skip], dim=1), p[f"channel_reduce{i}.weight"], p[f"channel_reduce{i}.bias"])

    d3 = stage(up(e4, e3, 1), p, 5, defect, chunk)
    d2 = stage(up(d3, e2, 2), p, 6, defect, chunk)
    d1 = stage(up(d2, e1, 3), p, 7, defect, chunk)
    out = F.leaky_relu(F.conv2d(d1, p["conv_out.weight"], p["conv_out.bias"], padding=1), 0.2)
    return R.pixel_shuffle2(out).clamp(0.0, 1.0)


# ---------------------------------------------------------------------------------------------- the forward composed from ops.*
def ops_stage(x, p, i):
    """``conv_tran<i>`` from the operator-level calls a user had to write before ``variant='wfb'`` existed (device tensors)."""
    from bayer_low_light_image_enhancement_amd import ops
    pre = f"conv_tran{i}."
    conv = ops.conv3x3(x, p[pre + "conv.weight"], p[pre + "conv.bias"], act="lrelu")
    t = ops.conv1x1(conv, p[pre + "channel_reduce.weight"], p[pre + "channel_reduce.bias"], x2=ops.wmb(x, p, pre + "Transformer."))
    return ops.conv3x3(t, p[pre + "Conv_out.weight"], p[pre + "Conv_out.bias"], act="lrelu")


def ops_forward(p, x):
    """The whole forward composed from ``ops.*`` on the device: every call folds and packs its own weights."""
    from bayer_low_light_image_enhancement_amd import ops
    t = ops.conv3x3(ops.downshuffle(x.clamp(0.0, 1.0)), p["embedding.weight"], p["embedding.bias"])
    e = []
    for i in (1, 2, 3):
        e.append(ops_stage(t, p, i))
        t = ops.conv3x3(e[-1], p[f"down{i}.body.0.weight"], None, store="unshuffle")
    t = ops_stage(t, p, 4)
    for i in (1, 2, 3):
        u = ops.conv_transpose2x2(t, p[f"up{i}.weight"], p[f"up{i}.bias"])
        t = ops_stage(ops.conv1x1(u, p[f"channel_reduce{i}.weight"], p[f"channel_reduce{i}.bias"], x2=e[3 - i]), p, 4 + i)
    return ops.conv3x3(t, p["conv_out.weight"], p["conv_out.bias"], act="lrelu", store="shuffle").clamp(0.0, 1.0)


# ---------------------------------------------------------------------------------------------- deterministic weights
DELTA = (0.005, 0.1)      # softplus(dt_proj.bias), log-uniform over the channels: the state survives a chunk boundary


def synth_state(shapes, seed, delta=DELTA):
    """float32 state for ``{key: shape}`` (a WFB state_dict's, from the module here or from the reference): ``synth.param_values``
    by name, except
    * the Mamba modules, which take the recipe of tests/test_mamba.py (matrices uniform in +-gain sqrt(3 / fan_in), x_proj with
      gain 2; A_log = log(1..32) per row; dt_proj.bias = softplus^-1 of ``delta``; D in [0.5, 1.5]);
    * the BatchNorm statistics: running_mean in [-0.5, 0.5] (either sign), running_var in [0.5, 2];
    * conv_out: the stages leave activations of standard deviation ~2 (every WMB starts from a LayerNorm), which the output clamp
      to [0, 1] would flatten to 0 / 1 for most pixels; the last convolution's weight is scaled by 0.1 and its bias raised by 0.4
      so that the frames the tests compare lie inside the clamp.
    Integer entries (num_batches_tracked) are zero."""
    gain = {"in_proj.weight": 1.0, "conv1d.weight": 1.0, "x_proj.weight": 2.0, "dt_proj.weight": 0.25, "out_proj.weight": 1.0}
    out = {}
    for k, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        leaf = k.rsplit(".", 1)[-1]
        tail2 = ".".join(k.rsplit(".", 2)[-2:])
        if leaf == "num_batches_tracked":
            out[k] = torch.zeros(shape, dtype=torch.int64)
            continue
        if ".mb.model" in k:
            if tail2 in gain:
                fan = shape[-1] if tail2 != "conv1d.weight" else 4
                b = gain[tail2] * math.sqrt(3.0 / fan)
                v = synth.uniform(seed, k, shape, -b, b)
            elif leaf == "A_log":
                out[k] = torch.log(torch.arange(1, shape[1] + 1, dtype=torch.float64)).float().repeat(shape[0], 1).contiguous()
                continue
            elif leaf == "D":
                v = synth.uniform(seed, k, shape, 0.5, 1.5)
            elif tail2 == "dt_proj.bias":
                dl = torch.exp(torch.from_numpy(synth.uniform(seed, k, shape, math.log(delta[0]), math.log(delta[1]))).double())
                out[k] = torch.log(torch.expm1(dl)).float()
                continue
            else:      # conv1d.bias
                v = synth.uniform(seed, k, shape, -0.1, 0.1)
        elif leaf == "running_mean":
            v = synth.uniform(seed, k, shape, -0.5, 0.5)
        elif leaf == "running_var":
            v = synth.uniform(seed, k, shape, 0.5, 2.0)
        else:
            v = synth.param_values(seed, k, shape)
            if k == "conv_out.weight":
                v = v * 0.1
            if k == "conv_out.bias":
                v = v + 0.4
        out[k] = torch.from_numpy(v).reshape(shape).float().contiguous()
    return out
