"""Mamba selective scan, the WM block and the complete WMB block (ops.mamba / ops.wm / ops.wmb, csrc/rf_mamba.hip) against
the float64 restatement tests/mamba_ref.py.

CPU: the restatement itself (recurrence against its closed form, WM's raw reshape), ops.mamba_param_shapes, the host checks of
the C ABI -- and, for every GPU case, that the asserted bound could not hide the defects the case exists for (below).

GPU cases (Lc = rf_mamba_chunk_len(), read from the library, so the cases follow it):

========================  ==================================================================================================
mamba (B, L, D)           branch
========================  ==================================================================================================
one_token (1, 1, 16)      L = 1: one partial tile, every convolution tap but the last in the padding
short (2, 3, 16)          L < d_conv
lc_minus_1 (1, Lc-1, 24)  one chunk with a partial last tile; Di = 48: a partial channel tile, dt_rank 2
lc (1, Lc, 24)            exactly one chunk: no carry pass
lc_plus_1 (2, Lc+1, 24)   a second chunk of one token
three_chunks (3, 3Lc+5, 32)  several chunks, odd L (the scalar GEMM path), B = 3
long_small_delta (1, 4096, 64)  delta around 1e-3: the state survives every chunk boundary; Di = 128: two channel tiles, dt_rank 4
underflow (1, 2Lc, 32)    delta around 5: exp(delta A) underflows to 0 for most states; the output must be finite
impulse (1, 2Lc, 32)      u non-zero at token Lc-2 only.  z = in_proj(u) is 0 wherever u is, so the gate silu(z) leaves exactly
                          ONE non-zero output token: the strict impulse cannot show a boundary (it still pins the taps' zero
                          padding and the bound at that token) ...
impulse_carrier           ... so the boundary case is the same impulse (amplitude 4) on a carrier of amplitude 0.05: the taps
(1, 2Lc, 32)              of tokens Lc-2 .. Lc+1 and the state built at Lc-2 cross the boundary at Lc and reach gated outputs
========================  ==================================================================================================

wm (n, c, h, w): (3, 16, 8, 8) L = 64, one chunk; (6, 32, 16, 24) L = 384; (3, 64, 32, 32) L = 1024, two channel tiles.
wmb x: [1, 32, 32, 32] (high bands [3, 32, 16, 16], L = 256) and [2, 16, 16, 32] ([6, 16, 8, 16], L = 128).

Parameters: the matrices are synth values by name, uniform in +-gain sqrt(3 / fan_in) (x_proj with gain 2 so that Bm, Cm are
O(1) and the scan term is not drowned by the D x skip); A_log = log(1..32) per row; dt_proj.bias = softplus^-1 of a per-case
delta range, log-uniform over the channels; D in [0.5, 1.5].  WM's and WMB's other modules take synth.param_values.

Every case runs twice (torch.equal between the runs) and leaves its input unchanged.

Truth and bound (the scheme of tests/test_train_shapes.py): e64 = max|hip - ref_f64|, e32 = max|ref_f32 - ref_f64| (the
restatement in float32 on the same inputs); asserted e64 <= RATIO e32 + FLOOR max|ref_f64|.
Measured on the MI355X (``-s`` prints each case): e64 / e32 lies between 0.59 (one_token) and 1.41 (impulse_carrier) for ops.mamba
and is 1.67-2.66 for ops.wm, 0.96-1.29 for ops.wmb; e64 / max|ref| is 2.1e-7 .. 5.2e-7 for ops.mamba and at most 2.8e-6
(wm_3x64x32x32: e64 6.83e-6, e32 2.57e-6, max|ref| 2.42).  That case is also the closest to the bound: 0.27 of it, a margin of
3.7 x, with RATIO = 8 and FLOOR = 2e-6; every ops.mamba case stays below 0.11 of its bound.  (e32 itself moves by up to 1.7 x
between hosts: the CPU's float32 GEMM and exp differ.)

Condition on the bound: before comparing, each case evaluates the float64 restatement with one deliberate defect -- the incoming
state of every chunk zeroed (cases with more than one chunk), the conv taps shifted by one token, dt_proj.bias dropped -- and
asserts that each moves the output by at least 100 x the asserted bound.  Where a defect cannot show by construction the case
leaves it out of its list in CASES: `underflow` (the state is dead long before a boundary: zeroing it changes nothing; that is what the case is
for) and the strict `impulse` (one live output token, in the first chunk).  The same condition runs on the CPU for every case
(test_bound_cannot_hide_the_defects).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
import mamba_ref as M
from bayer_low_light_image_enhancement_amd import _lib, ops, synth

# e64 <= RATIO e32 + FLOOR max|ref_f64|: 3.7 x above the worst case measured on the MI355X (module docstring), the margin of
# tests/test_train_shapes.py and for its reason: pool boxes and compiler schedules differ
RATIO = 8.0
FLOOR = 2e-6
SEED = 4100


def lc():
    return _lib.load().rf_mamba_chunk_len()


# ------------------------------------------------------------------------------------------ parameters and cases
def mamba_params(d_model, seed, dlo, dhi, prefix=""):
    """Mamba(d_model, 32, 4, 2) parameters: matrices from synth by name, A_log and dt_proj.bias explicit (module docstring)."""
    shapes = ops.mamba_param_shapes(d_model)
    di, r = shapes["D"][0], shapes["dt_proj.weight"][1]
    gain = {"in_proj.weight": (1.0, d_model), "conv1d.weight": (1.0, 4), "x_proj.weight": (2.0, di), "dt_proj.weight": (0.25, r),
            "out_proj.weight": (1.0, di)}
    p = {}
    for k, (g, fan) in gain.items():
        b = g * math.sqrt(3.0 / fan)
        p[prefix + k] = torch.from_numpy(synth.uniform(seed, prefix + k, shapes[k], -b, b))
    p[prefix + "conv1d.bias"] = torch.from_numpy(synth.uniform(seed, prefix + "conv1d.bias", (di,), -0.1, 0.1))
    p[prefix + "D"] = torch.from_numpy(synth.uniform(seed, prefix + "D", (di,), 0.5, 1.5))
    p[prefix + "A_log"] = torch.log(torch.arange(1, 33, dtype=torch.float64)).float().repeat(di, 1).contiguous()
    dl = torch.exp(torch.from_numpy(synth.uniform(seed, prefix + "delta", (di,), math.log(dlo), math.log(dhi))).double())
    p[prefix + "dt_proj.bias"] = torch.log(torch.expm1(dl)).float()          # softplus^-1
    return p


def wm_params(c, seed, dlo, dhi, prefix=""):
    spec = {"convb.0.weight": (2 * c, c, 3, 3), "convb.0.bias": (2 * c,), "convb.2.weight": (c, 2 * c, 3, 3), "convb.2.bias": (c,),
            "ln.weight": (c,), "ln.bias": (c,), "smooth.weight": (c, c, 3, 3), "smooth.bias": (c,)}
    p = cases.params(spec, seed=seed, prefix=prefix)
    p.update(mamba_params(c, seed, dlo, dhi, prefix + "model1."))
    return p


def wmb_params(c, seed, dlo, dhi):
    from test_ffab import wmb_params as ll_params
    p = ll_params(c)
    p.update(cases.params({"norm2.body.weight": (c,), "norm2.body.bias": (c,)}, seed=seed))
    p.update(cases.params(cases.wfb_ff_spec(c, 2.0), seed=seed + 1, prefix="ffn."))
    p.update(wm_params(c, seed + 2, dlo, dhi, "mb."))
    return p


ALL = ("zero_state", "shift_taps", "no_dt_bias")
# id: (kind, shape as a function of Lc, delta range, defects that must show)
CASES = {
    "one_token": ("mamba", lambda n: (1, 1, 16), (0.05, 0.5), ALL[1:]),
    "short": ("mamba", lambda n: (2, 3, 16), (0.05, 0.5), ALL[1:]),
    "lc_minus_1": ("mamba", lambda n: (1, n - 1, 24), (0.02, 0.3), ALL[1:]),
    "lc": ("mamba", lambda n: (1, n, 24), (0.02, 0.3), ALL[1:]),
    "lc_plus_1": ("mamba", lambda n: (2, n + 1, 24), (0.005, 0.05), ALL),
    "three_chunks": ("mamba", lambda n: (3, 3 * n + 5, 32), (0.01, 0.1), ALL),
    "long_small_delta": ("mamba", lambda n: (1, 4096, 64), (5e-4, 2e-3), ALL),
    "underflow": ("mamba", lambda n: (1, 2 * n, 32), (4.0, 6.0), ALL[1:]),
    "impulse": ("mamba", lambda n: (1, 2 * n, 32), (0.01, 0.1), ALL[2:]),
    "impulse_carrier": ("mamba", lambda n: (1, 2 * n, 32), (0.01, 0.1), ALL),
    "wm_3x16x8x8": ("wm", lambda n: (3, 16, 8, 8), (0.01, 0.2), ALL[1:]),
    "wm_6x32x16x24": ("wm", lambda n: (6, 32, 16, 24), (0.005, 0.1), ALL),
    "wm_3x64x32x32": ("wm", lambda n: (3, 64, 32, 32), (0.002, 0.05), ALL),
    "wmb_1x32x32x32": ("wmb", lambda n: (1, 32, 32, 32), (0.005, 0.1), ALL),
    "wmb_2x16x16x32": ("wmb", lambda n: (2, 16, 16, 32), (0.01, 0.2), ALL[1:]),
}
REF = {"mamba": M.mamba, "wm": M.wm, "wmb": M.wmb}


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Inputs, parameters, the float64 and float32 restatements and the bound of one case: computed once, shared, never changed."""
    kind, shape_of, (dlo, dhi), defects = CASES[tag]
    n = lc()
    shape = shape_of(n)
    seed = SEED + sorted(CASES).index(tag)
    if kind == "mamba":
        p = mamba_params(shape[2], seed, dlo, dhi)
        x = cases.rnd(f"mamba.{tag}.u", shape, seed=seed)
        if tag.startswith("impulse"):
            x = x * 0.05 if tag == "impulse_carrier" else torch.zeros_like(x)
            x[:, n - 2] = 4.0 * cases.rnd(f"mamba.{tag}.spike", (shape[0], shape[2]), seed=seed)
    elif kind == "wm":
        p = wm_params(shape[1], seed, dlo, dhi)
        x = cases.rnd(f"mamba.{tag}.x", shape, seed=seed)
    else:
        p = wmb_params(shape[1], seed, dlo, dhi)
        x = cases.rnd(f"mamba.{tag}.x", shape, seed=seed)
    p64 = {k: v.double() for k, v in p.items()}
    with torch.no_grad():
        ref64 = REF[kind](x.double(), p64, "")
        ref32 = REF[kind](x, p, "")
        assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
        moved = {d: float((REF[kind](x.double(), p64, "", defect=d, chunk=n) - ref64).abs().max()) for d in defects}
    e32 = float((ref32.double() - ref64).abs().max())
    mx = float(ref64.abs().max())
    return {"x": x, "p": p, "ref64": ref64, "e32": e32, "max": mx, "bound": RATIO * e32 + FLOOR * mx, "moved": moved, "kind": kind}


def assert_bound_sees_defects(tag):
    c = reference(tag)
    assert math.isfinite(c["max"]) and c["max"] > 0
    for d, moved in c["moved"].items():
        assert moved >= 100.0 * c["bound"], (f"[{tag}] defect {d} moves the output by {moved:.3e}, under 100 x the bound {c['bound']:.3e} "
                                             f"(e32 {c['e32']:.3e}, max|ref| {c['max']:.3e}): the case cannot see it")


# ------------------------------------------------------------------------------------------ CPU
def test_recurrence_equals_its_closed_form():
    """h_t = sum_{s <= t} exp(A sum_{r = s+1 .. t} delta_r) delta_s Bm_s x_s, evaluated term by term, against the loop."""
    b, l, di, n = 2, 9, 3, 32
    g = torch.Generator().manual_seed(7)
    delta = torch.rand(b, l, di, generator=g, dtype=torch.float64) * 0.5 + 0.01
    x = torch.randn(b, l, di, generator=g, dtype=torch.float64)
    bm = torch.randn(b, l, n, generator=g, dtype=torch.float64)
    A = -torch.arange(1, n + 1, dtype=torch.float64).repeat(di, 1) * (1.0 + 0.1 * torch.rand(di, n, generator=g, dtype=torch.float64))
    h = M.scan_states(delta, A, bm, x)
    assert h.dtype == torch.float64 and tuple(h.shape) == (b, l, di, n)
    for t in range(l):
        direct = torch.zeros(b, di, n, dtype=torch.float64)
        for s in range(t + 1):
            decay = torch.exp(A * delta[:, s + 1:t + 1].sum(dim=1)[:, :, None])
            direct += decay * (delta[:, s] * x[:, s])[:, :, None] * bm[:, s][:, None, :]
        assert float((h[:, t] - direct).abs().max()) <= 1e-12, t


@pytest.mark.parametrize("d_model,rank", [(16, 1), (24, 2), (32, 2), (64, 4)])
def test_param_shapes(d_model, rank):
    di = 2 * d_model
    assert ops.mamba_param_shapes(d_model) == {
        "in_proj.weight": (2 * di, d_model), "conv1d.weight": (di, 1, 4), "conv1d.bias": (di,), "x_proj.weight": (rank + 64, di),
        "dt_proj.weight": (di, rank), "dt_proj.bias": (di,), "A_log": (di, 32), "D": (di,), "out_proj.weight": (d_model, di)}
    assert list(ops.mamba_param_shapes(d_model)) == list(ops._MAMBA_KEYS)          # the order of the C ABI's pointer array
    assert ops.mamba_param_shapes(8, d_state=16, d_conv=3, expand=3)["x_proj.weight"] == (1 + 32, 24)


def test_wm_tokens_are_runs_of_c_floats():
    x = torch.arange(64, dtype=torch.float32).reshape(1, 8, 2, 4)
    flat = x.reshape(-1)
    sliced = torch.stack([flat[i * 8:(i + 1) * 8] for i in range(8)]).unsqueeze(0)
    assert torch.equal(M.wm_tokens(x), sliced)
    assert not torch.equal(M.wm_tokens(x), x.permute(0, 2, 3, 1).reshape(1, 8, 8))      # ... which a permute is not
    # and wm() feeds exactly those tokens to LayerNorm + Mamba: with convb = 0 and smooth = identity, wm(x) = Mamba(LN(tokens))
    c = 8
    p = wm_params(c, 5, 0.05, 0.5)
    for k in ("convb.0.weight", "convb.0.bias", "convb.2.weight", "convb.2.bias", "smooth.bias"):
        p[k] = torch.zeros_like(p[k])
    p["smooth.weight"] = torch.zeros(c, c, 3, 3)
    p["smooth.weight"][torch.arange(c), torch.arange(c), 1, 1] = 1.0
    xr = cases.rnd("mamba.reshape.x", (1, c, 2, 4), seed=5).double()
    p = {k: v.double() for k, v in p.items()}
    tok = torch.nn.functional.layer_norm(torch.stack([xr.reshape(-1)[i * c:(i + 1) * c] for i in range(8)]).unsqueeze(0), (c,),
                                         p["ln.weight"], p["ln.bias"], 1e-5)
    want = M.mamba(tok, p, "model1.").permute(0, 2, 1).reshape(1, c, 2, 4)
    assert float((M.wm(xr, p) - want).abs().max()) <= 1e-12


BAD = ((dict(d_state=8), b"d_state"), (dict(d_conv=3), b"d_conv"), (dict(d_model=18), b"d_model"), (dict(L=0), b": L 0 "))


def test_host_checks_refuse_unsupported_shapes_before_any_launch():
    lib = _lib.load()
    assert lib.rf_mamba_chunk_len() > 4
    good = dict(B=2, L=300, d_model=32, d_state=32, d_conv=4, expand=2)
    order = ("B", "L", "d_model", "d_state", "d_conv", "expand")
    assert lib.rf_mamba_workspace_bytes(*[good[k] for k in order]) > 0
    assert lib.rf_wm_workspace_bytes(6, 32, 16, 24) > lib.rf_mamba_workspace_bytes(6, 384, 32, 32, 4, 2) - 6 * 384 * 32 * 4
    fake = C.c_void_p(1 << 12)                      # 16-byte aligned, never dereferenced: the shape check comes first
    prm = (C.c_void_p * 9)(*[1 << 12] * 9)
    for change, word in BAD:
        a = [{**good, **change}[k] for k in order]
        assert lib.rf_mamba_workspace_bytes(*a) < 0
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_mamba_workspace_bytes: ") and word in msg, msg
        assert lib.rf_mamba_forward(fake, fake, prm, fake, 1 << 40, *a, 0, None) < 0
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_mamba_forward: ") and word in msg, msg
    assert lib.rf_wm_workspace_bytes(3, 18, 8, 8) < 0 and b"c 18" in lib.rf_last_error()
    prm17 = (C.c_void_p * 17)(*[1 << 12] * 17)
    assert lib.rf_wm_forward(fake, fake, prm17, fake, 1 << 40, 3, 18, 8, 8, None) < 0 and b"rf_wm_forward: c 18" in lib.rf_last_error()
    # a workspace that is too small is refused too, before any launch
    assert lib.rf_mamba_forward(fake, fake, prm, fake, 1024, *[good[k] for k in order], 0, None) == -12
    assert b"workspace" in lib.rf_last_error()


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_cannot_hide_the_defects(tag):
    assert_bound_sees_defects(tag)


def test_cases_reach_the_branches_they_are_named_for():
    n = lc()
    r = reference("underflow")
    assert np.isfinite(r["ref64"].numpy()).all()
    assert float(torch.exp(torch.tensor(-4.0 * 32.0))) < 1e-38                      # exp(delta A) at the far states: below float32's normals
    imp = reference("impulse")
    live = imp["ref64"].abs().amax(dim=(0, 2)).nonzero().flatten().tolist()
    assert live == [n - 2], live                                                    # the gate leaves one token (module docstring)
    car = reference("impulse_carrier")
    assert float(car["ref64"][:, n:].abs().max()) > 0


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_the_float64_restatement(device, tag):
    c = reference(tag)
    assert_bound_sees_defects(tag)
    fn = {"mamba": ops.mamba, "wm": ops.wm, "wmb": ops.wmb}[c["kind"]]
    x = c["x"].to(device)
    keep = x.clone()
    p = {k: v.to(device) for k, v in c["p"].items()}
    out = fn(x, p)
    again = fn(x, p)
    torch.cuda.synchronize()
    assert torch.equal(x, keep), f"[{tag}] the input was written"
    assert torch.equal(out, again), f"[{tag}] two runs differ"
    got = out.cpu().double()
    assert tuple(got.shape) == tuple(c["ref64"].shape)
    assert bool(torch.isfinite(got).all()), f"[{tag}] non-finite output"
    e64 = float((got - c["ref64"]).abs().max())
    msg = (f"[{tag}] e64 {e64:.3e} e32 {c['e32']:.3e} max|ref| {c['max']:.3e} | e64/e32 {e64 / max(c['e32'], 1e-30):.2f} "
           f"e64/max {e64 / c['max']:.2e} | bound {c['bound']:.3e} ({e64 / c['bound']:.3f} of it)")
    print(msg)
    assert e64 <= c["bound"], msg


@pytest.mark.gpu
def test_channel_major_is_the_same_operator(device):
    """ops.mamba(channel_major=True) on the transposed tensor: the same kernels without the two transpositions -- same bits."""
    c = reference("three_chunks")
    p = {k: v.to(device) for k, v in c["p"].items()}
    x = c["x"].to(device)
    a = ops.mamba(x, p)
    b = ops.mamba(x.transpose(1, 2).contiguous(), p, channel_major=True)
    assert torch.equal(a, b.transpose(1, 2).contiguous())
