"""ops.mamba_backward (csrc/rf_mamba_bwd.hip) against float64 autograd of the restatement tests/mamba_ref.py.

Loss: ``<mamba_ref.mamba(u, p), g>`` with a fixed random ``g``; truth = ``torch.autograd.grad`` in float64 with respect to ``u`` and
the nine parameter tensors (tests/mamba_grad_ref.py), e32 = the same computation in float32.  Parameters:
``test_mamba.mamba_params`` with its gains and its per-case delta ranges.

Cases (B, L, d_model), Lc = rf_mamba_chunk_len() read from the library:

=========================  =============================================================================================
one_token (1, 1, 16)       one token
short (2, 3, 16)           L < d_conv
lc_minus_1 (1, Lc-1, 24)   a partial tile; Di = 48: a partial channel tile; dt_rank 2
lc (1, Lc, 24)             exactly one chunk: no adjoint carry
lc_plus_1 (2, Lc+1, 24)    a second chunk of one token
three_chunks (3, 3Lc+5, 32)  several chunks, odd L
two_tiles (1, 2Lc+3, 64)   Di = 128: dBm / dCm are sums over channel tiles the restatement's first 64 channels do not cover
nine_chunks (1, 9Lc+1, 32)   delta around 1e-3: the state and the adjoint survive every boundary; more chunks than one carry
                           batch of eight
underflow (1, 2Lc, 32)     delta around 5: exp(delta A) underflows to 0 for most states; every gradient finite (a backward
                           that recovers h_{t-1} by dividing by exp(delta A) gives inf / nan here)
=========================  =============================================================================================

L % 4 == 0 (lc, underflow) takes launch_gram2 for the four weight gradients, every other case the scalar-row kernel
wgrad1x1_kernel<false> (csrc/rf_grad.hip), with the strides of the channel slices it reads.

Bound, per gradient tensor (the scheme of tests/test_mamba.py and tests/test_train_shapes.py): e64 = max|hip - ref_f64| <=
8 e32 + 2e-6 max|ref_f64|.  ``-s`` prints e64 / bound for every tensor of every case; DESIGN.md section 4, "Mamba backward", holds the table
measured on the MI355X.

Condition on the bound: before comparing, each case shows on the CPU that each defect of mamba_grad_ref.DEFECTS that applies to it
(``cut_adjoint``: more than one chunk; ``first_tile_bc``: Di > 64; ``straight_softplus`` and ``dead_gate``: all) moves at least
one gradient tensor by >= 100 x that tensor's bound.  (In `underflow` the adjoint decays by exp(-4) or more per token, so what
crosses the chunk boundary is small; whether ``cut_adjoint`` still shows depends on the tokens next to the boundary.  The case's
seed is one where it does, 700 x the bound of dA_log; with the seed before it in the list it moved nothing by more than 7 x.)

"""
import ctypes as C
import functools
import math

import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
import mamba_grad_ref as G
import mamba_ref as M
from bayer_low_light_image_enhancement_amd import _lib, ops
from test_mamba import BAD, FLOOR, RATIO, lc, mamba_params

SEED = 4300
NAMES = ("u",) + G.KEYS
# id: (shape as a function of Lc, delta range)
CASES = {
    "one_token": (lambda n: (1, 1, 16), (0.05, 0.5)),
    "short": (lambda n: (2, 3, 16), (0.05, 0.5)),
    "lc_minus_1": (lambda n: (1, n - 1, 24), (0.02, 0.3)),
    "lc": (lambda n: (1, n, 24), (0.02, 0.3)),
    "lc_plus_1": (lambda n: (2, n + 1, 24), (0.005, 0.05)),
    "three_chunks": (lambda n: (3, 3 * n + 5, 32), (0.01, 0.1)),
    "two_tiles": (lambda n: (1, 2 * n + 3, 64), (0.005, 0.05)),
    "nine_chunks": (lambda n: (1, 9 * n + 1, 32), (5e-4, 2e-3)),
    "underflow": (lambda n: (1, 2 * n, 32), (4.0, 6.0)),
}
# inputs and parameters of a case come from SEED + this (underflow: module docstring)
SEEDS = {"lc": 0, "lc_minus_1": 1, "lc_plus_1": 2, "nine_chunks": 3, "one_token": 4, "short": 5, "three_chunks": 6, "two_tiles": 7, "underflow": 9}


def defects_of(shape, n):
    out = ["straight_softplus", "dead_gate"]
    if shape[1] > n:
        out.append("cut_adjoint")
    if 2 * shape[2] > G.TILE:
        out.append("first_tile_bc")
    return out


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Inputs, parameters, the float64 and float32 gradients, the bounds and what each defect moves: computed once, shared, never
    changed."""
    shape_of, (dlo, dhi) = CASES[tag]
    n = lc()
    shape = shape_of(n)
    seed = SEED + SEEDS[tag]
    p = mamba_params(shape[2], seed, dlo, dhi)
    u = cases.rnd(f"mamba_bwd.{tag}.u", shape, seed=seed)
    g = cases.rnd(f"mamba_bwd.{tag}.g", shape, seed=seed)
    p64 = {k: v.double() for k, v in p.items()}
    ref64 = G.gradients(u.double(), p64, g.double())
    ref32 = G.gradients(u, p, g)
    assert all(ref64[k].dtype == torch.float64 and ref32[k].dtype == torch.float32 for k in NAMES)
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in NAMES}
    mx = {k: float(ref64[k].abs().max()) for k in NAMES}
    bound = {k: RATIO * e32[k] + FLOOR * mx[k] for k in NAMES}
    moved = {}
    for d in defects_of(shape, n):
        bad = G.gradients(u.double(), p64, g.double(), defect=d, chunk=n)
        moved[d] = {k: float((bad[k] - ref64[k]).abs().max()) for k in NAMES}
    return {"u": u, "g": g, "p": p, "ref64": ref64, "e32": e32, "max": mx, "bound": bound, "moved": moved}


def assert_bound_sees_defects(tag):
    c = reference(tag)
    assert all(math.isfinite(c["max"][k]) for k in NAMES) and c["max"]["u"] > 0
    for d, moved in c["moved"].items():
        # (dA_log of one_token is exactly 0, h_{-1} being 0: its bound is 0 and nothing moves it)
        ratio = {k: moved[k] / c["bound"][k] for k in NAMES if c["bound"][k] > 0}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {moved[best]:.3e} against the "
                                      f"bound {c['bound'][best]:.3e}): the case cannot see it")


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["short", "lc_plus_1", "two_tiles"])
def test_copy_with_detach_points_is_the_restatement(tag):
    c = reference(tag)
    p64 = {k: v.double() for k, v in c["p"].items()}
    with torch.no_grad():
        want = M.mamba(c["u"].double(), p64)
        for d in (None,) + G.DEFECTS:                      # a detach point changes the gradient, never the value
            got = G.mamba(c["u"].double(), p64, "", d, lc())
            assert float((got - want).abs().max()) <= 1e-12, (tag, d)


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_cannot_hide_the_defects(tag):
    assert_bound_sees_defects(tag)


def test_cases_reach_the_branches_they_are_named_for():
    n = lc()
    assert [t for t in CASES if "cut_adjoint" in reference(t)["moved"]] == ["lc_plus_1", "three_chunks", "two_tiles", "nine_chunks", "underflow"]
    assert [t for t in CASES if "first_tile_bc" in reference(t)["moved"]] == ["two_tiles"]
    assert CASES["nine_chunks"][0](n)[1] > 8 * n
    r = reference("underflow")
    assert all(bool(torch.isfinite(r["ref64"][k]).all()) for k in NAMES)
    assert float(torch.exp(torch.tensor(-4.0 * 32.0))) < 1e-38          # exp(delta A) at the far states: below float32's normals


def test_host_checks_refuse_unsupported_shapes_before_any_launch():
    lib = _lib.load()
    good = dict(B=2, L=300, d_model=32, d_state=32, d_conv=4, expand=2)
    order = ("B", "L", "d_model", "d_state", "d_conv", "expand")
    need = lib.rf_mamba_backward_workspace_bytes(*[good[k] for k in order])
    assert need >= lib.rf_mamba_workspace_bytes(*[good[k] for k in order]) > 0
    # never dereferenced: the checks come first.  Every buffer has an address of its own, of its true size, clear of the others
    n, plane = 9, 4 * good["B"] * good["L"] * good["d_model"]
    tensors = [4 * math.prod(s) for s in ops.mamba_param_shapes(good["d_model"]).values()]
    at = cases.fake_addresses([plane] * 3 + [need] + 2 * tensors)
    u, g, du, ws = (C.c_void_p(v) for v in at[:4])
    prm, grd = (C.c_void_p * n)(*at[4:4 + n]), (C.c_void_p * n)(*at[4 + n:])
    call = lib.rf_mamba_backward
    for change, word in BAD:
        a = [{**good, **change}[k] for k in order]
        assert lib.rf_mamba_backward_workspace_bytes(*a) < 0
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_mamba_backward_workspace_bytes: ") and word in msg, msg
        assert lib.rf_mamba_backward(u, g, du, prm, grd, ws, 1 << 40, *a, 0, 0, None) < 0
        msg = lib.rf_last_error()
        assert msg.startswith(b"rf_mamba_backward: ") and word in msg, msg
    a = [good[k] for k in order]
    assert lib.rf_mamba_backward(u, g, du, prm, grd, ws, need - 1, *a, 0, 0, None) == -12
    assert lib.rf_last_error().startswith(b"rf_mamba_backward: workspace")
    assert lib.rf_mamba_backward(u, g, du, prm, grd, ws, 1024, *a, 0, 1, None) == -12
    for trio in ((u, u, du), (u, g, u), (u, g, g)):
        assert lib.rf_mamba_backward(*trio, prm, grd, ws, 1 << 40, *a, 0, 0, None) == -22
        assert lib.rf_last_error().startswith(b"rf_mamba_backward: ") and b"alias" in lib.rf_last_error()
    assert lib.rf_mamba_backward(u, g, None, prm, grd, ws, 1 << 40, *a, 0, 0, None) == -22
    assert lib.rf_last_error().startswith(b"rf_mamba_backward: ")

    def refused_as_alias(*args):
        assert call(*args, 1 << 40, *a, 0, 0, None) == -22
        assert lib.rf_last_error().startswith(b"rf_mamba_backward: ") and b"alias" in lib.rf_last_error(), lib.rf_last_error()

    inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
    refused_as_alias(u, g, inside(g, 4096), prm, grd, ws)         # grad_in inside grad_out
    refused_as_alias(u, g, du, prm, grd, inside(u, 16))           # the workspace over in
    refused_as_alias(u, g, du, prm, grd, inside(du, 64))          # ... over grad_in
    refused_as_alias(u, g, du, prm, grd, C.c_void_p(prm[n - 1] - 256))      # ... over a parameter
    for i, target in ((3, prm[5]), (0, du.value), (2, grd[7]), (1, ws.value + 1024), (n - 1, g.value + 32), (4, grd[5] - 16)):
        bad_grd = (C.c_void_p * n)(*grd)
        bad_grd[i] = target                                       # a gradient on a parameter, grad_in, another gradient, the workspace, ...
        refused_as_alias(u, g, du, prm, bad_grd, ws)
    assert call(u, inside(u, 16), du, prm, grd, ws, need - 1, *a, 0, 0, None) == -12      # inputs may overlap: refused for the workspace alone


# ------------------------------------------------------------------------------------------ GPU
def run(device, tag):
    c = reference(tag)
    p = {k: v.to(device) for k, v in c["p"].items()}
    return c, p, c["u"].to(device), c["g"].to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_float64_autograd(device, tag):
    assert_bound_sees_defects(tag)
    c, p, u, g = run(device, tag)
    keep_u, keep_g = u.clone(), g.clone()
    du, grads = ops.mamba_backward(u, p, g)
    du2, grads2 = ops.mamba_backward(u, p, g)
    torch.cuda.synchronize()
    assert torch.equal(u, keep_u) and torch.equal(g, keep_g), f"[{tag}] an input was written"
    got = {"u": du, **grads}
    again = {"u": du2, **grads2}
    assert set(got) == set(NAMES)
    failed = []
    for k in NAMES:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (tag, k)
        assert torch.equal(got[k], again[k]), f"[{tag}] {k}: two runs differ"
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        msg = (f"[{tag}] {k:16s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} max|ref| {c['max'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / max(c['bound'][k], 1e-300):.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
def test_channel_major_is_the_same_operator(device):
    c, p, u, g = run(device, "three_chunks")
    du, grads = ops.mamba_backward(u, p, g)
    du_t, grads_t = ops.mamba_backward(u.transpose(1, 2).contiguous(), p, g.transpose(1, 2).contiguous(), channel_major=True)
    assert torch.equal(du, du_t.transpose(1, 2).contiguous())
    for k in G.KEYS:
        assert torch.equal(grads[k], grads_t[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["lc", "three_chunks"])          # launch_gram2's accumulation and the scalar-row kernel's
def test_passing_grads_accumulates(device, tag):
    c, p, u, g = run(device, tag)
    du, grads = ops.mamba_backward(u, p, g)
    once = {k: v.clone() for k, v in grads.items()}
    du2, same = ops.mamba_backward(u, p, g, grads=grads)
    assert same is grads
    assert torch.equal(du, du2), "grad_u is overwritten, never accumulated"
    for k in G.KEYS:
        assert torch.equal(grads[k], 2.0 * once[k]), k
