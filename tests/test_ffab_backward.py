"""ops.rfft2_polar_backward / polar_irfft2_backward / feb_backward / ffab_backward (csrc/rf_ffab_bwd.hip) against float64 autograd of
the restatement tests/ffab_grad_ref.py.

Loss: ``<op(x, p), g>`` with a fixed random ``g``; truth = ``torch.autograd.grad`` in float64 with respect to ``x`` and every parameter,
e32 = the same computation in float32.  Parameters: ``cases.params`` on ``test_ffab.feb_spec`` / ``ffab_spec``; inputs
``cases.rnd("ffab_bwd.<tag>.x" / ".g")``; seed = SEED + the case's place in its table.

Transforms alone, (b, c, h, w), against autograd of ``torch.fft`` with the symmetric-bin mask; ``grad_pha`` is a random field times
``|F|`` (the gradient of ``angle`` goes as 1 / |F|):

======================  ============================================================================================================
p2 (2,3,16,32)          radix 2 both ways
direct (1,2,10,14)      direct DFT both ways
tall (1,1,24,8)         direct columns, radix-2 rows, three rows of lines per row workgroup trip
odd_h (1,2,5,6)         odd h: only two bins are real by symmetry
all_sym (1,1,2,2)       every bin is real by symmetry; no interior column: neither doubling defect applies
long (1,1,2,4096)       the longest line, 64 KB of LDS
======================  ============================================================================================================

FEB (inputs in +-1.5) and FFAB (inputs in +-1, the forward's fixture shapes):

==========================  ========================================================================================================
feb_all_sym (1,4,2,2)       every bin symmetric: the phase carries no gradient to x, process2.* still receive theirs
feb_base (2,8,8,8)          gram2 with one tap at P = 64 and Pf = 40 (masked: Pf % 16 != 0)
feb_direct (1,4,6,10)       direct DFT both ways, Pf = 36
feb_odd_h (1,4,5,6)         P = 30: the plain weight-gradient kernel on the image plane too
feb_pf9 (1,4,3,4)           spectrum plane of 9 pixels: the plain weight-gradient kernel, scalar rows in the 1x1 GEMMs
feb_wide (1,4,2,64)         partial row groups; three column tiles, the last partial
feb_tall (1,4,64,4)         wf = 3 < the column tile
feb_c64 (1,64,4,4)          several channel tiles
clamp_in (2,8,8,8) +-15     >= 10 % of the inputs and >= 1 % of the outputs clamped: the two +-10 masks
dead4 (1,4,4,4)             row 1 of fpre zeroed: the spectrum of that channel is exactly 0; its gradients must be exactly 0
dead6 (1,4,6,10)            the same on the direct-DFT path
ffab4 (1,4,4,4)             the whole block; 2 nc = 8 channel blocks, the concatenation splits
ffab8 (1,8,8,12)
ffab16 (2,16,16,16)
==========================  ========================================================================================================

Bound, per gradient tensor (the scheme of tests/test_mamba.py, whose RATIO and FLOOR are imported): e64 = max|hip - ref_f64| <=
8 e32 + 2e-6 max|ref_f64|.  ``-s`` prints e64 / bound for every tensor of every case; DESIGN.md, "FFAB backward", holds the table
measured on the MI355X.

Conditions on every case, asserted on the CPU before any comparison:

1. every defect of ffab_grad_ref.DEFECTS that applies to the case (``defects_of``) moves at least one gradient tensor by >= 100 x
   that tensor's bound.  What does not apply, and why:
   * ``sym_bins_leak``: never.  The imaginary parts of the bins (0 | h/2, 0 | w/2) of ``rfft2`` of a REAL plane are identically zero
     functions of the plane (their sine factors are sin(pi n) = 0), so the adjoint of ``rfft2`` maps any gradient arriving there to
     exactly 0: the leak does not move float64 autograd at all (measured: exactly 0 in five cases), and no case can see it.
     test_symmetric_bin_leak_is_invisible_to_autograd asserts that.  The operator still drops the term, as the issue asks.
   * ``clamp_passthrough``: applies where the output clamp of some FEB stops a gradient, i.e. where a pre-clamp sum of the float64
     forward lies outside [-10, 10] (``clamped_outputs``, from the recorded ``sum`` taps): ``clamp_in`` (at least 1 % of its sums),
     ``ffab8`` (4 sums) and ``ffab16`` (870, in the 2 nc blocks, whose inputs exceed 10).  Every other case clamps no output and
     the defect moves nothing there (ratio exactly 0).
   * ``irfft_undoubled`` / ``rfft_as_irfft``: need an interior column, w >= 4.
   * ``no_phase_grad``: needs a bin that is not real by symmetry (not h = w = 2).
2. ``wfb_ref.branch_cut_margins`` >= 100 for every FEB of the case.
3. ``ffab_grad_ref.kink_margin`` >= 100 for every LeakyReLU input (kink at 0) and clamp edge (+-10, 0, 1e4): min |v64 - edge| /
   max(|v32 - v64|, 2^-24 |v64|).  One departure from that formula: a pre-clamp sum that IS +-10 bit for bit in float32 and in
   float64 is counted, not divided, provided the FEB's input is clamped at that pixel on that side and the magnitude MLP of that
   (image, channel) plane is <= 0 at every bin in both precisions (``kink_margin`` checks all three).  Then m = clamp(a, 0, 1e4) = 0
   on the plane, its inverse transform is exactly 0 in any arithmetic, and the sum is the clamped input itself.  The literal formula
   gives 0 there (most FFAB seeds have such planes in the 2 nc blocks), yet nothing is ill-conditioned: the closed interval of
   ``torch.clamp``'s backward passes the gradient in every precision alike, and that the plane stays <= 0 is the ``process1.2`` tap's
   own margin.  A sum on the edge for any other reason stays in the minimum and fails the case.
   The denominator is the float32 perturbation observed at one value, so a margin depends on the float32 FFT and GEMM code paths
   of the CPU that computes it.  SEED is the base, of 5200 .. 5599, with the largest smallest margin: ffab16 181 (a LeakyReLU input,
   one of about 6e5 in that case), ffab8 217, clamp_in 688, every other case >= 1.9e3; the branch-cut margins are 834 (ffab16)
   at the least.  If a CPU ever yields less than 100, the assertion reports the value and the tap.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import cases
import ffab_grad_ref as G
import wfb_ref as W
from bayer_low_light_image_enhancement_amd import _lib, ops
from test_ffab import feb_spec, ffab_spec
from test_mamba import FLOOR, RATIO

SEED = 5470          # of the bases 5200 .. 5599, the one with the largest smallest margin (conditions 2 and 3)
FFT_CASES = {"p2": (2, 3, 16, 32), "direct": (1, 2, 10, 14), "tall": (1, 1, 24, 8), "odd_h": (1, 2, 5, 6), "all_sym": (1, 1, 2, 2),
             "long": (1, 1, 2, 4096)}
# id: (operator, shape, input range, dead fpre row or None), in the order that fixes the seeds
CASES = {
    "feb_all_sym": ("feb", (1, 4, 2, 2), 1.5, None),
    "feb_base": ("feb", (2, 8, 8, 8), 1.5, None),
    "feb_direct": ("feb", (1, 4, 6, 10), 1.5, None),
    "feb_odd_h": ("feb", (1, 4, 5, 6), 1.5, None),
    "feb_pf9": ("feb", (1, 4, 3, 4), 1.5, None),
    "feb_wide": ("feb", (1, 4, 2, 64), 1.5, None),
    "feb_tall": ("feb", (1, 4, 64, 4), 1.5, None),
    "feb_c64": ("feb", (1, 64, 4, 4), 1.5, None),
    "clamp_in": ("feb", (2, 8, 8, 8), 15.0, None),
    "dead4": ("feb", (1, 4, 4, 4), 1.5, 1),
    "dead6": ("feb", (1, 4, 6, 10), 1.5, 1),
    "ffab4": ("ffab", (1, 4, 4, 4), 1.0, None),
    "ffab8": ("ffab", (1, 8, 8, 12), 1.0, None),
    "ffab16": ("ffab", (2, 16, 16, 16), 1.0, None),
}
OPS = {"feb": (G.feb, feb_spec, ops.feb_backward, ops.feb_param_shapes), "ffab": (G.ffab, ffab_spec, ops.ffab_backward, ops.ffab_param_shapes)}


def inputs(tag):
    kind, shape, rng, dead = CASES[tag]
    seed = SEED + list(CASES).index(tag)
    p = cases.params(OPS[kind][1](shape[1]), seed)
    if dead is not None:
        p["fpre.weight"][dead] = 0.0
        p["fpre.bias"][dead] = 0.0
    return p, cases.rnd(f"ffab_bwd.{tag}.x", shape, -rng, rng, seed=seed), cases.rnd(f"ffab_bwd.{tag}.g", shape, seed=seed)


@functools.lru_cache(maxsize=None)
def clamped_outputs(tag):
    """How many pre-clamp sums of the case lie outside [-10, 10] in float64: the values whose gradient the output clamp stops."""
    p, x, _ = inputs(tag)
    return sum(int((v.abs() > 10.0).sum()) for name, v, _ in G.record(OPS[CASES[tag][0]][0], x.double(), f64(p)) if name.endswith("sum"))


def defects_of(tag):
    _, shape, _, _ = CASES[tag]
    h, w = shape[2:]
    out = []
    if (h, w) != (2, 2):
        out.append("no_phase_grad")
    if w >= 4:
        out += ["irfft_undoubled", "rfft_as_irfft"]
    if clamped_outputs(tag) > 0:
        out.append("clamp_passthrough")
    return out


def f64(p):
    return {k: v.double() for k, v in p.items()}


def bounds(ref64, ref32):
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in ref64}
    mx = {k: float(ref64[k].abs().max()) for k in ref64}
    return e32, mx, {k: RATIO * e32[k] + FLOOR * mx[k] for k in ref64}


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Inputs, parameters, the float64 and float32 gradients, the bounds and what each defect moves: computed once, shared, never
    changed."""
    op = OPS[CASES[tag][0]][0]
    p, x, g = inputs(tag)
    ref64 = G.gradients(op, x.double(), f64(p), g.double())
    ref32 = G.gradients(op, x, p, g)
    e32, mx, bound = bounds(ref64, ref32)
    moved = {}
    for d in defects_of(tag):
        bad = G.gradients(op, x.double(), f64(p), g.double(), defect=d)
        moved[d] = {k: float((bad[k] - ref64[k]).abs().max()) for k in ref64}
    return {"x": x, "g": g, "p": p, "ref64": ref64, "e32": e32, "max": mx, "bound": bound, "moved": moved, "names": tuple(ref64)}


def as_block(kind, p, x):
    """wfb_ref's restatement (the one with the spectrum hook) on the case's tensors: FFAB as it is, a FEB inside a ProcessBlock."""
    if kind == "ffab":
        return W.ffab(x, p, "")
    nc = x.shape[1]
    q = {"frequency_process." + k: v for k, v in p.items()}
    q["cat.weight"] = torch.eye(nc, dtype=x.dtype).reshape(nc, nc, 1, 1)
    q["cat.bias"] = torch.zeros(nc, dtype=x.dtype)
    return W.process_block(x, q, "")


@functools.lru_cache(maxsize=None)
def margins(tag):
    kind = CASES[tag][0]
    c = reference(tag)
    cut, where = W.branch_cut_margins(lambda p, x: as_block(kind, p, x), c["p"], c["x"])
    kink, which, on_edge = G.kink_margin(OPS[kind][0], c["x"], c["p"])
    return cut, where, kink, which


def assert_case_is_conditioned(tag):
    c = reference(tag)
    assert all(math.isfinite(c["max"][k]) for k in c["names"]) and c["max"]["x"] > 0
    for d, moved in c["moved"].items():
        ratio = {k: moved[k] / c["bound"][k] for k in c["names"] if c["bound"][k] > 0}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {moved[best]:.3e} against the "
                                      f"bound {c['bound'][best]:.3e}): the case cannot see it")
    cut, where, kink, which = margins(tag)
    assert cut >= 100.0, f"[{tag}] a bin lies {cut:.1f} float32 perturbations from the branch cut of angle ({where})"
    assert kink >= 100.0, f"[{tag}] a value lies {kink:.1f} float32 perturbations from a kink ({which})"


# ---- the transforms alone
def fft_defects(shape):
    return ["rfft_as_irfft", "irfft_undoubled"] if shape[3] >= 4 else []


def fft_loss_fwd(x, gm, gp, defect=None):
    mag, pha = G.polar(G.spectrum(x, defect))
    return (mag * gm).sum() + (pha * gp).sum()


def fft_loss_inv(m, p, go, defect=None):
    return (G.inverse(m, p, go.shape[-2], go.shape[-1], defect) * go).sum()


def grads_of(loss, wrt, *rest, defect=None):
    wrt = [t.detach().clone().requires_grad_(True) for t in wrt]
    return [t.detach() for t in torch.autograd.grad(loss(*wrt, *rest, defect=defect), wrt)]


@functools.lru_cache(maxsize=None)
def fft_reference(tag):
    shape = FFT_CASES[tag]
    b, c, h, w = shape
    seed = SEED + 100 + list(FFT_CASES).index(tag)
    half = (b, c, h, w // 2 + 1)
    x = cases.rnd(f"ffab_bwd.fft.{tag}.x", shape, seed=seed)
    gm = cases.rnd(f"ffab_bwd.fft.{tag}.gm", half, seed=seed)
    gp = (cases.rnd(f"ffab_bwd.fft.{tag}.gp", half, seed=seed).double() * G.spectrum(x.double()).abs()).float()
    m = cases.rnd(f"ffab_bwd.fft.{tag}.m", half, 0.0, 2.0, seed=seed)
    p = cases.rnd(f"ffab_bwd.fft.{tag}.p", half, -3.0, 3.0, seed=seed)
    go = cases.rnd(f"ffab_bwd.fft.{tag}.go", shape, seed=seed)
    ref64, ref32, moved = {}, {}, {}
    (ref64["x"],) = grads_of(fft_loss_fwd, [x.double()], gm.double(), gp.double())
    (ref32["x"],) = grads_of(fft_loss_fwd, [x], gm, gp)
    ref64["mag"], ref64["pha"] = grads_of(fft_loss_inv, [m.double(), p.double()], go.double())
    ref32["mag"], ref32["pha"] = grads_of(fft_loss_inv, [m, p], go)
    e32, mx, bound = bounds(ref64, ref32)
    for d in fft_defects(shape):
        if d == "rfft_as_irfft":
            (bad,) = grads_of(fft_loss_fwd, [x.double()], gm.double(), gp.double(), defect=d)
            moved[d] = float((bad - ref64["x"]).abs().max()) / bound["x"]
        else:
            bm, bp = grads_of(fft_loss_inv, [m.double(), p.double()], go.double(), defect=d)
            moved[d] = max(float((bm - ref64["mag"]).abs().max()) / bound["mag"], float((bp - ref64["pha"]).abs().max()) / bound["pha"])
    return {"x": x, "gm": gm, "gp": gp, "m": m, "p": p, "go": go, "ref64": ref64, "e32": e32, "max": mx, "bound": bound, "moved": moved}


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["feb_odd_h", "clamp_in", "dead6", "ffab8"])
def test_restatement_has_the_forward_value_with_and_without_defects(tag):
    kind = CASES[tag][0]
    c = reference(tag)
    with torch.no_grad():
        want = as_block(kind, f64(c["p"]), c["x"].double())
        if kind == "feb":
            want = want - c["x"].double()                       # the ProcessBlock's skip; cat is the identity
        for d in (None,) + G.DEFECTS:                            # a defect changes the gradient, never the value
            got = OPS[kind][0](c["x"].double(), f64(c["p"]), "", d)
            assert float((got - want).abs().max()) <= 1e-12, (tag, d)


@pytest.mark.parametrize("tag", list(CASES))
def test_cases_are_conditioned_and_the_bound_sees_the_defects(tag):
    assert_case_is_conditioned(tag)
    cut, where, kink, which = margins(tag)
    print(f"[{tag}] branch cut margin {cut:.3g} {where} | kink margin {kink:.3g} ({which}) | defects x bound: "
          + ", ".join(f"{d} {max(m[k] / reference(tag)['bound'][k] for k in m if reference(tag)['bound'][k] > 0):.3g}"
                      for d, m in reference(tag)["moved"].items()))


@pytest.mark.parametrize("tag", list(FFT_CASES))
def test_transform_cases_see_the_doubling_defects(tag):
    c = fft_reference(tag)
    assert set(c["moved"]) == set(fft_defects(FFT_CASES[tag]))
    for d, r in c["moved"].items():
        assert r >= 100.0, (tag, d, r)


@pytest.mark.parametrize("tag", ["feb_base", "feb_odd_h", "ffab8"])
def test_symmetric_bin_leak_is_invisible_to_autograd(tag):
    """Why no case lists ``sym_bins_leak``: see the module docstring."""
    kind = CASES[tag][0]
    c = reference(tag)
    bad = G.gradients(OPS[kind][0], c["x"].double(), f64(c["p"]), c["g"].double(), defect="sym_bins_leak")
    for k in c["names"]:
        assert float((bad[k] - c["ref64"][k]).abs().max()) <= 1e-12 * max(c["max"][k], 1.0), k


def test_cases_reach_the_branches_they_are_named_for():
    shp = {t: CASES[t][1] for t in CASES}
    P = {t: s[2] * s[3] for t, s in shp.items()}
    Pf = {t: s[2] * (s[3] // 2 + 1) for t, s in shp.items()}
    assert [t for t in CASES if P[t] % 4 != 0] == ["feb_odd_h"]                                  # the plain weight gradient, image plane
    assert [t for t in CASES if Pf[t] % 4 != 0] == ["feb_pf9", "feb_wide"] and Pf["feb_pf9"] == 9      # ... on the spectrum plane
    assert Pf["feb_base"] % 16 != 0 and Pf["feb_base"] % 4 == 0                                  # gram2's masked form
    lib = _lib.load()
    plan = (C.c_int * 10)()
    for t, (l2w, l2h) in {"feb_base": (3, 3), "feb_direct": (-1, -1), "feb_odd_h": (-1, -1), "feb_tall": (2, 6), "feb_wide": (6, 1)}.items():
        b, c, h, w = shp[t]
        assert lib.rf_fft_plan(b * c, h, w, plan) == 0 and (plan[0], plan[1]) == (l2w, l2h), (t, list(plan))
    b, c, h, w = shp["feb_wide"]
    assert lib.rf_fft_plan(b * c, h, w, plan) == 0
    assert plan[2] == 32 and b * c * h == 8 and (w // 2 + 1) == 33 and plan[3] == 16            # 8 of a row group's 32 lines; column tiles 16, 16, 1
    b, c, h, w = shp["feb_tall"]
    assert lib.rf_fft_plan(b * c, h, w, plan) == 0 and w // 2 + 1 == 3 < plan[3]
    b, c, h, w = FFT_CASES["long"]
    assert lib.rf_fft_plan(b * c, h, w, plan) == 0 and plan[8] == 65536
    assert {t: clamped_outputs(t) for t in CASES if clamped_outputs(t)}.keys() == {"clamp_in", "ffab8", "ffab16"}      # who lists clamp_passthrough
    assert clamped_outputs("ffab8") == 4 and clamped_outputs("ffab16") == 870
    assert all(("clamp_passthrough" in reference(t)["moved"]) == (clamped_outputs(t) > 0) for t in CASES)
    c = reference("clamp_in")
    taps = G.record(G.feb, c["x"], c["p"])
    xin = [v for n, v, _ in taps if n == "x"][0]
    s = [v for n, v, _ in taps if n == "sum"][0]
    assert float((xin.abs() > 10).float().mean()) >= 0.10 and float((s.abs() > 10).float().mean()) >= 0.01
    for t in ("dead4", "dead6"):
        c = reference(t)
        f = G.spectrum(torch.nn.functional.conv2d(c["x"].clamp(-10, 10), c["p"]["fpre.weight"], c["p"]["fpre.bias"]))
        assert float(f[:, 1].abs().max()) == 0.0 and float(f[:, 0].abs().min()) > 0.0
        assert float(c["ref64"]["fpre.weight"][1].abs().max()) == 0.0 and float(c["ref64"]["fpre.bias"][1].abs()) == 0.0
        assert all(bool(torch.isfinite(v).all()) for v in c["ref64"].values())
    c = reference("feb_all_sym")                                  # no gradient to x through the phase, one to process2.*
    no_phase = G.gradients(G.feb, c["x"].double(), f64(c["p"]), c["g"].double(), defect="no_phase_grad")
    assert torch.equal(no_phase["x"], c["ref64"]["x"]) and c["max"]["process2.0.weight"] > 0 and c["max"]["process2.2.weight"] > 0


def test_param_shapes_follow_the_forward_specs():
    for nc in (4, 16):
        assert ops.feb_param_shapes(nc) == feb_spec(nc) and list(ops.feb_param_shapes(nc)) == list(G.FEB_KEYS)
        assert ops.ffab_param_shapes(nc) == ffab_spec(nc) and list(ops.ffab_param_shapes(nc)) == list(ffab_spec(nc))


def test_host_checks_refuse_unsupported_shapes_before_any_launch():
    lib = _lib.load()
    # 16-byte aligned, far apart, never dereferenced: the checks come first, and no call below passes all of them
    x, g, dx, y, z = (C.c_void_p(a << 30) for a in (1, 2, 3, 6, 7))
    ws = C.c_void_p(1 << 40)
    odd = C.c_void_p((3 << 30) + 4)
    for name, n in (("feb", 10), ("ffab", 92)):
        query, call = getattr(lib, f"rf_{name}_backward_workspace_bytes"), getattr(lib, f"rf_{name}_backward")
        fwd = getattr(lib, f"rf_{name}_scratch_bytes")

        def arrays():
            return ((C.c_void_p * n)(*[(4 << 30) + (i << 20) for i in range(n)]), (C.c_void_p * n)(*[(5 << 30) + (i << 20) for i in range(n)]))

        prm, grd = arrays()
        good = (2, 16, 16, 24)
        need = query(*good)
        assert need > 0
        for bad, word in (((2, 18, 16, 24), b"channels"), ((0, 16, 16, 24), b"channels"), ((2, 16, 16, 23), b"even width"),
                          ((2, 16, 4100, 24), b"4100"), ((2, 16, 16, 3000), b"3000"), ((2, 16, 1, 24), b"channels")):
            assert query(*bad) < 0
            msg = lib.rf_last_error()
            assert msg.startswith(f"rf_{name}_backward_workspace_bytes: ".encode()) and word in msg, msg
            assert call(x, g, dx, prm, grd, ws, 1 << 40, *bad, 0, None) == -22
            msg = lib.rf_last_error()
            assert msg.startswith(f"rf_{name}_backward: ".encode()) and word in msg, msg
        for ok in ((1, 4, 2, 2), (1, 4, 3, 4), (1, 4, 5, 6), (2, 16, 16, 16), (1, 8, 2048, 4), (1, 4, 2, 4096), (1, 4, 6, 2046)):
            sz = C.c_size_t()
            assert fwd(*ok, C.byref(sz)) == 0 and query(*ok) >= sz.value > 0          # every shape the forward accepts, and more room
        assert call(x, g, dx, prm, grd, ws, need - 1, *good, 0, None) == -12
        assert lib.rf_last_error().startswith(f"rf_{name}_backward: workspace".encode())

        def refused_as_alias(*args):
            assert call(*args, 1 << 40, *good, 0, None) == -22
            assert lib.rf_last_error().startswith(f"rf_{name}_backward: ".encode()) and b"alias" in lib.rf_last_error(), lib.rf_last_error()

        inside = lambda base, off: C.c_void_p(base.value + off)      # noqa: E731
        refused_as_alias(x, g, x, prm, grd, ws)                       # grad_in on in
        refused_as_alias(x, g, g, prm, grd, ws)                       # grad_in on grad_out
        refused_as_alias(x, g, inside(g, 4096), prm, grd, ws)         # ... or inside it
        refused_as_alias(x, g, dx, prm, grd, inside(x, 16))           # the workspace over in
        refused_as_alias(x, g, dx, prm, grd, inside(dx, 64))          # ... over grad_in
        refused_as_alias(x, g, dx, prm, grd, C.c_void_p(prm[n - 1] - 256))      # ... over a parameter
        for i, target in ((3, prm[5]), (0, dx.value), (2, grd[7]), (1, ws.value + 1024), (n - 1, g.value + 32), (4, grd[5] - 16)):
            _, bad_grd = arrays()
            bad_grd[i] = target                                       # a gradient on a parameter, grad_in, another gradient, the workspace, ...
            refused_as_alias(x, g, dx, prm, bad_grd, ws)
        assert call(x, x, dx, prm, grd, ws, need - 1, *good, 0, None) == -12      # inputs may overlap one another: refused for the workspace alone
        assert call(x, g, None, prm, grd, ws, 1 << 40, *good, 0, None) == -22
        assert call(x, g, odd, prm, grd, ws, 1 << 40, *good, 0, None) == -22 and b"aligned" in lib.rf_last_error()
        grd[n - 1] = None
        assert call(x, g, dx, prm, grd, ws, 1 << 40, *good, 0, None) == -22 and b"null" in lib.rf_last_error()
    for name, args in (("rf_rfft2_polar_backward", (x, g, y, dx, ws)), ("rf_polar_irfft2_backward", (x, g, y, dx, z, ws))):
        query, call = getattr(lib, name + "_scratch_bytes"), getattr(lib, name)
        assert query(6, 16, 24) == 6 * 16 * 13 * 8
        for bad in ((6, 16, 23), (6, 4100, 24), (6, 16, 3000), (0, 16, 24), (6, 1, 24)):
            assert query(*bad) < 0 and lib.rf_last_error().startswith((name + "_scratch_bytes: ").encode())
            assert call(*args, *bad, None) == -22 and lib.rf_last_error().startswith((name + ": ").encode())
        for i in range(len(args)):
            assert call(*args[:i], None, *args[i + 1:], 6, 16, 24, None) == -22
            assert call(*args[:i], odd, *args[i + 1:], 6, 16, 24, None) == -22 and b"aligned" in lib.rf_last_error()
        nin = 3
        for i in range(nin, len(args)):                          # an output or the scratch on top of an input, or of each other
            for j in range(i):
                assert call(*args[:i], args[j], *args[i + 1:], 6, 16, 24, None) == -22 and b"alias" in lib.rf_last_error(), (name, i, j)


# ------------------------------------------------------------------------------------------ GPU
def report(tag, c, got, again):
    failed = []
    for k in c["bound"]:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (tag, k)
        assert torch.equal(got[k], again[k]), f"[{tag}] {k}: two runs differ"
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        msg = (f"[{tag}] {k:44s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} S {c['max'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / max(c['bound'][k], 1e-300):.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(FFT_CASES))
def test_transform_adjoints_match_float64_autograd(device, tag):
    c = fft_reference(tag)
    assert all(r >= 100.0 for r in c["moved"].values())
    d = {k: c[k].to(device) for k in ("x", "gm", "gp", "m", "p", "go")}
    keep = {k: v.clone() for k, v in d.items()}

    def once():
        gx = ops.rfft2_polar_backward(d["x"], d["gm"], d["gp"])
        gmag, gpha = ops.polar_irfft2_backward(d["m"], d["p"], d["go"])
        return {"x": gx, "mag": gmag, "pha": gpha}

    got, again = once(), once()
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], keep[k]) for k in d), f"[{tag}] an input was written"
    report(tag, c, got, again)


def run(device, tag):
    c = reference(tag)
    p = {k: v.to(device) for k, v in c["p"].items()}
    return c, p, c["x"].to(device), c["g"].to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_matches_float64_autograd(device, tag):
    assert_case_is_conditioned(tag)
    c, p, x, g = run(device, tag)
    backward = OPS[CASES[tag][0]][2]
    keep_x, keep_g, keep_p = x.clone(), g.clone(), {k: v.clone() for k, v in p.items()}
    dx, grads = backward(x, p, g)
    dx2, grads2 = backward(x, p, g)
    torch.cuda.synchronize()
    assert torch.equal(x, keep_x) and torch.equal(g, keep_g), f"[{tag}] an input was written"
    assert all(torch.equal(p[k], keep_p[k]) for k in p), f"[{tag}] a parameter was written"
    got = {"x": dx, **grads}
    assert set(got) == set(c["names"])
    dead = CASES[tag][3]
    if dead is not None:
        assert float(grads["fpre.weight"][dead].abs().max()) == 0.0 and float(grads["fpre.bias"][dead].abs()) == 0.0
    report(tag, c, got, {"x": dx2, **grads2})


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["feb_base", "feb_odd_h", "ffab4"])          # launch_gram2's accumulation and the plain kernel's
def test_passing_grads_accumulates(device, tag):
    c, p, x, g = run(device, tag)
    backward = OPS[CASES[tag][0]][2]
    dx, grads = backward(x, p, g)
    once = {k: v.clone() for k, v in grads.items()}
    dx2, same = backward(x, p, g, grads=grads)
    assert same is grads and set(grads) == set(c["p"])
    assert torch.equal(dx, dx2), "grad_x is overwritten, never accumulated"
    for k in grads:
        assert torch.equal(grads[k], 2.0 * once[k]), k


GUARD = 64


def guarded(shape, device):
    """A tensor of `shape` inside a NaN-filled buffer, 16-byte aligned, and the buffer's tail."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), float("nan"), device=device)
    return buf[:n].view(shape), buf[n:]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["feb_pf9", "feb_odd_h", "feb_base", "ffab4"])
def test_nothing_is_written_past_an_output(device, tag):
    kind = CASES[tag][0]
    c, p, x, g = run(device, tag)
    keys = list(OPS[kind][3](x.shape[1]))
    lib = _lib.load()
    query, call = getattr(lib, f"rf_{kind}_backward_workspace_bytes"), getattr(lib, f"rf_{kind}_backward")
    dx, tails = guarded(tuple(x.shape), device)
    tails = [tails]
    gs = []
    for k in keys:
        t, tail = guarded(tuple(p[k].shape), device)
        gs.append(t)
        tails.append(tail)
    ws = torch.empty(query(*x.shape), dtype=torch.uint8, device=device)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])       # noqa: E731
    with torch.cuda.device(device):
        _lib.check(call(ptr(x), ptr(g), ptr(dx), arr([p[k] for k in keys]), arr(gs), ptr(ws), ws.numel(), *x.shape, 0,
                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "backward")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in tails), "written past an output"
    want_dx, want = OPS[kind][2](x, p, g)
    assert torch.equal(dx, want_dx) and all(torch.equal(a, want[k]) for k, a in zip(keys, gs))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["odd_h", "p2"])
def test_nothing_is_written_past_a_transform_output(device, tag):
    c = fft_reference(tag)
    d = {k: c[k].to(device) for k in ("x", "gm", "gp", "m", "p", "go")}
    b, ch, h, w = d["x"].shape
    lib = _lib.load()
    gx, t0 = guarded(tuple(d["x"].shape), device)
    gmag, t1 = guarded(tuple(d["m"].shape), device)
    gpha, t2 = guarded(tuple(d["m"].shape), device)
    scratch = torch.empty(lib.rf_rfft2_polar_backward_scratch_bytes(b * ch, h, w), dtype=torch.uint8, device=device)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(device):
        _lib.check(lib.rf_rfft2_polar_backward(ptr(d["x"]), ptr(d["gm"]), ptr(d["gp"]), ptr(gx), ptr(scratch), b * ch, h, w, st), "rfft2 backward")
        _lib.check(lib.rf_polar_irfft2_backward(ptr(d["m"]), ptr(d["p"]), ptr(d["go"]), ptr(gmag), ptr(gpha), ptr(scratch), b * ch, h, w, st),
                   "irfft2 backward")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (t0, t1, t2)), "written past an output"
    assert torch.equal(gx, ops.rfft2_polar_backward(d["x"], d["gm"], d["gp"]))
    wm, wp = ops.polar_irfft2_backward(d["m"], d["p"], d["go"])
    assert torch.equal(gmag, wm) and torch.equal(gpha, wp)
