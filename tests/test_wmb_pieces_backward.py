"""The gradient pieces of the WMB block (csrc/rf_wmb_bwd.hip): ops.wmb_front_backward, ops.wmb_back_backward, ops.dwconv5x5_backward,
ops.illumination_estimator_backward and ops.layernorm2d_backward against float64 autograd of the restatements in tests/wmb_grad_ref.py.

Truth: ``torch.autograd.grad`` of ``<f(inputs), g>`` in float64 over ``R.layernorm2d`` / ``R.dwt_init`` (oracle.rawformer_ref),
``wmb_grad_ref.iwt`` (``R.iwt_init`` for any dtype; shown below to be ``R.iwt_init`` bit for bit in float32), ``R.illumination_estimator``
(pinned by tests/golden/wfb_extras.npz) and ``F.conv2d``; e32 = the same computation in float32.  Inputs: ``cases.rnd("<op>.<tag>.*",
seed=4700 + 16 * place)``, place = the case's place in its table.

Bound, per output tensor: the scheme of tests/test_mamba.py, whose RATIO and FLOOR are imported: e64 = max|hip - ref_f64| <= 8 e32 +
2e-6 S with S = max|ref_f64|.  No tensor here is a sum that cancels to about 0 against its summands (the CPU test below asserts
max|ref_f64| >= 1e-3 max_c sum|summands| for every parameter gradient whose summands the restatement exposes: the two of the front, the
5x5's bias), so S is the plain maximum everywhere.  Two kinds of tensor are exact zeros and compared as such: the ``conv2.*`` gradients
of an illumination call without ``grad_map``, and nothing else.  ``-s`` prints e64 / bound for every tensor; DESIGN.md section 4, "WMB
backward pieces", holds the table measured on the MI355X.

Condition on the bound (CPU, and again at the head of each GPU test): every defect of wmb_grad_ref moves at least one gradient tensor of
every case of its operator by >= 100 x that tensor's bound.  One exception that arithmetic forces: ``taps_unflipped`` at ``one_px``, where
only the centre tap touches the one pixel and flipping the taps changes nothing; the test asserts that it moves exactly 0 there.

Cases.  front and back, (B, C, h, w) of the band; KS = the lanes that share an item's channels in wmb_front_bwd_kernel:

================  ==============  =================================================================================================
one_item          (1,4,1,2)       one item; KS = 4, one channel per lane
base              (2,16,4,4)      KS = 4, four channels per lane
odd               (1,24,3,6)      KS = 8, three channels per lane; full-resolution width 12: no multiple of 8
blocks            (2,4,17,32)     272 items per image on 64 per workgroup: 5 workgroups (= slabs) per image, the last partial; two images
c512              (1,512,1,2)     the largest C: KS = 64, eight channels per lane
masked            (1,6,1,2)       C no multiple of KS: two of the eight channel slots are masked
c48, c128         (1,48,1,2) ..   KS = 16 and KS = 32
trips             (64,4,33,64)    front only: 64 images cap the grid at 8 workgroups per image; 1056 items on 8 x 64: a third,
                                  partial trip.  The back pass has no such branch below 2^20 items per call (its grid-stride loop), and
                                  a draw that large cannot keep every value 1e-5 away from the clamp's edges: its second trip is not run
================  ==============  =================================================================================================

5x5 and illumination, (B, C, Cm, Co, h, w) (the 5x5 runs on the Cm planes):

================  ======================  =========================================================================================
one_px            (1,4,4,4,1,1)           one pixel
small             (1,4,4,4,2,3)           the image inside the window: every tap clipped somewhere
base              (2,16,16,16,8,8)        gram2 weight gradients, float4 rows
w_mod4_2          (2,16,16,16,6,10)       P % 4 == 0 but w % 4 == 2: scalar row ends in the 5x5 weight gradient
mixed             (1,8,12,4,5,7)          three different channel counts, odd sizes: the plain 1x1 weight-gradient kernels
c256              (1,256,256,256,4,4)     level-3 channels
slabs             (2,4,4,4,8,516)         8 x 129 = 1032 groups of 4 pixels: rf_dwconv5x5_backward_nblk = 2 slabs per plane, two images
================  ======================  =========================================================================================

Illumination runs with ``grad_map`` on ``base`` and ``mixed`` too.  layernorm2d_backward: (2,16,8,8) (ln_bwd_reg_kernel) and (1,24,5,7) (the
generic kernels), with and without ``residual``.

Host checks (CPU, fake addresses): every entry point refuses null, misaligned and aliased pointers, a workspace that is too small and
channel counts outside its range; the two band operators an odd band width.  rf_wmb_back_backward has no workspace and the 5x5,
illumination and LayerNorm operators take any width, so those refusals do not exist for them.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import cases
import wmb_grad_ref as G
from bayer_low_light_image_enhancement_amd import _lib, ops
from oracle import rawformer_ref as R
from test_mamba import FLOOR, RATIO

# the operators under test: without them nothing below has a subject, and the module stops at the first one that is missing
OPERATORS = (ops.wmb_front_backward, ops.wmb_back_backward, ops.dwconv5x5_backward, ops.illumination_estimator_backward, ops.layernorm2d_backward)

# operator -> (case table, inputs, gradients(inputs, defect=None), defects)
OPS = {
    "front": (G.BAND_CASES, G.front_inputs, G.front_grads, G.FRONT_DEFECTS),
    "back": (G.BACK_CASES, G.back_inputs, G.back_grads, G.BACK_DEFECTS),
    "dw5": (G.ILLU_CASES, G.dw5_inputs, G.dw5_grads, G.DW5_DEFECTS),
    "illu": (G.ILLU_CASES, G.illu_inputs, lambda i, defect=None: G.illu_grads(i, False, defect), G.ILLU_DEFECTS[:2]),
    "illu_map": (G.ILLU_CASES, G.illu_inputs, lambda i, defect=None: G.illu_grads(i, True, defect), G.ILLU_DEFECTS),
    "ln": (G.LN_CASES, G.ln_inputs, lambda i, defect=None: G.ln_grads(i, False), ()),
    "ln_res": (G.LN_CASES, G.ln_inputs, lambda i, defect=None: G.ln_grads(i, True), ()),
}
RUNS = ([("front", t) for t in G.BAND_CASES] + [("back", t) for t in G.BACK_CASES] + [("dw5", t) for t in G.ILLU_CASES]
        + [("illu", t) for t in G.ILLU_CASES] + [("illu_map", t) for t in ("base", "mixed")]
        + [(o, t) for o in ("ln", "ln_res") for t in G.LN_CASES])
IDS = [f"{o}-{t}" for o, t in RUNS]
CONV2 = ("conv2.weight", "conv2.bias")


@functools.lru_cache(maxsize=None)
def reference(op, tag):
    """Inputs, the float64 and float32 gradients, the bounds and what each defect moves: computed once, shared, never changed."""
    _, inputs, grads, defects = OPS[op]
    i = inputs(tag)
    i64 = G.as_dtype(i, torch.float64)
    ref64, ref32 = grads(i64), grads(i)
    names = tuple(ref64)
    assert all(ref64[k].dtype == torch.float64 and ref32[k].dtype == torch.float32 for k in names)
    e32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in names}
    scale = {k: float(ref64[k].abs().max()) for k in names}
    bound = {k: RATIO * e32[k] + FLOOR * scale[k] for k in names}
    moved = {d: {k: float((v - ref64[k]).abs().max()) for k, v in grads(i64, defect=d).items()} for d in defects}
    return {"i": i, "ref64": ref64, "e32": e32, "scale": scale, "bound": bound, "moved": moved, "names": names}


def assert_bound_sees_defects(op, tag):
    c = reference(op, tag)
    zero = CONV2 if op == "illu" else ()
    for k in c["names"]:
        assert math.isfinite(c["scale"][k]) and ((c["scale"][k] == 0.0) if k in zero else (c["bound"][k] > 0.0)), (op, tag, k)
    for d, moved in c["moved"].items():
        if (op, tag, d) == ("dw5", "one_px", "taps_unflipped"):      # one pixel meets the centre tap only: the flip changes nothing
            assert all(v == 0.0 for v in moved.values())
            continue
        ratio = {k: moved[k] / c["bound"][k] for k in c["names"] if k not in zero}
        best = max(ratio, key=ratio.get)
        assert ratio[best] >= 100.0, (f"[{op} {tag}] defect {d} moves no gradient by 100 x its bound (most: {best}, {moved[best]:.3e} against "
                                      f"the bound {c['bound'][best]:.3e}): the case cannot see it")
        if d in ("no_mean_fold", "taps_unflipped"):
            target = "img" if d == "no_mean_fold" else "x"
            assert best == target and all(moved[k] == 0.0 for k in c["names"] if k != target), (op, tag, d)
        if d == "no_mean_column":
            assert best == "conv1.weight"


# ------------------------------------------------------------------------------------------ CPU
def test_iwt_restatement_is_the_oracle_in_float32():
    for tag in ("base", "odd"):
        bands = G.back_inputs(tag)["bands"]
        assert torch.equal(G.iwt(bands), R.iwt_init(bands)) and G.iwt(bands.double()).dtype == torch.float64
        t = G.front_inputs(tag)["x"]
        assert float((G.iwt(R.dwt_init(t.double())) - t.double()).abs().max()) < 1e-15      # the Haar pair is orthogonal


@pytest.mark.parametrize("op,tag", RUNS, ids=IDS)
def test_bound_cannot_hide_the_defects(op, tag):
    assert_bound_sees_defects(op, tag)


@pytest.mark.parametrize("tag", list(G.BACK_CASES))
def test_clamp_cuts_both_sides_and_float32_agrees(tag):
    i = G.back_inputs(tag)
    low, high, gap, same = G.back_condition(i["bands"])
    print(f"[back {tag}] seed try {i['tries']}: cut low {low:.3f}, cut high {high:.3f}, nearest pre-clamp value to 0 or 1 {gap:.3e}")
    assert i["tries"] <= 4 and low >= 0.1 and high >= 0.1 and gap > 1e-5 and same
    assert float(i["bands"].abs().max()) < 2.0


def test_no_parameter_gradient_is_a_cancelling_sum():
    for tag in G.BAND_CASES:
        i = G.as_dtype(G.front_inputs(tag), torch.float64)
        x = i["x"]
        mu = x.mean(dim=1, keepdim=True)
        xh = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(dim=1, keepdim=True) + 1e-5)
        g = i["grad_t"] + G.iwt(i["grad_bands"])
        ref = reference("front", tag)["ref64"]
        assert float((ref["weight2"] - G.GRAD_SCALE * (g * xh).sum(dim=(0, 2, 3))).abs().max()) <= 1e-10 * float(ref["weight2"].abs().max())
        for k, summands in (("weight2", g * xh), ("bias2", g)):
            s = G.GRAD_SCALE * float(summands.abs().sum(dim=(0, 2, 3)).max())
            assert float(ref[k].abs().max()) >= 1e-3 * s, (tag, k)
    for tag in G.ILLU_CASES:
        i, ref = G.dw5_inputs(tag), reference("dw5", tag)["ref64"]
        assert float(ref["bias"].abs().max()) >= 1e-3 * float(i["grad_out"].double().abs().sum(dim=(0, 2, 3)).max()), tag


def test_cases_reach_the_branches_they_are_named_for():
    lib = _lib.load()
    nblk, nblk5 = lib.rf_wmb_front_backward_nblk, lib.rf_dwconv5x5_backward_nblk
    ks = {t: next(k for k in (4, 8, 16, 32, 64) if k == 64 or -(-s[1] // k) <= 4) for t, s in G.BAND_CASES.items()}
    assert ks == {"one_item": 4, "base": 4, "odd": 8, "blocks": 4, "c512": 64, "masked": 4, "c48": 16, "c128": 32, "trips": 4}
    assert G.BAND_CASES["masked"][1] % ks["masked"] and all(s[1] % ks[t] == 0 for t, s in G.BAND_CASES.items() if t != "masked")
    assert (2 * G.BAND_CASES["odd"][3]) % 8 and G.BAND_CASES["c512"][1] == 512
    items = {t: s[2] * s[3] // 2 for t, s in G.BAND_CASES.items()}
    per_wg = {t: 4 * 64 // ks[t] for t in ks}
    assert [nblk(*s) for s in G.BAND_CASES.values()] == [1, 1, 1, 5, 1, 1, 1, 1, 8]
    assert items["blocks"] == 272 and per_wg["blocks"] == 64 and G.BAND_CASES["blocks"][0] == 2          # 4 full workgroups and 16 items
    assert items["trips"] == 1056 and 2 * 8 * per_wg["trips"] == 1024 and nblk(63, 4, 33, 64) == 9        # the cap: ceil(512 / B)
    assert nblk(1, 3, 1, 2) == -22 and nblk(1, 4, 1, 3) == -22
    # 5x5: one slab per 1024 groups of 4 pixels
    shapes = {t: s[4:] for t, s in G.ILLU_CASES.items()}
    assert [nblk5(*s) for s in shapes.values()] == [1, 1, 1, 1, 1, 1, 2] and G.ILLU_CASES["slabs"][0] == 2
    h, w = shapes["slabs"]
    assert h * ((w + 3) // 4) == 1032 and nblk5(h, w - 8) == 1 and nblk5(h - 1, w) == 1 and nblk5(4096, 4096) == 32 and nblk5(0, 4) == -22
    assert shapes["one_px"] == (1, 1) and max(shapes["small"]) <= 3                                       # inside the 5 x 5 window
    assert shapes["w_mod4_2"][1] % 4 == 2 and (shapes["w_mod4_2"][0] * shapes["w_mod4_2"][1]) % 4 == 0
    assert (shapes["mixed"][0] * shapes["mixed"][1]) % 4 and len(set(G.ILLU_CASES["mixed"][1:4])) == 3
    assert (shapes["base"][0] * shapes["base"][1]) % 4 == 0 and G.ILLU_CASES["c256"][1:4] == (256, 256, 256)
    assert G.LN_CASES["base"][1] == 16 and (G.LN_CASES["odd"][2] * G.LN_CASES["odd"][3]) % 4


# ---- host checks.  Every entry point as (pointer names in call order, byte size of each, which are written, call tail)
def entry(name):
    lib = _lib.load()
    if name == "rf_wmb_front_backward":
        geo, plane, vec = (2, 16, 4, 4), 4 * 2 * 16 * 8 * 8, 4 * 16
        need = lib.rf_wmb_front_backward_workspace_bytes(*geo)
        ptrs = {"x": plane, "grad_t": plane, "grad_x": plane, "grad_bands": plane, "weight2": vec, "grad_weight2": vec, "grad_bias2": vec, "ws": need}
        return dict(ptrs=ptrs, outs=("grad_x", "grad_weight2", "grad_bias2", "ws"), geo=geo, tail=(2.0, 0, None), need=need,
                    aligned=("x", "grad_t", "grad_x", "grad_bands", "ws"), query=lib.rf_wmb_front_backward_workspace_bytes,
                    bad=(((2, 3, 4, 4), b"C 3"), ((2, 516, 4, 4), b"C 516"), ((2, 16, 4, 3), b"4 x 3"), ((0, 16, 4, 4), b"B 0")))
    if name == "rf_wmb_back_backward":
        geo, plane = (2, 16, 4, 4), 4 * 2 * 16 * 8 * 8
        return dict(ptrs={"bands": plane, "grad_out": plane, "grad_bands": plane}, outs=("grad_bands",), geo=geo, tail=(None,), need=None,
                    aligned=("bands", "grad_out", "grad_bands"), query=None,
                    bad=(((2, 3, 4, 4), b"C 3"), ((2, 513, 4, 4), b"C 513"), ((2, 16, 4, 5), b"4 x 5"), ((2, 16, 0, 4), b"0 x 4")))
    if name == "rf_dwconv5x5_backward":
        geo, plane = (2, 16, 8, 8), 4 * 2 * 16 * 64
        need = lib.rf_dwconv5x5_backward_workspace_bytes(*geo)
        ptrs = {"in": plane, "grad_out": plane, "grad_in": plane, "weight": 1600, "grad_weight": 1600, "grad_bias": 64, "ws": need}
        return dict(ptrs=ptrs, outs=("grad_in", "grad_weight", "grad_bias", "ws"), geo=geo, tail=(0, None), need=need,
                    aligned=("in", "grad_out", "grad_in", "ws"), query=lib.rf_dwconv5x5_backward_workspace_bytes,
                    bad=(((2, 0, 8, 8), b"C 0"), ((2, 70000, 8, 8), b"C 70000"), ((2, 16, 8, 0), b"8 x 0")))
    if name == "rf_layernorm2d_backward":
        geo, plane = (2, 16, 8, 8), 4 * 2 * 16 * 64
        need = lib.rf_layernorm2d_backward_workspace_bytes(*geo)
        ptrs = {"in": plane, "grad_out": plane, "grad_in": plane, "weight": 64, "grad_weight": 64, "grad_bias": 64, "residual": plane, "ws": need}
        return dict(ptrs=ptrs, outs=("grad_in", "grad_weight", "grad_bias", "ws"), geo=geo, tail=(1e-5, 0, None), need=need,
                    aligned=("in", "grad_out", "grad_in", "residual", "ws"), query=lib.rf_layernorm2d_backward_workspace_bytes,
                    bad=(((2, 0, 8, 8), b"C 0"), ((2, 513, 8, 8), b"C 513"), ((2, 16, -1, 8), b"-1 x 8")), optional=("residual",))
    assert name == "rf_illumination_estimator_backward"
    geo, px = (2, 8, 12, 4, 8, 8), 4 * 2 * 64
    need = lib.rf_illumination_estimator_backward_workspace_bytes(*geo, 1)
    assert 0 < lib.rf_illumination_estimator_backward_workspace_bytes(*geo, 0) < need
    prm = {"conv1.weight": 4 * 12 * 9, "conv1.bias": 48, "depth_conv.weight": 4 * 12 * 25, "depth_conv.bias": 48, "conv2.weight": 4 * 4 * 12,
           "conv2.bias": 16}
    ptrs = {"img": px * 8, "grad_fea": px * 12, "grad_map": px * 4, "grad_img": px * 8, **{"p." + k: v for k, v in prm.items()},
            **{"g." + k: v for k, v in prm.items()}, "ws": need}
    return dict(ptrs=ptrs, outs=("grad_img", "ws") + tuple("g." + k for k in prm), geo=geo, tail=(0, None), need=need,
                aligned=("img", "grad_fea", "grad_map", "grad_img", "ws"), query=lambda *g: lib.rf_illumination_estimator_backward_workspace_bytes(*g, 1),
                bad=(((2, 6, 12, 4, 8, 8), b"C 6"), ((2, 8, 10, 4, 8, 8), b"Cm 10"), ((2, 8, 12, 3, 8, 8), b"Co 3"), ((2, 516, 12, 4, 8, 8), b"C 516"),
                     ((2, 8, 0, 4, 8, 8), b"Cm 0"), ((2, 8, 12, 4, 8, 0), b"8 x 0")), optional=("grad_map",))


ENTRIES = ("rf_wmb_front_backward", "rf_wmb_back_backward", "rf_dwconv5x5_backward", "rf_illumination_estimator_backward", "rf_layernorm2d_backward")


def invoke(name, e, at, geo=None, ws_bytes=1 << 40):
    """The call on the addresses ``at`` (name -> integer or None); pointer arrays for the illumination operator's parameters."""
    vp = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    args, names = [], list(e["ptrs"])
    if name == "rf_illumination_estimator_backward":
        arr = lambda pre: None if at.get(pre, 0) is None else (C.c_void_p * 6)(*[at[k] for k in names if k.startswith(pre + ".")])  # noqa: E731
        args = [vp(at["img"]), vp(at["grad_fea"]), vp(at["grad_map"]), vp(at["grad_img"]), arr("p"), arr("g"), vp(at["ws"]), ws_bytes]
    else:
        for k in names:
            args.append(vp(at[k]))
            if k == "ws":
                args.append(ws_bytes)
    return getattr(_lib.load(), name)(*args, *(geo or e["geo"]), *e["tail"])


@pytest.mark.parametrize("name", ENTRIES)
def test_host_checks_refuse_before_any_launch(name):
    lib, e = _lib.load(), entry(name)
    err = lib.rf_last_error
    names = list(e["ptrs"])
    good = dict(zip(names, cases.fake_addresses(list(e["ptrs"].values()))))      # never dereferenced: the checks come first
    prefix = name.encode() + b": "

    def refused(at, word=None, code=-22, **kw):
        assert invoke(name, e, at, **kw) == code, (name, word, err())
        assert err().startswith(prefix) and (word is None or word in err()), err()

    # geometry: channel counts outside the range, an odd band width, empty sizes
    for bad, word in e["bad"]:
        refused(good, word, geo=bad)
        if e["query"]:
            assert e["query"](*bad) == -22 and err().startswith(name.encode() + b"_workspace_bytes: ") and word in err(), err()
    # null and misaligned pointers
    for k in names:
        if k in e.get("optional", ()):
            continue
        refused({**good, k: None}, b"null")
    if name == "rf_illumination_estimator_backward":
        refused({**good, "p": None}, b"null")
        refused({**good, "g": None}, b"null")
    for k in e["aligned"]:
        refused({**good, k: good[k] + 4}, b"aligned")
    for k in e.get("optional", ()):                            # the optional input may be absent: the call gets as far as the workspace
        refused({**good, k: None}, b"workspace", code=-12, ws_bytes=16)
    # a workspace that is too small
    if e["need"] is not None:
        assert e["need"] > 0
        refused(good, b"workspace", code=-12, ws_bytes=e["need"] - 1)
    # aliases: everything the call writes against everything it reads and everything else it writes
    ins = [k for k in names if k not in e["outs"]]
    for o in e["outs"]:
        for k in ins:
            refused({**good, o: good[k]}, b"alias")
        for o2 in e["outs"]:
            if o2 != o and e["ptrs"][o2] >= 32:
                refused({**good, o: good[o2] + 16}, b"alias")
    if e["need"] is not None:                                  # inputs may overlap each other
        refused({**good, ins[1]: good[ins[0]]}, b"workspace", code=-12, ws_bytes=e["need"] - 1)


# ------------------------------------------------------------------------------------------ GPU
def run_hip(op, i, device, grads=None):
    """One call of the operator on the case's inputs: ``(outputs by name, the grads object for a second call, the device inputs)``."""
    d = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in i.items()}
    if op == "front":
        gx, pair = ops.wmb_front_backward(d["x"], d["weight2"], d["bias2"], d["grad_t"], d["grad_bands"], grad_scale=G.GRAD_SCALE, grads=grads)
        return {"x": gx, "weight2": pair[0], "bias2": pair[1]}, pair, d
    if op == "back":
        return {"bands": ops.wmb_back_backward(d["bands"], d["grad_out"])}, None, d
    if op == "dw5":
        gx, g = ops.dwconv5x5_backward(d["x"], d["weight"], d["grad_out"], grads=grads)
        return {"x": gx, **g}, g, d
    if op in ("illu", "illu_map"):
        d["p"] = {k: v.to(device) for k, v in i["p"].items()}
        gi, g = ops.illumination_estimator_backward(d["img"], d["p"], d["grad_fea"], d["grad_map"] if op == "illu_map" else None, grads=grads)
        return {"img": gi, **g}, g, d
    gx, g = ops.layernorm2d_backward(d["x"], d["weight"], d["grad_out"], residual=d["residual"] if op == "ln_res" else None, grads=grads)
    return {"x": gx, **g}, g, d


def flat(d):
    return {**{k: v for k, v in d.items() if isinstance(v, torch.Tensor)}, **{"p." + k: v for k, v in d.get("p", {}).items()}}


@pytest.mark.gpu
@pytest.mark.parametrize("op,tag", RUNS, ids=IDS)
def test_hip_matches_float64_autograd(device, op, tag):
    assert_bound_sees_defects(op, tag)
    c = reference(op, tag)
    first = "img" if op.startswith("illu") else "bands" if op == "back" else "x"
    got, grads, d = run_hip(op, c["i"], device)
    again, _, d2 = run_hip(op, c["i"], device)
    torch.cuda.synchronize()
    assert set(got) == set(c["names"])
    assert all(torch.equal(got[k], again[k]) for k in got), f"[{op} {tag}] two calls differ"
    for k, v in flat(d).items():                              # inputs unchanged, the data gradient a new tensor
        src = c["i"]["p"][k[2:]] if k.startswith("p.") else c["i"][k]
        assert torch.equal(v.cpu(), src), f"[{op} {tag}] input {k} was written"
        assert got[first].data_ptr() != v.data_ptr()
    assert got[first].data_ptr() != again[first].data_ptr()
    failed = []
    for k in c["names"]:
        assert tuple(got[k].shape) == tuple(c["ref64"][k].shape), (op, tag, k)
        v = got[k].cpu().double()
        assert bool(torch.isfinite(v).all()), f"[{op} {tag}] {k}: non-finite"
        e64 = float((v - c["ref64"][k]).abs().max())
        if op == "illu" and k in CONV2:
            assert e64 == 0.0 and c["scale"][k] == 0.0, f"[{op} {tag}] {k}: not exact zeros without grad_map"
            continue
        msg = (f"[{op} {tag}] {k:20s} e64 {e64:.3e} e32 {c['e32'][k]:.3e} S {c['scale'][k]:.3e} | bound {c['bound'][k]:.3e} "
               f"({e64 / c['bound'][k]:.3f} of it)")
        print(msg)
        if not e64 <= c["bound"][k]:
            failed.append(msg)
    if grads is not None:                                     # a second call on the returned grads adds: twice the first, within twice the bound
        twice, same, _ = run_hip(op, c["i"], device, grads=grads)
        assert same is grads and torch.equal(twice[first], again[first]), f"[{op} {tag}] the data gradient is overwritten, never accumulated"
        for k in c["names"]:
            if k == first:
                continue
            e = float((twice[k].cpu().double() - 2.0 * c["ref64"][k]).abs().max())
            if not e <= 2.0 * c["bound"][k]:
                failed.append(f"[{op} {tag}] {k}: after a second, accumulating call {e:.3e} from twice the reference, bound {2 * c['bound'][k]:.3e}")
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
def test_conv2_gradients_are_untouched_without_grad_map(device):
    c = reference("illu", "base")
    _, grads, _ = run_hip("illu", c["i"], device)
    for k in CONV2:
        grads[k].fill_(7.0)
    run_hip("illu", c["i"], device, grads=grads)
    assert all(bool((grads[k] == 7.0).all()) for k in CONV2)
