"""The clamped criterion of the reference's loop (train.py:139, ``pred = torch.clamp(pred, 0, 1)`` before the loss) on the HIP
training step: ``Trainer(clamp_pred=True)`` / ``rf_set_loss_clamp``.

Protocol and bounds are those of tests/test_train_shapes.py, imported from there unchanged (TOL_REL 5e-5, RATIO 8, FLOOR 1e-5,
norm 1e-3, KINK_MARGIN 5e-6): float64 autograd on the oracle is the truth, float32 autograd on the same inputs the yardstick,
here with ``torch.clamp(pred, 0, 1)`` in front of the loss.  Cases (same seeds as there):

==============================  ===========================================================================================
d16_flca_l1_masked_b1           mosaic 48 x 64, L1.  On the CPU oracle 44.3 % of the prediction lies outside [0, 1] (38.2 %
                                below, 6.1 % above); the nearest element to a clamp edge is 3.3e-5 away
d24_plain_charb_b3_24x32        Charbonnier, B = 3: 62.8 % outside (62.2 % below, 0.6 % above), nearest edge 9.3e-6
d24_plain_charb_b3_24x32_io     the same configuration built with ``clamp_io=True``: the input clamp (model.py:475) and the
                                output clamp (:508) under the criterion's, against the oracle with both clamps; the returned
                                prediction is the clamped one.  Seed 404, not the base case's 402: with the stretched mosaic
                                seed 402 puts a LeakyReLU input 1.2e-6 from its kink in the float64 forward, under
                                KINK_MARGIN; with 404 the nearest kink is 7.8e-6 away and the nearest clamp edge 1.6e-5
                                (55.0 % of the prediction below 0, 5.4 % above 1, 2.3 % of the mosaic outside [0, 1])
==============================  ===========================================================================================

Well-posedness, asserted before anything is compared: the clamped share lies in [5 %, 95 %] (a clamp that never bites would
test nothing); every prediction element is at least KINK_MARGIN from 0 and from 1 in the float64 forward (the clamp's kinks:
closer than the float32 forward's own error the HIP step may mask the other way, a different valid subgradient), and for L1
``clamp(pred) - gt`` is that far from 0.

``test_flag_off_differs`` is the negative: without the flag the gradients of case 1 are NOT the clamped truth, by more than
the bound.  The last test (host only) checks that a ``clamp_io`` model is still refused while the flag is off.
"""
import ctypes as C

import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
from bayer_low_light_image_enhancement_amd import synth
from oracle import rawformer_ref as R
from test_train_shapes import CASES, FLOOR, KINK_MARGIN, RATIO, TOL_REL, _KinkDistance

_BY_ID = {c[0]: c for c in CASES}
# id, base case, clamp_io, seed (None: the base case's)
CLAMP_CASES = [
    ("d16_flca_l1_masked_b1", "d16_flca_l1_masked_b1", False, None),
    ("d24_plain_charb_b3_24x32", "d24_plain_charb_b3_24x32", False, None),
    ("d24_plain_charb_b3_24x32_io", "d24_plain_charb_b3_24x32", True, 404),
]


def _inputs(base, clamp_io, seed=None):
    tag, variant, loss, lrelu, dim, heads, hx, b, hm, wm, base_seed = _BY_ID[base]
    seed = base_seed if seed is None else seed
    cfg = R.RawFormerConfig(dim=dim, heads=heads, variant=variant, branch_lrelu=lrelu, clamp_io=clamp_io)
    shapes = R.param_shapes(cfg, ffn_expansion_factor=hx)
    sd = {k: torch.from_numpy(synth.param_values(seed, k, s)).reshape(s) for k, s in shapes.items()}
    x = torch.from_numpy(synth.bayer_mosaic(seed, b, hm, wm))
    if clamp_io:
        x = x * 2.5 - 0.125        # -0.125 .. 1.145, 2 % of the mosaic outside [0, 1]: the input clamp has something to do
    gt = torch.from_numpy(synth.smooth_rgb(seed, b, hm, wm))
    return cfg, sd, x, gt, loss


def _raw_prediction(sd, x, cfg):
    """float64 prediction in front of every output clamp."""
    import dataclasses
    with torch.no_grad():
        p = {k: v.double() for k, v in sd.items()}
        xin = x.double().clamp(0.0, 1.0) if cfg.clamp_io else x.double()
        return R.rawformer_forward(p, xin, dataclasses.replace(cfg, clamp_io=False))


def _autograd_clamped(sd, x, gt, cfg, loss, dtype):
    """Loss, gradients and prediction (the model's output: clamped for a clamp_io model) with the clamped criterion; the
    distance of the nearest LeakyReLU / ReLU input from its kink."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    kinks = _KinkDistance()
    with kinks:
        pred = R.rawformer_forward(p, x.to(dtype), cfg)
    d = torch.clamp(pred, 0, 1) - gt.to(dtype)
    val = d.abs().mean() if loss == "l1" else torch.sqrt(d * d + 1e-3 ** 2).mean()
    val.backward()
    return float(val.detach()), {k: v.grad for k, v in p.items()}, pred.detach(), kinks.min


def clamp_statistics(sd, x, gt, cfg, loss):
    """Share of the prediction below 0 / above 1 and the smallest distance from a kink of the clamped criterion."""
    raw = _raw_prediction(sd, x, cfg)
    below, above = float((raw < 0).double().mean()), float((raw > 1).double().mean())
    edge = float(torch.minimum(raw.abs(), (raw - 1).abs()).min())
    if loss == "l1":
        edge = min(edge, float((raw.clamp(0, 1) - gt.double()).abs().min()))
    return below, above, edge


def _trainer(device, base, clamp_io, clamp_pred, sd):
    from bayer_low_light_image_enhancement_amd import RawFormer
    from bayer_low_light_image_enhancement_amd.train import Trainer
    tag, variant, loss, lrelu, dim, heads, hx, b, hm, wm, seed = _BY_ID[base]
    m = RawFormer(dim=dim, num_heads=heads, ffn_expansion_factor=hx, variant=variant, branch_lrelu=lrelu, clamp_io=clamp_io)
    m.load_state_dict({**m.state_dict(), **sd}, strict=True)
    return Trainer(m.to(device).train(), loss=loss, clamp_pred=clamp_pred)


_TRUTH = {}


def _truth(case):
    """float64 / float32 autograd of a case, computed once and shared by the tests."""
    if case not in _TRUTH:
        tag, base, clamp_io, seed = case
        cfg, sd, x, gt, loss = _inputs(base, clamp_io, seed)
        below, above, edge = clamp_statistics(sd, x, gt, cfg, loss)
        loss64, g64, pred64, kink = _autograd_clamped(sd, x, gt, cfg, loss, torch.float64)
        _, g32, _, _ = _autograd_clamped(sd, x, gt, cfg, loss, torch.float32)
        _TRUTH[case] = (cfg, sd, x, gt, loss, below, above, min(edge, kink), loss64, g64, pred64, g32)
    return _TRUTH[case]


def _rows(tr, g64, g32):
    rows = []            # (name, e64, e32, bound, norm error / norm bound, ratio, max|g|)
    for k, t in g64.items():
        got = tr.grad_of(k).cpu().double()
        gmax, gnorm = float(t.abs().max()), float(t.norm())
        e64 = float((got - t).abs().max())
        e32 = float((g32[k].double() - t).abs().max())
        bound = TOL_REL * gmax + 1e-6
        nrm = abs(float(got.norm()) - gnorm) / (1e-3 * gnorm + 1e-12)
        ratio = e64 / max(e32, 1e-9 * gmax, 1e-30)
        rows.append((k, e64, e32, bound, nrm, ratio, gmax))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", CLAMP_CASES, ids=[c[0] for c in CLAMP_CASES])
def test_clamped_gradients_match_float64_autograd(device, case):
    tag, base, clamp_io, seed = case
    cfg, sd, x, gt, loss, below, above, kink, loss64, g64, pred64, g32 = _truth(case)
    print(f"[{tag}] outside [0,1]: {100 * (below + above):.1f} % ({100 * below:.1f} % below, {100 * above:.1f} % above), nearest kink {kink:.1e}")
    assert 0.05 <= below + above <= 0.95, f"[{tag}] the clamp bites on {100 * (below + above):.1f} % of the prediction: the case tests nothing"
    assert kink >= KINK_MARGIN, f"[{tag}] an element lies {kink:.1e} from a kink: the comparison is not well posed, pick another seed"
    tr = _trainer(device, base, clamp_io, True, sd)
    loss_dev, pred = tr.forward_backward(x.to(device), gt.to(device), want_pred=True)
    pred_err = float((pred.cpu().double() - pred64).abs().max())
    loss_err = abs(float(loss_dev) - loss64)
    rows = _rows(tr, g64, g32)
    worst_tol = max(rows, key=lambda r: r[1] / r[3])
    worst_ratio = max(rows, key=lambda r: r[5])
    msg = (f"[{tag}] pred {pred_err:.2e} loss {loss_err:.2e} | worst e64/bound: {worst_tol[0]} e64 {worst_tol[1]:.3e} "
           f"({worst_tol[1] / max(worst_tol[6], 1e-30):.2e} max|g|, {worst_tol[1] / worst_tol[3]:.3f} of the bound, e64/e32 {worst_tol[5]:.2f}) | "
           f"worst e64/e32: {worst_ratio[0]} {worst_ratio[5]:.2f} (e64 {worst_ratio[1]:.3e}, e32 {worst_ratio[2]:.3e}, "
           f"max|g| {worst_ratio[6]:.3e}) | worst norm {max(r[4] for r in rows):.3f} of the bound")
    print(msg)
    assert pred_err <= 5e-5, msg
    assert loss_err <= 1e-5, msg
    for k, e64, e32, bound, nrm, ratio, gmax in rows:
        assert e64 <= bound, (k, e64, bound, msg)
        assert nrm <= 1.0, (k, nrm, msg)
        assert e64 <= RATIO * e32 + FLOOR * gmax, (k, e64, e32, gmax, msg)


@pytest.mark.gpu
def test_flag_off_differs(device):
    """The switch is live: with ``clamp_pred=False`` the step computes the unclamped criterion, whose gradients miss the clamped
    truth of case 1 by more than the bound the clamped step meets (44 % of the seed gradient is masked there)."""
    case = CLAMP_CASES[0]
    cfg, sd, x, gt, loss, below, above, kink, loss64, g64, pred64, g32 = _truth(case)
    tr = _trainer(device, case[1], False, False, sd)
    loss_dev = tr.forward_backward(x.to(device), gt.to(device))
    rows = _rows(tr, g64, g32)
    over = [r for r in rows if r[1] > r[3]]
    worst = max(rows, key=lambda r: r[1] / r[3])
    print(f"flag off: {len(over)} of {len(rows)} tensors over the bound, worst {worst[0]} at {worst[1] / worst[3]:.1f} x the bound; "
          f"loss {float(loss_dev):.6f} against the clamped {loss64:.6f}")
    assert over, "the unclamped step meets the clamped truth: rf_set_loss_clamp changes nothing"
    assert abs(float(loss_dev) - loss64) > 1e-5


def test_clamp_io_without_the_flag_is_still_refused():
    """``clamp_io`` models have no adjoint of their own: refused as before unless the criterion is clamped, and the FLCA
    variant either way (host logic only: the check comes before any buffer is touched)."""
    from bayer_low_light_image_enhancement_amd import RawFormer, _lib
    lib = _lib.load()
    refusal = b"rf_train_step: variants 'plain' and 'flca' without clamp_io have their adjoint so far"
    fake = C.c_void_p(1 << 12)                  # 16-byte aligned, never dereferenced
    for variant, on, refused in (("plain", 0, True), ("flca", 0, True), ("flca", 1, True), ("plain", 1, False)):
        cfg = RawFormer(dim=16, variant=variant, clamp_io=True)._config()
        h = C.c_void_p()
        _lib.check(lib.rf_create(C.byref(cfg), C.byref(h)), "rf_create")
        try:
            assert lib.rf_set_loss_clamp(h, on) == 0
            rc = lib.rf_train_step(h, fake, fake, fake, fake, None, fake, 1 << 30, 1, 16, 48, 0, 1e-3, None)
            assert rc < 0
            if refused:
                assert lib.rf_last_error() == refusal
            else:                                   # past the refusal: the next check (the shape rule) answers
                assert lib.rf_last_error() == b"rf_train_step: packed width 48 is not a multiple of 32"
        finally:
            lib.rf_destroy(h)
    assert lib.rf_set_loss_clamp(None, 1) < 0 and lib.rf_last_error() == b"rf_set_loss_clamp: null handle"
