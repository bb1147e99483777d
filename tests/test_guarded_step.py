"""GPU: the guarded optimiser step -- segmented gradient statistics, the control block, the guarded Adam kernel
(csrc/rf_optim.hip) and their use by ``train.Trainer`` / ``train.fit``.

Tolerances, none of them taken from what the kernels give:

* norms against numpy float64: both sides square exactly and add in float64, in different orders.  N additions differ by at
  most N 2^-53 relative; N is about 4.2e6 here (5e-10), rounded up to 1e-9.
* updates: ``e = max |p - p64|`` against a float64 Adam on the CPU, for the guarded path AND for ``rf_adam_step`` (the plain
  step, the yardstick) on the same inputs; ``e_guarded <= e_plain + 2^-23 max|p|``.  The guarded kernel repeats the plain one's
  arithmetic; what may differ is the rounding of the two bias corrections (float64 then rounded, against float32 ``powf``) and,
  when clipping, of the one gradient factor: relative changes of a few 2^-24 in an update of size ``lr``, far inside one unit
  in the last place of the largest parameter.
* ``clip_coef``: computed in float64 from a norm that is good to 1e-9; 2^-23 relative.
* everything about skipping and resuming is bitwise.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib, synth

CHUNK, STATS_GRID = 4096, 1024            # csrc/rf_optim.hip: floats per chunk, workgroups of one statistics pass
ULP = 2.0 ** -23
B1, B2, EPS = 0.9, 0.999, 1e-8


def layout(counts):
    """16-byte aligned offsets of consecutive segments; the buffer ends with the last segment."""
    offsets, off = [], 0
    for c in counts:
        offsets.append(off)
        off = (off + c + 3) // 4 * 4
    return offsets, offsets[-1] + counts[-1]


class Guard:
    """The device state of the handle-free entry points over one flat buffer."""

    def __init__(self, counts, device):
        self.counts = list(counts)
        self.offsets, self.n = layout(self.counts)
        self.nseg = len(self.counts)
        self.state = torch.zeros(_lib.size("rf_optim_state_bytes", self.nseg, self.n), dtype=torch.uint8, device=device)
        arr = _lib.C.c_size_t * self.nseg
        _lib.launch("rf_optim_init", self.state, arr(*self.offsets), arr(*self.counts), self.nseg, self.n, self.state, self.state.numel())

    def stats(self, g):
        _lib.launch("rf_grad_stats", g, g, self.n, self.nseg, self.state, self.state.numel())

    def step(self, p, g, m, v, lr=1e-3, wd=0.0, decoupled=False, grad_scale=1.0, max_norm=math.inf, skip=True):
        self.stats(g)
        _lib.launch("rf_adam_step_guarded", p, p, g, m, v, self.n, lr, B1, B2, EPS, wd, int(decoupled), grad_scale, max_norm, int(skip), self.nseg,
                    self.state, self.state.numel())

    def set_steps(self, k):
        _lib.launch("rf_optim_set_steps", self.state, self.state, self.state.numel(), k)

    def control(self):
        return np.frombuffer(self.state[:80].cpu().numpy().tobytes(), dtype=np.dtype(_lib.OPTIM_CONTROL))[0]

    def segments(self):
        return np.frombuffer(self.state[80: 80 + 16 * self.nseg].cpu().numpy().tobytes(), dtype=np.dtype(_lib.OPTIM_SEGMENT))

    def mask(self):
        """True where a float of the buffer belongs to a segment."""
        k = np.zeros(self.n, dtype=bool)
        for o, c in zip(self.offsets, self.counts):
            k[o: o + c] = True
        return k


def plain_step(p, g, m, v, step, lr, wd, decoupled, grad_scale=1.0):
    _lib.launch("rf_adam_step", p, p, g, m, v, p.numel(), lr, B1, B2, EPS, wd, int(decoupled), step, grad_scale)


def adam64(p, m, v, grads, lr, wd, decoupled, coefs):
    """adam_kernel in float64 (betas and eps as the float32 values the kernels are given); gradient k is multiplied by coefs[k]."""
    b1, b2, eps = float(np.float32(B1)), float(np.float32(B2)), float(np.float32(EPS))
    lr, wd = float(np.float32(lr)), float(np.float32(wd))
    p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for k, (g, coef) in enumerate(zip(grads, coefs), 1):
        g = g.astype(np.float64) * coef
        if wd:
            if decoupled:
                p = p * (1.0 - lr * wd)
            else:
                g = g + wd * p
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - lr / (1.0 - b1 ** k) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** k) + eps)
    return p


def clip_coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. statistics
# ---------------------------------------------------------------------------------------------------------------------------
BIG = STATS_GRID * CHUNK + 2 * CHUNK + 5          # more chunks than one pass of the grid: the grid-stride loop runs twice
STAT_COUNTS = [1, 3, 4, 255, 256, 257, 4095, BIG, 4096, 4097]
HUGE_SEG = 8                                      # the segment that gets the 1e25 element


@pytest.fixture(scope="module")
def stat_case():
    """(flat float32 buffer with 1e30 in the gaps, per-segment float64 sums of squares)"""
    offsets, n = layout(STAT_COUNTS)
    rng = np.random.default_rng(20240607)
    g = np.full(n, 1e30, dtype=np.float32)
    scales = np.logspace(-8, 3, len(STAT_COUNTS))
    for i, (o, c) in enumerate(zip(offsets, STAT_COUNTS)):
        g[o: o + c] = (rng.standard_normal(c) * scales[i]).astype(np.float32)
    g[offsets[HUGE_SEG] + 1234] = 1e25            # its square overflows float32, not float64
    sumsq = np.array([np.sum(g[o: o + c].astype(np.float64) ** 2) for o, c in zip(offsets, STAT_COUNTS)])
    return g, sumsq


@pytest.mark.gpu
def test_segment_statistics_match_float64_and_never_read_a_gap(device, stat_case):
    g_host, want = stat_case
    guard = Guard(STAT_COUNTS, device)
    assert guard.n == g_host.size and (np.diff(guard.offsets) - np.array(STAT_COUNTS[:-1])).max() == 3        # gaps of up to 3 floats
    g = dev(g_host, device)
    guard.stats(g)
    seg, ctl = guard.segments(), guard.control()
    assert ctl["nseg"] == len(STAT_COUNTS) and ctl["nchunks"] == sum((c + CHUNK - 1) // CHUNK for c in STAT_COUNTS) > STATS_GRID
    worst = 0.0
    for i in range(guard.nseg):
        rel = abs(math.sqrt(seg[i]["sumsq"]) - math.sqrt(want[i])) / math.sqrt(want[i])
        print(f"segment {i}: {STAT_COUNTS[i]} floats, norm {math.sqrt(seg[i]['sumsq']):.17g}, float64 {math.sqrt(want[i]):.17g}, rel {rel:.3g}")
        worst = max(worst, rel)
    total, total_want = math.sqrt(ctl["grad_sumsq"]), math.sqrt(float(np.sum(want)))
    print(f"total norm {total:.17g}, float64 {total_want:.17g}, rel {abs(total - total_want) / total_want:.3g}")
    assert worst <= 1e-9 and abs(total - total_want) <= 1e-9 * total_want
    assert want[HUGE_SEG] > float(np.finfo(np.float32).max) and math.isfinite(seg[HUGE_SEG]["sumsq"])
    assert [int(s["nonfinite"]) for s in seg] == [0] * guard.nseg and ctl["nonfinite"] == 0
    # two runs: the same bits everywhere, partials included
    first = guard.state.clone()
    guard.stats(g)
    assert torch.equal(first, guard.state)


@pytest.mark.gpu
def test_nonfinite_counts_are_exact_per_segment(device, stat_case):
    g_host = stat_case[0].copy()
    guard = Guard(STAT_COUNTS, device)
    off = guard.offsets
    g_host[off[3] + 254] = np.nan                 # last element of the 255-float segment
    g_host[off[5] + 256] = np.inf                 # last element of the 257-float segment: the scalar tail
    g_host[off[7] + STATS_GRID * CHUNK + 17] = -np.inf        # a chunk of the second grid-stride pass
    g_host[off[7] + BIG - 1] = np.nan             # the big segment's short last chunk
    g_host[0] = np.nan                            # first element of the buffer (segment 0, one float)
    g_host[-1] = -np.inf                          # last element of the buffer
    want = [1, 0, 0, 1, 0, 1, 0, 2, 0, 1]
    guard.stats(dev(g_host, device))
    seg, ctl = guard.segments(), guard.control()
    assert [int(s["nonfinite"]) for s in seg] == want
    assert ctl["nonfinite"] == sum(want)
    for i, k in enumerate(want):                  # a clean segment keeps its finite sum
        assert math.isfinite(seg[i]["sumsq"]) == (k == 0), i


# ---------------------------------------------------------------------------------------------------------------------------
# 2.-4. skip, no trace, clip and parity: no model
# ---------------------------------------------------------------------------------------------------------------------------
SMALL_COUNTS = [4097, 37, 1, 300, 5000]


def small_case(device, seed, ngrads):
    guard = Guard(SMALL_COUNTS, device)
    rng = np.random.default_rng(seed)
    inside = guard.mask()
    p = (rng.standard_normal(guard.n) * 0.1).astype(np.float32)
    m = (rng.standard_normal(guard.n) * 1e-3).astype(np.float32)
    v = (rng.standard_normal(guard.n) ** 2 * 1e-5).astype(np.float32)
    grads = [np.where(inside, rng.standard_normal(guard.n) * 1e-2, 0.0).astype(np.float32) for _ in range(ngrads)]      # gaps hold zeros, as in a Trainer
    return guard, p, m, v, grads


@pytest.mark.gpu
def test_nonfinite_gradient_skips_the_whole_step(device):
    guard, p0, m0, v0, (g0,) = small_case(device, 5, 1)
    g0[guard.offsets[3] + 7] = np.nan
    p, m, v, g = (dev(a, device) for a in (p0, m0, v0, g0))
    guard.set_steps(3)
    guard.step(p, g, m, v, wd=1e-2, decoupled=True, skip=True)
    ctl = guard.control()
    assert torch.equal(p.cpu(), torch.from_numpy(p0)) and torch.equal(m.cpu(), torch.from_numpy(m0)) and torch.equal(v.cpu(), torch.from_numpy(v0))
    assert (ctl["skip"], ctl["steps_skipped"], ctl["steps_applied"], ctl["nonfinite"]) == (1, 1, 3, 1)
    assert np.array_equal(g.cpu().numpy(), g0, equal_nan=True)         # the gradient buffer is only read
    # skip_nonfinite = 0: the documented behaviour is that the step IS applied and the weights go non-finite
    guard.step(p, g, m, v, wd=1e-2, decoupled=True, skip=False)
    ctl = guard.control()
    assert (ctl["skip"], ctl["steps_skipped"], ctl["steps_applied"]) == (0, 1, 4)
    assert not bool(torch.isfinite(p).all()) and not bool(torch.isfinite(m).all())
    k = guard.offsets[3] + 7
    assert bool(torch.isfinite(p[:k]).all()) and bool(torch.isfinite(p[k + 1:]).all())         # element-wise: only that weight


@pytest.mark.gpu
def test_a_skipped_step_leaves_no_trace(device):
    guard_a, p0, m0, v0, (g1, g2) = small_case(device, 6, 2)
    guard_b = Guard(SMALL_COUNTS, device)
    bad = g1.copy()
    bad[guard_a.offsets[0]] = np.inf
    bad[guard_a.n - 1] = np.nan
    a = [dev(x, device) for x in (p0, m0, v0)]
    b = [dev(x, device) for x in (p0, m0, v0)]
    for g in (g1, bad, g2):
        guard_a.step(*a[:1], dev(g, device), *a[1:], wd=1e-2, decoupled=True)
    for g in (g1, g2):
        guard_b.step(*b[:1], dev(g, device), *b[1:], wd=1e-2, decoupled=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ca, cb = guard_a.control(), guard_b.control()
    assert (ca["steps_applied"], ca["steps_skipped"]) == (2, 1) and (cb["steps_applied"], cb["steps_skipped"]) == (2, 0)
    assert ca["bias_corr1"] == cb["bias_corr1"] and ca["bias_corr2"] == cb["bias_corr2"]
    assert not torch.equal(a[0].cpu(), torch.from_numpy(p0))


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (1e-2, True)], ids=["adam", "adamw"])
def test_clipped_update_matches_float64_as_well_as_the_plain_step(device, factor, wd, decoupled):
    lr = 1e-3
    guard, p0, m0, v0, grads = small_case(device, 7, 3)
    norms = [math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) for g in grads]
    max_norm = float(np.float32(factor * norms[0]))                 # the float32 the entry point receives
    coefs = [clip_coef64(nm, max_norm) for nm in norms]
    assert all(c < 1.0 for c in coefs) if factor < 1 else all(c == 1.0 for c in coefs)
    p64 = adam64(p0, m0, v0, grads, lr, wd, decoupled, coefs)
    # guarded path
    p, m, v = (dev(a, device) for a in (p0, m0, v0))
    for k, g in enumerate(grads):
        guard.step(p, dev(g, device), m, v, lr=lr, wd=wd, decoupled=decoupled, max_norm=max_norm)
        ctl = guard.control()
        assert abs(ctl["grad_norm"] - norms[k]) <= 1e-9 * norms[k]
        assert abs(ctl["clip_coef"] - coefs[k]) <= ULP * coefs[k], (ctl["clip_coef"], coefs[k])
        assert ctl["steps_applied"] == k + 1 and ctl["skip"] == 0
    e_guarded = float(np.abs(p.cpu().numpy().astype(np.float64) - p64).max())
    # yardstick: rf_adam_step on the same inputs, the gradients scaled beforehand by the float64 coefficient
    q, m, v = (dev(a, device) for a in (p0, m0, v0))
    for k, g in enumerate(grads):
        plain_step(q, dev((g.astype(np.float64) * coefs[k]).astype(np.float32), device), m, v, k + 1, lr, wd, decoupled)
    e_plain = float(np.abs(q.cpu().numpy().astype(np.float64) - p64).max())
    bound = e_plain + ULP * float(np.abs(p64).max())
    print(f"factor {factor} wd {wd}: e_guarded {e_guarded:.3e}, e_plain {e_plain:.3e}, bound {bound:.3e}")
    assert e_guarded <= bound
    assert float(np.abs(p64 - p0).max()) > 100 * bound          # the three steps moved the weights far more than the bound


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Trainer
# ---------------------------------------------------------------------------------------------------------------------------
DIM, SEED, HM, WM = 16, 77, 32, 64


def make_model(device, variant):
    from bayer_low_light_image_enhancement_amd import RawFormer
    m = RawFormer(dim=DIM, variant=variant, branch_lrelu=True)
    m.load_state_dict({**m.state_dict(), **cases.model_state(DIM, SEED, variant)}, strict=True)
    return m.to(device).train()


def make_trainer(device, variant, **kw):
    from bayer_low_light_image_enhancement_amd.train import Trainer
    return Trainer(make_model(device, variant), lr=1e-3, **kw)


def batch(device, seed=SEED):
    return torch.from_numpy(synth.bayer_mosaic(seed, 1, HM, WM)).to(device), torch.from_numpy(synth.smooth_rgb(seed, 1, HM, WM)).to(device)


def same_state(a, b):
    return torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "flca"])
def test_trainer_skips_a_poisoned_step_and_names_the_tensor(device, variant):
    x, gt = batch(device)
    kw = dict(skip_nonfinite=True, weight_decay=1e-2, decoupled=True)
    tr = make_trainer(device, variant, **kw)
    names = [k for k, _ in tr.model.named_parameters()]
    victim = names[len(names) // 2]
    tr.forward_backward(x, gt)
    tr.grad_of(victim).view(-1)[-1] = float("nan")
    before = (tr.flat.clone(), tr.m.clone(), tr.v.clone())
    tr.optimizer_step()
    assert torch.equal(tr.flat, before[0]) and torch.equal(tr.m, before[1]) and torch.equal(tr.v, before[2])
    norms = tr.grad_norms()
    assert sorted(norms) == sorted(names)
    assert [k for k, (_, bad) in norms.items() if bad] == [victim] and norms[victim][1] == 1
    assert all(math.isfinite(nm) and nm >= 0 for k, (nm, _) in norms.items() if k != victim)
    stats = tr.optimizer_stats()
    assert sorted(stats) == ["clip_coef", "grad_norm", "nonfinite", "steps_applied", "steps_skipped"]
    assert (stats["steps_skipped"], stats["steps_applied"], stats["nonfinite"], stats["clip_coef"]) == (1, 0, 1, 1.0)
    assert tr.step_no == 0
    # then a clean step: as if the poisoned one had never been
    tr.step(x, gt)
    twin = make_trainer(device, variant, **kw)
    twin.step(x, gt)
    assert same_state(tr, twin) and not torch.equal(tr.flat, before[0])
    assert tr.step_no == twin.step_no == 1 and tr.optimizer_stats()["steps_skipped"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "flca"])
def test_trainer_clips_to_max_grad_norm(device, variant):
    x, gt = batch(device)
    lr, wd = 1e-3, 1e-2
    tr = make_trainer(device, variant, max_grad_norm=1.0, weight_decay=wd, decoupled=True)
    tr.forward_backward(x, gt)
    g = tr.grads.cpu().numpy()
    norm = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))          # the gaps of the flat buffer hold zeros
    tr.max_grad_norm = float(np.float32(0.5 * norm))
    coef = clip_coef64(norm, tr.max_grad_norm)
    p0, m0, v0 = tr.flat.cpu().numpy(), tr.m.cpu().numpy(), tr.v.cpu().numpy()
    tr.optimizer_step()
    stats = tr.optimizer_stats()
    assert abs(stats["grad_norm"] - norm) <= 1e-9 * norm
    assert abs(stats["clip_coef"] - coef) <= ULP * coef and 0.49 < coef < 0.51
    assert np.array_equal(tr.grads.cpu().numpy(), g)                    # grad_of() keeps the unclipped gradient
    per_tensor = tr.grad_norms()
    assert abs(math.sqrt(sum(nm * nm for nm, _ in per_tensor.values())) - norm) <= 1e-9 * norm
    p64 = adam64(p0, m0, v0, [g], lr, wd, True, [coef])
    e_guarded = float(np.abs(tr.flat.cpu().numpy().astype(np.float64) - p64).max())
    q, m, v = (dev(a, device) for a in (p0, m0, v0))
    plain_step(q, dev((g.astype(np.float64) * coef).astype(np.float32), device), m, v, 1, lr, wd, True)
    e_plain = float(np.abs(q.cpu().numpy().astype(np.float64) - p64).max())
    bound = e_plain + ULP * float(np.abs(p64).max())
    print(f"{variant}: e_guarded {e_guarded:.3e}, e_plain {e_plain:.3e}, bound {bound:.3e}")
    assert e_guarded <= bound


@pytest.mark.gpu
def test_checkpoint_after_a_skip_resumes_with_the_right_step(device):
    x, gt = batch(device)
    x2, gt2 = batch(device, SEED + 1)
    kw = dict(skip_nonfinite=True, max_grad_norm=0.05)
    tr = make_trainer(device, "flca", **kw)
    tr.step(x, gt)
    tr.forward_backward(x2, gt2)
    tr.grads[0] = float("inf")
    tr.optimizer_step()                                # skipped
    tr.step(x2, gt2)
    assert tr.step_no == 2 and tr.optimizer_stats()["steps_skipped"] == 1
    sd = tr.optimizer_state_dict()
    assert {int(st["step"]) for st in sd["state"].values()} == {2}
    fresh = make_trainer(device, "flca", **kw)
    fresh.model.load_state_dict(tr.model.state_dict(), strict=True)
    fresh.load_optimizer_state_dict(sd)
    assert fresh.step_no == 2 and fresh.optimizer_stats()["steps_skipped"] == 0 and same_state(fresh, tr)
    tr.step(x, gt)
    fresh.step(x, gt)
    assert same_state(fresh, tr) and fresh.step_no == 3


@pytest.mark.gpu
def test_default_trainer_still_runs_the_plain_step(device):
    x, gt = batch(device)
    tr = make_trainer(device, "flca", weight_decay=1e-2, decoupled=True)
    assert not tr.guarded and not hasattr(tr, "opt_state")
    for k in (1, 2):
        tr.forward_backward(x, gt)
        p, m, v = tr.flat.clone(), tr.m.clone(), tr.v.clone()
        plain_step(p, tr.grads, m, v, k, 1e-3, 1e-2, True)
        tr.optimizer_step()
        assert torch.equal(tr.flat, p) and torch.equal(tr.m, m) and torch.equal(tr.v, v)
        assert tr.step_no == k and type(tr.step_no) is int
    with pytest.raises(RuntimeError, match="plain optimiser step"):
        tr.optimizer_stats()
    with pytest.raises(RuntimeError, match="plain optimiser step"):
        tr.grad_norms()


FIT_N, FIT_H, FIT_W, FIT_PATCH, FIT_EPOCHS = 2, 64, 128, (32, 64), 2
BASE_KEYS = ["best_epoch", "best_psnr", "epoch", "loss", "lr", "psnr"]
LOG_LINE_OF_TEST_FIT = re.compile(r"^Epoch (\d+)/2 \| Time: \d+\.\d\ds \| Loss: (\d+\.\d{4}) \| Avg PSNR: (\d+\.\d{4}) \| Best PSNR: (\d+\.\d{4}) \(Epoch (\d+)\)$")


def run_fit(device, out_dir, poison_step=None, **kw):
    from bayer_low_light_image_enhancement_amd import PatchSampler, RawFormer, ResidentSID
    from bayer_low_light_image_enhancement_amd.train import Trainer, fit
    amp = [100.0, 300.0]
    mosaic = synth.bayer_mosaic(41, FIT_N, FIT_H, FIT_W)[:, 0]
    raw = np.stack([512.0 + mosaic[k] * 15871.0 / amp[k] for k in range(FIT_N)]).round().astype(np.uint16)
    gt = np.ascontiguousarray((synth.smooth_rgb(41, FIT_N, FIT_H, FIT_W).transpose(0, 2, 3, 1) * 65535.0).round().astype(np.uint16))
    resident = ResidentSID(raw, gt, amp, device=device)
    model = RawFormer(dim=DIM)
    synth.fill_state_dict(model.state_dict(), 41)
    tr = Trainer(model.to(device).train(), lr=1e-3, loss="charbonnier", clamp_pred=True, **kw)
    calls = [0]

    def step(x, gt, loss_out=None):                    # Trainer.step with one gradient poisoned on the way
        loss = tr.forward_backward(x, gt, loss_out=loss_out)
        if calls[0] == poison_step:
            tr.grad_of("embedding.weight").view(-1)[3] = float("nan")
        calls[0] += 1
        tr.optimizer_step()
        return loss

    tr.step = step
    history = fit(tr, PatchSampler(resident, FIT_PATCH, seed=5), PatchSampler(resident, FIT_PATCH), FIT_EPOCHS, FIT_N, out_dir, shuffle_seed=9)
    return tr, history, open(os.path.join(out_dir, "train_log.txt")).read().splitlines()


@pytest.mark.gpu
def test_fit_reports_skipped_steps_and_the_gradient_norm(device, tmp_path):
    tr, history, lines = run_fit(device, str(tmp_path / "guarded"), poison_step=1, skip_nonfinite=True, max_grad_norm=10.0)
    assert [h["epoch"] for h in history] == [0, 1, 2] and len(lines) == 3          # epochs 0 .. 2 inclusive, one step each
    for h in history:
        assert sorted(h) == sorted(BASE_KEYS + ["skipped", "grad_norm"])
    assert [h["skipped"] for h in history] == [0, 1, 0]
    assert math.isnan(history[1]["grad_norm"]) and all(math.isfinite(history[e]["grad_norm"]) and history[e]["grad_norm"] > 0 for e in (0, 2))
    assert all(LOG_LINE_OF_TEST_FIT.match(lines[e]) for e in (0, 1, 2)), lines
    assert tr.step_no == 2 and bool(torch.isfinite(tr.flat).all())
    stats = tr.optimizer_stats()
    assert (stats["steps_applied"], stats["steps_skipped"]) == (2, 1)


@pytest.mark.gpu
def test_fit_history_of_a_default_trainer_has_todays_keys(device, tmp_path):
    tr, history, lines = run_fit(device, str(tmp_path / "default"))
    assert [sorted(h) for h in history] == [BASE_KEYS] * 3
    assert all(LOG_LINE_OF_TEST_FIT.match(line) for line in lines), lines
    assert tr.step_no == 3


# ---------------------------------------------------------------------------------------------------------------------------
# 6. behind the overlapped all-reduce
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guarded_step_behind_the_overlapped_reducer_on_rccl_with_one_rank(device, tmp_path):
    """One-rank RCCL, the pattern of tests/test_train.py: with ``overlap_allreduce='always'`` every bucket goes through RCCL from
    inside rf_train_step; the statistics, the control step and the guarded Adam are enqueued behind ``reducer.finish()``.  They
    must leave the bits of the serial path: weights, moments, and the control block."""
    import subprocess
    import sys
    code = r'''
import sys, os, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cases
from bayer_low_light_image_enhancement_amd import RawFormer, synth
from bayer_low_light_image_enhancement_amd.train import Trainer
dist.init_process_group("nccl", init_method="file://" + sys.argv[2], rank=0, world_size=1)
dev = torch.device("cuda:0")
dim, seed, b, hm, wm = 16, 61, 2, 64, 128
x = torch.from_numpy(synth.bayer_mosaic(seed, b, hm, wm)).to(dev)
gt = torch.from_numpy(synth.smooth_rgb(seed, b, hm, wm)).to(dev)
res = {}
for tag, ov in (("serial", False), ("overlapped", "always")):
    m = RawFormer(dim=dim)
    m.load_state_dict({**m.state_dict(), **cases.model_state(dim, seed, "flca")}, strict=True)
    m = m.to(dev).train()
    tr = Trainer(m, lr=1e-3, weight_decay=1e-2, decoupled=True, overlap_allreduce=ov, bucket_floats=1 << 14, max_grad_norm=1e-3, skip_nonfinite=True)
    tr.step(x, gt)
    tr.step(x, gt)
    tr.forward_backward(x, gt)
    tr.grad_of("embedding.weight").view(-1)[0] = float("nan")          # waits for the buckets, then poisons the reduced buffer
    tr.optimizer_step()
    torch.cuda.synchronize()
    res[tag] = (tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr.opt_state[:80].clone(), len(tr.reducer.buckets), tr.optimizer_stats())
s, o = res["serial"], res["overlapped"]
assert o[4] >= 3 and s[4] == 0, (s[4], o[4])
assert all(torch.equal(a, b) for a, b in zip(s[:4], o[:4]))
assert o[5]["steps_applied"] == 2 and o[5]["steps_skipped"] == 1 and o[5]["nonfinite"] == 1, o[5]
print("ok", o[4])
dist.destroy_process_group()
'''
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code, cases.REPO, str(tmp_path / "rdv")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
