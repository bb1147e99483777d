"""The epoch loop (``train.fit``) and the optimiser state of ``train.Trainer`` on the device.

Setup: RawFormer dim 16, three synthetic uint16 frames of 64 x 128 resident on the device, patches of 32 x 64, batch 2 (so every
epoch has a full and a short batch), ``epochs = 2`` -- epochs 0, 1 and 2, the reference's inclusive range -- and validation on
the whole frames.  Everything compared is bitwise: the same kernels run on the same data in the same order.
"""
import os
import random
import re

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
from bayer_low_light_image_enhancement_amd import synth

SEED, DIM, N, H, W, PATCH, BATCH, EPOCHS, BASE_LR = 41, 16, 3, 64, 128, (32, 64), 2, 2, 1e-3
AMP = [100.0, 300.0, 100.0]


def _frames():
    mosaic = synth.bayer_mosaic(SEED, N, H, W)[:, 0]                                     # [N,H,W] in [0, 1)
    raw = np.stack([512.0 + mosaic[k] * 15871.0 / AMP[k] for k in range(N)]).round().astype(np.uint16)
    gt = (synth.smooth_rgb(SEED, N, H, W).transpose(0, 2, 3, 1) * 65535.0).round().astype(np.uint16)
    return raw, np.ascontiguousarray(gt)


def _model(device):
    from bayer_low_light_image_enhancement_amd import RawFormer
    m = RawFormer(dim=DIM)
    synth.fill_state_dict(m.state_dict(), SEED)
    return m.to(device).train()


@pytest.fixture(scope="module")
def resident(device):
    from bayer_low_light_image_enhancement_amd import ResidentSID
    raw, gt = _frames()
    return ResidentSID(raw, gt, AMP, device=device)


@pytest.fixture(scope="module")
def fitted(device, resident, tmp_path_factory):
    """One ``fit`` run shared by the tests: (history, learning rate seen by every step, output directory)."""
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import Trainer, fit
    out_dir = str(tmp_path_factory.mktemp("fit"))
    tr = Trainer(_model(device), lr=BASE_LR, loss="charbonnier", clamp_pred=True)
    seen, step = [], tr.step

    def spy(x, gt, loss_out=None):
        seen.append(tr.lr)
        return step(x, gt, loss_out=loss_out)

    tr.step = spy
    history = fit(tr, PatchSampler(resident, PATCH, seed=5), PatchSampler(resident, PATCH), EPOCHS, BATCH, out_dir, shuffle_seed=9)
    return history, seen, out_dir


@pytest.mark.gpu
def test_epoch_losses_equal_a_hand_written_loop(device, resident, fitted):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import Trainer, warmup_cosine_lr
    history, seen, _ = fitted
    tr = Trainer(_model(device), lr=BASE_LR, loss="charbonnier", clamp_pred=True)
    sampler, order_rng = PatchSampler(resident, PATCH, seed=5), random.Random(9)
    assert [h["epoch"] for h in history] == [0, 1, 2]
    for epoch in range(EPOCHS + 1):
        tr.lr = warmup_cosine_lr(epoch, BASE_LR, EPOCHS)
        order = list(range(N))
        order_rng.shuffle(order)
        epoch_loss = 0
        for k in range(0, N, BATCH):
            x, gt = sampler.batch(order[k: k + BATCH])
            epoch_loss += float(tr.step(x, gt))
        assert history[epoch]["loss"] == epoch_loss, (epoch, history[epoch]["loss"], epoch_loss)
        assert history[epoch]["lr"] == tr.lr
    assert history[0]["loss"] > 0 and len({h["loss"] for h in history}) == 3


@pytest.mark.gpu
def test_learning_rate_of_every_step_is_the_schedules(fitted):
    from bayer_low_light_image_enhancement_amd.train import warmup_cosine_lr
    history, seen, _ = fitted
    want = [warmup_cosine_lr(e, BASE_LR, EPOCHS) for e in range(EPOCHS + 1)]
    assert want[0] == 0.0 and want[1] == BASE_LR / 20
    assert seen == [lr for lr in want for _ in range(2)]          # two steps per epoch (batches of 2 and 1)


@pytest.mark.gpu
def test_best_checkpoint_has_the_references_layout(device, fitted):
    from bayer_low_light_image_enhancement_amd import RawFormer
    history, _, out_dir = fitted
    ck = torch.load(os.path.join(out_dir, "model_best.pth"))
    assert sorted(ck) == ["epoch", "optimizer", "state_dict"]
    assert ck["epoch"] == history[-1]["best_epoch"] and history[ck["epoch"]]["psnr"] == history[-1]["best_psnr"]
    fresh = RawFormer(dim=DIM)
    fresh.load_state_dict(ck["state_dict"], strict=True)
    opt = torch.optim.Adam(fresh.parameters(), lr=1.0)
    opt.load_state_dict(ck["optimizer"])
    assert opt.param_groups[0]["lr"] == history[ck["epoch"]]["lr"] and opt.param_groups[0]["betas"] == (0.9, 0.999)
    params = list(fresh.parameters())
    assert len(opt.state) == len(params)
    for p in params:
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and int(st["step"]) == 2 * (ck["epoch"] + 1)


@pytest.mark.gpu
def test_log_has_one_reference_format_line_per_epoch(fitted):
    history, _, out_dir = fitted
    lines = open(os.path.join(out_dir, "train_log.txt")).read().splitlines()
    assert len(lines) == EPOCHS + 1
    pat = re.compile(r"^Epoch (\d+)/2 \| Time: \d+\.\d\ds \| Loss: (\d+\.\d{4}) \| Avg PSNR: (\d+\.\d{4}) \| Best PSNR: (\d+\.\d{4}) \(Epoch (\d+)\)$")
    for e, line in enumerate(lines):
        m = pat.match(line)
        assert m, line
        assert int(m.group(1)) == e and m.group(2) == f"{history[e]['loss']:.4f}" and m.group(3) == f"{history[e]['psnr']:.4f}"
        assert m.group(4) == f"{history[e]['best_psnr']:.4f}" and int(m.group(5)) == history[e]["best_epoch"]


@pytest.mark.gpu
def test_resume_is_bit_identical(device, resident, tmp_path):
    """Two steps, checkpoint, a NEW model and Trainer loaded from it, the third step: the parameters (and moments) equal those
    of three uninterrupted steps bit for bit."""
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import Trainer
    batches = [PatchSampler(resident, PATCH, seed=s).batch([0, 2]) for s in (1, 2, 3)]
    a = Trainer(_model(device), lr=BASE_LR, clamp_pred=True)
    for x, gt in batches:
        a.step(x, gt)
    b = Trainer(_model(device), lr=BASE_LR, clamp_pred=True)
    for x, gt in batches[:2]:
        b.step(x, gt)
    path = str(tmp_path / "resume.pth")
    torch.save({"epoch": 0, "state_dict": {k: v.detach().cpu() for k, v in b.model.state_dict().items()}, "optimizer": b.optimizer_state_dict()}, path)
    ck = torch.load(path)
    m = _model(device)
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()                          # nothing of the initial weights may survive the load
    c = Trainer(m, lr=7.0, clamp_pred=True)
    m.load_state_dict(ck["state_dict"], strict=True)
    c.load_optimizer_state_dict(ck["optimizer"])
    assert c.step_no == 2 and c.lr == BASE_LR
    assert torch.equal(c.flat, b.flat) and torch.equal(c.m, b.m) and torch.equal(c.v, b.v)
    c.step(*batches[2])
    assert not torch.equal(c.flat, b.flat)
    assert torch.equal(c.flat, a.flat) and torch.equal(c.m, a.m) and torch.equal(c.v, a.v)
    # the same state through a real torch.optim.Adam and back
    opt = torch.optim.Adam(m.parameters(), lr=1.0)
    opt.load_state_dict(a.optimizer_state_dict())
    c.load_optimizer_state_dict(opt.state_dict())
    assert c.step_no == 3 and torch.equal(c.m, a.m) and torch.equal(c.v, a.v)
