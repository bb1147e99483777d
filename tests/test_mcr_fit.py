"""The epoch loop, validation and the evaluation loop over a device-resident MCR set (``data.ResidentMCR``): ``train.fit``,
``train.validate`` and ``harness.evaluate_loader`` take it through the same ``PatchSampler`` as the SID set, unchanged.

Setup (that of tests/test_fit.py): RawFormer dim 16, three synthetic uint8 frames of 64 x 128 resident on the device, patches of
32 x 64, batch 2 (a full and a short batch per epoch), ``epochs = 1`` -- epochs 0 and 1, the reference's inclusive range.
Everything compared is bitwise: the same kernels run on the same data in the same order.  That the sampler's output equals the
reference's is pinned by tests/test_mcr_sampler.py.
"""
import math
import random

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)
from bayer_low_light_image_enhancement_amd import synth

SEED, DIM, N, H, W, PATCH, BATCH, EPOCHS, BASE_LR = 43, 16, 3, 64, 128, (32, 64), 2, 1, 1e-3
NAMES = ["Color_RAW_Input/C00100_48mp_0x8_0x0fff.tif", "Color_RAW_Input/C00499_48mp_0x8_0x1fff.tif", "Color_RAW_Input/C00500_48mp_0x8_0x03ff.tif"]


def _frames():
    from bayer_low_light_image_enhancement_amd import mcr_amp_from_names
    amp = mcr_amp_from_names(NAMES)                                                      # 3.0005, 1.5001, 1.0
    mosaic = synth.bayer_mosaic(SEED, N, H, W)[:, 0]                                     # [N,H,W] in [0, 1)
    raw = np.stack([mosaic[k] * 255.0 / amp[k] for k in range(N)]).round().astype(np.uint8)
    gt = (synth.smooth_rgb(SEED, N, H, W).transpose(0, 2, 3, 1) * 255.0).round().astype(np.uint8)
    return raw, np.ascontiguousarray(gt), amp


def _model(device):
    from bayer_low_light_image_enhancement_amd import RawFormer
    m = RawFormer(dim=DIM)
    synth.fill_state_dict(m.state_dict(), SEED)
    return m.to(device).train()


@pytest.fixture(scope="module")
def resident(device):
    from bayer_low_light_image_enhancement_amd import ResidentMCR
    raw, gt, amp = _frames()
    return ResidentMCR(raw, gt, amp, device=device)


@pytest.fixture(scope="module")
def fitted(device, resident, tmp_path_factory):
    """One ``fit`` run shared by the tests: (history, the trained model)."""
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import Trainer, fit
    tr = Trainer(_model(device), lr=BASE_LR, loss="charbonnier", clamp_pred=True)
    history = fit(tr, PatchSampler(resident, PATCH, seed=5), PatchSampler(resident, PATCH), EPOCHS, BATCH, str(tmp_path_factory.mktemp("mcr_fit")), shuffle_seed=9)
    return history, tr.model


@pytest.mark.gpu
def test_epoch_losses_equal_a_hand_written_loop(device, resident, fitted):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import Trainer, warmup_cosine_lr
    history, _ = fitted
    tr = Trainer(_model(device), lr=BASE_LR, loss="charbonnier", clamp_pred=True)
    sampler, order_rng = PatchSampler(resident, PATCH, seed=5), random.Random(9)
    assert [h["epoch"] for h in history] == [0, 1]
    for epoch in range(EPOCHS + 1):
        tr.lr = warmup_cosine_lr(epoch, BASE_LR, EPOCHS)
        order = list(range(N))
        order_rng.shuffle(order)
        epoch_loss = 0
        for k in range(0, N, BATCH):
            x, gt = sampler.batch(order[k: k + BATCH])
            assert x.shape == (len(order[k: k + BATCH]), 1, *PATCH) and gt.shape == (len(order[k: k + BATCH]), 3, *PATCH)
            epoch_loss += float(tr.step(x, gt))
        assert history[epoch]["loss"] == epoch_loss, (epoch, history[epoch]["loss"], epoch_loss)
        assert history[epoch]["lr"] == tr.lr
    assert history[0]["loss"] > 0 and history[0]["loss"] != history[1]["loss"]


@pytest.mark.gpu
def test_validation_runs_on_the_whole_frames(device, resident, fitted):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    from bayer_low_light_image_enhancement_amd.train import validate
    history, model = fitted
    sampler = PatchSampler(resident, PATCH)
    psnr = validate(model, sampler)
    assert math.isfinite(psnr) and psnr > 0 and psnr == history[-1]["psnr"]
    raw, _, amp = _frames()
    model.eval()
    with torch.no_grad():
        for k in range(N):
            x, gt = sampler.whole([k])
            assert x.shape == (1, 1, H, W) and gt.shape == (1, 3, H, W)
            host = (raw[k] / 255 * amp[k]).astype(np.float32)                            # the reference's expression (load_dataset.py:151)
            assert torch.equal(model(x), model(torch.from_numpy(host)[None, None].to(device))), k
    model.train()


@pytest.mark.gpu
def test_evaluation_loop_takes_the_sampler(resident, fitted):
    from bayer_low_light_image_enhancement_amd import PatchSampler, harness
    _, model = fitted
    sampler = PatchSampler(resident, PATCH)
    model.eval()
    res = harness.evaluate_loader(model, (sampler.whole([k]) for k in range(N)))
    model.train()
    assert len(res["psnr"]) == len(res["ssim"]) == N
    assert all(math.isfinite(p) and math.isfinite(s) and -1.0 <= s <= 1.0 for p, s in zip(res["psnr"], res["ssim"]))
    assert math.isfinite(res["psnr_average"]) and math.isfinite(res["ssim_average"])
