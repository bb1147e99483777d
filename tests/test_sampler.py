"""Batch assembly from a device-resident SID set (``rf_sid_sample``, ``data.ResidentSID`` / ``data.PatchSampler``) against what the
reference's ``load_data_SID.__getitem__`` returns (tests/golden/sid_sampler.npz, written by tools/make_train_fixtures.py).

The comparison is ``torch.equal``: the kernel restates the reference's float32 / float64 arithmetic operation by operation.
Shapes are the smallest that reach every branch: 3 frames of 40 x 72 (not square, width no power of two), explicit patches
of 16 x 32 with all four flip combinations, offsets (0, 0) and the last legal (H - ph, W - pw), a repeated and a descending
frame index, raw values below / at the black level and at / above the white level, ground truth 0 and 65535, amplification
100 and 300; the seeded draws use the reference's own square 16 x 16 crops.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import cases  # noqa: F401  (puts the repository on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sid_sampler.npz")
N, H, W = 3, 40, 72


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def resident(device, fx):
    from bayer_low_light_image_enhancement_amd import ResidentSID, amp_from_names
    assert amp_from_names(fx["long_names"].tolist()) == fx["amp"].tolist() == [100.0, 300.0, 100.0]
    ds = ResidentSID(fx["raw"], fx["gt"], amp_from_names(fx["long_names"].tolist()), black=int(fx["black"]), white=int(fx["white"]), device=device)
    assert len(ds) == N and (ds.h, ds.w) == (H, W)
    return ds


def test_fixture_covers_the_branches(fx):
    desc = fx["explicit_desc"]
    assert desc.shape == (6, 4) and fx["explicit_x"].shape == (6, 1, 16, 32) and fx["explicit_gt"].shape == (6, 3, 16, 32)
    assert sorted(set(desc[:, 3].tolist())) == [0, 1, 2, 3]
    assert [0, 0] in desc[:, 1:3].tolist() and [H - 16, W - 32] in desc[:, 1:3].tolist()
    frames = desc[:, 0].tolist()
    assert any(a == b for a, b in zip(frames, frames[1:])) and any(a > b for a, b in zip(frames, frames[1:]))
    assert {100.0, 300.0} == set(fx["amp"][desc[:, 0]].tolist())
    raw, gt = [], []
    for f, i, j, _ in desc.tolist():
        raw.append(fx["raw"][f, i:i + 16, j:j + 32].ravel())
        gt.append(fx["gt"][f, i:i + 16, j:j + 32].ravel())
    raw, gt = set(np.concatenate(raw).tolist()), set(np.concatenate(gt).tolist())
    assert {0, 511, 512, 16383, 16384, 65535} <= raw and {0, 65535} <= gt


@pytest.mark.gpu
def test_explicit_patches_equal_the_reference(resident, fx):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    x, gt = PatchSampler(resident, patch_size=16).gather(fx["explicit_desc"].tolist(), 16, 32)
    assert x.shape == (6, 1, 16, 32) and gt.shape == (6, 3, 16, 32) and x.dtype == gt.dtype == torch.float32
    assert torch.equal(x.cpu(), torch.from_numpy(fx["explicit_x"]))
    assert torch.equal(gt.cpu(), torch.from_numpy(fx["explicit_gt"]))


@pytest.mark.gpu
def test_whole_frames_equal_the_reference(resident, fx):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    x, gt = PatchSampler(resident, patch_size=16).whole([2, 0, 1])
    assert torch.equal(x.cpu(), torch.from_numpy(fx["whole_x"][[2, 0, 1]]))
    assert torch.equal(gt.cpu(), torch.from_numpy(fx["whole_gt"][[2, 0, 1]]))


@pytest.mark.gpu
def test_seeded_draws_equal_the_reference(resident, fx):
    from bayer_low_light_image_enhancement_amd import PatchSampler
    for seed in fx["seeds"].tolist():
        x, gt = PatchSampler(resident, patch_size=int(fx["seeded_patch"]), seed=seed).batch(fx[f"seed{seed}_indices"].tolist())
        assert torch.equal(x.cpu(), torch.from_numpy(fx[f"seed{seed}_x"])), seed
        assert torch.equal(gt.cpu(), torch.from_numpy(fx[f"seed{seed}_gt"])), seed


@pytest.mark.gpu
def test_out_of_range_descriptor_is_skipped_on_the_device(resident, fx):
    """A table the host check never saw (the C entry point called directly): the bad patch is left untouched, the others are
    written, nothing faults."""
    from bayer_low_light_image_enhancement_amd import _lib
    desc = fx["explicit_desc"].copy()
    desc[1] = (N, 0, 0, 0)                 # frame index out of range
    desc[3] = (1, H - 16 + 2, 0, 0)        # over the lower border
    dev = resident.device
    table = torch.from_numpy(desc).to(dev)
    x = torch.full((6, 1, 16, 32), -7.0, device=dev)
    gt = torch.full((6, 3, 16, 32), -7.0, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().rf_sid_sample(C.c_void_p(resident.raw.data_ptr()), C.c_void_p(resident.gt.data_ptr()), C.c_void_p(resident.amp.data_ptr()),
                                             C.c_void_p(table.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(gt.data_ptr()),
                                             N, H, W, 6, 16, 32, resident.black, resident.white, stream), "rf_sid_sample")
    x, gt = x.cpu(), gt.cpu()
    for b in range(6):
        if b in (1, 3):
            assert bool((x[b] == -7.0).all()) and bool((gt[b] == -7.0).all())
        else:
            assert torch.equal(x[b], torch.from_numpy(fx["explicit_x"][b])) and torch.equal(gt[b], torch.from_numpy(fx["explicit_gt"][b]))


def test_argument_checks_answer_before_any_launch():
    """Host logic only (runs without a GPU): the pointers are fake and never dereferenced."""
    from bayer_low_light_image_enhancement_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(1 << 12)
    args = lambda ph, pw: (fake, fake, fake, fake, fake, fake, N, H, W, 2, ph, pw, 512, 16383, None)   # noqa: E731
    assert lib.rf_sid_sample(*args(16, 30)) < 0
    assert lib.rf_last_error() == b"rf_sid_sample: patch width 30 is not a multiple of 4"
    assert lib.rf_sid_sample(*args(48, 32)) < 0
    assert lib.rf_last_error() == b"rf_sid_sample: a 48x32 patch does not fit a 40x72 frame"
    assert lib.rf_sid_sample(fake, fake, fake, fake, fake, fake, N, H, 71, 2, 16, 32, 512, 16383, None) < 0
    assert lib.rf_last_error() == b"rf_sid_sample: frame width 71 is odd"

    def check(rows, ph=16, pw=32):
        table = np.ascontiguousarray(np.array(rows, dtype=np.int32))
        return lib.rf_sid_check_desc(table.ctypes.data_as(C.POINTER(C.c_int)), N, H, W, len(rows), ph, pw)

    assert check([(0, 0, 0, 0), (2, H - 16, W - 32, 3)]) == 0
    assert check([(0, 0, 0, 0), (1, 4, 7, 0)]) < 0                           # odd j
    assert lib.rf_last_error() == b"rf_sid_check_desc: patch 1: offset (4, 7) must be even and not negative"
    assert check([(1, H - 16 + 2, 0, 0)]) < 0                                # over the lower border
    assert lib.rf_last_error() == b"rf_sid_check_desc: patch 0: 16x32 at (26, 0) leaves the 40x72 frame"
    assert check([(0, 0, W - 32 + 2, 0)]) < 0                                # over the right border
    assert lib.rf_last_error() == b"rf_sid_check_desc: patch 0: 16x32 at (0, 42) leaves the 40x72 frame"
    assert check([(0, 0, 0, 0), (0, 0, 0, 0), (N, 0, 0, 0)]) < 0             # frame index >= N
    assert lib.rf_last_error() == b"rf_sid_check_desc: patch 2: frame index 3 out of range (3 frames)"
    assert check([(0, 0, 0, 4)]) < 0
    assert lib.rf_last_error() == b"rf_sid_check_desc: patch 0: flips 4 (bit 0 left-right, bit 1 up-down)"


def test_draw_order_is_the_references(fx):
    """``PatchSampler.draw`` consumes its generator as ``__getitem__`` does: i, j, left-right, up-down per item (no device:
    the dataset is a stand-in with the frame shape)."""
    from bayer_low_light_image_enhancement_amd import PatchSampler
    shape_only = types.SimpleNamespace(n=N, h=H, w=W)
    for seed in fx["seeds"].tolist():
        got = PatchSampler(shape_only, patch_size=int(fx["seeded_patch"]), seed=seed).draw(fx[f"seed{seed}_indices"].tolist())
        assert got == [tuple(r) for r in fx[f"seed{seed}_desc"].tolist()], seed
    a, b = PatchSampler(shape_only, 16, seed=3), PatchSampler(shape_only, 16, seed=3)
    assert a.draw([0, 1]) + a.draw([2]) == b.draw([0, 1, 2])                # a private generator: one stream across calls
