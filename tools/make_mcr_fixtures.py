"""Fixture of the MCR data path, written by the reference project's own code:

    python tools/make_mcr_fixtures.py --reference <checkout of the reference project>

``tests/golden/mcr_sampler.npz``   small uint8 frames and what ``load_data_MCR.__getitem__`` (RawFomer_WFB_FFAB/load_dataset.py:117-179)
                                   returns for them

Only data is written; nothing of the reference's program text is copied.  The reference is imported with ``rawpy`` / ``tqdm`` /
``imageio`` stubbed where they are absent (file decoding is not exercised) and the dataset object is built without its
``__init__`` (which reads tif / jpg files): the frame lists and the path list are set directly.  The exposure ratio the
reference computes from a file name is a local of ``__getitem__``; it is read from that frame when the call returns.

Set A, 3 frames of 41 x 74 (W = 2 and H W = 2 mod 4: a row segment starts on either half of a dword, changing from row to
row and from frame to frame), has two parts:

* ``explicit``: 16 x 32 patches at chosen descriptors (all flip combinations, j = 0 and 2 mod 4, the corners (0, 0) and the last
  legal even (24, 42), repeated and descending frame indices).  The reference only cuts square patches at offsets up to
  H - P - 2, so here the crop and the flips are numpy slicing in this tool and the reference's ``training=False`` path
  normalises the result.
* ``seeded``: ``random.seed(s)`` then ``dataset[idx]`` for an index list, ``patch_size = 16`` -- crop, flips and normalisation
  are all the reference's.  The four draws of every item are recorded through a logging proxy of the ``random`` module the
  dataset uses, as ``(i, j, flips)``.

Set B, 2 frames of 32 x 48: ``training=False`` on the frames themselves (``whole``); the last frame ends on the last byte of
the arrays.
"""
from __future__ import annotations

import argparse
import importlib
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_train_fixtures import GOLDEN, LoggedRandom, stub_missing  # noqa: E402

N, H, W = 3, 41, 74
EDGES = [0, 1, 254, 255]
# MCR's own naming, C<5-digit image number>_48mp_0x8_0x<exposure, 4 hex digits>.tif: [-23:-20] = the number's last three digits,
# [-8:-4] = the exposure.  gt_expo 12287 below number 500, 1023 from there on: 12287 / 255, 12287 / 8191, 1023 / 1023 = 1.0
NAMES = ["Mono_Colored_RAW_Paired_DATASET/Color_RAW_Input/C00012_48mp_0x8_0x00ff.tif",
         "Mono_Colored_RAW_Paired_DATASET/Color_RAW_Input/C00499_48mp_0x8_0x1fff.tif",
         "Mono_Colored_RAW_Paired_DATASET/Color_RAW_Input/C00500_48mp_0x8_0x03ff.tif"]
PH, PW = 16, 32
# frame, i, j, flips (bit 0 left-right, bit 1 up-down); (24, 42) = the last even offsets at which 16 x 32 fits 41 x 74
EXPLICIT = [(0, 0, 0, 0), (2, 24, 42, 1), (2, 0, 42, 2), (1, 24, 0, 3), (1, 12, 22, 1), (0, 6, 36, 2), (0, 24, 42, 0)]
SEEDED = {7: [0, 1, 2, 2, 1, 0, 1, 1], 1234: [2, 2, 0, 1, 0, 2, 1, 0, 0, 1, 2, 1]}
SEEDED_PATCH = 16
NB, HB, WB = 2, 32, 48
NAMES_B = ["Mono_Colored_RAW_Paired_DATASET/Color_RAW_Input/C00100_48mp_0x8_0x0fff.tif",
           "Mono_Colored_RAW_Paired_DATASET/Color_RAW_Input/C00700_48mp_0x8_0x00ff.tif"]


def make_frames(seed, n, h, w):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, h, w), dtype=np.int64)
    pick = rng.random(raw.shape) < 0.10
    raw[pick] = rng.choice(EDGES, size=int(pick.sum()))
    gt = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.int64)
    pick = rng.random(gt.shape) < 0.10
    gt[pick] = rng.choice(EDGES, size=int(pick.sum()))
    return raw.astype(np.uint8), gt.astype(np.uint8)


def dataset(mod, inp_list, gt_list, names, patch, training):
    ds = mod.load_data_MCR.__new__(mod.load_data_MCR)
    ds.training, ds.patch_size, ds.train_c_path = training, patch, names
    ds.inp_list, ds.gt_list = inp_list, gt_list
    return ds


def items_and_amps(ds, indices):
    """``ds[k]`` for every index, and the ``amp`` each call computed (a local of the reference's ``__getitem__``)."""
    amps = []

    def tracer(frame, event, arg):
        if event == "call" and frame.f_code.co_name == "__getitem__":
            def local(frame, event, arg):
                if event == "return":
                    amps.append(frame.f_locals["amp"])
                return local
            return local
        return None

    sys.settrace(tracer)
    try:
        items = [ds[k] for k in indices]
    finally:
        sys.settrace(None)
    assert len(amps) == len(items) and all(type(a) is float for a in amps)
    return items, amps


def sampler_fixture(mod):
    raw, gt = make_frames(20241018, N, H, W)
    assert W % 4 == 2 and (H * W) % 4 == 2
    frames, truths = [raw[k] for k in range(N)], [gt[k] for k in range(N)]
    out = {"raw": raw, "gt": gt, "names": np.array(NAMES)}

    # the reference's amp of every frame (whole frames through training=False; the arrays themselves are not kept for set A)
    _, amps = items_and_amps(dataset(mod, frames, truths, NAMES, SEEDED_PATCH, False), range(N))
    out["amp"] = np.array(amps, dtype=np.float64)
    assert out["amp"][0] > 1 and out["amp"][1] > 1 and out["amp"][2] == 1.0, out["amp"]

    # explicit descriptors: crop and flip here, the reference normalises
    inps, gts, names = [], [], []
    for f, i, j, flips in EXPLICIT:
        assert i % 2 == 0 and j % 2 == 0 and i + PH <= H and j + PW <= W
        s, t = raw[f, i:i + PH, j:j + PW], gt[f, i:i + PH, j:j + PW, :]
        if flips & 1:
            s, t = s[:, ::-1], t[:, ::-1]
        if flips & 2:
            s, t = s[::-1], t[::-1]
        inps.append(np.ascontiguousarray(s))
        gts.append(np.ascontiguousarray(t))
        names.append(NAMES[f])
    assert set(EDGES) <= set(np.concatenate([s.ravel() for s in inps]).tolist()), "the explicit patches must hold every raw edge value"
    assert {0, 255} <= set(np.concatenate([t.ravel() for t in gts]).tolist()), "the explicit patches must hold both ground-truth ends"
    assert {d[3] for d in EXPLICIT} == {0, 1, 2, 3} and {d[2] % 4 for d in EXPLICIT} == {0, 2}
    ds = dataset(mod, inps, gts, names, SEEDED_PATCH, False)
    items = [ds[k] for k in range(len(EXPLICIT))]
    out["explicit_desc"] = np.array(EXPLICIT, dtype=np.int32)
    out["explicit_x"] = np.stack([a.numpy() for a, _ in items])
    out["explicit_gt"] = np.stack([b.numpy() for _, b in items])

    # seeded draws: everything by the reference
    ds = dataset(mod, frames, truths, NAMES, SEEDED_PATCH, True)
    real_random = mod.random
    for seed, indices in SEEDED.items():
        log = LoggedRandom()
        mod.random = log
        try:
            random.seed(seed)
            items = [ds[k] for k in indices]
        finally:
            mod.random = real_random
        draws = np.array(log.calls, dtype=np.int64).reshape(len(indices), 4)
        desc = np.stack([np.array(indices), draws[:, 0] * 2, draws[:, 1] * 2, (draws[:, 2] > 50) + 2 * (draws[:, 3] < 20)], axis=1)
        out[f"seed{seed}_indices"] = np.array(indices, dtype=np.int32)
        out[f"seed{seed}_desc"] = desc.astype(np.int32)
        out[f"seed{seed}_x"] = np.stack([a.numpy() for a, _ in items])
        out[f"seed{seed}_gt"] = np.stack([b.numpy() for _, b in items])
    out["seeds"] = np.array(sorted(SEEDED), dtype=np.int32)
    out["seeded_patch"] = np.int32(SEEDED_PATCH)
    flips_seen = set(int(v) for s in SEEDED for v in out[f"seed{s}_desc"][:, 3])
    assert flips_seen == {0, 1, 2, 3}, f"the seeded draws reach flips {sorted(flips_seen)} only: choose other seeds"

    # set B: whole frames
    raw_b, gt_b = make_frames(20241019, NB, HB, WB)
    ds = dataset(mod, [raw_b[k] for k in range(NB)], [gt_b[k] for k in range(NB)], NAMES_B, SEEDED_PATCH, False)
    items, amps = items_and_amps(ds, range(NB))
    out.update({"raw_b": raw_b, "gt_b": gt_b, "names_b": np.array(NAMES_B), "amp_b": np.array(amps, dtype=np.float64)})
    out["whole_x"] = np.stack([a.numpy() for a, _ in items])
    out["whole_gt"] = np.stack([b.numpy() for _, b in items])

    for k, v in out.items():
        if k.endswith("_x") or k.endswith("_gt"):
            assert v.dtype == np.float32, (k, v.dtype)
    path = os.path.join(GOLDEN, "mcr_sampler.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; amp", out["amp"].tolist(), out["amp_b"].tolist())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    stub_missing(["rawpy", "tqdm", "imageio"])
    sys.path.insert(0, os.path.join(args.reference, "RawFomer_WFB_FFAB"))
    mod = importlib.import_module("load_dataset")
    os.makedirs(GOLDEN, exist_ok=True)
    sampler_fixture(mod)


if __name__ == "__main__":
    main()
