"""Fixtures of the training data path, written by the reference project's own code:

    python tools/make_train_fixtures.py --reference <checkout of the reference project>

``tests/golden/sid_sampler.npz``   small uint16 frames and what ``load_data_SID.__getitem__`` (RawFomer_WFB_FFAB/load_dataset.py)
                                   returns for them
``tests/golden/lr_schedule.json``  the learning rates a real ``torch.optim.Adam`` holds under the reference's scheduler pair
                                   (train.py:113-115, RawFomer_WFB_FFAB/warmup_scheduler.py)

Only data is written; nothing of the reference's program text is copied.  The reference is imported with ``rawpy`` / ``tqdm`` /
``imageio`` stubbed where they are absent (file decoding is not exercised) and the dataset object is built without its
``__init__`` (which reads ARW files): the frame lists are set directly.

The sampler fixture has three parts:

* ``seeded``: ``random.seed(s)`` then ``dataset[idx]`` for an index list, ``patch_size = 16`` on 40 x 72 frames -- crop, flips
  and normalisation are all the reference's.  The four draws of every item are recorded through a logging proxy of the
  ``random`` module the dataset uses, as ``(i, j, flips)``.
* ``explicit``: 16 x 32 patches at chosen descriptors (all flip combinations, the corners of the legal offset range, repeated
  and descending frame indices).  The reference only cuts square patches at offsets up to H - P - 2, so here the crop and the
  flips are numpy slicing in this tool and the reference's ``training=False`` path normalises the result.
* ``whole``: ``training=False`` on the frames themselves.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import random
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

N, H, W = 3, 40, 72
BLACK, WHITE = 512, 16383
RAW_EDGES = [0, 511, 512, 513, 16382, 16383, 16384, 65535]          # below / at the black level, at / above the white level
GT_EDGES = [0, 1, 65534, 65535]
LONG_NAMES = ["long/00001_00_10s.ARW", "long/00002_00_30s.ARW", "long/10003_00_10s.ARW"]      # [-7] == '3' -> 300, else 100
PH, PW = 16, 32
# frame, i, j, flips (bit 0 left-right, bit 1 up-down)
EXPLICIT = [(0, 0, 0, 0), (2, H - PH, W - PW, 1), (2, 0, W - PW, 2), (1, H - PH, 0, 3), (1, 12, 22, 1), (0, 6, 38, 2)]
SEEDED = {7: [0, 1, 2, 2, 1, 0, 1, 1], 1234: [2, 2, 0, 1, 0, 2, 1, 0, 0, 1, 2, 1]}
SEEDED_PATCH = 16


def stub_missing(names):
    for name in names:
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)


class LoggedRandom:
    """Stands in for the ``random`` module inside the reference's dataset module: same generator, every ``randint`` recorded."""

    def __init__(self):
        self.calls = []

    def randint(self, a, b):
        v = random.randint(a, b)
        self.calls.append(v)
        return v


def make_frames():
    rng = np.random.default_rng(20240607)
    raw = rng.integers(0, 20000, size=(N, H, W), dtype=np.int64)
    pick = rng.random(raw.shape) < 0.15
    raw[pick] = rng.choice(RAW_EDGES, size=int(pick.sum()))
    gt = rng.integers(0, 65536, size=(N, H, W, 3), dtype=np.int64)
    pick = rng.random(gt.shape) < 0.05
    gt[pick] = rng.choice(GT_EDGES, size=int(pick.sum()))
    return raw.astype(np.uint16), gt.astype(np.uint16)


def dataset(mod, short_list, long_list, names, patch, training):
    ds = mod.load_data_SID.__new__(mod.load_data_SID)
    ds.training, ds.patch_size, ds.long_expo_files = training, patch, names
    ds.short_list, ds.long_list = short_list, long_list
    return ds


def sampler_fixture(mod):
    raw, gt = make_frames()
    out = {"raw": raw, "gt": gt, "amp": np.array([300.0 if n[-7] == "3" else 100.0 for n in LONG_NAMES], dtype=np.float32),
           "long_names": np.array(LONG_NAMES), "black": np.int32(BLACK), "white": np.int32(WHITE)}
    frames, truths = [raw[k] for k in range(N)], [gt[k] for k in range(N)]

    # whole frames
    ds = dataset(mod, frames, truths, LONG_NAMES, SEEDED_PATCH, False)
    items = [ds[k] for k in range(N)]
    out["whole_x"] = np.stack([a.numpy() for a, _ in items])
    out["whole_gt"] = np.stack([b.numpy() for _, b in items])

    # explicit descriptors: crop and flip here, the reference normalises
    shorts, longs, names = [], [], []
    for f, i, j, flips in EXPLICIT:
        s, t = raw[f, i:i + PH, j:j + PW], gt[f, i:i + PH, j:j + PW, :]
        if flips & 1:
            s, t = s[:, ::-1], t[:, ::-1]
        if flips & 2:
            s, t = s[::-1], t[::-1]
        shorts.append(np.ascontiguousarray(s))
        longs.append(np.ascontiguousarray(t))
        names.append(LONG_NAMES[f])
    assert set(RAW_EDGES) <= set(np.concatenate([s.ravel() for s in shorts]).tolist()), "the explicit patches must hold every raw edge value"
    assert set(GT_EDGES) <= set(np.concatenate([t.ravel() for t in longs]).tolist()), "the explicit patches must hold every ground-truth edge value"
    ds = dataset(mod, shorts, longs, names, SEEDED_PATCH, False)
    items = [ds[k] for k in range(len(EXPLICIT))]
    out["explicit_desc"] = np.array(EXPLICIT, dtype=np.int32)
    out["explicit_x"] = np.stack([a.numpy() for a, _ in items])
    out["explicit_gt"] = np.stack([b.numpy() for _, b in items])

    # seeded draws: everything by the reference
    ds = dataset(mod, frames, truths, LONG_NAMES, SEEDED_PATCH, True)
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
    print("seeded flips seen:", sorted(flips_seen))
    for k, v in out.items():
        if k.endswith("_x") or k.endswith("_gt"):
            assert v.dtype == np.float32, (k, v.dtype)
    np.savez_compressed(os.path.join(GOLDEN, "sid_sampler.npz"), **out)


def schedule_fixture(warm):
    import torch
    result = {"base_lr": 1e-4, "warmup": 20, "eta_min": 1e-5, "runs": []}
    for epochs, keep in ((60, list(range(61))), (3000, list(range(41)) + [1500, 3000])):
        p = torch.nn.Parameter(torch.zeros(1))
        optimizer = torch.optim.Adam([p], lr=result["base_lr"])
        scheduler_cosine = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, epochs, eta_min=result["eta_min"])
        scheduler = warm.GradualWarmupScheduler(optimizer, multiplier=1, total_epoch=result["warmup"], after_scheduler=scheduler_cosine)
        lrs = {}
        for epoch in range(epochs + 1):
            if epoch in keep:
                lrs[str(epoch)] = float(optimizer.param_groups[0]["lr"])
            p.grad = torch.ones(1)
            optimizer.step()
            scheduler.step()
        result["runs"].append({"epochs": epochs, "lr": lrs})
    with open(os.path.join(GOLDEN, "lr_schedule.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    stub_missing(["rawpy", "tqdm", "imageio"])
    sys.path.insert(0, os.path.join(args.reference, "RawFomer_WFB_FFAB"))
    mod = importlib.import_module("load_dataset")
    warm = importlib.import_module("warmup_scheduler")
    os.makedirs(GOLDEN, exist_ok=True)
    sampler_fixture(mod)
    schedule_fixture(warm)


if __name__ == "__main__":
    main()
