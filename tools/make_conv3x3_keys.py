#!/usr/bin/env python3
"""``tests/golden/conv3x3_keys.json``: which 3x3 convolution kernel launch_conv3x3 takes for each of ``cases.CONV3X3_CASES`` and
what it computes, recorded on the MI355X from the library as built (run it at the revision whose selection and results are to be
kept).  Per case ``{"census": {kernel: [launches, flops, bytes]}, "sha256": digest of the output}``: the ``rf_profile_end``
aggregate of the case's one call restricted to the ``conv3x3_kernel`` instantiations.  The same for the output of each of
``cases.CONV3X3_SPLIT_STAGES`` (forward_stage of a ``cases.LAUNCH_CASES`` entry), whose deep 3x3 convolutions run with their input
channels split.  Uses only ops.conv3x3, forward_stage and the profiler brackets, so it runs against any earlier library
(RF_LIB_PATH).

Usage:  python tools/make_conv3x3_keys.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

import cases  # noqa: E402
from make_conv1x1_keys import write  # noqa: E402


def entry(fn):
    y, census = cases.census(fn)
    return {"census": {k: v for k, v in census.items() if k.startswith("conv3x3_kernel")},
            "sha256": hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()}


def record():
    import torch
    from bayer_low_light_image_enhancement_amd import ops

    device = torch.device("cuda:0")
    out = {}
    for tag in cases.CONV3X3_CASES:
        _, run = cases.conv3x3_case(tag)
        out[tag] = entry(lambda: run(ops, device))
        print(f"{tag}: {out[tag]}", flush=True)
    for tag in cases.CONV3X3_SPLIT_STAGES:
        _, run = cases.launch_case(tag, device)
        with torch.no_grad():
            out[tag] = entry(run)
            assert entry(run) == out[tag], f"{tag}: two runs differ"      # the split sums in split order, whatever the arrival order
        print(f"{tag}: {out[tag]}", flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(cases.GOLDEN, "conv3x3_keys.json"))
    a = ap.parse_args()
    write(a.out, record())
