#!/usr/bin/env python3
"""Fixtures that pin what the handle's host code decides, recorded from the library as built (run it at the revision whose
behaviour is to be kept, before editing the registry or the schedules):

* ``tests/golden/handle_layout.json`` (no GPU): per ``cases.HANDLE_CONFIGS`` entry the parameter count, a SHA-256 over the ordered
  ``(name, shape, flags)`` list, ``rf_packed_bytes`` and ``rf_workspace_bytes`` (or its error code) at ``cases.LAYOUT_FRAMES``;
* ``tests/golden/forward_launches.json`` (``--launches``, on the MI355X): per ``cases.LAUNCH_CASES`` entry the ``rf_profile_end``
  aggregate of one call without the times, ``{kernel: [launches, flops, bytes]}``.

Usage:  python tools/make_handle_layout.py [--dump FILE] [--launches] [--out DIR]

``--dump FILE`` also writes the full parameter lists (what the digests are taken over) as JSON, to compare two revisions by hand;
tests/test_handle_layout.py names the first differing parameter against such a file (RF_LAYOUT_DUMP).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import cases  # noqa: E402


def layout():
    out = {}
    for tag in cases.HANDLE_CONFIGS:
        rows, plans = cases.handle_params(tag)
        out[tag] = {"params": len(rows), "sha256": cases.params_digest(rows), **plans}
    return out


def launch_census():
    import torch

    device = torch.device("cuda:0")
    out = {}
    for tag in cases.LAUNCH_CASES:
        _, run = cases.launch_case(tag, device)
        with torch.no_grad():
            run()                                  # parameters packed, workspace allocated
            _, out[tag] = cases.census(run)
        print(f"{tag}: {sum(v[0] for v in out[tag].values())} launches of {len(out[tag])} kernels", flush=True)
    return out


def write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="also write the full (name, shape, flags) lists to this file")
    ap.add_argument("--launches", action="store_true", help="record forward_launches.json instead (needs the GPU)")
    ap.add_argument("--out", default=cases.GOLDEN, help="directory of the fixtures")
    a = ap.parse_args()
    if a.launches:
        write(os.path.join(a.out, "forward_launches.json"), launch_census())
    else:
        write(os.path.join(a.out, "handle_layout.json"), layout())
    if a.dump:
        write(os.path.abspath(a.dump), {tag: cases.handle_params(tag)[0] for tag in cases.HANDLE_CONFIGS})
