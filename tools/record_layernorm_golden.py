#!/usr/bin/env python3
"""MI355X: record tests/golden/layernorm_parent.json, the digests tests/test_layernorm_bits.py compares with.

    python3 tools/record_layernorm_golden.py [out.json [commit]]

Run it on the commit whose bits are the reference (the parent of a change that must not move them), TWICE, into two files: the
two recordings must be the same bytes (the file holds no time stamp) before one of them is committed.  Per case of the test and
per array the SHA-256 of the bytes (little-endian float32), the shape and a handful of values in hex.  The test module and this
tool use only operators that the parent has, so both run in a checkout of it.
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import torch  # noqa: E402
import test_layernorm_bits as T  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
device = torch.device("cuda:0")
try:                                     # (a tree exported without its .git: pass the commit as the second argument)
    rev = sys.argv[2] if len(sys.argv) > 2 else subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True, stderr=subprocess.DEVNULL).strip()
except Exception:
    rev = None
doc = {"tool": "tools/record_layernorm_golden.py", "recorded_at_commit": rev, "device": torch.cuda.get_device_name(0), "cases": {}}
for tag in T.CASE_IDS:
    doc["cases"][tag] = T.record(T.run_case(tag, device))
    print(tag, {k: v["sha256"][:16] for k, v in doc["cases"][tag].items()}, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", out_path)
