#!/usr/bin/env python3
"""MI355X: record tests/golden/attn_mid_parent.json, the digests tests/test_attn_mid_bits.py compares with.

    python3 tools/record_attn_mid_golden.py [out.json [commit]]

Run it on the commit whose bits are the reference (the parent of a change that must not move them).  Per case of the test: the
SHA-256 of the output bytes of ops.channel_attention (little-endian float32) and a handful of values in hex, for diagnosis.
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import torch  # noqa: E402
import test_attn_mid_bits as T  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
device = torch.device("cuda:0")
try:                                     # (a tree exported without its .git: pass the commit as the second argument)
    rev = sys.argv[2] if len(sys.argv) > 2 else subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True, stderr=subprocess.DEVNULL).strip()
except Exception:
    rev = None
doc = {"tool": "tools/record_attn_mid_golden.py", "recorded_at_commit": rev, "device": torch.cuda.get_device_name(0),
       "heads": T.HEADS, "seed": T.SEED, "cases": {}}
for case in T.CASES:
    out = T.run_case(case, device)
    flat = out.reshape(-1)
    doc["cases"][T.case_id(case)] = {"shape": list(out.shape), "sha256": T.digest(out),
                                    "samples": [float(flat[i]).hex() for i in T.sample_index(flat.size)]}
    print(T.case_id(case), doc["cases"][T.case_id(case)]["sha256"], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", out_path)
