"""GPU: the host schedule launches what it launched before it was rewritten around one table of variant facts and one run_stage.

tests/golden/forward_launches.json (tools/make_handle_layout.py --launches, on the MI355X, from the library before that change)
holds per case of ``cases.LAUNCH_CASES`` the ``rf_profile_end`` aggregate of ONE call -- a whole forward, or forward_stage at
stage 1 and stage 4 for the variants that have it -- without the times: ``{kernel: [launches, flops, bytes]}``.  flops and bytes
are what each launch reports from its own arguments (channels, pixels, batch), so a launch that moved to another shape shows
even where the counts agree.  The census must be equal, exactly.  The cases and the schedule decisions they cover: cases.py.

Profiling keeps every launch on the caller's stream: fork and join are not covered here (tests/test_gpu_model.py and the
RF_FAIL_FORK tests do that)."""
import json
import os

import pytest
import torch

import cases

FIXTURE = json.load(open(os.path.join(cases.GOLDEN, "forward_launches.json")))


def recorded(tag, prefix):
    """Launches recorded for ``tag`` of the kernels whose name starts with ``prefix``."""
    return sum(v[0] for k, v in FIXTURE[tag].items() if k.startswith(prefix))


def test_fixture_covers_the_cases_and_both_sides_of_the_decisions():
    assert sorted(FIXTURE) == sorted(cases.LAUNCH_CASES)
    # fuse_tail: the FFN kernel with the stage tail (stages 1 and 7) | without it where the branch follows the block
    assert recorded("flca_d32_b2_64x64", "ffn_fused_kernel<32, true>") == 2 and recorded("plain_d32_b1_32x32", "ffn_fused_kernel<32, true>") == 2
    assert recorded("truecolor_d32_b1_32x32", "ffn_fused_kernel<32, true>") == 0 and recorded("truecolor_d32_b1_32x32", "ffn_fused_kernel<32>") == 2
    # fuse_up: all three decoder steps at a packed width of 64 | only the last one at 72 (level widths 9, 18, 36)
    assert recorded("flca_d32_b2_64x64", "upcat_kernel") == 3 and recorded("flca_d32_b1_40x72", "upcat_kernel") == 1
    # the multi-level step fused (levels 0-1: stages 1, 2, 6, 7) and composed (stages 3, 4, 5), three steps per stage at flca_levels 2
    assert recorded("multilvl_d16_b2_32x48", "ml_step_fused_kernel") == 12 and recorded("multilvl_d16_b2_32x48", "ml_modulate_kernel") == 9
    # WMB: norm2 inside project_in's GEMM | as its own pass at C = 96, 192 (dim 24, stages 3, 4, 5)
    assert recorded("wfb_d16_b1_32x32", "layernorm2d_kernel") == 0 and recorded("wfb_d24_b1_32x32", "layernorm2d_kernel") == 3


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(cases.LAUNCH_CASES))
def test_launch_census_is_the_recorded_one(device, tag):
    _, run = cases.launch_case(tag, device)
    with torch.no_grad():
        run()                                  # parameters packed, workspace allocated
        _, got = cases.census(run)
    want = FIXTURE[tag]
    for k in sorted(set(got) | set(want)):
        if got.get(k) != want.get(k):
            print(f"{tag}: {k}: recorded {want.get(k)}, now {got.get(k)}")
    assert got == want
