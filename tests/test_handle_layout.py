"""CPU: what the handle's registry and plans decide, against tests/golden/handle_layout.json (tools/make_handle_layout.py recorded it
from the library before the registry moved to csrc/rf_registry.hip and the variant facts into one table): per configuration of
``cases.HANDLE_CONFIGS`` -- every variant, the dims and options at which its registration or its plan takes another path -- the
parameter count, a SHA-256 over the ordered (name, shape, flags) list, rf_packed_bytes, and rf_workspace_bytes or its error code at
``cases.LAYOUT_FRAMES``.  Equality, nothing else: the order of the parameters is the reference's state_dict order, and the packed
size moves with every add_pack call or reservation that is lost, added or reordered across an alignment boundary.

A digest cannot say what moved.  With ``RF_LAYOUT_DUMP=<file>`` naming what ``tools/make_handle_layout.py --dump <file>`` wrote
at the recorded revision, a mismatch prints the first parameter that differs."""
import json
import os

import pytest

import cases

FIXTURE = json.load(open(os.path.join(cases.GOLDEN, "handle_layout.json")))


def first_difference(tag, rows):
    path = os.environ.get("RF_LAYOUT_DUMP")
    if not path or not os.path.exists(path):
        return "set RF_LAYOUT_DUMP to a `tools/make_handle_layout.py --dump` file of the recorded revision to see the first difference"
    want = [tuple(r) for r in json.load(open(path))[tag]]
    got = [tuple(r) for r in rows]
    i = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    return f"first difference at parameter {i}: recorded {want[i] if i < len(want) else None}, now {got[i] if i < len(got) else None}"


def test_fixture_covers_the_configurations():
    assert sorted(FIXTURE) == sorted(cases.HANDLE_CONFIGS)
    assert all(len(v["workspace_bytes"]) == len(cases.LAYOUT_FRAMES) for v in FIXTURE.values())


@pytest.mark.parametrize("tag", list(cases.HANDLE_CONFIGS))
def test_registry_and_plans_are_the_recorded_ones(tag):
    rows, plans = cases.handle_params(tag)
    want = FIXTURE[tag]
    assert len(rows) == want["params"]
    digest = cases.params_digest(rows)
    if digest != want["sha256"]:
        print(first_difference(tag, rows))
    assert digest == want["sha256"]
    assert plans["packed_bytes"] == want["packed_bytes"]
    assert plans["workspace_bytes"] == want["workspace_bytes"]
