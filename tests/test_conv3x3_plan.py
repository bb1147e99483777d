"""The 3x3 convolution launch plan (plan_conv3x3, rf_conv3x3.hip): one host function chooses the kernel instantiation, the launch
geometry and the profiler key; launch_conv3x3 looks the plan up in the table of instantiations and launches what it says.

tests/golden/conv3x3_keys.json (tools/make_conv3x3_keys.py, on the MI355X, from the library before launch_conv3x3 was split into
plan and table) holds per case of ``cases.CONV3X3_CASES`` the ``rf_profile_end`` aggregate of the case's one call restricted to
the conv3x3_kernel instantiations, ``{kernel: [launches, flops, bytes]}``, and the SHA-256 of its output; and the same for the two
``cases.CONV3X3_SPLIT_STAGES``, whose level-3 convolutions run with their input channels split.

CPU: rf_conv3x3_plan names the recorded kernel for every case; it agrees with ``parent_plan``, a restatement of the ladder that
launch_conv3x3 / launch_rw / ksplit_for / level0_path were before the plan existed, over a sweep that selects every instantiation;
and the library holds exactly those.  GPU: the launch is the recorded one, the result is within the tolerance of
tests/test_gpu_ops.py::test_conv3x3 of a float64 convolution, and bit for bit what the library computed before.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import re

import pytest
import torch

import cases
from bayer_low_light_image_enhancement_amd import _lib, build, isa_check
from oracle import rawformer_ref as R

TOL = 2e-5   # tests/test_gpu_ops.py: TOL of test_conv3x3
FIXTURE = json.load(open(os.path.join(cases.GOLDEN, "conv3x3_keys.json")))
STORE = {"plain": 0, "unshuffle": 1, "shuffle": 2}

# every instantiation there is, as (NCO, LOG2_RW, RPW, NWV, KS, L0): the 4-wave tiles with and without the input-channel split,
# the 8-wave forms, the two 16-row forms and their level-0 twins
NARROW = [(n, l, 1, 4, ks, 0) for n in (1, 2, 3, 4) for l in (0, 1, 2) for ks in (0, 1)]
SELECTABLE = sorted(NARROW + [(n, 0, 1, 8, 0, 0) for n in (1, 2, 3, 4)] + [(2, 0, 2, 8, 0, 0), (2, 0, 2, 8, 0, 3), (1, 0, 1, 16, 0, 0), (1, 0, 1, 16, 0, 3)])


def key_of(inst):
    """The profiler key of an instantiation: a split launch reports the key of the unsplit kernel."""
    return "conv3x3_kernel<%d, %d, %d, %d%s>" % (*inst[:4], ", false, 3" if inst[5] else "")


def cdiv(a, b):
    return -(-a // b)


def split_floats(b, cout, h, w):
    """conv3x3_ksplit_floats: the split scratch the forward pass gives a convolution of this size."""
    return 4096 + 8 * b * cout * h * w if b * h * w <= 16384 else 0


def plan(b, cin, cout, h, w, store=0, unshuffle_in=0, aligned=1, ks_floats=0):
    """rf_conv3x3_plan: (key, grid, block, ksplit, level-0 path)."""
    key, grid, block, ksplit, l0 = C.create_string_buffer(64), (C.c_int * 3)(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().rf_conv3x3_plan(b, cin, cout, h, w, store, unshuffle_in, aligned, ks_floats, key, len(key), grid, C.byref(block),
                                           C.byref(ksplit), C.byref(l0)), "rf_conv3x3_plan")
    return key.value.decode(), tuple(grid), block.value, ksplit.value, bool(l0.value)


def parent_plan(b, cin, cout, h, w, store=0, unshuffle_in=0, aligned=1, ks_floats=0):
    """What the launcher did before plan_conv3x3, restated from its four functions in their own order: launch_conv3x3 (output
    tiles per workgroup, the small rule, vec), launch_rw (the five-branch ladder and grid_for_tiles), ksplit_for and level0_path.
    Returns (instantiation, grid, block, ksplit)."""
    nt = cdiv(cout, 16)
    nco = 4
    if nt % 4:
        nco = 3 if nt % 3 == 0 else 2 if nt % 2 == 0 else 1 if nt == 1 else 4
    small = False
    if w > 32 and h >= 8 and cdiv(w, 64) * cdiv(h, 16 if nco <= 2 else 8) * cdiv(nt, nco) * b < 128:
        small = True
        t4 = cdiv(w, 64) * cdiv(h, 4) * b
        while nco > 1 and t4 * cdiv(nt, nco) < 192:
            nco = nco // 2 if nco in (4, 2) else 1
    ngroups = cdiv(nt, nco)
    vec = w % 4 == 0 and bool(aligned)                  # dense strides Cin h w / Cout h w are multiples of 4 where w is
    lrw = 0 if w > 32 else 1 if w > 16 else 2
    rpwb = 2 if nco <= 2 else 1
    level0 = not small and nco <= 2 and w > 32 and h >= 16 and cin <= 32 and not unshuffle_in and w % 4 == 0 and bool(aligned)

    def grid_x(ntiles):
        return ngroups * cdiv(ntiles, (ntiles * ngroups * b + 255) // 256)

    def ksplit_for(ntiles):
        total, nchunks = ntiles * ngroups * b, cdiv(cin, 8)
        if not ks_floats or not vec or total > 64 or total > 4096 or nchunks < 8 or grid_x(ntiles) != ngroups * ntiles:
            return 1
        s = min(nchunks // 4, 8)
        while s > 1 and total * s > 256:
            s -= 1
        return 1 if s < 2 or 4096 + s * b * cout * h * w > ks_floats else s

    s = 1
    if small and lrw == 0:
        ntiles = cdiv(w, 64) * cdiv(h, 4)
        s = ksplit_for(ntiles)
        inst = (nco, 0, 1, 4, int(s > 1), 0)
    elif nco == 1 and lrw == 0 and h >= 16:
        ntiles = cdiv(w, 64) * cdiv(h, 16)
        inst = (1, 0, 1, 16, 0, 3 if level0 else 0)
    elif lrw == 0 and h >= 8 * rpwb:
        ntiles = cdiv(w, 64) * cdiv(h, 8 * rpwb)
        inst = (nco, 0, rpwb, 8, 0, 3 if nco == 2 and level0 else 0)
    elif lrw == 0 and h >= 8:
        ntiles = cdiv(w, 64) * cdiv(h, 8)
        inst = (nco, 0, 1, 8, 0, 0)
    else:
        ntiles = cdiv(w, 64 >> lrw) * cdiv(h, 4 << lrw)
        s = ksplit_for(ntiles)
        inst = (nco, lrw, 1, 4, int(s > 1), 0)
    return inst, (grid_x(ntiles), b, s), 64 * inst[3], s, ngroups * ntiles * b


def test_fixture_covers_the_cases_and_every_unsplit_instantiation():
    assert sorted(FIXTURE) == sorted([*cases.CONV3X3_CASES, *cases.CONV3X3_SPLIT_STAGES])
    assert all(len(FIXTURE[t]["census"]) == 1 and next(iter(FIXTURE[t]["census"].values()))[0] == 1 for t in cases.CONV3X3_CASES), "one launch per case"
    assert sorted({k for t in cases.CONV3X3_CASES for k in FIXTURE[t]["census"]}) == sorted({key_of(i) for i in SELECTABLE})
    stores = {c[5] for c in cases.CONV3X3_CASES.values()}
    assert stores == set(STORE) and any(c[4] % 4 for c in cases.CONV3X3_CASES.values()) and any(c[1] % 8 for c in cases.CONV3X3_CASES.values())


@pytest.mark.parametrize("tag", list(cases.CONV3X3_CASES))
def test_plan_names_the_recorded_kernel(tag):
    b, cin, cout, h, w, store = cases.CONV3X3_CASES[tag]
    key, grid, block, ksplit, l0 = plan(b, cin, cout, h, w, STORE[store])
    assert [key] == list(FIXTURE[tag]["census"]), tag
    assert ksplit == 1 and grid[1:] == (b, 1) and grid[0] >= 1 and l0 == key.endswith("false, 3>"), "no split scratch through ops.conv3x3"
    assert block == 64 * int(re.search(r"(\d+)(, false, 3)?>$", key).group(1))


def test_plan_of_the_split_stages():
    """Level 3 of a 32 x 32 frame: a 4 x 4 frame of 128 (dim 16) or 256 (dim 32) channels, one 16 x 16 tile in four output groups."""
    for c, s in ((128, 4), (256, 8)):
        assert plan(1, c, c, 4, 4, ks_floats=split_floats(1, c, 4, 4)) == ("conv3x3_kernel<4, 2, 1, 4>", (c // 64, 1, s), 256, s, False)
        assert plan(1, c, c, 4, 4) == ("conv3x3_kernel<4, 2, 1, 4>", (c // 64, 1, 1), 256, 1, False)


# the sweep of the parent's ladder.  The two frames of 16 images are not part of the product: <1, 0, 1, 8> and <2, 0, 1, 8> need 128
# workgroups of ONE 16-row tile each at one or two output tiles, which no batch up to 8 and width up to 512 has.
SWEEP = list(itertools.product((1, 2, 8), (4, 8, 20, 32, 40, 64, 128, 256), (3, 12, 16, 32, 48, 64, 80, 128, 256),
                               (4, 7, 8, 15, 16, 17, 32, 33, 64, 66, 128, 512), (4, 7, 8, 15, 16, 17, 32, 33, 64, 66, 128, 512)))
SWEEP += [(16, 8, 16, 15, 512), (16, 40, 32, 8, 512)]


def test_plan_equals_the_parents_ladder_and_selects_every_instantiation():
    lib = _lib.load()
    key, grid, block, ksplit, l0 = C.create_string_buffer(64), (C.c_int * 3)(), C.c_int(), C.c_int(), C.c_int()
    out = (key, len(key), grid, C.byref(block), C.byref(ksplit), C.byref(l0))
    seen = set()
    for (b, cin, cout, h, w), aligned, scratch in itertools.product(SWEEP, (1, 0), (1, 0)):
        ks_floats = split_floats(b, cout, h, w) if scratch else 0
        inst, pgrid, pblock, s, total = parent_plan(b, cin, cout, h, w, 0, 0, aligned, ks_floats)
        assert lib.rf_conv3x3_plan(b, cin, cout, h, w, 0, 0, aligned, ks_floats, *out) == 0, lib.rf_last_error()
        got = (key.value.decode(), tuple(grid), block.value, ksplit.value, bool(l0.value))
        assert got == (key_of(inst), pgrid, pblock, s, inst[5] == 3), (b, cin, cout, h, w, aligned, ks_floats)
        if s > 1:      # the split invariant: one tile per workgroup, at most 64 of them, split into at most 256
            assert pgrid[0] * b == total <= 64 and total * s <= 256 and inst[4] == 1
        seen.add(inst)
    assert sorted(seen) == SELECTABLE and len(SELECTABLE) == 32


def test_library_holds_exactly_the_selectable_instantiations():
    names = [n for n in isa_check.kernel_names(build.build_library()) if re.search(r"\d+conv3x3_kernelI", n)]      # not dwconv3x3_kernel
    insts = sorted(tuple(int(v) for v in re.search(r"conv3x3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE", n).groups()) for n in names)
    assert insts == SELECTABLE, (sorted(set(insts) - set(SELECTABLE)), sorted(set(SELECTABLE) - set(insts)))


def test_plan_refuses_what_the_launch_refuses():
    lib = _lib.load()
    out = (C.create_string_buffer(64), 64, (C.c_int * 3)(), C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_int()))
    for args, text in (((0, 8, 16, 8, 8, 0, 0), b"bad sizes"), ((1, 8, 0, 8, 8, 0, 0), b"bad sizes"), ((65536, 8, 16, 8, 8, 0, 0), b"bad sizes"),
                       ((1, 8, 16, 7, 8, 1, 0), b"store mode 1 incompatible"), ((1, 8, 18, 8, 8, 2, 0), b"store mode 2 incompatible"),
                       ((1, 8, 16, 8, 8, 3, 0), b"store mode 3 incompatible"), ((1, 8, 16, 8, 8, 0, 1), b"exactly 4 channels"),
                       ((1, 128, 16, 2048, 2048, 0, 0), b"too large for 32-bit gather offsets")):
        assert lib.rf_conv3x3_plan(*args, 1, 0, *out) == -22 and text in lib.rf_last_error(), args
    assert lib.rf_conv3x3_plan(1, 4, 16, 8, 8, 0, 1, 1, 0, *out) == 0                   # the embedding conv reads the mosaic
    assert lib.rf_conv3x3_plan(1, 8, 16, 8, 8, 0, 0, 1, 0, None, 0, *out[2:]) == -22


def reference(tag, t):
    """float64 result of the case."""
    import torch.nn.functional as F
    y = F.leaky_relu(F.conv2d(t["x"].double(), t["w"].double(), t["bias"].double(), padding=1), 0.2)
    return {"plain": lambda v: v, "unshuffle": R.pixel_unshuffle2, "shuffle": R.pixel_shuffle2}[cases.CONV3X3_CASES[tag][5]](y)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(cases.CONV3X3_CASES))
def test_launch_is_the_recorded_one_and_the_result_is_right_and_unchanged(device, tag):
    from bayer_low_light_image_enhancement_amd import ops
    t, run = cases.conv3x3_case(tag)
    y, census = cases.census(lambda: run(ops, device))
    got = {k: v for k, v in census.items() if k.startswith("conv3x3_kernel")}
    e = float((y.cpu().double() - reference(tag, t)).abs().max())
    digest = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
    print(tag, got, "max-abs error against float64:", e, "sha256:", digest)
    assert got == FIXTURE[tag]["census"], (tag, got, FIXTURE[tag]["census"])
    assert e <= TOL, (tag, e)
    assert digest == FIXTURE[tag]["sha256"], tag


@pytest.mark.gpu
@pytest.mark.parametrize("tag", cases.CONV3X3_SPLIT_STAGES)
def test_split_stage_is_bit_for_bit_the_recorded_one(device, tag):
    _, run = cases.launch_case(tag, device)
    with torch.no_grad():
        y, census = cases.census(run)
    got = {k: v for k, v in census.items() if k.startswith("conv3x3_kernel")}
    assert got == FIXTURE[tag]["census"], (tag, got)
    assert hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest() == FIXTURE[tag]["sha256"], tag
