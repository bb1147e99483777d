"""Exact full-frame sharding on a rows x columns grid of windows: planner, C-ABI argument checks and a
gloo rehearsal of the stitch on the CPU; on the GPU box the ranks are processes on the one GPU (gloo all-reduce of the device
buffers), compared with the CPU oracle's whole-frame forward as tests/test_exact_shard.py does for row shards."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from bayer_low_light_image_enhancement_amd import _lib, tiling

HERE = os.path.dirname(os.path.abspath(__file__))
PLANS = [(1424, 2128, (2, 4), 80), (1424, 2128, (4, 2), 80), (1424, 2128, (1, 8), 80), (128, 512, (1, 2), 80), (256, 256, (2, 2), 80),
         (64, 384, (1, 2), 40), (64, 400, (1, 2), 80), (712, 1064, (3, 3), 40), (64, 64, (1, 2), 80)]


@pytest.mark.parametrize("rows,cols,grid,halo", PLANS)
def test_grid_shards_tile_the_frame_with_full_context_on_four_sides(rows, cols, grid, halo):
    shards = tiling.plan_grid_shards(rows, cols, grid, halo)
    assert len(shards) == grid[0] * grid[1]
    assert len({(s.row.rows, s.col.cols) for s in shards}) == 1                    # one window shape: equal slab grids
    cover = torch.zeros((rows, cols), dtype=torch.int32)
    row_plan = tiling.plan_row_shards(rows, grid[0], halo)
    for i, s in enumerate(shards):
        assert s.row == row_plan[i // grid[1]]                                      # rank order row-major; the row half as it is
        r, c = s.row, s.col
        assert 0 <= r.start and r.start + r.rows <= rows and 0 <= c.start and c.start + c.cols <= cols
        assert r.start + r.y_lo == r.dst and c.start + c.x_lo == c.dst and 0 <= c.x_lo < c.x_hi <= c.cols
        # alignment: rows on 8; column cuts and window origins on 32, the right frame border excepted (x_hi = window width)
        assert r.y_lo % 8 == 0 and r.y_hi % 8 == 0 and r.start % 8 == 0 and r.rows % 8 == 0
        assert c.start % tiling.COL_ALIGN == 0 and c.x_lo % tiling.COL_ALIGN == 0 and c.cols % 8 == 0
        assert c.x_hi % tiling.COL_ALIGN == 0 or (c.x_hi == c.cols and c.start + c.cols == cols)
        # context: `halo` beyond the interior, or the frame border, on each of the four sides
        assert r.y_lo >= halo or r.start == 0
        assert r.rows - r.y_hi >= halo or r.start + r.rows == rows
        assert c.x_lo >= halo or c.start == 0
        assert c.cols - c.x_hi >= halo or c.start + c.cols == cols
        cover[r.dst: r.dst + r.y_hi - r.y_lo, c.dst: c.dst + c.x_hi - c.x_lo] += 1
    assert int(cover.min()) == 1 and int(cover.max()) == 1


def test_column_plan_invariants_over_many_widths():
    g = torch.Generator().manual_seed(3)
    n = 0
    for _ in range(3000):
        cols = 8 * int(torch.randint(4, 400, (1,), generator=g))
        parts = int(torch.randint(1, 10, (1,), generator=g))
        halo = 8 * int(torch.randint(0, 15, (1,), generator=g))
        if cols // tiling.COL_ALIGN < parts:
            with pytest.raises(ValueError):
                tiling.plan_col_shards(cols, parts, halo)
            continue
        cs = tiling.plan_col_shards(cols, parts, halo)
        pos = 0
        for c in cs:
            assert c.dst == pos and c.cols == cs[0].cols and c.start % 32 == 0 and c.x_lo % 32 == 0 and c.start + c.x_lo == c.dst
            assert 0 <= c.start and c.start + c.cols <= cols and c.x_lo < c.x_hi <= c.cols
            assert c.x_hi % 32 == 0 or (c.x_hi == c.cols and c.start + c.cols == cols)
            assert (c.x_lo >= halo or c.start == 0) and (c.cols - c.x_hi >= halo or c.start + c.cols == cols)
            pos += c.x_hi - c.x_lo
        assert pos == cols
        n += 1
    assert n > 1000


def test_grid_windows_at_cfg4_are_smaller_than_row_windows():
    """8 ranks on the 1424 x 2128 packed frame of cfg4.  Row shards: 344 x 2128 = 1.93 x the ideal 1/8 of the frame.  A 2 x 4
    grid by pixel counts: (712 + 80) x (544 + 160) / 378 784 = 1.47; the bound of 1.6 leaves room for the alignment and for the
    row plan, which is plan_row_shards as it is and makes a two-shard window 712 + 2 x 80 rows tall.  The planner returns
    872 x 688 = 1.58."""
    ideal = 1424 * 2128 / 8
    rows = tiling.plan_row_shards(1424, 8)[0].rows * 2128
    assert rows == 344 * 2128
    s = tiling.plan_grid_shards(1424, 2128, (2, 4))[0]
    area = s.row.rows * s.col.cols
    print("grid window", s.row.rows, s.col.cols, area / ideal, "row window", rows / ideal)
    assert area < rows and area / ideal < 1.6


def test_grid_planner_rejects_bad_sizes():
    with pytest.raises(ValueError):
        tiling.plan_grid_shards(64, 100, (1, 2))        # columns not a multiple of 8
    with pytest.raises(ValueError):
        tiling.plan_grid_shards(64, 96, (1, 4))         # fewer than 32 columns per shard
    with pytest.raises(ValueError):
        tiling.plan_grid_shards(16, 512, (4, 2))        # fewer than 8 rows per shard
    with pytest.raises(ValueError):
        tiling.plan_grid_shards(64, 512, (1, 2), halo=12)


def _handle(variant):
    cfg = _lib.RfConfig(16, (C.c_int32 * 4)(8, 8, 8, 8), 1, 3, 2, variant, 1, 0)
    h = C.c_void_p()
    assert _lib.load().rf_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_set_shard_grid_checks_its_arguments_without_a_launch():
    lib = _lib.load()
    cb = _lib.ALLREDUCE_FN(lambda *a: None)
    off = _lib.ALLREDUCE_FN(0)
    h = _handle(_lib.RF_VARIANT_FLCA)
    assert lib.rf_set_shard_grid(h, 0, 64, 64, 96, 288, 384, cb, None) == 0
    assert lib.rf_set_shard_grid(h, 0, 64, 64, 0, 192, 384, cb, None) == 0
    for x_lo, x_hi, total in ((8, 288, 384), (16, 288, 384), (96, 100, 384), (96, 96, 384), (-32, 96, 384), (0, 0, 384), (0, 192, 100),
                              (0, 192, 160)):
        assert lib.rf_set_shard_grid(h, 0, 64, 64, x_lo, x_hi, total, cb, None) == -22, (x_lo, x_hi, total)
        assert b"rf_set_shard_grid" in lib.rf_last_error() and b"columns" in lib.rf_last_error()
    assert lib.rf_set_shard_grid(h, 0, 60, 64, 0, 192, 384, cb, None) == -22 and b"rows" in lib.rf_last_error()
    # the window's width is known to rf_forward only: x_hi beyond it, or inside it off the 32-column grid, is refused before
    # anything else is looked at (no parameters are packed here, nothing is launched)
    assert lib.rf_set_shard_grid(h, 0, 64, 64, 96, 288, 384, cb, None) == 0
    args = (C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 0, 1, 64)
    assert lib.rf_forward(h, *args, 256, 0, None) == -22 and b"columns" in lib.rf_last_error()
    assert lib.rf_set_shard_grid(h, 0, 64, 64, 96, 280, 384, cb, None) == 0      # legal only as the width of a 280-column window
    assert lib.rf_forward(h, *args, 288, 0, None) == -22 and b"columns" in lib.rf_last_error()
    assert lib.rf_forward(h, *args, 280, 0, None) == -2 and b"not packed" in lib.rf_last_error()     # passes the shard checks
    # switching off, and the row entry point as the all-columns case
    assert lib.rf_set_shard_grid(h, 0, 0, 0, 0, 0, 0, off, None) == 0
    assert lib.rf_forward(h, *args, 256, 0, None) == -2
    assert lib.rf_set_shard(h, 0, 64, 64, cb, None) == 0
    assert lib.rf_forward(h, *args, 256, 0, None) == -2
    assert lib.rf_set_shard(h, 0, 0, 0, off, None) == 0
    lib.rf_destroy(h)
    t = _handle(_lib.RF_VARIANT_TRUECOLOR)
    assert lib.rf_set_shard_grid(t, 0, 64, 64, 0, 192, 384, cb, None) == -22 and b"flca and plain" in lib.rf_last_error()
    lib.rf_destroy(t)


# ---- CPU rehearsal of the stitch: two gloo ranks, a stand-in for the model ------------------------------------------
class _Echo:
    """forward_window stand-in: three copies of the window it is given, and a check that every rank got the same shape and the
    bounds of the plan."""

    def __init__(self, shards, rank, frame):
        self.me, self.frame = shards[rank], frame

    def forward_window(self, win, y_lo, y_hi, total_rows, group=None, *, x_lo=0, x_hi=0, total_cols=None):
        r, c = self.me.row, self.me.col
        assert (y_lo, y_hi, x_lo, x_hi) == (r.y_lo, r.y_hi, c.x_lo, c.x_hi) and (2 * total_rows, 2 * total_cols) == self.frame
        assert tuple(win.shape[2:]) == (2 * r.rows, 2 * c.cols)
        return win.repeat(1, 3, 1, 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stitch_worker(rank, world, port, grid, h, w, halo):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.arange(h * w, dtype=torch.float32).reshape(1, 1, h, w)
    shards = tiling.plan_grid_shards(h // 2, w // 2, grid, halo)
    out = tiling.forward_full_frame_exact(_Echo(shards, rank, (h, w)), x, halo=halo, grid=grid)
    assert torch.equal(out, x.repeat(1, 3, 1, 1))
    with pytest.raises(ValueError):
        tiling.forward_full_frame_exact(_Echo(shards, rank, (h, w)), x, halo=halo, grid=(2, 2))      # 4 windows, 2 ranks
    dist.destroy_process_group()


@pytest.mark.parametrize("grid,h,w", [((1, 2), 48, 528), ((2, 1), 160, 80)])
def test_two_rank_stitch_puts_every_interior_in_its_place(grid, h, w):
    """(1, 2) on 264 packed columns: unequal interiors (128 and 136 columns: the second is padded for the all-gather)."""
    mp.spawn(_stitch_worker, args=(2, _free_port(), grid, h, w, 16), nprocs=2, join=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _run_ranks(variant, rows, cols, dim, halo, grid, env=None):
    world = grid[0] * grid[1]
    with tempfile.TemporaryDirectory() as d:
        rdv = os.path.join(d, "rdv")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "grid_shard_worker.py"), str(r), str(world), rdv, str(rows), str(cols),
                                   str(dim), variant, str(halo), str(grid[0]), str(grid[1])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True, env=env)
                 for r in range(world)]
        outs = []
        for r, p in enumerate(procs):
            try:
                o, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            if p.returncode != 0:              # the others wait for this rank in a collective: end them, no second try
                for q in procs:
                    q.kill()
                pytest.fail(f"rank {r} failed:\n{o[-3000:]}")
            outs.append(o)
    return [json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]) for o in outs]


def _check_exact(recs):
    r0 = recs[0]
    for r in recs:
        print(r)
    assert r0["err_vs_oracle"] is not None and r0["err_vs_oracle"] <= 5e-5 * max(r0["scale"], 1.0), r0
    for r in recs:
        assert r["err_vs_hip_whole"] <= 5e-5 * max(r["scale"], 1.0), r
        assert r["err_independent_tiles"] > 20 * r["err_vs_hip_whole"], r          # the statistics, not the context, make it exact


@pytest.mark.gpu
@pytest.mark.parametrize("variant,rows,cols,dim,halo", [("flca", 64, 384, 16, tiling.HALO_ROWS), ("plain", 40, 352, 16, tiling.HALO_ROWS),
                                                         ("flca", 128, 512, 32, tiling.HALO_ROWS), ("flca", 64, 384, 16, 40),
                                                         ("flca", 64, 400, 16, tiling.HALO_ROWS)])
def test_two_windows_side_by_side_match_the_oracle_whole_frame(variant, rows, cols, dim, halo):
    """The row cases of test_exact_shard.py transposed: a column cut crosses attn_front (dim 32, level 0), attn_mid, gram_kernel
    and the FLCA kernels.  The windows are 288, 288, 352 and 256 columns wide, multiples of 32.  The fifth case is a frame whose
    width is not one, like cfg4's 2128: 400 = 12.5 x 32 gives 304-column windows = 38 columns at level 3, where the 4-pixel
    groups of gram_kernel wrap around row ends (its per-pixel column test) and FLCA runs its 2-pixel lanes.

    Measured: 3.0e-6 .. 6.2e-6 to the HIP whole frame at halo 80 (independent tiles 2.5e-2 .. 4.8e-2).  The halo-40 case is not
    the row test's: plan_row_shards gives a two-rank window 2 * halo of one-sided context (80 rows, the whole receptive field),
    the column plan gives what was asked for, rounded up to the alignment: 64 columns, less than the receptive field of 77.  Its
    error is 1.04e-4 against the bound of 1.22e-4 (5e-5 x scale 2.43): inside the tolerance, but context, not summation order."""
    _check_exact(_run_ranks(variant, rows, cols, dim, halo, (1, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("variant,rows,cols,dim", [("flca", 256, 256, 16), ("plain", 256, 256, 16)])
def test_four_windows_two_by_two_match_the_oracle_whole_frame(variant, rows, cols, dim):
    """Four processes on the one GPU; every window has a row cut and a column cut."""
    _check_exact(_run_ranks(variant, rows, cols, dim, tiling.HALO_ROWS, (2, 2)))


@pytest.mark.gpu
def test_too_little_column_context_is_visible():
    """halo 8: windows of 224 columns around interiors of 192, i.e. 32 columns of context after alignment, far inside the
    receptive field of 77: the frame must NOT match (guards the comparison itself against passing vacuously)."""
    recs = _run_ranks("flca", 64, 384, 16, 8, (1, 2))
    print(recs)
    assert max(r["err_vs_hip_whole"] for r in recs) > 1e-4, recs


@pytest.mark.gpu
def test_one_column_of_windows_gives_the_bits_of_the_row_shards():
    recs = _run_ranks("flca", 384, 64, 16, tiling.HALO_ROWS, (2, 1))
    for r in recs:
        assert r["same_bits_as_row_shards"] is True, r
    _check_exact(recs)


@pytest.mark.gpu
def test_single_window_on_rccl_equals_the_whole_frame_bit_for_bit():
    """One rank can initialise the ``nccl`` backend on the one GPU (see test_exact_shard.py): the collectives of the grid path go
    through RCCL and are identities, the interior is the whole window."""
    env = dict(os.environ, RF_SHARD_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0")
    (r,) = _run_ranks("flca", 128, 64, 16, tiling.HALO_ROWS, (1, 1), env=env)
    assert r["err_vs_hip_whole"] == 0.0 and r["same_bits_as_row_shards"] is True, r
    assert r["err_vs_oracle"] <= 5e-5 * max(r["scale"], 1.0), r
