"""The forward kernels of csrc/rf_tokattn.hip, csrc/rf_wfb.hip and csrc/rf_upcat.hip one by one, through ops.token_attention,
ops.luma_film, ops.bayer_luma, ops.dwgate3x3, ops.dwconv5x5 and ops.upsample_cat_reduce, against the float64 restatements of
tests/wfb_ops_ref.py; and ops.wfb_feed_forward / ops.illumination_estimator, which are composed of them.

Truth and bound (the scheme and the constants of tests/test_mamba.py): e64 = max|hip - ref_f64|, e32 = max|ref_f32 - ref_f64|
(the same restatement in float32 on the same inputs); asserted e64 <= RATIO e32 + FLOOR max|ref_f64| and a finite output.  No
operator needed a bound of its own.  Every GPU case runs twice (torch.equal between the runs) and leaves its inputs unchanged.
Inputs are synth values by name (cases.rnd); weights are uniform in +-sqrt(3 / fan_in).

Condition on the bound (test_bound_sees_every_defect, on the CPU, every case): each defect on the case's list -- a keyword of the
restatement, see tests/wfb_ops_ref.py -- moves the float64 output by at least 10 x the case's bound.  A defect is left out of a list
only where it cannot show by construction; the reason stands in the table ("not:").  Every defect is on some list
(test_every_defect_is_on_some_list).  An output that a defect makes non-finite counts as moved by infinity: every case asserts a
finite output.

Cases
=====
token attention (B, heads, d, h, w); N = h w keys in blocks of 64, d in k-sets of 4, DT = 2 tiles of 16 rows above d = 16.  Not:
drop_tail_channels and padded_scale at d % 4 == 0 (unless the case passes a scale, which padded_scale replaces); v_rows_16 at
d <= 16; drop_tail_keys and pad_keys at N % 64 == 0.  At N < 64 drop_tail_keys leaves no key: 0 / 0.
  ta_d1_n1        (1,1,1,1,1)      one key: softmax is 1 whatever the score, so only drop_tail_keys can show
  ta_d2_n15       (2,2,2,3,5)      N < 16: one partly dead query tile; B = 2 and 2 heads: every stride
  ta_d3_n16       (1,3,3,4,4)      N = 16, one whole query tile; scale = 1.0
  ta_d5_n17       (1,2,5,1,17)     a second query tile of one query; a partial second k-set
  ta_d16_n63      (1,2,16,7,9)     d = 16: DT = 1 with every row live; N = 63
  ta_d17_n64      (1,1,17,8,8)     DT = 2 with 15 dead rows; N = 64: one full block and no partial one; float4 V loads
  ta_d31_n65      (2,2,31,5,13)    a partial block of one key; N % 4 != 0: scalar V loads in the full block
  ta_d1_n65       (1,2,1,13,5)     d = 1 with a partial block
  ta_d32_n128     (1,2,32,8,16)    d = 32, two full blocks, float4 V loads; scale = 0.37
  ta_d5_n130      (2,3,5,10,13)    two full blocks and 2 keys; N % 4 != 0; B = 2, 3 heads
  ta_d3_n264      (1,2,3,12,22)    four full blocks and 8 keys, float4 V loads; five workgroups of queries
  ta_d17_n264     (1,2,17,22,12)   the same at DT = 2
  ta_uniform_n65, ta_uniform_n130  (1,2,5,5,13), (1,1,17,10,13), q = 0: the output is the mean of v over exactly N keys (asserted
                                   as such too).  Not: the two defects of the score, which is 0.
  ta_peaked_first, ta_peaked_last  (1,2,32,10,13), q and k of amplitude 8, one key (5 | 128) ahead of every other by more than 150
                                   base-2 logits for every query (test_peaked_cases_are_peaked: 300 and 322; logits up to 478).  The
                                   running sum is rescaled by exp2(-150 or less) at the last block | never.  Not: pad_keys (the copies
                                   are of key 129, whose weight is 0), and drop_tail_keys where the key sits in the first block.
  ta_spread       (1,2,32,10,13)   amplitude 8 and no planted key: base-2 logits beyond +-100 with near ties at the top
luma_film (B, inner, h, w), with luma and alpha | `_plain`: without, which also stays bit-exact against the float32 restatement.
Not: every defect without luma (there is no bias); mean_head at P <= 65536.
  lf_9x14         (2,5,9,14)       alpha 0.8; the shape of tests/test_tokattn.py
  lf_3x3          (1,2,3,3)        alpha -0.6; every pixel is on a border of the pool
  lf_1x1          (1,1,1,1)        alpha 0.8; the pooled value is its own mean, the bias 0: no defect can show
  lf_129x128      (2,1,129,128)    alpha -0.6; P = 16512 > 64 x 256: the FiLM grid's second trip
  lf_257x256      (2,1,257,256)    alpha 0.8; P = 65792: 257 partial sums, luma_mean_kernel's second loop trip.  The frame is bright
                                   with dark rows from 250 on, so that the pixels from 65536 on carry a mean of their own.
bayer_luma (B, H, W), pattern.  Not: range_head at P <= 262144; no_eps wherever max - min is O(0.1) or more (it moves the output by
1e-6 / (max - min), under the bound) -- which includes `bl_two_ranges`: the zero padding makes the top row and left column of any
frame darker than its interior, so image 1 in [0.5, 0.501] has max - min = 0.44, not 0.001.  The narrow range is `bl_dim`.
  bl_18x22_*      (2,18,22)        all four patterns; the frame of tests/test_tokattn.py's shape
  bl_1x1_*        (1,1,1)          every tap but (1, 1) in the padding; luma - min = 0 and the output exactly 0; 0 / 0 without the 1e-6.
                                   Not: swap_rb (the output is 0 whatever the luma)
  bl_2x3_*        (1,2,3)          more border than interior
  bl_two_ranges   (2,16,16) rggb   image 0 in [0, 1], image 1 in [0.5, 0.501]: the statistics are per image
  bl_const        (1,8,8) grbg     0.25 everywhere: a constant interior above a darker border
  bl_dim          (1,16,16) bggr   mosaic in [0, 1e-4]: max - min is 1e-4 and the 1e-6 is 1 % of the divisor
  bl_520x512_*    (1,520,512)      rggb and gbrg; 1040 blocks: the normaliser's second trip; rows 0..511 scaled by 0.8, so the maximum
                                   lies among the pixels from 262144 on
dwgate3x3 (B, C, h, w); x in +-2, both biases unless named.  Not: no_right at w <= 4 (column x0 + 4 is outside); no_row_above at
h <= 4; no_ba without ba.
  dg_1x1 (1,1,1,1), dg_4x4 (1,2,4,4: one item per plane, vector rows), dg_3x6 (1,5,3,6: scalar rows, a dead row in the item)
  dg_5x13*        (2,3,5,13)       scalar rows, partial last group, h % 4 == 1; `_no_ba`, `_no_bb`, `_no_biases`
  dg_9x8*         (2,3,9,8)        vector rows, h % 4 == 1; the same four bias forms
  dg_trip2_scalar (1,2049,4096,1)  2049 x 1024 = 8192 x 256 + 1024 items: the grid-stride second trip, scalar rows
  dg_trip2_vector (1,2049,4096,4)  the same count, vector rows.  x is a per-channel draw plus a per-row draw (+-2); in the GPU test the
                                   float64 and float32 restatements of these two cases and of d5_trip2 run on the device
dwconv5x5 (B, C, h, w), each with bias and `_no_bias`.  Not: no_outer_halo at w <= 4; transposed_taps at 1 x 1 (the centre tap only).
  d5_1x1 (1,1,1,1), d5_2x3 (1,2,2,3), d5_5x13 (2,3,5,13: an odd row, a partial group), d5_9x8 (2,3,9,8), d5_1x9 (1,4,1,9: one row,
  four of five tap rows in the padding), d5_7x2 (1,4,7,2: two columns), d5_trip2 (1,2049,2048,4): 8192 x 256 + 1024 items
upsample_cat_reduce (B, C, h, w), low-resolution size; both biases unless named.  Not: drop_tail_chunk where 2C % 16 == 0 and
C % 8 == 0 (whole chunks); no_up_bias_term without up_b.
  uc_c4           (1,4,1,4)        2 x k-sets and 1 skip k-set: less than one chunk in either phase
  uc_c20*         (2,20,5,4)       10 and 5 k-sets: a partial last chunk in both phases; two channel tiles, 4 live channels in the
                                   second; `_no_up_b`, `_no_cr_b`, `_no_biases`
  uc_c40          (1,40,5,52)      five chunks in each phase (odd); two groups, the last tile of group 1 dead; 260 pixels: a second
                                   pixel tile with one live lane group
  uc_c16          (2,16,16,16)     bf16x3 phase 1 with one K block (the prefetch re-reads); exactly one full pixel tile
  uc_c48*         (1,48,8,12)      bf16x3, three K blocks; the four bias forms
  uc_c128         (1,128,8,8)      bf16x3, eight K blocks, four groups
  uc_c512         (1,512,1,4)      Wc is 256 x 128 x 64 floats = the 8192 x 256 items of the compose grid's first trip: Wb and b' are
                                   written by its second trip alone
composites: ff48 (cases.WFB_FF_CASES: dim 48, hidden 120, 10 x 14; defect: the rep-conv fold left at the identity), ie_3ch (32 middle
channels, 2 x 3 x 9 x 14: the image padded to 4 channels) and ie_4ch (40, 1 x 4 x 10 x 12: no pad); defect: the mean column not folded.

Measured on the MI355X (one run with -s): per operator, e64 / e32 over the cases and the largest e64 / bound
  token attention      0.60 (ta_uniform_n65) .. 1.49 (ta_d3_n264); 0.122 of the bound (ta_d17_n264).  The two peaked cases have e32 = 0:
                       ta_peaked_last is exact, ta_peaked_first is one ulp off (1.2e-7, 0.030 of the floor term)
  luma_film            1.00 .. 1.14 (lf_3x3); 0.041 (lf_129x128)
  bayer_luma           1.00 in every case: with its products kept from contracting the kernel lands on the float32 restatement's own
                       values; 0.066 (bl_two_ranges); the 1 x 1 frames give exactly 0
  dwgate3x3            0.54 (dg_5x13_no_ba) .. 1.88 (dg_5x13_no_biases); 0.061 (dg_trip2_vector)
  dwconv5x5            0.91 (d5_trip2) .. 1.00; 0.053 (d5_trip2)
  upsample_cat_reduce  0.64 (uc_c48) .. 3.16 (uc_c512: each composed weight carries one more rounded sum of 512 terms); 0.208 of the
                       bound (uc_c512), then 0.104 (uc_c128)
  composites           ff48 1.13 and 0.085; ie_3ch / ie_4ch 0.99 / 0.96 and 0.047
No case lands above a quarter of its bound.  (e32 itself moves between hosts: the CPU's float32 kernels differ.)

What the cases found: no kernel was wrong.  ops.token_attention with no channels at all (d = 0) raised ZeroDivisionError from its
default scale d ** -0.5 instead of the library's refusal; it now makes rf_token_attn's head-dimension check itself, first.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import cases
import wfb_ops_ref as W
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

RATIO, FLOOR = 8.0, 2e-6          # tests/test_mamba.py
FACTOR = 10.0                     # test_bound_sees_every_defect of tests/test_wfb_model.py
SEED = 5200
LOG2E = 1.4426950408889634

TA, LF, BL, DG, D5, UC = "token_attention", "luma_film", "bayer_luma", "dwgate3x3", "dwconv5x5", "upsample_cat_reduce"
FF, IE = "feed_forward", "illumination_estimator"
KEYS, PAD, CH, SC, V16 = W.DEFECTS[TA]
ONK, XPAD, MHEAD = W.DEFECTS[LF]
SWAP, NOEPS, RHEAD = W.DEFECTS[BL]
NORIGHT, NOROW, NOBA = W.DEFECTS[DG]
HALO, TRANSP, NOBIAS = W.DEFECTS[D5]
NOUPB, SWAPIJ, TAILCH = W.DEFECTS[UC]

# tag: (operator, arguments, defects that must show); the arguments are spelled out in the module docstring
CASES = {
    # ---- token attention: (B, heads, d, h, w, scale, kind)
    "ta_d1_n1": (TA, (1, 1, 1, 1, 1, None, None), (KEYS,)),
    "ta_d2_n15": (TA, (2, 2, 2, 3, 5, None, None), (KEYS, PAD, CH, SC)),
    "ta_d3_n16": (TA, (1, 3, 3, 4, 4, 1.0, None), (KEYS, PAD, CH, SC)),
    "ta_d5_n17": (TA, (1, 2, 5, 1, 17, None, None), (KEYS, PAD, CH, SC)),
    "ta_d16_n63": (TA, (1, 2, 16, 7, 9, None, None), (KEYS, PAD)),
    "ta_d17_n64": (TA, (1, 1, 17, 8, 8, None, None), (CH, SC, V16)),
    "ta_d31_n65": (TA, (2, 2, 31, 5, 13, None, None), (KEYS, PAD, CH, SC, V16)),
    "ta_d1_n65": (TA, (1, 2, 1, 13, 5, None, None), (KEYS, PAD, CH, SC)),
    "ta_d32_n128": (TA, (1, 2, 32, 8, 16, 0.37, None), (SC, V16)),
    "ta_d5_n130": (TA, (2, 3, 5, 10, 13, None, None), (KEYS, PAD, CH, SC)),
    "ta_d3_n264": (TA, (1, 2, 3, 12, 22, None, None), (KEYS, PAD, CH, SC)),
    "ta_d17_n264": (TA, (1, 2, 17, 22, 12, None, None), (KEYS, PAD, CH, SC, V16)),
    "ta_uniform_n65": (TA, (1, 2, 5, 5, 13, None, "uniform"), (KEYS, PAD)),
    "ta_uniform_n130": (TA, (1, 1, 17, 10, 13, None, "uniform"), (KEYS, PAD, V16)),
    "ta_peaked_first": (TA, (1, 2, 32, 10, 13, None, "peaked_first"), (V16,)),
    "ta_peaked_last": (TA, (1, 2, 32, 10, 13, None, "peaked_last"), (KEYS, V16)),
    "ta_spread": (TA, (1, 2, 32, 10, 13, None, "spread"), (KEYS, PAD, V16)),
    # ---- luma_film: (B, inner, h, w, alpha | None = no luma)
    "lf_9x14": (LF, (2, 5, 9, 14, 0.8), (ONK, XPAD)),
    "lf_9x14_plain": (LF, (2, 5, 9, 14, None), ()),
    "lf_3x3": (LF, (1, 2, 3, 3, -0.6), (ONK, XPAD)),
    "lf_3x3_plain": (LF, (1, 2, 3, 3, None), ()),
    "lf_1x1": (LF, (1, 1, 1, 1, 0.8), ()),
    "lf_1x1_plain": (LF, (1, 1, 1, 1, None), ()),
    "lf_129x128": (LF, (2, 1, 129, 128, -0.6), (ONK, XPAD)),
    "lf_129x128_plain": (LF, (2, 1, 129, 128, None), ()),
    "lf_257x256": (LF, (2, 1, 257, 256, 0.8), (ONK, XPAD, MHEAD)),
    "lf_257x256_plain": (LF, (2, 1, 257, 256, None), ()),
    # ---- bayer_luma: (B, H, W, pattern, kind)
    **{f"bl_18x22_{p}": (BL, (2, 18, 22, p, None), (SWAP,)) for p in ("rggb", "bggr", "grbg", "gbrg")},
    **{f"bl_1x1_{p}": (BL, (1, 1, 1, p, None), (NOEPS,)) for p in ("rggb", "bggr", "grbg", "gbrg")},
    **{f"bl_2x3_{p}": (BL, (1, 2, 3, p, None), (SWAP,)) for p in ("rggb", "bggr", "grbg", "gbrg")},
    "bl_two_ranges": (BL, (2, 16, 16, "rggb", "two_ranges"), (SWAP,)),
    "bl_const": (BL, (1, 8, 8, "grbg", "const"), (SWAP,)),
    "bl_dim": (BL, (1, 16, 16, "bggr", "dim"), (SWAP, NOEPS)),
    "bl_520x512_rggb": (BL, (1, 520, 512, "rggb", "bright_tail"), (SWAP, RHEAD)),
    "bl_520x512_gbrg": (BL, (1, 520, 512, "gbrg", "bright_tail"), (SWAP, RHEAD)),
    # ---- dwgate3x3: (B, C, h, w, ba, bb, second trip)
    "dg_1x1": (DG, (1, 1, 1, 1, True, True, False), (NOBA,)),
    "dg_4x4": (DG, (1, 2, 4, 4, True, True, False), (NOBA,)),
    "dg_5x13": (DG, (2, 3, 5, 13, True, True, False), (NORIGHT, NOROW, NOBA)),
    "dg_5x13_no_ba": (DG, (2, 3, 5, 13, False, True, False), (NORIGHT, NOROW)),
    "dg_5x13_no_bb": (DG, (2, 3, 5, 13, True, False, False), (NORIGHT, NOROW, NOBA)),
    "dg_5x13_no_biases": (DG, (2, 3, 5, 13, False, False, False), (NORIGHT, NOROW)),
    "dg_9x8": (DG, (2, 3, 9, 8, True, True, False), (NORIGHT, NOROW, NOBA)),
    "dg_9x8_no_ba": (DG, (2, 3, 9, 8, False, True, False), (NORIGHT, NOROW)),
    "dg_9x8_no_bb": (DG, (2, 3, 9, 8, True, False, False), (NORIGHT, NOROW, NOBA)),
    "dg_9x8_no_biases": (DG, (2, 3, 9, 8, False, False, False), (NORIGHT, NOROW)),
    "dg_3x6": (DG, (1, 5, 3, 6, True, True, False), (NORIGHT, NOBA)),
    "dg_trip2_scalar": (DG, (1, 2049, 4096, 1, True, True, True), (NOROW, NOBA)),
    "dg_trip2_vector": (DG, (1, 2049, 4096, 4, True, True, True), (NOROW, NOBA)),
    # ---- dwconv5x5: (B, C, h, w, bias, second trip)
    **{f"d5_{h}x{w}{'' if b else '_no_bias'}": (D5, (bb, c, h, w, b, False), tuple(d for d in dd if b or d != NOBIAS))
       for bb, c, h, w, dd in ((1, 1, 1, 1, (NOBIAS,)), (1, 2, 2, 3, (TRANSP, NOBIAS)), (2, 3, 5, 13, (HALO, TRANSP, NOBIAS)),
                               (2, 3, 9, 8, (HALO, TRANSP, NOBIAS)), (1, 4, 1, 9, (HALO, TRANSP, NOBIAS)), (1, 4, 7, 2, (TRANSP, NOBIAS)))
       for b in (True, False)},
    "d5_trip2": (D5, (1, 2049, 2048, 4, True, True), (TRANSP, NOBIAS)),
    # ---- upsample_cat_reduce: (B, C, h, w, up_b, cr_b)
    "uc_c4": (UC, (1, 4, 1, 4, True, True), (NOUPB, SWAPIJ, TAILCH)),
    "uc_c20": (UC, (2, 20, 5, 4, True, True), (NOUPB, SWAPIJ, TAILCH)),
    "uc_c20_no_up_b": (UC, (2, 20, 5, 4, False, True), (SWAPIJ, TAILCH)),
    "uc_c20_no_cr_b": (UC, (2, 20, 5, 4, True, False), (NOUPB, SWAPIJ, TAILCH)),
    "uc_c20_no_biases": (UC, (2, 20, 5, 4, False, False), (SWAPIJ, TAILCH)),
    "uc_c40": (UC, (1, 40, 5, 52, True, True), (NOUPB, SWAPIJ)),
    "uc_c16": (UC, (2, 16, 16, 16, True, True), (NOUPB, SWAPIJ)),
    "uc_c48": (UC, (1, 48, 8, 12, True, True), (NOUPB, SWAPIJ)),
    "uc_c48_no_up_b": (UC, (1, 48, 8, 12, False, True), (SWAPIJ,)),
    "uc_c48_no_cr_b": (UC, (1, 48, 8, 12, True, False), (NOUPB, SWAPIJ)),
    "uc_c48_no_biases": (UC, (1, 48, 8, 12, False, False), (SWAPIJ,)),
    "uc_c128": (UC, (1, 128, 8, 8, True, True), (NOUPB, SWAPIJ)),
    "uc_c512": (UC, (1, 512, 1, 4, True, True), (NOUPB, SWAPIJ)),
    # ---- composites
    "ff48": (FF, cases.WFB_FF_CASES[1], ("fold_identity",)),
    "ie_3ch": (IE, (32, 3, 2, 9, 14), ("no_mean_fold",)),
    "ie_4ch": (IE, (40, 4, 1, 10, 12), ("no_mean_fold",)),
}
BIG = tuple(t for t, c in CASES.items() if c[0] in (DG, D5) and c[1][-1])      # reference on the device in the GPU test
PEAK_KEY = {"peaked_first": 5, "peaked_last": 128}                                # N = 130: blocks 0..63, 64..127, 128..129


def rnd(tag, name, shape, lo=-1.0, hi=1.0):
    return cases.rnd(f"wfbk.{tag}.{name}", shape, lo, hi, seed=SEED)


def gained(tag, name, shape, fan_in):
    g = math.sqrt(3.0 / fan_in)
    return rnd(tag, name, shape, -g, g)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(tensors by name: float32 on the CPU or None, keyword arguments that are no tensors)."""
    op, a, _ = CASES[tag]
    if op == TA:
        b, heads, d, h, w, scale, kind = a
        n = h * w
        amp = 8.0 if kind in ("peaked_first", "peaked_last", "spread") else 2.0
        qkv = rnd(tag, "qkv", (b, 3, heads, d, n), -1.0, 1.0)
        qkv[:, :2] *= amp
        qkv[:, 2] *= 2.0
        if kind == "uniform":
            qkv[:, 0] = 0.0
        if kind in PEAK_KEY:      # every query lies within 8 s [0.75, 1], key PEAK_KEY is 8 s: see test_peaked_cases_are_peaked
            s = torch.sign(rnd(tag, "sign", (1, heads, d, 1)))
            qkv[:, 0] = 8.0 * s * rnd(tag, "u", (b, heads, d, n), 0.75, 1.0)
            qkv[:, 1, :, :, PEAK_KEY[kind]] = 8.0 * s[..., 0]
        return {"qkv": qkv.reshape(b, 3 * heads * d, h, w).contiguous()}, {"heads": heads, "scale": scale}
    if op == LF:
        b, inner, h, w, alpha = a
        t = {"qkv": rnd(tag, "qkv", (b, 3 * inner, h, w)), "gamma": rnd(tag, "g", (b, inner, h, w), 0.5, 1.5),
             "beta": rnd(tag, "b", (b, inner, h, w)), "luma": None, "alpha": None}
        if alpha is not None:
            t["luma"], t["alpha"] = rnd(tag, "l", (b, 1, h, w), 0.0, 1.0), torch.tensor([alpha])
            if h * w > 65536:     # bright frame, dark rows at the bottom: the pixels from 65536 on carry a mean of their own
                t["luma"] = 0.5 + 0.5 * t["luma"]
                t["luma"][:, :, 250:] *= 0.05
        return t, {}
    if op == BL:
        b, hh, ww, pattern, kind = a
        m = rnd(tag.rsplit("_", 1)[0] if kind is None else tag, "mosaic", (b, 1, hh, ww), 0.0, 1.0)
        if kind == "two_ranges":
            m[1] = 0.5 + 0.001 * m[1]
        if kind == "const":
            m[:] = 0.25
        if kind == "dim":
            m *= 1e-4
        if kind == "bright_tail":     # the rows from pixel 262144 on hold the maximum
            m[:, :, :512] *= 0.8
        return {"mosaic": m}, {"pattern": pattern}
    if op == DG:
        b, c, h, w, ba, bb, big = a
        if big:       # a sum of a per-channel and a per-row draw: distinct planes and rows without drawing 33 M values
            x = rnd(tag, "xc", (b, c, 1, w)) + rnd(tag, "xr", (b, 1, h, w))
        else:
            x = rnd(tag, "x", (b, c, h, w), -2.0, 2.0)
        return {"x": x, "wa": gained(tag, "wa", (c, 1, 3, 3), 9), "ba": rnd(tag, "ba", (c,)) if ba else None,
                "wb": gained(tag, "wb", (c, 1, 3, 3), 9), "bb": rnd(tag, "bb", (c,)) if bb else None}, {}
    if op == D5:
        b, c, h, w, bias, big = a
        x = rnd(tag, "xc", (b, c, 1, w)) + rnd(tag, "xr", (b, 1, h, w)) if big else rnd(tag, "x", (b, c, h, w), -2.0, 2.0)
        return {"x": x, "w": gained(tag, "w", (c, 1, 5, 5), 25), "b": rnd(tag, "b", (c,)) if bias else None}, {}
    if op == UC:
        b, c, h, w, ub, cb = a
        return {"x": rnd(tag, "x", (b, 2 * c, h, w)), "skip": rnd(tag, "skip", (b, c, 2 * h, 2 * w)),
                "up_w": gained(tag, "up_w", (2 * c, c, 2, 2), 2 * c), "up_b": rnd(tag, "up_b", (c,)) if ub else None,
                "cr_w": gained(tag, "cr_w", (c, 2 * c, 1, 1), 2 * c), "cr_b": rnd(tag, "cr_b", (c,)) if cb else None}, {}
    if op == FF:
        name, dim, fac, b, h, w = a
        t = {"x": cases.rnd(f"wfb.{name}.x", (b, dim, h, w), seed=51)}
        t.update(cases.params(cases.wfb_ff_spec(dim, fac), seed=800 + dim))
        return t, {}
    mid, ch, b, h, w = a
    spec = dict(cases.wfb_ie_spec(mid))
    spec["conv1.weight"] = (mid, ch + 1, 1, 1)
    t = {"x": rnd(tag, "img", (b, ch, h, w), 0.0, 1.0)}
    t.update(cases.params(spec, seed=SEED + mid))
    return t, {}


def restated(op, t, kw, defect=None):
    if op == TA:
        return W.token_attention(t["qkv"], kw["heads"], kw["scale"], defect)
    if op == LF:
        return W.luma_film(t["qkv"], t["gamma"], t["beta"], t["luma"], t["alpha"], defect)
    if op == BL:
        return W.bayer_luma(t["mosaic"], kw["pattern"], defect)
    if op == DG:
        return W.dwgate3x3(t["x"], t["wa"], t["ba"], t["wb"], t["bb"], defect)
    if op == D5:
        return W.dwconv5x5(t["x"], t["w"], t["b"], defect)
    if op == UC:
        return W.upsample_cat_reduce(t["x"], t["skip"], t["up_w"], t["up_b"], t["cr_w"], t["cr_b"], defect)
    p = {k: v for k, v in t.items() if k != "x"}
    if op == FF:
        return W.feed_forward(t["x"], p, defect)
    return torch.cat(W.illumination_estimator(t["x"], p, defect), dim=1)


def on_hip(op, t, kw):
    from bayer_low_light_image_enhancement_amd import ops
    if op == TA:
        return ops.token_attention(t["qkv"], kw["heads"], kw["scale"])
    if op == LF:
        return ops.luma_film(t["qkv"], t["gamma"], t["beta"], t["luma"], t["alpha"])
    if op == BL:
        return ops.bayer_luma(t["mosaic"], kw["pattern"])
    if op == DG:
        return ops.dwgate3x3(t["x"], t["wa"], t["ba"], t["wb"], t["bb"])
    if op == D5:
        return ops.dwconv5x5(t["x"], t["w"], t["b"])
    if op == UC:
        return ops.upsample_cat_reduce(t["x"], t["skip"], t["up_w"], t["up_b"], t["cr_w"], t["cr_b"])
    p = {k: v for k, v in t.items() if k != "x"}
    if op == FF:
        return ops.wfb_feed_forward(t["x"], p)
    return torch.cat(ops.illumination_estimator(t["x"], p), dim=1)


def evaluate(tag, device="cpu", defects=True):
    """The float64 and float32 restatements on ``device``, the bound, and what each listed defect moves (inf for an output
    that is no longer finite: every case asserts a finite output)."""
    op = CASES[tag][0]
    t, kw = inputs(tag)
    t32 = {k: None if v is None else v.to(device) for k, v in t.items()}
    t64 = {k: None if v is None else v.double() for k, v in t32.items()}
    with torch.no_grad():
        ref64, ref32 = restated(op, t64, kw), restated(op, t32, kw)
        assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and bool(torch.isfinite(ref64).all())
        e32, mx = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
        out = {"ref64": ref64, "ref32": ref32, "e32": e32, "max": mx, "bound": RATIO * e32 + FLOOR * mx, "moved": {}}
        for d in CASES[tag][2] if defects else ():
            m = (restated(op, t64, kw, d) - ref64).abs().max()
            out["moved"][d] = float(m) if bool(torch.isfinite(m)) else math.inf
    return out


@functools.lru_cache(maxsize=None)
def reference(tag):
    """On the CPU, computed once, shared, never changed.  The second-trip cases keep their scalars only."""
    out = evaluate(tag)
    if tag in BIG:
        out["ref64"] = out["ref32"] = None
    return out


def check(tag, got, c):
    got = got.double()
    assert tuple(got.shape) == tuple(c["ref64"].shape)
    assert bool(torch.isfinite(got).all()), f"[{tag}] non-finite output"
    e64 = float((got - c["ref64"].to(got.device)).abs().max())
    bound = c["bound"]
    msg = (f"[{tag}] e64 {e64:.3e} e32 {c['e32']:.3e} max|ref| {c['max']:.3e} | e64/e32 {e64 / c['e32'] if c['e32'] else math.nan:.2f} | "
           f"bound {bound:.3e} ({e64 / max(bound, 1e-300):.3f} of it)")
    print(msg)
    assert e64 <= bound, msg


# ------------------------------------------------------------------------------------------------ no GPU
def test_restatements_match_the_oracle():
    """Each restatement in float32 against the oracle or torch.nn.functional on one case, 1e-6 max-abs."""
    def close(a, b):
        assert a.dtype == b.dtype == torch.float32 and float((a - b).abs().max()) < 1e-6

    t, kw = inputs("ta_d5_n130")
    close(W.token_attention(t["qkv"], kw["heads"]), R.token_attention(t["qkv"], kw["heads"]))
    t, _ = inputs("lf_9x14")
    close(W.luma_film(t["qkv"], t["gamma"], t["beta"], t["luma"], t["alpha"]),
          R.luma_film(t["qkv"], t["gamma"], t["beta"], t["luma"], t["alpha"][0]))
    close(W.luma_film(t["qkv"], t["gamma"], t["beta"], None, None), R.luma_film(t["qkv"], t["gamma"], t["beta"], None, None))
    for p in ("rggb", "bggr", "grbg", "gbrg"):
        t, _ = inputs(f"bl_18x22_{p}")
        close(W.bayer_luma(t["mosaic"], p), R.bayer_luma(t["mosaic"], p))
    t, _ = inputs("dg_5x13")
    a = F.conv2d(t["x"], t["wa"], t["ba"], padding=1, groups=3)
    g = F.conv2d(t["x"], t["wb"], t["bb"], padding=1, groups=3)
    close(W.dwgate3x3(t["x"], t["wa"], t["ba"], t["wb"], t["bb"]), F.gelu(g) * a + F.gelu(a) * g)
    t, _ = inputs("d5_5x13")
    close(W.dwconv5x5(t["x"], t["w"], t["b"]), F.conv2d(t["x"], t["w"], t["b"], padding=2, groups=3))
    t, _ = inputs("uc_c20")
    up = F.conv_transpose2d(t["x"], t["up_w"], t["up_b"], stride=2)
    close(W.upsample_cat_reduce(*(t[k] for k in ("x", "skip", "up_w", "up_b", "cr_w", "cr_b"))),
          F.conv2d(torch.cat((up, t["skip"]), 1), t["cr_w"], t["cr_b"]))
    t, _ = inputs("ie_3ch")
    p = {k: v for k, v in t.items() if k != "x"}
    for a, b in zip(W.illumination_estimator(t["x"], p), R.illumination_estimator(t["x"], p, "")):
        close(a, b)


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_sees_every_defect(tag):
    c = reference(tag)
    op, _, listed = CASES[tag]
    assert c["max"] > 0 or tag.startswith("bl_1x1")                         # a single pixel normalises to 0
    assert set(listed) <= set(W.DEFECTS[op]) and set(c["moved"]) == set(listed)
    for d, moved in c["moved"].items():
        print(f"[{tag}] {d} moves {moved:.3e} = {moved / max(c['bound'], 1e-300):.1f} x the bound {c['bound']:.3e}")
        assert moved >= FACTOR * c["bound"], f"[{tag}] defect {d} moves the output by {moved:.3e}, under 10 x the bound {c['bound']:.3e}"


def test_every_defect_is_on_some_list():
    for op, names in W.DEFECTS.items():
        seen = {d for o, _, ds in CASES.values() if o == op for d in ds}
        assert seen == set(names), (op, set(names) - seen)


def test_cases_reach_the_branches_they_are_named_for():
    items = lambda tag, rows: CASES[tag][1][0] * CASES[tag][1][1] * -(-CASES[tag][1][2] // rows) * -(-CASES[tag][1][3] // 4)  # noqa: E731
    for tag, rows in (("dg_trip2_scalar", 4), ("dg_trip2_vector", 4), ("d5_trip2", 2)):
        assert 8192 * 256 < items(tag, rows) <= 8192 * 256 + 1024, tag       # a second trip, and a short one
    assert CASES["dg_trip2_scalar"][1][3] % 4 and CASES["dg_trip2_vector"][1][3] % 4 == 0
    assert 129 * 128 > 64 * 256 and 257 * 256 > 256 * 256 == 65536              # FiLM's grid of 64; luma_mean_kernel's 256 partial sums
    assert 520 * 512 > 1024 * 256 == 262144                                    # the normaliser's grid of 1024
    lib, sz = _lib.load(), C.c_size_t()
    _lib.check(lib.rf_upcat_scratch_bytes(512, C.byref(sz)), "rf_upcat_scratch_bytes")
    assert 256 * 128 * 64 == 8192 * 256 and sz.value // 4 > 8192 * 256         # Wc fills the compose grid's first trip exactly


@pytest.mark.parametrize("tag", ["ta_peaked_first", "ta_peaked_last", "ta_spread"])
def test_peaked_cases_are_peaked(tag):
    """In base-2 logits the planted key beats every other key of every query by more than 150; `spread` has no such key."""
    (b, heads, d, h, w, _, kind), t = CASES[tag][1], inputs(tag)[0]
    q, k, _ = t["qkv"].double().reshape(b, 3, heads, d, h * w).unbind(1)
    s = torch.einsum("bhdi,bhdj->bhij", q, k) * d ** -0.5 * LOG2E
    if kind == "spread":
        top = s.topk(2, dim=-1).values
        assert float(s.abs().max()) > 100 and float((top[..., 0] - top[..., 1]).min()) < 1.0
        return
    key = PEAK_KEY[kind]
    rest = torch.cat((s[..., :key], s[..., key + 1:]), dim=-1).amax(dim=-1)
    margin = float((s[..., key] - rest).min())
    print(f"{tag}: key {key} leads by {margin:.1f} base-2 logits, the largest logit is {float(s.max()):.1f}")
    assert margin > 150 and (key < 64 if kind == "peaked_first" else key >= 64 * (h * w // 64))


def test_rf_upcat_and_rf_token_attn_refuse_before_any_launch():
    """Fake addresses: rf_upcat makes every check before pack_upcat's first launch (csrc/rf_api.hip), rf_token_attn both of its
    checks before its one launch (csrc/rf_tokattn.hip)."""
    lib = _lib.load()
    fake = C.c_void_p(1 << 12)
    for d in (33, 0):
        assert lib.rf_token_attn(fake, fake, fake, fake, 3 * 64, 64, 1, 1, d, 16, 1.0, None) == -22
        assert f"head dimension {d} not in 1..32".encode() in lib.rf_last_error()
    args = [fake] * 8
    assert lib.rf_upcat(*args, 1, 8, 4, 6, None) == -22 and b"unsupported shape C=8 4x6" in lib.rf_last_error()
    assert lib.rf_upcat(*args, 1, 6, 4, 4, None) == -22 and b"unsupported shape C=6 4x4" in lib.rf_last_error()
    assert lib.rf_upcat(*args, 0, 8, 4, 4, None) == -22 and b"unsupported shape" in lib.rf_last_error()
    assert lib.rf_upcat(fake, C.c_void_p((1 << 12) + 4), *args[2:], 1, 8, 4, 4, None) == -22 and b"unsupported shape" in lib.rf_last_error()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_kernel_matches_float64(device, tag):
    op = CASES[tag][0]
    t, kw = inputs(tag)
    c = evaluate(tag, device, defects=False) if tag in BIG else reference(tag)
    td = {k: None if v is None else v.to(device) for k, v in t.items()}
    keep = {k: None if v is None else v.clone() for k, v in td.items()}
    with torch.no_grad():
        got = on_hip(op, td, kw)
        again = on_hip(op, td, kw)
    assert all(v is None or torch.equal(v, keep[k]) for k, v in td.items()), "an input was written"
    assert torch.equal(got, again), "two runs differ"
    check(tag, got, c)
    if op == LF and t["luma"] is None:        # one multiply and one add per element, each rounded on its own: bit-exact
        assert torch.equal(got.cpu(), c["ref32"])
    if tag.startswith("ta_uniform"):          # the mean of v over exactly N keys
        b, heads, d, h, w = CASES[tag][1][:5]
        mean = t["qkv"].double().reshape(b, 3, heads * d, h * w)[:, 2].mean(dim=-1)
        assert float((got.cpu().double() - mean[:, :, None, None]).abs().max()) <= c["bound"]


@pytest.mark.gpu
def test_refusals(device):
    from bayer_low_light_image_enhancement_amd import ops
    z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
    with pytest.raises(RuntimeError, match="head dimension 33 not in 1..32"):
        ops.token_attention(z(1, 3 * 33, 4, 4), 1)
    with pytest.raises(RuntimeError, match="head dimension 0 not in 1..32"):      # no channels at all
        ops.token_attention(z(1, 0, 4, 4), 1)
    def up(c, h, w):
        return ops.upsample_cat_reduce(z(1, 2 * c, h, w), z(1, c, 2 * h, 2 * w), z(2 * c, c, 2, 2), None, z(c, 2 * c, 1, 1), None)

    with pytest.raises(RuntimeError, match="upcat: unsupported shape C=8 4x6"):
        up(8, 4, 6)
    with pytest.raises(RuntimeError, match="upcat"):
        up(6, 4, 4)
    with pytest.raises(RuntimeError, match="one-channel mosaic"):
        ops.bayer_luma(z(1, 2, 8, 8))
    with pytest.raises(RuntimeError, match="luma_film: gamma/beta"):
        ops.luma_film(z(1, 6, 4, 4), z(1, 2, 4, 5), z(1, 2, 4, 4))
