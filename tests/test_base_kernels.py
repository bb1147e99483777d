"""The kernels of the base RawFormer block (variants 'flca' and 'plain') one by one, through ops.channel_attention,
ops.bayer_luma_chroma, ops.flca_guidance, ops.flca, ops.layernorm2d, ops.dwconv3x3, ops.conv_ffn and ops.transformer_block, against
the float64 restatements of tests/base_ops_ref.py (csrc/rf_attn.hip, rf_attn_mid.hip, rf_block.hip, rf_fused.hip, rf_flca.hip,
rf_pointwise.hip).

Truth and bound (the scheme and the constants of tests/test_mamba.py): e64 = max|hip - ref_f64|, e32 = max|ref_f32 - ref_f64|
(the same restatement in float32 on the same inputs); asserted e64 <= RATIO e32 + FLOOR max|ref_f64| and a finite output.  No
operator has a bound of its own: gelu_fast, fast_sigmoid / fast_tanh and the bf16x3 operands all stay inside it (figures below).
Every GPU case runs twice (torch.equal between the runs), leaves its inputs unchanged and asserts through cases.census that the
kernel class it exists for was launched.  Inputs are synth values by name; weights are uniform in +-sqrt(3 / fan_in).

Condition on the bound (test_bound_sees_every_defect, on the CPU, every case): each defect on the case's list -- a keyword of the
restatement, see tests/base_ops_ref.py -- moves the float64 output by at least 10 x the case's bound.  The lists follow the rules of
``listed`` below, one rule per defect; a rule leaves a defect out only where it cannot show by construction, and says why ("not:").
Every defect is on some list (test_every_defect_is_on_some_list).  An output that a defect makes non-finite counts as moved by
infinity.  A case that exists for a value condition asserts that condition on the float64 reference alone
(test_value_conditions); a case that exists for a branch asserts it from the plan arithmetic (test_cases_reach_their_branches)
and, on the GPU, by census.

Cases
=====
channel attention (B, C, heads, h, w); c = C / heads, P = h w.  attn_mid_kernel runs at C = 64 / 128 with w % 4 == 0 and a head
size that divides 16; everything else takes the depthwise kernel + gram_kernel.
  gram_kernel's loops (C = 16, 2 heads unless named)
    ca_p64          (1,16,2,8,8)       one slab, the fast loop with one step
    ca_p192         (1,16,2,12,16)     three steps: leaves by the `!more1` exit after a reload
    ca_p140         (1,16,2,10,14)     P % 64 != 0: per-lane guarded float4 loads
    ca_p35          (2,16,2,5,7)       P % 4 != 0: scalar loads; B = 2
    ca_p2100        (1,16,2,30,70)     slabs of 768, 768, 564: two fast slabs and a slow last one
    ca_p16384       (1,16,1,128,128)   nslab = 16 at RS = 1: the fold's 16-batch, exactly
    ca_c4_p16384    (1,16,4,128,128)   RS = 10 < nslab = 16: the remainder loop takes two slabs for rs < 6
    ca_p163840_h1   (1,16,1,320,512)   nslab = 20, RS = 1: 16-batch + 4-batch
    ca_p163840_h2   (1,16,2,320,512)   nslab = 20, c = 8, RS = 3: 4-batch + remainder
    ca_p163840_h8   (1,16,8,320,512)   nslab = 20, c = 2, RS = 16: two slabs in the remainder loop for rs < 4
  head sizes (band_of and the fold's RS; P = 64 unless named)
    ca_c2 (1,16,8,8,8: RS 16), ca_c4 (1,16,4,8,8: RS 10), ca_c6 (1,24,4,8,8), ca_c12 (1,24,2,8,8), ca_c24 (1,48,2,8,8),
    ca_c48 (1,96,2,8,8): 16-channel tiles that straddle heads, bands of 2 and 3 k tiles; ca_c64 (1,64,1,6,6: the widest band, w % 4 = 2);
    ca_c8x3 (1,24,3,8,8): the last q tile is partial and takes the slow loop beside a fast tile 0; C % 32 != 0 at 24, 48: the
    zero-padded columns of the bf16x3 fold output, written by the last head
  attn_mid_kernel: cm64_3x20, cm128_3x20 (1,C,8,3,20: one ragged tile, every halo outside the image), cm64_6x72 (1,64,8,6,72: four ragged tiles), cm128_10x136 (2,128,8,10,136: nine tiles, ragged),
    cm64_130x256 (1,64,8,130,256: 132 tiles, per = 2, 66 slabs: rgroups = 3), cm64_b4_130x256 (4,64,8,130,256: 264 workgroups:
    rgroups = 1); the reference of these two on the device in the GPU test
  values, each on gram (1,16,2,8,8) `g_` and attn_mid (1,64,8,6,72) `m_`:
    dead_q, dead_k  every weight and bias that feeds q channel 1 | k channel 1 is zero: the row | column of logits is exactly 0 and
                    (dead_q) the attention row exactly uniform, asserted on the reference
    tiny_q          the depthwise weights and bias of q channel 1 times 1e-14: |q| < 1e-12 with |q|^2 > 1e-36, a normal float32
    T0, T_neg       temperature 0 | -3 in every head;   tl4: temperature of shape [1, heads, 1, 1]
    peaked          temperature 50, k channel 2 a copy of q channel 1 (its depthwise bias + 1e-3): top-to-second logit gap >= 30
    ties            k channel 3 a copy of k channel 2: two equal logits in every row of the head
  not: no_clamp off the dead / tiny cases and clamp_squared off tiny_q (every norm is O(1)); head0_temperature at one head and at
  T0 / T_neg / peaked (one temperature); full_cxc at one head; softmax_over_i, drop_last_slab, drop_tail_64, k_norm_from_q at T0
  (the logits are 0 whatever the Gram sums); drop_tail_64 at P % 64 == 0 and on attn_mid (tiles, not 64-pixel steps); from
  P = 16384 on only drop_last_slab and no_proj_bias are evaluated (the run time of the CPU test; the small cases carry the others)
guidance (B, H, W) -> size | None = ops.bayer_luma_chroma (y, cr, cb at the frame's size)
    gd_2x2 (1,2,2)->(2,2); gd_2x6 (1,2,6)->(1,3); gd_up (2,8,12)->(8,12): LL and the magnitude upscaled by 2; gd_20x28 (2,20,28)->(7,9);
    lc_8x12 (2,8,12)->None; gd_black: zeros, both epsilons rule and y_high is exactly 1e-4; gd_dark: frame in [0, 1e-7];
    gd_negative (2,8,12): image 0 = -image 1, luma < 0 everywhere in image 0: both sides of atomic_max_float; gd_mixed: +-1;
    gd_over: values up to 40; gd_luma_trip2 (64,96,96)->(3,3): 36 blocks on a grid of 32, each image's maximum (0.6 .. 1) in its last pixel;
    gd_haar_trip2 (1,1024,1026)->(8,8): 262656 quads on 1024 x 256 threads; gd_level_trip2 (1,16,16)->(520,512): 266240 outputs
  not: no_luma_eps where the maximum is far above 1e-6; no_mag_eps off gd_black (it moves y_high by 1e-8 / 2 mag); every other
  defect at gd_black (all planes are 0 or constant); batch_max at B = 1 and at gd_dark (every maximum is under the clamp);
  swap_cr_cb at gd_dark and gd_negative (cr = cb = -y to one part in 1e6); align_corners, ll_no_half, no_mag_eps without a resize
  (size None); align_corners at gd_2x2 (LL is one pixel, the chroma planes keep their size); no_far_clamp where nothing is upscaled
flca (B, C, h, w): the spatial gates, the pooled mean and the squeeze-excite gate through ops.flca on a 12 x 20 packed frame
    fl_c8_8x8 (2,8,8,8), fl_c16_6x10 (1,16,6,10: w % 4 = 2), fl_c40_5x7 (1,40,5,7: odd w; a partial channel group at cg = 8),
    fl_1x4, fl_1x2, fl_1x1 (1,8,1,w), fl_c40_36x32 (1,40,36,32: two blocks, the second with 128 live pixels),
    fl_c16_33x31 (1,16,33,31: four blocks of the scalar kernel + 255 pixels), fl_c512 (1,512,4,4: squeeze-excite hidden 64, its
    second channel pass), fl_c264 (1,264,2,6: 8 channels in the second pass), fl_c256_cg32 (4,256,62,126: nblk 16 x 8 groups x 4 =
    512: cg = 32), fl_c40_cg32 (16,40,62,126: a partial second group of 32), fl_c16_nblk113 (1,16,113,255: 113 blocks at nsl = 16:
    the squeeze-excite 8-batch, then one more), fl_c8_nblk7 (1,8,7,255), fl_c8_nblk8 (1,8,8,255: 8 blocks at nsl = 32: no batch)
    values on (2,8,8,8): alpha0, beta0, gamma0; sat40: gate weights scaled until the largest sum is 40 (sigmoid / tanh saturate,
    __expf overflows inside); sum1e-4: largest sum 1e-4 (the cancellation in 1 - 2 rcp); relu_dead: se.1.bias = -2, every hidden
    unit negative before the ReLU on features of mean 0 (everywhere else the features lie in [-0.5, 1.5]: a pooled mean of 0.5 and more);
    fl_sat40_w2 (1,16,6,10), fl_sat40_odd, fl_sum1e-4_odd (1,8,5,7): the same values on the other two kernels
  The squeeze-excite width follows the channel count (flca_hidden: max(8, C / 8)): 8, 33 (C = 264) and 64 are reached, widths 1 and
  4 do not exist in this library.
  not: no_group_left / _right at odd w (one pixel per lane) and at w <= the group; swap_chroma_taps at gamma 0; mean_padded at
  P % block == 0; replicate_pad, no_group_left / _right and swap_chroma_taps at sum1e-4 (they move a gate by 1e-4 at most);
  last_block_unpooled and mean_padded at relu_dead (the gate is sigmoid(se.3.bias) whatever the mean); on the three largest frames
  only last_block_unpooled and no_se3_bias are evaluated (run time of the CPU test)
layernorm2d (B, C, h, w), bias | `_nb` without
    ln_c{16,32,48,64,96,128,192,256,384,512} (1,C,4,6): the register kernel's table; ln_c24 (1,24,4,6: the generic float4 kernel),
    ln_c40_p35 (1,40,5,7: the scalar kernel; the three share one census name, base_ops_ref.layernorm_kernel restates the switch), ln_c32_p35 (2,32,5,7: a table C at P % 4 != 0), ln_c32_nb, ln_c24_nb, ln_c40_p35_nb;
    ln_offset(_nb), ln_outlier0(_nb), ln_flat(_nb) on (1,32,4,6): 30 +- 0.05 | channel 0 = 10, the rest +-0.01 | all channels equal;
    ln_trip2 (64,16,4,2060): 2060 pixel groups of 4 per image, 32 workgroups of 64 groups: a second trip with 12 live groups
  not: eps_outside where the variance is O(0.1) or more (it moves the output by 1e-5 / sigma); both at ln_flat with bias (the
  output is the bias); unbiased_var at ln_flat_nb (the variance is 0)
dwconv3x3 (B, C, h, w), bias and GELU unless named
    dw_8x8 (2,3,8,8: halo<8>), dw_16x12 (1,5,16,12), dw_5x8 (2,3,5,8: halo<4>), dw_5x6 (2,3,5,6: <2, 8>), dw_9x10 (1,2,9,10),
    dw_5x7 (2,3,5,7: <1, 4>), dw_1x1, dw_1x2, dw_1x4 (1,4,1,w); dw_8x8_plain, dw_5x6_plain, dw_5x7_plain (no bias, no GELU),
    dw_8x8_nogelu, dw_5x8_pm6 / dw_5x7_pm6: the input scaled until the largest pre-activation is 6;
    dw_trip2 (1,1016000,4,4): 16388 waves of 62 strips on a grid of 16384: halo<4>'s second trip
  not: no_group_left at w <= 4; no_row_above at h <= rows; no_bias / tanh_gelu without them
conv_ffn (B, C, hidden, h, w): ffn_c16 (1,16,32,5,7), ffn_c64 (2,64,128,8,12), ffn_c32_x4 (1,32,128,6,68)
transformer_block (B, C, heads, h, w)
    tb32_4x64 (1,32,8,4,64: one full tile; attn_front<32> + ffn_fused<32>), tb32_h2_5x68 (1,32,2,5,68: ragged both ways),
    tb32_1x64, tb32_4x4 (a single row | column group), tb32_260x256 (1,32,8,260,256: 260 tiles, four per slab of attn_front),
    tb48_5x68 (ffn_fused8<48>), tb64_6x72 (attn_mid<64>, unfused FFN), tb32_6x10 (w % 4 = 2: gram_kernel, <2, 8>, nothing fused),
    tb32_offset / _outlier0 / _flat (1,32,8,5,68), tb32_lowvar (x in +-0.02: the variance is 13 eps),
    tb64_offset, tb64_outlier0 (1,64,8,6,72), tb128_outlier0 (1,128,8,6,72), tb256_outlier0 (1,256,8,4,8) and tb32_6x10_offset: the same
    frames through the LayerNorm prologue of the 1x1 GEMMs, a shifted single pass whose shift is channel 0 (K = 32 ... 256),
    tb32_x4 (expansion 4: unfused FFN), tb32_pm6 (ffn.depthwise scaled until the largest pre-GELU value is 6: the erf polynomial's
    whole range and GELU's flat tail)
  not: no_seam_row at h <= 4, no_seam_col at w <= 64; unbiased_var at tb32_flat (LN1 gives its bias); eps_outside off tb32_lowvar
  (it moves the output by 1e-5 / sigma; at tb32_offset by 9.9 x the bound); tanh_gelu at the offset and flat frames, whose bound is
  100 x the others': e32 there is the float32 LayerNorm's own cancellation at an offset of 30 | a variance of 0, amplified by
  1 / sqrt(eps); on tb32_260x256 only ln2_of_x and no_seam_col are evaluated (run time of the CPU test)

Measured on the MI355X (one run with -s): per operator, e64 / e32 over the cases and the largest e64 / bound
  channel attention, gram_kernel   0.50 (g_dead_k) .. 2.48 (g_peaked), then 1.85 (g_dead_q); 0.139 of the bound (g_peaked), then 0.079 (ca_c64)
  channel attention, attn_mid      0.62 (cm128_10x136) .. 1.42 (m_dead_k); 0.088 (m_dead_k); the single ragged tile 0.82 / 0.79 and 0.057
  guidance                         0.53 (gd_black) .. 2.83 (gd_2x6: e32 is 4e-8 on 12 pixels), then 1.04; 0.086 (gd_mixed)
  flca                             0.72 (fl_1x1) .. 1.68 (fl_c512); 0.117 (fl_sat40_odd), 0.116 (fl_sat40_w2): fast_sigmoid / fast_tanh
                                   at sums of +-40 stay at an eighth of the bound, at +-1e-4 under 0.05
  layernorm2d                      0.49 (ln_c16) .. 1.55 (ln_c40_p35_nb); 0.125 (ln_flat), 0.124 (ln_offset): the kernels' two-pass
                                   statistics land on the float32 restatement's own error there (e64 / e32 = 1.00)
  dwconv3x3                        0.81 (dw_5x8_pm6) .. 1.64 (dw_5x7), and 5.42 / 5.18 at dw_1x1 / dw_1x2 (four and eight outputs, e32 1e-8:
                                   gelu_fast against erf); 0.058 of the bound (dw_1x2): gelu_fast needs no floor of its own up to +-6
  conv_ffn                         0.71 (ffn_c64) .. 1.50 (ffn_c32_x4); 0.101 (ffn_c32_x4)
  transformer_block                0.53 (tb32_flat) .. 1.84 (tb32_x4) and 0.118 of the bound (tb32_x4, then tb32_6x10_offset 0.116) away from the
                                   channel-0 outlier; the fused kernels with their bf16x3 operands (tb32_*, tb48_5x68) 0.53 .. 1.25 and
                                   at most 0.082 (tb32_offset).  The outlier in channel 0 through the GEMMs' LayerNorm prologue:
                                   5.13, 7.69, 14.7 and 0.239, 0.383, 0.671 of the bound at C = 64, 128, 256 (tb64_ / tb128_ /
                                   tb256_outlier0).  Its single pass shifts by channel 0, here the outlier itself, so the variance
                                   o^2 / K is the difference of two sums near o^2 and loses about K ulp; the fused kernels' LayerNorm
                                   (tb32_outlier0: 1.02) and layernorm2d (0.74) are two-pass and do not.  Still inside the bound at the
                                   largest K that takes the single pass (256); the nearest any case comes.  Since e32 decides how near,
                                   and the CPU's float32 kernels differ between hosts, tb256_outlier0 takes both restatements on the
                                   device, as the large frames do (with the CPU's e32, 9.7e-7 on the recording host, it stood at 0.768).
Every other case lands below a seventh of its bound.  (e32 itself moves between hosts: the CPU's float32 kernels differ.)

What the cases found: no kernel was wrong.  Two entry points refused an unsupported shape only after they had launched kernels:
rf_flca ran the spatial kernel, which writes the output, before launch_flca_se turned away a channel count that is no multiple of 8,
and rf_chan_attn ran the qkv GEMM, the depthwise filter and gram_kernel before launch_attn_fold turned away C % 4 != 0.  Both now
make those checks first (test_rf_flca_and_rf_chan_attn_refuse_before_any_launch).
"""
import ctypes as C
import functools
import math

import pytest
import torch

import base_ops_ref as B
import cases
from bayer_low_light_image_enhancement_amd import _lib
from oracle import rawformer_ref as R

RATIO, FLOOR = 8.0, 2e-6          # tests/test_mamba.py
FACTOR = 10.0
SEED = 6100

CA, GD, FL, LN, DW, FFN, TB = "channel_attention", "guidance", "flca", "layernorm2d", "dwconv3x3", "conv_ffn", "transformer_block"
G_SHAPE, M_SHAPE = (1, 16, 2, 8, 8), (1, 64, 8, 6, 72)
CA_KINDS = ("dead_q", "dead_k", "tiny_q", "T0", "T_neg", "peaked", "ties", "tl4")

# tag: (operator, arguments, kernel classes the census must show)
CASES = {
    # ---- channel attention: (B, C, heads, h, w, kind)
    "ca_p64": (CA, (1, 16, 2, 8, 8, None), ("gram_kernel", "dwconv3x3_halo_kernel<8>")),
    "ca_p192": (CA, (1, 16, 2, 12, 16, None), ("gram_kernel",)),
    "ca_p140": (CA, (1, 16, 2, 10, 14, None), ("gram_kernel", "dwconv3x3_kernel<2, 8>")),
    "ca_p35": (CA, (2, 16, 2, 5, 7, None), ("gram_kernel", "dwconv3x3_kernel<1, 4>")),
    "ca_p2100": (CA, (1, 16, 2, 30, 70, None), ("gram_kernel",)),
    "ca_p16384": (CA, (1, 16, 1, 128, 128, None), ("gram_kernel",)),
    "ca_c4_p16384": (CA, (1, 16, 4, 128, 128, None), ("gram_kernel",)),
    "ca_p163840_h1": (CA, (1, 16, 1, 320, 512, None), ("gram_kernel",)),
    "ca_p163840_h2": (CA, (1, 16, 2, 320, 512, None), ("gram_kernel",)),
    "ca_p163840_h8": (CA, (1, 16, 8, 320, 512, None), ("gram_kernel",)),
    "ca_c2": (CA, (1, 16, 8, 8, 8, None), ("gram_kernel",)),
    "ca_c4": (CA, (1, 16, 4, 8, 8, None), ("gram_kernel",)),
    "ca_c6": (CA, (1, 24, 4, 8, 8, None), ("gram_kernel",)),
    "ca_c12": (CA, (1, 24, 2, 8, 8, None), ("gram_kernel",)),
    "ca_c24": (CA, (1, 48, 2, 8, 8, None), ("gram_kernel",)),
    "ca_c48": (CA, (1, 96, 2, 8, 8, None), ("gram_kernel",)),
    "ca_c64": (CA, (1, 64, 1, 6, 6, None), ("gram_kernel",)),
    "ca_c8x3": (CA, (1, 24, 3, 8, 8, None), ("gram_kernel",)),
    "cm64_6x72": (CA, M_SHAPE + (None,), ("attn_mid_kernel<64>",)),
    "cm128_10x136": (CA, (2, 128, 8, 10, 136, None), ("attn_mid_kernel<128>",)),
    "cm64_3x20": (CA, (1, 64, 8, 3, 20, None), ("attn_mid_kernel<64>",)),
    "cm128_3x20": (CA, (1, 128, 8, 3, 20, None), ("attn_mid_kernel<128>",)),
    "cm64_130x256": (CA, (1, 64, 8, 130, 256, None), ("attn_mid_kernel<64>",)),
    "cm64_b4_130x256": (CA, (4, 64, 8, 130, 256, None), ("attn_mid_kernel<64>",)),
    **{f"g_{k}": (CA, G_SHAPE + (k,), ("gram_kernel",)) for k in CA_KINDS},
    **{f"m_{k}": (CA, M_SHAPE + (k,), ("attn_mid_kernel<64>",)) for k in CA_KINDS},
    # ---- guidance: (B, H, W, size | None, kind)
    "gd_2x2": (GD, (1, 2, 2, (2, 2), None), ("guide_level_kernel",)),
    "gd_2x6": (GD, (1, 2, 6, (1, 3), None), ("guide_level_kernel",)),
    "gd_up": (GD, (2, 8, 12, (8, 12), None), ("guide_level_kernel",)),
    "gd_20x28": (GD, (2, 20, 28, (7, 9), None), ("guide_level_kernel",)),
    "lc_8x12": (GD, (2, 8, 12, None, None), ("guidance_base(3 kernels)",)),
    "gd_black": (GD, (2, 8, 12, (8, 12), "black"), ("guidance_base(3 kernels)",)),
    "gd_dark": (GD, (2, 8, 12, (8, 12), "dark"), ("guidance_base(3 kernels)",)),
    "gd_negative": (GD, (2, 8, 12, (8, 12), "negative"), ("guidance_base(3 kernels)",)),
    "lc_negative": (GD, (2, 8, 12, None, "negative"), ("guidance_base(3 kernels)",)),
    "gd_mixed": (GD, (2, 8, 12, (5, 7), "mixed"), ("guidance_base(3 kernels)",)),
    "gd_over": (GD, (2, 8, 12, (8, 12), "over"), ("guidance_base(3 kernels)",)),
    "gd_luma_trip2": (GD, (64, 96, 96, (3, 3), "max_last"), ("guidance_base(3 kernels)",)),
    "gd_haar_trip2": (GD, (1, 1024, 1026, (8, 8), None), ("guidance_base(3 kernels)",)),
    "gd_level_trip2": (GD, (1, 16, 16, (520, 512), None), ("guide_level_kernel",)),
    # ---- flca: (B, C, h, w, kind)
    "fl_c8_8x8": (FL, (2, 8, 8, 8, None), ("flca_spatial_vec_kernel",)),
    "fl_c16_6x10": (FL, (1, 16, 6, 10, None), ("flca_spatial_vec_kernel<2>",)),
    "fl_c40_5x7": (FL, (1, 40, 5, 7, None), ("flca_spatial_kernel",)),
    "fl_1x4": (FL, (1, 8, 1, 4, None), ("flca_spatial_vec_kernel",)),
    "fl_1x2": (FL, (1, 8, 1, 2, None), ("flca_spatial_vec_kernel<2>",)),
    "fl_1x1": (FL, (1, 8, 1, 1, None), ("flca_spatial_kernel",)),
    "fl_c40_36x32": (FL, (1, 40, 36, 32, None), ("flca_spatial_vec_kernel",)),
    "fl_c16_33x31": (FL, (1, 16, 33, 31, None), ("flca_spatial_kernel",)),
    "fl_c512": (FL, (1, 512, 4, 4, None), ("flca_spatial_vec_kernel",)),
    "fl_c264": (FL, (1, 264, 2, 6, None), ("flca_spatial_vec_kernel<2>",)),
    "fl_c256_cg32": (FL, (4, 256, 62, 126, None), ("flca_spatial_vec_kernel<2>",)),
    "fl_c40_cg32": (FL, (16, 40, 62, 126, None), ("flca_spatial_vec_kernel<2>",)),
    "fl_c16_nblk113": (FL, (1, 16, 113, 255, None), ("flca_spatial_kernel",)),
    "fl_c8_nblk7": (FL, (1, 8, 7, 255, None), ("flca_spatial_kernel",)),
    "fl_c8_nblk8": (FL, (1, 8, 8, 255, None), ("flca_spatial_kernel",)),
    **{f"fl_{k}": (FL, (2, 8, 8, 8, k), ("flca_spatial_vec_kernel",)) for k in ("alpha0", "beta0", "gamma0", "sat40", "sum1e-4", "relu_dead")},
    "fl_sat40_w2": (FL, (1, 16, 6, 10, "sat40"), ("flca_spatial_vec_kernel<2>",)),
    "fl_sat40_odd": (FL, (1, 8, 5, 7, "sat40"), ("flca_spatial_kernel",)),
    "fl_sum1e-4_odd": (FL, (1, 8, 5, 7, "sum1e-4"), ("flca_spatial_kernel",)),
    # ---- layernorm2d: (B, C, h, w, bias, kind)
    **{f"ln_c{c}": (LN, (1, c, 4, 6, True, None), ("layernorm2d_kernel",)) for c in (16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 24)},
    "ln_c40_p35": (LN, (1, 40, 5, 7, True, None), ("layernorm2d_kernel",)),
    "ln_c32_p35": (LN, (2, 32, 5, 7, True, None), ("layernorm2d_kernel",)),
    "ln_c32_nb": (LN, (1, 32, 4, 6, False, None), ("layernorm2d_kernel",)),
    "ln_c24_nb": (LN, (1, 24, 4, 6, False, None), ("layernorm2d_kernel",)),
    "ln_c40_p35_nb": (LN, (1, 40, 5, 7, False, None), ("layernorm2d_kernel",)),
    **{f"ln_{k}{'' if b else '_nb'}": (LN, (1, 32, 4, 6, b, k), ("layernorm2d_kernel",)) for k in ("offset", "outlier0", "flat") for b in (True, False)},
    "ln_trip2": (LN, (64, 16, 4, 2060, True, None), ("layernorm2d_kernel",)),
    # ---- dwconv3x3: (B, C, h, w, bias, gelu, kind)
    "dw_8x8": (DW, (2, 3, 8, 8, True, True, None), ("dwconv3x3_halo_kernel<8>",)),
    "dw_16x12": (DW, (1, 5, 16, 12, True, True, None), ("dwconv3x3_halo_kernel<8>",)),
    "dw_5x8": (DW, (2, 3, 5, 8, True, True, None), ("dwconv3x3_halo_kernel<4>",)),
    "dw_5x6": (DW, (2, 3, 5, 6, True, True, None), ("dwconv3x3_kernel<2, 8>",)),
    "dw_9x10": (DW, (1, 2, 9, 10, True, True, None), ("dwconv3x3_kernel<2, 8>",)),
    "dw_5x7": (DW, (2, 3, 5, 7, True, True, None), ("dwconv3x3_kernel<1, 4>",)),
    "dw_1x1": (DW, (1, 4, 1, 1, True, True, None), ("dwconv3x3_kernel<1, 4>",)),
    "dw_1x2": (DW, (1, 4, 1, 2, True, True, None), ("dwconv3x3_kernel<2, 8>",)),
    "dw_1x4": (DW, (1, 4, 1, 4, True, True, None), ("dwconv3x3_halo_kernel<4>",)),
    "dw_8x8_plain": (DW, (2, 3, 8, 8, False, False, None), ("dwconv3x3_halo_kernel<8>",)),
    "dw_5x6_plain": (DW, (2, 3, 5, 6, False, False, None), ("dwconv3x3_kernel<2, 8>",)),
    "dw_5x7_plain": (DW, (2, 3, 5, 7, False, False, None), ("dwconv3x3_kernel<1, 4>",)),
    "dw_8x8_nogelu": (DW, (2, 3, 8, 8, True, False, None), ("dwconv3x3_halo_kernel<8>",)),
    "dw_5x8_pm6": (DW, (2, 3, 5, 8, True, True, "pm6"), ("dwconv3x3_halo_kernel<4>",)),
    "dw_5x7_pm6": (DW, (2, 3, 5, 7, True, True, "pm6"), ("dwconv3x3_kernel<1, 4>",)),
    "dw_trip2": (DW, (1, 1016000, 4, 4, True, True, None), ("dwconv3x3_halo_kernel<4>",)),
    # ---- conv_ffn: (B, C, hidden, h, w)
    "ffn_c16": (FFN, (1, 16, 32, 5, 7), ("dwconv3x3_kernel<1, 4>",)),
    "ffn_c64": (FFN, (2, 64, 128, 8, 12), ("dwconv3x3_halo_kernel<8>",)),
    "ffn_c32_x4": (FFN, (1, 32, 128, 6, 68), ("dwconv3x3_halo_kernel<4>",)),
    # ---- transformer_block: (B, C, heads, h, w, kind, expansion)
    "tb32_4x64": (TB, (1, 32, 8, 4, 64, None, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")),
    "tb32_h2_5x68": (TB, (1, 32, 2, 5, 68, None, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")),
    "tb32_1x64": (TB, (1, 32, 8, 1, 64, None, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")),
    "tb32_4x4": (TB, (1, 32, 8, 4, 4, None, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")),
    "tb32_260x256": (TB, (1, 32, 8, 260, 256, None, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")),
    "tb48_5x68": (TB, (1, 48, 8, 5, 68, None, 2), ("gram_kernel", "ffn_fused8_kernel<48>")),
    "tb64_6x72": (TB, (1, 64, 8, 6, 72, None, 2), ("attn_mid_kernel<64>", "dwconv3x3_halo_kernel<4>")),
    "tb32_6x10": (TB, (1, 32, 8, 6, 10, None, 2), ("gram_kernel", "dwconv3x3_kernel<2, 8>")),
    **{f"tb32_{k}": (TB, (1, 32, 8, 5, 68, k, 2), ("attn_front_kernel<32>", "ffn_fused_kernel<32>")) for k in ("offset", "outlier0", "flat", "lowvar", "pm6")},
    "tb64_offset": (TB, (1, 64, 8, 6, 72, "offset", 2), ("attn_mid_kernel<64>",)),
    "tb64_outlier0": (TB, (1, 64, 8, 6, 72, "outlier0", 2), ("attn_mid_kernel<64>",)),
    "tb128_outlier0": (TB, (1, 128, 8, 6, 72, "outlier0", 2), ("attn_mid_kernel<128>",)),
    "tb256_outlier0": (TB, (1, 256, 8, 4, 8, "outlier0", 2), ("gram_kernel",)),
    "tb32_6x10_offset": (TB, (1, 32, 8, 6, 10, "offset", 2), ("gram_kernel", "dwconv3x3_kernel<2, 8>")),
    "tb32_x4": (TB, (1, 32, 8, 5, 68, None, 4), ("attn_front_kernel<32>", "dwconv3x3_halo_kernel<4>")),
}
# the float64 and float32 restatements run on the device in the GPU test
BIG = ("ca_p163840_h1", "ca_p163840_h2", "ca_p163840_h8", "cm64_130x256", "cm64_b4_130x256", "tb256_outlier0", "fl_c256_cg32", "fl_c40_cg32", "dw_trip2", "tb32_260x256")
FL_LARGE = ("fl_c256_cg32", "fl_c40_cg32", "fl_c16_nblk113")


def rnd(tag, name, shape, lo=-1.0, hi=1.0):
    return cases.rnd(f"basek.{tag}.{name}", shape, lo, hi, seed=SEED)


def gained(tag, name, shape, fan_in):
    g = math.sqrt(3.0 / fan_in)
    return rnd(tag, name, shape, -g, g)


def attention_params(tag, c, heads, pre=""):
    return {pre + "qkv.weight": gained(tag, pre + "qkv_w", (3 * c, c, 1, 1), c), pre + "qkv.bias": rnd(tag, pre + "qkv_b", (3 * c,), -0.2, 0.2),
            pre + "qkv_dwconv.weight": gained(tag, pre + "dw_w", (3 * c, 1, 3, 3), 9), pre + "qkv_dwconv.bias": rnd(tag, pre + "dw_b", (3 * c,), -0.2, 0.2),
            pre + "temperature": rnd(tag, pre + "T", (heads, 1, 1), 0.5, 2.0),
            pre + "project_out.weight": gained(tag, pre + "po_w", (c, c, 1, 1), c), pre + "project_out.bias": rnd(tag, pre + "po_b", (c,), -0.2, 0.2)}


def ffn_params(tag, c, hid, pre=""):
    return {pre + "pointwise1.weight": gained(tag, pre + "p1_w", (hid, c, 1, 1), c), pre + "pointwise1.bias": rnd(tag, pre + "p1_b", (hid,), -0.2, 0.2),
            pre + "depthwise.weight": gained(tag, pre + "d_w", (hid, 1, 3, 3), 9), pre + "depthwise.bias": rnd(tag, pre + "d_b", (hid,), -0.2, 0.2),
            pre + "pointwise2.weight": gained(tag, pre + "p2_w", (c, hid, 1, 1), hid), pre + "pointwise2.bias": rnd(tag, pre + "p2_b", (c,), -0.2, 0.2)}


CA_KEYS = ("qkv.weight", "qkv.bias", "qkv_dwconv.weight", "qkv_dwconv.bias", "temperature", "project_out.weight", "project_out.bias")
FFN_KEYS = ("pointwise1.weight", "pointwise1.bias", "depthwise.weight", "depthwise.bias", "pointwise2.weight", "pointwise2.bias")
Q1, K1, K2, K3 = 1, 1, 2, 3          # the channels (inside head 0) the value cases of channel attention work on


def _value_frame(kind, tag, shape):
    """x of the LayerNorm / block value cases."""
    if kind == "offset":
        return 30.0 + rnd(tag, "x", shape, -0.05, 0.05)
    if kind == "outlier0":
        x = rnd(tag, "x", shape, -0.01, 0.01)
        x[:, 0] = 10.0
        return x
    if kind == "lowvar":
        return rnd(tag, "x", shape, -0.02, 0.02)
    if kind == "flat":
        return rnd(tag, "x", (shape[0], 1) + tuple(shape[2:])).expand(shape).contiguous()
    return rnd(tag, "x", shape)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(tensors by name: float32 on the CPU or None, keyword arguments that are no tensors)."""
    op, a, _ = CASES[tag]
    if op == CA:
        b, c, heads, h, w, kind = a
        t = {"x": rnd(tag, "x", (b, c, h, w)), **attention_params(tag, c, heads)}
        rows = lambda i: [t[k][i] for k in CA_KEYS[:4]]  # noqa: E731
        if kind == "dead_q":
            for r in rows(Q1):
                r.zero_()
        if kind == "dead_k":
            for r in rows(c + K1):
                r.zero_()
        if kind == "tiny_q":
            t["qkv_dwconv.weight"][Q1] *= 1e-14
            t["qkv_dwconv.bias"][Q1] *= 1e-14
        if kind in ("T0", "T_neg", "peaked"):
            t["temperature"][:] = {"T0": 0.0, "T_neg": -3.0, "peaked": 50.0}[kind]
        if kind == "peaked":
            for k in CA_KEYS[:4]:
                t[k][c + K2] = t[k][Q1]
            t["qkv_dwconv.bias"][c + K2] += 1e-3
        if kind == "ties":
            for k in CA_KEYS[:4]:
                t[k][c + K3] = t[k][c + K2]
        if kind == "tl4":
            t["temperature"] = t["temperature"].reshape(1, heads, 1, 1)
        return t, {"heads": heads}
    if op == GD:
        b, hh, ww, size, kind = a
        x = rnd(tag, "x4", (b, 4, hh, ww), 0.0, 1.0)
        if kind == "black":
            x.zero_()
        if kind == "dark":
            x *= 1e-7
        if kind == "negative":
            x[1] = x[0]
            x[0] = -x[0]
        if kind == "mixed":
            x = 2.0 * x - 1.0
        if kind == "over":
            x *= 40.0
        if kind == "max_last":
            x *= 0.5
            x[:, :, -1, -1] = torch.linspace(0.6, 1.0, b)[:, None]          # a maximum of its own per image
        return {"x4": x}, {"size": size}
    if op == FL:
        b, c, h, w, kind = a
        hid = max(8, c // 8)
        lo, hi = (-1.0, 1.0) if kind == "relu_dead" else (-0.5, 1.5)          # a pooled mean of about 0 | 0.5 and more
        t = {"feat": rnd(tag, "feat", (b, c, h, w), lo, hi), "x4": rnd(tag, "x4", (b, 4, 12, 20), 0.0, 1.0),
             "alpha": rnd(tag, "alpha", (), 0.3, 1.0), "beta": rnd(tag, "beta", (), 0.3, 1.0), "gamma": rnd(tag, "gamma", (), 0.3, 1.0),
             "low_attn.0.weight": gained(tag, "wl", (c, 1, 3, 3), 9), "high_attn.0.weight": gained(tag, "wh", (c, 1, 3, 3), 9),
             "chroma_attn.0.weight": gained(tag, "wc", (c, 2, 3, 3), 18),
             "se.1.weight": gained(tag, "se1", (hid, c, 1, 1), c), "se.1.bias": rnd(tag, "se1b", (hid,), -0.2, 0.2),
             "se.3.weight": gained(tag, "se3", (c, hid, 1, 1), hid), "se.3.bias": rnd(tag, "se3b", (c,), -0.2, 0.2)}
        if kind in ("alpha0", "beta0", "gamma0"):
            t[kind[:-1]].zero_()
        if kind == "relu_dead":
            t["se.1.bias"][:] = -2.0
        if kind in ("sat40", "sum1e-4"):          # scale each gate's weights until its largest sum is 40 | 1e-4, on the float64 reference
            d = {k: v.double() for k, v in t.items()}
            parts = B.flca(d["feat"], B.flca_guidance(d["x4"], (h, w)), d, parts=True)[1]
            want = 40.0 if kind == "sat40" else 1e-4
            for key, s in (("low_attn.0.weight", "s_low"), ("high_attn.0.weight", "s_high"), ("chroma_attn.0.weight", "s_chr")):
                t[key] = (t[key].double() * (want / float(parts[s].abs().max()))).float()
        return t, {}
    if op == LN:
        b, c, h, w, bias, kind = a
        return {"x": _value_frame(kind, tag, (b, c, h, w)), "weight": rnd(tag, "w", (c,), 0.5, 1.5),
                "bias": rnd(tag, "b", (c,), -0.5, 0.5) if bias else None}, {}
    if op == DW:
        b, c, h, w, bias, gelu, kind = a
        t = {"x": rnd(tag, "x", (b, c, h, w), -2.0, 2.0), "weight": gained(tag, "w", (c, 1, 3, 3), 9), "bias": rnd(tag, "b", (c,), -0.5, 0.5) if bias else None}
        if kind == "pm6":
            pre = B.dwconv3x3(t["x"].double(), t["weight"].double(), None)
            t["x"] = (t["x"].double() * ((6.0 - 0.5) / float(pre.abs().max()))).float()      # the bias adds at most 0.5
        return t, {"gelu": gelu}
    if op == FFN:
        b, c, hid, h, w = a
        return {"x": rnd(tag, "x", (b, c, h, w)), **ffn_params(tag, c, hid)}, {}
    b, c, heads, h, w, kind, exp = a
    t = {"x": _value_frame(kind, tag, (b, c, h, w)),
         "norm1.body.weight": rnd(tag, "n1w", (c,), 0.5, 1.5), "norm1.body.bias": rnd(tag, "n1b", (c,), -0.2, 0.2),
         "norm2.body.weight": rnd(tag, "n2w", (c,), 0.5, 1.5), "norm2.body.bias": rnd(tag, "n2b", (c,), -0.2, 0.2),
         **attention_params(tag, c, heads, "attn."), **ffn_params(tag, c, exp * c, "ffn.")}
    if kind == "pm6":
        d = {k: v.double() for k, v in t.items()}
        pre = B.transformer_block(d["x"], d, heads, parts=True)[1]["pre"]
        lin = pre - d["ffn.depthwise.bias"].view(1, -1, 1, 1)
        t["ffn.depthwise.weight"] = (d["ffn.depthwise.weight"] * ((6.0 - 0.2) / float(lin.abs().max()))).float()
    return t, {"heads": heads, "exp": exp}


def restated(op, t, kw, defect=None, parts=False):
    if op == CA:
        return B.channel_attention(t["x"], *(t[k] for k in CA_KEYS), kw["heads"], defect, parts)
    if op == GD:
        if kw["size"] is None:
            return torch.cat(B.bayer_luma_chroma(t["x4"], defect), dim=1)
        return B.flca_guidance(t["x4"], kw["size"], defect)
    if op == FL:
        return B.flca(t["feat"], B.flca_guidance(t["x4"], t["feat"].shape[-2:]), t, defect, parts)
    if op == LN:
        return B.layernorm2d(t["x"], t["weight"], t["bias"], defect=defect)
    if op == DW:
        rows = 4 if (t["x"].shape[-1] % 2 or (t["x"].shape[-1] % 4 == 0 and t["x"].shape[-2] % 8)) else 8
        return B.dwconv3x3(t["x"], t["weight"], t["bias"], kw["gelu"], defect, rows)
    if op == FFN:
        return B.conv_ffn(t["x"], *(t[k] for k in FFN_KEYS), defect, parts)
    return B.transformer_block(t["x"], t, kw["heads"], defect, parts)


def on_hip(op, t, kw):
    from bayer_low_light_image_enhancement_amd import ops
    if op == CA:
        return ops.channel_attention(t["x"], *(t[k] for k in CA_KEYS), kw["heads"])
    if op == GD:
        if kw["size"] is None:
            return torch.cat(ops.bayer_luma_chroma(t["x4"]), dim=1)
        return ops.flca_guidance(t["x4"], kw["size"])
    if op == FL:
        return ops.flca(t["feat"], t["x4"], t)
    if op == LN:
        return ops.layernorm2d(t["x"], t["weight"], t["bias"])
    if op == DW:
        return ops.dwconv3x3(t["x"], t["weight"], t["bias"], gelu=kw["gelu"])
    if op == FFN:
        return ops.conv_ffn(t["x"], *(t[k] for k in FFN_KEYS))
    return ops.transformer_block(t["x"], t, heads=kw["heads"], ffn_expansion_factor=kw["exp"])


def listed(tag):
    """The defects that must show at ``tag``: one rule per defect (the "not:" lines of the module docstring)."""
    op, a, _ = CASES[tag]
    out = []
    if op == CA:
        b, c, heads, h, w, kind = a
        p, gram = h * w, B.attn_path(c, heads, h, w) == "gram"
        rules = {"no_clamp": kind in ("dead_q", "dead_k", "tiny_q"), "clamp_squared": kind == "tiny_q",
                 "head0_temperature": heads > 1 and kind not in ("T0", "T_neg", "peaked"), "softmax_over_i": kind != "T0",
                 "full_cxc": heads > 1, "drop_last_slab": kind != "T0", "drop_tail_64": gram and p % 64 != 0 and kind != "T0",
                 "k_norm_from_q": kind != "T0", "no_proj_bias": True, "replicate_pad": True}
        if p >= 16384:
            rules = {k: v and k in ("drop_last_slab", "no_proj_bias") for k, v in rules.items()}
    elif op == GD:
        b, hh, ww, size, kind = a
        black, resized = kind == "black", size is not None
        up = resized and (size[0] > hh // 2 or size[1] > ww // 2)
        rules = {"no_luma_eps": kind in ("black", "dark", "negative"), "no_mag_eps": black and resized, "g1_only": not black,
                 "swap_cr_cb": not black and kind not in ("dark", "negative"), "batch_max": b > 1 and kind not in ("black", "dark"),
                 "align_corners": resized and not black and tag != "gd_2x2",
                 "no_far_clamp": up and not black, "ll_no_half": resized and not black}
    elif op == FL:
        b, c, h, w, kind = a
        grp, blk = (4 if w % 4 == 0 else 2), B.flca_block(w)
        stencil, pooled = kind != "sum1e-4", kind != "relu_dead"
        rules = {"replicate_pad": stencil, "no_group_left": stencil and w % 2 == 0 and w > grp, "no_group_right": stencil and w % 2 == 0 and w > grp,
                 "tanh_sigmoid": True, "swap_chroma_taps": stencil and kind != "gamma0", "last_block_unpooled": pooled,
                 "mean_padded": pooled and (h * w) % blk != 0, "no_relu": True, "no_se3_bias": True}
        if tag in FL_LARGE:
            rules = {k: v and k in ("last_block_unpooled", "no_se3_bias") for k, v in rules.items()}
    elif op == LN:
        b, c, h, w, bias, kind = a
        flat = kind == "flat"
        rules = {"unbiased_var": not flat, "eps_outside": kind == "offset" or (flat and not bias)}
    elif op == DW:
        b, c, h, w, bias, gelu, kind = a
        rows = 4 if (w % 2 or (w % 4 == 0 and h % 8)) else 8
        rules = {"replicate_pad": True, "no_bias": bias, "tanh_gelu": gelu, "no_group_left": w > 4, "no_row_above": h > rows}
        if tag == "dw_trip2":
            rules = {k: v and k in ("replicate_pad", "no_bias") for k, v in rules.items()}
    elif op == FFN:
        b, c, hid, h, w = a
        rules = {"tanh_gelu": True, "no_seam_row": h > 4, "no_seam_col": w > 64}
    else:
        b, c, heads, h, w, kind, exp = a
        rules = {"unbiased_var": kind != "flat", "eps_outside": kind == "lowvar", "ln2_of_x": True, "no_ffn_residual": True,
                 "tanh_gelu": kind not in ("offset", "flat"), "no_seam_row": h > 4, "no_seam_col": w > 64}
        if tag == "tb32_260x256":
            rules = {k: v and k in ("ln2_of_x", "no_seam_col") for k, v in rules.items()}
    for d in B.DEFECTS[op]:
        if rules[d]:
            out.append(d)
    return tuple(out)


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
        for d in listed(tag) if defects else ():
            m = (restated(op, t64, kw, d) - ref64).abs().max()
            out["moved"][d] = float(m) if bool(torch.isfinite(m)) else math.inf
    return out


@functools.lru_cache(maxsize=None)
def reference(tag):
    """On the CPU, computed once, shared, never changed.  The cases of BIG keep their scalars only."""
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
    """Every restatement without a defect against oracle/rawformer_ref.py in float64, 1e-12 relative to the largest value; dwconv3x3,
    which the oracle has only inside conv_ffn, against torch.nn.functional.conv2d and gelu."""
    def close(a, b):
        assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), float((a - b).abs().max())

    def f64(tag):
        t, kw = inputs(tag)
        return {k: None if v is None else v.double() for k, v in t.items()}, kw

    for tag in ("ca_p35", "ca_c12", "cm64_6x72", "g_tl4"):
        t, kw = f64(tag)
        close(restated(CA, t, kw), R.channel_attention(t["x"], *(t[k] for k in CA_KEYS), kw["heads"]))
    for tag in ("gd_2x6", "gd_up", "gd_20x28", "gd_mixed", "gd_negative", "gd_dark", "gd_black"):
        t, kw = f64(tag)
        planes = R.bayer_luma_chroma(t["x4"])
        close(torch.cat(B.bayer_luma_chroma(t["x4"]), 1), torch.cat(planes, 1))
        close(restated(GD, t, kw), R.flca_guidance(*planes, kw["size"]))
        close(B.bilinear_resize(planes[1], kw["size"]), R.bilinear_resize(planes[1], kw["size"]))
        close(B.bilinear_resize(planes[1], kw["size"]), torch.nn.functional.interpolate(planes[1], kw["size"], mode="bilinear", align_corners=False))
    for tag in ("fl_c8_8x8", "fl_c16_6x10", "fl_c40_5x7", "fl_c40_36x32", "fl_sat40"):
        t, kw = f64(tag)
        close(restated(FL, t, kw), R.flca(t["feat"], *R.bayer_luma_chroma(t["x4"]), t, ""))
    for tag in ("ln_c32", "ln_c32_nb", "ln_c40_p35", "ln_offset", "ln_flat_nb"):
        t, kw = f64(tag)
        close(restated(LN, t, kw), R.layernorm2d(t["x"], t["weight"], t["bias"]))
    for tag in ("dw_5x7", "dw_8x8_plain", "dw_5x8_pm6"):
        t, kw = f64(tag)
        want = torch.nn.functional.conv2d(t["x"], t["weight"], t["bias"], padding=1, groups=t["x"].shape[1])
        close(restated(DW, t, kw), torch.nn.functional.gelu(want) if kw["gelu"] else want)
    for tag in ("ffn_c16", "ffn_c32_x4"):
        t, kw = f64(tag)
        close(restated(FFN, t, kw), R.conv_ffn(t["x"], *(t[k] for k in FFN_KEYS)))
    for tag in ("tb32_h2_5x68", "tb64_6x72", "tb32_x4", "tb32_offset"):
        t, kw = f64(tag)
        close(restated(TB, t, kw), R.transformer_block(t["x"], t, "", kw["heads"]))


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_sees_every_defect(tag):
    c = reference(tag)
    op = CASES[tag][0]
    assert c["max"] > 0
    assert set(c["moved"]) == set(listed(tag)) <= set(B.DEFECTS[op])
    for d, moved in c["moved"].items():
        print(f"[{tag}] {d} moves {moved:.3e} = {moved / max(c['bound'], 1e-300):.1f} x the bound {c['bound']:.3e}")
        assert moved >= FACTOR * c["bound"], f"[{tag}] defect {d} moves the output by {moved:.3e}, under 10 x the bound {c['bound']:.3e}"


def test_every_defect_is_on_some_list():
    for op, names in B.DEFECTS.items():
        seen = {d for tag, (o, _, _) in CASES.items() if o == op for d in listed(tag)}
        assert seen == set(names), (op, set(names) - seen)


def _parts64(tag):
    t, kw = inputs(tag)
    with torch.no_grad():
        return restated(CASES[tag][0], {k: None if v is None else v.double() for k, v in t.items()}, kw, parts=True)


@pytest.mark.parametrize("tag", [t for t, c in CASES.items() if c[0] == CA and c[1][5] is not None])
def test_value_conditions_of_channel_attention(tag):
    b, c, heads, h, w, kind = CASES[tag][1]
    out, p = _parts64(tag)
    hs = c // heads
    if kind == "dead_q":
        assert float(p["nq"][:, 0, Q1].abs().max()) == 0.0 and bool((p["logits"][:, 0, Q1] == 0).all())
        assert bool((p["attn"][:, 0, Q1] == 1.0 / hs).all())
    if kind == "dead_k":
        assert float(p["nk"][:, 0, K1].abs().max()) == 0.0 and bool((p["logits"][:, 0, :, K1] == 0).all())
    if kind == "tiny_q":
        n2 = float(p["nq"][:, 0, Q1].max())
        print(f"{tag}: |q|^2 = {n2:.3e}")
        assert math.sqrt(n2) < 1e-12 and float(p["nq"][:, 0, Q1].min()) > 1e-36
        # the clamp divides by 1e-12, not by the norm: the normalised row is shorter than 1
        assert float((p["logits"][:, 0, Q1].abs().max())) < 2.0 * math.sqrt(n2) / 1e-12
    if kind == "T0":
        assert bool((p["attn"] == 1.0 / hs).all())
    if kind == "T_neg":
        cos = torch.einsum("bhin,bhjn->bhij", p["q"] / p["nq"].sqrt()[..., None], p["k"] / p["nk"].sqrt()[..., None])
        assert bool((inputs(tag)[0]["temperature"] == -3.0).all()) and float((p["logits"] + 3.0 * cos).abs().max()) < 1e-12
        assert float(p["logits"].min()) < 0.0 < float(p["logits"].max()) <= 3.0
        assert torch.equal(p["attn"].argmax(dim=-1), cos.argmin(dim=-1))          # the least similar k row gets the largest weight
    if kind == "peaked":
        top = p["logits"][:, 0, Q1].topk(2, dim=-1)
        gap = float((top.values[:, 0] - top.values[:, 1]).min())
        print(f"{tag}: top-to-second logit gap {gap:.1f}, weight {float(p['attn'][:, 0, Q1, K2].min()):.17f}")
        assert gap >= 30.0 and bool((top.indices[:, 0] == K2).all()) and float(p["attn"][:, 0, Q1, K2].min()) > 1.0 - 1e-12
    if kind == "ties":
        assert torch.equal(p["logits"][:, 0, :, K2], p["logits"][:, 0, :, K3])


@pytest.mark.parametrize("tag", [t for t, c in CASES.items() if c[0] in (GD, FL, DW) and c[1][-1] is not None or c[0] in (LN, TB) and c[1][5] is not None])
def test_value_conditions(tag):
    op, a, _ = CASES[tag]
    t, kw = inputs(tag)
    if op == GD:
        x = t["x4"].double()
        luma = 0.299 * x[:, 0] + 0.587 * 0.5 * (x[:, 1] + x[:, 2]) + 0.114 * x[:, 3]
        top = luma.amax(dim=(1, 2))
        if a[4] == "black":
            ref = restated(GD, {"x4": x}, kw)
            assert float(top.max()) == 0.0 and float((ref[:, 1] - 1e-4).abs().max()) < 1e-18 and bool((ref[:, (0, 2, 3)] == 0).all())
        if a[4] == "dark":
            assert 0.0 < float(top.max()) < 1e-6
        if a[4] == "negative":
            assert float(luma[0].max()) < 0.0 < float(luma[1].min())
        if a[4] == "mixed":
            assert float(luma.amin(dim=(1, 2)).max()) < -0.1 and float(top.min()) > 0.1 and float(x.min()) < -0.9
        if a[4] == "over":
            assert float(x.max()) > 39.0
        if a[4] == "max_last":
            assert bool((luma.flatten(1).argmax(dim=1) == luma[0].numel() - 1).all())
    if op == FL:
        p = _parts64(tag)[1]
        sums = [float(p[s].abs().max()) for s in ("s_low", "s_high", "s_chr")]
        if a[4] == "sat40":
            assert all(abs(s - 40.0) < 1e-3 for s in sums)        # float32 weights: 40 to rounding
        if a[4] == "sum1e-4":
            assert all(abs(s - 1e-4) < 1e-9 for s in sums)
        if a[4] == "relu_dead":
            assert float(p["hid"].max()) == 0.0
    if op in (LN, TB):
        x = t["x"].double()
        var = x.var(dim=1, unbiased=False)
        if a[5] == "lowvar":
            assert 0.0 < float(var.max()) < 20e-5 and float(var.min()) > 5e-5          # about 13 eps

        if a[5] == "flat":
            assert float(var.max()) == 0.0
        if a[5] == "offset":
            assert float(x.mean(dim=1).min()) > 29.9 and float(var.max()) < 2e-3          # uniform +-0.05: 8.3e-4
        if a[5] == "outlier0":
            assert bool((x[:, 0] == 10).all()) and float(x[:, 1:].abs().max()) <= 0.01
    if op in (DW, TB) and a[-2 if op == TB else -1] == "pm6":
        if op == DW:
            pre = B.dwconv3x3(t["x"].double(), t["weight"].double(), t["bias"].double())
        else:
            pre = _parts64(tag)[1]["pre"]
        print(f"{tag}: pre-GELU values in [{float(pre.min()):.2f}, {float(pre.max()):.2f}]")
        assert 5.0 <= float(pre.abs().max()) <= 6.01 and float(pre.min()) < -3.0 and float(pre.max()) > 3.0


def test_cases_reach_their_branches():
    """The plan arithmetic of the kernels' host code, restated in base_ops_ref.py, at the shapes of the cases named for a branch."""
    arg = lambda tag: CASES[tag][1]  # noqa: E731
    # gram_plan's slabs and the fold's loops: for rs < RS the 16-batch takes slabs while sl + 15 RS < nslab, the 4-batch while
    # sl + 3 RS < nslab, the remainder the rest
    def fold_trips(nslab, rs_count):
        trips = []
        for rs in range(rs_count):
            sl, n16, n4, n1 = rs, 0, 0, 0
            while sl + 15 * rs_count < nslab:
                sl, n16 = sl + 16 * rs_count, n16 + 1
            while sl + 3 * rs_count < nslab:
                sl, n4 = sl + 4 * rs_count, n4 + 1
            while sl < nslab:
                sl, n1 = sl + rs_count, n1 + 1
            trips.append((n16, n4, n1))
        return trips

    for tag, nslab, slab in (("ca_p64", 1, 256), ("ca_p192", 1, 256), ("ca_p140", 1, 256), ("ca_p35", 1, 256), ("ca_p2100", 3, 768),
                             ("ca_p16384", 16, 1024), ("ca_c4_p16384", 16, 1024), ("ca_p163840_h1", 20, 8192), ("ca_p163840_h2", 20, 8192),
                             ("ca_p163840_h8", 20, 8192)):
        b, c, heads, h, w, _ = arg(tag)
        assert B.attn_path(c, heads, h, w) == "gram" and B.gram_slabs(h * w) == (nslab, slab), tag
    assert 2100 - 2 * 768 == 564 and 768 % 64 == 0 and 564 % 64 != 0 and 2100 % 4 == 0
    assert 64 % 64 == 0 and 192 // 64 == 3 and 140 % 64 and 140 % 4 == 0 and 35 % 4
    assert [B.fold_rs(c) for c in (2, 4, 8, 16, 64)] == [16, 10, 3, 1, 1]
    assert fold_trips(16, 1) == [(1, 0, 0)]                                        # ca_p16384: the 16-batch, exactly
    assert fold_trips(20, 1) == [(1, 1, 0)]                                        # ca_p163840_h1
    assert fold_trips(20, 3) == [(0, 1, 3), (0, 1, 3), (0, 1, 2)]                  # ca_p163840_h2
    assert fold_trips(20, 16) == [(0, 0, 2)] * 4 + [(0, 0, 1)] * 12                # ca_p163840_h8
    assert fold_trips(16, 10) == [(0, 0, 2)] * 6 + [(0, 0, 1)] * 4                 # ca_c4_p16384
    # band_of per 16-channel q tile (first k tile, k tiles, may take the fast loop) at the head-size cases, all at P = 64 or 36
    for tag in ("ca_c2", "ca_c4", "ca_c6", "ca_c12", "ca_c24", "ca_c48", "ca_c8x3"):
        assert arg(tag)[3] * arg(tag)[4] == 64                                     # float4 loads, one slab of a multiple of 64
    tiles = lambda tag: B.gram_tiles(arg(tag)[1], arg(tag)[2])  # noqa: E731
    assert tiles("ca_c2") == tiles("ca_c4") == [(0, 1, True)]
    assert tiles("ca_c6") == tiles("ca_c12") == [(0, 2, False), (0, 2, False)]      # both tiles straddle heads and reach the partial k tile
    assert tiles("ca_c24") == [(0, 2, True), (0, 3, True), (1, 2, True)]            # tile 1 straddles the two heads
    assert tiles("ca_c48") == [(0, 3, True), (0, 3, True), (0, 3, True), (3, 3, True), (3, 3, True), (3, 3, True)]
    assert tiles("ca_c64") == [(0, 4, True)] * 4 and 36 % 64                        # the widest band, on the slow loop (P = 36)
    assert tiles("ca_c8x3") == [(0, 1, True), (1, 1, False)]                        # a partial last q tile beside a fast tile 0
    assert [32 * -(-c // 32) - c for c in (24, 48)] == [8, 16]                      # zero-padded columns of the bf16x3 fold output
    # launch_layernorm2d's switch under the one census name
    for tag, (op, a, _) in CASES.items():
        if op == LN:
            want = "scalar" if "p35" in tag else "vec4" if "c24" in tag else "reg"
            assert B.layernorm_kernel(a[1], a[2] * a[3]) == want, tag
    # attn_mid_plan: tiles, tiles per slab
    assert B.mid_slabs(3, 20) == (1, 1, 1) and 3 < 4 and 20 < 64                   # cm64_3x20, cm128_3x20: one tile, ragged both ways
    assert B.mid_slabs(6, 72) == (4, 1, 4) and B.mid_slabs(10, 136) == (9, 1, 9) and B.mid_slabs(130, 256) == (66, 2, 132)
    for tag, rgroups in (("cm64_3x20", 3), ("cm128_3x20", 3), ("cm64_6x72", 3), ("cm128_10x136", 3), ("cm64_130x256", 3), ("cm64_b4_130x256", 1)):
        b, c, heads, h, w, _ = arg(tag)
        assert B.attn_path(c, heads, h, w) == "mid" and (3 if B.mid_slabs(h, w)[0] * b < 256 else 1) == rgroups      # launch_attn_mid
    # the restated slab counts against the library's own plans: rf_chan_attn's scratch of one image is a constant of (C, heads), two
    # buffers of 3 C P floats and the slab partials (nslab x C / 16 tiles x 16 rows x 66 floats; the larger of gram_plan's and
    # attn_mid_plan's where attn_mid runs), each rounded up to 64 floats
    lib, sz = _lib.load(), C.c_size_t()
    up64 = lambda n: -(-n // 64) * 64  # noqa: E731

    def rest(c, heads, h, w):
        _lib.check(lib.rf_chan_attn_scratch_bytes(1, c, heads, h, w, C.byref(sz)), "rf_chan_attn_scratch_bytes")
        nslab = B.gram_slabs(h * w)[0]
        if B.attn_path(c, heads, h, w) == "mid":
            nslab = max(nslab, B.mid_slabs(h, w)[0])
        return sz.value - 4 * (2 * up64(3 * c * h * w) + up64(nslab * -(-c // 16) * 16 * 66))

    assert len({rest(16, 2, h, w) for h, w in ((8, 8), (12, 16), (10, 14), (5, 7), (30, 70), (128, 128), (320, 512))}) == 1
    assert len({rest(64, 8, h, w) for h, w in ((6, 72), (130, 256), (6, 6), (30, 70))}) == 1
    # fused_attn_plan: more than 256 tiles of 4 x 64 -> four per slab
    assert -(-260 // 4) * (256 // 64) == 260 > 256
    # guidance: the capped grids
    b, hh, ww = arg("gd_luma_trip2")[:3]
    assert -(-hh * ww // 256) == 36 > max(2048 // b, 32) == 32
    assert (1024 // 2) * (1026 // 2) == 262656 > 1024 * 256
    assert 520 * 512 == 266240 > 1024 * 256
    # FLCA: blocks and channels per workgroup (cg = 32 from nblk ceil(C / 32) B >= 512 on)
    def cg(tag):
        b, c, h, w, _ = arg(tag)
        nblk = -(-h * w // B.flca_block(w))
        return nblk, (8 if nblk * -(-c // 32) * b < 512 else 32)

    assert cg("fl_c256_cg32") == (16, 32) and cg("fl_c40_cg32") == (16, 32) and 40 % 32 == 8
    assert all(cg(t)[1] == 8 for t in CASES if CASES[t][0] == FL and t not in ("fl_c256_cg32", "fl_c40_cg32"))
    assert cg("fl_c40_36x32")[0] == 2 and 36 * 32 - 1024 == 128 and cg("fl_c16_33x31")[0] == 4
    assert cg("fl_c16_nblk113")[0] == 113 and 256 // 16 == 16 and 0 + 7 * 16 < 113      # squeeze-excite: one 8-batch at slice 0
    assert cg("fl_c8_nblk7")[0] == 7 and cg("fl_c8_nblk8")[0] == 8 and 7 * 32 >= 8
    # LayerNorm: ceil(2048 / B) workgroups of 4 x 64 / KS pixel groups (KS = 4 at C = 16)
    b, c, h, w = arg("ln_trip2")[:4]
    assert (h * w) % 4 == 0 and h * w // 4 == 2060 and -(-2048 // b) * 64 == 2048 < 2060
    # depthwise: waves of 62 strips on 16 x 256 blocks of four waves
    b, c, h, w = arg("dw_trip2")[:4]
    assert -(-(b * c * -(-h // 4) * (w // 4)) // 62) == 16388 > 256 * 16 * 4


def test_rf_flca_and_rf_chan_attn_refuse_before_any_launch():
    """Fake addresses.  rf_flca used to run the spatial kernel (which writes `out`) before launch_flca_se turned a channel count
    away, and rf_chan_attn the qkv GEMM, the depthwise filter and gram_kernel before launch_attn_fold did: both make those checks first."""
    lib = _lib.load()
    fake = C.c_void_p(1 << 12)
    prm = (C.c_void_p * 10)(*([1 << 12] * 10))
    for c in (12, 4, 520):
        assert lib.rf_flca(fake, fake, fake, prm, fake, 1, c, 4, 4, None) == -22
        assert f"flca: unsupported shape B=1 C={c} 4x4".encode() in lib.rf_last_error()
    args = [fake] * 10
    assert lib.rf_chan_attn(*args, 1, 6, 1, 4, 4, None) == -22 and b"chan_attn: unsupported shape B=1 C=6 heads=1 4x4" in lib.rf_last_error()
    assert lib.rf_chan_attn(*args, 1, 80, 2, 4, 4, None) == -22 and b"key tiles" in lib.rf_last_error()
    assert lib.rf_chan_attn(*args, 1, 130, 2, 4, 4, None) == -22 and b"head size 65" in lib.rf_last_error()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_kernel_matches_float64(device, tag):
    op, _, kernels = CASES[tag]
    t, kw = inputs(tag)
    c = evaluate(tag, device, defects=False) if tag in BIG else reference(tag)
    td = {k: None if v is None else v.to(device) for k, v in t.items()}
    keep = {k: None if v is None else v.clone() for k, v in td.items()}
    with torch.no_grad():
        got, seen = cases.launches(lambda: on_hip(op, td, kw))
        again = on_hip(op, td, kw)
    assert all(v is None or torch.equal(v, keep[k]) for k, v in td.items()), "an input was written"
    assert torch.equal(got, again), "two runs differ"
    for k in kernels:
        assert seen.get(k, 0) >= 1, f"[{tag}] {k} was not launched: {sorted(seen)}"
    check(tag, got, c)
    if tag == "gd_black":
        assert bool((got[:, (0, 2, 3)] == 0).all())


@pytest.mark.gpu
def test_refusals(device):
    from bayer_low_light_image_enhancement_amd import ops
    z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
    t, _ = inputs("fl_c8_8x8")
    p = {k: v.to(device) for k, v in t.items()}
    with pytest.raises(RuntimeError, match="flca: unsupported shape B=1 C=12 4x4"):
        ops.flca(z(1, 12, 4, 4), z(1, 4, 8, 8), p)
    with pytest.raises(RuntimeError, match="chan_attn: unsupported shape B=1 C=6"):
        ops.channel_attention(z(1, 6, 4, 4), z(18, 6, 1, 1), z(18), z(18, 1, 3, 3), z(18), z(1, 1, 1), z(6, 6, 1, 1), z(6), 1)
