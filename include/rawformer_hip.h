/*
 * rawformer_hip.h -- C ABI of the MI355X (gfx950) RawFormer inference path.
 *
 * This is the drop-in boundary.  The reference is pure
 * Python/PyTorch with no FFI of its own; what a maintainer would bind is the
 * call `pred = model(inp)` in test.py:116 (RawFomer_WFB_FFAB/test.py:78), i.e.
 * `RawFormer.forward` (RawFomer_WFB_FFAB/model.py:473-508 ==
 * FrequencyawareLumaChromaAttentionRAWFormer.py:330-370), plus the operators it
 * is made of.  Every entry point below names the reference function it
 * replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer to float32 unless
 *     the comment says host;
 *   - tensors are NCHW, contiguous;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     calls are asynchronous on it and allocate nothing;
 *   - return value 0 = ok, negative = error (RF_E_*); rf_last_error() gives the
 *     message of the calling thread's last failure;
 *   - a handle is re-entrant across handles, not thread-safe on one handle.
 */
#ifndef RAWFORMER_HIP_H
#define RAWFORMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_OK 0
#define RF_E_INVALID (-22)   /* bad argument / shape          */
#define RF_E_NOMEM (-12)     /* workspace too small           */
#define RF_E_MISSING (-2)    /* a required parameter not set  */
#define RF_E_DEVICE (-5)     /* HIP runtime error             */

#define RF_VARIANT_FLCA 0    /* FrequencyawareLumaChromaAttentionRAWFormer.py:257-278 branch */
#define RF_VARIANT_PLAIN 1   /* conv branch: RawFomer_WFB_FFAB/model.py:393-412, model.py:94-108 */
#define RF_VARIANT_TRUECOLOR 2 /* TrueColorRawFormer, BayerTORGBColorMultiLvl.py:387-462: learned Bayer front end
                                  (EnhancedBayerProcessor), EnhancedFLCA branch, exp(log_temperature) attention, ReLU before
                                  the PixelShuffle, CameraAwareColorCorrection head */
#define RF_VARIANT_MULTILVL 3  /* MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:313-416: FLCA_Pyramid branch (gated
                                  progressive residuals over the Haar pyramid of the luma), per-channel colour anchor and
                                  luminance nudge towards the 2-level LL after the PixelShuffle; forward only */
#define RF_VARIANT_WFB 4       /* RawFomer_WFB_FFAB/model.py:437-508: the plain variant's stage (conv branch + LeakyReLU, I/O
                                  clamps) with WMB (model.py:203-245) as its Transformer: LayerNorm, Haar DWT,
                                  Illumination_Estimator + FFAB on the LL band, WM / Mamba on the high bands, IWT, gated
                                  FeedForward with BatchNorm (eval mode).  `heads` is not read; hidden = dim * ffn_expansion.
                                  Packed H % 16 == 0, H >= 32, W % 32 == 0, dim * 8 <= 512; forward only */

typedef struct rf_handle rf_handle;

typedef struct rf_config {
    int32_t dim;              /* 32 / 48 / 64 (any multiple of 8)                     */
    int32_t heads[4];         /* per U-Net level, reference default {8,8,8,8}         */
    int32_t inp_channels;     /* 1 (Bayer mosaic)                                     */
    int32_t out_channels;     /* 3                                                    */
    int32_t ffn_expansion;    /* 2                                                    */
    int32_t variant;          /* RF_VARIANT_*                                         */
    int32_t branch_lrelu;     /* plain variant: LeakyReLU on the conv branch (WFB) or not (model.py) */
    int32_t clamp_io;         /* clamp input and output to [0,1]: RawFomer_WFB_FFAB/model.py:475,508 */
    int32_t flca_levels;      /* TRUECOLOR, MULTILVL: wavelet pyramid depth of the FLCA branch, 1..3 (reference default 2; 0 = 2) */
} rf_config;

const char* rf_last_error(void);
int rf_version(void);

/* Diagnostic: bracket every kernel launch made by this library between the two calls with
 * HIP events on the launch stream; rf_profile_end writes a JSON array of
 * {kernel, launches, ms, flops, bytes} (algorithmic work per kernel class) into `json`.
 * Single-threaded use only; adds event overhead, so never leave it on in a timed region. */
int rf_profile_begin(void);
int rf_profile_end(char* json, size_t len);

/* ---- whole model: RawFormer.__init__/load_state_dict/forward ------------------------------ */
int rf_create(const rf_config* cfg, rf_handle** out);
void rf_destroy(rf_handle* h);
/* Parameter registry: names are the reference's state_dict keys
 * (FrequencyawareLumaChromaAttentionRAWFormer.py:297-328).  Pointers are borrowed. */
int rf_param_count(const rf_handle* h);
int rf_param_info(const rf_handle* h, int index, const char** name, int64_t shape[4], int* ndim);
int rf_set_param(rf_handle* h, const char* name, const float* dev_ptr, const int64_t* shape, int ndim);
/* What kind of state_dict entry a registry slot is: RF_PARAM_BUFFER = a float32 module buffer (BatchNorm running statistics),
 * not an nn.Parameter; RF_PARAM_UNUSED = the reference registers the tensor and its forward never reads it (RF_VARIANT_WFB:
 * illu.conv2.*, mb.model2.*): it keeps its place in the key order, takes no pointer and rf_set_param refuses it. */
#define RF_PARAM_BUFFER 1
#define RF_PARAM_UNUSED 2
int rf_param_flags(const rf_handle* h, int index, int* flags);
/* Repack the registered weights into MFMA operand order inside caller memory.  Call again
 * whenever a parameter tensor changed. */
int rf_packed_bytes(const rf_handle* h, size_t* bytes);
int rf_pack_params(rf_handle* h, void* packed_dev, size_t bytes, void* stream);
/* H, W are the PACKED sizes (mosaic is 2H x 2W); both must be multiples of 8. */
int rf_workspace_bytes(const rf_handle* h, int B, int H, int W, size_t* bytes);
/* in: mosaic [B, inp_channels, 2H, 2W] (packed_input = 0) or packed [B, 4*inp_channels, H, W];
 * out: [B, out_channels, 2H, 2W].  Replaces RawFormer.forward (test.py:116). */
int rf_forward(rf_handle* h, const float* in, float* out, void* workspace, size_t workspace_bytes,
               int B, int H, int W, int packed_input, void* stream);

/* Exact spatial sharding of ONE frame over several devices (the reference has no counterpart: it
 * runs whole frames on one device, test.py:116).  Each rank runs rf_forward on a WINDOW of the packed frame: its interior
 * rows [y_lo, y_hi) (local row indices, multiples of 8) plus enough halo rows for the U-Net's receptive field (77 packed rows from 8-aligned cuts; tiling.HALO_ROWS = 80)
 * and the same window height on every rank.  What is global in RawFormer -- the channel attention's Gram / norm statistics
 * (FrequencyawareLumaChromaAttentionRAWFormer.py:205-221) and FLCA's squeeze-excite pooling (:150-154) -- is accumulated over the
 * interior rows only and reduced over the ranks through `allreduce(user, buf, n, op, stream)` (n floats, in place, ordered on
 * `stream`: RCCL all-reduce; op 0 = sum, 1 = max) before it is used; FLCA's luma normaliser (the frame maximum, :59-62) is
 * the max over the windows; total_rows is the frame's packed height (the pooled mean's denominator).
 * Interior rows of the output then equal the whole-frame forward up to summation order.  y_lo = y_hi = 0 and a null
 * callback switch sharding off.  Variants flca and plain. */
typedef void (*rf_allreduce_fn)(void* user, float* buf, size_t n, int op, void* stream);
int rf_set_shard(rf_handle* h, int y_lo, int y_hi, int total_rows, rf_allreduce_fn allreduce, void* user);
/* The same on a rows x columns grid of windows: the interior is the rectangle [y_lo, y_hi) x [x_lo, x_hi) of the local window,
 * total_cols the frame's packed width.  x_lo is a multiple of 32 and x_hi a multiple of 32 or the window's width (the frame's
 * right border; checked by rf_forward): at every U-Net level the bounds then fall on the kernels' groups of 4 pixels, which
 * means that window origins are multiples of 32 packed columns too.  The receptive field is the same along both axes, so the
 * halo is the same number of columns.  All ranks run the same window shape.  rf_set_shard is the all-columns case. */
int rf_set_shard_grid(rf_handle* h, int y_lo, int y_hi, int total_rows, int x_lo, int x_hi, int total_cols,
                      rf_allreduce_fn allreduce, void* user);

/* One Conv_Transformer stage of the model, exactly as rf_forward schedules it (branch || TransformerBlock -> cat ->
 * 1x1 -> 3x3 -> LeakyReLU; FrequencyawareLumaChromaAttentionRAWFormer.py:257-278, RawFomer_WFB_FFAB/model.py:393-412,
 * model.py:94-108), including the squeeze-excite fold into channel_reduce.  stage = 1..7 (conv_tran<stage>), at U-Net
 * level l = stage-1 (encoder) or 7-stage (decoder): in/out [B, dim*2^l, H>>l, W>>l]; packed [B,4,H,W] feeds the FLCA
 * guidance, and for RF_VARIANT_TRUECOLOR its front end (EnhancedBayerProcessor with the handle's parameters), which runs first
 * (may be NULL for the plain and wfb variants).  Workspace as for rf_forward(B, H, W). */
int rf_forward_stage(rf_handle* h, int stage, const float* in, const float* packed, float* out, void* workspace,
                     size_t workspace_bytes, int B, int H, int W, void* stream);
/* RF_VARIANT_TRUECOLOR, diagnostic: the front end (EnhancedBayerProcessor, BayerTORGBColorMultiLvl.py:100-134, and the Haar pyramid
 * of its luma) on a packed frame [B,4,H,W] with the handle's parameters, and the seven guidance planes an EnhancedFLCA block sees
 * at U-Net level `level` (0..3), exactly as rf_forward runs them.  Copies out y [B,1,H,W], crcb [B,2,H,W], rgb [B,3,H,W] (the
 * refined rgb) and guide [B,7,H>>level,W>>level] = (y, cr, cb, R, G, y_low, y_high).  Workspace as for rf_forward(B, H, W). */
int rf_tc_guidance(rf_handle* h, const float* packed, int level, float* y, float* crcb, float* rgb, float* guide, void* workspace,
                   size_t workspace_bytes, int B, int H, int W, void* stream);
/* RF_VARIANT_MULTILVL, diagnostic.  rf_ml_guidance: y / cr / cb and the Haar pyramid of a packed frame [B,4,H,W], then the
 * guidance an FLCA_Pyramid block sees at U-Net level `level` (0..3), exactly as rf_forward runs them.  Copies out guide
 * [B,2L+2,H>>level,W>>level] = (y_low_0, y_high_0, .., y_low_{L-1}, y_high_{L-1}, cr, cb) (L = flca_levels) and that level's means
 * table [B,8] as the kernels lay it out: entries 2l and 2l+1 are the means of y_low_l and y_high_l at this size, entry 6 the mean of
 * sqrt(cr^2 + cb^2 + 1e-8); the other entries are not used.
 * rf_ml_tail: the colour anchor and the luminance nudge (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:403-414) in place on
 * image [B,3,2H,2W], from the model input `in` (the mosaic [B,1,2H,2W], or with packed_input the packed frame [B,4,H,W]): the front
 * end on `in`, then the tail as rf_forward runs it.  Both: workspace as for rf_forward(B, H, W), buffers 16-byte aligned. */
int rf_ml_guidance(rf_handle* h, const float* packed, int level, float* guide, float* means, void* workspace, size_t workspace_bytes,
                   int B, int H, int W, void* stream);
int rf_ml_tail(rf_handle* h, float* image, const float* in, int packed_input, void* workspace, size_t workspace_bytes, int B, int H, int W,
               void* stream);

/* ---- training step (reference train.py:127-147: forward, loss, backward; optimiser train.py:113) ----
 * Parameters, gradients and the Adam moments live in FLAT float buffers: parameter i of the registry sits at float offset
 * rf_flat_offset(i) (16-byte aligned), rf_flat_param_floats floats in all.  The host points rf_set_param at views of its flat
 * parameter buffer, all-reduces the flat gradient buffer across ranks (RCCL) and calls rf_adam_step on the three buffers.
 * rf_train_step: in [B,1,2H,2W] mosaic, gt [B,3,2H,2W]; writes grads (flat), *loss_out (device float), optionally the prediction.
 * loss_mode 0: L1 (RawFomer_WFB_FFAB/train.py:124); 1: Charbonnier sqrt(d^2 + eps^2) (train.py:16-25).
 * Adjoint schedule for variants PLAIN and FLCA (no clamp_io); packed W must be a multiple of 32.
 * rf_set_loss_clamp(h, 1): the criterion of train.py:139, loss(clamp(pred, 0, 1), gt).  The seed gradient is multiplied by
 * (0 <= pred <= 1), torch.clamp's subgradient, ends included; pred_out stays the model's output.  With it on, PLAIN models
 * with clamp_io train too: their output clamp (model.py:508) under the criterion's is the same mask and their input clamp
 * (:475) carries no parameter gradient; pred_out is then the clamped output, which is what such a model returns.  Default off. */
int rf_set_loss_clamp(rf_handle* h, int on);
int rf_flat_param_floats(const rf_handle* h, size_t* floats);
int rf_flat_offset(const rf_handle* h, int index, size_t* offset);
int rf_train_workspace_bytes(const rf_handle* h, int B, int H, int W, size_t* bytes);
/* Overlap of the gradient all-reduce with the backward pass (the reference reduces inside backward through nn.DataParallel,
 * train.py:108-111).  The registry -- and so the flat buffer -- is in FORWARD order, the backward finishes modules in reverse
 * order: rf_train_step calls `ready(user, offset, count, stream)` each time the gradients of flat floats [offset, offset + count)
 * are final (their last kernel has been enqueued on `stream`), from the end of the buffer towards its start, every float
 * exactly once.  The host starts its collective for that range behind those kernels.  NULL switches the notifications off.
 * rf_grad_range_count / rf_grad_range: the ranges a step will announce, in announcement order (static per model). */
typedef void (*rf_grad_ready_fn)(void* user, size_t offset, size_t count, void* stream);
int rf_set_grad_ready(rf_handle* h, rf_grad_ready_fn ready, void* user);
int rf_grad_range_count(const rf_handle* h, int* count);
int rf_grad_range(const rf_handle* h, int index, size_t* offset, size_t* count);
int rf_train_step(rf_handle* h, const float* in, const float* gt, float* grads, float* loss_out, float* pred_out, void* workspace,
                  size_t workspace_bytes, int B, int H, int W, int loss_mode, float loss_eps, void* stream);
/* torch.optim.Adam / AdamW (decoupled != 0) on flat buffers; grads are multiplied by grad_scale first (1 / world size). */
int rf_adam_step(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int decoupled, int step, float grad_scale, void* stream);

/* ---- guarded optimiser step (csrc/rf_optim.hip) ----
 * What the reference's loops put around optimizer.step(): torch.cuda.amp.GradScaler.step, which applies NO step when a gradient
 * holds an inf or a NaN (training.py:233,251-253; RawFomer_WFB_FFAB/train.py:139,183-190), and torch.nn.utils.clip_grad_norm_.
 * Every decision is taken on the device: no entry point below reads device memory or waits for the stream (rf_optim_init waits
 * once, for its own copy).  Handle-free; all memory comes from the caller.
 *
 * The gradient buffer is described by nseg SEGMENTS [offset_i, offset_i + count_i) of floats: ascending, disjoint, every offset
 * a multiple of 4 floats (16 bytes) -- for a model, rf_flat_offset(i) and the element count of parameter i.  Floats between
 * segments (alignment gaps) belong to no segment and are never read by the statistics.
 *
 * Device state, one caller-owned buffer of rf_optim_state_bytes(nseg, n) bytes, 16-byte aligned, set up once by rf_optim_init:
 *   byte 0                              rf_optim_control (below)
 *   byte 80                             rf_optim_segment[nseg]: the per-segment results of the last rf_grad_stats
 *   behind them                         the segment -> chunk table, the chunk table and the chunk partials (private)
 * Every later call takes the same nseg, n and state; a state buffer smaller than the query's answer is refused.
 *
 * rf_grad_stats: per segment and in total, the sum of g^2 and the number of non-finite elements (inf or NaN) of the RAW
 *   buffer (no grad_scale).  Squares and sums are float64 (a float32 square is exact there: a finite gradient cannot overflow).
 *   Each segment is cut into chunks of 4096 floats; a chunk is summed by one workgroup in a fixed order, a segment's chunks are
 *   added in chunk order and the segments in a fixed order, whatever the grid: two runs give the same bits.  No float atomics.
 *   Writes rf_optim_segment[], grad_sumsq and nonfinite.  grads is 16-byte aligned.
 * rf_adam_step_guarded: called BEHIND rf_grad_stats on the same buffer and stream.  One workgroup writes the control block:
 *     grad_norm = grad_scale sqrt(grad_sumsq)                        (float64; the norm of segment i is grad_scale sqrt(sumsq_i))
 *     clip_coef = min(1, max_norm / (grad_norm + 1e-6))              (clip_grad_norm_'s formula; 1 with max_norm = +inf and for
 *                                                                     a NaN norm)
 *     skip      = skip_nonfinite && nonfinite > 0
 *     skip: steps_skipped += 1;  else steps_applied += 1 and bias_corr{1,2} = 1 - beta{1,2}^steps_applied, computed in float64
 *     and rounded to float32;  grad_mul = (float)(grad_scale clip_coef)
 *   then rf_adam_step's arithmetic runs element for element with g[i] * grad_mul and the two bias corrections.  On skip nothing is
 *   read or written in params, m and v (no decoupled weight decay either: GradScaler does not call optimizer.step()).  With
 *   skip_nonfinite = 0 a non-finite gradient IS applied and the weights become non-finite, as with rf_adam_step.  grads is
 *   const: clipping happens on the way into the update and the buffer keeps the unclipped gradient.
 * rf_optim_set_steps: sets steps_applied on the stream (resume from a checkpoint); steps_skipped stays.
 * Refusals come before any launch, -22 with an rf_last_error message: null buffers, nseg <= 0, a segment that passes n, starts
 * off a 16-byte boundary or overlaps its predecessor, max_norm <= 0 or NaN, a state buffer that is too small or misaligned. */
typedef struct rf_optim_control {
    double grad_norm;            /*  0  grad_scale * sqrt(grad_sumsq), last rf_adam_step_guarded                   */
    double grad_sumsq;           /*  8  sum of g^2 over all segments, last rf_grad_stats                           */
    double clip_coef;            /* 16                                                                             */
    long long nonfinite;         /* 24  inf / NaN elements over all segments, last rf_grad_stats                   */
    long long steps_applied;     /* 32                                                                             */
    long long steps_skipped;     /* 40                                                                             */
    float bias_corr1, bias_corr2;/* 48, 52  1 - beta^steps_applied of the last applied step                        */
    float grad_mul;              /* 56  what the update multiplies g[i] by                                         */
    int skip;                    /* 60  the last step's decision                                                   */
    long long n;                 /* 64  set by rf_optim_init, with the next two                                    */
    int nseg, nchunks;           /* 72, 76                                                                         */
} rf_optim_control;
typedef struct rf_optim_segment {
    double sumsq;                /* sum of g^2 over the segment  */
    long long nonfinite;         /* its inf / NaN elements       */
} rf_optim_segment;
int rf_optim_state_bytes(int nseg, size_t n, size_t* bytes);
/* offsets, counts: HOST arrays of nseg entries, in floats.  Zeroes the control block (both counters) and the results. */
int rf_optim_init(const size_t* offsets, const size_t* counts, int nseg, size_t n, void* state, size_t state_bytes, void* stream);
int rf_grad_stats(const float* grads, size_t n, int nseg, void* state, size_t state_bytes, void* stream);
int rf_adam_step_guarded(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int decoupled, float grad_scale, float max_norm, int skip_nonfinite, int nseg, void* state,
                         size_t state_bytes, void* stream);
int rf_optim_set_steps(void* state, size_t state_bytes, long long steps_applied, void* stream);

/* ---- operators (parity-test surface) -----------------------------------------------------------
 * Each entry runs the kernels the forward uses for that operator at that shape.  Where the forward
 * fuses ACROSS operators the fused kernel belongs to the wider entry point: rf_chan_attn (no LayerNorm
 * in its contract) takes the depthwise+Gram kernel of levels 1-2 (attn_mid) but not the level-0 kernel
 * that also contains LayerNorm and the qkv 1x1 (attn_front) -- that one, and the fused FFN, are reached
 * through rf_transformer_block. */
/* downshuffle(var, 2): RawFomer_WFB_FFAB/model.py:287-298.  [B,C,2h,2w] -> [B,4C,h,w] */
int rf_pixel_unshuffle2(const float* in, float* out, int B, int C, int h, int w, void* stream);
/* nn.PixelShuffle(2): RawFomer_WFB_FFAB/model.py:471,507.    [B,4C,h,w] -> [B,C,2h,2w] */
int rf_pixel_shuffle2(const float* in, float* out, int B, int C, int h, int w, void* stream);
/* dwt_init / DWT: RawFomer_WFB_FFAB/blocks.py:102-115.       [B,C,2h,2w] -> [4B,C,h,w] (LL,HL,LH,HH) */
int rf_dwt_haar(const float* in, float* out, int B, int C, int h, int w, void* stream);
/* iwt_init / IWT: RawFomer_WFB_FFAB/blocks.py:119-136.       [4B,C,h,w] -> [B,C,2h,2w] */
int rf_idwt_haar(const float* in, float* out, int B, int C, int h, int w, void* stream);
/* CustomDWT: README.md:92-117.  k16 = HOST pointer to the 4x4 kernel, row-major; norm!=0 halves it.
 * [B,C,2h,2w] -> [B,4C,h,w], sub-band-major channels. */
int rf_dwt_custom(const float* in, float* out, const float* k16, int norm, int B, int C, int h, int w, void* stream);
/* CustomIDWT: README.md:120-144.  [B,4C,h,w] -> [B,C,2h,2w] */
int rf_idwt_custom(const float* in, float* out, const float* k16, int norm, int B, int C, int h, int w, void* stream);
/* HaarDWT: FrequencyawareLumaChromaAttentionRAWFormer.py:39-73 (odd sizes reflect-padded).
 * [B,C,hin,win] -> out[4][B,C,ceil(hin/2),ceil(win/2)] in the order LL, LH, HL, HH. */
int rf_haar_dwt(const float* in, float* out, int B, int C, int hin, int win, void* stream);
/* LayerNorm over channels: FrequencyawareLumaChromaAttentionRAWFormer.py:180-187;
 * bias == NULL selects BiasFree_LayerNorm (RawFomer_WFB_FFAB/model.py:89-103). */
int rf_layernorm2d(const float* in, float* out, const float* weight, const float* bias, float eps,
                   int B, int C, int h, int w, void* stream);
/* nn.Conv2d(Cin, Cout, 1) with raw [Cout,Cin] weights; scratch holds the repacked weights
 * (rf_conv1x1_scratch_bytes).  Optional fused LayerNorm prologue (ln_w != NULL), residual add
 * (res != NULL) and a second input (in2, C2 channels, concatenated after the first). */
int rf_conv1x1_scratch_bytes(int Cin_total, int Cout, size_t* bytes);
int rf_conv1x1(const float* in, const float* in2, float* out, const float* weight, const float* bias,
               const float* ln_w, const float* ln_b, const float* res, void* scratch,
               int B, int C1, int C2, int Cout, int h, int w, void* stream);
/* Host only, no launch: the workgroup order of the 1x1 GEMM whose output groups share their input.  A launch of `units`
 * pixel tiles x `ngroups` groups has *ids workgroups (whole chunks of 8 units); workgroup `id` works on (*unit, *group), or on
 * nothing (*unit = *group = -1: padding of the last chunk).  All groups of a unit have ids 8 apart. */
int rf_conv1x1_group_grid(int units, int ngroups, int* ids);
int rf_conv1x1_group_map(int units, int ngroups, int id, int* unit, int* group);
/* nn.Conv2d(C, C, 3, padding=1, groups=C) (+bias), optional exact GELU: conv_ffn middle
 * (RawFomer_WFB_FFAB/model.py:326-334). */
int rf_dwconv3x3(const float* in, float* out, const float* weight, const float* bias, int gelu,
                 int B, int C, int h, int w, void* stream);
/* nn.Conv2d(Cin, Cout, 3, padding=1) with raw [Cout,Cin,3,3] weights.
 * act: 0 none, 1 LeakyReLU(0.2), 2 ReLU (LumaCond, Attenblock.py:148-153).  store: 0 plain, 1 pixel-unshuffle (Downsample,
 * RawFomer_WFB_FFAB/model.py:300-307), 2 pixel-shuffle (conv_out + PixelShuffle, :505-507). */
int rf_conv3x3_scratch_bytes(int Cin, int Cout, size_t* bytes);
int rf_conv3x3(const float* in, float* out, const float* weight, const float* bias, void* scratch,
               int act, int store, int B, int Cin, int Cout, int h, int w, void* stream);
/* Host only, no launch, no GPU needed: what a dense 3x3 convolution of these sizes launches.  store as for rf_conv3x3;
 * unshuffle_in: the input is read through the Bayer pack (Cin = 4, the embedding conv of the forward pass); aligned: input, output
 * and split scratch are 16-byte aligned, as rf_conv3x3's always are (0: none is: scalar stores, no level-0 path, no split; the
 * batch strides Cin h w / Cout h w follow from the sizes); ks_floats: floats of scratch for the input-channel split of small
 * launches (0: none, as in rf_conv3x3; the forward pass has 4096 + 8 B Cout h w where B h w <= 16384).  key: the kernel
 * instantiation (= its profiler key; a split launch keeps the key of the unsplit kernel), grid[3] with grid[2] = *ksplit, the
 * workgroups that share a tile's input channels (1: no split), block, and *level0: the level-0 path (resident weights, input
 * staged by row segments) is taken.  Refuses what rf_conv3x3 refuses. */
int rf_conv3x3_plan(int B, int Cin, int Cout, int h, int w, int store, int unshuffle_in, int aligned, size_t ks_floats,
                    char* key, size_t key_len, int* grid, int* block, int* ksplit, int* level0);
/* nn.ConvTranspose2d(Cin, Cout, 2, stride=2) with raw [Cin,Cout,2,2] weights
 * (RawFomer_WFB_FFAB/model.py:461).  [B,Cin,h,w] -> [B,Cout,2h,2w] */
int rf_convT2x2_scratch_bytes(int Cin, int Cout, size_t* bytes);
int rf_convT2x2(const float* in, float* out, const float* weight, const float* bias, void* scratch,
                int B, int Cin, int Cout, int h, int w, void* stream);
/* Host only, no launch, no GPU needed: what rf_conv1x1 (transposed == 0: b3_weights = 1) or rf_convT2x2 (transposed != 0: C1 = Cin,
 * C2 = ln = res = b3_weights = 0) launches for these sizes with 16-byte aligned dense operands; ln / res: a LayerNorm prologue /
 * a residual is present; b3_weights = 0 plans as the internal callers without bf16x3 weights do.  key: the kernel instantiation
 * (= its profiler key), grid[3], block and dynamic LDS bytes of the launch; *ln_single_pass: the LayerNorm prologue would read the
 * input once (the schedules run LayerNorm as its own pass where it would not). */
int rf_conv1x1_plan(int B, int C1, int C2, int Cout, int h, int w, int ln, int res, int transposed, int b3_weights,
                    char* key, size_t key_len, int* grid, int* block, size_t* lds_bytes, int* ln_single_pass);
/* The same for the GEMM that closes a Conv_Transformer stage where pointwise2 is composed into channel_reduce: three sources
 * [xs (C) ; x1 (C) ; hidden (hc)] -> C channels of B images of h x w, asked WITH the descriptor that lets the GEMM apply the FFN's
 * depthwise 3x3 + GELU to the hidden source as it reads.  *on_the_fly: the plan takes that form (the stage then launches no
 * depthwise convolution); otherwise key / grid / block are those of the GEMM over the finished hidden tensor. */
int rf_conv1x1_dw3_plan(int B, int C, int hc, int h, int w, char* key, size_t key_len, int* grid, int* block, int* on_the_fly);
/* Attention.forward: FrequencyawareLumaChromaAttentionRAWFormer.py:212-235.
 * Takes the 6 raw parameter tensors; scratch from rf_chan_attn_scratch_bytes. */
int rf_chan_attn_scratch_bytes(int B, int C, int heads, int h, int w, size_t* bytes);
int rf_chan_attn(const float* in, float* out, const float* qkv_w, const float* qkv_b,
                 const float* dw_w, const float* dw_b, const float* temperature,
                 const float* proj_w, const float* proj_b, void* scratch,
                 int B, int C, int heads, int h, int w, void* stream);
/* TransformerBlock.forward: FrequencyawareLumaChromaAttentionRAWFormer.py:238-254 (model.py:81-92).
 * prm = HOST array of 17 device pointers in state_dict order: norm1.{w,b}, attn.temperature,
 * attn.qkv.{w,b}, attn.qkv_dwconv.{w,b}, attn.project_out.{w,b}, norm2.{w,b},
 * ffn.pointwise1.{w,b}, ffn.depthwise.{w,b}, ffn.pointwise2.{w,b}.  Uses the fused gfx950 kernels
 * (rf_fused.hip) where the shape allows, exactly as rf_forward does. */
int rf_transformer_block_scratch_bytes(int B, int C, int heads, int ffn_expansion, int h, int w, size_t* bytes);
int rf_transformer_block(const float* in, float* out, const float* const* prm, void* scratch,
                         int B, int C, int heads, int ffn_expansion, int h, int w, void* stream);
/* The same on one window of a spatially sharded frame, as rf_forward runs it after rf_set_shard_grid: only rows [y_lo, y_hi) and
 * columns [x_lo, x_hi) of the window enter the attention's Gram sums and norms (x_lo and x_hi whole groups of 4 pixels, or x_hi = w;
 * all four 0: everything; x_lo = x_hi = 0: all columns; column bounds only together with row bounds: -22 otherwise).  No all-reduce: the statistics are the interior's alone.  Scratch: rf_transformer_block_scratch_bytes. */
int rf_transformer_block_window(const float* in, float* out, const float* const* prm, void* scratch,
                                int B, int C, int heads, int ffn_expansion, int h, int w, int y_lo, int y_hi, int x_lo, int x_hi, void* stream);
/* Host only, no launch, no GPU needed: how the fused attention front (LayerNorm -> qkv 1x1 -> depthwise 3x3 -> Gram partials + v;
 * C = 32, w % 4 == 0, heads that divide 16-channel tiles: -22 otherwise) is launched for [B,C,h,w].  out[0]: 1 = the eight-wave
 * kernel on tiles of 12 rows x 64 px, two per workgroup (above 256 x 256), 0 = the four-wave kernel on tiles of 4 x 64; out[1]:
 * workgroups per image = Gram partials per image; out[2]: floats of partials written, [B][out[1]][C/16][16][66]; out[3]: floats the
 * scratch layouts set aside for them (>= out[2]).  out[0] and out[1] depend on (h, w) alone, so an image's sums are added in the same
 * order whatever the batch. */
int rf_attn_front_plan(int B, int C, int heads, int h, int w, long long out[4]);
/* FLCA.forward given the guidance planes: FrequencyawareLumaChromaAttentionRAWFormer.py:134-162.
 * guide = [B,4,h,w] from rf_flca_guidance at the feature size; prm = HOST array of 10 device pointers:
 * alpha, beta, gamma, low_attn.0.w, high_attn.0.w, chroma_attn.0.w, se.1.{w,b}, se.3.{w,b}. */
int rf_flca_scratch_bytes(int B, int C, int h, int w, size_t* bytes);
int rf_flca(const float* feat, const float* guide, float* out, const float* const* prm, void* scratch,
            int B, int C, int h, int w, void* stream);
/* BayerLumaChroma + HaarDWT + bilinear resize = the guidance planes of FLCA
 * (FrequencyawareLumaChromaAttentionRAWFormer.py:79-97,138-149).
 * packed [B,4,H,W] -> guide [B,4,hf,wf] = (y_low, y_high, cr, cb); scratch >= rf_guidance_scratch_bytes.
 * On return the scratch area starts with the BayerLumaChroma output itself: y | cr | cb, each [B,H,W] floats. */
int rf_guidance_scratch_bytes(int B, int H, int W, size_t* bytes);
int rf_flca_guidance(const float* packed, float* guide, void* scratch, int B, int H, int W, int hf, int wf, void* stream);

/* ---- FFAB / FEB: the frequency block of the WFB variant (RawFomer_WFB_FFAB/blocks.py:11-92) ------------------------
 * rfft2 / irfft2 are hand-written LDS transforms (power-of-two lines: radix 2; any other length up to 2048: direct DFT);
 * norm='ortho'.  Widths must be even (irfft2 with s=(H,W) inverts rfft2 only then).
 * rf_rfft2_polar: [planes,h,w] -> |F| + 1e-6 and angle(F), each [planes,h,w/2+1]  (FEB, blocks.py:27-29)
 * rf_polar_irfft2: mag, pha [planes,h,w/2+1] -> irfft2(mag e^{i pha}) [planes,h,w]  (blocks.py:32-35) */
int rf_rfft2_polar_scratch_bytes(int planes, int h, int w, size_t* bytes);
int rf_rfft2_polar(const float* in, float* mag, float* pha, void* scratch, int planes, int h, int w, void* stream);
int rf_polar_irfft2(const float* mag, const float* pha, float* out, void* scratch, int planes, int h, int w, void* stream);
/* Host only, no launch, no GPU needed: what rf_rfft2_polar and rf_polar_irfft2 launch for [planes,h,w], or the error they return.
 * out = { log2 w, log2 h (-1: that axis takes the direct DFT),  L (rows per row workgroup), TC (columns per column workgroup),
 *         grid of the row kernel, grid of the column kernel,  most trips of a row / of a column workgroup through its persistent
 *         loop,  dynamic LDS bytes of the row / of the column kernel }. */
int rf_fft_plan(int planes, int h, int w, int out[10]);
/* FEB.forward (blocks.py:23-39).  prm = HOST array of 10 device pointers in state_dict order:
 * fpre.{w,b}, process1.0.{w,b}, process1.2.{w,b}, process2.0.{w,b}, process2.2.{w,b}.  [B,nc,h,w] -> same. */
int rf_feb_scratch_bytes(int B, int nc, int h, int w, size_t* bytes);
int rf_feb(const float* in, float* out, const float* const* prm, void* scratch, int B, int nc, int h, int w, void* stream);
/* FFAB.forward (blocks.py:83-92).  prm = HOST array of the module's 92 tensors in state_dict order
 * (conv0.0.{w,b}, conv0.1.<ProcessBlock: 10 FEB tensors, cat.{w,b}>, conv1..conv3, conv4.0.<PB>, conv4.1.{w,b}, conv5.*, convout.*). */
int rf_ffab_scratch_bytes(int B, int nc, int h, int w, size_t* bytes);
int rf_ffab(const float* in, float* out, const float* const* prm, void* scratch, int B, int nc, int h, int w, void* stream);
/* The gradients of the four operators above.  Conventions of rf_wm_backward: a *_bytes query returns a negative error code for a
 * geometry the operator refuses (the forward's: nc % 4 == 0, even w; and the transforms': lengths 2 .. 4096, a length that is no
 * power of two at most 2048); every tensor pointer is 16-byte aligned; outputs and scratch may not alias an input or each other
 * (-22 with an rf_last_error message otherwise; the byte ranges are compared, and rf_feb_backward / rf_ffab_backward, like
 * rf_mamba_backward / rf_wm_backward below, take in, grad_out, grad_in, every parameter, every gradient and the workspace into
 * that comparison; inputs alone may overlap one another); inputs and parameters are not written; every sum runs in a fixed order
 * (no float atomics): two runs give the same bits.
 * rf_rfft2_polar_backward: (in [planes,h,w], dL/dmag, dL/dpha [planes,h,w/2+1]) -> grad_in = dL/din.  The spectrum F of `in` is
 *   recomputed; G = dL/dmag F/|F| + dL/dpha (-Im F, Re F)/|F|^2, and 0 where F = 0 (torch's abs / angle backward).
 * rf_polar_irfft2_backward: (mag, pha, grad_out = dL/d irfft2(mag e^{i pha}) [planes,h,w]) -> dL/dmag, dL/dpha.
 * Both take planes * h * (w/2+1) complex values of scratch (the queries return that in bytes). */
long long rf_rfft2_polar_backward_scratch_bytes(int planes, int h, int w);
int rf_rfft2_polar_backward(const float* in, const float* grad_mag, const float* grad_pha, float* grad_in, void* scratch, int planes, int h, int w,
                            void* stream);
long long rf_polar_irfft2_backward_scratch_bytes(int planes, int h, int w);
int rf_polar_irfft2_backward(const float* mag, const float* pha, const float* grad_out, float* grad_mag, float* grad_pha, void* scratch,
                             int planes, int h, int w, void* stream);
/* rf_feb_backward / rf_ffab_backward: (in, grad_out = dL/d out, prm) -> grad_in = dL/d in and grad_prm, a HOST array of 10 / 92
 * device pointers with prm's order and shapes.  Nothing is kept from a forward call: the intermediates are recomputed with the
 * forward's own kernels.  Every shape rf_feb / rf_ffab accept is accepted, within the transforms' length limits.  grad_in is always
 * overwritten; accumulate != 0 ADDS to the grad_prm tensors, 0 overwrites them.  A workspace smaller than the query's answer is
 * refused with -12. */
long long rf_feb_backward_workspace_bytes(int B, int nc, int h, int w);
int rf_feb_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                    size_t workspace_bytes, int B, int nc, int h, int w, int accumulate, void* stream);
long long rf_ffab_backward_workspace_bytes(int B, int nc, int h, int w);
int rf_ffab_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                     size_t workspace_bytes, int B, int nc, int h, int w, int accumulate, void* stream);
/* out = add + clamp(in * scale + shift, lo, hi): inverse_data_transform + residual of WMB (model.py:13-15, 241-243). */
int rf_affine_clamp_add(const float* in, const float* add, float* out, size_t n, float scale, float shift, float lo, float hi, void* stream);

/* Decoder step of RawFormer.forward (RawFomer_WFB_FFAB/model.py:461-468, 494-503) as one kernel on composed weights:
 *   out = Conv2d(2C, C, 1)(cat[ConvTranspose2d(2C, C, 2, stride=2)(x), skip])
 * x [B,2C,h,w], skip and out [B,C,2h,2w]; up_w [2C,C,2,2], up_b [C], cr_w [C,2C,1,1], cr_b [C]; w % 4 == 0. */
int rf_upcat_scratch_bytes(int C, size_t* bytes);
int rf_upcat(const float* x, const float* skip, float* out, const float* up_w, const float* up_b, const float* cr_w, const float* cr_b,
             void* scratch, int B, int C, int h, int w, void* stream);

/* ---- evaluation harness: test.py:117-124 on the device ----------- */
/* (clamp(pred,0,1) * 255).astype(uint8), CHW float32 -> HWC uint8 (truncation): test.py:117-118 */
int rf_to_uint8_hwc(const float* in, unsigned char* out, int B, int C, int h, int w, void* stream);
/* per-image sum of squared differences of two uint8 images, exact uint64: PSNR (test.py:123) =
 * 10 log10(255^2 * n_per_image / sse) */
int rf_u8_sse(const unsigned char* a, const unsigned char* b, unsigned long long* sse, int B, size_t n_per_image, void* stream);
/* per-image, per-channel sums of HWC uint8 images (auto_correct_rb compares channel means, test.py:31-40) */
int rf_u8_channel_sums(const unsigned char* a, unsigned long long* sums, int B, int C, size_t hw, void* stream);
/* SSIM (test.py:124, structural_similarity(a, b, channel_axis=-1)) of uint8 HWC images [B,h,w,C]: 7x7 uniform window, K1 0.01,
 * K2 0.03, data range 255, sample covariance.  The five window sums are exact integers; ssim_sums[b*C + c] (float64) receives the
 * sum of the per-position values over the (h-6)(w-6) fully covered window positions of channel c, added in a fixed order (bitwise
 * reproducible, and the same for an image alone or in a batch); the caller divides by (h-6)(w-6) and averages the channels.
 * scratch: rf_u8_ssim_scratch_bytes bytes, 8-byte aligned, no initialisation needed.  h, w >= 7; C in 1..4; B in 1..65535. */
int rf_u8_ssim_scratch_bytes(int B, int C, int h, int w, size_t* bytes);
int rf_u8_ssim(const unsigned char* a, const unsigned char* b, double* ssim_sums /* [B*C] */, void* scratch,
               int B, int C, int h, int w, void* stream);

/* ---- SID front-end: correctdataloader.py:58-72 (pack_raw), :86 (x ratio),
 * :103 (min 1) fused into one pass over the uint16 Bayer frame [B, 2h, 2w]:
 *   v = min(clip((raw - black) / (white - black), 0, 1) * ratio, 1), evaluated in double, rounded once.
 * mode 0: the loader's packing [B,4,h,w] = sites (0,0) (0,1) (1,1) (1,0); mode 1: pixel_unshuffle order
 * (0,0) (0,1) (1,0) (1,1) (a1); mode 2: normalised mosaic [B,1,2h,2w] (RawFormer.forward's input).
 * black = min(black_level_per_channel); w % 4 == 0. */
int rf_sid_pack(const unsigned short* raw, float* out, int B, int h, int w, int black, int white, double ratio, int mode, void* stream);

/* ---- SID training batches from a device-resident set: load_data_SID.__getitem__, RawFomer_WFB_FFAB/load_dataset.py:53-95 ----
 * raw [N,H,W] uint16 short exposures, gt [N,H,W,3] uint16 long exposures (HWC), amp [N] float (100 / 300, :81-84).  Patch b is
 * rows i..i+ph, columns j..j+pw of frame desc[b][0], flipped left-right (flips bit 0) then up-down (bit 1) -- the mosaic itself
 * is flipped, as in the reference, so the CFA phase changes -- and normalised:
 *   x  = ((clip((float)raw, black, white) - black) / (float)(white - black + 1e-6)) * amp    in float32, each step rounded (:88-89)
 *   gt = (float)((double)v / 65535.0)                                                        (:90, :93)
 * x_out [B,1,ph,pw], gt_out [B,3,ph,pw].  pw % 4 == 0, W even, i and j even.  `desc` [B,4] = (frame, i, j, flips) is a DEVICE
 * table: the host that built it checks it with rf_sid_check_desc (HOST pointer, no device work); a patch whose descriptor is out of range
 * all the same is skipped by the kernel, which never reads or writes outside the buffers. */
int rf_sid_check_desc(const int* desc_host, int N, int H, int W, int B, int ph, int pw);
int rf_sid_sample(const unsigned short* raw, const unsigned short* gt, const float* amp, const int* desc, float* x_out, float* gt_out,
                  int N, int H, int W, int B, int ph, int pw, int black, int white, void* stream);

/* ---- MCR training batches from a device-resident set: load_data_MCR.__getitem__, RawFomer_WFB_FFAB/load_dataset.py:136-179 ----
 * raw [N,H,W] uint8 colour-raw frames, gt [N,H,W,3] uint8 RGB (HWC, as imageio returns it), amp [N] DOUBLE = gt_expo / img_expo
 * (:141-149).  Patches, flips, outputs and the descriptor table are those of rf_sid_sample (same rules, same rf_sid_check_desc);
 *   x  = (float)(((double)v / 255.0) * amp)     float64 quotient and product, rounded once (:151)
 *   gt = (float)((double)v / 255.0)             (:152)
 * raw and gt need 2-byte alignment only (the kernel reads aligned halfwords, and no byte outside the patches); amp 8, desc 4,
 * the outputs 16.  pw % 4 == 0, W even, i and j even. */
int rf_mcr_sample(const unsigned char* raw, const unsigned char* gt, const double* amp, const int* desc, float* x_out, float* gt_out,
                  int N, int H, int W, int B, int ph, int pw, void* stream);

/* ---- luminance-aware token attention: Attenblock.py:161-220 -----------------
 * softmax(q_i . k_j * scale) v_j per (image, head), flash style (the N x N scores are never stored).
 * q, k, v: [B, heads*d, N] with `bstride_qkv` floats between images (so they may be the three thirds of one
 * [B, 3*heads*d, N] tensor); out: [B, heads*d, N].  Einsums of Attenblock.py:212-216.  d <= 32. */
int rf_token_attn(const float* q, const float* k, const float* v, float* out, long long bstride_qkv, long long bstride_out,
                  int B, int heads, int d, int N, float scale, void* stream);
/* BayerLuma (Attenblock.py:79-138): mosaic [B,1,H,W] -> luma [B,1,H,W] in [0,1]: the 3x3 mask convolutions of the
 * pattern (0 rggb, 1 bggr, 2 grbg, 3 gbrg), .299 r + .587 g + .114 b, per-image (x - min) / (max - min + 1e-6). */
int rf_bayer_luma_scratch_bytes(int B, int H, int W, size_t* bytes);
int rf_bayer_luma(const float* mosaic, float* luma, void* scratch, int B, int H, int W, int pattern, void* stream);
/* FiLM of q,k,v and the query luma bias (Attenblock.py:193-210): out = gamma * qkv + beta on each third of
 * qkv [B, 3*inner, h*w]; the q third also gets alpha * (avg_pool3(1 - luma) - mean) when luma [B,1,h,w] != NULL.
 * gamma, beta: [B, inner, h*w] with `gb_bstride` floats between images; alpha: device scalar. */
int rf_luma_film_scratch_bytes(int B, int h, int w, size_t* bytes);
int rf_luma_film(const float* qkv, const float* gamma, const float* beta, long long gb_bstride, const float* luma, const float* alpha,
                 float* out, void* scratch, int B, int inner, int h, int w, void* stream);

/* ---- WFB extras without Mamba: RawFomer_WFB_FFAB/model.py:42-87, 174-200 -------
 * Middle of the gated FeedForward in eval mode: a = dw3x3(x; wa, ba) (the fused rep-conv branch, fuse() at
 * model.py:66-87), g = dw3x3(x; wb, bb) (dwconv), out = gelu(g) * a + gelu(a) * g (model.py:59); one pass. */
int rf_dwgate3x3(const float* in, float* out, const float* wa, const float* ba, const float* wb, const float* bb,
                 int B, int C, int h, int w, void* stream);
/* nn.Conv2d(C, C, 5, padding=2, groups=C) (+bias): Illumination_Estimator.depth_conv (model.py:182-183) */
int rf_dwconv5x5(const float* in, float* out, const float* weight, const float* bias, int B, int C, int h, int w, void* stream);

/* ---- the gated FeedForward in TRAINING mode and its gradient (RawFomer_WFB_FFAB/model.py:42-65; csrc/rf_wfb_train.hip) --------
 * in, out [B,dim,h,w]; hidden = project_in's output channels.  prm = HOST array of 16 device pointers: the 12 parameters
 *   project_in.{weight,bias}, dwconv.{weight,bias}, project_out.{weight,bias}, rep_conv1.c.weight, rep_conv1.bn.{weight,bias},
 *   rep_conv2.c.weight, rep_conv2.bn.{weight,bias}
 * then the 4 buffers rep_conv1.bn.running_{mean,var}, rep_conv2.bn.running_{mean,var}.
 * rf_wfb_ffn_train_forward: FeedForward.forward under train(): both Conv2d_BN branches normalise with the mean and the BIASED
 *   variance of their convolution's output over (B, h, w), N = B h w values per channel.  batch_stats [4][hidden] receives
 *   mu1, v1, mu2, v2.  update_running != 0 also updates the four buffers as nn.BatchNorm2d does (running <- (1 - momentum) running
 *   + momentum new, the variance UNBIASED, v N / (N - 1)); 0 leaves them unwritten (num_batches_tracked is the caller's).  The
 *   statistics are summed around a per-channel pivot, so the variance survives |mean| >> std, and folded on the device into the
 *   weights of rf_dwgate3x3: no host synchronisation.
 * rf_wfb_ffn_backward: (in, grad_out = dL/d out, prm) -> grad_in = dL/d in and grad_prm, a HOST array of 12 device pointers with the
 *   order and shapes of the 12 parameters.  training != 0: the gradient of rf_wfb_ffn_train_forward, through the batch statistics
 *   (the buffers are not read); 0: the gradient of the eval-mode forward on the running statistics (what rf_dwgate3x3 computes on
 *   FeedForward.fuse()'s weights).  Nothing is kept from a forward call: the intermediates and the statistics are recomputed.
 *   grad_in is always overwritten; accumulate != 0 ADDS to the 12 grad_prm tensors, 0 overwrites them.
 * Conventions of rf_wm_backward: a *_bytes query returns a negative error code for a geometry the operator refuses; refusals come
 * before any launch, -22 with an rf_last_error message that starts with the entry point's name: dim % 4 != 0, hidden % 4 != 0,
 * non-positive sizes, training mode with B h w < 2 (torch raises too), null or misaligned pointers (16 bytes: in, out, grad_out,
 * grad_in, batch_stats, workspace), and any byte range the call writes (out / grad_in, batch_stats, the gradients, the workspace, the
 * buffers of an updating forward) overlapping anything it reads or anything else it writes; a workspace smaller than the query's
 * answer is refused with -12.  Inputs and parameters are not written.  Every sum over pixels goes through per-workgroup slabs added
 * in a fixed order (no float atomics): two runs give the same bits.
 * rf_wfb_ffn_nblk: the slabs per image and channel of those sums for an h x w plane (one per 256 tiles of 4 x 4 pixels, at most 32). */
int rf_wfb_ffn_nblk(int h, int w);
long long rf_wfb_ffn_train_workspace_bytes(int B, int dim, int hidden, int h, int w);
int rf_wfb_ffn_train_forward(const float* in, float* out, float* const* prm, float* batch_stats, void* workspace, size_t workspace_bytes,
                             int B, int dim, int hidden, int h, int w, float eps, float momentum, int update_running, void* stream);
long long rf_wfb_ffn_backward_workspace_bytes(int B, int dim, int hidden, int h, int w);
int rf_wfb_ffn_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm,
                        void* workspace, size_t workspace_bytes, int B, int dim, int hidden, int h, int w, int training, float eps,
                        int accumulate, void* stream);

/* ---- Mamba selective scan and the WM block (RawFomer_WFB_FFAB/model.py:138-172): inference, and Mamba's gradient -------------------
 * mamba_ssm.modules.mamba_simple.Mamba(d_model, d_state, d_conv, expand).forward with the module's defaults
 * (dt_rank = ceil(d_model / 16), no projection biases, conv1d bias).  Di = expand * d_model, R = dt_rank.
 * prm = HOST array of 9 device pointers: in_proj.weight [2Di,D], conv1d.weight [Di,1,4], conv1d.bias [Di],
 * x_proj.weight [R+2N,Di], dt_proj.weight [Di,R], dt_proj.bias [Di], A_log [Di,N], D [Di], out_proj.weight [D,Di].
 * Supported: d_state 32, d_conv 4, expand >= 1, d_model % 4 == 0, d_model <= 512, Di <= 4096, any B >= 1 and L >= 1;
 * anything else is refused with a message (rf_last_error) before any launch.
 * The scan over L runs in chunks of rf_mamba_chunk_len() tokens: every chunk's end state from a zero start in parallel,
 * a short pass over the chunks in order, every chunk again from its incoming state.  No float atomics: two runs of one
 * input give the same bits.
 * rf_mamba_workspace_bytes: the workspace size in bytes (> 0), or a negative rf error code.
 * rf_mamba_forward: channel_major = 0: in and out are [B,L,D] (the module's own layout); 1: [B,D,L], L contiguous (the
 * layout of every other operator here).  in is not written; in, out and workspace are 16-byte aligned. */
int rf_mamba_chunk_len(void);
long long rf_mamba_workspace_bytes(int B, int L, int d_model, int d_state, int d_conv, int expand);
int rf_mamba_forward(const float* in, float* out, const float* const* prm, void* workspace, size_t workspace_bytes,
                     int B, int L, int d_model, int d_state, int d_conv, int expand, int channel_major, void* stream);
/* The module's gradient: (in, grad_out = dL/d out, prm) -> grad_in = dL/d in and grad_prm, a HOST array of 9 device pointers
 * with prm's order and shapes (conv1d.weight's gradient is [Di,1,4]).  Nothing is kept from a forward call: the intermediates
 * are recomputed.  The limits and refusals are rf_mamba_forward's; in, grad_out, grad_in and workspace are 16-byte aligned.
 * Nothing the call writes (grad_in, the nine gradients, the workspace) may overlap, in any byte, anything it reads (in, grad_out,
 * the nine parameters) or anything else it writes, and in may not be grad_out (-22); in, grad_out and the parameters are not
 * written.  grad_in is always overwritten;
 * accumulate != 0 ADDS to the nine grad_prm tensors (a training step sums several modules' calls), 0 overwrites them.
 * The adjoint recurrence runs in the forward's chunks, last to first, with every sum in a fixed order (no float atomics): two
 * runs give the same bits.  A workspace smaller than rf_mamba_backward_workspace_bytes is refused with -12. */
long long rf_mamba_backward_workspace_bytes(int B, int L, int d_model, int d_state, int d_conv, int expand);
int rf_mamba_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm,
                      void* workspace, size_t workspace_bytes, int B, int L, int d_model, int d_state, int d_conv, int expand,
                      int channel_major, int accumulate, void* stream);
/* WM.forward (model.py:165-172): x = convb(x) + x; tokens = LayerNorm_c(x.reshape(n, -1, c)) -- a RAW reshape of the NCHW
 * memory: token i is the run flat[i c : (i + 1) c] of an image; y = Mamba(c, 32, 4, 2)(tokens), stored channel-major, which
 * IS permute(0,2,1).reshape(n,c,h,w); out = smooth(y).  in, out [n,c,h,w].  prm = HOST array of 17 device pointers:
 * convb.0.{weight,bias}, convb.2.{weight,bias}, ln.{weight,bias}, model1.<the 9 above>, smooth.{weight,bias}. */
long long rf_wm_workspace_bytes(int n, int c, int h, int w);
int rf_wm_forward(const float* in, float* out, const float* const* prm, void* workspace, size_t workspace_bytes,
                  int n, int c, int h, int w, void* stream);
/* WM's gradient: (in, grad_out = dL/d out, prm) -> grad_in = dL/d in and grad_prm, a HOST array of 17 device pointers with
 * prm's order and shapes.  Nothing is kept from a forward call: the intermediates are recomputed with the forward's own kernels.
 * Every shape rf_wm_forward accepts is accepted (widths that are no multiple of 4 take a plain 3x3 weight-gradient kernel).
 * in, grad_out, grad_in and workspace are 16-byte aligned; the alias rule is rf_mamba_backward's, over the 17 tensors; in,
 * grad_out and the parameters are not written.  grad_in is always overwritten; accumulate != 0 ADDS to the 17 grad_prm tensors, 0 overwrites
 * them.  Every sum runs in a fixed order (no float atomics): two runs give the same bits.  A workspace smaller than
 * rf_wm_backward_workspace_bytes is refused with -12. */
long long rf_wm_backward_workspace_bytes(int n, int c, int h, int w);
int rf_wm_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm,
                   void* workspace, size_t workspace_bytes, int n, int c, int h, int w, int accumulate, void* stream);


/* ---- the three fused element-wise kernels of a WMB block as RF_VARIANT_WFB schedules it (csrc/rf_wmb.hip) ----------
 * All tensors NCHW float32, 16-byte aligned, the full-resolution width a multiple of 4 and the height even; 4 <= C <= 512.
 * rf_wmb_front: t = (x - mean_c) * rstd_c * w2[c] + b2[c] per pixel (w2 = 2 norm1.weight, b2 = 2 norm1.bias - 1, i.e.
 * data_transform(norm1(x))) and bands = dwt_init(t) in dwt_init's own expression order: x, t [B,C,2h,2w], bands [4B,C,h,w].
 * rf_wmb_back: out = t + clamp((iwt_init(bands) + 1) / 2, 0, 1).
 * rf_wmb_ffn_sum: out = t + y + LayerNorm_c(t; ln_w, ln_b), the tail of x + ffn(norm2(x)) with y = project_out(..):
 * t, y, out [B,C,h,w] (w % 4 == 0). */
int rf_wmb_front(const float* x, float* t, float* bands, const float* w2, const float* b2, int B, int C, int h, int w, void* stream);
int rf_wmb_back(const float* bands, const float* t, float* out, int B, int C, int h, int w, void* stream);
int rf_wmb_ffn_sum(const float* t, const float* y, float* out, const float* ln_w, const float* ln_b, int B, int C, int h, int w,
                    void* stream);

/* ---- the gradient pieces of a WMB block that the block operators above do not cover (csrc/rf_wmb_bwd.hip) ---------------------
 * Conventions of rf_wm_backward: a *_bytes query returns a negative error code for a geometry the operator refuses; refusals come
 * before any launch, -22 with an rf_last_error message that starts with the entry point's name; every tensor pointer is 16-byte
 * aligned; nothing the call writes (grad_in, the gradients, the workspace) may overlap anything it reads or anything else it
 * writes; a workspace smaller than the query's answer is refused with -12.  Nothing is kept from a forward call; inputs are not
 * written; grad_in / grad_bands are always overwritten; accumulate != 0 ADDS to the parameter gradients, 0 overwrites them.  Every
 * sum over pixels goes through per-workgroup slabs added in a fixed order (no float atomics): two runs give the same bits.
 * rf_wmb_front_backward: the gradient of rf_wmb_front.  x, grad_t, grad_x [B,C,2h,2w], grad_bands [4B,C,h,w]; with
 *   g = grad_t + iwt_init(grad_bands) (= dwt_init^T; never stored), grad_x = the LayerNorm adjoint of g under the weight w2 and
 *   grad_w2 [C] (+)= grad_scale sum g xhat, grad_b2 [C] (+)= grad_scale sum g (a block passes w2 = 2 norm1.weight and grad_scale 2).
 *   Limits of rf_wmb_front: 4 <= C <= 512, even w.  rf_wmb_front_backward_nblk: its slabs per image.
 * rf_wmb_back_backward: the gradient of rf_wmb_back with respect to bands: grad_bands = dwt_init(m grad_out / 2), m = 1 where the
 *   forward's value before the clamp lies in [0, 1] (torch.clamp's backward), recomputed in the forward's expression order.  The
 *   gradient with respect to t is grad_out itself.  No parameters, no workspace.
 * rf_dwconv5x5_backward: the gradient of rf_dwconv5x5: grad_in = the stencil of grad_out on the flipped taps, grad_weight [C,1,5,5]
 *   and grad_bias [C].  rf_dwconv5x5_backward_nblk: the slabs per plane of the tap sums (one per 1024 groups of 4 pixels, at most 32).
 * rf_illumination_estimator_backward: the gradient of Illumination_Estimator.forward (model.py:186-200).  img, grad_img [B,C,h,w],
 *   grad_fea [B,Cm,h,w], grad_map [B,Co,h,w] or NULL (WMB.forward discards illu_map): then conv2's two gradients are not touched.
 *   prm / grad_prm = HOST arrays of 6 device pointers: conv1.weight [Cm,C+1,1,1], conv1.bias, depth_conv.weight [Cm,1,5,5],
 *   depth_conv.bias, conv2.weight [Co,Cm,1,1], conv2.bias.  C, Cm, Co are multiples of 4 in 4 .. 512.  with_map of the query: whether
 *   grad_map will be given.
 * rf_layernorm2d_backward: the gradient of rf_layernorm2d (with bias): grad_in = residual (NULL: none) + the adjoint, grad_weight,
 *   grad_bias [C]; 1 <= C <= 512. */
int rf_wmb_front_backward_nblk(int B, int C, int h, int w);
long long rf_wmb_front_backward_workspace_bytes(int B, int C, int h, int w);
int rf_wmb_front_backward(const float* x, const float* grad_t, float* grad_x, const float* grad_bands, const float* weight2, float* grad_weight2,
                          float* grad_bias2, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, float grad_scale, int accumulate,
                          void* stream);
int rf_wmb_back_backward(const float* bands, const float* grad_out, float* grad_bands, int B, int C, int h, int w, void* stream);
int rf_dwconv5x5_backward_nblk(int h, int w);
long long rf_dwconv5x5_backward_workspace_bytes(int B, int C, int h, int w);
int rf_dwconv5x5_backward(const float* in, const float* grad_out, float* grad_in, const float* weight, float* grad_weight, float* grad_bias,
                          void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int accumulate, void* stream);
long long rf_illumination_estimator_backward_workspace_bytes(int B, int C, int Cm, int Co, int h, int w, int with_map);
int rf_illumination_estimator_backward(const float* img, const float* grad_fea, const float* grad_map, float* grad_img, const float* const* prm,
                                       float* const* grad_prm, void* workspace, size_t workspace_bytes, int B, int C, int Cm, int Co, int h, int w,
                                       int accumulate, void* stream);
long long rf_layernorm2d_backward_workspace_bytes(int B, int C, int h, int w);
int rf_layernorm2d_backward(const float* in, const float* grad_out, float* grad_in, const float* weight, float* grad_weight, float* grad_bias,
                            const float* residual, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, float eps, int accumulate,
                            void* stream);

/* ---- the gradient of a whole WMB block (RawFomer_WFB_FFAB/model.py:203-245; csrc/rf_wmb_block_bwd.hip) -------------------------
 * rf_wmb_backward: (in, grad_out = dL/d out, prm) -> grad_in = dL/d in and grad_prm, for out = WMB.forward(in); in, grad_out,
 *   grad_in [B,C,h,w], h x w the FULL-resolution plane.  One host schedule over the operators above: the forward is recomputed
 *   (rf_wmb_front, illu.conv1 + rf_dwconv5x5, rf_ffab, rf_wm_forward, rf_wmb_back, rf_layernorm2d), then rf_wfb_ffn_backward,
 *   rf_layernorm2d_backward with residual = grad_out, rf_wmb_back_backward, rf_ffab_backward, rf_illumination_estimator_backward,
 *   rf_wm_backward and rf_wmb_front_backward with grad_scale 2 run in that order, each on the arguments the stand-alone call would
 *   get: the results have the bits of that composition.  Nothing is kept from a forward call.
 *   prm = HOST array of 135 device pointers: the block's 131 parameters in state_dict order -- norm1.body.{weight,bias}, illu.<the 6
 *   of rf_illumination_estimator_backward, Cm = Co = C>, ffab.<92>, norm2.body.{weight,bias}, ffn.<the 12 parameters of
 *   rf_wfb_ffn_backward>, mb.<the 17 of rf_wm_backward> -- then ffn's 4 BatchNorm buffers (rep_conv1.bn.running_{mean,var},
 *   rep_conv2.bn.running_{mean,var}); grad_prm = HOST array of the 131 gradients.  hidden = ffn.project_in's output channels.
 *   training != 0: ffn's gradient runs through the batch statistics (the buffers are not read); 0: on the running statistics.  eps
 *   is the BatchNorms'; both LayerNorms use 1e-5.  grad_in is always overwritten; accumulate != 0 ADDS to the gradients, 0 overwrites
 *   them.  illu.conv2.{weight,bias} feed only illu_map, which WMB.forward discards: their gradients are set to exact zeros
 *   (accumulate == 0) or left untouched.
 *   Limits, the intersection of the pieces': B <= 21845 (WM runs on 3 B images), C % 4 == 0 in 4 .. 512, hidden % 4 == 0, h even,
 *   w % 4 == 0, h / 2 and w / 2 within the transform's lengths (2 .. 4096, at most 2048 when no power of two); B h w >= 16
 *   follows, so the batch statistics of training mode always have more than one value per channel.  Conventions of rf_wm_backward: the query returns a negative error code for a refused geometry; every refusal comes before the first launch,
 *   -22 with an rf_last_error message that starts with the entry point's name, -12 for a workspace smaller than the query's
 *   answer; in, grad_out, grad_in and workspace are 16-byte aligned; nothing the call writes may overlap anything it reads or
 *   anything else it writes; in, grad_out, the parameters and the buffers are not written; no float atomics: two calls give the
 *   same bits.  The workspace holds six planes and two quarter planes of activations and ONE region, the largest of the pieces'
 *   workspaces, that the pieces use in turn. */
long long rf_wmb_backward_workspace_bytes(int B, int C, int hidden, int h, int w);
int rf_wmb_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm,
                    void* workspace, size_t workspace_bytes, int B, int C, int hidden, int h, int w, int training, float eps,
                    int accumulate, void* stream);

/* ---- the element-wise kernels of RF_VARIANT_TRUECOLOR one by one (csrc/rf_truecolor.hip; BayerTORGBColorMultiLvl.py) ----------
 * No handle: the caller passes the raw parameter tensors.  Every argument is checked before any launch (RF_E_INVALID).
 * rf_tc_spatial: xs = feat * (1 + sigmoid(conv3x3(guide[0:5]; w_col, b_col)) + tanh(sigmoid(conv3x3(guide[5]; w_low, b_low)) +
 * tanh(conv3x3(guide[6]; w_high, b_high)))) (EnhancedFLCA.forward, :277-283).  feat, xs [B,C,h,w]; guide [B,7,h,w]; w_col [C,5,3,3],
 * w_low, w_high [C,1,3,3], the biases [C]; C <= 512.  16 bytes per lane where w % 4 == 0 and feat, xs are 16-byte aligned.
 * rf_tc_residual: x2 = xs + 0.2 tanh(r) (:285-288) and partial[b][blk][c] = the sum of x2 over the pixels of block blk, the
 * squeeze-excite pooling sums (:289); a block is 1024 consecutive pixels where w % 4 == 0 (then xs, r, x2 must be 16-byte
 * aligned), else 256; rf_tc_nblk(h, w) blocks per image.  x2 may be xs.  C <= 512.  Fixed summation order, no atomics.
 * rf_tc_color_head: CameraAwareColorCorrection.forward (:160-176) in place on x [B,3,P]; gamma [1], ct0_w [64,3], ct0_b [64],
 * ct2_w [3,64], ct2_b [3], tone0_w [32], tone0_b [32], tone2_w [32], tone2_b [1].
 * rf_tc_pyramid: one more level of EnhancedFLCA._pyramid_y (:236-247): ll = Haar LL of src, mag = sqrt(LH^2 + HL^2 + HH^2 + 1e-8);
 * src [B,hs,ws] with hs, ws >= 2 (an odd side is reflect-padded as HaarDWT does), ll, mag [B,ceil(hs/2),ceil(ws/2)]. */
int rf_tc_spatial(const float* feat, const float* guide, const float* w_col, const float* b_col, const float* w_low, const float* b_low,
                  const float* w_high, const float* b_high, float* xs, int B, int C, int h, int w, void* stream);
int rf_tc_nblk(int h, int w);
int rf_tc_residual(const float* xs, const float* r, float* x2, float* partial, int B, int C, int h, int w, void* stream);
int rf_tc_color_head(float* x, const float* gamma, const float* ct0_w, const float* ct0_b, const float* ct2_w, const float* ct2_b,
                     const float* tone0_w, const float* tone0_b, const float* tone2_w, const float* tone2_b, int B, size_t P, void* stream);
int rf_tc_pyramid(const float* src, float* ll, float* mag, int B, int hs, int ws, void* stream);

/* ---- the element-wise kernels of RF_VARIANT_MULTILVL one by one (csrc/rf_multilvl.hip; FLCA_Pyramid.forward,
 * MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:132-183) ----------
 * No handle: the caller passes the raw parameter tensors.  Every argument is checked before any launch (RF_E_INVALID): nulls, 4-byte
 * alignment, B <= 65535, C <= 512, levels in 1..3, step in 0..levels.  guide [B,2 levels+2,h,w] and means [B,8] as rf_ml_guidance
 * leaves them.  step < levels is pyramid level `step`: w_a = low_attn[step] [C,1,3,3], w_b = high_attn[step] [C,1,3,3], gate_w / gate_b
 * = freq_gate_head[step] [2,2], [2]; step == levels is the chroma form: w_a = chroma_attn [C,2,3,3], w_b unused (may be NULL),
 * gate_w / gate_b = chroma_gate [1], [1].
 * rf_ml_modulate: out = x * (g0 sigmoid(conv3x3(y_low; w_a)) + g1 tanh(conv3x3(y_high; w_b))), (g0, g1) = sigmoid(gate_w (mean y_low,
 * mean y_high) + gate_b) (:147-162), or out = x * sigmoid(gate_w mean|c| + gate_b) sigmoid(conv3x3([cr, cb]; w_a)) (:170-173).
 * x, out [B,C,h,w]; 16 bytes per lane where w % 4 == 0 and x, out are 16-byte aligned.
 * rf_ml_step_fused: out = x + 0.2 tanh(W2 relu(W0 m + b0) + b2) with m = rf_ml_modulate's result, in one kernel; w0, w2 [C,C], b0, b2
 * [C] (res_proj.0 / .2).  C = 16, 32, 48 or 64, w % 4 == 0, h * w % 64 == 0.  partial: NULL, or [B,rf_tc_nblk(h, w),C], the sums of
 * out over each block of 1024 consecutive pixels (rf_tc_residual's layout).  out may be x.
 * rf_ml_residual: out = x + 0.2 tanh(r) over B C h w elements; 16 bytes per lane where that count is a multiple of 4 and all three
 * are 16-byte aligned.  out may be x. */
int rf_ml_modulate(const float* x, const float* guide, const float* means, int step, int levels, const float* w_a, const float* w_b,
                   const float* gate_w, const float* gate_b, float* out, int B, int C, int h, int w, void* stream);
int rf_ml_step_fused(const float* x, const float* guide, const float* means, int step, int levels, const float* w_a, const float* w_b,
                     const float* gate_w, const float* gate_b, const float* w0, const float* b0, const float* w2, const float* b2,
                     float* out, float* partial, int B, int C, int h, int w, void* stream);
int rf_ml_residual(const float* x, const float* r, float* out, int B, int C, int h, int w, void* stream);

/* ---- FLCA_Pyramid as an operator and its gradient (csrc/rf_flca_pyramid.hip, csrc/rf_flca_pyramid_bwd.hip;
 * MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:86-183) ----------
 * No handle.  feat, out [B,C,h,w]; packed [B,4,H,W], the packed Bayer frame the guidance is made from inside the call (the planes
 * resized to (h, w), the means those of the resized planes; (h, w) need not be (H >> k, W >> k)).  prm = HOST array of
 * 4 levels + 11 device pointers in state_dict order: low_attn.<l>.0.weight [C,1,3,3] for every l, high_attn.<l>.0.weight for every
 * l, freq_gate_head.<l>.{weight [2,2], bias [2]} for every l, chroma_attn.0.weight [C,2,3,3], chroma_gate.{weight [1], bias [1]},
 * se.1.{weight [hid,C], bias [hid]}, se.3.{weight [C,hid], bias [C]} with hid = max(8, C / 8), res_proj.0.{weight [C,C], bias [C]},
 * res_proj.2.{weight, bias}.
 *   x_0 = feat;  x_{s+1} = x_s + 0.2 tanh(res_proj(x_s S_s)), s = 0 .. levels (S_s: rf_ml_modulate's gate of step s);
 *   out = x_{levels+1} sigmoid(se.3 relu(se.1 mean_p(x_{levels+1})))
 * Supported: 1 <= B <= 65535, 1 <= C <= 512, levels 1..3, H % 8 == 0, W % 8 == 0, any h, w >= 1 with h w <= 2^28.  Anything else is
 * refused before the first launch: the *_bytes queries return the negative error code, the entry points -22, with an rf_last_error
 * message that starts with the entry point's name.  -12 for a workspace smaller than the query's answer.
 * rf_flca_pyramid_forward: feat, packed, out and workspace 16-byte aligned; out may not overlap feat.  A step is one kernel where
 * rf_ml_step_fused runs (C = 16, 32, 48, 64, w % 4 == 0, h w % 64 == 0), elsewhere rf_ml_modulate, two 1x1 GEMMs and the residual.
 * rf_flca_pyramid_backward: (feat, packed, grad_out = dL/d out) -> grad_in = dL/d feat and the 4 levels + 11 parameter gradients
 * (shapes of prm).  packed and the guidance carry no gradient.  Conventions of rf_wm_backward: nothing is kept from a forward call
 * (x_1 .. x_{levels+1} are recomputed, then each step's intermediates in turn); feat, packed, grad_out and the parameters are not
 * written; grad_in is always overwritten; accumulate != 0 ADDS to the grad_prm tensors, 0 overwrites them (res_proj's are the sum
 * over the levels + 1 steps either way); every pointer but the two arrays is 16-byte aligned; nothing the call writes (grad_in,
 * the gradients, the workspace) may overlap anything it reads (feat, grad_out, the parameters, packed) or anything else it writes;
 * every sum runs in a fixed order (no float atomics): two runs give the same bits.
 * rf_ml_corrections_backward: the adjoint of rf_ml_tail's map image -> image (affine in the image with constant coefficients, so no other
 * input): with G = sum_c g_c and w = (0.299, 0.587, 0.114), g1_c = g_c - 0.03 w_c G and grad_image_c = g1_c - 0.12 mean_p(g1_c).
 * grad_out, grad_image [B,3,h2,w2], 16-byte aligned, not overlapping; any h2 w2 >= 1 (<= 2^30), B <= 65535; 16 bytes per lane where
 * w2 % 4 == 0.  workspace >= rf_ml_corrections_backward_workspace_bytes(B, h2, w2). */
long long rf_flca_pyramid_workspace_bytes(int B, int C, int h, int w, int H, int W, int levels);
int rf_flca_pyramid_forward(const float* feat, const float* packed, float* out, const float* const* prm, void* workspace,
                            size_t workspace_bytes, int B, int C, int h, int w, int H, int W, int levels, void* stream);
long long rf_flca_pyramid_backward_workspace_bytes(int B, int C, int h, int w, int H, int W, int levels);
int rf_flca_pyramid_backward(const float* feat, const float* packed, const float* grad_out, float* grad_in, const float* const* prm,
                             float* const* grad_prm, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                             int levels, int accumulate, void* stream);
long long rf_ml_corrections_backward_workspace_bytes(int B, int h2, int w2);
int rf_ml_corrections_backward(const float* grad_out, float* grad_image, void* workspace, size_t workspace_bytes, int B, int h2, int w2,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAWFORMER_HIP_H */
