// The RawFormer handle (internal): parameter registry, packed-weight plans, the variant's traits and the index table.  The
// registry (rf_registry.hip) fills all of it before the first forward: rf_create registers every tensor by name once (add_param)
// and records its registry index where the schedules need it: per Conv_Transformer stage in `stage[1..7]`, per other module in
// the fields below; a group of parameters that travels together (FLCA, the TrueColor modules) is one struct with a named field
// per tensor.  The forward schedule (rf_model.hip) and the training schedule (rf_trainstep.hip) only read: pointers through those
// indices (prm / pk / pk3 / flca_prm), model facts through `vt`; names serve rf_set_param and rf_param_info only.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>
#include "rf_common.h"

// Forms of a weight in the training step's pack cache: as it multiplies in the forward (PF_N); transposed -- 3x3: also
// tap-flipped -- for the dX product of the backward (PF_T); a ConvTranspose2d's dX GEMM (PF_CTB); ..3: the same matrix in b3 form
enum PackForm { PF_N, PF_T, PF_CTB, PF_N3, PF_T3, PF_CTB3, PF_COUNT };
constexpr size_t kNotCached = ~(size_t)0;

struct Param {
    std::string name;
    int64_t shape[4];
    int ndim;
    const float* ptr;
    int flags = 0;                    // RF_PARAM_BUFFER | RF_PARAM_UNUSED (rawformer_hip.h)
    int pack = -1, pack3 = -1;        // packs[] entries of its packed and its b3 form (rf_pack_params), -1: none
    size_t cache[PF_COUNT];           // floats into the training pack cache per PackForm, kNotCached: not held
    size_t numel() const {
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
        return n;
    }
};

enum PackKind { PK_1x1, PK_3x3, PK_CONVT, PK_1x1_B3 };
struct PackItem {
    int param;       // index of the raw weight
    PackKind kind;
    size_t offset;   // floats into the packed buffer
    size_t floats;
};

struct CachePack {   // one weight form of the training pack cache: `d` without its addresses (src = the parameter, dst = offset)
    int param;
    size_t offset;
    rf::PackDesc d;
};

// registry indices of the TrueColor parameter groups, in registration order (the FLCA group and SeGroup: rf_common.h)
struct TcIx {        // EnhancedFLCA branch of a stage: weight and bias of color_attention.0, low_attn.0, high_attn.0, se, res_proj.0 / .2
    int col_w, col_b, low_w, low_b, high_w, high_b;
    rf::SeGroup<int> se;
    int res0_w, res0_b, res2_w, res2_b;
};
struct MlIx {        // FLCA_Pyramid branch of a stage: low_attn.<l>.0 / high_attn.<l>.0 weights, freq_gate_head.<l>, chroma_attn.0, chroma_gate, se, res_proj.0 / .2
    int low_w[3], high_w[3], gate_w[3], gate_b[3];
    int chr_w, cgate_w, cgate_b;
    rf::SeGroup<int> se;
    int res0_w, res0_b, res2_w, res2_b;
};
struct BayerProcIx { int wb_gains, color_matrix, dm0_w, dm0_b, dm2_w, dm2_b, ce0_w, ce0_b, ce2_w, ce2_b; };   // bayer_processor.*: demosaic_refine.0 / .2, chroma_extractor.0 / .2
struct ColorCorrIx { int gamma, ct0_w, ct0_b, ct2_w, ct2_b, tone0_w, tone0_b, tone2_w, tone2_b; };             // color_correction.*: color_transform.0 / .2, tone_curve.0 / .2

// registry indices of a WMB block (RF_VARIANT_WFB, RawFomer_WFB_FFAB/model.py:203-245); bn = weight, bias, running_mean, running_var
struct WmbIx {
    int ln1_w, ln1_b, illu1_w, illu1_b, illu_dw_w, illu_dw_b;
    int ffab[92];                     // rf_ffab's order (= state_dict order)
    int ln2_w, ln2_b, rep1_w, bn1[4], rep2_w, bn2[4], pin_w, pin_b, dw_w, dw_b, pout_w, pout_b;
    int wm[17];                       // rf_wm_forward's order: convb.0, convb.2, ln, model1.<9>, smooth
    int hid;                          // FeedForward's hidden width
    size_t fold = 0, illu_pk = 0;     // floats into the packed buffer: launch_wmb_fold's outputs [ln2 | rep_w | rep_b | illu_fold], packed illu.conv1
};

// Stage tail  channel_reduce(cat(branch, x1 + pointwise2(g)))  as one bf16x3 GEMM over [branch ; x1 ; g] (K = 2C + hidden):
// K blocks of 32 channels must not straddle the sources.  Level 0 of RawFormer-S / -B runs the fused FFN kernel instead
// (run_stage decides per call: the fused kernel takes only some image sizes).
inline bool tail_composable(int C, int hc) { return C % 32 == 0 && hc % 32 == 0 && hc > 0; }

// registry indices of one Conv_Transformer stage (add_stage)
struct StageIx {
    int lvl;         // U-Net level: channels dim << lvl, size H >> lvl
    int first;       // its first parameter
    int ln1_w, ln1_b, temperature /* or log_temperature */, qkv_w, qkv_b, qkv_dw_w, qkv_dw_b, proj_w, proj_b;
    int ln2_w, ln2_b, pw1_w, pw1_b, dw_w, dw_b, pw2_w, pw2_b;
    int cr_w, cr_b, out_w, out_b;     // channel_reduce, Conv_out
    int conv_w, conv_b;               // plain branch
    rf::FlcaGroup<int> flca;            // FLCA branch
    TcIx tc;                          // TrueColor branch
    MlIx ml;                          // multi-level FLCA branch
    WmbIx wmb;                        // WFB: the WMB block in place of the TransformerBlock
    // composed tail (rf_flca.hip pack_tail), floats into the packed buffer of [Wb W2 | b'] (0 = not composed) and, plain variant
    // only, of the static b3 weights [Wa | Wb | Wb W2]
    size_t tail_offset = 0, tail3_offset = 0;
};

// The handle's second stream.  rf_forward and rf_train_step run part of their work on it: fork = an event on the caller's stream
// that the side stream waits for, join = the reverse.  The stream and both events are created on first use; if that fails,
// everything stays on the caller's stream.  Defined in rf_model.hip (one definition for the product and the diagnostic objects).
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool failed = false;    // creation failed: one stream from then on
    bool pending = false;   // forked and not joined yet
    int forks = 0;          // forks since the current call began (the diagnostic build's RF_FAIL_FORK counts them)
    hipStream_t get(hipStream_t st);                // the side stream; `st` while profiling or when it cannot be created
    int fork(hipStream_t st, hipStream_t side);     // everything enqueued on st so far precedes what is enqueued on side from now on
    int join(hipStream_t st, hipStream_t side);     // ... and the reverse; both no-ops when side == st
    void join_pending(hipStream_t st);              // join what a fork left pending, reporting nothing (SideJoinGuard)
    void destroy();
};

// One at the top of every entry point that forks: on an early error return it joins what is still pending, so from the
// caller's side all work of the call is ordered on `st` also then.  On success paths every fork is already joined and it issues
// no HIP call.
struct SideJoinGuard {
    SideStream& s;
    hipStream_t st;
    SideJoinGuard(SideStream& s_, hipStream_t st_) : s(s_), st(st_) { s.forks = 0; }
    ~SideJoinGuard() { s.join_pending(st); }
};

// What the schedules need to know about cfg.variant: plain data, set once by rf_create and read in its place.
enum BranchKind { BR_CONV, BR_FLCA, BR_TC, BR_ML };   // a stage's branch: 3x3 conv (plain, wfb), FLCA, EnhancedFLCA (TrueColor), FLCA_Pyramid (multilvl)
struct VariantTraits {
    BranchKind branch;
    bool wmb_block;                  // the stage's block is WMB (rf_wmb.hip), not the TransformerBlock
    bool branch_after;               // BR_TC, BR_ML: the branch borrows bufA and pools with tc_residual, so it follows the block on the caller's stream
    int levels;                      // flca_levels, resolved (0 = the default 2)
    int guide_planes;                // planes of the guidance pyramid at every U-Net level
    bool log_temperature;            // the attention's `temperature` holds log T
    bool shardable;                  // rf_set_shard / rf_set_shard_grid accept it
    bool stage_needs_packed_frame;   // rf_forward_stage derives the branch's guidance from the packed frame
};

struct rf_handle {
    rf_config cfg;
    VariantTraits vt;
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;   // name -> params[] (rf_set_param)
    std::vector<PackItem> packs;
    size_t packed_floats = 0;
    const float* packed = nullptr;   // caller memory, valid after rf_pack_params
    // the index table
    StageIx stage[8];                // 1..7
    int embedding_w, embedding_b, conv_out_w, conv_out_b;
    int down_w[3], up_w[3], up_b[3], upcr_w[3], upcr_b[3];   // down<i>, up<i>, channel_reduce<i> at [i - 1]
    BayerProcIx bp;                  // TrueColor: bayer_processor.*
    ColorCorrIx cc;                  //            color_correction.*
    size_t upcat_offset[3] = {0, 0, 0};   // composed decoder-step weights (rf_upcat.hip), floats into the packed buffer
    // training (plan_training): float offset of every parameter in the flat parameter / gradient buffers; the gradient ranges in
    // the order the step announces them; the pack cache's forms in the order it writes them
    std::vector<size_t> flat_offset;
    size_t flat_floats = 0;
    struct GradRange { size_t offset, count; };
    std::vector<GradRange> grad_ranges;
    std::vector<CachePack> cache_packs;
    size_t cache_floats = 0;
    // spatial shard of one frame (rf_set_shard / rf_set_shard_grid): interior rows [y_lo, y_hi) of the local window and the
    // frame's total rows, in packed (level-0) rows, and the same for columns (x_hi = 0: all columns, total_cols = 0: the window's
    // width -- a row shard); `allreduce` sums a float buffer over the ranks on the given stream
    int shard_y_lo = 0, shard_y_hi = 0, shard_total_rows = 0;
    int shard_x_lo = 0, shard_x_hi = 0, shard_total_cols = 0;
    void (*shard_allreduce)(void* user, float* buf, size_t n, int op, void* stream) = nullptr;
    void* shard_user = nullptr;
    // second stream: the forward's branches and the training step's weight-gradient kernels run on it (SideStream above)
    SideStream side;
    // training: notification that a range of the flat gradient buffer is final (rf_set_grad_ready)
    void (*grad_ready)(void* user, size_t offset, size_t count, void* stream) = nullptr;
    void* grad_ready_user = nullptr;
    // training: the criterion sees clamp(pred, 0, 1) (rf_set_loss_clamp)
    int loss_clamp = 0;

    const float* prm(int ix) const { return params[ix].ptr; }
    const float* pk(int ix) const { return packed + packs[params[ix].pack].offset; }
    const float* pk3(int ix) const { return packed + packs[params[ix].pack3].offset; }
    rf::SePrm se_prm(const rf::SeGroup<int>& x) const { return {prm(x.se1_w), prm(x.se1_b), prm(x.se3_w), prm(x.se3_b)}; }
    rf::FlcaPrm flca_prm(const rf::FlcaGroup<int>& x) const {
        return {prm(x.alpha), prm(x.beta), prm(x.gamma), prm(x.w_low), prm(x.w_high), prm(x.w_chr), se_prm(x.se)};
    }
};

// rf_wmb.hip: one WMB block of the WFB variant.  Buffers (U = B C h w floats of the stage's activation, f = ffn_expansion):
// t U, bands U, illu and fea U / 4 each, hid and gated f U each, ffab / wm = ffab_scratch_floats / wm_workspace_floats of the
// half-resolution bands.  pack_wmb writes the block's folds (wmb_fold_floats at WmbIx::fold) and the packed illu.conv1.
namespace rf {
struct WmbBufs { float *t, *bands, *illu, *fea, *hid, *gated, *ffab, *wm; };
size_t wmb_fold_floats(int C, int hid);
int pack_wmb(rf_handle* h, int stage, float* base, hipStream_t st);
int run_wmb(const rf_handle* h, int stage, const float* in, float* out, const WmbBufs& b, int B, int hh, int ww, hipStream_t st);
}  // namespace rf

// rf_trainstep.hip: lay out the flat buffers, the gradient ranges and the pack cache (rf_create, once the registry is complete)
void plan_training(rf_handle* h);
