// RawFormer handle, the forward: workspace plan, the stage schedule, rf_forward and rf_forward_stage
// (RawFomer_WFB_FFAB/model.py:473-508 == FrequencyawareLumaChromaAttentionRAWFormer.py:330-370).  What the model is -- parameters,
// packed weights, the variant's traits `vt` -- is rf_registry.hip's; nothing here asks which variant runs.
// Host code only; every kernel lives in the rf_*.hip files next to this one.
#include <cstdlib>
#include "rf_common.h"

using namespace rf;

#include "rf_handle.h"

namespace {

// ---- workspace plan ---------------------------------------------------------------------
struct Plan {
    size_t total;
    size_t gscratch, guide[4], skip[3], tA, tB, tU, bufA, bufB, x1, trans, xs, cr;
    size_t gram_partial, wfold_attn, wfold_cr, wfold_attn3, wfold_cr3, flca_partial, ch;
    size_t ffab, wm;            // WMB: FFAB scratch and WM workspace at their largest level, shared by the stages
    size_t ks, ks_floats;       // scratch of the 3x3 convs' input-channel split (small frames only: ks_floats = 0 otherwise)
};

int make_plan(const rf_handle* h, int B, int H, int W, Plan& p) {
    const rf_config& c = h->cfg;
    const VariantTraits& vt = h->vt;
    const size_t U0 = (size_t)B * c.dim * H * W;   // floats of a level-0 activation
    Bump b;      // offsets into the caller's workspace
    switch (vt.branch) {
    case BR_ML: p.gscratch = b.off(ml_scratch_floats(B, H, W, vt.levels)); break;
    case BR_TC: p.gscratch = b.off(tc_front_scratch_floats(B, H, W, vt.levels)); break;
    default: p.gscratch = b.off(guidance_scratch_floats(B, H, W));      // BR_FLCA's; the conv branch leaves it unused
    }
    for (int l = 0; l < 4; ++l) p.guide[l] = b.off((size_t)B * vt.guide_planes * (H >> l) * (W >> l));
    for (int l = 0; l < 3; ++l) p.skip[l] = b.off(U0 >> l);
    p.tA = b.off(U0);
    p.tB = b.off(U0);
    p.tU = b.off(U0);
    // widest TransformerBlock intermediate: qkv (3C) or the FFN hidden tensor (ffn_expansion * C) on the op-by-op path
    const size_t wide = (size_t)(c.ffn_expansion > 3 ? c.ffn_expansion : 3);
    p.bufA = b.off(wide * U0);
    p.bufB = b.off(wide * U0);
    p.x1 = b.off(U0);
    p.trans = b.off(U0);
    p.xs = b.off(U0);
    p.cr = b.off(U0);
    size_t gp = 0, wa = 0, wc = 0, fp = 0, wa3 = 0, wc3 = 0;
    p.ffab = p.wm = 0;
    if (vt.wmb_block) {      // no channel attention and no fold: `heads` is not read
        size_t ff = 0, wf = 0;
        for (int l = 0; l < 4; ++l) {
            const int C = c.dim << l, h2 = (H >> l) / 2, w2 = (W >> l) / 2;
            size_t f;
            RF_TRY(wm_workspace_floats("rf_workspace_bytes", 3 * B, C, h2, w2, &f));
            if (f > wf) wf = f;
            f = ffab_scratch_floats(B, C, h2, w2);
            if (f > ff) ff = f;
        }
        p.ffab = b.off(ff);
        p.wm = b.off(wf);
    }
    for (int l = 0; l < 4 && !vt.wmb_block; ++l) {
        const int C = c.dim << l, Pl = (H >> l) * (W >> l);
        int ns, sl;
        size_t pf;
        const int rc = gram_plan(B, C, c.heads[l], Pl, &ns, &sl, &pf);
        if (rc) return rc;
        if (pf > gp) gp = pf;
        if (fused_attn_supported(C, c.heads[l], H >> l, W >> l)) {
            size_t pf2, used;
            fused_attn_plan(H >> l, W >> l, &ns, &used, B, C, nullptr, &pf2);
            if (pf2 > gp) gp = pf2;
        }
        if (attn_mid_supported(C, c.heads[l], H >> l, W >> l)) {
            size_t pf2;
            attn_mid_plan(H >> l, W >> l, &ns, &pf2, B, C);
            if (pf2 > gp) gp = pf2;
        }
        const int hcl = C * c.ffn_expansion;
        // the channel_reduce fold; at a level whose FFN kernel carries the stage tail, [Wa' | Wb | Wb W2] in the same slot
        const bool tailf = !vt.branch_after && fused_ffn_tail_supported(C) && tail_composable(C, hcl);
        const size_t a = (size_t)B * packed1x1_floats(C, C), cr = (size_t)B * packed1x1_floats(tailf ? 2 * C + hcl : 2 * C, C);
        if (a > wa) wa = a;
        if (cr > wc) wc = cr;
        const size_t a3 = (size_t)B * packed1x1_b3_floats(C, C),
                     cr3 = (size_t)B * packed1x1_b3_floats(tail_composable(C, hcl) ? 2 * C + hcl : 2 * C, C);
        if (a3 > wa3) wa3 = a3;
        if (cr3 > wc3) wc3 = cr3;
        const size_t f = (size_t)B * (vt.branch_after ? tc_nblk(H >> l, W >> l) : flca_nblk(H >> l, W >> l)) * C;
        if (f > fp) fp = f;
    }
    p.gram_partial = b.off(gp);
    p.wfold_attn = b.off(wa);
    p.wfold_cr = b.off(wc);
    p.wfold_attn3 = b.off(wa3);
    p.wfold_cr3 = b.off(wc3);
    p.flca_partial = b.off(fp);
    p.ch = b.off((size_t)B * (c.dim << 3));
    p.ks_floats = 0;
    for (int l = 0; l < 4; ++l) {
        const size_t f = conv3x3_ksplit_floats(B, c.dim << l, H >> l, W >> l);
        if (f > p.ks_floats) p.ks_floats = f;
    }
    p.ks = b.off(p.ks_floats);
    p.total = b.used;
    return RF_OK;
}

// ---- one Conv_Transformer stage:  [fork] -> branch -> block -> [join] -> channel_reduce -> Conv_out -------------------------
// What every part of a stage reads: the level's sizes, the stage's buffers, the two streams, how the tail runs, and the
// arguments of the two launches the parts complete between them (the block's, channel_reduce's).
struct StageCtx {
    rf_handle* h;
    const StageIx& x;
    const Plan& p;
    float* ws;
    int stage, B, H, W, lvl, C, hh, ww, Pn, hc, heads;
    const float* in;
    float *xs, *trans, *crb;       // the branch's, the block's and channel_reduce's output
    hipStream_t st, side;          // the caller's stream and the branch's (== st when there is no second stream)
    bool compose, fuse_tail;       // run_stage
    const float* composed;         // [Wb W2 | b'] in the packed buffer when either is set
    float *fold_wp, *fold_wp3;     // where a branch's per-image fold writes channel_reduce's weights: the form(s) the tail reads
    TbParams tp;                   // TransformerBlock (rf_block.hip); unset under wmb_block
    Conv1x1Args r;                 // channel_reduce
};

// TransformerBlock: x + attn(LN1(x)), then x + ffn(LN2(x))  (rf_block.hip)
TbParams tb_params(const rf_handle* h, const StageIx& x) {
    TbParams tp{};
    tp.ln1_w = h->prm(x.ln1_w); tp.ln1_b = h->prm(x.ln1_b);
    tp.temperature = h->prm(x.temperature); tp.log_temperature = h->vt.log_temperature;
    tp.qkv_wp = h->pk(x.qkv_w); tp.qkv_b = h->prm(x.qkv_b);
    tp.qkv_dw_w = h->prm(x.qkv_dw_w); tp.qkv_dw_b = h->prm(x.qkv_dw_b);
    tp.proj_w = h->prm(x.proj_w); tp.proj_b = h->prm(x.proj_b);
    tp.ln2_w = h->prm(x.ln2_w); tp.ln2_b = h->prm(x.ln2_b);
    tp.pw1_wp = h->pk(x.pw1_w); tp.pw1_b = h->prm(x.pw1_b);
    tp.dw_w = h->prm(x.dw_w); tp.dw_b = h->prm(x.dw_b);
    tp.pw2_wp = h->pk(x.pw2_w); tp.pw2_b = h->prm(x.pw2_b);
    tp.qkv_wp3 = h->pk3(x.qkv_w); tp.pw1_wp3 = h->pk3(x.pw1_w); tp.pw2_wp3 = h->pk3(x.pw2_w);
    if (h->shard_allreduce) {      // spatial shard: this level's interior rows and columns
        tp.ylo = h->shard_y_lo >> x.lvl; tp.yhi = h->shard_y_hi >> x.lvl; tp.xlo = h->shard_x_lo >> x.lvl; tp.xhi = h->shard_x_hi >> x.lvl;
        tp.allreduce = h->shard_allreduce; tp.allreduce_user = h->shard_user;
    }
    return tp;
}

TbBufOffsets tb_bufs(const Plan& p) { return {p.bufA, p.bufB, p.x1, p.gram_partial, p.wfold_attn, p.wfold_attn3}; }

// the stage's block in one piece, in -> trans: WMB, or the TransformerBlock
int run_block(const StageCtx& c) {
    const Plan& p = c.p;
    float* ws = c.ws;
    if (!c.h->vt.wmb_block) return run_transformer(c.tp, c.in, c.trans, ws, tb_bufs(p), c.B, c.C, c.heads, c.hc, c.hh, c.ww, c.st);
    // t in the x1 slot, the bands in tU (idle inside a stage), the quarter-size illumination tensors at the head of bufA until
    // project_in writes the hidden tensor there
    const size_t U = (size_t)c.B * c.C * c.Pn;
    const WmbBufs wb{ws + p.x1, ws + p.tU, ws + p.bufA, ws + p.bufA + U, ws + p.bufA, ws + p.bufB, ws + p.ffab, ws + p.wm};
    return run_wmb(c.h, c.stage, c.in, c.trans, wb, c.B, c.hh, c.ww, c.st);
}

// channel_reduce reads the weights a branch folded per image into the workspace (its squeeze-excite gate: launch_flca_se_fold)
int fold_cr(StageCtx& c, const float* partial, int nblk, int P_pool, const SePrm& se, hipStream_t st) {
    const Plan& p = c.p;
    RF_TRY(launch_flca_se_fold(partial, nblk, P_pool, se, c.h->prm(c.x.cr_w), c.fold_wp, c.fold_wp3, c.ws + p.ch, c.B, c.C, st, c.composed, c.hc));
    c.r.wp = c.ws + p.wfold_cr; c.r.wp_bstride = (int64_t)packed1x1_floats(2 * c.C, c.C);
    c.r.wp3 = c.ws + p.wfold_cr3; c.r.wp3_bstride = (int64_t)packed1x1_b3_floats(c.compose ? 2 * c.C + c.hc : 2 * c.C, c.C);
    return RF_OK;
}

// res_proj of the TrueColor and multi-level branches:  src -> res_proj.0, ReLU -> mid -> res_proj.2 -> dst
void res_proj_pair(const StageCtx& c, int w0, int b0, int w2, int b2, const float* src, float* mid, float* dst, Conv1x1Args& r0, Conv1x1Args& r2) {
    const rf_handle* h = c.h;
    r0 = conv1x1_dense(src, c.C, h->pk(w0), h->pk3(w0), h->prm(b0), mid, c.C, c.B, c.Pn, c.ww);
    r0.act = 2;
    r2 = conv1x1_dense(mid, c.C, h->pk(w2), h->pk3(w2), h->prm(b2), dst, c.C, c.B, c.Pn, c.ww);
}

// The branches.  Each leaves its output in xs and tells channel_reduce (c.r) where its weights are: the static pack, or the
// per-image fold in the workspace (fold_cr).  BR_CONV and BR_FLCA run on the branch stream, BR_TC and BR_ML after the block on st.
int branch_conv(StageCtx& c) {      // plain and wfb: one 3x3 convolution, one shared set of channel_reduce weights
    const rf_handle* h = c.h;
    const StageIx& x = c.x;
    const Conv3x3Args cb = conv3x3_dense(c.in, h->pk(x.conv_w), h->prm(x.conv_b), c.xs, c.B, c.C, c.C, c.hh, c.ww, h->cfg.branch_lrelu ? 1 : 0);
    RF_TRY(launch_conv3x3(cb, c.side));
    // the fused FFN reads [Wa | Wb | Wb W2] in f32 operand order from the fold slot, folded per call: the packed buffer has no room for it
    if (c.fuse_tail) RF_TRY(launch_tail_fold(h->prm(x.cr_w), nullptr, c.composed, nullptr, 1, c.C, c.hc, c.side, c.fold_wp));
    c.r.wp = h->pk(x.cr_w);
    c.r.wp3 = c.compose ? h->packed + x.tail3_offset : h->pk3(x.cr_w);
    return RF_OK;
}

int branch_flca(StageCtx& c) {
    rf_handle* h = c.h;
    const Plan& p = c.p;
    const FlcaPrm fp = h->flca_prm(c.x.flca);
    const bool sharded = h->shard_allreduce != nullptr;
    FlcaSpatialArgs s{};
    s.feat = c.in; s.xs = c.xs; s.guide = c.ws + p.guide[c.lvl];
    s.set_params(fp);
    s.partial = c.ws + p.flca_partial; s.B = c.B; s.C = c.C; s.h = c.hh; s.w = c.ww; s.nblk = flca_nblk(c.hh, c.ww);
    s.ylo = c.tp.ylo; s.yhi = c.tp.yhi; s.xlo = c.tp.xlo; s.xhi = c.tp.xhi;
    RF_TRY(launch_flca_spatial(s, c.side));
    if (sharded) h->shard_allreduce(h->shard_user, s.partial, (size_t)c.B * s.nblk * c.C, 0, (void*)c.side);
    // the pooled mean is over the frame's pixels, not the window's
    const int P_pool = sharded ? (h->shard_total_rows >> c.lvl) * (h->shard_total_cols ? h->shard_total_cols >> c.lvl : c.ww) : c.Pn;
    c.tp.tail.wp_bstride = (int64_t)packed1x1_floats(2 * c.C + c.hc, c.C);      // the fused tail's weights are per image too
    return fold_cr(c, s.partial, s.nblk, P_pool, fp.se, c.side);
}

// EnhancedFLCA (BayerTORGBColorMultiLvl.py:249-293): spatial gate -> x + 0.2 tanh(res_proj(x)) -> squeeze-excite (folded into
// channel_reduce like the FLCA variant's); r0 writes crb, r2 bufA
int branch_tc(StageCtx& c) {
    const rf_handle* h = c.h;
    const Plan& p = c.p;
    const TcIx& t = c.x.tc;
    float* ws = c.ws;
    RF_TRY(launch_tc_spatial(c.in, c.xs, ws + p.guide[c.lvl], h->prm(t.col_w), h->prm(t.col_b), h->prm(t.low_w), h->prm(t.low_b), h->prm(t.high_w),
                             h->prm(t.high_b), c.B, c.C, c.hh, c.ww, c.st));
    Conv1x1Args r0, r2;
    res_proj_pair(c, t.res0_w, t.res0_b, t.res2_w, t.res2_b, c.xs, c.crb, ws + p.bufA, r0, r2);
    RF_TRY(launch_conv1x1(r0, c.st));
    RF_TRY(launch_conv1x1(r2, c.st));
    RF_TRY(launch_tc_residual(c.xs, ws + p.bufA, c.xs, ws + p.flca_partial, c.B, c.C, c.hh, c.ww, c.st));
    return fold_cr(c, ws + p.flca_partial, tc_nblk(c.hh, c.ww), c.Pn, h->se_prm(t.se), c.st);
}

// FLCA_Pyramid (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:132-183): for every pyramid level and then for the chroma
// planes  x <- x + 0.2 tanh(res_proj(x * gated spatial attention)),  one res_proj for all steps; squeeze-excite folded into
// channel_reduce.  A composed step is modulate -> 1x1 (ReLU) -> 1x1 -> residual; the last one leaves the pooling sums.
int branch_ml(StageCtx& c) {
    const rf_handle* h = c.h;
    const Plan& p = c.p;
    const MlIx& m = c.x.ml;
    float* ws = c.ws;
    const int B = c.B, C = c.C, hh = c.hh, ww = c.ww, L = h->vt.levels;
    const float* means = ml_level_means(ws + p.gscratch, c.lvl, B, c.H, c.W, L);
    float* t1 = ws + p.bufA;
    float* t2 = t1 + (size_t)B * C * c.Pn;
    Conv1x1Args r0, r2;
    res_proj_pair(c, m.res0_w, m.res0_b, m.res2_w, m.res2_b, c.crb, t1, t2, r0, r2);
    // level 0 (C = dim <= 64, the largest tensor): one kernel per step, nothing but x and the result in HBM
    bool fused_step = ml_step_fused_supported(C, hh, ww);
#ifdef RF_DIAG   // diagnostic build only: the composed steps everywhere
    if (getenv("RF_NO_ML_FUSED")) fused_step = false;
#endif
    const float* cur = c.in;
    for (int s = 0; s <= L; ++s) {
        const bool chroma = s == L;
        const float* w_a = h->prm(chroma ? m.chr_w : m.low_w[s]);
        const float* w_b = chroma ? nullptr : h->prm(m.high_w[s]);
        const float* g_w = h->prm(chroma ? m.cgate_w : m.gate_w[s]);
        const float* g_b = h->prm(chroma ? m.cgate_b : m.gate_b[s]);
        if (fused_step) {
            RF_TRY(launch_ml_step_fused(cur, c.xs, ws + p.guide[c.lvl], means, s, L, w_a, w_b, g_w, g_b, h->prm(m.res0_w), h->prm(m.res0_b),
                                        h->prm(m.res2_w), h->prm(m.res2_b), chroma ? ws + p.flca_partial : nullptr, B, C, hh, ww, c.st));
        } else {
            RF_TRY(launch_ml_modulate(cur, c.crb, ws + p.guide[c.lvl], means, s, L, w_a, w_b, g_w, g_b, B, C, hh, ww, c.st));
            RF_TRY(launch_conv1x1(r0, c.st));
            RF_TRY(launch_conv1x1(r2, c.st));
            if (chroma) RF_TRY(launch_tc_residual(cur, t2, c.xs, ws + p.flca_partial, B, C, hh, ww, c.st));   // the last step: + pooling sums
            else RF_TRY(launch_ml_residual(cur, t2, c.xs, B, C, hh, ww, c.st));
        }
        cur = c.xs;
    }
    return fold_cr(c, ws + p.flca_partial, tc_nblk(hh, ww), c.Pn, h->se_prm(m.se), c.st);
}

int run_stage(rf_handle* h, int i, const float* in, float* out, float* ws, const Plan& p,
              int B, int H, int W, hipStream_t st, hipStream_t side) {
    const VariantTraits& vt = h->vt;
    const StageIx& x = h->stage[i];
    const int lvl = x.lvl, C = h->cfg.dim << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww, hc = C * h->cfg.ffn_expansion;
    StageCtx c{h, x, p, ws, i, B, H, W, lvl, C, hh, ww, Pn, hc, h->cfg.heads[lvl], in, ws + p.xs, ws + p.trans, ws + p.cr, st, side};
    if (!vt.wmb_block) c.tp = tb_params(h, x);
    // Composed tail: where the FFN runs op by op, its last GEMM (x1 + W2 g + b2 -> trans, K = hidden) and channel_reduce
    // ([Wa' | Wb] [xs ; trans], K = 2C) become ONE GEMM over [xs ; x1 ; g] with [Wa' | Wb | Wb W2] (same MFMA count; `trans` --
    // C floats per pixel written and read back -- never exists).  The bias and Wb W2 are composed at parameter load.
    const bool ffn_fused = !vt.wmb_block && transformer_ffn_is_fused(c.tp, C, hc, hh, ww);
    c.compose = x.tail_offset != 0 && Pn % 4 == 0 && !ffn_fused;
    // Fused tail: where the FFN is ffn_fused_kernel<32> (level 0), the same composition runs INSIDE it -- xs and x1 are 16 more
    // k-steps of its second GEMM, Wb W2 replaces W2 -- so neither `trans` nor the channel_reduce launch exists.  The kernel reads
    // the weights in f32 operand order from the fold slot of the workspace (per image: the FLCA gate; one set for the conv
    // branch).  Not where the branch runs after the block.
    c.fuse_tail = x.tail_offset != 0 && ffn_fused && fused_ffn_tail_supported(C) && !vt.branch_after;
#ifdef RF_DIAG   // diagnostic build only: the two-GEMM form
    if (getenv("RF_NO_COMPOSE") || getenv("RF_NO_B3")) c.compose = false;
    if (getenv("RF_NO_COMPOSE")) c.fuse_tail = false;
#endif
    c.tp.defer_pw2 = c.compose;
    c.composed = c.compose || c.fuse_tail ? h->packed + x.tail_offset : nullptr;
    c.fold_wp = c.compose ? nullptr : ws + p.wfold_cr;
    c.fold_wp3 = c.fuse_tail ? nullptr : ws + p.wfold_cr3;
    if (c.fuse_tail) { c.tp.tail.xs = c.xs; c.tp.tail.wp = c.fold_wp; c.tp.tail_bias = c.composed + (size_t)C * hc; }
    c.r = conv1x1_dense(c.xs, C, nullptr, nullptr, h->prm(x.cr_b), c.crb, C, B, Pn, ww);
    c.r.x2 = c.trans; c.r.C2 = C; c.r.x2_bstride = (int64_t)C * Pn;
    // Composed tail with the depthwise 3x3 + GELU inside the GEMM (conv1x1_b3_dw3_kernel; cfg2: level 1): where plan_conv1x1 takes
    // that form for the GEMM of `compose`, the block stops after pointwise1 and the GEMM reads the hidden tensor from bufA.  The
    // plan looks at shapes, presence and alignment only, so the weights the branch has yet to name stand in as the packed buffer.
    const Conv1x1Dw3 dw3{c.tp.dw_w, c.tp.dw_b, hh, ww};
    bool tail_dw = false;
    if (c.compose && !vt.branch_after) {      // (a branch that follows the block borrows bufA)
        Conv1x1Args probe = c.r;
        probe.x2 = ws + p.x1;
        probe.x3 = ws + p.bufA; probe.C3 = hc; probe.x3_bstride = (int64_t)hc * Pn;
        probe.wp3 = h->packed;
        Conv1x1Plan pl;
        RF_TRY(plan_conv1x1(probe, &pl, &dw3));
        tail_dw = pl.dw3;
    }
    c.tp.defer_dw = tail_dw;

    // the branch is launched first (on the branch stream when there is one), the block beside it; a branch that borrows bufA
    // follows the block on the same stream instead
    if (vt.branch_after) RF_TRY(run_block(c));
    else RF_TRY(h->side.fork(st, side));
    int rc = RF_E_INVALID;
    switch (vt.branch) {
    case BR_CONV: rc = branch_conv(c); break;
    case BR_FLCA: rc = branch_flca(c); break;
    case BR_TC: rc = branch_tc(c); break;
    case BR_ML: rc = branch_ml(c); break;
    }
    if (rc) return rc;
    if (c.fuse_tail) {
        // the FFN kernel reads the branch's output and weights, and writes channel_reduce's: the join sits between the block's halves.
        // Where fused_ffn_proj_rule holds it applies the attention projection as well: the attention half stops after the fold, and
        // x1 never reaches HBM.
        FfnProj pj{};
        FfnProj* const proj = fused_ffn_proj_rule(lvl, hh, ww) ? &pj : nullptr;
        RF_TRY(run_transformer_attn(c.tp, in, ws, tb_bufs(p), B, C, c.heads, hh, ww, st, proj));
        RF_TRY(h->side.join(st, side));
        RF_TRY(run_transformer_ffn(c.tp, c.crb, ws, tb_bufs(p), B, C, hc, hh, ww, st, in, proj));
    } else if (!vt.branch_after) {
        RF_TRY(run_block(c));
        RF_TRY(h->side.join(st, side));
    }
    if (c.compose) {
        c.r.wp = nullptr;
        c.r.x2 = ws + p.x1;
        c.r.x3 = ws + (tail_dw ? p.bufA : p.bufB); c.r.C3 = hc; c.r.x3_bstride = (int64_t)hc * Pn;
        c.r.bias = c.composed + (size_t)C * hc;
    }
    if (!c.fuse_tail) RF_TRY(launch_conv1x1(c.r, st, tail_dw ? &dw3 : nullptr));

    Conv3x3Args co = conv3x3_dense(c.crb, h->pk(x.out_w), h->prm(x.out_b), out, B, C, C, hh, ww, 1);
    if (p.ks_floats) { co.ks_scratch = ws + p.ks; co.ks_floats = p.ks_floats; }
    return launch_conv3x3(co, st);
}

// The guidance pyramid of the branches, every level (lvl < 0: rf_forward, where a shard all-reduces the frame's maximum) or one.
// FLCA's feeds the branches only: it runs on their stream, beside the embedding.
int run_guidance(rf_handle* h, const float* in, int mosaic, int lvl, float* ws, const Plan& p, int B, int H, int W, hipStream_t st, hipStream_t side) {
    const VariantTraits& vt = h->vt;
    const int l0 = lvl < 0 ? 0 : lvl, l1 = lvl < 0 ? 3 : lvl;
    float* gs = ws + p.gscratch;
    switch (vt.branch) {
    case BR_CONV: break;
    case BR_FLCA:
        RF_TRY(h->side.fork(st, side));
        RF_TRY(launch_guidance_base(in, mosaic, h->cfg.clamp_io, gs, B, H, W, side, lvl < 0 ? h->shard_allreduce : nullptr, lvl < 0 ? h->shard_user : nullptr));
        for (int l = l0; l <= l1; ++l) RF_TRY(launch_guidance_level(gs, ws + p.guide[l], B, H, W, H >> l, W >> l, side));
        break;
    case BR_TC: {
        const BayerProcIx& bp = h->bp;
        RF_TRY(launch_tc_front(in, mosaic, h->prm(bp.wb_gains), h->prm(bp.color_matrix), h->pk(bp.ce0_w), h->prm(bp.ce0_b), h->pk(bp.ce2_w),
                               h->prm(bp.ce2_b), h->pk(bp.dm0_w), h->prm(bp.dm0_b), h->pk(bp.dm2_w), h->prm(bp.dm2_b), gs, B, H, W, vt.levels, st));
        for (int l = l0; l <= l1; ++l) RF_TRY(launch_tc_guide_level(gs, ws + p.guide[l], B, H, W, vt.levels, H >> l, W >> l, st));
        break;
    }
    case BR_ML:
        RF_TRY(launch_ml_guidance(in, mosaic, gs, B, H, W, vt.levels, st));
        for (int l = l0; l <= l1; ++l) RF_TRY(launch_ml_guide_level(gs, ws + p.guide[l], l, B, H, W, vt.levels, H >> l, W >> l, st));
        break;
    }
    return RF_OK;
}

// conv_out + LeakyReLU + PixelShuffle (+ clamp), then what the variant does to the image
int run_output(rf_handle* h, const float* in, int mosaic, const float* x, float* out, float* ws, const Plan& p, int B, int H, int W, hipStream_t st) {
    const rf_config& cfg = h->cfg;
    const BranchKind br = h->vt.branch;
    // TrueColor: F.relu before the PixelShuffle (BayerTORGBColorMultiLvl.py:458)
    Conv3x3Args o = conv3x3_dense(x, h->pk(h->conv_out_w), h->prm(h->conv_out_b), out, B, cfg.dim, 4 * cfg.out_channels, H, W, br == BR_TC ? 2 : 1);
    o.store = 2; o.clamp_out = cfg.clamp_io;
    RF_TRY(launch_conv3x3(o, st));
    if (br == BR_TC) {
        const ColorCorrIx& cc = h->cc;
        const float* prm[9] = {h->prm(cc.gamma),   h->prm(cc.ct0_w),   h->prm(cc.ct0_b),   h->prm(cc.ct2_w),  h->prm(cc.ct2_b),
                               h->prm(cc.tone0_w), h->prm(cc.tone0_b), h->prm(cc.tone2_w), h->prm(cc.tone2_b)};
        return launch_tc_color_head(out, prm, B, (size_t)4 * H * W, st);
    }
    // colour anchor and luminance nudge (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:403-414)
    return br == BR_ML ? launch_ml_tail(out, in, mosaic, ws + p.gscratch, B, H, W, h->vt.levels, st) : RF_OK;
}

// Sizes the WFB variant admits (packed H x W), checked before any launch.  Level 3 works on H/8 x W/8 and its LL band on
// H/16 x W/16: the DWT needs even sizes there, FFAB at least 2 rows and an even width, the vector kernels widths in multiples of 4.
// The FFT of the level-0 LL band (H/2 x W/2) has rf_fft.hip's line limits; every lower level halves them.
int wfb_check_size(const char* who, int H, int W) {
    RF_CHECK_ARG(H % 16 == 0, "%s: variant wfb: packed height %d must be a multiple of 16 (the Haar DWT at U-Net level 3)", who, H);
    RF_CHECK_ARG(H >= 32, "%s: variant wfb: packed height %d must be at least 32 (FFAB needs 2 rows of the level-3 LL band)", who, H);
    RF_CHECK_ARG(W % 32 == 0, "%s: variant wfb: packed width %d must be a multiple of 32 (an even level-3 LL band for FFAB's rfft2)", who, W);
    for (int n : {H / 2, W / 2}) {
        RF_CHECK_ARG(n <= 4096, "%s: variant wfb: a line of %d samples in the level-0 LL band exceeds the FFT's 4096", who, n);
        RF_CHECK_ARG((n & (n - 1)) == 0 || n <= 2048, "%s: variant wfb: a line of %d samples in the level-0 LL band is no power of two and exceeds 2048",
                     who, n);
    }
    return RF_OK;
}
// What rf_workspace_bytes, rf_forward_stage and rf_forward check alike, and the plan.  workspace == nullptr: rf_workspace_bytes,
// which sizes only (and, as ever, sets no limit on B).
int check_call(const char* who, const rf_handle* h, const void* in, const void* out, const void* workspace, size_t workspace_bytes,
               int B, int H, int W, Plan& p) {
    RF_CHECK_ARG(B > 0 && (B <= 65535 || !workspace) && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
                 "%s: packed size %dx%d must be positive multiples of 8 (mosaic divisible by 16)", who, H, W);
    if (h->vt.wmb_block) RF_TRY(wfb_check_size(who, H, W));
    if (workspace) {
        if (!h->packed) {
            set_error("%s: parameters not packed (call rf_pack_params after rf_set_param)", who);
            return RF_E_MISSING;
        }
        RF_CHECK_ARG(aligned16(workspace) && aligned16(in) && aligned16(out), "%s: buffers must be 16-byte aligned", who);
    }
    RF_TRY(make_plan(h, B, H, W, p));
    if (workspace && workspace_bytes < p.total * sizeof(float)) {
        set_error("%s: workspace of %zu bytes, need %zu", who, workspace_bytes, p.total * sizeof(float));
        return RF_E_NOMEM;
    }
    return RF_OK;
}

}  // namespace

// ---- second stream (rf_handle.h) ----------------------------------------------------------
hipStream_t SideStream::get(hipStream_t st) {
    if (failed || profiling_active()) return st;       // the per-kernel profiling brackets assume one stream
    if (!stream &&
        (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess ||
         hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess)) {
        (void)hipGetLastError();
        destroy();
        failed = true;          // no second stream: the single-stream schedule is always valid
        return st;
    }
    return stream;
}

int SideStream::fork(hipStream_t st, hipStream_t side) {
    if (side == st) return RF_OK;
    pending = true;
    ++forks;
    RF_TRY(check_hip(hipEventRecord(ev_fork, st), "side stream fork (record)"));
    RF_TRY(check_hip(hipStreamWaitEvent(side, ev_fork, 0), "side stream fork (wait)"));
#ifdef RF_DIAG   // diagnostic build only: the n-th fork of a call fails after it has been enqueued
    const char* n = getenv("RF_FAIL_FORK");
    if (n && forks == atoi(n)) {
        set_error("RF_FAIL_FORK=%s: injected failure of fork %d", n, forks);
        return RF_E_DEVICE;
    }
#endif
    return RF_OK;
}

int SideStream::join(hipStream_t st, hipStream_t side) {
    if (side == st) return RF_OK;
    RF_TRY(check_hip(hipEventRecord(ev_join, side), "side stream join (record)"));
    RF_TRY(check_hip(hipStreamWaitEvent(st, ev_join, 0), "side stream join (wait)"));
    pending = false;
    return RF_OK;
}

void SideStream::destroy() {
    if (stream) (void)hipStreamDestroy(stream);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    stream = nullptr;
    ev_fork = ev_join = nullptr;
}

// An event record and wait are legal inside a stream capture, a host synchronise is not: the fallback is for a failed record
// or wait only.  rf_last_error keeps the call's own error.
void SideStream::join_pending(hipStream_t st) {
    if (!pending) return;
    if (hipEventRecord(ev_join, stream) != hipSuccess || hipStreamWaitEvent(st, ev_join, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream);
    }
    pending = false;
}
extern "C" {

int rf_workspace_bytes(const rf_handle* h, int B, int H, int W, size_t* bytes) {
    RF_CHECK_ARG(h && bytes, "rf_workspace_bytes: null argument");
    Plan p;
    RF_TRY(check_call("rf_workspace_bytes", h, nullptr, nullptr, nullptr, 0, B, H, W, p));
    *bytes = p.total * sizeof(float);
    return RF_OK;
}

// the one place that writes the shard state: rf_set_shard is the all-columns case (x_lo = x_hi = total_cols = 0)
static int set_shard_state(rf_handle* h, const char* who, int y_lo, int y_hi, int total_rows, int x_lo, int x_hi, int total_cols,
                           rf_allreduce_fn allreduce, void* user) {
    RF_CHECK_ARG(h, "%s: null handle", who);
    if (!allreduce) {
        h->shard_y_lo = h->shard_y_hi = h->shard_total_rows = 0;
        h->shard_x_lo = h->shard_x_hi = h->shard_total_cols = 0;
        h->shard_allreduce = nullptr; h->shard_user = nullptr;
        return RF_OK;
    }
    RF_CHECK_ARG(h->vt.shardable, "%s: variants flca and plain only", who);
    RF_CHECK_ARG(y_lo >= 0 && y_hi > y_lo && y_lo % 8 == 0 && y_hi % 8 == 0 && total_rows >= y_hi - y_lo && total_rows % 8 == 0,
                 "%s: interior rows [%d, %d) of %d must be multiples of 8", who, y_lo, y_hi, total_rows);
    // columns: cuts on multiples of 32 keep the bounds of every level (>> 3 at the coarsest) on the kernels' groups of 4 pixels;
    // x_hi may instead be the window's width (the frame's right border), which rf_forward checks when it knows the width
    RF_CHECK_ARG(x_lo >= 0 && x_lo % 32 == 0 && x_hi % 8 == 0 && (x_hi == 0 ? x_lo == 0 && total_cols == 0 : x_hi > x_lo) &&
                     total_cols >= x_hi - x_lo && total_cols % 8 == 0,
                 "%s: interior columns [%d, %d) of %d: x_lo must be a multiple of 32, x_hi of 32 or the window's width, the total of 8",
                 who, x_lo, x_hi, total_cols);
    h->shard_y_lo = y_lo; h->shard_y_hi = y_hi; h->shard_total_rows = total_rows;
    h->shard_x_lo = x_lo; h->shard_x_hi = x_hi; h->shard_total_cols = total_cols;
    h->shard_allreduce = allreduce; h->shard_user = user;
    return RF_OK;
}

int rf_set_shard(rf_handle* h, int y_lo, int y_hi, int total_rows, rf_allreduce_fn allreduce, void* user) {
    return set_shard_state(h, "rf_set_shard", y_lo, y_hi, total_rows, 0, 0, 0, allreduce, user);
}

int rf_set_shard_grid(rf_handle* h, int y_lo, int y_hi, int total_rows, int x_lo, int x_hi, int total_cols,
                      rf_allreduce_fn allreduce, void* user) {
    RF_CHECK_ARG(!allreduce || (x_hi > 0 && total_cols > 0), "rf_set_shard_grid: interior columns [%d, %d) of %d must not be empty",
                 x_lo, x_hi, total_cols);
    return set_shard_state(h, "rf_set_shard_grid", y_lo, y_hi, total_rows, x_lo, x_hi, total_cols, allreduce, user);
}
int rf_forward_stage(rf_handle* h, int stage, const float* in, const float* packed, float* out, void* workspace,
                     size_t workspace_bytes, int B, int H, int W, void* stream) {
    RF_CHECK_ARG(h && in && out && workspace && stage >= 1 && stage <= 7, "rf_forward_stage: bad arguments (stage 1..7)");
    const VariantTraits& vt = h->vt;
    RF_CHECK_ARG(!vt.stage_needs_packed_frame || packed, "rf_forward_stage: the FLCA branch needs the packed frame for its guidance");
    Plan p;
    RF_TRY(check_call("rf_forward_stage", h, in, out, workspace, workspace_bytes, B, H, W, p));
    RF_CHECK_ARG(vt.branch != BR_ML || aligned16(packed), "rf_forward_stage: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    RF_TRY(run_guidance(h, packed, 0, h->stage[stage].lvl, ws, p, B, H, W, st, st));
    if (p.ks_floats) RF_TRY(check_hip(hipMemsetAsync(ws + p.ks, 0, conv3x3_ksplit_counter_bytes(), st), "rf_forward_stage: memset"));
    return run_stage(h, stage, in, out, ws, p, B, H, W, st, st);
}

int rf_tc_guidance(rf_handle* h, const float* packed, int level, float* y, float* crcb, float* rgb, float* guide, void* workspace,
                   size_t workspace_bytes, int B, int H, int W, void* stream) {
    RF_CHECK_ARG(h && packed && y && crcb && rgb && guide && workspace, "rf_tc_guidance: null argument");
    RF_CHECK_ARG(h->vt.branch == BR_TC, "rf_tc_guidance: the TrueColor variant only");
    RF_CHECK_ARG(level >= 0 && level <= 3, "rf_tc_guidance: U-Net level %d (0..3)", level);
    Plan p;
    RF_TRY(check_call("rf_tc_guidance", h, packed, guide, workspace, workspace_bytes, B, H, W, p));
    RF_CHECK_ARG(aligned16(y) && aligned16(crcb) && aligned16(rgb), "rf_tc_guidance: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    RF_TRY(run_guidance(h, packed, 0, level, ws, p, B, H, W, st, st));
    const float *sy, *scrcb, *srgb;
    RF_TRY(tc_front_outputs(ws + p.gscratch, &sy, &scrcb, &srgb, B, H, W, h->vt.levels));
    const size_t hw = (size_t)H * W, f = sizeof(float);
    // y is plane 3 of cin4 [B,4,H,W]: one row of hw floats per image, 4 hw apart
    RF_TRY(check_hip(hipMemcpy2DAsync(y, hw * f, sy, 4 * hw * f, hw * f, (size_t)B, hipMemcpyDeviceToDevice, st), "rf_tc_guidance: copy y"));
    RF_TRY(check_hip(hipMemcpyAsync(crcb, scrcb, (size_t)B * 2 * hw * f, hipMemcpyDeviceToDevice, st), "rf_tc_guidance: copy crcb"));
    RF_TRY(check_hip(hipMemcpyAsync(rgb, srgb, (size_t)B * 3 * hw * f, hipMemcpyDeviceToDevice, st), "rf_tc_guidance: copy rgb"));
    return check_hip(hipMemcpyAsync(guide, ws + p.guide[level], (size_t)B * 7 * (H >> level) * (W >> level) * f, hipMemcpyDeviceToDevice, st),
                     "rf_tc_guidance: copy guide");
}

int rf_ml_guidance(rf_handle* h, const float* packed, int level, float* guide, float* means, void* workspace, size_t workspace_bytes,
                   int B, int H, int W, void* stream) {
    RF_CHECK_ARG(h && packed && guide && means && workspace, "rf_ml_guidance: null argument");
    RF_CHECK_ARG(h->vt.branch == BR_ML, "rf_ml_guidance: the multi-level variant only");
    RF_CHECK_ARG(level >= 0 && level <= 3, "rf_ml_guidance: U-Net level %d (0..3)", level);
    Plan p;
    RF_TRY(check_call("rf_ml_guidance", h, packed, guide, workspace, workspace_bytes, B, H, W, p));
    RF_CHECK_ARG(aligned16(means), "rf_ml_guidance: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int L = h->vt.levels;
    RF_TRY(run_guidance(h, packed, 0, level, ws, p, B, H, W, st, st));
    const size_t f = sizeof(float);
    RF_TRY(check_hip(hipMemcpyAsync(guide, ws + p.guide[level], (size_t)B * (2 * L + 2) * (H >> level) * (W >> level) * f, hipMemcpyDeviceToDevice, st),
                     "rf_ml_guidance: copy guide"));
    return check_hip(hipMemcpyAsync(means, ml_level_means(ws + p.gscratch, level, B, H, W, L), (size_t)B * 8 * f, hipMemcpyDeviceToDevice, st),
                     "rf_ml_guidance: copy means");
}

int rf_ml_tail(rf_handle* h, float* image, const float* in, int packed_input, void* workspace, size_t workspace_bytes, int B, int H, int W,
               void* stream) {
    RF_CHECK_ARG(h && image && in && workspace, "rf_ml_tail: null argument");
    RF_CHECK_ARG(h->vt.branch == BR_ML, "rf_ml_tail: the multi-level variant only");
    RF_CHECK_ARG((size_t)H * W < (1u << 30), "rf_ml_tail: frame too large");
    Plan p;
    RF_TRY(check_call("rf_ml_tail", h, in, image, workspace, workspace_bytes, B, H, W, p));
    hipStream_t st = (hipStream_t)stream;
    float* gs = (float*)workspace + p.gscratch;
    const int mosaic = packed_input ? 0 : 1;
    RF_TRY(launch_ml_guidance(in, mosaic, gs, B, H, W, h->vt.levels, st));
    return launch_ml_tail(image, in, mosaic, gs, B, H, W, h->vt.levels, st);
}

int rf_forward(rf_handle* h, const float* in, float* out, void* workspace, size_t workspace_bytes,
               int B, int H, int W, int packed_input, void* stream) {
    RF_CHECK_ARG(h && in && out && workspace, "rf_forward: null argument");
    RF_CHECK_ARG((size_t)H * W < (1u << 30), "rf_forward: frame too large");
    RF_CHECK_ARG(!h->shard_allreduce || h->shard_y_hi <= H, "rf_forward: shard interior [%d, %d) outside the %d-row window",
                 h->shard_y_lo, h->shard_y_hi, H);
    RF_CHECK_ARG(!h->shard_allreduce || h->shard_x_hi == W || (h->shard_x_hi < W && h->shard_x_hi % 32 == 0),
                 "rf_forward: shard interior columns [%d, %d) must end on a multiple of 32 inside the %d-column window or at its width",
                 h->shard_x_lo, h->shard_x_hi, W);
    Plan p;
    RF_TRY(check_call("rf_forward", h, in, out, workspace, workspace_bytes, B, H, W, p));
    hipStream_t st = (hipStream_t)stream;
    SideJoinGuard joined(h->side, st);
    float* ws = (float*)workspace;
    const int d = h->cfg.dim;
    const int mosaic = packed_input ? 0 : 1;

    // A stage's branch (FLCA gates + squeeze-excite fold, or the 3x3 conv) depends on the stage input only, like the block beside
    // it; so does the guidance pyramid at the head of the forward.  On a single frame every kernel of both chains is a few dozen
    // microseconds of mostly latency, so the branch runs on the handle's second stream, forked before it and joined before
    // channel_reduce.  Not for a spatial shard (its collectives stay on the caller's stream) nor where the branch shares bufA with
    // the block and follows it.
    bool use_side = !h->shard_allreduce && !h->vt.branch_after;
#ifdef RF_DIAG   // diagnostic build only: everything on the caller's stream
    if (getenv("RF_NO_SIDE")) use_side = false;
#endif
    const hipStream_t side = use_side ? h->side.get(st) : st;
    if (p.ks_floats)      // tickets of the 3x3 convs' input-channel split (the kernels leave them zero; the workspace is the caller's)
        RF_TRY(check_hip(hipMemsetAsync(ws + p.ks, 0, conv3x3_ksplit_counter_bytes(), st), "rf_forward: memset"));
    RF_TRY(run_guidance(h, in, mosaic, -1, ws, p, B, H, W, st, side));
    // embedding (reads the mosaic through the Bayer pack)
    Conv3x3Args e = conv3x3_dense(in, h->pk(h->embedding_w), h->prm(h->embedding_b), ws + p.tA, B, 4, d, H, W, 0);
    e.unshuffle_in = mosaic; e.clamp_in = h->cfg.clamp_io;
    RF_TRY(launch_conv3x3(e, st));

    // encoder
    float* skip[3] = {ws + p.skip[0], ws + p.skip[1], ws + p.skip[2]};
    for (int i = 1; i <= 3; ++i) {
        const int lvl = i - 1, C = d << lvl;
        RF_TRY(run_stage(h, i, ws + p.tA, skip[lvl], ws, p, B, H, W, st, side));
        Conv3x3Args dn = conv3x3_dense(skip[lvl], h->pk(h->down_w[i - 1]), nullptr, ws + p.tA, B, C, C / 2, H >> lvl, W >> lvl, 0);
        dn.store = 1;
        if (p.ks_floats) { dn.ks_scratch = ws + p.ks; dn.ks_floats = p.ks_floats; }
        RF_TRY(launch_conv3x3(dn, st));
    }
    RF_TRY(run_stage(h, 4, ws + p.tA, ws + p.tB, ws, p, B, H, W, st, side));
    // decoder
    for (int i = 1; i <= 3; ++i) {
        const int lvl = 3 - i, C = d << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww;
        bool fuse_up = upcat_supported(C, hh / 2, ww / 2, ws + p.tB, skip[lvl], ws + p.tA);
#ifdef RF_DIAG   // diagnostic build only (build.py --diag): force the two-kernel decoder step
        if (getenv("RF_NO_UPCAT")) fuse_up = false;
#endif
        if (fuse_up) {
            // ConvTranspose2d + cat + 1x1 as one kernel on composed weights: `up` never reaches HBM
            RF_TRY(launch_upcat(ws + p.tB, skip[lvl], ws + p.tA, h->packed + h->upcat_offset[i - 1], B, C, hh / 2, ww / 2, st));
        } else {
            Conv1x1Args up = conv1x1_dense(ws + p.tB, 2 * C, h->pk(h->up_w[i - 1]), nullptr, h->prm(h->up_b[i - 1]), ws + p.tU, 4 * C, B, Pn / 4, ww / 2);
            up.mode = 1;
            RF_TRY(launch_conv1x1(up, st));
            Conv1x1Args cr = conv1x1_dense(ws + p.tU, C, h->pk(h->upcr_w[i - 1]), nullptr, h->prm(h->upcr_b[i - 1]), ws + p.tA, C, B, Pn, ww);
            cr.x2 = skip[lvl]; cr.C2 = C; cr.x2_bstride = (int64_t)C * Pn;
            RF_TRY(launch_conv1x1(cr, st));
        }
        RF_TRY(run_stage(h, 4 + i, ws + p.tA, ws + p.tB, ws, p, B, H, W, st, side));
    }
    return run_output(h, in, mosaic, ws + p.tB, out, ws, p, B, H, W, st);
}

}  // extern "C"
