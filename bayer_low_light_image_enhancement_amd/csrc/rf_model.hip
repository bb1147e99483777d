// RawFormer handle: parameter registry, weight packing, workspace plan and the forward
// schedule (RawFomer_WFB_FFAB/model.py:473-508 == FrequencyawareLumaChromaAttentionRAWFormer.py:330-370).
// Host code only; every kernel lives in the rf_*.hip files next to this one.
#include <string>
#include <unordered_map>
#include <vector>
#include <cstring>
#include <cstdlib>
#include "rf_common.h"

using namespace rf;

#include "rf_handle.h"

namespace {

int add_param(rf_handle* h, const std::string& name, std::initializer_list<int64_t> shape) {
    Param p;
    p.name = name;
    p.ndim = (int)shape.size();
    int i = 0;
    for (auto s : shape) p.shape[i++] = s;
    for (; i < 4; ++i) p.shape[i] = 1;
    p.ptr = nullptr;
    h->index[name] = (int)h->params.size();
    h->params.push_back(p);
    return (int)h->params.size() - 1;
}

void add_pack(rf_handle* h, int pi, PackKind kind) {
    Param& p = h->params[pi];
    PackItem it;
    it.param = pi;
    it.kind = kind;
    it.offset = h->packed_floats;
    if (kind == PK_1x1) it.floats = packed1x1_floats((int)p.shape[1], (int)p.shape[0]);
    else if (kind == PK_3x3) it.floats = packed3x3_floats((int)p.shape[1], (int)p.shape[0]);
    else if (kind == PK_1x1_B3) it.floats = packed1x1_b3_floats((int)p.shape[1], (int)p.shape[0]);
    else it.floats = packed1x1_floats((int)p.shape[0], 4 * (int)p.shape[1]);
    h->packed_floats += align_up(it.floats, 64);
    (kind == PK_1x1_B3 ? p.pack3 : p.pack) = (int)h->packs.size();
    h->packs.push_back(it);
}

// Stage tail  channel_reduce(cat(branch, x1 + pointwise2(g)))  as one bf16x3 GEMM over [branch ; x1 ; g] (K = 2C + hidden):
// K blocks of 32 channels must not straddle the sources.  Level 0 of RawFormer-S / -B runs the fused FFN kernel instead
// (run_stage decides per call: the fused kernel takes only some image sizes).
bool tail_composable(int C, int hc) { return C % 32 == 0 && hc % 32 == 0 && hc > 0; }

int add_flagged(rf_handle* h, const std::string& name, std::initializer_list<int64_t> shape, int flags) {
    const int ix = add_param(h, name, shape);
    h->params[ix].flags = flags;
    return ix;
}

// mamba_ssm's Mamba(d, 32, 4, expand) in the order of rf_mamba_forward's pointer array (ops.mamba_param_shapes); the package is
// not available to pin the order of these keys inside the module's state_dict
void add_mamba(rf_handle* h, const std::string& q, int d, int expand, int flags, int* ix) {
    const int di = expand * d, r = cdiv(d, 16);
    ix[0] = add_flagged(h, q + "in_proj.weight", {2 * di, d}, flags);
    ix[1] = add_flagged(h, q + "conv1d.weight", {di, 1, 4}, flags);
    ix[2] = add_flagged(h, q + "conv1d.bias", {di}, flags);
    ix[3] = add_flagged(h, q + "x_proj.weight", {r + 64, di}, flags);
    ix[4] = add_flagged(h, q + "dt_proj.weight", {di, r}, flags);
    ix[5] = add_flagged(h, q + "dt_proj.bias", {di}, flags);
    ix[6] = add_flagged(h, q + "A_log", {di, 32}, flags);
    ix[7] = add_flagged(h, q + "D", {di}, flags);
    ix[8] = add_flagged(h, q + "out_proj.weight", {d, di}, flags);
}

// Conv_Transformer of RawFomer_WFB_FFAB/model.py:414-433 with WMB (model.py:203-245) as its Transformer, state_dict order.  Every
// GEMM and 3x3 weight is packed once (rf_pack_params); illu.conv2 and mb.model2 are registered and never read.
void add_stage_wfb(rf_handle* h, int i, int lvl) {
    const rf_config& cfg = h->cfg;
    const int C = cfg.dim << lvl, hid = C * cfg.ffn_expansion;
    StageIx& s = h->stage[i];
    s.lvl = lvl;
    s.first = (int)h->params.size();
    const std::string pre = "conv_tran" + std::to_string(i) + ".", t = pre + "Transformer.";
    WmbIx& m = s.wmb;
    m.hid = hid;
    s.conv_w = add_param(h, pre + "conv.weight", {C, C, 3, 3});
    s.conv_b = add_param(h, pre + "conv.bias", {C});
    add_pack(h, s.conv_w, PK_3x3);
    m.ln1_w = add_param(h, t + "norm1.body.weight", {C});
    m.ln1_b = add_param(h, t + "norm1.body.bias", {C});
    m.illu1_w = add_param(h, t + "illu.conv1.weight", {C, C + 1, 1, 1});
    m.illu1_b = add_param(h, t + "illu.conv1.bias", {C});
    m.illu_dw_w = add_param(h, t + "illu.depth_conv.weight", {C, 1, 5, 5});
    m.illu_dw_b = add_param(h, t + "illu.depth_conv.bias", {C});
    add_flagged(h, t + "illu.conv2.weight", {C, C, 1, 1}, RF_PARAM_UNUSED);
    add_flagged(h, t + "illu.conv2.bias", {C}, RF_PARAM_UNUSED);
    int* f = m.ffab;
    auto conv = [&](const std::string& q, int cout, int cin) {
        *f = add_param(h, q + ".weight", {cout, cin, 1, 1});
        add_pack(h, *f++, PK_1x1);
        *f++ = add_param(h, q + ".bias", {cout});
    };
    auto block = [&](const std::string& q, int n) {      // ProcessBlock(n): FEB, then cat
        for (const char* name : {"frequency_process.fpre", "frequency_process.process1.0", "frequency_process.process1.2",
                                 "frequency_process.process2.0", "frequency_process.process2.2", "cat"})
            conv(q + name, n, n);
    };
    const std::string fb = t + "ffab.";
    conv(fb + "conv0.0", C, C);
    block(fb + "conv0.1.", C);
    for (const char* name : {"conv1.", "conv2.", "conv3."}) block(fb + name, C);
    for (const char* name : {"conv4", "conv5", "convout"}) {
        block(fb + name + ".0.", 2 * C);
        conv(fb + name + ".1", C, 2 * C);
    }
    m.ln2_w = add_param(h, t + "norm2.body.weight", {C});
    m.ln2_b = add_param(h, t + "norm2.body.bias", {C});
    auto conv_bn = [&](const std::string& q, int k, int& w, int* bn) {
        w = add_param(h, q + "c.weight", {hid, 1, k, k});
        bn[0] = add_param(h, q + "bn.weight", {hid});
        bn[1] = add_param(h, q + "bn.bias", {hid});
        bn[2] = add_flagged(h, q + "bn.running_mean", {hid}, RF_PARAM_BUFFER);
        bn[3] = add_flagged(h, q + "bn.running_var", {hid}, RF_PARAM_BUFFER);
    };
    conv_bn(t + "ffn.rep_conv1.", 3, m.rep1_w, m.bn1);
    conv_bn(t + "ffn.rep_conv2.", 1, m.rep2_w, m.bn2);
    m.pin_w = add_param(h, t + "ffn.project_in.weight", {hid, C, 1, 1});
    m.pin_b = add_param(h, t + "ffn.project_in.bias", {hid});
    m.dw_w = add_param(h, t + "ffn.dwconv.weight", {hid, 1, 3, 3});
    m.dw_b = add_param(h, t + "ffn.dwconv.bias", {hid});
    m.pout_w = add_param(h, t + "ffn.project_out.weight", {C, hid, 1, 1});
    m.pout_b = add_param(h, t + "ffn.project_out.bias", {C});
    for (int w : {m.pin_w, m.pout_w}) {
        add_pack(h, w, PK_1x1);
        add_pack(h, w, PK_1x1_B3);
    }
    const std::string mb = t + "mb.";
    m.wm[0] = add_param(h, mb + "convb.0.weight", {2 * C, C, 3, 3});
    m.wm[1] = add_param(h, mb + "convb.0.bias", {2 * C});
    m.wm[2] = add_param(h, mb + "convb.2.weight", {C, 2 * C, 3, 3});
    m.wm[3] = add_param(h, mb + "convb.2.bias", {C});
    add_mamba(h, mb + "model1.", C, 2, 0, m.wm + 6);
    int unused[9];
    add_mamba(h, mb + "model2.", C, 9, RF_PARAM_UNUSED, unused);
    m.wm[15] = add_param(h, mb + "smooth.weight", {C, C, 3, 3});
    m.wm[16] = add_param(h, mb + "smooth.bias", {C});
    m.wm[4] = add_param(h, mb + "ln.weight", {C});
    m.wm[5] = add_param(h, mb + "ln.bias", {C});
    for (int w : {m.wm[0], m.wm[2], m.wm[15]}) add_pack(h, w, PK_3x3);
    for (int w : {m.wm[6], m.wm[9], m.wm[14]}) {
        add_pack(h, w, PK_1x1);
        add_pack(h, w, PK_1x1_B3);
    }
    m.fold = h->packed_floats;
    h->packed_floats += wmb_fold_floats(C, hid);
    m.illu_pk = h->packed_floats;
    h->packed_floats += align_up(packed1x1_floats(C, C), 64);
    s.cr_w = add_param(h, pre + "channel_reduce.weight", {C, 2 * C, 1, 1});
    s.cr_b = add_param(h, pre + "channel_reduce.bias", {C});
    s.out_w = add_param(h, pre + "Conv_out.weight", {C, C, 3, 3});
    s.out_b = add_param(h, pre + "Conv_out.bias", {C});
    add_pack(h, s.cr_w, PK_1x1);
    add_pack(h, s.cr_w, PK_1x1_B3);
    add_pack(h, s.out_w, PK_3x3);
}

void add_stage(rf_handle* h, int i, int lvl) {
    const rf_config& cfg = h->cfg;
    if (cfg.variant == RF_VARIANT_WFB) return add_stage_wfb(h, i, lvl);
    const int C = cfg.dim << lvl;
    StageIx& s = h->stage[i];
    s.lvl = lvl;
    s.first = (int)h->params.size();
    const std::string pre = "conv_tran" + std::to_string(i) + ".";
    if (cfg.variant == RF_VARIANT_TRUECOLOR) {
        // EnhancedFLCA (BayerTORGBColorMultiLvl.py:192-231), state_dict order
        const std::string f = pre + "FLCA.";
        const int hid = flca_hidden(C);
        s.tc.col_w = add_param(h, f + "color_attention.0.weight", {C, 5, 3, 3});
        s.tc.col_b = add_param(h, f + "color_attention.0.bias", {C});
        s.tc.low_w = add_param(h, f + "low_attn.0.weight", {C, 1, 3, 3});
        s.tc.low_b = add_param(h, f + "low_attn.0.bias", {C});
        s.tc.high_w = add_param(h, f + "high_attn.0.weight", {C, 1, 3, 3});
        s.tc.high_b = add_param(h, f + "high_attn.0.bias", {C});
        s.tc.se.se1_w = add_param(h, f + "se.1.weight", {hid, C, 1, 1});
        s.tc.se.se1_b = add_param(h, f + "se.1.bias", {hid});
        s.tc.se.se3_w = add_param(h, f + "se.3.weight", {C, hid, 1, 1});
        s.tc.se.se3_b = add_param(h, f + "se.3.bias", {C});
        s.tc.res0_w = add_param(h, f + "res_proj.0.weight", {C, C, 1, 1});
        s.tc.res0_b = add_param(h, f + "res_proj.0.bias", {C});
        s.tc.res2_w = add_param(h, f + "res_proj.2.weight", {C, C, 1, 1});
        s.tc.res2_b = add_param(h, f + "res_proj.2.bias", {C});
        for (int w : {s.tc.res0_w, s.tc.res2_w}) {
            add_pack(h, w, PK_1x1);
            add_pack(h, w, PK_1x1_B3);
        }
    } else if (cfg.variant == RF_VARIANT_MULTILVL) {
        // FLCA_Pyramid (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:90-116), state_dict order
        const std::string f = pre + "FLCA.";
        const int hid = flca_hidden(C), L = cfg.flca_levels > 0 ? cfg.flca_levels : 2;
        MlIx& m = s.ml;
        for (int l = 0; l < L; ++l) m.low_w[l] = add_param(h, f + "low_attn." + std::to_string(l) + ".0.weight", {C, 1, 3, 3});
        for (int l = 0; l < L; ++l) m.high_w[l] = add_param(h, f + "high_attn." + std::to_string(l) + ".0.weight", {C, 1, 3, 3});
        for (int l = 0; l < L; ++l) {
            m.gate_w[l] = add_param(h, f + "freq_gate_head." + std::to_string(l) + ".weight", {2, 2, 1, 1});
            m.gate_b[l] = add_param(h, f + "freq_gate_head." + std::to_string(l) + ".bias", {2});
        }
        m.chr_w = add_param(h, f + "chroma_attn.0.weight", {C, 2, 3, 3});
        m.cgate_w = add_param(h, f + "chroma_gate.weight", {1, 1, 1, 1});
        m.cgate_b = add_param(h, f + "chroma_gate.bias", {1});
        m.se.se1_w = add_param(h, f + "se.1.weight", {hid, C, 1, 1});
        m.se.se1_b = add_param(h, f + "se.1.bias", {hid});
        m.se.se3_w = add_param(h, f + "se.3.weight", {C, hid, 1, 1});
        m.se.se3_b = add_param(h, f + "se.3.bias", {C});
        m.res0_w = add_param(h, f + "res_proj.0.weight", {C, C, 1, 1});
        m.res0_b = add_param(h, f + "res_proj.0.bias", {C});
        m.res2_w = add_param(h, f + "res_proj.2.weight", {C, C, 1, 1});
        m.res2_b = add_param(h, f + "res_proj.2.bias", {C});
        for (int w : {m.res0_w, m.res2_w}) {
            add_pack(h, w, PK_1x1);
            add_pack(h, w, PK_1x1_B3);
        }
    } else if (cfg.variant == RF_VARIANT_FLCA) {
        const std::string f = pre + "FLCA.";
        const int hid = flca_hidden(C);
        s.flca.alpha = add_param(h, f + "alpha", {});
        s.flca.beta = add_param(h, f + "beta", {});
        s.flca.gamma = add_param(h, f + "gamma", {});
        s.flca.w_low = add_param(h, f + "low_attn.0.weight", {C, 1, 3, 3});
        s.flca.w_high = add_param(h, f + "high_attn.0.weight", {C, 1, 3, 3});
        s.flca.w_chr = add_param(h, f + "chroma_attn.0.weight", {C, 2, 3, 3});
        s.flca.se.se1_w = add_param(h, f + "se.1.weight", {hid, C, 1, 1});
        s.flca.se.se1_b = add_param(h, f + "se.1.bias", {hid});
        s.flca.se.se3_w = add_param(h, f + "se.3.weight", {C, hid, 1, 1});
        s.flca.se.se3_b = add_param(h, f + "se.3.bias", {C});
    } else {
        s.conv_w = add_param(h, pre + "conv.weight", {C, C, 3, 3});
        s.conv_b = add_param(h, pre + "conv.bias", {C});
        add_pack(h, s.conv_w, PK_3x3);
    }
    const std::string t = pre + "Transformer.";
    const int hc = C * cfg.ffn_expansion, heads = cfg.heads[lvl];
    s.ln1_w = add_param(h, t + "norm1.body.weight", {C});
    s.ln1_b = add_param(h, t + "norm1.body.bias", {C});
    s.temperature = add_param(h, t + (cfg.variant == RF_VARIANT_TRUECOLOR ? "attn.log_temperature" : "attn.temperature"), {heads, 1, 1});
    s.qkv_w = add_param(h, t + "attn.qkv.weight", {3 * C, C, 1, 1});
    s.qkv_b = add_param(h, t + "attn.qkv.bias", {3 * C});
    s.qkv_dw_w = add_param(h, t + "attn.qkv_dwconv.weight", {3 * C, 1, 3, 3});
    s.qkv_dw_b = add_param(h, t + "attn.qkv_dwconv.bias", {3 * C});
    s.proj_w = add_param(h, t + "attn.project_out.weight", {C, C, 1, 1});
    s.proj_b = add_param(h, t + "attn.project_out.bias", {C});
    s.ln2_w = add_param(h, t + "norm2.body.weight", {C});
    s.ln2_b = add_param(h, t + "norm2.body.bias", {C});
    s.pw1_w = add_param(h, t + "ffn.pointwise1.weight", {hc, C, 1, 1});
    s.pw1_b = add_param(h, t + "ffn.pointwise1.bias", {hc});
    s.dw_w = add_param(h, t + "ffn.depthwise.weight", {hc, 1, 3, 3});
    s.dw_b = add_param(h, t + "ffn.depthwise.bias", {hc});
    s.pw2_w = add_param(h, t + "ffn.pointwise2.weight", {C, hc, 1, 1});
    s.pw2_b = add_param(h, t + "ffn.pointwise2.bias", {C});
    s.cr_w = add_param(h, pre + "channel_reduce.weight", {C, 2 * C, 1, 1});
    s.cr_b = add_param(h, pre + "channel_reduce.bias", {C});
    s.out_w = add_param(h, pre + "Conv_out.weight", {C, C, 3, 3});
    s.out_b = add_param(h, pre + "Conv_out.bias", {C});
    for (int w : {s.qkv_w, s.pw1_w, s.pw2_w}) add_pack(h, w, PK_1x1);
    for (int w : {s.qkv_w, s.pw1_w, s.pw2_w}) add_pack(h, w, PK_1x1_B3);      // b3 forms for the bf16x3 GEMM kernels (rf_common.h)
    if (cfg.variant == RF_VARIANT_PLAIN) {
        add_pack(h, s.cr_w, PK_1x1);
        add_pack(h, s.cr_w, PK_1x1_B3);
    }
    if (tail_composable(C, hc)) {      // pointwise2 composed into channel_reduce (run_stage)
        s.tail_offset = h->packed_floats;
        h->packed_floats += align_up(tail_composed_floats(C, hc), 64);
        if (cfg.variant == RF_VARIANT_PLAIN) {
            s.tail3_offset = h->packed_floats;
            h->packed_floats += align_up(packed1x1_b3_floats(2 * C + hc, C), 64);
        }
    }
    add_pack(h, s.out_w, PK_3x3);
}

// ---- workspace plan ---------------------------------------------------------------------
struct Plan {
    size_t total;
    size_t gscratch, guide[4], skip[3], tA, tB, tU, bufA, bufB, x1, trans, xs, cr;
    size_t gram_partial, wfold_attn, wfold_cr, wfold_attn3, wfold_cr3, flca_partial, ch;
    size_t ffab, wm;            // WFB: FFAB scratch and WM workspace at their largest level, shared by the stages
    size_t ks, ks_floats;       // scratch of the 3x3 convs' input-channel split (small frames only: ks_floats = 0 otherwise)
    int guide_planes;
};

int make_plan(const rf_handle* h, int B, int H, int W, Plan& p) {
    const rf_config& c = h->cfg;
    const size_t U0 = (size_t)B * c.dim * H * W;   // floats of a level-0 activation
    const bool ml = c.variant == RF_VARIANT_MULTILVL;
    const bool tc = c.variant == RF_VARIANT_TRUECOLOR || ml;      // the branch follows the block on one stream and pools with tc_residual
    const int levels = c.flca_levels > 0 ? c.flca_levels : 2;
    p.guide_planes = ml ? 2 * levels + 2 : tc ? 7 : 4;
    Bump b;      // offsets into the caller's workspace
    p.gscratch = b.off(ml ? ml_scratch_floats(B, H, W, levels) : tc ? tc_front_scratch_floats(B, H, W, levels) : guidance_scratch_floats(B, H, W));
    for (int l = 0; l < 4; ++l) p.guide[l] = b.off((size_t)B * p.guide_planes * (H >> l) * (W >> l));
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
    const bool wfb = c.variant == RF_VARIANT_WFB;      // no channel attention and no fold: `heads` is not read
    p.ffab = p.wm = 0;
    if (wfb) {
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
    for (int l = 0; l < 4 && !wfb; ++l) {
        const int C = c.dim << l, Pl = (H >> l) * (W >> l);
        int ns, sl;
        size_t pf;
        const int rc = gram_plan(B, C, c.heads[l], Pl, &ns, &sl, &pf);
        if (rc) return rc;
        if (pf > gp) gp = pf;
        if (fused_attn_supported(C, c.heads[l], H >> l, W >> l)) {
            size_t pf2;
            fused_attn_plan(H >> l, W >> l, &ns, &pf2, B, C);
            if (pf2 > gp) gp = pf2;
        }
        if (attn_mid_supported(C, c.heads[l], H >> l, W >> l)) {
            size_t pf2;
            attn_mid_plan(H >> l, W >> l, &ns, &pf2, B, C);
            if (pf2 > gp) gp = pf2;
        }
        const int hcl = C * c.ffn_expansion;
        // the channel_reduce fold; at a level whose FFN kernel carries the stage tail, [Wa' | Wb | Wb W2] in the same slot
        const bool tailf = !tc && fused_ffn_tail_supported(C) && tail_composable(C, hcl);
        const size_t a = (size_t)B * packed1x1_floats(C, C), cr = (size_t)B * packed1x1_floats(tailf ? 2 * C + hcl : 2 * C, C);
        if (a > wa) wa = a;
        if (cr > wc) wc = cr;
        const size_t a3 = (size_t)B * packed1x1_b3_floats(C, C),
                     cr3 = (size_t)B * packed1x1_b3_floats(tail_composable(C, hcl) ? 2 * C + hcl : 2 * C, C);
        if (a3 > wa3) wa3 = a3;
        if (cr3 > wc3) wc3 = cr3;
        const size_t f = (size_t)B * (tc ? tc_nblk(H >> l, W >> l) : flca_nblk(H >> l, W >> l)) * C;
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

// one Conv_Transformer stage of the WFB variant: the plain variant's wiring around a WMB block (rf_wmb.hip)
int run_stage_wfb(rf_handle* h, int i, const float* in, float* out, float* ws, const Plan& p, int B, int H, int W, hipStream_t st,
                  hipStream_t side) {
    const StageIx& x = h->stage[i];
    const int lvl = x.lvl, C = h->cfg.dim << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww;
    const size_t U = (size_t)B * C * Pn;
    float *trans = ws + p.trans, *xs = ws + p.xs, *crb = ws + p.cr;
    RF_TRY(h->side.fork(st, side));
    Conv3x3Args cb{};
    cb.x = in; cb.x_bstride = (int64_t)C * Pn; cb.wp = h->pk(x.conv_w); cb.bias = h->prm(x.conv_b);
    cb.out = xs; cb.out_bstride = (int64_t)C * Pn; cb.B = B; cb.Cin = C; cb.Cout = C; cb.h = hh; cb.w = ww; cb.act = 1;
    RF_TRY(launch_conv3x3(cb, side));
    // t in the x1 slot, the bands in tU (idle inside a stage), the quarter-size illumination tensors at the head of bufA until
    // project_in writes the hidden tensor there
    const WmbBufs wb{ws + p.x1, ws + p.tU, ws + p.bufA, ws + p.bufA + U, ws + p.bufA, ws + p.bufB, ws + p.ffab, ws + p.wm};
    RF_TRY(run_wmb(h, i, in, trans, wb, B, hh, ww, st));
    RF_TRY(h->side.join(st, side));
    Conv1x1Args r{};
    r.x1 = xs; r.C1 = C; r.x1_bstride = (int64_t)C * Pn;
    r.x2 = trans; r.C2 = C; r.x2_bstride = (int64_t)C * Pn;
    r.wp = h->pk(x.cr_w); r.wp3 = h->pk3(x.cr_w); r.bias = h->prm(x.cr_b);
    r.out = crb; r.out_bstride = (int64_t)C * Pn; r.Cout = C; r.B = B; r.P = Pn; r.w = ww;
    RF_TRY(launch_conv1x1(r, st));
    Conv3x3Args co{};
    co.x = crb; co.x_bstride = (int64_t)C * Pn; co.wp = h->pk(x.out_w); co.bias = h->prm(x.out_b);
    co.out = out; co.out_bstride = (int64_t)C * Pn; co.B = B; co.Cin = C; co.Cout = C; co.h = hh; co.w = ww; co.act = 1;
    if (p.ks_floats) { co.ks_scratch = ws + p.ks; co.ks_floats = p.ks_floats; }
    return launch_conv3x3(co, st);
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

// one Conv_Transformer stage
int run_stage(rf_handle* h, int i, const float* in, float* out, float* ws, const Plan& p,
              int B, int H, int W, hipStream_t st, hipStream_t side) {
    const rf_config& cfg = h->cfg;
    if (cfg.variant == RF_VARIANT_WFB) return run_stage_wfb(h, i, in, out, ws, p, B, H, W, st, side);
    const StageIx& x = h->stage[i];
    const int lvl = x.lvl, C = cfg.dim << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww, heads = cfg.heads[lvl];
    const int hc = C * cfg.ffn_expansion;
    float* trans = ws + p.trans;
    float* xs = ws + p.xs;
    float* crb = ws + p.cr;

    // TransformerBlock: x + attn(LN1(x)), then x + ffn(LN2(x))  (rf_block.hip)
    TbParams tp{};
    tp.ln1_w = h->prm(x.ln1_w); tp.ln1_b = h->prm(x.ln1_b);
    tp.temperature = h->prm(x.temperature); tp.log_temperature = cfg.variant == RF_VARIANT_TRUECOLOR;
    tp.qkv_wp = h->pk(x.qkv_w); tp.qkv_b = h->prm(x.qkv_b);
    tp.qkv_dw_w = h->prm(x.qkv_dw_w); tp.qkv_dw_b = h->prm(x.qkv_dw_b);
    tp.proj_w = h->prm(x.proj_w); tp.proj_b = h->prm(x.proj_b);
    tp.ln2_w = h->prm(x.ln2_w); tp.ln2_b = h->prm(x.ln2_b);
    tp.pw1_wp = h->pk(x.pw1_w); tp.pw1_b = h->prm(x.pw1_b);
    tp.dw_w = h->prm(x.dw_w); tp.dw_b = h->prm(x.dw_b);
    tp.pw2_wp = h->pk(x.pw2_w); tp.pw2_b = h->prm(x.pw2_b);
    tp.qkv_wp3 = h->pk3(x.qkv_w); tp.pw1_wp3 = h->pk3(x.pw1_w); tp.pw2_wp3 = h->pk3(x.pw2_w);
    // spatial shard: this level's interior rows and columns, and the frame's pixel count for the pooled mean
    const bool sharded = h->shard_allreduce != nullptr;
    const int ylo = sharded ? h->shard_y_lo >> lvl : 0, yhi = sharded ? h->shard_y_hi >> lvl : 0;
    const int xlo = sharded ? h->shard_x_lo >> lvl : 0, xhi = sharded ? h->shard_x_hi >> lvl : 0;
    const int P_pool = sharded ? (h->shard_total_rows >> lvl) * (h->shard_total_cols ? h->shard_total_cols >> lvl : ww) : Pn;
    if (sharded) {
        tp.ylo = ylo; tp.yhi = yhi; tp.xlo = xlo; tp.xhi = xhi;
        tp.allreduce = h->shard_allreduce; tp.allreduce_user = h->shard_user;
    }
    TbBufOffsets to{p.bufA, p.bufB, p.x1, p.gram_partial, p.wfold_attn, p.wfold_attn3};
    // Composed tail: where the FFN runs op by op, its last GEMM (x1 + W2 g + b2 -> trans, K = hidden) and channel_reduce
    // ([Wa' | Wb] [xs ; trans], K = 2C) become ONE GEMM over [xs ; x1 ; g] with [Wa' | Wb | Wb W2] (same MFMA count; `trans` --
    // C floats per pixel written and read back -- never exists).  The bias and Wb W2 are composed at parameter load.
    const bool ffn_fused = transformer_ffn_is_fused(tp, C, hc, hh, ww);
    bool compose = x.tail_offset != 0 && Pn % 4 == 0 && !ffn_fused;
    // Fused tail: where the FFN is ffn_fused_kernel<32> (level 0), the same composition runs INSIDE it -- xs and x1 are 16 more
    // k-steps of its second GEMM, Wb W2 replaces W2 -- so neither `trans` nor the channel_reduce launch exists.  The kernel reads
    // the weights in f32 operand order from the fold slot of the workspace (per image: the FLCA gate; one set for the plain
    // variant, folded per call: the packed buffer has no room for it).  Not TrueColor, whose branch runs after the block.
    const bool branch_after = cfg.variant == RF_VARIANT_TRUECOLOR || cfg.variant == RF_VARIANT_MULTILVL;
    bool fuse_tail = x.tail_offset != 0 && ffn_fused && fused_ffn_tail_supported(C) && !branch_after;
#ifdef RF_DIAG   // diagnostic build only: the two-GEMM form
    if (getenv("RF_NO_COMPOSE") || getenv("RF_NO_B3")) compose = false;
    if (getenv("RF_NO_COMPOSE")) fuse_tail = false;
#endif
    tp.defer_pw2 = compose;
    const float* composed = compose || fuse_tail ? h->packed + x.tail_offset : nullptr;
    float* const fold_wp = compose ? nullptr : ws + p.wfold_cr;          // the fold writes the form(s) the tail reads
    float* const fold_wp3 = fuse_tail ? nullptr : ws + p.wfold_cr3;
    // the branch is launched first (on the branch stream when there is one), the block beside it; the TrueColor and multi-level
    // branches borrow bufA and therefore follow the block on the same stream
    if (branch_after) RF_TRY(run_transformer(tp, in, trans, ws, to, B, C, heads, hc, hh, ww, st));
    else RF_TRY(h->side.fork(st, side));

    // branch, cat, channel_reduce -------------------------------------------------------------
    Conv1x1Args r{};
    r.x1 = xs; r.C1 = C; r.x1_bstride = (int64_t)C * Pn;
    r.x2 = trans; r.C2 = C; r.x2_bstride = (int64_t)C * Pn;
    r.bias = h->prm(x.cr_b);
    r.out = crb; r.out_bstride = (int64_t)C * Pn; r.Cout = C; r.B = B; r.P = Pn; r.w = ww;
    if (cfg.variant == RF_VARIANT_TRUECOLOR) {
        // EnhancedFLCA (BayerTORGBColorMultiLvl.py:249-293): spatial gate -> x + 0.2 tanh(res_proj(x)) -> squeeze-excite (folded
        // into channel_reduce like the FLCA variant's)
        const TcIx& t = x.tc;
        RF_TRY(launch_tc_spatial(in, xs, ws + p.guide[lvl], h->prm(t.col_w), h->prm(t.col_b), h->prm(t.low_w), h->prm(t.low_b), h->prm(t.high_w),
                                 h->prm(t.high_b), B, C, hh, ww, st));
        Conv1x1Args r0{};
        r0.x1 = xs; r0.C1 = C; r0.x1_bstride = (int64_t)C * Pn; r0.wp = h->pk(t.res0_w); r0.wp3 = h->pk3(t.res0_w);
        r0.bias = h->prm(t.res0_b); r0.out = crb; r0.out_bstride = (int64_t)C * Pn; r0.Cout = C; r0.B = B; r0.P = Pn; r0.w = ww; r0.act = 2;
        RF_TRY(launch_conv1x1(r0, st));
        Conv1x1Args r2 = r0;
        r2.x1 = crb; r2.wp = h->pk(t.res2_w); r2.wp3 = h->pk3(t.res2_w); r2.bias = h->prm(t.res2_b);
        r2.out = ws + p.bufA; r2.act = 0;
        RF_TRY(launch_conv1x1(r2, st));
        RF_TRY(launch_tc_residual(xs, ws + p.bufA, xs, ws + p.flca_partial, B, C, hh, ww, st));
        RF_TRY(launch_flca_se_fold(ws + p.flca_partial, tc_nblk(hh, ww), Pn, h->se_prm(t.se), h->prm(x.cr_w), fold_wp, fold_wp3,
                                   ws + p.ch, B, C, st, composed, hc));
        r.wp = ws + p.wfold_cr; r.wp_bstride = (int64_t)packed1x1_floats(2 * C, C);
        r.wp3 = ws + p.wfold_cr3; r.wp3_bstride = (int64_t)packed1x1_b3_floats(compose ? 2 * C + hc : 2 * C, C);
    } else if (cfg.variant == RF_VARIANT_MULTILVL) {
        // FLCA_Pyramid (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:132-183): for every pyramid level and then for the
        // chroma planes  x <- x + 0.2 tanh(res_proj(x * gated spatial attention)),  one res_proj for all steps; squeeze-excite
        // folded into channel_reduce.  A composed step is modulate -> 1x1 (ReLU) -> 1x1 -> residual; the last one leaves the pooling sums.
        const MlIx& m = x.ml;
        const int L = cfg.flca_levels > 0 ? cfg.flca_levels : 2;
        const float* means = ml_level_means(ws + p.gscratch, lvl, B, H, W, L);
        float* t1 = ws + p.bufA;
        float* t2 = t1 + (size_t)B * C * Pn;
        Conv1x1Args r0{};
        r0.x1 = crb; r0.C1 = C; r0.x1_bstride = (int64_t)C * Pn; r0.wp = h->pk(m.res0_w); r0.wp3 = h->pk3(m.res0_w);
        r0.bias = h->prm(m.res0_b); r0.out = t1; r0.out_bstride = (int64_t)C * Pn; r0.Cout = C; r0.B = B; r0.P = Pn; r0.w = ww; r0.act = 2;
        Conv1x1Args r2 = r0;
        r2.x1 = t1; r2.wp = h->pk(m.res2_w); r2.wp3 = h->pk3(m.res2_w); r2.bias = h->prm(m.res2_b); r2.out = t2; r2.act = 0;
        // level 0 (C = dim <= 64, the largest tensor): one kernel per step, nothing but x and the result in HBM
        bool fused_step = ml_step_fused_supported(C, hh, ww);
#ifdef RF_DIAG   // diagnostic build only: the composed steps everywhere
        if (getenv("RF_NO_ML_FUSED")) fused_step = false;
#endif
        const float* cur = in;
        for (int s = 0; s <= L; ++s) {
            const bool chroma = s == L;
            const float* w_a = h->prm(chroma ? m.chr_w : m.low_w[s]);
            const float* w_b = chroma ? nullptr : h->prm(m.high_w[s]);
            const float* g_w = h->prm(chroma ? m.cgate_w : m.gate_w[s]);
            const float* g_b = h->prm(chroma ? m.cgate_b : m.gate_b[s]);
            if (fused_step) {
                RF_TRY(launch_ml_step_fused(cur, xs, ws + p.guide[lvl], means, s, L, w_a, w_b, g_w, g_b, h->prm(m.res0_w), h->prm(m.res0_b),
                                            h->prm(m.res2_w), h->prm(m.res2_b), chroma ? ws + p.flca_partial : nullptr, B, C, hh, ww, st));
            } else {
                RF_TRY(launch_ml_modulate(cur, crb, ws + p.guide[lvl], means, s, L, w_a, w_b, g_w, g_b, B, C, hh, ww, st));
                RF_TRY(launch_conv1x1(r0, st));
                RF_TRY(launch_conv1x1(r2, st));
                if (chroma) RF_TRY(launch_tc_residual(cur, t2, xs, ws + p.flca_partial, B, C, hh, ww, st));   // the last step: + pooling sums
                else RF_TRY(launch_ml_residual(cur, t2, xs, B, C, hh, ww, st));
            }
            cur = xs;
        }
        RF_TRY(launch_flca_se_fold(ws + p.flca_partial, tc_nblk(hh, ww), Pn, h->se_prm(m.se), h->prm(x.cr_w), fold_wp, fold_wp3,
                                   ws + p.ch, B, C, st, composed, hc));
        r.wp = ws + p.wfold_cr; r.wp_bstride = (int64_t)packed1x1_floats(2 * C, C);
        r.wp3 = ws + p.wfold_cr3; r.wp3_bstride = (int64_t)packed1x1_b3_floats(compose ? 2 * C + hc : 2 * C, C);
    } else if (cfg.variant == RF_VARIANT_FLCA) {
        const FlcaPrm fp = h->flca_prm(x.flca);
        FlcaSpatialArgs s{};
        s.feat = in; s.xs = xs; s.guide = ws + p.guide[lvl];
        s.set_params(fp);
        s.partial = ws + p.flca_partial; s.B = B; s.C = C; s.h = hh; s.w = ww; s.nblk = flca_nblk(hh, ww);
        s.ylo = ylo; s.yhi = yhi; s.xlo = xlo; s.xhi = xhi;
        RF_TRY(launch_flca_spatial(s, side));
        if (sharded) h->shard_allreduce(h->shard_user, s.partial, (size_t)B * s.nblk * C, 0, (void*)side);
        RF_TRY(launch_flca_se_fold(s.partial, s.nblk, P_pool, fp.se, h->prm(x.cr_w), fold_wp, fold_wp3, ws + p.ch, B, C, side, composed, hc));
        tp.tail.wp_bstride = (int64_t)packed1x1_floats(2 * C + hc, C);
        r.wp = ws + p.wfold_cr; r.wp_bstride = (int64_t)packed1x1_floats(2 * C, C);
        r.wp3 = ws + p.wfold_cr3; r.wp3_bstride = (int64_t)packed1x1_b3_floats(compose ? 2 * C + hc : 2 * C, C);
    } else {
        Conv3x3Args cb{};
        cb.x = in; cb.x_bstride = (int64_t)C * Pn; cb.wp = h->pk(x.conv_w); cb.bias = h->prm(x.conv_b);
        cb.out = xs; cb.out_bstride = (int64_t)C * Pn; cb.B = B; cb.Cin = C; cb.Cout = C; cb.h = hh; cb.w = ww;
        cb.act = cfg.branch_lrelu ? 1 : 0;
        RF_TRY(launch_conv3x3(cb, side));
        if (fuse_tail) RF_TRY(launch_tail_fold(h->prm(x.cr_w), nullptr, composed, nullptr, 1, C, hc, side, fold_wp));
        r.wp = h->pk(x.cr_w);
        r.wp3 = compose ? h->packed + x.tail3_offset : h->pk3(x.cr_w);
    }
    if (fuse_tail) {
        // the FFN kernel reads the branch's output and weights: the join sits between the block's two halves
        tp.tail.xs = xs; tp.tail.wp = fold_wp; tp.tail_bias = composed + (size_t)C * hc;
        RF_TRY(run_transformer_attn(tp, in, ws, to, B, C, heads, hh, ww, st));
        RF_TRY(h->side.join(st, side));
        RF_TRY(run_transformer_ffn(tp, crb, ws, to, B, C, hc, hh, ww, st));
    } else if (!branch_after) {
        RF_TRY(run_transformer(tp, in, trans, ws, to, B, C, heads, hc, hh, ww, st));
        RF_TRY(h->side.join(st, side));
    }
    if (compose) {
        r.wp = nullptr;
        r.x2 = ws + p.x1;
        r.x3 = ws + p.bufB; r.C3 = hc; r.x3_bstride = (int64_t)hc * Pn;
        r.bias = composed + (size_t)C * hc;
    }
    if (!fuse_tail) RF_TRY(launch_conv1x1(r, st));

    Conv3x3Args co{};
    co.x = crb; co.x_bstride = (int64_t)C * Pn; co.wp = h->pk(x.out_w); co.bias = h->prm(x.out_b);
    co.out = out; co.out_bstride = (int64_t)C * Pn; co.B = B; co.Cin = C; co.Cout = C; co.h = hh; co.w = ww; co.act = 1;
    if (p.ks_floats) { co.ks_scratch = ws + p.ks; co.ks_floats = p.ks_floats; }
    RF_TRY(launch_conv3x3(co, st));
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

int rf_create(const rf_config* cfg, rf_handle** out) {
    RF_CHECK_ARG(cfg && out, "rf_create: null argument");
    RF_CHECK_ARG(cfg->dim > 0 && cfg->dim % 8 == 0, "rf_create: dim=%d must be a positive multiple of 8", cfg->dim);
    RF_CHECK_ARG(cfg->inp_channels == 1, "rf_create: inp_channels=%d (only the 1-channel Bayer mosaic is supported)", cfg->inp_channels);
    RF_CHECK_ARG(cfg->out_channels > 0 && cfg->ffn_expansion > 0, "rf_create: bad out_channels / ffn_expansion");
    RF_CHECK_ARG(cfg->variant == RF_VARIANT_FLCA || cfg->variant == RF_VARIANT_PLAIN || cfg->variant == RF_VARIANT_TRUECOLOR ||
                     cfg->variant == RF_VARIANT_MULTILVL || cfg->variant == RF_VARIANT_WFB,
                 "rf_create: unknown variant %d", cfg->variant);
    const bool wfb = cfg->variant == RF_VARIANT_WFB;
    RF_CHECK_ARG(!wfb || (cfg->clamp_io && cfg->branch_lrelu), "rf_create: variant wfb always clamps its input and output and applies the "
                 "LeakyReLU on the conv branch (clamp_io = branch_lrelu = 1)");
    RF_CHECK_ARG(!wfb || cfg->dim * 8 <= 512, "rf_create: variant wfb: dim * 8 = %d channels at level 3 exceed the 512 of the Mamba token LayerNorm",
                 cfg->dim * 8);
    RF_CHECK_ARG(cfg->flca_levels >= 0 && cfg->flca_levels <= 3, "rf_create: flca_levels=%d (1..3, 0 = default 2)", cfg->flca_levels);
    RF_CHECK_ARG(cfg->variant != RF_VARIANT_TRUECOLOR || cfg->out_channels == 3, "rf_create: the TrueColor colour head is defined for 3 output channels");
    RF_CHECK_ARG(cfg->variant != RF_VARIANT_MULTILVL || (cfg->out_channels == 3 && !cfg->clamp_io),
                 "rf_create: the multilvl output corrections are defined for 3 output channels and no clamp_io");
    for (int l = 0; l < 4 && !wfb; ++l) {
        const int C = cfg->dim << l;
        RF_CHECK_ARG(cfg->heads[l] > 0 && C % cfg->heads[l] == 0 && C / cfg->heads[l] <= 64,
                     "rf_create: heads[%d]=%d incompatible with %d channels (head size must divide and be <= 64)", l, cfg->heads[l], C);
        int ns, sl;
        size_t pf;
        RF_TRY(gram_plan(1, C, cfg->heads[l], 256, &ns, &sl, &pf));   // rejects head sizes whose query tiles straddle too many key tiles
    }
    rf_handle* h = new rf_handle();
    h->cfg = *cfg;
    const int d = cfg->dim;
    if (cfg->variant == RF_VARIANT_TRUECOLOR) {   // EnhancedBayerProcessor (BayerTORGBColorMultiLvl.py:73-98), state_dict order
        h->bp.wb_gains = add_param(h, "bayer_processor.wb_gains", {4});
        h->bp.color_matrix = add_param(h, "bayer_processor.color_matrix", {3, 4});
        h->bp.dm0_w = add_param(h, "bayer_processor.demosaic_refine.0.weight", {32, 3, 3, 3});
        h->bp.dm0_b = add_param(h, "bayer_processor.demosaic_refine.0.bias", {32});
        h->bp.dm2_w = add_param(h, "bayer_processor.demosaic_refine.2.weight", {3, 32, 3, 3});
        h->bp.dm2_b = add_param(h, "bayer_processor.demosaic_refine.2.bias", {3});
        h->bp.ce0_w = add_param(h, "bayer_processor.chroma_extractor.0.weight", {16, 4, 3, 3});
        h->bp.ce0_b = add_param(h, "bayer_processor.chroma_extractor.0.bias", {16});
        h->bp.ce2_w = add_param(h, "bayer_processor.chroma_extractor.2.weight", {2, 16, 3, 3});
        h->bp.ce2_b = add_param(h, "bayer_processor.chroma_extractor.2.bias", {2});
        for (int w : {h->bp.dm0_w, h->bp.dm2_w, h->bp.ce0_w, h->bp.ce2_w}) add_pack(h, w, PK_3x3);
    }
    h->embedding_w = add_param(h, "embedding.weight", {d, 4 * cfg->inp_channels, 3, 3});
    h->embedding_b = add_param(h, "embedding.bias", {d});
    add_pack(h, h->embedding_w, PK_3x3);
    for (int i = 1; i <= 3; ++i) {
        const int C = d << (i - 1);
        add_stage(h, i, i - 1);
        // (the multi-level file's down<i> is a bare nn.Sequential: no `body`)
        h->down_w[i - 1] = add_param(h, "down" + std::to_string(i) + (cfg->variant == RF_VARIANT_MULTILVL ? ".0.weight" : ".body.0.weight"), {C / 2, C, 3, 3});
        add_pack(h, h->down_w[i - 1], PK_3x3);
    }
    add_stage(h, 4, 3);
    for (int i = 1; i <= 3; ++i) {
        const int lvl = 3 - i, C = d << lvl;
        const std::string u = "up" + std::to_string(i), r = "channel_reduce" + std::to_string(i);
        h->up_w[i - 1] = add_param(h, u + ".weight", {2 * C, C, 2, 2});
        h->up_b[i - 1] = add_param(h, u + ".bias", {C});
        h->upcr_w[i - 1] = add_param(h, r + ".weight", {C, 2 * C, 1, 1});
        h->upcr_b[i - 1] = add_param(h, r + ".bias", {C});
        add_pack(h, h->up_w[i - 1], PK_CONVT);      // the two-kernel form stays available for widths that are not
        add_pack(h, h->upcr_w[i - 1], PK_1x1);      // multiples of 4 (e.g. level 3 of a 1424 x 2128 frame)
        h->upcat_offset[i - 1] = h->packed_floats;
        h->packed_floats += align_up(upcat_packed_floats(C), 64);
        add_stage(h, 4 + i, lvl);
    }
    h->conv_out_w = add_param(h, "conv_out.weight", {4 * cfg->out_channels, d, 3, 3});
    h->conv_out_b = add_param(h, "conv_out.bias", {4 * cfg->out_channels});
    add_pack(h, h->conv_out_w, PK_3x3);
    if (cfg->variant == RF_VARIANT_TRUECOLOR) {   // CameraAwareColorCorrection (BayerTORGBColorMultiLvl.py:139-158)
        h->cc.gamma = add_param(h, "color_correction.gamma_param", {});
        h->cc.ct0_w = add_param(h, "color_correction.color_transform.0.weight", {64, 3, 1, 1});
        h->cc.ct0_b = add_param(h, "color_correction.color_transform.0.bias", {64});
        h->cc.ct2_w = add_param(h, "color_correction.color_transform.2.weight", {3, 64, 1, 1});
        h->cc.ct2_b = add_param(h, "color_correction.color_transform.2.bias", {3});
        h->cc.tone0_w = add_param(h, "color_correction.tone_curve.0.weight", {32, 1, 1, 1});
        h->cc.tone0_b = add_param(h, "color_correction.tone_curve.0.bias", {32});
        h->cc.tone2_w = add_param(h, "color_correction.tone_curve.2.weight", {1, 32, 1, 1});
        h->cc.tone2_b = add_param(h, "color_correction.tone_curve.2.bias", {1});
    }
    plan_training(h);
    *out = h;
    return RF_OK;
}

void rf_destroy(rf_handle* h) {
    if (!h) return;
    h->side.destroy();
    delete h;
}

int rf_param_count(const rf_handle* h) { return h ? (int)h->params.size() : RF_E_INVALID; }

int rf_param_info(const rf_handle* h, int index, const char** name, int64_t shape[4], int* ndim) {
    RF_CHECK_ARG(h && index >= 0 && index < (int)h->params.size(), "rf_param_info: index %d out of range", index);
    const Param& p = h->params[index];
    if (name) *name = p.name.c_str();
    if (shape) std::memcpy(shape, p.shape, sizeof(p.shape));
    if (ndim) *ndim = p.ndim;
    return RF_OK;
}

int rf_param_flags(const rf_handle* h, int index, int* flags) {
    RF_CHECK_ARG(h && flags && index >= 0 && index < (int)h->params.size(), "rf_param_flags: index %d out of range", index);
    *flags = h->params[index].flags;
    return RF_OK;
}

int rf_set_param(rf_handle* h, const char* name, const float* dev_ptr, const int64_t* shape, int ndim) {
    RF_CHECK_ARG(h && name && dev_ptr, "rf_set_param: null argument");
    auto it = h->index.find(name);
    if (it == h->index.end()) {
        set_error("rf_set_param: unexpected key '%s'", name);
        return RF_E_MISSING;
    }
    Param& p = h->params[it->second];
    RF_CHECK_ARG(!(p.flags & RF_PARAM_UNUSED), "rf_set_param: %s is never read by the forward and takes no pointer", name);
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    bool same = n == p.numel();
    // accept [heads,1,1] vs [1,heads,1,1] style differences, reject anything that changes sizes
    if (same && ndim == p.ndim)
        for (int i = 0; i < ndim; ++i) same = same && shape[i] == p.shape[i];
    else if (same)
        same = p.ndim <= 1 || p.name.find("temperature") != std::string::npos;
    RF_CHECK_ARG(same, "rf_set_param: size mismatch for %s: got %zu elements in %d dims, expected %zu", name, n, ndim, p.numel());
    RF_CHECK_ARG((reinterpret_cast<uintptr_t>(dev_ptr) & 3) == 0, "rf_set_param: %s is not 4-byte aligned", name);
    p.ptr = dev_ptr;
    h->packed = nullptr;
    return RF_OK;
}

int rf_packed_bytes(const rf_handle* h, size_t* bytes) {
    RF_CHECK_ARG(h && bytes, "rf_packed_bytes: null argument");
    *bytes = h->packed_floats * sizeof(float);
    return RF_OK;
}

int rf_pack_params(rf_handle* h, void* packed_dev, size_t bytes, void* stream) {
    RF_CHECK_ARG(h && packed_dev, "rf_pack_params: null argument");
    RF_CHECK_ARG(aligned16(packed_dev), "rf_pack_params: buffer must be 16-byte aligned");
    if (bytes < h->packed_floats * sizeof(float)) {
        set_error("rf_pack_params: buffer of %zu bytes, need %zu", bytes, h->packed_floats * sizeof(float));
        return RF_E_NOMEM;
    }
    for (const Param& p : h->params)
        if (!p.ptr && !(p.flags & RF_PARAM_UNUSED)) {
            set_error("rf_pack_params: missing key '%s'", p.name.c_str());
            return RF_E_MISSING;
        }
    hipStream_t st = (hipStream_t)stream;
    float* base = (float*)packed_dev;
    for (const PackItem& it : h->packs) {
        const Param& p = h->params[it.param];
        int rc;
        if (it.kind == PK_1x1) rc = pack_1x1(p.ptr, base + it.offset, (int)p.shape[0], (int)p.shape[1], p.shape[1], 1, st);
        else if (it.kind == PK_1x1_B3) rc = pack_1x1_b3(p.ptr, base + it.offset, (int)p.shape[0], (int)p.shape[1], p.shape[1], 1, st);
        else if (it.kind == PK_3x3) rc = pack_3x3(p.ptr, base + it.offset, (int)p.shape[0], (int)p.shape[1], st);
        else rc = pack_convT(p.ptr, base + it.offset, (int)p.shape[0], (int)p.shape[1], st);
        if (rc) return rc;
    }
    for (int i = 0; i < 3; ++i)
        RF_TRY(pack_upcat(h->prm(h->up_w[i]), h->prm(h->up_b[i]), h->prm(h->upcr_w[i]), h->prm(h->upcr_b[i]), base + h->upcat_offset[i],
                          h->cfg.dim << (2 - i), st));
    for (int i = 1; i <= 7; ++i) {
        const StageIx& x = h->stage[i];
        if (!x.tail_offset) continue;
        const int C = h->cfg.dim << x.lvl, hc = C * h->cfg.ffn_expansion;
        float* composed = base + x.tail_offset;
        RF_TRY(pack_tail(h->prm(x.cr_w), h->prm(x.cr_b), h->prm(x.pw2_w), h->prm(x.pw2_b), composed, C, hc, st));
        if (x.tail3_offset) RF_TRY(launch_tail_fold(h->prm(x.cr_w), nullptr, composed, base + x.tail3_offset, 1, C, hc, st));
    }
    h->packed = base;
    if (h->cfg.variant == RF_VARIANT_WFB)
        for (int i = 1; i <= 7; ++i)
            if (int rc = pack_wmb(h, i, base, st)) {
                h->packed = nullptr;
                return rc;
            }
    return RF_OK;
}

int rf_workspace_bytes(const rf_handle* h, int B, int H, int W, size_t* bytes) {
    RF_CHECK_ARG(h && bytes, "rf_workspace_bytes: null argument");
    RF_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "packed size %dx%d must be positive multiples of 8 (mosaic divisible by 16)", H, W);
    if (h->cfg.variant == RF_VARIANT_WFB) RF_TRY(wfb_check_size("rf_workspace_bytes", H, W));
    Plan p;
    RF_TRY(make_plan(h, B, H, W, p));
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
    RF_CHECK_ARG(h->cfg.variant == RF_VARIANT_FLCA || h->cfg.variant == RF_VARIANT_PLAIN, "%s: variants flca and plain only", who);
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
    RF_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
                 "rf_forward_stage: packed size %dx%d must be positive multiples of 8", H, W);
    RF_CHECK_ARG((h->cfg.variant != RF_VARIANT_FLCA && h->cfg.variant != RF_VARIANT_MULTILVL) || packed,
                 "rf_forward_stage: the FLCA branch needs the packed frame for its guidance");
    RF_CHECK_ARG(h->cfg.variant != RF_VARIANT_TRUECOLOR, "rf_forward_stage: not available for the TrueColor variant");
    if (h->cfg.variant == RF_VARIANT_WFB) RF_TRY(wfb_check_size("rf_forward_stage", H, W));
    if (!h->packed) {
        set_error("rf_forward_stage: parameters not packed (call rf_pack_params after rf_set_param)");
        return RF_E_MISSING;
    }
    RF_CHECK_ARG(aligned16(workspace) && aligned16(in) && aligned16(out), "rf_forward_stage: buffers must be 16-byte aligned");
    Plan p;
    RF_TRY(make_plan(h, B, H, W, p));
    if (workspace_bytes < p.total * sizeof(float)) {
        set_error("rf_forward_stage: workspace of %zu bytes, need %zu", workspace_bytes, p.total * sizeof(float));
        return RF_E_NOMEM;
    }
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int lvl = h->stage[stage].lvl;
    if (h->cfg.variant == RF_VARIANT_FLCA) {
        RF_TRY(launch_guidance_base(packed, 0, h->cfg.clamp_io, ws + p.gscratch, B, H, W, st));
        RF_TRY(launch_guidance_level(ws + p.gscratch, ws + p.guide[lvl], B, H, W, H >> lvl, W >> lvl, st));
    } else if (h->cfg.variant == RF_VARIANT_MULTILVL) {
        const int levels = h->cfg.flca_levels > 0 ? h->cfg.flca_levels : 2;
        RF_CHECK_ARG(aligned16(packed), "rf_forward_stage: buffers must be 16-byte aligned");
        RF_TRY(launch_ml_guidance(packed, 0, ws + p.gscratch, B, H, W, levels, st));
        RF_TRY(launch_ml_guide_level(ws + p.gscratch, ws + p.guide[lvl], lvl, B, H, W, levels, H >> lvl, W >> lvl, st));
    }
    if (p.ks_floats) RF_TRY(check_hip(hipMemsetAsync(ws + p.ks, 0, conv3x3_ksplit_counter_bytes(), st), "rf_forward_stage: memset"));
    return run_stage(h, stage, in, out, ws, p, B, H, W, st, st);
}

int rf_forward(rf_handle* h, const float* in, float* out, void* workspace, size_t workspace_bytes,
               int B, int H, int W, int packed_input, void* stream) {
    RF_CHECK_ARG(h && in && out && workspace, "rf_forward: null argument");
    RF_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
                 "rf_forward: packed size %dx%d must be positive multiples of 8 (mosaic divisible by 16)", H, W);
    RF_CHECK_ARG((size_t)H * W < (1u << 30), "rf_forward: frame too large");
    if (h->cfg.variant == RF_VARIANT_WFB) RF_TRY(wfb_check_size("rf_forward", H, W));
    RF_CHECK_ARG(!h->shard_allreduce || h->shard_y_hi <= H, "rf_forward: shard interior [%d, %d) outside the %d-row window",
                 h->shard_y_lo, h->shard_y_hi, H);
    RF_CHECK_ARG(!h->shard_allreduce || h->shard_x_hi == W || (h->shard_x_hi < W && h->shard_x_hi % 32 == 0),
                 "rf_forward: shard interior columns [%d, %d) must end on a multiple of 32 inside the %d-column window or at its width",
                 h->shard_x_lo, h->shard_x_hi, W);
    if (!h->packed) {
        set_error("rf_forward: parameters not packed (call rf_pack_params after rf_set_param)");
        return RF_E_MISSING;
    }
    RF_CHECK_ARG(aligned16(workspace) && aligned16(in) && aligned16(out), "rf_forward: buffers must be 16-byte aligned");
    Plan p;
    RF_TRY(make_plan(h, B, H, W, p));
    if (workspace_bytes < p.total * sizeof(float)) {
        set_error("rf_forward: workspace of %zu bytes, need %zu", workspace_bytes, p.total * sizeof(float));
        return RF_E_NOMEM;
    }
    const rf_config& cfg = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    SideJoinGuard joined(h->side, st);
    float* ws = (float*)workspace;
    const int d = cfg.dim;
    const int mosaic = packed_input ? 0 : 1;

    const int levels = cfg.flca_levels > 0 ? cfg.flca_levels : 2;
    // A stage's branch (FLCA gates + squeeze-excite fold, or the plain variant's 3x3) depends on the stage input only, like the
    // TransformerBlock beside it; so does the guidance pyramid at the head of the forward.  On a single frame every kernel of
    // both chains is a few dozen microseconds of mostly latency, so the branch runs on the handle's second stream, forked
    // before it and joined before channel_reduce.  Not for a spatial shard (its collectives stay on the caller's stream) nor
    // for TrueColor (its branch shares bufA with the block).
    bool use_side = !h->shard_allreduce && cfg.variant != RF_VARIANT_TRUECOLOR && cfg.variant != RF_VARIANT_MULTILVL;
#ifdef RF_DIAG   // diagnostic build only: everything on the caller's stream
    if (getenv("RF_NO_SIDE")) use_side = false;
#endif
    const hipStream_t side = use_side ? h->side.get(st) : st;
    if (p.ks_floats)      // tickets of the 3x3 convs' input-channel split (the kernels leave them zero; the workspace is the caller's)
        RF_TRY(check_hip(hipMemsetAsync(ws + p.ks, 0, conv3x3_ksplit_counter_bytes(), st), "rf_forward: memset"));
    if (cfg.variant == RF_VARIANT_FLCA) {
        // the guidance pyramid feeds the FLCA branches only: it runs on their stream, beside the embedding
        RF_TRY(h->side.fork(st, side));
        RF_TRY(launch_guidance_base(in, mosaic, cfg.clamp_io, ws + p.gscratch, B, H, W, side, h->shard_allreduce, h->shard_user));
        for (int l = 0; l < 4; ++l)
            RF_TRY(launch_guidance_level(ws + p.gscratch, ws + p.guide[l], B, H, W, H >> l, W >> l, side));
    } else if (cfg.variant == RF_VARIANT_TRUECOLOR) {
        const BayerProcIx& bp = h->bp;
        RF_TRY(launch_tc_front(in, mosaic, h->prm(bp.wb_gains), h->prm(bp.color_matrix), h->pk(bp.ce0_w), h->prm(bp.ce0_b), h->pk(bp.ce2_w),
                               h->prm(bp.ce2_b), h->pk(bp.dm0_w), h->prm(bp.dm0_b), h->pk(bp.dm2_w), h->prm(bp.dm2_b),
                               ws + p.gscratch, B, H, W, levels, st));
        for (int l = 0; l < 4; ++l)
            RF_TRY(launch_tc_guide_level(ws + p.gscratch, ws + p.guide[l], B, H, W, levels, H >> l, W >> l, st));
    } else if (cfg.variant == RF_VARIANT_MULTILVL) {
        RF_TRY(launch_ml_guidance(in, mosaic, ws + p.gscratch, B, H, W, levels, st));
        for (int l = 0; l < 4; ++l)
            RF_TRY(launch_ml_guide_level(ws + p.gscratch, ws + p.guide[l], l, B, H, W, levels, H >> l, W >> l, st));
    }
    // embedding (reads the mosaic through the Bayer pack)
    Conv3x3Args e{};
    e.x = in; e.x_bstride = (int64_t)4 * H * W; e.wp = h->pk(h->embedding_w); e.bias = h->prm(h->embedding_b);
    e.out = ws + p.tA; e.out_bstride = (int64_t)d * H * W; e.B = B; e.Cin = 4; e.Cout = d; e.h = H; e.w = W;
    e.unshuffle_in = mosaic; e.clamp_in = cfg.clamp_io;
    RF_TRY(launch_conv3x3(e, st));

    // encoder
    float* skip[3] = {ws + p.skip[0], ws + p.skip[1], ws + p.skip[2]};
    for (int i = 1; i <= 3; ++i) {
        const int lvl = i - 1, C = d << lvl, hh = H >> lvl, ww = W >> lvl;
        RF_TRY(run_stage(h, i, ws + p.tA, skip[lvl], ws, p, B, H, W, st, side));
        Conv3x3Args dn{};
        dn.x = skip[lvl]; dn.x_bstride = (int64_t)C * hh * ww; dn.wp = h->pk(h->down_w[i - 1]);
        dn.out = ws + p.tA; dn.out_bstride = (int64_t)2 * C * (hh / 2) * (ww / 2);
        dn.B = B; dn.Cin = C; dn.Cout = C / 2; dn.h = hh; dn.w = ww; dn.store = 1;
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
            RF_TRY(run_stage(h, 4 + i, ws + p.tA, ws + p.tB, ws, p, B, H, W, st, side));
            continue;
        }
        Conv1x1Args up{};
        up.x1 = ws + p.tB; up.C1 = 2 * C; up.x1_bstride = (int64_t)2 * C * (Pn / 4);
        up.wp = h->pk(h->up_w[i - 1]); up.bias = h->prm(h->up_b[i - 1]);
        up.out = ws + p.tU; up.out_bstride = (int64_t)C * Pn; up.Cout = 4 * C; up.B = B; up.P = Pn / 4; up.w = ww / 2; up.mode = 1;
        RF_TRY(launch_conv1x1(up, st));
        Conv1x1Args cr{};
        cr.x1 = ws + p.tU; cr.C1 = C; cr.x1_bstride = (int64_t)C * Pn;
        cr.x2 = skip[lvl]; cr.C2 = C; cr.x2_bstride = (int64_t)C * Pn;
        cr.wp = h->pk(h->upcr_w[i - 1]); cr.bias = h->prm(h->upcr_b[i - 1]);
        cr.out = ws + p.tA; cr.out_bstride = (int64_t)C * Pn; cr.Cout = C; cr.B = B; cr.P = Pn; cr.w = ww;
        RF_TRY(launch_conv1x1(cr, st));
        RF_TRY(run_stage(h, 4 + i, ws + p.tA, ws + p.tB, ws, p, B, H, W, st, side));
    }
    // conv_out + LeakyReLU + PixelShuffle (+ clamp)
    Conv3x3Args o{};
    o.x = ws + p.tB; o.x_bstride = (int64_t)d * H * W; o.wp = h->pk(h->conv_out_w); o.bias = h->prm(h->conv_out_b);
    o.out = out; o.out_bstride = (int64_t)cfg.out_channels * 4 * H * W;
    o.B = B; o.Cin = d; o.Cout = 4 * cfg.out_channels; o.h = H; o.w = W; o.act = 1; o.store = 2; o.clamp_out = cfg.clamp_io;
    if (cfg.variant == RF_VARIANT_TRUECOLOR) o.act = 2;      // F.relu before the PixelShuffle (BayerTORGBColorMultiLvl.py:458)
    RF_TRY(launch_conv3x3(o, st));
    if (cfg.variant == RF_VARIANT_TRUECOLOR) {
        const ColorCorrIx& cc = h->cc;
        const float* prm[9] = {h->prm(cc.gamma),   h->prm(cc.ct0_w),   h->prm(cc.ct0_b),   h->prm(cc.ct2_w),  h->prm(cc.ct2_b),
                               h->prm(cc.tone0_w), h->prm(cc.tone0_b), h->prm(cc.tone2_w), h->prm(cc.tone2_b)};
        RF_TRY(launch_tc_color_head(out, prm, B, (size_t)4 * H * W, st));
    }
    // colour anchor and luminance nudge (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:403-414)
    if (cfg.variant == RF_VARIANT_MULTILVL) RF_TRY(launch_ml_tail(out, in, mosaic, ws + p.gscratch, B, H, W, levels, st));
    return RF_OK;
}

}  // extern "C"
