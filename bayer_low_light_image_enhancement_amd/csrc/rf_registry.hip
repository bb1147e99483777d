// RawFormer handle, everything that runs before the first forward: the parameter registry in the reference's state_dict order
// (RawFomer_WFB_FFAB/model.py:437-508 and its siblings), the variant's traits, the pack plan and rf_pack_params.
// Host code only; the schedules that read the handle are rf_model.hip (forward) and rf_trainstep.hip (training).
#include <string>
#include <cstring>
#include "rf_common.h"

using namespace rf;

#include "rf_handle.h"

namespace {

int add_param(rf_handle* h, const std::string& name, std::initializer_list<int64_t> shape, int flags = 0) {
    Param p;
    p.name = name;
    p.flags = flags;      // RF_PARAM_BUFFER | RF_PARAM_UNUSED
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

// <name>.weight of `shape` and <name>.bias of its leading dimension
void add_wb(rf_handle* h, const std::string& name, std::initializer_list<int64_t> shape, int& w, int& b, int flags = 0) {
    w = add_param(h, name + ".weight", shape, flags);
    b = add_param(h, name + ".bias", {*shape.begin()}, flags);
}

void add_pack_1x1(rf_handle* h, int w) {      // the f32 form and the b3 form for the bf16x3 GEMM kernels (rf_common.h)
    add_pack(h, w, PK_1x1);
    add_pack(h, w, PK_1x1_B3);
}

SeGroup<int> add_se(rf_handle* h, const std::string& f, int C) {
    const int hid = flca_hidden(C);
    SeGroup<int> s;
    add_wb(h, f + "se.1", {hid, C, 1, 1}, s.se1_w, s.se1_b);
    add_wb(h, f + "se.3", {C, hid, 1, 1}, s.se3_w, s.se3_b);
    return s;
}

void add_res_proj(rf_handle* h, const std::string& f, int C, int* w0, int* b0, int* w2, int* b2) {
    add_wb(h, f + "res_proj.0", {C, C, 1, 1}, *w0, *b0);
    add_wb(h, f + "res_proj.2", {C, C, 1, 1}, *w2, *b2);
    for (int w : {*w0, *w2}) add_pack_1x1(h, w);
}

// mamba_ssm's Mamba(d, 32, 4, expand) in the order of rf_mamba_forward's pointer array (ops.mamba_param_shapes); the package is
// not available to pin the order of these keys inside the module's state_dict
void add_mamba(rf_handle* h, const std::string& q, int d, int expand, int flags, int* ix) {
    const int di = expand * d, r = cdiv(d, 16);
    ix[0] = add_param(h, q + "in_proj.weight", {2 * di, d}, flags);
    ix[1] = add_param(h, q + "conv1d.weight", {di, 1, 4}, flags);
    ix[2] = add_param(h, q + "conv1d.bias", {di}, flags);
    ix[3] = add_param(h, q + "x_proj.weight", {r + 64, di}, flags);
    ix[4] = add_param(h, q + "dt_proj.weight", {di, r}, flags);
    ix[5] = add_param(h, q + "dt_proj.bias", {di}, flags);
    ix[6] = add_param(h, q + "A_log", {di, 32}, flags);
    ix[7] = add_param(h, q + "D", {di}, flags);
    ix[8] = add_param(h, q + "out_proj.weight", {d, di}, flags);
}

// ---- one Conv_Transformer stage: branch, block, channel_reduce, Conv_out (state_dict order) ------------------------------
void add_branch(rf_handle* h, StageIx& s, const std::string& pre, int C) {
    const std::string f = pre + "FLCA.";
    switch (h->vt.branch) {
    case BR_CONV:
        add_wb(h, pre + "conv", {C, C, 3, 3}, s.conv_w, s.conv_b);
        add_pack(h, s.conv_w, PK_3x3);
        break;
    case BR_FLCA:
        s.flca.alpha = add_param(h, f + "alpha", {});
        s.flca.beta = add_param(h, f + "beta", {});
        s.flca.gamma = add_param(h, f + "gamma", {});
        s.flca.w_low = add_param(h, f + "low_attn.0.weight", {C, 1, 3, 3});
        s.flca.w_high = add_param(h, f + "high_attn.0.weight", {C, 1, 3, 3});
        s.flca.w_chr = add_param(h, f + "chroma_attn.0.weight", {C, 2, 3, 3});
        s.flca.se = add_se(h, f, C);
        break;
    case BR_TC:      // EnhancedFLCA (BayerTORGBColorMultiLvl.py:192-231)
        add_wb(h, f + "color_attention.0", {C, 5, 3, 3}, s.tc.col_w, s.tc.col_b);
        add_wb(h, f + "low_attn.0", {C, 1, 3, 3}, s.tc.low_w, s.tc.low_b);
        add_wb(h, f + "high_attn.0", {C, 1, 3, 3}, s.tc.high_w, s.tc.high_b);
        s.tc.se = add_se(h, f, C);
        add_res_proj(h, f, C, &s.tc.res0_w, &s.tc.res0_b, &s.tc.res2_w, &s.tc.res2_b);
        break;
    case BR_ML: {    // FLCA_Pyramid (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:90-116)
        MlIx& m = s.ml;
        const int L = h->vt.levels;
        for (int l = 0; l < L; ++l) m.low_w[l] = add_param(h, f + "low_attn." + std::to_string(l) + ".0.weight", {C, 1, 3, 3});
        for (int l = 0; l < L; ++l) m.high_w[l] = add_param(h, f + "high_attn." + std::to_string(l) + ".0.weight", {C, 1, 3, 3});
        for (int l = 0; l < L; ++l) add_wb(h, f + "freq_gate_head." + std::to_string(l), {2, 2, 1, 1}, m.gate_w[l], m.gate_b[l]);
        m.chr_w = add_param(h, f + "chroma_attn.0.weight", {C, 2, 3, 3});
        add_wb(h, f + "chroma_gate", {1, 1, 1, 1}, m.cgate_w, m.cgate_b);
        m.se = add_se(h, f, C);
        add_res_proj(h, f, C, &m.res0_w, &m.res0_b, &m.res2_w, &m.res2_b);
        break;
    }
    }
}

void add_transformer(rf_handle* h, StageIx& s, const std::string& t, int C, int hc) {
    const int heads = h->cfg.heads[s.lvl];
    add_wb(h, t + "norm1.body", {C}, s.ln1_w, s.ln1_b);
    s.temperature = add_param(h, t + (h->vt.log_temperature ? "attn.log_temperature" : "attn.temperature"), {heads, 1, 1});
    add_wb(h, t + "attn.qkv", {3 * C, C, 1, 1}, s.qkv_w, s.qkv_b);
    add_wb(h, t + "attn.qkv_dwconv", {3 * C, 1, 3, 3}, s.qkv_dw_w, s.qkv_dw_b);
    add_wb(h, t + "attn.project_out", {C, C, 1, 1}, s.proj_w, s.proj_b);
    add_wb(h, t + "norm2.body", {C}, s.ln2_w, s.ln2_b);
    add_wb(h, t + "ffn.pointwise1", {hc, C, 1, 1}, s.pw1_w, s.pw1_b);
    add_wb(h, t + "ffn.depthwise", {hc, 1, 3, 3}, s.dw_w, s.dw_b);
    add_wb(h, t + "ffn.pointwise2", {C, hc, 1, 1}, s.pw2_w, s.pw2_b);
    for (int w : {s.qkv_w, s.pw1_w, s.pw2_w}) add_pack(h, w, PK_1x1);
    for (int w : {s.qkv_w, s.pw1_w, s.pw2_w}) add_pack(h, w, PK_1x1_B3);
}

// WMB (RawFomer_WFB_FFAB/model.py:203-245).  Every GEMM and 3x3 weight is packed once (rf_pack_params); illu.conv2 and mb.model2
// are registered and never read.
void add_wmb(rf_handle* h, WmbIx& m, const std::string& t, int C, int hid) {
    int unused[9];
    m.hid = hid;
    add_wb(h, t + "norm1.body", {C}, m.ln1_w, m.ln1_b);
    add_wb(h, t + "illu.conv1", {C, C + 1, 1, 1}, m.illu1_w, m.illu1_b);
    add_wb(h, t + "illu.depth_conv", {C, 1, 5, 5}, m.illu_dw_w, m.illu_dw_b);
    add_wb(h, t + "illu.conv2", {C, C, 1, 1}, unused[0], unused[1], RF_PARAM_UNUSED);
    int* f = m.ffab;
    auto conv = [&](const std::string& q, int cout, int cin) {
        add_wb(h, q, {cout, cin, 1, 1}, f[0], f[1]);
        add_pack(h, f[0], PK_1x1);
        f += 2;
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
    add_wb(h, t + "norm2.body", {C}, m.ln2_w, m.ln2_b);
    auto conv_bn = [&](const std::string& q, int k, int& w, int* bn) {
        w = add_param(h, q + "c.weight", {hid, 1, k, k});
        add_wb(h, q + "bn", {hid}, bn[0], bn[1]);
        bn[2] = add_param(h, q + "bn.running_mean", {hid}, RF_PARAM_BUFFER);
        bn[3] = add_param(h, q + "bn.running_var", {hid}, RF_PARAM_BUFFER);
    };
    conv_bn(t + "ffn.rep_conv1.", 3, m.rep1_w, m.bn1);
    conv_bn(t + "ffn.rep_conv2.", 1, m.rep2_w, m.bn2);
    add_wb(h, t + "ffn.project_in", {hid, C, 1, 1}, m.pin_w, m.pin_b);
    add_wb(h, t + "ffn.dwconv", {hid, 1, 3, 3}, m.dw_w, m.dw_b);
    add_wb(h, t + "ffn.project_out", {C, hid, 1, 1}, m.pout_w, m.pout_b);
    for (int w : {m.pin_w, m.pout_w}) add_pack_1x1(h, w);
    const std::string mb = t + "mb.";
    add_wb(h, mb + "convb.0", {2 * C, C, 3, 3}, m.wm[0], m.wm[1]);
    add_wb(h, mb + "convb.2", {C, 2 * C, 3, 3}, m.wm[2], m.wm[3]);
    add_mamba(h, mb + "model1.", C, 2, 0, m.wm + 6);
    add_mamba(h, mb + "model2.", C, 9, RF_PARAM_UNUSED, unused);
    add_wb(h, mb + "smooth", {C, C, 3, 3}, m.wm[15], m.wm[16]);
    add_wb(h, mb + "ln", {C}, m.wm[4], m.wm[5]);
    for (int w : {m.wm[0], m.wm[2], m.wm[15]}) add_pack(h, w, PK_3x3);
    for (int w : {m.wm[6], m.wm[9], m.wm[14]}) add_pack_1x1(h, w);
    m.fold = h->packed_floats;
    h->packed_floats += wmb_fold_floats(C, hid);
    m.illu_pk = h->packed_floats;
    h->packed_floats += align_up(packed1x1_floats(C, C), 64);
}

void add_stage(rf_handle* h, int i, int lvl) {
    const VariantTraits& vt = h->vt;
    const int C = h->cfg.dim << lvl, hc = C * h->cfg.ffn_expansion;
    StageIx& s = h->stage[i];
    s.lvl = lvl;
    s.first = (int)h->params.size();
    const std::string pre = "conv_tran" + std::to_string(i) + ".";
    add_branch(h, s, pre, C);
    if (vt.wmb_block) add_wmb(h, s.wmb, pre + "Transformer.", C, hc);
    else add_transformer(h, s, pre + "Transformer.", C, hc);
    add_wb(h, pre + "channel_reduce", {C, 2 * C, 1, 1}, s.cr_w, s.cr_b);
    add_wb(h, pre + "Conv_out", {C, C, 3, 3}, s.out_w, s.out_b);
    const bool static_cr = vt.branch == BR_CONV;      // the other branches fold their gate into channel_reduce per image
    if (static_cr) add_pack_1x1(h, s.cr_w);
    if (!vt.wmb_block && tail_composable(C, hc)) {      // pointwise2 composed into channel_reduce (run_stage)
        s.tail_offset = h->packed_floats;
        h->packed_floats += align_up(tail_composed_floats(C, hc), 64);
        if (static_cr) {
            s.tail3_offset = h->packed_floats;
            h->packed_floats += align_up(packed1x1_b3_floats(2 * C + hc, C), 64);
        }
    }
    add_pack(h, s.out_w, PK_3x3);
}

// TrueColor's front end and colour head: EnhancedBayerProcessor (BayerTORGBColorMultiLvl.py:73-98), CameraAwareColorCorrection (:139-158)
void add_bayer_processor(rf_handle* h) {
    BayerProcIx& bp = h->bp;
    bp.wb_gains = add_param(h, "bayer_processor.wb_gains", {4});
    bp.color_matrix = add_param(h, "bayer_processor.color_matrix", {3, 4});
    add_wb(h, "bayer_processor.demosaic_refine.0", {32, 3, 3, 3}, bp.dm0_w, bp.dm0_b);
    add_wb(h, "bayer_processor.demosaic_refine.2", {3, 32, 3, 3}, bp.dm2_w, bp.dm2_b);
    add_wb(h, "bayer_processor.chroma_extractor.0", {16, 4, 3, 3}, bp.ce0_w, bp.ce0_b);
    add_wb(h, "bayer_processor.chroma_extractor.2", {2, 16, 3, 3}, bp.ce2_w, bp.ce2_b);
    for (int w : {bp.dm0_w, bp.dm2_w, bp.ce0_w, bp.ce2_w}) add_pack(h, w, PK_3x3);
}

void add_color_correction(rf_handle* h) {
    ColorCorrIx& cc = h->cc;
    cc.gamma = add_param(h, "color_correction.gamma_param", {});
    add_wb(h, "color_correction.color_transform.0", {64, 3, 1, 1}, cc.ct0_w, cc.ct0_b);
    add_wb(h, "color_correction.color_transform.2", {3, 64, 1, 1}, cc.ct2_w, cc.ct2_b);
    add_wb(h, "color_correction.tone_curve.0", {32, 1, 1, 1}, cc.tone0_w, cc.tone0_b);
    add_wb(h, "color_correction.tone_curve.2", {1, 32, 1, 1}, cc.tone2_w, cc.tone2_b);
}

}  // namespace

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
    VariantTraits& vt = h->vt;
    const int v = cfg->variant;
    vt.branch = v == RF_VARIANT_FLCA ? BR_FLCA : v == RF_VARIANT_TRUECOLOR ? BR_TC : v == RF_VARIANT_MULTILVL ? BR_ML : BR_CONV;
    vt.wmb_block = wfb;
    vt.branch_after = vt.branch == BR_TC || vt.branch == BR_ML;
    vt.levels = cfg->flca_levels > 0 ? cfg->flca_levels : 2;
    vt.guide_planes = vt.branch == BR_ML ? 2 * vt.levels + 2 : vt.branch == BR_TC ? 7 : 4;
    vt.log_temperature = vt.branch == BR_TC;
    vt.shardable = v == RF_VARIANT_FLCA || v == RF_VARIANT_PLAIN;
    vt.stage_needs_packed_frame = vt.branch == BR_FLCA || vt.branch == BR_ML || vt.branch == BR_TC;
    if (vt.branch == BR_TC) add_bayer_processor(h);
    add_wb(h, "embedding", {d, 4 * cfg->inp_channels, 3, 3}, h->embedding_w, h->embedding_b);
    add_pack(h, h->embedding_w, PK_3x3);
    for (int i = 1; i <= 3; ++i) {
        const int C = d << (i - 1);
        add_stage(h, i, i - 1);
        // (the multi-level file's down<i> is a bare nn.Sequential: no `body`)
        h->down_w[i - 1] = add_param(h, "down" + std::to_string(i) + (vt.branch == BR_ML ? ".0.weight" : ".body.0.weight"), {C / 2, C, 3, 3});
        add_pack(h, h->down_w[i - 1], PK_3x3);
    }
    add_stage(h, 4, 3);
    for (int i = 1; i <= 3; ++i) {
        const int lvl = 3 - i, C = d << lvl;
        h->up_w[i - 1] = add_param(h, "up" + std::to_string(i) + ".weight", {2 * C, C, 2, 2});
        h->up_b[i - 1] = add_param(h, "up" + std::to_string(i) + ".bias", {C});
        add_wb(h, "channel_reduce" + std::to_string(i), {C, 2 * C, 1, 1}, h->upcr_w[i - 1], h->upcr_b[i - 1]);
        add_pack(h, h->up_w[i - 1], PK_CONVT);      // the two-kernel form stays available for widths that are not
        add_pack(h, h->upcr_w[i - 1], PK_1x1);      // multiples of 4 (e.g. level 3 of a 1424 x 2128 frame)
        h->upcat_offset[i - 1] = h->packed_floats;
        h->packed_floats += align_up(upcat_packed_floats(C), 64);
        add_stage(h, 4 + i, lvl);
    }
    add_wb(h, "conv_out", {4 * cfg->out_channels, d, 3, 3}, h->conv_out_w, h->conv_out_b);
    add_pack(h, h->conv_out_w, PK_3x3);
    if (vt.branch == BR_TC) add_color_correction(h);
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
    if (h->vt.wmb_block)
        for (int i = 1; i <= 7; ++i)
            if (int rc = pack_wmb(h, i, base, st)) {
                h->packed = nullptr;
                return rc;
            }
    return RF_OK;
}

}  // extern "C"
