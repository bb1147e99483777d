// TransformerBlock schedule (a7):  x1 = x + attn(LN1(x));  out = x1 + ffn(LN2(x1)).
// Shared by the whole-model forward (rf_model.hip) and the operator entry point
// rf_transformer_block (rf_api.hip).  Host code only.
#include <cstdlib>
#include "rf_common.h"

namespace rf {

size_t transformer_scratch_floats(int B, int C, int heads, int hc, int h, int w, TbBufOffsets* o) {
    const size_t P = (size_t)h * w;
    Bump b;
    const size_t wide = (size_t)(3 * C > hc ? 3 * C : hc);
    o->bufA = b.off((size_t)B * wide * P);
    o->bufB = b.off((size_t)B * wide * P);
    o->x1 = b.off((size_t)B * C * P);
    int ns, sl;
    size_t pf = 0, pf2 = 0;
    if (gram_plan(B, C, heads, (int)P, &ns, &sl, &pf)) return 0;   // unsupported head layout: rf_last_error() says why
    if (fused_attn_supported(C, heads, h, w)) { size_t used; fused_attn_plan(h, w, &ns, &used, B, C, nullptr, &pf2); }
    if (attn_mid_supported(C, heads, h, w)) attn_mid_plan(h, w, &ns, &pf2, B, C);
    o->partial = b.off(pf > pf2 ? pf : pf2);
    o->wfold = b.off((size_t)B * packed1x1_floats(C, C));
    o->wfold3 = b.off((size_t)B * packed1x1_b3_floats(C, C));
    return b.used;
}

bool transformer_ffn_is_fused(const TbParams& p, int C, int hc, int hh, int ww) {
#ifdef RF_DIAG
    if (getenv("RF_NO_FUSE") || getenv("RF_NO_FUSE_FFN")) return false;
#endif
    return p.pw1_wp3 && fused_ffn_supported(C, hc, hh, ww);
}

int run_chan_attn(const TbParams& p, const float* in, float* out, bool residual, const AttnBufs& buf, int B, int C, int heads, int hh, int ww,
                  hipStream_t st, bool no_fuse, bool no_fuse_attn, FfnProj* proj) {
    const int Pn = hh * ww;
    float* const partial = buf.partial;
    Conv1x1Args av{};
    int nslab = 0;
    size_t partial_floats = 0;
    if (p.ln1_w && !no_fuse_attn && fused_attn_supported(C, heads, hh, ww)) {
        // LN1 -> qkv 1x1 -> depthwise 3x3 -> {Gram partials, v} in one kernel: qkv never reaches HBM
        RF_TRY(fused_attn_plan(hh, ww, &nslab, &partial_floats, B, C));
        AttnFrontArgs f{};
        f.x = in; f.v = buf.qkv; f.partial = partial; f.nslab = nslab;
        f.ln_w = p.ln1_w; f.ln_b = p.ln1_b; f.wp = p.qkv_wp3; f.bq = p.qkv_b; f.wd = p.qkv_dw_w; f.bd = p.qkv_dw_b;
        f.B = B; f.h = hh; f.w = ww;
        f.ylo = p.ylo; f.yhi = p.yhi; f.xlo = p.xlo; f.xhi = p.xhi;
        RF_TRY(launch_attn_front(f, C, st));
        av.x1 = buf.qkv; av.x1_bstride = (int64_t)C * Pn;
    } else {
        Conv1x1Args q{};
        q.x1 = in; q.C1 = C; q.x1_bstride = (int64_t)C * Pn;
        q.wp = p.qkv_wp; q.wp3 = p.qkv_wp3; q.bias = p.qkv_b;
        q.ln_w = p.ln1_w; q.ln_b = p.ln1_b; q.ln_eps = 1e-5f;
        q.out = buf.pre; q.out_bstride = (int64_t)3 * C * Pn; q.Cout = 3 * C; q.B = B; q.P = Pn; q.w = ww;
        if (!conv1x1_ln_single_pass(q)) {      // LN1 as its own pass (buf.qkv is free until the depthwise kernel writes it)
            RF_TRY(launch_layernorm2d(in, buf.qkv, p.ln1_w, p.ln1_b, 1e-5f, B, C, Pn, st));
            q.x1 = buf.qkv; q.ln_w = nullptr; q.ln_b = nullptr;
        }
        RF_TRY(launch_conv1x1(q, st));

        if (!no_fuse && attn_mid_supported(C, heads, hh, ww)) {
            // depthwise 3x3 of q, k, v + Gram partials in one kernel: dw(q), dw(k) never reach HBM
            RF_TRY(attn_mid_plan(hh, ww, &nslab, &partial_floats, B, C));
            AttnMidArgs m{};
            m.qkv = buf.pre; m.v = buf.qkv; m.partial = partial; m.nslab = nslab;
            m.wd = p.qkv_dw_w; m.bd = p.qkv_dw_b;
            m.B = B; m.h = hh; m.w = ww;
            m.ylo = p.ylo; m.yhi = p.yhi; m.xlo = p.xlo; m.xhi = p.xhi;
            RF_TRY(launch_attn_mid(m, C, st));
            av.x1 = buf.qkv; av.x1_bstride = (int64_t)C * Pn;
        } else {
            DwConvArgs d{};
            d.x = buf.pre; d.x_bstride = (int64_t)3 * C * Pn; d.out = buf.qkv; d.out_bstride = (int64_t)3 * C * Pn;
            d.w = p.qkv_dw_w; d.bias = p.qkv_dw_b;
            d.B = B; d.C = 3 * C; d.h = hh; d.w_ = ww; d.gelu = 0;
            RF_TRY(launch_dwconv3x3(d, st));

            GramArgs g{};
            g.q = buf.qkv; g.k = buf.qkv + (size_t)C * Pn; g.bstride = (int64_t)3 * C * Pn;
            g.B = B; g.C = C; g.heads = heads; g.P = Pn; g.partial = partial;
            RF_TRY(gram_plan(B, C, heads, Pn, &g.nslab, &g.slab, &partial_floats));
            g.p_lo = p.ylo * ww; g.p_hi = p.yhi * ww;
            if (p.xhi > 0 && (p.xlo > 0 || p.xhi < ww)) { g.w = ww; g.x_lo = p.xlo; g.x_hi = p.xhi; }
            RF_TRY(launch_gram(g, st));
            nslab = g.nslab;
            av.x1 = buf.qkv + (size_t)2 * C * Pn; av.x1_bstride = (int64_t)3 * C * Pn;
        }
    }
    // spatial shard: every rank holds the same slab grid (equal local shapes), so the element-wise sum of the partial buffers is
    // the partial buffer of the whole frame; the fold then sums the slabs as always
    if (p.allreduce) p.allreduce(p.allreduce_user, partial, partial_floats, 0, (void*)st);
    if (proj) {
        // the fused FFN kernel applies the projection (launch_ffn_fused): the fold writes the b3 form alone, rows permuted, and the
        // attention half ends here
        RF_CHECK_ARG(residual && C == 32, "chan_attn: the projection moves into the FFN kernel at C = 32, with the residual (C = %d)", C);
        RF_TRY(launch_attn_fold(partial, nslab, p.temperature, p.proj_w, nullptr, buf.wfold3, B, C, heads, st, p.log_temperature, true));
        *proj = FfnProj{av.x1, av.x1_bstride, buf.wfold3, p.proj_b};
        return RF_OK;
    }
    RF_TRY(launch_attn_fold(partial, nslab, p.temperature, p.proj_w, buf.wfold, buf.wfold3, B, C, heads, st, p.log_temperature));
    av.C1 = C;
    av.wp = buf.wfold; av.wp_bstride = (int64_t)packed1x1_floats(C, C);
    av.wp3 = buf.wfold3; av.wp3_bstride = (int64_t)packed1x1_b3_floats(C, C);
    av.bias = p.proj_b;
    if (residual) { av.res = in; av.res_bstride = (int64_t)C * Pn; }
    av.out = out; av.out_bstride = (int64_t)C * Pn; av.Cout = C; av.B = B; av.P = Pn; av.w = ww;
    return launch_conv1x1(av, st);
}

int run_transformer(const TbParams& p, const float* in, float* out, float* ws, const TbBufOffsets& o,
                    int B, int C, int heads, int hc, int hh, int ww, hipStream_t st) {
    RF_TRY(run_transformer_attn(p, in, ws, o, B, C, heads, hh, ww, st));
    return run_transformer_ffn(p, out, ws, o, B, C, hc, hh, ww, st);
}

// x + attn(LN1(x)) -> x1 ---------------------------------------------------------------------
int run_transformer_attn(const TbParams& p, const float* in, float* ws, const TbBufOffsets& o, int B, int C, int heads, int hh, int ww,
                         hipStream_t st, FfnProj* proj) {
#ifdef RF_DIAG   // diagnostic build only (build.py --diag): force the op-by-op path; the shipped library has no switch
    const bool no_fuse = getenv("RF_NO_FUSE") != nullptr;
    const bool no_fuse_attn = no_fuse || getenv("RF_NO_FUSE_ATTN") != nullptr;
#else
    constexpr bool no_fuse = false, no_fuse_attn = false;
#endif

    return run_chan_attn(p, in, ws + o.x1, true, AttnBufs{ws + o.bufA, ws + o.bufB, ws + o.partial, ws + o.wfold, ws + o.wfold3}, B, C, heads,
                         hh, ww, st, no_fuse, no_fuse_attn, proj);
}

// x1 + ffn(LN2(x1)) -> out -------------------------------------------------------------------
int run_transformer_ffn(const TbParams& p, float* out, float* ws, const TbBufOffsets& o, int B, int C, int hc, int hh, int ww, hipStream_t st,
                        const float* proj_in, const FfnProj* proj) {
    const int Pn = hh * ww;
    float* bufA = ws + o.bufA;
    float* bufB = ws + o.bufB;
    float* x1 = ws + o.x1;
    const bool fused = transformer_ffn_is_fused(p, C, hc, hh, ww);
    RF_CHECK_ARG(!p.tail.xs || (fused && fused_ffn_tail_supported(C)), "transformer: the stage tail needs the fused FFN kernel (C = %d)", C);
    RF_CHECK_ARG(!proj || (p.tail.xs && proj_in), "transformer: the projection moves into the FFN kernel only with the stage tail");
    if (fused) {
        // LN2 -> 1x1 -> depthwise 3x3 -> GELU -> 1x1 + residual in one kernel: the hidden tensor stays on chip
        FfnArgs f{};
        f.x = proj ? proj_in : x1; f.out = out;      // proj: the kernel forms x1 itself
        f.ln_w = p.ln2_w; f.ln_b = p.ln2_b; f.w1p = p.pw1_wp3; f.b1 = p.pw1_b; f.wd = p.dw_w; f.bd = p.dw_b; f.w2p = p.pw2_wp; f.b2 = p.pw2_b;
        f.B = B; f.h = hh; f.w = ww;
        if (p.tail.xs) f.b2 = p.tail_bias;      // ... and the caller's channel_reduce on top
        RF_TRY(launch_ffn_fused(f, C, st, p.tail, proj));
    } else {
        Conv1x1Args f1{};
        f1.x1 = x1; f1.C1 = C; f1.x1_bstride = (int64_t)C * Pn;
        f1.wp = p.pw1_wp; f1.wp3 = p.pw1_wp3; f1.bias = p.pw1_b;
        f1.ln_w = p.ln2_w; f1.ln_b = p.ln2_b; f1.ln_eps = 1e-5f;
        f1.out = bufA; f1.out_bstride = (int64_t)hc * Pn; f1.Cout = hc; f1.B = B; f1.P = Pn; f1.w = ww;
        if (!conv1x1_ln_single_pass(f1)) {     // LN2 as its own pass (bufB: the projection GEMM has consumed v)
            RF_TRY(launch_layernorm2d(x1, bufB, p.ln2_w, p.ln2_b, 1e-5f, B, C, Pn, st));
            f1.x1 = bufB; f1.ln_w = nullptr; f1.ln_b = nullptr;
        }
        RF_TRY(launch_conv1x1(f1, st));
        RF_CHECK_ARG(!p.defer_dw || p.defer_pw2, "transformer: the depthwise convolution is deferred only together with pointwise2");
        if (p.defer_dw) return RF_OK;

        DwConvArgs d2{};
        d2.x = bufA; d2.x_bstride = (int64_t)hc * Pn; d2.out = bufB; d2.out_bstride = (int64_t)hc * Pn;
        d2.w = p.dw_w; d2.bias = p.dw_b;
        d2.B = B; d2.C = hc; d2.h = hh; d2.w_ = ww; d2.gelu = 1;
        RF_TRY(launch_dwconv3x3(d2, st));
        if (p.defer_pw2) return RF_OK;

        Conv1x1Args f2{};
        f2.x1 = bufB; f2.C1 = hc; f2.x1_bstride = (int64_t)hc * Pn;
        f2.wp = p.pw2_wp; f2.wp3 = p.pw2_wp3; f2.bias = p.pw2_b;
        f2.res = x1; f2.res_bstride = (int64_t)C * Pn;
        f2.out = out; f2.out_bstride = (int64_t)C * Pn; f2.Cout = C; f2.B = B; f2.P = Pn; f2.w = ww;
        RF_TRY(launch_conv1x1(f2, st));
    }
    return RF_OK;
}

}  // namespace rf
