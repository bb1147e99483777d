// FLCA_Pyramid (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py:86-183) as a stand-alone operator: the guidance made from
// the packed frame inside the call, levels + 1 gated residual steps through one res_proj, the squeeze-excite gate applied.
//   x_0 = feat;   x_{s+1} = x_s + 0.2 tanh(W2 relu(W0 (x_s S_s) + b0) + b2),  s = 0 .. L;   out = x_{L+1} ch
//   ch = sigmoid(W3 relu(W1 mean_p(x_{L+1}) + b1) + b3) per image
// The schedule is branch_ml's (rf_model.hip) on raw parameter tensors: launch_ml_step_fused where it exists, elsewhere
// launch_ml_modulate, two 1x1 GEMMs (weights packed per call) and launch_ml_residual / launch_tc_residual; the last step leaves the
// pooling sums.  The model folds ch into channel_reduce; here pyr_se_kernel computes it and launch_scale_channels_to applies it.
// pyr_se_kernel is the block's own: launch_flca_se takes multiples of 8 channels only, and the backward (rf_flca_pyramid_bwd.hip)
// runs the same kernel with the adjoint switched on; the MLP and its adjoint are rf_flca_adjoint.h's, the in-order column sums
// are its own.  PyrFwdPlan is the one layout behind the size query and the pointers.
#include "rf_flca_adjoint.h"

namespace rf {

namespace {

// One workgroup per image.  pool [B][nblk][C]: per-block channel sums of x_{L+1}, added in block order.  dch_part == nullptr: the
// gate alone.  Otherwise dch_part [B][dnblk][C] (per-block sums of dz x_{L+1}, added in block order) and the MLP adjoint
// (se_adjoint): the image's share of the four gradients -> g_*[b], dmP
__global__ void __launch_bounds__(256) pyr_se_kernel(const float* __restrict__ pool, int nblk, const float* __restrict__ dch_part, int dnblk,
                                                     const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w3,
                                                     const float* __restrict__ b3, float* __restrict__ ch, float* __restrict__ dmP,
                                                     float* __restrict__ g_w1, float* __restrict__ g_b1, float* __restrict__ g_w3,
                                                     float* __restrict__ g_b3, int C, int hid, int P) {
    __shared__ float mean[512], ds3[512], hv[64], dh[64];
    const size_t b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int k = 0; k < nblk; ++k) s += pool[(b * nblk + k) * C + c];
        mean[c] = s / (float)P;
    }
    __syncthreads();
    se_hidden(w1, b1, mean, hv, C, hid);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float chv = se_gate(w3, b3, hv, c, hid);
        ch[b * C + c] = chv;
        if (dch_part) {      // kernel argument: uniform
            float d = 0.f;
            for (int q = 0; q < dnblk; ++q) d += dch_part[(b * dnblk + q) * C + c];
            ds3[c] = d * chv * (1.0f - chv);
        }
    }
    if (!dch_part) return;
    const size_t n = (size_t)hid * C;
    se_adjoint(w1, w3, mean, hv, ds3, dh, g_w1 + b * n, g_b1 + b * hid, g_w3 + b * n, g_b3 + b * C, dmP + b * C, C, hid, P);
}

}  // namespace

size_t pyr_prm_floats(int i, int C, int levels) {
    const size_t c = C, hid = flca_hidden(C);
    if (i < 2 * levels) return c * 9;                                   // low_attn, high_attn
    if (i < 4 * levels) return (i - 2 * levels) % 2 == 0 ? 4 : 2;       // freq_gate_head weight, bias
    const size_t rest[11] = {c * 18, 1, 1, hid * c, hid, c * hid, c, c * c, c, c * c, c};
    return rest[i - 4 * levels];
}

int pyr_fwd_plan(const char* who, int B, int C, int h, int w, int H, int W, int levels, bool backward, PyrFwdPlan* p, Bump* b) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1,
                 "%s: B=%d C=%d h=%d w=%d H=%d W=%d: every size must be positive and B <= 65535", who, B, C, h, w, H, W);
    RF_CHECK_ARG(C <= 512, "%s: C=%d > 512 not supported", who, C);
    RF_CHECK_ARG(levels >= 1 && levels <= 3, "%s: levels=%d (1..3)", who, levels);
    RF_CHECK_ARG(H % 8 == 0 && W % 8 == 0, "%s: the sides of the packed frame, %d x %d, must be multiples of 8", who, H, W);
    RF_CHECK_ARG((size_t)h * w <= (1u << 28) && (size_t)H * W <= (1u << 28), "%s: a plane of %dx%d or %dx%d exceeds 2^28 pixels", who, h, w, H, W);
    const size_t el = (size_t)B * C * h * w;
    p->fused = ml_step_fused_supported(C, h, w);
    p->nblk = tc_nblk(h, w);
    const bool mtr = backward || !p->fused;
    p->gscratch = b->off(ml_scratch_floats(B, H, W, levels));
    p->guide = b->off((size_t)B * (2 * levels + 2) * h * w);
    p->m = b->off(mtr ? el : 0);
    p->t = b->off(mtr ? el : 0);
    p->r = b->off(mtr ? el : 0);
    p->wp0 = b->off(mtr ? packed1x1_floats(C, C) : 0);
    p->wp2 = b->off(mtr ? packed1x1_floats(C, C) : 0);
    p->pool = b->off((size_t)B * p->nblk * C);
    p->ch = b->off((size_t)B * C);
    return RF_OK;
}

const float* pyr_means(const PyrFwdPlan& p, const float* ws, int B, int H, int W, int levels) {
    return ml_level_means(ws + p.gscratch, 0, B, H, W, levels);
}

namespace {

struct StepPrm { const float *w_a, *w_b, *g_w, *g_b; };
StepPrm step_prm(const PyrGroup<const float*>& prm, int s, int L) {
    return s == L ? StepPrm{prm.chr_w, nullptr, prm.cgate_w, prm.cgate_b} : StepPrm{prm.low[s], prm.high[s], prm.gate_w[s], prm.gate_b[s]};
}

int pack_res_proj(const PyrFwdPlan& p, float* ws, const PyrGroup<const float*>& prm, int C, hipStream_t st) {
    RF_TRY(pack_1x1(prm.r0_w, ws + p.wp0, C, C, C, 1, st));
    return pack_1x1(prm.r2_w, ws + p.wp2, C, C, C, 1, st);
}

}  // namespace

int pyr_step_mtr(const PyrFwdPlan& p, float* ws, const float* x, int step, const PyrGroup<const float*>& prm, bool pack, int B, int C,
                 int h, int w, int H, int W, int levels, hipStream_t st) {
    if (pack) RF_TRY(pack_res_proj(p, ws, prm, C, st));
    const StepPrm s = step_prm(prm, step, levels);
    RF_TRY(launch_ml_modulate(x, ws + p.m, ws + p.guide, pyr_means(p, ws, B, H, W, levels), step, levels, s.w_a, s.w_b, s.g_w, s.g_b, B, C, h, w, st));
    Conv1x1Args r0 = conv1x1_dense(ws + p.m, C, ws + p.wp0, nullptr, prm.r0_b, ws + p.t, C, B, h * w, w);
    r0.act = 2;
    RF_TRY(launch_conv1x1(r0, st));
    return launch_conv1x1(conv1x1_dense(ws + p.t, C, ws + p.wp2, nullptr, prm.r2_b, ws + p.r, C, B, h * w, w), st);
}

int pyr_forward_steps(const PyrFwdPlan& p, float* ws, const float* feat, const float* packed, float* const* x_next,
                      const PyrGroup<const float*>& prm, int B, int C, int h, int w, int H, int W, int levels, hipStream_t st) {
    float* gs = ws + p.gscratch;
    RF_TRY(launch_ml_guidance(packed, 0, gs, B, H, W, levels, st));
    RF_TRY(launch_ml_guide_level(gs, ws + p.guide, 0, B, H, W, levels, h, w, st));
    if (!p.fused) RF_TRY(pack_res_proj(p, ws, prm, C, st));
    const float* cur = feat;
    for (int s = 0; s <= levels; ++s) {
        float* pool = s == levels ? ws + p.pool : nullptr;      // the last step leaves the pooling sums
        if (p.fused) {
            const StepPrm q = step_prm(prm, s, levels);
            RF_TRY(launch_ml_step_fused(cur, x_next[s], ws + p.guide, pyr_means(p, ws, B, H, W, levels), s, levels, q.w_a, q.w_b, q.g_w, q.g_b,
                                        prm.r0_w, prm.r0_b, prm.r2_w, prm.r2_b, pool, B, C, h, w, st));
        } else {
            RF_TRY(pyr_step_mtr(p, ws, cur, s, prm, false, B, C, h, w, H, W, levels, st));
            if (pool) RF_TRY(launch_tc_residual(cur, ws + p.r, x_next[s], pool, B, C, h, w, st));
            else RF_TRY(launch_ml_residual(cur, ws + p.r, x_next[s], B, C, h, w, st));
        }
        cur = x_next[s];
    }
    return RF_OK;
}

int launch_pyr_se(const float* pool, int nblk, int P, const SePrm& se, float* ch, const float* dch_part, int dnblk, float* dmP, float* contrib,
                  int B, int C, hipStream_t st) {
    const int hid = flca_hidden(C);
    RF_CHECK_ARG(C <= 512 && hid <= 64, "FLCA_Pyramid squeeze-excite: C=%d unsupported", C);
    RF_CHECK_ARG(!dch_part || (dmP && contrib), "FLCA_Pyramid squeeze-excite: the adjoint needs dmP and contrib");
    const size_t n = (size_t)B * hid * C, off = dch_part ? 1 : 0;      // (the gate alone: four null pointers)
    float *g_w1 = contrib, *g_b1 = g_w1 + off * n, *g_w3 = g_b1 + off * B * hid, *g_b3 = g_w3 + off * n;
    ProfScope prof(st, "pyr_se_kernel", 0.0, 4.0 * B * ((double)nblk + dnblk + 2.0 * hid) * C);
    pyr_se_kernel<<<B, 256, 0, st>>>(pool, nblk, dch_part, dnblk, se.se1_w, se.se1_b, se.se3_w, se.se3_b, ch, dmP, g_w1, g_b1, g_w3, g_b3, C, hid, P);
    return check_launch("pyr_se");
}

}  // namespace rf

using namespace rf;

extern "C" {

long long rf_flca_pyramid_workspace_bytes(int B, int C, int h, int w, int H, int W, int levels) {
    PyrFwdPlan p;
    Bump b;
    const int rc = pyr_fwd_plan("rf_flca_pyramid_workspace_bytes", B, C, h, w, H, W, levels, false, &p, &b);
    return rc ? rc : (long long)(b.used * sizeof(float));
}

int rf_flca_pyramid_forward(const float* feat, const float* packed, float* out, const float* const* prm, void* workspace,
                            size_t workspace_bytes, int B, int C, int h, int w, int H, int W, int levels, void* stream) {
    const char* const who = "rf_flca_pyramid_forward";
    PyrFwdPlan p;
    Bump b;
    RF_TRY(pyr_fwd_plan(who, B, C, h, w, H, W, levels, false, &p, &b));
    RF_CHECK_ARG(feat && packed && out && prm && workspace && aligned16(feat) && aligned16(packed) && aligned16(out) && aligned16(workspace),
                 "%s: feat, packed, out, prm and workspace must be non-null and 16-byte aligned", who);
    if (workspace_bytes < b.used * sizeof(float)) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, b.used * sizeof(float));
        return RF_E_NOMEM;
    }
    for (int i = 0; i < 4 * levels + 11; ++i) RF_CHECK_ARG(prm[i] != nullptr && aligned4(prm[i]), "%s: parameter %d is null or misaligned", who, i);
    const size_t plane = (size_t)B * C * h * w * sizeof(float);
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(feat), o0 = reinterpret_cast<uintptr_t>(out);
    RF_CHECK_ARG(o0 + plane <= f0 || f0 + plane <= o0, "%s: out may not alias feat", who);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* x_next[4] = {out, out, out, out};                   // every step after the first runs in place
    const PyrGroup<const float*> g = pyr_group(prm, levels);
    RF_TRY(pyr_forward_steps(p, ws, feat, packed, x_next, g, B, C, h, w, H, W, levels, st));
    RF_TRY(launch_pyr_se(ws + p.pool, p.nblk, h * w, g.se, ws + p.ch, nullptr, 0, nullptr, nullptr, B, C, st));
    return launch_scale_channels_to(out, out, ws + p.ch, B, C, h * w, st);
}

}  // extern "C"
