// The WMB block of the WFB variant (RawFomer_WFB_FFAB/model.py:203-245) as the RawFormer handle schedules it, eval mode:
//
//   t  = 2 LN1(x) - 1;  [LL ; high] = dwt_init(t)                         wmb_front_kernel
//   LL = FFAB(depth_conv(conv1([LL ; mean_c LL])))                         1x1 GEMM on the folded weight, dwconv5x5, ffab_forward
//   high = WM(high)                                                        wm_forward, its last convolution writing the high slots
//   u  = t + clamp((iwt_init([LL ; high]) + 1) / 2, 0, 1)                  wmb_back_kernel
//   out = u + ffn(LN2(u)),  ffn(v) = project_out(gate(project_in(v))) + v  1x1 GEMM (LN2 in its prologue), dwgate3x3 on the folded
//                                                                          rep-conv weights, 1x1 GEMM, wmb_ffn_tail_kernel
//
// The three kernels here are HBM-bound element-wise passes with a per-pixel reduction over C.  A lane owns 4 consecutive
// pixels of a row (front: of two adjacent rows, i.e. two 2x2 quads) and walks the channels with 16-byte loads C planes apart;
// a workgroup's 256 lanes cover a strip of quads.  The statistics are the exact two-pass form of layernorm2d_kernel (mean, then
// the centred second moment), so x is read three times by the same lane: once from HBM, twice from L2.  Nothing is kept per
// channel in registers, so the kernels serve C = 4 .. 512 without scratch.  No atomics; every sum runs over c in ascending order.
//
// Algorithmic HBM bytes per element of the full-resolution tensor:
//   front  4 read (x) + 4 written (t) + 4 written (bands) = 12     (layernorm2d 8 + dwt 8 = 16 as separate passes)
//   back   4 read (bands) + 4 read (t) + 4 written        = 12     (iwt 8 + affine_clamp_add 12 = 20)
//   tail   4 read (t) + 4 read (y) + 4 written            = 12     (layernorm2d 8 + residual read in the GEMM 4 + add 12 = 24)
#include "rf_layernorm.h"
#include "rf_handle.h"

namespace rf {

static constexpr int kWb = 256;
static inline unsigned wmb_grid(size_t items) {
    size_t g = (items + kWb - 1) / kWb;
    if (g > 4096) g = 4096;
    return (unsigned)(g < 1 ? 1 : g);
}

// x, t [B][C][2h][2w], bands [4B][C][h][w] (band s of image b at batch index s B + b); 2w % 4 == 0
__global__ void __launch_bounds__(kWb) wmb_front_kernel(const float* __restrict__ x, float* __restrict__ t, float* __restrict__ bands,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, float eps,
                                                        int B, int C, int h, int w) {
    const int W = 2 * w, wv = W / 4;
    const size_t P = (size_t)4 * h * w, bs = (size_t)B * C * h * w, items = (size_t)B * h * wv;
    const float invC = 1.0f / (float)C;
    for (size_t it = blockIdx.x * (size_t)kWb + threadIdx.x; it < items; it += (size_t)gridDim.x * kWb) {
        const int xv = (int)(it % wv), y = (int)((it / wv) % h);
        const size_t b = it / ((size_t)wv * h);
        const size_t o0 = b * C * P + (size_t)(2 * y) * W + 4 * xv;
        const float* r0 = x + o0;
        const float* r1 = r0 + W;
        float m0[4] = {0.f, 0.f, 0.f, 0.f}, m1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            acc4(m0, *reinterpret_cast<const float4*>(r0 + c * P));
            acc4(m1, *reinterpret_cast<const float4*>(r1 + c * P));
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) { m0[v] *= invC; m1[v] *= invC; }
        float q0[4] = {0.f, 0.f, 0.f, 0.f}, q1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            sq4(q0, *reinterpret_cast<const float4*>(r0 + c * P), m0);
            sq4(q1, *reinterpret_cast<const float4*>(r1 + c * P), m1);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) { q0[v] = ln_rstd(q0[v], invC, eps); q1[v] = ln_rstd(q1[v], invC, eps); }
        float* bo = bands + (b * C * h + y) * (size_t)w + 2 * xv;
        for (int c = 0; c < C; ++c) {
            const float g = w2[c], s = b2[c];
            const float4 a = norm4(*reinterpret_cast<const float4*>(r0 + c * P), m0, q0, g, s);
            const float4 d = norm4(*reinterpret_cast<const float4*>(r1 + c * P), m1, q1, g, s);
            *reinterpret_cast<float4*>(t + o0 + c * P) = a;
            *reinterpret_cast<float4*>(t + o0 + c * P + W) = d;
            float2 ll, hl, lh, hh;
            haar_analysis(a.x, a.y, d.x, d.y, ll.x, hl.x, lh.x, hh.x);
            haar_analysis(a.z, a.w, d.z, d.w, ll.y, hl.y, lh.y, hh.y);
            float* o = bo + (size_t)c * h * w;
            *reinterpret_cast<float2*>(o) = ll;
            *reinterpret_cast<float2*>(o + bs) = hl;
            *reinterpret_cast<float2*>(o + 2 * bs) = lh;
            *reinterpret_cast<float2*>(o + 3 * bs) = hh;
        }
    }
}

// out = t + clamp((iwt_init(bands) + 1) / 2, 0, 1)   (blocks.py:123-134, model.py:13-15, 241-243); out may be t
__global__ void __launch_bounds__(kWb) wmb_back_kernel(const float* __restrict__ bands, const float* t, float* out, int B, int C, int h, int w) {
    const int wv = w / 2, W = 2 * w;
    const size_t bs = (size_t)B * C * h * w, items = (size_t)B * C * h * wv;
    for (size_t it = blockIdx.x * (size_t)kWb + threadIdx.x; it < items; it += (size_t)gridDim.x * kWb) {
        const int xv = (int)(it % wv), y = (int)((it / wv) % h);
        const size_t pl = it / ((size_t)wv * h);
        const float* i0 = bands + (pl * h + y) * (size_t)w + 2 * xv;
        const float2 p0 = *reinterpret_cast<const float2*>(i0), p1 = *reinterpret_cast<const float2*>(i0 + bs);
        const float2 p2 = *reinterpret_cast<const float2*>(i0 + 2 * bs), p3 = *reinterpret_cast<const float2*>(i0 + 3 * bs);
        const size_t o = (pl * 2 * h + 2 * y) * (size_t)W + 4 * xv;
        const float4 ta = *reinterpret_cast<const float4*>(t + o), tb = *reinterpret_cast<const float4*>(t + o + W);
        float r[2][4];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            haar_synthesis(k ? p0.y : p0.x, k ? p1.y : p1.x, k ? p2.y : p2.x, k ? p3.y : p3.x, r[0][2 * k], r[0][2 * k + 1], r[1][2 * k], r[1][2 * k + 1]);
        auto f = [](float tv, float v) { return tv + fminf(fmaxf((v + 1.0f) * 0.5f, 0.0f), 1.0f); };
        *reinterpret_cast<float4*>(out + o) = make_float4(f(ta.x, r[0][0]), f(ta.y, r[0][1]), f(ta.z, r[0][2]), f(ta.w, r[0][3]));
        *reinterpret_cast<float4*>(out + o + W) = make_float4(f(tb.x, r[1][0]), f(tb.y, r[1][1]), f(tb.z, r[1][2]), f(tb.w, r[1][3]));
    }
}

// out = t + (y + LN(t)): x + ffn(norm2(x)) where FeedForward adds its own input norm2(x) (model.py:58-65, 244); P % 4 == 0
__global__ void __launch_bounds__(kWb) wmb_ffn_tail_kernel(const float* __restrict__ t, const float* __restrict__ y, float* __restrict__ out,
                                                           const float* __restrict__ gw, const float* __restrict__ gb, float eps,
                                                           int B, int C, size_t P) {
    const size_t pv = P / 4, items = (size_t)B * pv;
    const float invC = 1.0f / (float)C;
    for (size_t it = blockIdx.x * (size_t)kWb + threadIdx.x; it < items; it += (size_t)gridDim.x * kWb) {
        const size_t o0 = (it / pv) * C * P + (it % pv) * 4;
        float m[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) acc4(m, *reinterpret_cast<const float4*>(t + o0 + c * P));
#pragma unroll
        for (int v = 0; v < 4; ++v) m[v] *= invC;
        for (int c = 0; c < C; ++c) sq4(q, *reinterpret_cast<const float4*>(t + o0 + c * P), m);
#pragma unroll
        for (int v = 0; v < 4; ++v) q[v] = ln_rstd(q[v], invC, eps);
        for (int c = 0; c < C; ++c) {
            const float4 tv = *reinterpret_cast<const float4*>(t + o0 + c * P), yv = *reinterpret_cast<const float4*>(y + o0 + c * P);
            const float4 n = norm4(tv, m, q, gw[c], gb[c]);
            *reinterpret_cast<float4*>(out + o0 + c * P) = make_float4(tv.x + (yv.x + n.x), tv.y + (yv.y + n.y), tv.z + (yv.z + n.z), tv.w + (yv.w + n.w));
        }
    }
}

// Pack-time folds of one block (once per parameter load; what ops.fuse_rep_convs / ops.illumination_estimator do on the host):
//   ln2      [2C]      2 w | 2 b - 1 of norm1
//   rep_w    [hid][9]  rep_conv1.c * s1 (+ at the centre tap: rep_conv2.c * s2 + 1),  s = bn.weight / sqrt(bn.running_var + 1e-5)
//   rep_b    [hid]     (bn1.bias - mean1 s1) + (bn2.bias - mean2 s2)
//   illu     [C][C]    W_img + w_mean / C of illu.conv1 [C][C + 1]
struct WmbFoldArgs {
    const float *ln_w, *ln_b, *rep1_w, *bn1[4], *rep2_w, *bn2[4], *illu_w;
    float *ln2, *rep_w, *rep_b, *illu;
    int C, hid;
};
__global__ void __launch_bounds__(kWb) wmb_fold_kernel(WmbFoldArgs a) {
    const int C = a.C, hid = a.hid;
    const int n = max(max(C * C, hid * 9), 2 * C);
    for (int i = blockIdx.x * kWb + threadIdx.x; i < n; i += gridDim.x * kWb) {
        if (i < C) {
            a.ln2[i] = 2.0f * a.ln_w[i];
            a.ln2[C + i] = 2.0f * a.ln_b[i] - 1.0f;
        }
        if (i < hid * 9) {
            const int c = i / 9;
            float v = a.rep1_w[i] * (a.bn1[0][c] / sqrtf(a.bn1[3][c] + 1e-5f));
            if (i % 9 == 4) v = (v + a.rep2_w[c] * (a.bn2[0][c] / sqrtf(a.bn2[3][c] + 1e-5f))) + 1.0f;
            a.rep_w[i] = v;
        }
        if (i < hid) {
            const float s1 = a.bn1[0][i] / sqrtf(a.bn1[3][i] + 1e-5f), s2 = a.bn2[0][i] / sqrtf(a.bn2[3][i] + 1e-5f);
            a.rep_b[i] = (a.bn1[1][i] - a.bn1[2][i] * s1) + (a.bn2[1][i] - a.bn2[2][i] * s2);
        }
        if (i < C * C) {
            const int r = i / C, k = i - r * C;
            a.illu[i] = a.illu_w[r * (C + 1) + k] + a.illu_w[r * (C + 1) + C] / (float)C;
        }
    }
}

static int wmb_shape(const char* who, const void* a, const void* b, const void* c, int B, int C, int h, int w) {
    RF_CHECK_ARG(a && b && c && aligned16(a) && aligned16(b) && aligned16(c), "%s: tensors must be non-null and 16-byte aligned", who);
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 4 && C <= 512, "%s: B %d, C %d (C must be 4 .. 512)", who, B, C);
    RF_CHECK_ARG(h >= 1 && w >= 2 && w % 2 == 0 && (double)h * w * 4.0 * C * B < 9.0e18 && (double)h * w < (double)(1 << 28),
                 "%s: band size %d x %d (the full-resolution width 2w must be a multiple of 4)", who, h, w);
    return RF_OK;
}

int launch_wmb_front(const float* x, float* t, float* bands, const float* w2, const float* b2, int B, int C, int h, int w, hipStream_t st) {
    RF_TRY(wmb_shape("wmb_front", x, t, bands, B, C, h, w));
    RF_CHECK_ARG(w2 && b2, "wmb_front: null LayerNorm parameters");
    const double el = 4.0 * B * C * (double)h * w;
    ProfScope prof(st, "wmb_front_kernel", 12.0 * el, 12.0 * el);
    wmb_front_kernel<<<wmb_grid((size_t)B * h * (w / 2)), kWb, 0, st>>>(x, t, bands, w2, b2, 1e-5f, B, C, h, w);
    return check_launch("wmb_front");
}

int launch_wmb_back(const float* bands, const float* t, float* out, int B, int C, int h, int w, hipStream_t st) {
    RF_TRY(wmb_shape("wmb_back", bands, t, out, B, C, h, w));
    const double el = 4.0 * B * C * (double)h * w;
    ProfScope prof(st, "wmb_back_kernel", 6.0 * el, 12.0 * el);
    wmb_back_kernel<<<wmb_grid((size_t)B * C * h * (w / 2)), kWb, 0, st>>>(bands, t, out, B, C, h, w);
    return check_launch("wmb_back");
}

int launch_wmb_ffn_tail(const float* t, const float* y, float* out, const float* ln_w, const float* ln_b, int B, int C, int h, int w,
                        hipStream_t st) {
    RF_CHECK_ARG(t && y && out && ln_w && ln_b && aligned16(t) && aligned16(y) && aligned16(out), "wmb_ffn_tail: tensors must be non-null and 16-byte aligned");
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 4 && C <= 512, "wmb_ffn_tail: B %d, C %d (C must be 4 .. 512)", B, C);
    RF_CHECK_ARG(h >= 1 && w >= 4 && w % 4 == 0 && (double)h * w < (double)(1 << 30), "wmb_ffn_tail: size %d x %d (the width must be a multiple of 4)", h, w);
    const double el = (double)B * C * h * w;
    ProfScope prof(st, "wmb_ffn_tail_kernel", 12.0 * el, 12.0 * el);
    wmb_ffn_tail_kernel<<<wmb_grid((size_t)B * h * (w / 4)), kWb, 0, st>>>(t, y, out, ln_w, ln_b, 1e-5f, B, C, (size_t)h * w);
    return check_launch("wmb_ffn_tail");
}

int launch_wmb_fold(const float* ln_w, const float* ln_b, float* ln2, const float* rep1_w, const float* const* bn1, const float* rep2_w,
                    const float* const* bn2, float* rep_w, float* rep_b, const float* illu_w, float* illu_fold, int C, int hid, hipStream_t st) {
    WmbFoldArgs a{};
    a.ln_w = ln_w; a.ln_b = ln_b; a.rep1_w = rep1_w; a.rep2_w = rep2_w; a.illu_w = illu_w;
    for (int i = 0; i < 4; ++i) { a.bn1[i] = bn1[i]; a.bn2[i] = bn2[i]; }
    a.ln2 = ln2; a.rep_w = rep_w; a.rep_b = rep_b; a.illu = illu_fold; a.C = C; a.hid = hid;
    int n = C * C > hid * 9 ? C * C : hid * 9;
    if (n < 2 * C) n = 2 * C;
    wmb_fold_kernel<<<wmb_grid((size_t)n), kWb, 0, st>>>(a);
    return check_launch("wmb_fold");
}

// ---- the block's schedule -----------------------------------------------------------------------------------------------
size_t wmb_fold_floats(int C, int hid) { return align_up(2 * (size_t)C, 64) + align_up((size_t)hid * 9, 64) + align_up((size_t)hid, 64) + align_up((size_t)C * C, 64); }

int pack_wmb(rf_handle* h, int stage, float* base, hipStream_t st) {
    const StageIx& x = h->stage[stage];
    const WmbIx& m = x.wmb;
    const int C = h->cfg.dim << x.lvl, hid = m.hid;
    float* ln2 = base + m.fold;
    float* rep_w = ln2 + align_up(2 * (size_t)C, 64);
    float* rep_b = rep_w + align_up((size_t)hid * 9, 64);
    float* illu = rep_b + align_up((size_t)hid, 64);
    const float *bn1[4], *bn2[4];
    for (int i = 0; i < 4; ++i) { bn1[i] = h->prm(m.bn1[i]); bn2[i] = h->prm(m.bn2[i]); }
    RF_TRY(launch_wmb_fold(h->prm(m.ln1_w), h->prm(m.ln1_b), ln2, h->prm(m.rep1_w), bn1, h->prm(m.rep2_w), bn2, rep_w, rep_b,
                           h->prm(m.illu1_w), illu, C, hid, st));
    return pack_1x1(illu, base + m.illu_pk, C, C, C, 1, st);
}

int run_wmb(const rf_handle* h, int stage, const float* in, float* out, const WmbBufs& b, int B, int hh, int ww, hipStream_t st) {
    const StageIx& x = h->stage[stage];
    const WmbIx& m = x.wmb;
    const int C = h->cfg.dim << x.lvl, hid = m.hid, h2 = hh / 2, w2 = ww / 2, Pn = hh * ww, P2 = h2 * w2;
    const float* ln2 = h->packed + m.fold;
    const float* rep_w = ln2 + align_up(2 * (size_t)C, 64);
    const float* rep_b = rep_w + align_up((size_t)hid * 9, 64);
    const size_t U4 = (size_t)B * C * P2;
    // 1. t = 2 LN1(x) - 1 and its four bands
    RF_TRY(launch_wmb_front(in, b.t, b.bands, ln2, ln2 + C, B, C, h2, w2, st));
    // 2. Illumination_Estimator on the LL band: conv1 with the channel mean folded in, depthwise 5x5 (conv2's illu_map is discarded
    //    by WMB.forward and not computed)
    const Conv1x1Args c1 = conv1x1_dense(b.bands, C, h->packed + m.illu_pk, nullptr, h->prm(m.illu1_b), b.illu, C, B, P2, w2);
    RF_TRY(launch_conv1x1(c1, st));
    RF_TRY(launch_dwconv5x5(b.illu, b.fea, h->prm(m.illu_dw_w), h->prm(m.illu_dw_b), B, C, h2, w2, st));
    // 3. FFAB into the LL slot, 4. WM on the three high bands, in place (its first convolution and its token pass are the only
    //    readers of the input, its last convolution the only writer of the output): the IWT reads [LL ; high] as it lies
    const float* fp[92];
    for (int i = 0; i < 92; ++i) fp[i] = h->params[m.ffab[i]].pack >= 0 ? h->pk(m.ffab[i]) : h->prm(m.ffab[i]);
    RF_TRY(ffab_forward(b.fea, b.bands, fp, true, b.ffab, B, C, h2, w2, st));
    const float* wp[17];
    for (int i = 0; i < 17; ++i) wp[i] = h->prm(m.wm[i]);
    const WmPacked pk{h->pk(m.wm[0]), h->pk(m.wm[2]), h->pk(m.wm[15]), h->pk(m.wm[6]), h->pk(m.wm[9]), h->pk(m.wm[14]),
                      h->pk3(m.wm[6]), h->pk3(m.wm[9]), h->pk3(m.wm[14])};
    RF_TRY(wm_forward(b.bands + U4, b.bands + U4, wp, &pk, b.wm, 3 * B, C, h2, w2, st));
    // 5. u = t + clamp((IWT + 1) / 2, 0, 1), over t
    RF_TRY(launch_wmb_back(b.bands, b.t, b.t, B, C, h2, w2, st));
    // 6. project_in(LN2(u)) with the LayerNorm in the GEMM's prologue where that reads u once
    Conv1x1Args pi = conv1x1_dense(b.t, C, h->pk(m.pin_w), h->pk3(m.pin_w), h->prm(m.pin_b), b.hid, hid, B, Pn, ww);
    pi.ln_w = h->prm(m.ln2_w); pi.ln_b = h->prm(m.ln2_b); pi.ln_eps = 1e-5f;
    if (!conv1x1_ln_single_pass(pi)) {
        RF_TRY(launch_layernorm2d(b.t, b.gated, pi.ln_w, pi.ln_b, 1e-5f, B, C, Pn, st));
        pi.x1 = b.gated; pi.ln_w = nullptr; pi.ln_b = nullptr;
    }
    RF_TRY(launch_conv1x1(pi, st));
    // 7. the gate on the folded rep-conv weights, 8. project_out, 9. out = u + y + LN2(u)
    RF_TRY(launch_dwgate3x3(b.hid, b.gated, rep_w, rep_b, h->prm(m.dw_w), h->prm(m.dw_b), B, hid, hh, ww, st));
    const Conv1x1Args po = conv1x1_dense(b.gated, hid, h->pk(m.pout_w), h->pk3(m.pout_w), h->prm(m.pout_b), b.hid, C, B, Pn, ww);
    RF_TRY(launch_conv1x1(po, st));
    return launch_wmb_ffn_tail(b.t, b.hid, out, h->prm(m.ln2_w), h->prm(m.ln2_b), B, C, hh, ww, st);
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_wmb_front(const float* x, float* t, float* bands, const float* w2, const float* b2, int B, int C, int h, int w, void* stream) {
    return launch_wmb_front(x, t, bands, w2, b2, B, C, h, w, (hipStream_t)stream);
}

int rf_wmb_back(const float* bands, const float* t, float* out, int B, int C, int h, int w, void* stream) {
    return launch_wmb_back(bands, t, out, B, C, h, w, (hipStream_t)stream);
}

int rf_wmb_ffn_sum(const float* t, const float* y, float* out, const float* ln_w, const float* ln_b, int B, int C, int h, int w, void* stream) {
    return launch_wmb_ffn_tail(t, y, out, ln_w, ln_b, B, C, h, w, (hipStream_t)stream);
}

}  // extern "C"
