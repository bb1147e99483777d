// The gradient of a whole WMB block (RawFomer_WFB_FFAB/model.py:203-245) as ONE host schedule over the operators of rf_wmb.hip,
// rf_ffab.hip, rf_mamba.hip, rf_wfb_train.hip, rf_ffab_bwd.hip, rf_wm_bwd.hip and rf_wmb_bwd.hip.  With the names of rf_wmb.hip's header:
//
//   recompute   1  t, [LL ; hi] = front(x)                  rf_wmb_front on [2 w | 2 b - 1] of norm1 (wmb_bwd_fold_kernel, below)
//               2  fea = depth_conv(conv1([LL ; mean LL]))  rf_conv1x1 on the folded weight (the same kernel), rf_dwconv5x5
//               3  LL' = FFAB(fea)                          rf_ffab, into the LL slot of a second band buffer
//               4  hi' = WM(hi)                             rf_wm_forward, into its three high slots
//               5  u = t + clamp((iwt([LL' ; hi']) + 1) / 2, 0, 1)      rf_wmb_back, over t
//               6  v = LN2(u)                               rf_layernorm2d
//   walk back   7  grad_v = d ffn(v) / dv ^T grad_out       rf_wfb_ffn_backward (carries FeedForward's own identity)
//               8  grad_u = grad_out + LN2^T(grad_v)        rf_layernorm2d_backward, residual = grad_out
//               9  grad_[LL' ; hi'] = back^T(grad_u)        rf_wmb_back_backward
//              10  grad_fea = FFAB^T(grad_LL')              rf_ffab_backward
//              11  grad_LL = illu^T(grad_fea)               rf_illumination_estimator_backward, no grad_map
//              12  grad_hi = WM^T(grad_hi')                 rf_wm_backward
//              13  grad_x = front^T(grad_t = grad_u, [grad_LL ; grad_hi])       rf_wmb_front_backward, grad_scale 2: straight into norm1's gradients
//
// Every step is the entry point an ops.* call reaches, on the same arguments: the block's gradient has the bits of that composition.
// The LL band and the three high bands are the leading B and the trailing 3B images of one [4B,C,h/2,w/2] buffer (run_wmb's
// layout), for the activations and for the gradients alike: nothing is concatenated.  FFAB and WM recompute their forward inside
// their backward, so steps 3 and 4 run twice per call ("WMB backward", has what that costs).
//
// Workspace (floats, every buffer rounded up to 64; U = B C h w, the plane):
//   tu     U      t, then u (rf_wmb_back writes over its t)                       steps 1-8
//   bands  U      [LL ; hi]                                                       1-12
//   bands2 U      [LL' ; hi']                                                     3-9
//   fea    U / 4                                                                  2-10
//   gfea   U / 4  grad_fea                                                        10-11
//   va     U      conv1's output in its first quarter (2), v (6-7), then grad_[LL' ; hi'] (9-12)
//   vb     U      grad_v (7-8), then [grad_LL ; grad_hi] (11-13)
//   gu     U      grad_u                                                          8-13
//   fold   2C + C^2     [2 w | 2 b - 1] of norm1 and illu.conv1 with the channel mean folded in
//   sub    the LARGEST of the workspaces of the calls above, which run one after another on one stream
#include <string>
#include "rf_grad.h"

namespace rf {

namespace {

constexpr int kBlk = 256;
// the block's 131 parameters in state_dict order, then the four BatchNorm buffers of ffn
enum { kN1 = 0, kIllu = 2, kFfab = 8, kN2 = 100, kFfn = 102, kMb = 114, kWmbPrm = 131, kWmbTensors = 135 };

// ln2 [2C] = [2 w | 2 b - 1] of norm1 (data_transform folded into the LayerNorm's affine); wf [C][C] = W_img + w_mean / C of
// illu.conv1.weight [C][C + 1] (wmb_fold_kernel's two folds, for a caller without a handle)
__global__ void __launch_bounds__(kBlk) wmb_bwd_fold_kernel(const float* __restrict__ ln_w, const float* __restrict__ ln_b, const float* __restrict__ w1,
                                                            float* __restrict__ ln2, float* __restrict__ wf, int C) {
    for (int i = blockIdx.x * kBlk + threadIdx.x; i < C * C; i += gridDim.x * kBlk) {
        if (i < C) {
            ln2[i] = 2.0f * ln_w[i];
            ln2[C + i] = 2.0f * ln_b[i] - 1.0f;
        }
        const int r = i / C, k = i - r * C;
        wf[i] = w1[r * (C + 1) + k] + w1[r * (C + 1) + C] / (float)C;
    }
}

size_t wmb_prm_floats(int i, int C, int hidden) {
    if (i < kIllu || (i >= kN2 && i < kFfn)) return (size_t)C;
    if (i < kFfab) return illu_prm_floats(i - kIllu, C, C, C);
    if (i < kN2) return ffab_prm_floats(i - kFfab, C);
    if (i < kMb) return wfb_prm_floats(i - kFfn, C, hidden);
    return wm_prm_floats(i - kMb, C);
}

struct WmbBwdPlan { size_t tu, bands, bands2, fea, gfea, va, vb, gu, ln2, wf, sub, sub_bytes, total; };

// h, w: the full-resolution plane.  Every limit of the calls above, refused here under the caller's name
int wmb_bwd_plan(const char* who, int B, int C, int hidden, int h, int w, WmbBwdPlan* p) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 / 3, "%s: B %d (1 .. %d: WM runs on 3 B images)", who, B, 65535 / 3);
    RF_CHECK_ARG(C >= 4 && C <= 512 && C % 4 == 0, "%s: C %d (the channels must be a multiple of 4 in 4 .. 512)", who, C);
    RF_CHECK_ARG(hidden >= 4 && hidden <= 65535 && hidden % 4 == 0, "%s: hidden %d (ffn's channels must be a multiple of 4 in 4 .. 65535)", who, hidden);
    RF_CHECK_ARG(h >= 2 && w >= 4 && h % 2 == 0 && w % 4 == 0, "%s: plane %d x %d (the height must be even, the width a multiple of 4)", who, h, w);
    const int bh = h / 2, bw = w / 2;
    for (const int len : {bh, bw})
        RF_CHECK_ARG(len >= 2 && len <= 4096 && (len <= 2048 || (len & (len - 1)) == 0),
                     "%s: band %d x %d (FFAB's transform takes lengths 2 .. 4096, at most 2048 when no power of two)", who, bh, bw);
    // (B h w >= 16 now: the batch statistics of training mode always have more than one value per channel)
    size_t sub = 0, fwd_ffab = 0, pk = 0;
    long long refused = 0;
    // a piece's answer joins the maximum; a limit of a piece that the checks above do not restate keeps its own message, under this
    // entry point's name
    const auto joins = [&](long long n) {
        if (n < 0) {
            const std::string why = rf_last_error();
            set_error("%s: %s", who, why.c_str());
            refused = n;
            return false;
        }
        sub = sub > (size_t)n ? sub : (size_t)n;
        return true;
    };
    if (!(joins(rf_ffab_scratch_bytes(B, C, bh, bw, &fwd_ffab)) && joins((long long)fwd_ffab) &&
          joins(rf_conv1x1_scratch_bytes(C, C, &pk)) && joins((long long)pk) &&
          joins(rf_wm_workspace_bytes(3 * B, C, bh, bw)) &&
          joins(rf_wfb_ffn_backward_workspace_bytes(B, C, hidden, h, w)) &&
          joins(rf_layernorm2d_backward_workspace_bytes(B, C, h, w)) &&
          joins(rf_ffab_backward_workspace_bytes(B, C, bh, bw)) &&
          joins(rf_illumination_estimator_backward_workspace_bytes(B, C, C, C, bh, bw, 0)) &&
          joins(rf_wm_backward_workspace_bytes(3 * B, C, bh, bw)) &&
          joins(rf_wmb_front_backward_workspace_bytes(B, C, bh, bw))))
        return (int)refused;
    Bump b;
    const size_t U = (size_t)B * C * h * w;
    p->tu = b.off(U); p->bands = b.off(U); p->bands2 = b.off(U);
    p->fea = b.off(U / 4); p->gfea = b.off(U / 4);
    p->va = b.off(U); p->vb = b.off(U); p->gu = b.off(U);
    p->ln2 = b.off((size_t)2 * C);
    p->wf = b.off((size_t)C * C);
    p->sub_bytes = align_up(sub, 256);
    p->sub = b.off(p->sub_bytes / sizeof(float));
    p->total = b.used;
    return RF_OK;
}

int run_wmb_backward(const WmbBwdPlan& p, const float* x, const float* go, float* dx, const float* const* prm, float* const* grd, float* ws, int B, int C,
                     int hidden, int h, int w, int training, float eps, int acc, hipStream_t st) {
    const int bh = h / 2, bw = w / 2;
    const size_t U4 = (size_t)B * C * bh * bw;
    float *tu = ws + p.tu, *bands = ws + p.bands, *bands2 = ws + p.bands2, *fea = ws + p.fea, *gfea = ws + p.gfea, *va = ws + p.va, *vb = ws + p.vb,
          *gu = ws + p.gu, *ln2 = ws + p.ln2, *wf = ws + p.wf;
    void* sub = ws + p.sub;
    const float *ln2_w = prm[kN2], *ln2_b = prm[kN2 + 1];
    const float* ffn[16];      // rf_wfb_ffn_backward's order: the 12 parameters, then the 4 buffers
    for (int i = 0; i < 16; ++i) ffn[i] = prm[i < 12 ? kFfn + i : kWmbPrm + i - 12];

    wmb_bwd_fold_kernel<<<grid1d((size_t)C * C), kBlk, 0, st>>>(prm[kN1], prm[kN1 + 1], prm[kIllu], ln2, wf, C);
    RF_TRY(check_launch("wmb_bwd_fold"));
    // 1-6: the forward, every value a later step reads kept
    RF_TRY(rf_wmb_front(x, tu, bands, ln2, ln2 + C, B, C, bh, bw, st));
    RF_TRY(rf_conv1x1(bands, nullptr, va, wf, prm[kIllu + 1], nullptr, nullptr, nullptr, sub, B, C, 0, C, bh, bw, st));      // x1, in va's first quarter
    RF_TRY(rf_dwconv5x5(va, fea, prm[kIllu + 2], prm[kIllu + 3], B, C, bh, bw, st));
    RF_TRY(rf_ffab(fea, bands2, prm + kFfab, sub, B, C, bh, bw, st));
    RF_TRY(rf_wm_forward(bands + U4, bands2 + U4, prm + kMb, sub, p.sub_bytes, 3 * B, C, bh, bw, st));
    RF_TRY(rf_wmb_back(bands2, tu, tu, B, C, bh, bw, st));
    RF_TRY(rf_layernorm2d(tu, va, ln2_w, ln2_b, 1e-5f, B, C, h, w, st));
    // 7-8: out = u + ffn(LN2(u))
    RF_TRY(rf_wfb_ffn_backward(va, go, vb, ffn, grd + kFfn, sub, p.sub_bytes, B, C, hidden, h, w, training, eps, acc, st));
    RF_TRY(rf_layernorm2d_backward(tu, vb, gu, ln2_w, grd[kN2], grd[kN2 + 1], go, sub, p.sub_bytes, B, C, h, w, 1e-5f, acc, st));
    // 9-12: the wavelet branch; grad_t = grad_u joins in step 13
    float *gb2 = va, *gb = vb;
    RF_TRY(rf_wmb_back_backward(bands2, gu, gb2, B, C, bh, bw, st));
    RF_TRY(rf_ffab_backward(fea, gb2, gfea, prm + kFfab, grd + kFfab, sub, p.sub_bytes, B, C, bh, bw, acc, st));
    if (!acc)      // illu.conv2 feeds illu_map alone, which WMB.forward discards: exact zeros, or what the caller accumulates into
        for (int i = 4; i < 6; ++i) RF_TRY(check_hip(hipMemsetAsync(grd[kIllu + i], 0, illu_prm_floats(i, C, C, C) * sizeof(float), st), "rf_wmb_backward: memset"));
    RF_TRY(rf_illumination_estimator_backward(bands, gfea, nullptr, gb, prm + kIllu, grd + kIllu, sub, p.sub_bytes, B, C, C, C, bh, bw, acc, st));
    RF_TRY(rf_wm_backward(bands + U4, gb2 + U4, gb + U4, prm + kMb, grd + kMb, sub, p.sub_bytes, 3 * B, C, bh, bw, acc, st));
    // 13: t = 2 LN1(x) - 1 runs on weight2 = 2 w, so d w = 2 d weight2
    return rf_wmb_front_backward(x, gu, dx, gb, ln2, grd[kN1], grd[kN1 + 1], sub, p.sub_bytes, B, C, bh, bw, 2.0f, acc, st);
}

}  // namespace
}  // namespace rf

using namespace rf;

extern "C" {

long long rf_wmb_backward_workspace_bytes(int B, int C, int hidden, int h, int w) {
    WmbBwdPlan p;
    const int rc = wmb_bwd_plan("rf_wmb_backward_workspace_bytes", B, C, hidden, h, w, &p);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_wmb_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                    size_t workspace_bytes, int B, int C, int hidden, int h, int w, int training, float eps, int accumulate, void* stream) {
    const char* who = "rf_wmb_backward";
    WmbBwdPlan p;
    RF_TRY(wmb_bwd_plan(who, B, C, hidden, h, w, &p));
    Span buffers[kWmbTensors - kWmbPrm];
    if (prm)
        for (int i = kWmbPrm; i < kWmbTensors; ++i) buffers[i - kWmbPrm] = {prm[i], (size_t)hidden * sizeof(float)};
    RF_TRY(check_backward_args({who, in, grad_out, grad_in, (size_t)B * C * h * w * sizeof(float), prm, grad_prm, kWmbPrm, workspace, workspace_bytes,
                                p.total * sizeof(float), buffers, kWmbTensors - kWmbPrm},
                               [=](int i) { return wmb_prm_floats(i, C, hidden); }));
    return run_wmb_backward(p, in, grad_out, grad_in, prm, grad_prm, (float*)workspace, B, C, hidden, h, w, training, eps, accumulate,
                            (hipStream_t)stream);
}

}  // extern "C"
