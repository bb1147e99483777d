// The per-pixel LayerNorm over channels as the element-wise kernels spell it: what their copies share.
//
//   walk form    a lane owns 4 consecutive pixels and walks the channels with 16-byte loads C planes apart (layernorm2d_kernel<4>,
//                wmb_front_kernel, wmb_ffn_tail_kernel): nothing per channel in registers, x read three times (HBM, L2, L2)
//   slice form   lane = (pixel group j, channel slice ks) of a wave, G = 64 / KS groups; a lane keeps channels ks, ks + KS, .. of its
//                pixels in registers and the sums over channels end in butterflies over the KS lanes of a group, o = G .. 32
//                (layernorm2d_reg_kernel, ln_bwd_reg_kernel, wmb_front_bwd_kernel): x read once.  Its loops stay in the three
//                kernels ("LayerNorm and Haar steps on shared pieces"); they share ln_rstd and the table below.
//
// Both are the exact two-pass statistics: the mean, then the centred second moment, then ln_rstd.  (ln_bwd_kernel of rf_train.hip
// divides by C where these multiply by invC and stays as it is; the MFMA tile layouts of the 1x1 GEMM prologues and of
// rf_fused_tile.h have their own steps.)
#pragma once
#include "rf_common.h"

namespace rf {

// the centred second moment summed over the C channels -> 1 / standard deviation
__device__ __forceinline__ float ln_rstd(float ssq, float invC, float eps) { return 1.0f / sqrtf(ssq * invC + eps); }

// ---- walk form: s and q are the running sums of one lane's 4 pixels.  Between the two passes s becomes the mean (s[v] *= invC),
// after the second q becomes ln_rstd(q[v]); m is the mean, or 0 where the bias-free form keeps it in the numerator
__device__ __forceinline__ void acc4(float (&s)[4], const float4& v) { s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w; }
__device__ __forceinline__ void sq4(float (&q)[4], const float4& v, const float (&m)[4]) {
    q[0] += (v.x - m[0]) * (v.x - m[0]); q[1] += (v.y - m[1]) * (v.y - m[1]);
    q[2] += (v.z - m[2]) * (v.z - m[2]); q[3] += (v.w - m[3]) * (v.w - m[3]);
}
__device__ __forceinline__ float4 norm4(const float4& v, const float (&m)[4], const float (&r)[4], float g, float b) {
    return make_float4((v.x - m[0]) * r[0] * g + b, (v.y - m[1]) * r[1] * g + b, (v.z - m[2]) * r[2] * g + b, (v.w - m[3]) * r[3] * g + b);
}

// ---- host: the channel counts the slice form of layernorm2d / ln_bwd serves, C = CPL * KS, as X(C, CPL, KS).  (wmb_front_bwd_kernel
// picks its KS by a rule of its own, front_ks of rf_wmb_bwd.hip.)
#define RF_LN_SLICE_TABLE(X) \
    X(16, 4, 4) X(32, 8, 4) X(48, 12, 4) X(64, 16, 4) X(96, 12, 8) X(128, 16, 8) X(192, 12, 16) X(256, 16, 16) X(384, 12, 32) X(512, 16, 32)
static inline bool ln_slice_channels(int C) {
#define RF_LN_CASE(C_, CPL, KS) case C_:
    switch (C) { RF_LN_SLICE_TABLE(RF_LN_CASE) return true; default: return false; }
#undef RF_LN_CASE
}
// workgroups per image: one per 4 * (64 / KS) groups of 4 pixels, at most about wg_per_cu per CU over the batch, grid-stride beyond
static inline int ln_slice_grid(int B, int P, int KS, int wg_per_cu) {
    const int gx = cdiv(P / 4, 4 * (64 / KS)), cap = cdiv(256 * wg_per_cu, B);
    return gx > cap ? cap : gx;
}

}  // namespace rf
