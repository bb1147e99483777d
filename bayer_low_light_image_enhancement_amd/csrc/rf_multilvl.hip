// Multi-level FLCA RawFormer (MultiLvlFrequencyawareLumaChromaAttentionRAWFormer.py): what the variant adds around the shared U-Net.
//   ml_guide_level   the 2 L + 2 guidance planes an FLCA_Pyramid block sees at its feature size (:143-145, :168-169):
//                    [y_low_0, y_high_0, .., y_low_{L-1}, y_high_{L-1}, cr, cb], bilinear, align_corners=False, and per-block sums
//                    of every y plane and of sqrt(cr^2 + cb^2 + 1e-8) for the pooled gates (:151-152, :171-172)
//   ml_means         those sums in fixed order -> the 2 L + 1 means of one (image, U-Net level)
//   ml_modulate      x * (alpha sigmoid(conv3(y_low_l)) + beta tanh(conv3(y_high_l)))  (:147-162) or, chroma form,
//                    x * (gamma sigmoid(conv3([cr, cb])))  (:170-173); the gate heads (2 -> 2 and 1 -> 1 affine maps of the means
//                    of THIS stage size, then a sigmoid, :153-156, :172) are evaluated in the kernel: they are per stage, the
//                    means per U-Net level
//   ml_step_fused    level 0 (C = dim <= 64): modulate -> 1x1 -> ReLU -> 1x1 -> 0.2 tanh + residual per pixel tile, both matrices in LDS
//   ml_residual      x + 0.2 tanh(r) for the composed steps that need no pooling sums
//   ml_tail_sums     per-block channel sums of the model output and of the packed input's [R, (G1 + G2) / 2, B]
//   ml_tail_delta    0.12 (in_mean - out_mean) per image and channel (:270-288; the mean of the x2 bilinear upsample equals the
//                    mean of the packed plane: every source pixel carries a total weight of 4)
//   ml_tail_apply    colour anchor + the luminance nudge towards the x8 bilinear upsample of LL2 (:403-414), one read and one
//                    write of the output
// Elsewhere (C > 64, widths that are no multiple of 4) a step is composed: ml_modulate, the shared GEMM kernels twice, ml_residual or,
// for a block's last step, tc_residual_kernel (rf_truecolor.hip), which leaves the pooling sums; the
// squeeze-excite gate is folded into channel_reduce by flca_se_fold (rf_flca.hip).  No float atomics: two forwards are bit-identical.
// The bilinear sampling, the Bayer read, the neighbourhood load and the gate heads are rf_guidance.h's, shared with the other variants.
#include "rf_guidance.h"

namespace rf {

namespace {

constexpr int kMlMeans = 8;          // floats per (level, image) in the means table: 2 L + 1 <= 7 used
constexpr int kMlGuideBlocks = 256;  // most workgroups per image of ml_guide_level_kernel (= partial sums per plane)
constexpr int kMlTailBlocks = 1024;  // most workgroups per image of ml_tail_sums_kernel

// sum over the 256 threads of a workgroup, the same order every time; valid in thread 0.  `red` holds 4 floats.
__device__ __forceinline__ float block_sum(float s, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();                       // the previous use of `red` is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct MlGuideSrc {
    const float* cr; const float* cb;    // [B][H][W]
    GuidePyramid pyr;                    // its first `levels` levels
};

// guide [B][2 L + 2][hf][wf]; partial [B][gridDim.x][kMlMeans]
__global__ void __launch_bounds__(256) ml_guide_level_kernel(MlGuideSrc s, float* __restrict__ guide, float* __restrict__ partial,
                                                             int H, int W, int hf, int wf) {
    const size_t b = blockIdx.y, hw = (size_t)H * W, pf = (size_t)hf * wf;
    const GuidePyramid& r = s.pyr;
    const int L = r.levels, NP = 2 * L + 2;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t p = blockIdx.x * 256ull + threadIdx.x; p < pf; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / wf), x = (int)(p % wf);
        float* o = guide + b * NP * pf + p;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < L) {
                const size_t off = b * (size_t)r.lh[i] * r.lw[i];
                const float lo = bilerp(r.ll[i] + off, r.lh[i], r.lw[i], hf, wf, y, x);
                const float hi = bilerp(r.mag[i] + off, r.lh[i], r.lw[i], hf, wf, y, x);
                o[(2 * i) * pf] = lo;
                o[(2 * i + 1) * pf] = hi;
                acc[2 * i] += lo;
                acc[2 * i + 1] += hi;
            }
        const float cr = bilerp(s.cr + b * hw, H, W, hf, wf, y, x), cb = bilerp(s.cb + b * hw, H, W, hf, wf, y, x);
        o[(2 * L) * pf] = cr;
        o[(2 * L + 1) * pf] = cb;
        acc[6] += sqrtf(cr * cr + cb * cb + 1e-8f);
    }
    __shared__ float red[4];
    float* out = partial + (b * gridDim.x + blockIdx.x) * kMlMeans;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float t = block_sum(acc[k], red);
        if (threadIdx.x == 0) out[k] = t;
    }
}

// means[b][k] = (sum over the nblk partials, in index order per lane and then over the lanes) / pf; k = 6: the chroma magnitude
__global__ void __launch_bounds__(64) ml_means_kernel(const float* __restrict__ partial, int nblk, float inv_pf, float* __restrict__ means) {
    const size_t b = blockIdx.x;
    for (int k = 0; k < 7; ++k) {
        float s = 0.f;
        for (int i = threadIdx.x; i < nblk; i += 64) s += partial[(b * nblk + i) * kMlMeans + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (threadIdx.x == 0) means[b * kMlMeans + k] = s * inv_pf;
    }
}

struct MlModArgs {
    const float* x; float* out;          // [B][C][P]
    const float* planes;                 // the two guidance planes of image 0 (adjacent); images are plane_bstride floats apart
    int64_t plane_bstride;
    const float* w_a; const float* w_b;  // level: low_attn[l] / high_attn[l] [C][1][3][3]; chroma: chroma_attn [C][2][3][3], w_b unused
    const float* means;                  // [B][kMlMeans] of this U-Net level
    const float* gate_w; const float* gate_b;   // level: freq_gate_head[l] [2][2], [2]; chroma: chroma_gate [1], [1]
    int level;                           // pyramid level (selects the means)
    int B, C, h, w;
};

// PX = pixels per thread along x (4: float4 feature traffic, needs w % 4 == 0; 1: any shape)
template <int PX, bool CHROMA>
__global__ void __launch_bounds__(256) ml_modulate_kernel(MlModArgs a) {
    constexpr int CG = 32;
    const size_t b = blockIdx.z;
    const int h = a.h, w = a.w, P = h * w, C = a.C;
    const int c_lo = blockIdx.y * CG, c_hi = (c_lo + CG < C) ? c_lo + CG : C;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    const bool live = p < P;
    const int y = live ? p / w : 0, x = live ? p - (p / w) * w : 0;
    float g0, g1 = 0.f;      // the gate heads of this stage (wave-uniform)
    ml_gate_heads<CHROMA>(a.means + b * kMlMeans, a.gate_w, a.gate_b, a.level, g0, g1);
    float nb[2][3][PX + 2];
    guide_nb<2, PX>(nb, a.planes + b * a.plane_bstride, P, y, x, h, w, live);
    const float* fb = a.x + b * (size_t)C * P + (live ? p : 0);
    float* ob = a.out + b * (size_t)C * P + p;
    for (int c = c_lo; c < c_hi; ++c) {
        const float* wa = CHROMA ? a.w_a + c * 18 : a.w_a + c * 9;
        const float* wb = CHROMA ? a.w_a + c * 18 + 9 : a.w_b + c * 9;
        float sa[PX], sb[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) { sa[q] = 0.f; sb[q] = 0.f; }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float ka = wa[dy * 3 + dx], kb = wb[dy * 3 + dx];
#pragma unroll
                for (int q = 0; q < PX; ++q) {
                    sa[q] = fmaf(ka, nb[0][dy][q + dx], sa[q]);
                    sb[q] = fmaf(kb, nb[1][dy][q + dx], sb[q]);
                }
            }
        if (live) {
            float fv[PX], v[PX];
            load_px<PX>(fb + (size_t)c * P, fv);
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                if constexpr (CHROMA) v[q] = fv[q] * (g0 * fast_sigmoid(sa[q] + sb[q]));
                else v[q] = fv[q] * (g0 * fast_sigmoid(sa[q]) + g1 * fast_tanh(sb[q]));
            }
            store_px<PX>(ob + (size_t)c * P, v);
        }
    }
}

// x + 0.2 tanh(r) without the pooling sums: the residual of every composed step but a block's last (that one is
// tc_residual_kernel, which also leaves the squeeze-excite partial sums).  out may be x.
template <int PX>
__global__ void __launch_bounds__(256) ml_residual_kernel(const float* x, const float* __restrict__ r, float* out, size_t n) {
    const size_t i = (blockIdx.x * 256ull + threadIdx.x) * PX;
    if (i >= n) return;
    if constexpr (PX == 4) {
        const float4 a = *reinterpret_cast<const float4*>(x + i), t = *reinterpret_cast<const float4*>(r + i);
        *reinterpret_cast<float4*>(out + i) = make_float4(a.x + 0.2f * fast_tanh(t.x), a.y + 0.2f * fast_tanh(t.y), a.z + 0.2f * fast_tanh(t.z), a.w + 0.2f * fast_tanh(t.w));
    } else {
        out[i] = x[i] + 0.2f * fast_tanh(r[i]);
    }
}

// One whole residual step at level 0 (C = dim <= 64):  out = x + 0.2 tanh(W2 relu(W0 (x * spatial) + b0) + b2)  per pixel tile,
// `spatial` as in ml_modulate_kernel.  Neither x * spatial, the hidden tensor nor raw_res reaches HBM: x is read once and out
// written once.  Both res_proj matrices, the 3x3 gate weights and the biases sit in LDS (C = 64: 39 KB).
//   A wave owns 16 consecutive pixels (MFMA column j = lane & 15).  The contraction index of BOTH GEMMs is ordered the way the
//   16x16x4 MFMA hands back its result -- k-set 4 t + r, lane group q = lane >> 4  <->  channel 16 t + 4 q + r -- so the ReLU
//   output of GEMM 1 is GEMM 2's B operand as it stands, and the x values a lane loaded for the modulation are the ones its
//   residual needs: no LDS transpose, no cross-lane move.  The weights are laid out to match when they are copied to LDS:
//   s_w[((4 t + r) * NT + to) * 64 + l] = W[16 to + (l & 15)][16 t + 4 (l >> 4) + r].
//   A workgroup owns 1024 consecutive pixels of one image (P % 64 == 0: whole groups of 16); with `partial` it leaves the sums
//   of `out` over them per channel in tc_residual_kernel's layout [B][gridDim.x][C], added in a fixed order.  out may be x: a
//   wave reads x only at the pixels it writes.
struct MlStepArgs {
    const float* x; float* out;          // [B][C][P]
    const float* planes; int64_t plane_bstride;
    const float* w_a; const float* w_b;  // as MlModArgs
    const float* means; const float* gate_w; const float* gate_b;
    int level;
    const float* w0; const float* b0; const float* w2; const float* b2;   // res_proj.0 / .2: [C][C], [C]
    float* partial;                      // or nullptr
    int h, w;
};

template <int C, bool CHROMA>
__global__ void __launch_bounds__(256) ml_step_fused_kernel(MlStepArgs a) {
    constexpr int NT = C / 16, KS = C / 4;
    __shared__ float s_w0[C * C], s_w2[C * C], s_ca[C * 9], s_cb[C * 9], s_b0[C], s_b2[C], s_red[4][C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, j = lane & 15;
    for (int i = tid; i < C * C; i += 256) {
        const int l = i & 63, tile = i >> 6, to = tile % NT, ks = tile / NT;
        const int co = 16 * to + (l & 15), k = 16 * (ks >> 2) + 4 * (l >> 4) + (ks & 3);
        s_w0[i] = a.w0[co * C + k];
        s_w2[i] = a.w2[co * C + k];
    }
    for (int i = tid; i < C * 9; i += 256) {
        const int c = i / 9, t = i - 9 * c;
        s_ca[i] = CHROMA ? a.w_a[c * 18 + t] : a.w_a[i];
        s_cb[i] = CHROMA ? a.w_a[c * 18 + 9 + t] : a.w_b[i];
    }
    for (int i = tid; i < C; i += 256) { s_b0[i] = a.b0[i]; s_b2[i] = a.b2[i]; }
    __syncthreads();
    const size_t b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    float g0, g1 = 0.f;
    ml_gate_heads<CHROMA>(a.means + b * kMlMeans, a.gate_w, a.gate_b, a.level, g0, g1);
    const float* gb = a.planes + b * a.plane_bstride;
    const float* xb = a.x + b * (size_t)C * P;
    float* ob = a.out + b * (size_t)C * P;
    const int p_lo = blockIdx.x * 1024, p_hi = p_lo + 1024 < P ? p_lo + 1024 : P;
    float csum[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) csum[ks] = 0.f;
    for (int p0 = p_lo + wave * 16; p0 < p_hi; p0 += 64) {
        const int p = p0 + j, y = p / w, x = p - y * w;
        float nb[2][3][3];
        guide_nb<2, 1>(nb, gb, P, y, x, h, w, true);
        float xv[KS];
        f32x4 acc[NT], acc2[NT];
#pragma unroll
        for (int to = 0; to < NT; ++to)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc[to][r] = s_b0[16 * to + 4 * q + r]; acc2[to][r] = s_b2[16 * to + 4 * q + r]; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c = 16 * (ks >> 2) + 4 * q + (ks & 3);
            xv[ks] = xb[(size_t)c * P + p];
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    sa = fmaf(s_ca[c * 9 + dy * 3 + dx], nb[0][dy][dx], sa);
                    sb = fmaf(s_cb[c * 9 + dy * 3 + dx], nb[1][dy][dx], sb);
                }
            const float m = CHROMA ? xv[ks] * (g0 * fast_sigmoid(sa + sb)) : xv[ks] * (g0 * fast_sigmoid(sa) + g1 * fast_tanh(sb));
#pragma unroll
            for (int to = 0; to < NT; ++to) acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w0[(ks * NT + to) * 64 + lane], m, acc[to], 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const float hid = fmaxf(acc[ks >> 2][ks & 3], 0.f);
#pragma unroll
            for (int to = 0; to < NT; ++to) acc2[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w2[(ks * NT + to) * 64 + lane], hid, acc2[to], 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c = 16 * (ks >> 2) + 4 * q + (ks & 3);
            const float v = xv[ks] + 0.2f * fast_tanh(acc2[ks >> 2][ks & 3]);
            ob[(size_t)c * P + p] = v;
            csum[ks] += v;
        }
    }
    if (a.partial) {      // kernel argument: uniform
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float s = csum[ks];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (j == 0) s_red[wave][16 * (ks >> 2) + 4 * q + (ks & 3)] = s;
        }
        __syncthreads();
        if (tid < C) a.partial[(b * gridDim.x + blockIdx.x) * C + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    }
}

// partial[(b * gridDim.x + blk) * 8 + k]: k = 0..2 sums of out[b][k] over the block's pixels, k = 3..5 sums of the packed
// input's R, (G1 + G2) / 2, B.  P4 = 4 H W output pixels per channel, a multiple of 4.
__global__ void __launch_bounds__(256) ml_tail_sums_kernel(const float* __restrict__ out, const float* __restrict__ in, int mosaic,
                                                           float* __restrict__ partial, int H, int W) {
    const size_t b = blockIdx.y, hw = (size_t)H * W, P4 = 4 * hw;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float4* oc = reinterpret_cast<const float4*>(out + (b * 3 + c) * P4);
        for (size_t q = blockIdx.x * 256ull + threadIdx.x; q < P4 / 4; q += (size_t)gridDim.x * 256) {
            const float4 v = oc[q];
            acc[c] += (v.x + v.y) + (v.z + v.w);
        }
    }
    for (size_t p = blockIdx.x * 256ull + threadIdx.x; p < hw; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p % W);
        acc[3] += packed_at(in, mosaic, 0, b, 0, y, x, H, W);
        acc[4] += 0.5f * (packed_at(in, mosaic, 0, b, 1, y, x, H, W) + packed_at(in, mosaic, 0, b, 2, y, x, H, W));
        acc[5] += packed_at(in, mosaic, 0, b, 3, y, x, H, W);
    }
    __shared__ float red[4];
    float* o = partial + (b * gridDim.x + blockIdx.x) * 8;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float t = block_sum(acc[k], red);
        if (threadIdx.x == 0) o[k] = t;
    }
}

// delta[b][c] = 0.12 (in_mean - out_mean)
__global__ void __launch_bounds__(64) ml_tail_delta_kernel(const float* __restrict__ partial, int nblk, float inv_p4, float inv_hw,
                                                           float* __restrict__ delta) {
    const size_t b = blockIdx.x;
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float s = 0.f;
        for (int i = threadIdx.x; i < nblk; i += 64) s += partial[(b * nblk + i) * 8 + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        m[k] = s;
    }
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const float in_mean = (c == 0 ? m[3] : c == 1 ? m[4] : m[5]) * inv_hw, out_mean = (c == 0 ? m[0] : c == 1 ? m[1] : m[2]) * inv_p4;
        delta[b * 4 + c] = 0.12f * (in_mean - out_mean);
    }
}

// out[b][c] += delta[b][c], then += 0.03 (bilinear_up(LL2) - luma(out)) on all three channels.  ll2 [B][h2][w2], out [B][3][Ho][Wo]
// with Wo % 4 == 0; a thread owns 4 consecutive pixels of a row.
__global__ void __launch_bounds__(256) ml_tail_apply_kernel(float* __restrict__ out, const float* __restrict__ delta, const float* __restrict__ ll2,
                                                            int h2, int w2, int Ho, int Wo) {
    const size_t b = blockIdx.y, P4 = (size_t)Ho * Wo;
    const float d0 = delta[b * 4], d1 = delta[b * 4 + 1], d2 = delta[b * 4 + 2];
    const float* l2 = ll2 + b * (size_t)h2 * w2;
    float* ob = out + b * 3 * P4;
    for (size_t q = blockIdx.x * 256ull + threadIdx.x; q < P4 / 4; q += (size_t)gridDim.x * 256) {
        const size_t p = q * 4;
        const int y = (int)(p / Wo), x = (int)(p % Wo);
        const float4 r4 = *reinterpret_cast<const float4*>(ob + p), g4 = *reinterpret_cast<const float4*>(ob + P4 + p),
                     b4 = *reinterpret_cast<const float4*>(ob + 2 * P4 + p);
        float r[4] = {r4.x, r4.y, r4.z, r4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w}, bl[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r[i] += d0; g[i] += d1; bl[i] += d2;
            const float oy = (0.299f * r[i] + 0.587f * g[i]) + 0.114f * bl[i];
            const float n = (bilerp(l2, h2, w2, Ho, Wo, y, x + i) - oy) * 0.03f;
            r[i] += n; g[i] += n; bl[i] += n;
        }
        *reinterpret_cast<float4*>(ob + p) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(ob + P4 + p) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(ob + 2 * P4 + p) = make_float4(bl[0], bl[1], bl[2], bl[3]);
    }
}

int pyr_levels(int levels) { return levels > 2 ? levels : 2; }   // the model-level anchor is the 2-level LL whatever flca_levels is

struct MlBufs {
    float* base;                 // guidance_base's planes (rf_flca.hip)
    float *y, *cr, *cb;
    GuidePyramid pyr;            // pyr_levels(levels) levels; level 0 is guidance_base's
    float* means;               // [4 U-Net levels][B][kMlMeans]
    float* gpart;                // [B][kMlGuideBlocks][kMlMeans]
    float* tpart;                // [B][kMlTailBlocks][8]
    float* delta;                // [B][4]
    size_t used;
};

MlBufs ml_layout(float* s, int B, int H, int W, int levels) {
    MlBufs f{};
    Bump b{s};
    f.base = b.take(guidance_scratch_floats(B, H, W));
    if (s) guidance_planes(f.base, B, H, W, &f.y, &f.cr, &f.cb, &f.pyr.ll[0], &f.pyr.mag[0]);
    f.pyr.lh[0] = H / 2; f.pyr.lw[0] = W / 2;
    pyramid_layout(f.pyr, b, B, H / 2, W / 2, 1, pyr_levels(levels));
    f.means = b.take((size_t)4 * B * kMlMeans);
    f.gpart = b.take((size_t)B * kMlGuideBlocks * kMlMeans);
    f.tpart = b.take((size_t)B * kMlTailBlocks * 8);
    f.delta = b.take((size_t)B * 4);
    f.used = b.used;
    return f;
}

}  // namespace

size_t ml_scratch_floats(int B, int H, int W, int levels) { return ml_layout(nullptr, B, H, W, levels).used; }

// y, cr, cb and the Haar pyramid of y (levels 1 .. max(levels, 2))
int launch_ml_guidance(const float* in, int mosaic, float* scratch, int B, int H, int W, int levels, hipStream_t st) {
    RF_CHECK_ARG(levels >= 1 && levels <= 3 && H % 8 == 0 && W % 8 == 0 && B <= 65535, "multilvl guidance: levels=%d H=%d W=%d unsupported", levels, H, W);
    const MlBufs f = ml_layout(scratch, B, H, W, levels);
    RF_TRY(launch_guidance_base(in, mosaic, 0, f.base, B, H, W, st));
    const GuidePyramid& r = f.pyr;
    for (int i = 1; i < r.levels; ++i)
        RF_TRY(launch_tc_pyramid(r.ll[i - 1], r.ll[i], r.mag[i], B, r.lh[i - 1], r.lw[i - 1], st));
    return RF_OK;
}

// the guidance planes of U-Net level `lvl` (size hf x wf) and their means
int launch_ml_guide_level(float* scratch, float* guide, int lvl, int B, int H, int W, int levels, int hf, int wf, hipStream_t st) {
    RF_CHECK_ARG(lvl >= 0 && lvl < 4, "multilvl guidance: level %d", lvl);
    const MlBufs f = ml_layout(scratch, B, H, W, levels);
    MlGuideSrc s{};
    s.cr = f.cr; s.cb = f.cb; s.pyr = f.pyr; s.pyr.levels = levels;
    int nblk = cdiv(hf * wf, 256);
    if (nblk > kMlGuideBlocks) nblk = kMlGuideBlocks;
    ProfScope prof(st, "ml_guide_level_kernel", 0.0, 4.0 * B * hf * wf * (2 * levels + 2) * 2);
    ml_guide_level_kernel<<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(s, guide, f.gpart, H, W, hf, wf);
    ml_means_kernel<<<B, 64, 0, st>>>(f.gpart, nblk, 1.0f / (float)((size_t)hf * wf), f.means + (size_t)lvl * B * kMlMeans);
    return check_launch("ml_guide_level");
}

const float* ml_level_means(const float* scratch, int lvl, int B, int H, int W, int levels) {
    return ml_layout(const_cast<float*>(scratch), B, H, W, levels).means + (size_t)lvl * B * kMlMeans;
}

// step = pyramid level 0 .. levels - 1, or levels: the chroma form.  guide [B][2 levels + 2][h][w]; w_a / w_b / gate_w / gate_b: the
// step's weights (chroma: chroma_attn, nullptr, chroma_gate weight and bias)
int launch_ml_modulate(const float* x, float* out, const float* guide, const float* means, int step, int levels, const float* w_a,
                       const float* w_b, const float* gate_w, const float* gate_b, int B, int C, int h, int w, hipStream_t st) {
    RF_CHECK_ARG(C <= 512 && B <= 65535 && step >= 0 && step <= levels && levels <= 3, "multilvl flca: C=%d step=%d unsupported", C, step);
    const size_t P = (size_t)h * w;
    MlModArgs a{};
    a.x = x; a.out = out; a.planes = guide + (size_t)2 * step * P; a.plane_bstride = (int64_t)(2 * levels + 2) * P;
    a.w_a = w_a; a.w_b = w_b; a.means = means; a.gate_w = gate_w; a.gate_b = gate_b; a.level = step;
    a.B = B; a.C = C; a.h = h; a.w = w;
    const bool chroma = step == levels;
    const double el = (double)B * C * P;
    ProfScope prof(st, "ml_modulate_kernel", 50.0 * el, 8.0 * el);
    const bool vec = (w % 4 == 0) && aligned16(x) && aligned16(out);
    const dim3 gv((unsigned)cdiv(h * w, 1024), (unsigned)cdiv(C, 32), (unsigned)B), gs((unsigned)cdiv(h * w, 256), (unsigned)cdiv(C, 32), (unsigned)B);
    if (vec && chroma) ml_modulate_kernel<4, true><<<gv, 256, 0, st>>>(a);
    else if (vec) ml_modulate_kernel<4, false><<<gv, 256, 0, st>>>(a);
    else if (chroma) ml_modulate_kernel<1, true><<<gs, 256, 0, st>>>(a);
    else ml_modulate_kernel<1, false><<<gs, 256, 0, st>>>(a);
    return check_launch("ml_modulate");
}

// x + 0.2 tanh(r), no pooling sums (the composed path's steps before a block's last); out may be x
int launch_ml_residual(const float* x, const float* r, float* out, int B, int C, int h, int w, hipStream_t st) {
    const size_t n = (size_t)B * C * h * w;
    ProfScope prof(st, "ml_residual_kernel", 8.0 * n, 12.0 * n);
    const bool vec = n % 4 == 0 && aligned16(x) && aligned16(r) && aligned16(out);
    if (vec) ml_residual_kernel<4><<<(unsigned)((n / 4 + 255) / 256), 256, 0, st>>>(x, r, out, n);
    else ml_residual_kernel<1><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, r, out, n);
    return check_launch("ml_residual");
}

// the fused step exists for C = 16 / 32 / 48 / 64, widths that are multiples of 4 and whole groups of 16 pixels per wave
bool ml_step_fused_supported(int C, int h, int w) { return C % 16 == 0 && C <= 64 && w % 4 == 0 && (h * w) % 64 == 0; }

// one whole residual step (launch_ml_modulate's arguments + res_proj's raw weights); partial: [B][tc_nblk(h, w)][C] or nullptr
int launch_ml_step_fused(const float* x, float* out, const float* guide, const float* means, int step, int levels, const float* w_a,
                         const float* w_b, const float* gate_w, const float* gate_b, const float* w0, const float* b0, const float* w2,
                         const float* b2, float* partial, int B, int C, int h, int w, hipStream_t st) {
    RF_CHECK_ARG(ml_step_fused_supported(C, h, w) && B <= 65535 && step >= 0 && step <= levels && levels <= 3,
                 "multilvl fused step: C=%d %dx%d step=%d unsupported", C, h, w, step);
    const size_t P = (size_t)h * w;
    MlStepArgs a{};
    a.x = x; a.out = out; a.planes = guide + (size_t)2 * step * P; a.plane_bstride = (int64_t)(2 * levels + 2) * P;
    a.w_a = w_a; a.w_b = w_b; a.means = means; a.gate_w = gate_w; a.gate_b = gate_b; a.level = step;
    a.w0 = w0; a.b0 = b0; a.w2 = w2; a.b2 = b2; a.partial = partial; a.h = h; a.w = w;
    const bool chroma = step == levels;
    const double el = (double)B * C * P;
    ProfScope prof(st, "ml_step_fused_kernel", (4.0 * C + 60.0) * el, 8.0 * el);
    const dim3 grid((unsigned)cdiv(h * w, 1024), (unsigned)B);
#define RF_ML_STEP(CC)                                                              \
    if (C == CC) {                                                                  \
        if (chroma) ml_step_fused_kernel<CC, true><<<grid, 256, 0, st>>>(a);        \
        else ml_step_fused_kernel<CC, false><<<grid, 256, 0, st>>>(a);              \
    }
    RF_ML_STEP(16) RF_ML_STEP(32) RF_ML_STEP(48) RF_ML_STEP(64)
#undef RF_ML_STEP
    return check_launch("ml_step_fused");
}

// out [B][3][2H][2W] (conv_out + LeakyReLU + PixelShuffle already applied) -> colour anchor + luminance nudge, in place
int launch_ml_tail(float* out, const float* in, int mosaic, float* scratch, int B, int H, int W, int levels, hipStream_t st) {
    RF_CHECK_ARG(aligned16(out) && W % 4 == 0 && B <= 65535, "multilvl tail: B=%d W=%d unsupported or the output is not 16-byte aligned", B, W);
    const MlBufs f = ml_layout(scratch, B, H, W, levels);
    const size_t hw = (size_t)H * W, P4 = 4 * hw;
    int nblk = (int)((P4 / 4 + 255) / 256 < (size_t)kMlTailBlocks ? (P4 / 4 + 255) / 256 : (size_t)kMlTailBlocks);
    {
        ProfScope prof(st, "ml_tail_sums_kernel", 0.0, 4.0 * B * (3.0 * P4 + 4.0 * hw));
        ml_tail_sums_kernel<<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(out, in, mosaic, f.tpart, H, W);
        ml_tail_delta_kernel<<<B, 64, 0, st>>>(f.tpart, nblk, 1.0f / (float)P4, 1.0f / (float)hw, f.delta);
    }
    ProfScope prof(st, "ml_tail_apply_kernel", 0.0, 4.0 * B * 6.0 * P4);
    int gx = (int)((P4 / 4 + 255) / 256);
    if (gx > 4096) gx = 4096;
    ml_tail_apply_kernel<<<dim3((unsigned)gx, (unsigned)B), 256, 0, st>>>(out, f.delta, f.pyr.ll[1], f.pyr.lh[1], f.pyr.lw[1], 2 * H, 2 * W);
    return check_launch("ml_tail");
}

}  // namespace rf

using namespace rf;

// ---- the kernels one by one (include/rawformer_hip.h): argument checks, then the launch functions above ----------------------
namespace {

// what the modulation and the fused step index with int: B and the channel groups in the grid, h * w pixels
int ml_check_step(const char* who, int B, int C, int h, int w, int step, int levels) {
    RF_TRY(check_gate_shape(who, B, C, h, w));
    RF_CHECK_ARG(levels >= 1 && levels <= 3, "%s: levels=%d (1..3)", who, levels);
    RF_CHECK_ARG(step >= 0 && step <= levels, "%s: step=%d (0..levels-1: a pyramid level; levels = %d: the chroma form)", who, step, levels);
    return RF_OK;
}

}  // namespace

extern "C" {

int rf_ml_modulate(const float* x, const float* guide, const float* means, int step, int levels, const float* w_a, const float* w_b,
                   const float* gate_w, const float* gate_b, float* out, int B, int C, int h, int w, void* stream) {
    RF_TRY(ml_check_step("rf_ml_modulate", B, C, h, w, step, levels));
    RF_CHECK_ARG(x && guide && means && w_a && (w_b || step == levels) && gate_w && gate_b && out, "rf_ml_modulate: null argument");
    RF_CHECK_ARG(aligned4(x) && aligned4(guide) && aligned4(means) && aligned4(w_a) && aligned4(w_b) && aligned4(gate_w) &&
                     aligned4(gate_b) && aligned4(out), "rf_ml_modulate: buffers must be 4-byte aligned");
    return launch_ml_modulate(x, out, guide, means, step, levels, w_a, w_b, gate_w, gate_b, B, C, h, w, (hipStream_t)stream);
}

int rf_ml_step_fused(const float* x, const float* guide, const float* means, int step, int levels, const float* w_a, const float* w_b,
                     const float* gate_w, const float* gate_b, const float* w0, const float* b0, const float* w2, const float* b2,
                     float* out, float* partial, int B, int C, int h, int w, void* stream) {
    RF_TRY(ml_check_step("rf_ml_step_fused", B, C, h, w, step, levels));
    RF_CHECK_ARG(ml_step_fused_supported(C, h, w),
                 "rf_ml_step_fused: C=%d at %dx%d: the fused step needs C = 16, 32, 48 or 64, w %% 4 == 0 and h * w %% 64 == 0", C, h, w);
    RF_CHECK_ARG(x && guide && means && w_a && (w_b || step == levels) && gate_w && gate_b && w0 && b0 && w2 && b2 && out,
                 "rf_ml_step_fused: null argument");
    for (const void* p : {(const void*)x, (const void*)guide, (const void*)means, (const void*)w_a, (const void*)w_b, (const void*)gate_w,
                          (const void*)gate_b, (const void*)w0, (const void*)b0, (const void*)w2, (const void*)b2, (const void*)out,
                          (const void*)partial})
        RF_CHECK_ARG(aligned4(p), "rf_ml_step_fused: buffers must be 4-byte aligned");
    return launch_ml_step_fused(x, out, guide, means, step, levels, w_a, w_b, gate_w, gate_b, w0, b0, w2, b2, partial, B, C, h, w,
                                (hipStream_t)stream);
}

int rf_ml_residual(const float* x, const float* r, float* out, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(x && r && out, "rf_ml_residual: null argument");
    RF_CHECK_ARG(B >= 1 && C >= 1 && h >= 1 && w >= 1, "rf_ml_residual: B=%d C=%d h=%d w=%d: every size must be positive", B, C, h, w);
    RF_CHECK_ARG((double)B * C * h * w <= (double)((size_t)1 << 38), "rf_ml_residual: B=%d C=%d h=%d w=%d exceeds 2^38 elements", B, C, h, w);
    RF_CHECK_ARG(aligned4(x) && aligned4(r) && aligned4(out), "rf_ml_residual: buffers must be 4-byte aligned");
    return launch_ml_residual(x, r, out, B, C, h, w, (hipStream_t)stream);
}

}  // extern "C"
