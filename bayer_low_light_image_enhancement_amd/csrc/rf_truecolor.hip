// TrueColorRawFormer-specific kernels (BayerTORGBColorMultiLvl.py): everything the variant adds around the shared U-Net.
//   tc_front        EnhancedBayerProcessor up to the small convolutions (:100-125): softplus white balance, 3x3 colour
//                   matrix + bias, BT.709 luma and its per-image maximum; writes the inputs of the two conv chains
//   tc_normalise    y / max(amax, eps) (:124), Haar pyramid of y (EnhancedFLCA._pyramid_y, :236-247: LL and high-band
//                   magnitude of every level)
//   tc_guide_level  the seven guidance planes an EnhancedFLCA block sees at its feature size (:255-275):
//                   [y, cr, cb, R, G, y_low (deepest LL), y_high (mean of the resized magnitudes)], bilinear, align_corners=False
//   tc_spatial      feat * (1 + sigmoid(conv3x3(5 planes)) + tanh(sigmoid(conv3x3(y_low)) + tanh(conv3x3(y_high))))   (:277-283)
//   tc_residual     x + 0.2 tanh(res_proj(x)) and the per-block channel sums for the squeeze-excite pooling (:285-292); the
//                   two 1x1 convolutions of res_proj are the GEMM kernels of rf_gemm1x1.hip
//   tc_color_head   CameraAwareColorCorrection (:160-176) per pixel: clamp, pow(1/gamma), 3->64->3 MLP, per-channel tone curve
// All HBM-bound or VALU-bound element-wise work; the dense parts of the variant run on the shared conv / GEMM kernels.  The Bayer
// read, the bilinear sampling, the Haar step, the luma maximum and the steps of the gate kernel are rf_guidance.h's.
#include "rf_guidance.h"

namespace rf {

namespace {

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
// cin4 [B,4,H,W] = (r, g, b, y_raw) after white balance; lin3 [B,3,H,W] = colour matrix output
__global__ void __launch_bounds__(256) tc_front_kernel(const float* __restrict__ in, int mosaic, const float* __restrict__ wb_gains,
                                                       const float* __restrict__ cm, float* __restrict__ cin4, float* __restrict__ lin3,
                                                       int* __restrict__ amax, int H, int W) {
    const size_t b = blockIdx.y, hw = (size_t)H * W;
    float gn[4], m[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) gn[i] = softplus_f(wb_gains[i]) + 1e-6f;
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = cm[i];
    float mx = -INFINITY;
    for (size_t p = blockIdx.x * 256ull + threadIdx.x; p < hw; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p % W);
        const float r = packed_at(in, mosaic, 0, b, 0, y, x, H, W) * gn[0];
        const float g = 0.5f * (packed_at(in, mosaic, 0, b, 1, y, x, H, W) * gn[1] + packed_at(in, mosaic, 0, b, 2, y, x, H, W) * gn[2]);
        const float bl = packed_at(in, mosaic, 0, b, 3, y, x, H, W) * gn[3];
        float l[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) l[o] = ((r * m[4 * o] + g * m[4 * o + 1]) + bl * m[4 * o + 2]) + m[4 * o + 3];
        const float yr = (l[0] * 0.2126f + l[1] * 0.7152f) + l[2] * 0.0722f;
        float* c4 = cin4 + b * 4 * hw + p;
        c4[0] = r; c4[hw] = g; c4[2 * hw] = bl; c4[3 * hw] = yr;
        float* l3 = lin3 + b * 3 * hw + p;
        l3[0] = l[0]; l3[hw] = l[1]; l3[2 * hw] = l[2];
        mx = fmaxf(mx, yr);
    }
    block_max_atomic(mx, amax + b);
}

// y = y_raw / max(amax, eps) written back into plane 3 of cin4; first pyramid level (LL1, mag1) from 2x2 blocks of y.
// One thread per 2x2 block (H, W even: packed sizes are multiples of 8).
__global__ void __launch_bounds__(256) tc_normalise_kernel(float* __restrict__ cin4, const int* __restrict__ amax, float* __restrict__ ll1,
                                                           float* __restrict__ mag1, int H, int W) {
    const size_t b = blockIdx.y, hw = (size_t)H * W;
    const int H2 = H / 2, W2 = W / 2;
    const float inv = 1.0f / fmaxf(__int_as_float(amax[b]), 1e-6f);
    float* yp = cin4 + (b * 4 + 3) * hw;
    for (size_t q = blockIdx.x * 256ull + threadIdx.x; q < (size_t)H2 * W2; q += (size_t)gridDim.x * 256) {
        const int y2 = (int)(q / W2), x2 = (int)(q % W2);
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const size_t p = (size_t)(2 * y2 + (t >> 1)) * W + 2 * x2 + (t & 1);
            v[t] = yp[p] * inv;
            yp[p] = v[t];
        }
        haar_ll_mag(v, ll1[b * (size_t)H2 * W2 + q], mag1[b * (size_t)H2 * W2 + q]);
    }
}

// deeper pyramid levels: HaarDWT of the previous LL (reflect padding when a side is odd: HaarDWT.forward, :54-58)
__global__ void __launch_bounds__(256) tc_pyramid_kernel(const float* __restrict__ src, float* __restrict__ ll, float* __restrict__ mag, int hs, int ws) {
    const size_t b = blockIdx.y;
    const int h2 = (hs + 1) / 2, w2 = (ws + 1) / 2;
    const float* s = src + b * (size_t)hs * ws;
    for (size_t q = blockIdx.x * 256ull + threadIdx.x; q < (size_t)h2 * w2; q += (size_t)gridDim.x * 256) {
        const int y2 = (int)(q / w2), x2 = (int)(q % w2);
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int y = 2 * y2 + (t >> 1), x = 2 * x2 + (t & 1);
            if (y >= hs) y = hs - 2;            // reflect (no edge repeat): index hs -> hs - 2
            if (x >= ws) x = ws - 2;
            v[t] = s[(size_t)(y < 0 ? 0 : y) * ws + (x < 0 ? 0 : x)];
        }
        haar_ll_mag(v, ll[b * (size_t)h2 * w2 + q], mag[b * (size_t)h2 * w2 + q]);
    }
}

struct TcGuideSrc {
    const float* y;        // plane 3 of cin4, image stride 4 * H * W
    const float* crcb;     // [B,2,H,W]
    const float* rgb;      // refined rgb [B,3,H,W]
    GuidePyramid pyr;
};

__global__ void __launch_bounds__(256) tc_guide_level_kernel(TcGuideSrc s, float* __restrict__ guide, int H, int W, int hf, int wf) {
    const size_t b = blockIdx.y, hw = (size_t)H * W, pf = (size_t)hf * wf;
    for (size_t p = blockIdx.x * 256ull + threadIdx.x; p < pf; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / wf), x = (int)(p % wf);
        float* o = guide + b * 7 * pf + p;
        o[0] = bilerp(s.y + b * 4 * hw, H, W, hf, wf, y, x);
        o[pf] = bilerp(s.crcb + b * 2 * hw, H, W, hf, wf, y, x);
        o[2 * pf] = bilerp(s.crcb + (b * 2 + 1) * hw, H, W, hf, wf, y, x);
        o[3 * pf] = bilerp(s.rgb + b * 3 * hw, H, W, hf, wf, y, x);
        o[4 * pf] = bilerp(s.rgb + (b * 3 + 1) * hw, H, W, hf, wf, y, x);
        const GuidePyramid& r = s.pyr;
        const int L = r.levels - 1;
        o[5 * pf] = bilerp(r.ll[L] + b * (size_t)r.lh[L] * r.lw[L], r.lh[L], r.lw[L], hf, wf, y, x);
        float hsum = 0.f;
        for (int i = 0; i < r.levels; ++i) hsum += bilerp(r.mag[i] + b * (size_t)r.lh[i] * r.lw[i], r.lh[i], r.lw[i], hf, wf, y, x);
        o[6 * pf] = r.levels > 1 ? hsum / (float)r.levels : hsum;
    }
}

// Spatial gate.  PX = pixels per thread along x (4: float4 feature traffic, needs w % 4 == 0; 1: any shape).
struct TcSpatialArgs {
    const float* feat; float* xs; const float* guide;         // [B,C,P], [B,C,P], [B,7,P]
    const float* w_col; const float* b_col;                   // [C,5,3,3], [C]
    const float* w_low; const float* b_low; const float* w_high; const float* b_high;   // [C,1,3,3], [C]
    int B, C, h, w;
};

template <int PX>
__global__ void __launch_bounds__(256) tc_spatial_kernel(TcSpatialArgs a) {
    constexpr int CG = 32;
    const size_t b = blockIdx.z;
    const int h = a.h, w = a.w, P = h * w, C = a.C;
    const int c_lo = blockIdx.y * CG, c_hi = (c_lo + CG < C) ? c_lo + CG : C;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    const bool live = p < P;
    const int y = live ? p / w : 0, x = live ? p - (p / w) * w : 0;
    float nb[7][3][PX + 2];
    const float* gb = a.guide + b * 7 * (size_t)P;      // guide_nb<7, PX> written out: as the helper it ran slower at level 1
#pragma unroll
    for (int pl = 0; pl < 7; ++pl)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < PX + 2; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                const bool ok = live && yy >= 0 && yy < h && xx >= 0 && xx < w;
                nb[pl][dy][dx] = ok ? gb[(size_t)pl * P + (size_t)yy * w + xx] : 0.f;
            }
    const float* fb = a.feat + b * (size_t)C * P + (live ? p : 0);
    float* xb = a.xs + b * (size_t)C * P + p;
    for (int c = c_lo; c < c_hi; ++c) {
        const float* wc = a.w_col + c * 45;
        const float* wl = a.w_low + c * 9;
        const float* wh = a.w_high + c * 9;
        float sc[PX], sl[PX], sh[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) { sc[q] = a.b_col[c]; sl[q] = a.b_low[c]; sh[q] = a.b_high[c]; }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int t = dy * 3 + dx;
                const float k0 = wc[t], k1 = wc[9 + t], k2 = wc[18 + t], k3 = wc[27 + t], k4 = wc[36 + t], kl = wl[t], kh = wh[t];
#pragma unroll
                for (int q = 0; q < PX; ++q) {
                    sc[q] = fmaf(k4, nb[4][dy][q + dx], fmaf(k3, nb[3][dy][q + dx], fmaf(k2, nb[2][dy][q + dx],
                            fmaf(k1, nb[1][dy][q + dx], fmaf(k0, nb[0][dy][q + dx], sc[q])))));
                    sl[q] = fmaf(kl, nb[5][dy][q + dx], sl[q]);
                    sh[q] = fmaf(kh, nb[6][dy][q + dx], sh[q]);
                }
            }
        if (live) {
            float fv[PX], v[PX];
            load_px<PX>(fb + (size_t)c * P, fv);
#pragma unroll
            for (int q = 0; q < PX; ++q) v[q] = fv[q] * (1.0f + fast_sigmoid(sc[q]) + fast_tanh(fast_sigmoid(sl[q]) + fast_tanh(sh[q])));
            store_px<PX>(xb + (size_t)c * P, v);
        }
    }
}

// x2 = xs + 0.2 tanh(r); partial[(b * nblk + blk) * C + c] = sum over the block's pixels of x2 (fixed-order: no atomics)
template <int PX>
__global__ void __launch_bounds__(256) tc_residual_kernel(const float* __restrict__ xs, const float* __restrict__ r, float* __restrict__ x2,
                                                          float* __restrict__ partial, int nblk, int C, int P) {
    const int blk = blockIdx.x;
    const size_t b = blockIdx.y;
    const int p = (blk * 256 + threadIdx.x) * PX;
    const bool live = p < P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ float red[512][4];
    const size_t base = b * (size_t)C * P + (live ? p : 0);
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        if (live) {
            if constexpr (PX == 4) {
                const float4 a = *reinterpret_cast<const float4*>(xs + base + (size_t)c * P);
                const float4 t = *reinterpret_cast<const float4*>(r + base + (size_t)c * P);
                const float4 v = make_float4(a.x + 0.2f * fast_tanh(t.x), a.y + 0.2f * fast_tanh(t.y), a.z + 0.2f * fast_tanh(t.z), a.w + 0.2f * fast_tanh(t.w));
                *reinterpret_cast<float4*>(x2 + base + (size_t)c * P) = v;
                s = (v.x + v.y) + (v.z + v.w);
            } else {
                const float v = xs[base + (size_t)c * P] + 0.2f * fast_tanh(r[base + (size_t)c * P]);
                x2[base + (size_t)c * P] = v;
                s = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) red[c][wave] = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        partial[(b * nblk + blk) * C + c] = (red[c][0] + red[c][1]) + (red[c][2] + red[c][3]);
}

// refined = lin + d (demosaic_refine residual, :131)
__global__ void __launch_bounds__(256) tc_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = a[i] + b[i];
}

// CameraAwareColorCorrection in place on [B,3,P]
__global__ void __launch_bounds__(256) tc_color_head_kernel(float* __restrict__ x, const float* __restrict__ gamma_param,
                                                            const float* __restrict__ w0, const float* __restrict__ b0,   // [64,3], [64]
                                                            const float* __restrict__ w2, const float* __restrict__ b2,   // [3,64], [3]
                                                            const float* __restrict__ t0w, const float* __restrict__ t0b, // [32], [32]
                                                            const float* __restrict__ t2w, const float* __restrict__ t2b, // [32], [1]
                                                            size_t P) {
    __shared__ float s_w0[192], s_b0[64], s_w2[192], s_t0w[32], s_t0b[32], s_t2w[32];
    for (int i = threadIdx.x; i < 192; i += 256) { s_w0[i] = w0[i]; s_w2[i] = w2[i]; }
    for (int i = threadIdx.x; i < 64; i += 256) s_b0[i] = b0[i];
    for (int i = threadIdx.x; i < 32; i += 256) { s_t0w[i] = t0w[i]; s_t0b[i] = t0b[i]; s_t2w[i] = t2w[i]; }
    __syncthreads();
    const float inv_gamma = 1.0f / (softplus_f(*gamma_param) + 1e-6f);
    const float bb[3] = {b2[0], b2[1], b2[2]}, tb = t2b[0];
    const size_t b = blockIdx.y;
    float* xb = x + b * 3 * P;
    for (size_t p = blockIdx.x * 256ull + threadIdx.x; p < P; p += (size_t)gridDim.x * 256) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = powf(fminf(fmaxf(xb[c * P + p], 0.f), 1.f), inv_gamma);
        float o[3] = {bb[0], bb[1], bb[2]};
        for (int m = 0; m < 64; ++m) {
            const float hid = fmaxf(fmaf(s_w0[3 * m + 2], v[2], fmaf(s_w0[3 * m + 1], v[1], fmaf(s_w0[3 * m], v[0], s_b0[m]))), 0.f);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(s_w2[64 * c + m], hid, o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = tb;
            for (int m = 0; m < 32; ++m) t = fmaf(s_t2w[m], fmaxf(fmaf(s_t0w[m], o[c], s_t0b[m]), 0.f), t);
            const float mod = 1.0f / (1.0f + expf(-t));
            xb[c * P + p] = fminf(fmaxf(o[c] * (0.8f + 0.4f * mod), 0.f), 1.f);
        }
    }
}

}  // namespace

// scratch of the front end (floats): cin4 4hw | lin3 3hw | t16 16hw | crcb 2hw | t32 32hw | d3 3hw | rgb 3hw | pyramid | amax
size_t tc_front_scratch_floats(int B, int H, int W, int levels) {
    const size_t hw = (size_t)H * W;
    GuidePyramid pyr{};
    Bump none;
    return (size_t)B * (4 + 3 + 16 + 2 + 32 + 3 + 3) * hw + pyramid_layout(pyr, none, B, H, W, 0, levels) + align_up((size_t)B, 64) + 64 * 16;
}

struct TcFrontBufs { float *cin4, *lin3, *t16, *crcb, *t32, *d3, *rgb; GuidePyramid pyr; int* amax; };

static TcFrontBufs tc_front_layout(float* s, int B, int H, int W, int levels) {
    const size_t hw = (size_t)H * W;
    TcFrontBufs f{};
    Bump b{s};
    f.cin4 = b.take(B * 4 * hw); f.lin3 = b.take(B * 3 * hw); f.t16 = b.take(B * 16 * hw); f.crcb = b.take(B * 2 * hw);
    f.t32 = b.take(B * 32 * hw); f.d3 = b.take(B * 3 * hw); f.rgb = b.take(B * 3 * hw);
    pyramid_layout(f.pyr, b, B, H, W, 0, levels);
    f.amax = reinterpret_cast<int*>(b.take(B));
    return f;
}

// EnhancedBayerProcessor + pyramid.  wp_* = packed 3x3 weights of the four small convolutions.
int launch_tc_front(const float* in, int mosaic, const float* wb_gains, const float* color_matrix, const float* wp_c0, const float* b_c0,
                    const float* wp_c2, const float* b_c2, const float* wp_d0, const float* b_d0, const float* wp_d2, const float* b_d2,
                    float* scratch, int B, int H, int W, int levels, hipStream_t st) {
    RF_CHECK_ARG(levels >= 1 && levels <= 3 && H % 2 == 0 && W % 2 == 0 && B <= 65535, "truecolor front: levels=%d H=%d W=%d unsupported", levels, H, W);
    const TcFrontBufs f = tc_front_layout(scratch, B, H, W, levels);
    const size_t hw = (size_t)H * W;
    ProfScope prof(st, "tc_front(EnhancedBayerProcessor)", 2.0 * B * hw * 9.0 * (4 * 16 + 16 * 2 + 3 * 32 + 32 * 3), 4.0 * B * hw * 80.0);
    launch_guide_init(f.amax, B, st);
    const int cap = 2048 / B > 32 ? 2048 / B : 32;
    tc_front_kernel<<<dim3((unsigned)grid1d(hw, cap), (unsigned)B), 256, 0, st>>>(in, mosaic, wb_gains, color_matrix, f.cin4, f.lin3, f.amax, H, W);
    const GuidePyramid& r = f.pyr;
    tc_normalise_kernel<<<dim3((unsigned)grid1d(hw / 4, 1024), (unsigned)B), 256, 0, st>>>(f.cin4, f.amax, r.ll[0], r.mag[0], H, W);
    for (int i = 1; i < levels; ++i)
        tc_pyramid_kernel<<<dim3((unsigned)grid1d((size_t)r.lh[i] * r.lw[i], 1024), (unsigned)B), 256, 0, st>>>(r.ll[i - 1], r.ll[i], r.mag[i], r.lh[i - 1], r.lw[i - 1]);
    if (int rc = check_launch("tc_front")) return rc;
    auto conv = [&](const float* x, float* out, const float* wp, const float* bias, int cin, int cout, int act) {
        Conv3x3Args a{};
        a.x = x; a.x_bstride = (int64_t)cin * hw; a.wp = wp; a.bias = bias; a.out = out; a.out_bstride = (int64_t)cout * hw;
        a.B = B; a.Cin = cin; a.Cout = cout; a.h = H; a.w = W; a.act = act;
        return launch_conv3x3(a, st);
    };
    if (int rc = conv(f.cin4, f.t16, wp_c0, b_c0, 4, 16, 2)) return rc;       // chroma_extractor: conv, ReLU, conv, Tanh
    if (int rc = conv(f.t16, f.crcb, wp_c2, b_c2, 16, 2, 4)) return rc;
    if (int rc = conv(f.lin3, f.t32, wp_d0, b_d0, 3, 32, 3)) return rc;       // demosaic_refine: conv, GELU, conv (+ residual)
    if (int rc = conv(f.t32, f.d3, wp_d2, b_d2, 32, 3, 0)) return rc;
    tc_add_kernel<<<grid1d(B * 3 * hw), 256, 0, st>>>(f.lin3, f.d3, f.rgb, B * 3 * hw);
    return check_launch("tc_front");
}

// one more pyramid level: Haar LL and high-band magnitude of `src` [B][hs][ws] (the multi-level FLCA variant builds its own pyramid)
int launch_tc_pyramid(const float* src, float* ll, float* mag, int B, int hs, int ws, hipStream_t st) {
    RF_CHECK_ARG(B <= 65535 && hs >= 2 && ws >= 2, "pyramid level of a %dx%d plane", hs, ws);
    const size_t n = (size_t)((hs + 1) / 2) * ((ws + 1) / 2);
    ProfScope prof(st, "tc_pyramid_kernel", 0.0, 4.0 * B * n * 6);
    tc_pyramid_kernel<<<dim3((unsigned)grid1d(n, 1024), (unsigned)B), 256, 0, st>>>(src, ll, mag, hs, ws);
    return check_launch("tc_pyramid");
}

int launch_tc_guide_level(const float* scratch, float* guide, int B, int H, int W, int levels, int hf, int wf, hipStream_t st) {
    const TcFrontBufs f = tc_front_layout(const_cast<float*>(scratch), B, H, W, levels);
    TcGuideSrc s{};
    s.y = f.cin4 + 3 * (size_t)H * W; s.crcb = f.crcb; s.rgb = f.rgb; s.pyr = f.pyr;
    ProfScope prof(st, "tc_guide_level_kernel", 0.0, 4.0 * B * hf * wf * 14);
    tc_guide_level_kernel<<<dim3((unsigned)grid1d((size_t)hf * wf, 1024), (unsigned)B), 256, 0, st>>>(s, guide, H, W, hf, wf);
    return check_launch("tc_guide_level");
}

// the bayer-processor outputs themselves, for operator-level parity tests: y [B,1,H,W], crcb [B,2,H,W], rgb [B,3,H,W]
int tc_front_outputs(const float* scratch, const float** y, const float** crcb, const float** rgb, int B, int H, int W, int levels) {
    const TcFrontBufs f = tc_front_layout(const_cast<float*>(scratch), B, H, W, levels);
    *y = f.cin4 + 3 * (size_t)H * W; *crcb = f.crcb; *rgb = f.rgb;
    return RF_OK;
}

int tc_nblk(int h, int w) { return (w % 4 == 0) ? cdiv(h * w, 1024) : cdiv(h * w, 256); }

int launch_tc_spatial(const float* feat, float* xs, const float* guide, const float* w_col, const float* b_col, const float* w_low,
                      const float* b_low, const float* w_high, const float* b_high, int B, int C, int h, int w, hipStream_t st) {
    RF_CHECK_ARG(C <= 512 && B <= 65535, "truecolor flca: C=%d > 512 not supported", C);
    TcSpatialArgs a{feat, xs, guide, w_col, b_col, w_low, b_low, w_high, b_high, B, C, h, w};
    const double el = (double)B * C * h * w;
    ProfScope prof(st, "tc_spatial_kernel", 130.0 * el, 8.0 * el);
    const bool vec = (w % 4 == 0) && aligned16(feat) && aligned16(xs);
    if (vec) tc_spatial_kernel<4><<<dim3((unsigned)cdiv(h * w, 1024), (unsigned)cdiv(C, 32), (unsigned)B), 256, 0, st>>>(a);
    else tc_spatial_kernel<1><<<dim3((unsigned)cdiv(h * w, 256), (unsigned)cdiv(C, 32), (unsigned)B), 256, 0, st>>>(a);
    return check_launch("tc_spatial");
}

int launch_tc_residual(const float* xs, const float* r, float* x2, float* partial, int B, int C, int h, int w, hipStream_t st) {
    RF_CHECK_ARG(C <= 512 && B <= 65535, "truecolor flca: C=%d > 512 not supported", C);
    const int P = h * w, nblk = tc_nblk(h, w);
    ProfScope prof(st, "tc_residual_kernel", 8.0 * B * C * P, 12.0 * B * C * P);
    const bool vec = (w % 4 == 0) && aligned16(xs) && aligned16(r) && aligned16(x2);
    RF_CHECK_ARG(vec || w % 4 != 0, "truecolor flca: buffers must be 16-byte aligned");
    if (vec) tc_residual_kernel<4><<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(xs, r, x2, partial, nblk, C, P);
    else tc_residual_kernel<1><<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(xs, r, x2, partial, nblk, C, P);
    return check_launch("tc_residual");
}

int launch_tc_color_head(float* x, const float* const* prm /* gamma, ct.0.w, ct.0.b, ct.2.w, ct.2.b, tone.0.w, tone.0.b, tone.2.w, tone.2.b */,
                         int B, size_t P, hipStream_t st) {
    ProfScope prof(st, "tc_color_head_kernel", 2.0 * B * P * (3 * 64 * 2 + 3 * 64), 24.0 * B * P);
    const int cap = 4096 / B > 64 ? 4096 / B : 64;
    tc_color_head_kernel<<<dim3((unsigned)grid1d(P, cap), (unsigned)B), 256, 0, st>>>(x, prm[0], prm[1], prm[2], prm[3], prm[4], prm[5], prm[6], prm[7], prm[8], P);
    return check_launch("tc_color_head");
}

// what the gate and residual kernels of this file and of rf_multilvl.hip index with int: B in the grid, h * w pixels
int check_gate_shape(const char* who, int B, int C, int h, int w) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && h >= 1 && w >= 1, "%s: B=%d C=%d h=%d w=%d: every size must be positive and B <= 65535", who, B, C, h, w);
    RF_CHECK_ARG(C <= 512, "%s: C=%d > 512 not supported", who, C);
    RF_CHECK_ARG((size_t)h * w <= (1u << 28), "%s: a %dx%d plane exceeds 2^28 pixels", who, h, w);
    return RF_OK;
}

}  // namespace rf

using namespace rf;

// ---- the kernels one by one (include/rawformer_hip.h): argument checks, then the launch functions above ----------------------
extern "C" {

int rf_tc_spatial(const float* feat, const float* guide, const float* w_col, const float* b_col, const float* w_low, const float* b_low,
                  const float* w_high, const float* b_high, float* xs, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(feat && guide && w_col && b_col && w_low && b_low && w_high && b_high && xs, "rf_tc_spatial: null argument");
    RF_TRY(check_gate_shape("rf_tc_spatial", B, C, h, w));
    RF_CHECK_ARG(aligned4(feat) && aligned4(guide) && aligned4(xs) && aligned4(w_col) && aligned4(b_col) && aligned4(w_low) && aligned4(b_low) &&
                     aligned4(w_high) && aligned4(b_high), "rf_tc_spatial: buffers must be 4-byte aligned");
    return launch_tc_spatial(feat, xs, guide, w_col, b_col, w_low, b_low, w_high, b_high, B, C, h, w, (hipStream_t)stream);
}

int rf_tc_nblk(int h, int w) {
    RF_CHECK_ARG(h >= 1 && w >= 1 && (size_t)h * w <= (1u << 28), "rf_tc_nblk: a %dx%d plane", h, w);
    return tc_nblk(h, w);
}

int rf_tc_residual(const float* xs, const float* r, float* x2, float* partial, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(xs && r && x2 && partial, "rf_tc_residual: null argument");
    RF_TRY(check_gate_shape("rf_tc_residual", B, C, h, w));
    RF_CHECK_ARG(aligned4(xs) && aligned4(r) && aligned4(x2) && aligned4(partial), "rf_tc_residual: buffers must be 4-byte aligned");
    RF_CHECK_ARG(w % 4 != 0 || (aligned16(xs) && aligned16(r) && aligned16(x2)),
                 "rf_tc_residual: buffers must be 16-byte aligned where the width is a multiple of 4");
    return launch_tc_residual(xs, r, x2, partial, B, C, h, w, (hipStream_t)stream);
}

int rf_tc_color_head(float* x, const float* gamma, const float* ct0_w, const float* ct0_b, const float* ct2_w, const float* ct2_b,
                     const float* tone0_w, const float* tone0_b, const float* tone2_w, const float* tone2_b, int B, size_t P, void* stream) {
    const float* prm[9] = {gamma, ct0_w, ct0_b, ct2_w, ct2_b, tone0_w, tone0_b, tone2_w, tone2_b};
    RF_CHECK_ARG(x && aligned4(x), "rf_tc_color_head: the image is null or not 4-byte aligned");
    for (const float* p : prm) RF_CHECK_ARG(p && aligned4(p), "rf_tc_color_head: a parameter pointer is null or not 4-byte aligned");
    RF_CHECK_ARG(B >= 1 && B <= 65535 && P >= 1 && P <= ((size_t)1 << 40), "rf_tc_color_head: B=%d P=%zu: B in 1..65535, P in 1..2^40", B, P);
    return launch_tc_color_head(x, prm, B, P, (hipStream_t)stream);
}

int rf_tc_pyramid(const float* src, float* ll, float* mag, int B, int hs, int ws, void* stream) {
    RF_CHECK_ARG(src && ll && mag && aligned4(src) && aligned4(ll) && aligned4(mag), "rf_tc_pyramid: a buffer is null or not 4-byte aligned");
    RF_CHECK_ARG(B >= 1 && (size_t)(hs > 0 ? hs : 0) * (ws > 0 ? ws : 0) <= (1u << 30), "rf_tc_pyramid: B=%d, a %dx%d plane", B, hs, ws);
    return launch_tc_pyramid(src, ll, mag, B, hs, ws, (hipStream_t)stream);
}

}  // extern "C"
