// The gradient pieces of the WMB block (RawFomer_WFB_FFAB/model.py:215-245) that the block operators of rf_mamba_bwd.hip,
// rf_wm_bwd.hip, rf_ffab_bwd.hip and rf_wfb_train.hip do not cover.  With the names of rf_wmb.hip's header:
//
//   front     t = 2 LN1(x) - 1, bands = dwt_init(t)                    g  = grad_t + dwt_init^T(grad_bands) = grad_t + iwt_init(grad_bands)
//                                                                      dx = r (g w2 - mean_c(g w2) - xh mean_c(g w2 xh)),  xh = (x - mu) r
//                                                                      d w2 = sum g xh,  d b2 = sum g                        wmb_front_bwd_kernel
//   back      u = t + clamp((iwt_init(bands) + 1) / 2, 0, 1)           grad_t = grad_u;  grad_bands = iwt_init^T(m grad_u / 2) = dwt_init(m grad_u / 2),
//                                                                      m = [0 <= pre-clamp value <= 1]                       wmb_back_bwd_kernel
//   5x5       depth_conv of Illumination_Estimator                     dx = the stencil on flipped taps;  25 tap sums and the bias sum per channel
//                                                                                                           dw5_dgrad_kernel, dw5_wgrad_kernel
//   Illumination_Estimator                                             a schedule over rf_grad.h, the 5x5 pair and two small weight kernels
//   LN2       v = LN2(u)                                               launch_ln_bwd of rf_train.hip behind an entry point
//
// The Haar pair is orthogonal: dwt_init^T is iwt_init and iwt_init^T is dwt_init, halves and signs included.
//
// wmb_front_bwd_kernel.  An item is what a lane of wmb_front_kernel owns: 4 consecutive pixels of two adjacent rows (two 2x2 quads,
// two band pixels), but here KS lanes share an item's channels (the layout of ln_bwd_reg_kernel): lane (j, ks) of a wave keeps
// channels ks, ks + KS, .. of item j in registers, x and g both, so x, grad_t and grad_bands are read once and grad_x written
// once; g never exists in memory.  KS is the smallest of 4, 8, 16, 32, 64 that leaves at most 4 channels per lane (at 64: up to 8),
// so C = 256 runs one item per wave where wmb_front_kernel runs one per lane.  Slots past C (C no multiple of KS) load channel 0 and
// are masked out of every sum.  The channel sums of d w2 / d b2 stay in registers over the workgroup's items and leave as one
// slab per workgroup.
//
// Every per-parameter sum over pixels goes to per-workgroup slabs that reduce_rows adds in a fixed order: no float atomics, two
// calls give the same bits.  The entry points follow rf_grad.h: check_backward_args, a *_workspace_bytes query, an accumulate flag,
// nothing kept from a forward call, inputs never written.
#include "rf_grad.h"
#include "rf_layernorm.h"

namespace rf {

namespace {

constexpr int kBlk = 256;

__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// ---- front.  x, gt, dx [B][C][2h][2w], gb [4B][C][h][w]; grid (nblk, B); partial[(image, workgroup)][2][C]: the slabs of d w2 and
// d b2, gscale applied
template <int CPL, int KS>
__global__ void __launch_bounds__(kBlk) wmb_front_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gt, const float* __restrict__ gb,
                                                             const float* __restrict__ gamma, float* __restrict__ dx, float* __restrict__ partial,
                                                             float eps, float gscale, int B, int C, int h, int w) {
    constexpr int G = 64 / KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % G, ks = lane / G;
    const int W = 2 * w, wv = w / 2, nit = h * wv, per_wg = 4 * G;
    const size_t P = (size_t)4 * h * w, hw = (size_t)h * w, bs = (size_t)B * C * hw, img = blockIdx.y;
    const float* xb = x + img * C * P;
    const float* tb = gt + img * C * P;
    const float* bb = gb + img * C * hw;
    float* ob = dx + img * C * P;
    float gam[CPL], lm[CPL], ag[CPL], ab[CPL];
    int cs[CPL];
#pragma unroll
    for (int s = 0; s < CPL; ++s) {
        const int c = ks + KS * s;
        cs[s] = c < C ? c : 0;
        lm[s] = c < C ? 1.0f : 0.f;
        gam[s] = c < C ? gamma[c] : 0.f;
        ag[s] = 0.f;
        ab[s] = 0.f;
    }
    const float invC = 1.0f / (float)C;
    for (int i0 = blockIdx.x * per_wg; i0 < nit; i0 += gridDim.x * per_wg) {
        const int it = i0 + wave * G + j;
        const bool ok = it < nit;                     // lanes past the end work on item 0 and store nothing
        const int itc = ok ? it : 0, xv = itc % wv, y = itc / wv;
        const size_t o0 = (size_t)(2 * y) * W + 4 * xv, o1 = (size_t)y * w + 2 * xv;
        float xs[CPL][8], gs[CPL][8];
#pragma unroll
        for (int s = 0; s < CPL; ++s) {
            const size_t co = (size_t)cs[s] * P + o0;
            const float4 xa = ld4(xb + co), xd = ld4(xb + co + W), ta = ld4(tb + co), td = ld4(tb + co + W);
            const float* bp = bb + (size_t)cs[s] * hw + o1;
            const float2 p0 = ld2(bp), p1 = ld2(bp + bs), p2 = ld2(bp + 2 * bs), p3 = ld2(bp + 3 * bs);
            float r[8];
            haar_synthesis(p0.x, p1.x, p2.x, p3.x, r[0], r[1], r[4], r[5]);
            haar_synthesis(p0.y, p1.y, p2.y, p3.y, r[2], r[3], r[6], r[7]);
            xs[s][0] = xa.x; xs[s][1] = xa.y; xs[s][2] = xa.z; xs[s][3] = xa.w;
            xs[s][4] = xd.x; xs[s][5] = xd.y; xs[s][6] = xd.z; xs[s][7] = xd.w;
            gs[s][0] = ta.x + r[0]; gs[s][1] = ta.y + r[1]; gs[s][2] = ta.z + r[2]; gs[s][3] = ta.w + r[3];
            gs[s][4] = td.x + r[4]; gs[s][5] = td.y + r[5]; gs[s][6] = td.z + r[6]; gs[s][7] = td.w + r[7];
#pragma unroll
            for (int q = 0; q < 8; ++q) { xs[s][q] *= lm[s]; gs[s][q] *= lm[s]; }
        }
        float mu[8], rstd[8], s1[8], s2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float m = 0.f;
#pragma unroll
            for (int s = 0; s < CPL; ++s) m += xs[s][q];
#pragma unroll
            for (int o = G; o < 64; o <<= 1) m += __shfl_xor(m, o, 64);
            mu[q] = m * invC;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                xs[s][q] = (xs[s][q] - mu[q]) * lm[s];
                v = fmaf(xs[s][q], xs[s][q], v);
            }
#pragma unroll
            for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            rstd[q] = ln_rstd(v, invC, eps);
            s1[q] = 0.f;
            s2[q] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < CPL; ++s) {
            float ta = 0.f, tb2 = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                xs[s][q] *= rstd[q];                   // xhat in place
                ta = fmaf(gs[s][q], xs[s][q], ta);
                tb2 += gs[s][q];
                gs[s][q] *= gam[s];
                s1[q] += gs[s][q];
                s2[q] = fmaf(gs[s][q], xs[s][q], s2[q]);
            }
            ag[s] += ok ? ta : 0.f;
            ab[s] += ok ? tb2 : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int o = G; o < 64; o <<= 1) { s1[q] += __shfl_xor(s1[q], o, 64); s2[q] += __shfl_xor(s2[q], o, 64); }
            s1[q] *= invC;
            s2[q] *= invC;
        }
        if (ok) {
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                if (ks + KS * s >= C) continue;
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = rstd[q] * (gs[s][q] - s1[q] - xs[s][q] * s2[q]);
                float* o = ob + (size_t)cs[s] * P + o0;
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(o + W) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
    }
    // channel sums: over the G item lanes of a slice (butterfly), then over the four waves in a fixed order
    __shared__ float red[4][2][CPL * KS];
#pragma unroll
    for (int s = 0; s < CPL; ++s) {
#pragma unroll
        for (int o = 1; o < G; o <<= 1) { ag[s] += __shfl_xor(ag[s], o, 64); ab[s] += __shfl_xor(ab[s], o, 64); }
        if (j == 0) { red[wave][0][ks + KS * s] = ag[s]; red[wave][1][ks + KS * s] = ab[s]; }
    }
    __syncthreads();
    const size_t row = img * gridDim.x + blockIdx.x;
    for (int c = threadIdx.x; c < C; c += kBlk) {
        partial[row * 2 * C + c] = gscale * ((red[0][0][c] + red[1][0][c]) + (red[2][0][c] + red[3][0][c]));
        partial[row * 2 * C + C + c] = gscale * ((red[0][1][c] + red[1][1][c]) + (red[2][1][c] + red[3][1][c]));
    }
}

// ---- back.  bands, gbands [4B][C][h][w], go [B][C][2h][2w]; an item is wmb_back_kernel's: two band pixels
__global__ void __launch_bounds__(kBlk) wmb_back_bwd_kernel(const float* __restrict__ bands, const float* __restrict__ go, float* __restrict__ gbands,
                                                            int B, int C, int h, int w) {
    const int wv = w / 2, W = 2 * w;
    const size_t bs = (size_t)B * C * h * w, items = (size_t)B * C * h * wv;
    for (size_t it = blockIdx.x * (size_t)kBlk + threadIdx.x; it < items; it += (size_t)gridDim.x * kBlk) {
        const int xv = (int)(it % wv), y = (int)((it / wv) % h);
        const size_t pl = it / ((size_t)wv * h);
        const size_t ib = (pl * h + y) * (size_t)w + 2 * xv;
        const float* i0 = bands + ib;
        const float2 p0 = ld2(i0), p1 = ld2(i0 + bs), p2 = ld2(i0 + 2 * bs), p3 = ld2(i0 + 3 * bs);
        const size_t o = (pl * 2 * h + 2 * y) * (size_t)W + 4 * xv;
        const float4 ga = ld4(go + o), gd = ld4(go + o + W);
        float r[8];
        haar_synthesis(p0.x, p1.x, p2.x, p3.x, r[0], r[1], r[4], r[5]);
        haar_synthesis(p0.y, p1.y, p2.y, p3.y, r[2], r[3], r[6], r[7]);
        const float g[8] = {ga.x, ga.y, ga.z, ga.w, gd.x, gd.y, gd.z, gd.w};
        float m[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float v = (r[q] + 1.0f) * 0.5f;      // the forward's value before the clamp; torch.clamp passes the gradient on [0, 1]
            m[q] = (v >= 0.0f && v <= 1.0f) ? 0.5f * g[q] : 0.f;
        }
        float2 ll, hl, lh, hh;      // dwt_init of the quad (m0 m1 / m4 m5), then of (m2 m3 / m6 m7)
        haar_analysis(m[0], m[1], m[4], m[5], ll.x, hl.x, lh.x, hh.x);
        haar_analysis(m[2], m[3], m[6], m[7], ll.y, hl.y, lh.y, hh.y);
        float* ob = gbands + ib;
        *reinterpret_cast<float2*>(ob) = ll;
        *reinterpret_cast<float2*>(ob + bs) = hl;
        *reinterpret_cast<float2*>(ob + 2 * bs) = lh;
        *reinterpret_cast<float2*>(ob + 3 * bs) = hh;
    }
}

// ---- depthwise 5x5, padding 2.  Data gradient: dwconv5x5_kernel's geometry (a thread owns 4 pixels x 2 rows) on the flipped taps,
// no bias; everything outside the plane is zero
__global__ void __launch_bounds__(kBlk) dw5_dgrad_kernel(const float* __restrict__ dy, float* __restrict__ dx, const float* __restrict__ wgt, int B,
                                                         int C, int h, int w) {
    const int wv = (w + 3) / 4, hr = (h + 1) / 2;
    const size_t items = (size_t)B * C * hr * wv;
    for (size_t it = blockIdx.x * (size_t)kBlk + threadIdx.x; it < items; it += (size_t)gridDim.x * kBlk) {
        const int xv = (int)(it % wv), yr = (int)((it / wv) % hr);
        const size_t pl = it / ((size_t)wv * hr);
        const float* gp = dy + pl * (size_t)h * w;
        float* op = dx + pl * (size_t)h * w;
        const float* k = wgt + (pl % C) * 25;
        const int x0 = xv * 4, y0 = yr * 2;
        float acc[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[r][p] = 0.f;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            const int y = y0 + rr - 2;
            if (y < 0 || y >= h) continue;
            const float* row = gp + (size_t)y * w;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int xx = x0 - 2 + i;
                v[i] = (xx >= 0 && xx < w) ? row[xx] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int ky = rr - r;
                if (ky >= 0 && ky < 5) {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int kx = 0; kx < 5; ++kx) acc[r][p] = fmaf(k[24 - (ky * 5 + kx)], v[p + kx], acc[r][p]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + r;
            if (y >= h) continue;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (x0 + p < w) op[(size_t)y * w + x0 + p] = acc[r][p];
        }
    }
}

// Weight gradient: grid (slab, channel, image); a lane owns 4 consecutive pixels of a row of dy and walks the 5 x 8 window of x
// around them.  pw[(image, slab)][c][25], pb[(image, slab)][c]
__global__ void __launch_bounds__(kBlk) dw5_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ pw,
                                                         float* __restrict__ pb, int C, int h, int w, int nblk, int vec) {
    __shared__ float red[26 * 4];
    const int c = blockIdx.y, img = blockIdx.z;
    const size_t off = ((size_t)img * C + c) * h * w;
    const float* xr = x + off;
    const float* dr = dy + off;
    const int wv = (w + 3) / 4, items = h * wv, per = (items + nblk - 1) / nblk;
    const int lo = blockIdx.x * per, hi = lo + per < items ? lo + per : items;
    float s[26];
#pragma unroll
    for (int k = 0; k < 26; ++k) s[k] = 0.f;
    for (int it = lo + threadIdx.x; it < hi; it += kBlk) {
        const int x0 = (it % wv) * 4, y = it / wv;
        float d[4];
        if (vec) {
            const float4 t = ld4(dr + (size_t)y * w + x0);
            d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) d[p] = x0 + p < w ? dr[(size_t)y * w + x0 + p] : 0.f;
        }
        s[25] += (d[0] + d[1]) + (d[2] + d[3]);
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const int yy = y + ky - 2;
            if (yy < 0 || yy >= h) continue;
            const float* row = xr + (size_t)yy * w;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int xx = x0 - 2 + i;
                v[i] = (xx >= 0 && xx < w) ? row[xx] : 0.f;
            }
#pragma unroll
            for (int kx = 0; kx < 5; ++kx)
#pragma unroll
                for (int p = 0; p < 4; ++p) s[ky * 5 + kx] = fmaf(d[p], v[p + kx], s[ky * 5 + kx]);
        }
    }
    block_sums<26>(s, red);
    if (threadIdx.x == 0) {
        const size_t row = (size_t)img * nblk + blockIdx.x;
#pragma unroll
        for (int k = 0; k < 25; ++k) pw[(row * C + c) * 25 + k] = s[k];
        pb[row * C + c] = s[25];
    }
}

// ---- Illumination_Estimator's weight helpers.  wf [Cm][C] = W_img + w_mean / C of conv1.weight [Cm][C + 1] (wmb_fold_kernel's fold)
__global__ void __launch_bounds__(kBlk) illu_fold_kernel(const float* __restrict__ w1, float* __restrict__ wf, int Cm, int C) {
    for (int i = blockIdx.x * kBlk + threadIdx.x; i < Cm * C; i += gridDim.x * kBlk) {
        const int r = i / C, k = i - r * C;
        wf[i] = w1[r * (C + 1) + k] + w1[r * (C + 1) + C] / (float)C;
    }
}
// d conv1.weight [Cm][C + 1] (+)= [fresh | row mean of fresh] for fresh [Cm][C] = sum g_x1 img^T of THIS call: the mean column is
// sum g_x1 mean_c(img) = the mean over k of row r, added in order
__global__ void __launch_bounds__(kBlk) illu_dw1_kernel(const float* __restrict__ fresh, float* __restrict__ dw1, int Cm, int C, int accumulate) {
    const int r = blockIdx.x * kBlk + threadIdx.x;
    if (r >= Cm) return;
    float s = 0.f;
    for (int k = 0; k < C; ++k) {
        const float v = fresh[r * C + k];
        s += v;
        float* o = dw1 + r * (C + 1) + k;
        *o = accumulate ? *o + v : v;
    }
    float* o = dw1 + r * (C + 1) + C;
    s /= (float)C;
    *o = accumulate ? *o + s : s;
}

}  // namespace

// ---- host side
static int band_geometry(const char* who, int B, int C, int h, int w) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 4 && C <= 512, "%s: B %d, C %d (C must be 4 .. 512)", who, B, C);
    RF_CHECK_ARG(h >= 1 && w >= 2 && w % 2 == 0 && (double)h * w < (double)(1 << 28),
                 "%s: band size %d x %d (the band width w must be even: the full-resolution width 2w a multiple of 4)", who, h, w);
    return RF_OK;
}

// lanes per item of wmb_front_bwd_kernel, and its workgroups per image: one per 4 * (64 / KS) items, at most about 512 over the batch
// (at up to 192 registers a CU holds two of them: 512 are resident at once, and every slab is a row for reduce_rows to add).
// Not RF_LN_SLICE_TABLE of rf_layernorm.h: with 8 pixels and x and g per slot the rule here is at most 4 channels per lane, for any C
static int front_ks(int C) {
    int ks = 4;
    while (ks < 64 && cdiv(C, ks) > 4) ks <<= 1;
    return ks;
}
int wmb_front_bwd_nblk(int B, int C, int h, int w) {
    const int per_wg = 4 * (64 / front_ks(C)), gx = cdiv(h * (w / 2), per_wg), cap = cdiv(512, B);
    return gx > cap ? cap : gx;
}

int launch_wmb_front_bwd(const float* x, const float* gt, const float* gb, const float* gamma, float* dx, float* partial, float gscale, int B, int C,
                         int h, int w, hipStream_t st) {
    const int ks = front_ks(C), cpl = cdiv(C, ks);
    const dim3 grid((unsigned)wmb_front_bwd_nblk(B, C, h, w), (unsigned)B);
    const double el = 4.0 * B * C * (double)h * w;
    ProfScope prof(st, "wmb_front_bwd_kernel", 30.0 * el, 16.0 * el);
#define RF_FRONT(CPL, KS) \
    case CPL * 100 + KS: wmb_front_bwd_kernel<CPL, KS><<<grid, kBlk, 0, st>>>(x, gt, gb, gamma, dx, partial, 1e-5f, gscale, B, C, h, w); break
    switch (cpl * 100 + ks) {
        RF_FRONT(1, 4); RF_FRONT(2, 4); RF_FRONT(3, 4); RF_FRONT(4, 4);
        RF_FRONT(3, 8); RF_FRONT(4, 8); RF_FRONT(3, 16); RF_FRONT(4, 16); RF_FRONT(3, 32); RF_FRONT(4, 32);
        RF_FRONT(3, 64); RF_FRONT(4, 64); RF_FRONT(5, 64); RF_FRONT(6, 64); RF_FRONT(7, 64); RF_FRONT(8, 64);
        default: RF_CHECK_ARG(false, "wmb_front_backward: no kernel for C %d", C);
    }
#undef RF_FRONT
    return check_launch("wmb_front_bwd");
}

int launch_wmb_back_bwd(const float* bands, const float* go, float* gbands, int B, int C, int h, int w, hipStream_t st) {
    const double el = 4.0 * B * C * (double)h * w;
    ProfScope prof(st, "wmb_back_bwd_kernel", 8.0 * el, 12.0 * el);
    wmb_back_bwd_kernel<<<grid1d((size_t)B * C * h * (w / 2)), kBlk, 0, st>>>(bands, go, gbands, B, C, h, w);
    return check_launch("wmb_back_bwd");
}

// slabs per plane of dw5_wgrad_kernel: one per 1024 groups of 4 pixels, at most 32
static int dw5_nblk(int h, int w) {
    const long long n = ((long long)h * cdiv(w, 4) + 1023) / 1024;
    return (int)(n > 32 ? 32 : n < 1 ? 1 : n);
}
static int dw5_geometry(const char* who, int B, int C, int h, int w) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && C <= 65535, "%s: B %d, C %d (1 .. 65535 each)", who, B, C);
    RF_CHECK_ARG(h >= 1 && w >= 1 && (double)h * w < (double)(1 << 28), "%s: plane %d x %d", who, h, w);
    return RF_OK;
}
struct Dw5Plan { size_t pw, pb, total; };
static Dw5Plan dw5_plan(int B, int C, int h, int w) {
    Bump b;
    Dw5Plan p;
    const size_t rows = (size_t)B * dw5_nblk(h, w);
    p.pw = b.off(rows * C * 25);
    p.pb = b.off(rows * C);
    p.total = b.used;
    return p;
}
// dx = the 5x5 stencil of dy on the flipped taps; dw [C][25], db [C] (+)= the tap and bias sums
static int run_dw5_backward(const float* x, const float* dy, float* dx, const float* wgt, float* dw, float* db, float* pw, float* pb, int B, int C, int h,
                            int w, int acc, hipStream_t st) {
    const int nblk = dw5_nblk(h, w), vec = w % 4 == 0 && aligned16(dy);
    const double el = (double)B * C * h * w;
    {
        ProfScope prof(st, "dw5_wgrad_kernel", 202.0 * el, 8.0 * el);
        dw5_wgrad_kernel<<<dim3((unsigned)nblk, (unsigned)C, (unsigned)B), kBlk, 0, st>>>(x, dy, pw, pb, C, h, w, nblk, vec);
        RF_TRY(check_launch("dw5_wgrad"));
    }
    RF_TRY(reduce_rows(pw, dw, B * nblk, (size_t)C * 25, acc, st));
    RF_TRY(reduce_rows(pb, db, B * nblk, (size_t)C, acc, st));
    ProfScope prof(st, "dw5_dgrad_kernel", 50.0 * el, 8.0 * el);
    dw5_dgrad_kernel<<<grid1d((size_t)B * C * cdiv(h, 2) * cdiv(w, 4), 8192), kBlk, 0, st>>>(dy, dx, wgt, B, C, h, w);
    return check_launch("dw5_dgrad");
}

// ---- Illumination_Estimator.  prm: conv1.weight [Cm][C + 1], conv1.bias, depth_conv.weight [Cm][25], depth_conv.bias,
// conv2.weight [Co][Cm], conv2.bias
enum { kW1, kB1, kWd, kBd, kW2, kB2, kIlluPrm };
size_t illu_prm_floats(int i, int C, int Cm, int Co) {
    switch (i) {
        case kW1: return (size_t)Cm * (C + 1);
        case kWd: return (size_t)Cm * 25;
        case kW2: return (size_t)Co * Cm;
        case kB2: return (size_t)Co;
        default: return (size_t)Cm;
    }
}
struct IlluPlan { size_t x1, fea, gf, gx1, wf, wpack, dw1, db1, dw5, wpart, wpart_cap, total; };
static int illu_plan(const char* who, int B, int C, int Cm, int Co, int h, int w, bool with_map, IlluPlan* p) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (double)h * w < (double)(1 << 28), "%s: B %d, plane %d x %d", who, B, h, w);
    RF_CHECK_ARG(C >= 4 && C <= 512 && C % 4 == 0, "%s: C %d (the image's channels must be a multiple of 4 in 4 .. 512)", who, C);
    RF_CHECK_ARG(Cm >= 4 && Cm <= 512 && Cm % 4 == 0, "%s: Cm %d (conv1's output channels must be a multiple of 4 in 4 .. 512)", who, Cm);
    RF_CHECK_ARG(Co >= 4 && Co <= 512 && Co % 4 == 0, "%s: Co %d (conv2's output channels must be a multiple of 4 in 4 .. 512)", who, Co);
    Bump b;
    const int P = h * w;
    const size_t U = (size_t)B * Cm * P;
    p->x1 = b.off(U);
    p->fea = b.off(with_map ? U : 0);
    p->gf = b.off(with_map ? U : 0);
    p->gx1 = b.off(U);
    p->wf = b.off((size_t)Cm * C);
    size_t pk = 0;
    for (const size_t f : {packed1x1_floats(C, Cm), packed1x1_floats(Cm, C), packed1x1_floats(Co, Cm), packed1x1_floats(Cm, Co)}) pk = pk > f ? pk : f;
    p->wpack = b.off(pk);
    p->dw1 = b.off((size_t)Cm * C);
    p->db1 = b.off((size_t)Cm);
    p->dw5 = b.off(dw5_plan(B, Cm, h, w).total);
    size_t cap = wgrad1x1_partial_floats(B, Cm, C, P, true);
    if (with_map) {
        const size_t f = wgrad1x1_partial_floats(B, Co, Cm, P, true);
        cap = cap > f ? cap : f;
    }
    p->wpart_cap = cap;
    p->wpart = b.off(cap);
    p->total = b.used;
    return RF_OK;
}

static int run_illu_backward(const char* who, const IlluPlan& p, const float* img, const float* grad_fea, const float* grad_map, float* grad_img,
                      const float* const* prm, float* const* grd, float* ws, int B, int C, int Cm, int Co, int h, int w, int acc, hipStream_t st) {
    const int P = h * w;
    float *x1 = ws + p.x1, *gx1 = ws + p.gx1, *wf = ws + p.wf, *wpack = ws + p.wpack;
    const Dw5Plan d5 = dw5_plan(B, Cm, h, w);
    illu_fold_kernel<<<grid1d((size_t)Cm * C), kBlk, 0, st>>>(prm[kW1], wf, Cm, C);
    RF_TRY(check_launch("illu_fold"));
    // x1 = conv1([img ; mean_c img]) on the folded weight
    RF_TRY(conv1x1_raw(img, x1, wf, prm[kB1], nullptr, wpack, B, C, Cm, P, 0, st));
    const float* gf = grad_fea;
    if (grad_map) {      // g_f = grad_fea + W2^T grad_map;  d conv2 from (grad_map, fea), fea recomputed
        RF_TRY(launch_dwconv5x5(x1, ws + p.fea, prm[kWd], prm[kBd], B, Cm, h, w, st));
        RF_TRY(dgrad1x1(grad_map, Co, prm[kW2], Cm, wpack, grad_fea, ws + p.gf, B, P, st));
        gf = ws + p.gf;
        RF_TRY(wgrad1x1(Wgrad{who, ws + p.wpart, p.wpart_cap, B, P, acc, st}, grad_map, Co, ws + p.fea, Cm, grd[kW2], grd[kB2]));
    }
    RF_TRY(run_dw5_backward(x1, gf, gx1, prm[kWd], grd[kWd], grd[kBd], ws + p.dw5 + d5.pw, ws + p.dw5 + d5.pb, B, Cm, h, w, acc, st));
    // d conv1: this call's sum g_x1 img^T into the workspace first; the mean column comes from those sums, not from the destination
    RF_TRY(wgrad1x1(Wgrad{who, ws + p.wpart, p.wpart_cap, B, P, 0, st}, gx1, Cm, img, C, ws + p.dw1, ws + p.db1));
    illu_dw1_kernel<<<cdiv(Cm, kBlk), kBlk, 0, st>>>(ws + p.dw1, grd[kW1], Cm, C, acc);
    RF_TRY(check_launch("illu_dw1"));
    RF_TRY(reduce_rows(ws + p.db1, grd[kB1], 1, (size_t)Cm, acc, st));
    // grad_img = (W_img + w_mean / C)^T g_x1
    return dgrad1x1(gx1, Cm, wf, C, wpack, nullptr, grad_img, B, P, st);
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_wmb_front_backward_nblk(int B, int C, int h, int w) {
    RF_TRY(band_geometry("rf_wmb_front_backward_nblk", B, C, h, w));
    return wmb_front_bwd_nblk(B, C, h, w);
}

long long rf_wmb_front_backward_workspace_bytes(int B, int C, int h, int w) {
    const int rc = band_geometry("rf_wmb_front_backward_workspace_bytes", B, C, h, w);
    return rc ? rc : (long long)((align_up((size_t)B * wmb_front_bwd_nblk(B, C, h, w) * 2 * C, 64) + align_up((size_t)2 * C, 64)) * sizeof(float));
}

int rf_wmb_front_backward(const float* x, const float* grad_t, float* grad_x, const float* grad_bands, const float* weight2, float* grad_weight2,
                          float* grad_bias2, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, float grad_scale, int accumulate,
                          void* stream) {
    const char* who = "rf_wmb_front_backward";
    RF_TRY(band_geometry(who, B, C, h, w));
    RF_CHECK_ARG(grad_bands && aligned16(grad_bands), "%s: grad_bands must be non-null and 16-byte aligned", who);
    const int rows = B * wmb_front_bwd_nblk(B, C, h, w);
    const size_t plane = (size_t)4 * B * C * h * w * sizeof(float), slabs = align_up((size_t)rows * 2 * C, 64);
    const float* prm[2] = {weight2, weight2};
    float* grd[2] = {grad_weight2, grad_bias2};
    const Span band{grad_bands, plane};
    RF_TRY(check_backward_args({who, x, grad_t, grad_x, plane, prm, grd, 2, workspace, workspace_bytes, (slabs + align_up((size_t)2 * C, 64)) * sizeof(float), &band, 1},
                               [=](int) { return (size_t)C; }));
    const hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    float* dgb = partial + slabs;      // [d w2 | d b2] of this call in ONE pass over the slabs, then to the two tensors
    RF_TRY(launch_wmb_front_bwd(x, grad_t, grad_bands, weight2, grad_x, partial, grad_scale, B, C, h, w, st));
    RF_TRY(reduce_rows(partial, dgb, rows, (size_t)2 * C, 0, st));
    RF_TRY(reduce_rows(dgb, grad_weight2, 1, (size_t)C, accumulate, st));
    return reduce_rows(dgb + C, grad_bias2, 1, (size_t)C, accumulate, st);
}

int rf_wmb_back_backward(const float* bands, const float* grad_out, float* grad_bands, int B, int C, int h, int w, void* stream) {
    const char* who = "rf_wmb_back_backward";      // no parameters and no workspace: check_backward_args's rules on its three tensors
    RF_TRY(band_geometry(who, B, C, h, w));
    RF_CHECK_ARG(bands && grad_out && grad_bands && aligned16(bands) && aligned16(grad_out) && aligned16(grad_bands),
                 "%s: bands, grad_out and grad_bands must be non-null and 16-byte aligned", who);
    const size_t plane = (size_t)4 * B * C * h * w * sizeof(float);
    RF_CHECK_ARG(!overlaps(grad_bands, plane, bands, plane) && !overlaps(grad_bands, plane, grad_out, plane),
                 "%s: grad_bands may not alias bands or grad_out", who);
    return launch_wmb_back_bwd(bands, grad_out, grad_bands, B, C, h, w, (hipStream_t)stream);
}

int rf_dwconv5x5_backward_nblk(int h, int w) {
    RF_CHECK_ARG(h > 0 && w > 0, "rf_dwconv5x5_backward_nblk: %d x %d", h, w);
    return dw5_nblk(h, w);
}

long long rf_dwconv5x5_backward_workspace_bytes(int B, int C, int h, int w) {
    const int rc = dw5_geometry("rf_dwconv5x5_backward_workspace_bytes", B, C, h, w);
    return rc ? rc : (long long)(dw5_plan(B, C, h, w).total * sizeof(float));
}

int rf_dwconv5x5_backward(const float* in, const float* grad_out, float* grad_in, const float* weight, float* grad_weight, float* grad_bias,
                          void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int accumulate, void* stream) {
    const char* who = "rf_dwconv5x5_backward";
    RF_TRY(dw5_geometry(who, B, C, h, w));
    const Dw5Plan p = dw5_plan(B, C, h, w);
    const float* prm[2] = {weight, weight};
    float* grd[2] = {grad_weight, grad_bias};
    RF_TRY(check_backward_args({who, in, grad_out, grad_in, (size_t)B * C * h * w * sizeof(float), prm, grd, 2, workspace, workspace_bytes,
                                p.total * sizeof(float)},
                               [=](int i) { return i == 0 ? (size_t)C * 25 : (size_t)C; }));
    float* ws = (float*)workspace;
    return run_dw5_backward(in, grad_out, grad_in, weight, grad_weight, grad_bias, ws + p.pw, ws + p.pb, B, C, h, w, accumulate, (hipStream_t)stream);
}

long long rf_illumination_estimator_backward_workspace_bytes(int B, int C, int Cm, int Co, int h, int w, int with_map) {
    IlluPlan p;
    const int rc = illu_plan("rf_illumination_estimator_backward_workspace_bytes", B, C, Cm, Co, h, w, with_map != 0, &p);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_illumination_estimator_backward(const float* img, const float* grad_fea, const float* grad_map, float* grad_img, const float* const* prm,
                                       float* const* grad_prm, void* workspace, size_t workspace_bytes, int B, int C, int Cm, int Co, int h, int w,
                                       int accumulate, void* stream) {
    const char* who = "rf_illumination_estimator_backward";
    IlluPlan p;
    RF_TRY(illu_plan(who, B, C, Cm, Co, h, w, grad_map != nullptr, &p));
    RF_CHECK_ARG(grad_fea && aligned16(grad_fea) && aligned16(grad_map), "%s: grad_fea must be non-null, grad_fea and grad_map 16-byte aligned", who);
    // in and grad_in are [B][C] planes; grad_fea and grad_map have their own sizes and travel as read-only buffers
    const size_t px = (size_t)B * h * w * sizeof(float);
    const Span extra[2] = {{grad_fea, px * Cm}, {grad_map, px * Co}};
    RF_TRY(check_backward_args({who, img, img, grad_img, px * C, prm, grad_prm, kIlluPrm, workspace, workspace_bytes, p.total * sizeof(float), extra,
                                grad_map ? 2 : 1},
                               [=](int i) { return illu_prm_floats(i, C, Cm, Co); }));
    return run_illu_backward(who, p, img, grad_fea, grad_map, grad_img, prm, grad_prm, (float*)workspace, B, C, Cm, Co, h, w, accumulate,
                             (hipStream_t)stream);
}

static int ln_geometry(const char* who, int B, int C, int h, int w) {
    RF_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && C <= 512, "%s: B %d, C %d (C must be 1 .. 512)", who, B, C);
    RF_CHECK_ARG(h >= 1 && w >= 1 && (double)h * w < (double)(1 << 28), "%s: plane %d x %d", who, h, w);
    return RF_OK;
}

long long rf_layernorm2d_backward_workspace_bytes(int B, int C, int h, int w) {
    const int rc = ln_geometry("rf_layernorm2d_backward_workspace_bytes", B, C, h, w);
    return rc ? rc : (long long)((align_up(ln_bwd_partial_floats(B, C, h * w), 64) + align_up((size_t)2 * C, 64)) * sizeof(float));
}

int rf_layernorm2d_backward(const float* in, const float* grad_out, float* grad_in, const float* weight, float* grad_weight, float* grad_bias,
                            const float* residual, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, float eps, int accumulate,
                            void* stream) {
    const char* who = "rf_layernorm2d_backward";
    RF_TRY(ln_geometry(who, B, C, h, w));
    RF_CHECK_ARG(aligned16(residual), "%s: residual must be 16-byte aligned", who);
    const int P = h * w;
    const size_t plane = (size_t)B * C * P * sizeof(float), part = align_up(ln_bwd_partial_floats(B, C, P), 64);
    const float* prm[2] = {weight, weight};
    float* grd[2] = {grad_weight, grad_bias};
    const Span res{residual, plane};
    RF_TRY(check_backward_args({who, in, grad_out, grad_in, plane, prm, grd, 2, workspace, workspace_bytes,
                                (part + align_up((size_t)2 * C, 64)) * sizeof(float), &res, residual ? 1 : 0},
                               [=](int) { return (size_t)C; }));
    const hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* dgb = ws + part;      // launch_ln_bwd writes [dgamma | dbeta] as one block: through the workspace, then to the two tensors
    RF_TRY(launch_ln_bwd(in, grad_out, weight, grad_in, dgb, ws, B, C, P, eps, 0, 0, st, residual, (int64_t)C * P));
    RF_TRY(reduce_rows(dgb, grad_weight, 1, (size_t)C, accumulate, st));
    return reduce_rows(dgb + C, grad_bias, 1, (size_t)C, accumulate, st);
}

}  // extern "C"
