// Training mode of the WFB FeedForward (RawFomer_WFB_FFAB/model.py:42-65) and its gradient.  In train() the two Conv2d_BN branches
// normalise with BATCH statistics, so the eval-mode fold of rf_wfb.hip (running statistics, folded once on the host) does not apply:
//
//   hid = project_in(x)                                                          [B][C][h][w], C = hidden
//   u1 = dw3x3(hid; w1)    u2 = w2 (.) hid                                       (no bias)
//   training: mu_i, v_i = mean and BIASED variance of u_i over (B, h, w), N = B h w;   eval: running_mean / running_var
//   uh_i = (u_i - mu_i) / sqrt(v_i + eps)
//   a = hid + g1 uh1 + b1 + g2 uh2 + b2      g = dw3x3(hid; wd) + bd
//   m = gelu(g) a + gelu(a) g      y = project_out(m) + x
//
// Forward: wfb_pivot_kernel / wfb_stats_kernel / wfb_stats_finish_kernel give the statistics in one pass over hid, fold them ON
// THE DEVICE into the weights of rf_wfb.hip's dwgate_kernel (given the statistics, a is one depthwise 3x3 of hid) and update the
// running statistics as nn.BatchNorm2d does; nothing is read back by the host.  The sums are taken around a per-channel pivot
// (u at the middle pixel of image 0): sum (u - p) and sum (u - p)^2 keep the variance where |mean| >> std, which
// E[u^2] - E[u]^2 loses.
//
// Backward (dy = dL/dy; sums over (B, h, w) per channel), nothing kept from a forward call:
//
//   dm = W_out^T dy;   dW_out, db_out = wgrad(dy, m);
//   da = dm (gelu(g) + gelu'(a) g)      dg = dm (gelu'(g) a + gelu(a))            wfb_gate_adjoint_kernel (writes m, da, dg, uh1)
//   db_i = sum da      dg_i = sum da uh_i                                         its per-workgroup slabs, reduce_rows
//   training: du_i = g_i / s_i (da - db_i / N - uh_i dg_i / N)     eval: du_i = g_i / s_i da          wfb_du_kernel
//   d w2 = sum du2 hid                                                            its slabs, reduce_rows
//   d w1 = dw3x3 weight gradient of (du1, hid);  d wd, d bd = that of (dg, hid)   launch_dw_wgrad
//   dhid = da + w2 du2 + dw3x3^T(du1; w1) + dw3x3^T(dg; wd)                       wfb_du_kernel (pointwise part), wfb_dhid_kernel
//   dW_in, db_in = wgrad(dhid, x);   dx = W_in^T dhid + dy
//
// A workgroup of the four plane kernels owns a run of 4 x 4 pixel tiles of ONE channel plane (grid: run, channel, image), so the
// per-channel parameters are uniform and a channel's sums leave as one slab per workgroup, added in a fixed order afterwards: no
// float atomics, two runs give the same bits.  Widths that are no multiple of 4 take the scalar row paths of dwgate_kernel.
#include <vector>
#include "rf_grad.h"

namespace rf {

namespace {

constexpr int kBlk = 256;
constexpr int kMaxRuns = 32;      // workgroups per channel plane, at most

// gelu(v) and gelu'(v), exact erf form (gelu_exact of rf_wfb.hip)
__device__ __forceinline__ void gelu_pair(float v, float* f, float* df) {
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
    *f = v * cdf;
    *df = fmaf(v * 0.39894228040143267794f, expf(-0.5f * v * v), cdf);
}

// columns x0 - 1 .. x0 + 4 of row y of a plane, zero outside it
__device__ __forceinline__ void load_row6(const float* __restrict__ plane, int y, int x0, int h, int w, int vec, float (&v)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = 0.f;
    if (y >= 0 && y < h) {
        const float* row = plane + (size_t)y * w;
        if (vec) {
            const float4 t = *reinterpret_cast<const float4*>(row + x0);
            v[1] = t.x; v[2] = t.y; v[3] = t.z; v[4] = t.w;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) v[1 + p] = x0 + p < w ? row[x0 + p] : 0.f;
        }
        v[0] = x0 > 0 ? row[x0 - 1] : 0.f;
        v[5] = x0 + 4 < w ? row[x0 + 4] : 0.f;
    }
}

// columns x0 .. x0 + 3 of row y < h, zero past the row's end
__device__ __forceinline__ void load_row4(const float* __restrict__ plane, int y, int x0, int w, int vec, float (&v)[4]) {
    const float* row = plane + (size_t)y * w;
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(row + x0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = x0 + p < w ? row[x0 + p] : 0.f;
    }
}

__device__ __forceinline__ void store_row4(float* __restrict__ plane, int y, int x0, int w, int vec, const float (&v)[4]) {
    float* row = plane + (size_t)y * w;
    if (vec) {
        *reinterpret_cast<float4*>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (x0 + p < w) row[x0 + p] = v[p];
    }
}

// the tiles [lo, hi) of workgroup blockIdx.x among the plane's `tiles`
__device__ __forceinline__ void tile_run(int tiles, int nblk, int* lo, int* hi) {
    const int per = (tiles + nblk - 1) / nblk;
    *lo = blockIdx.x * per;
    *hi = *lo + per < tiles ? *lo + per : tiles;
}

// ---- statistics.  piv[c], piv[C + c] = u1, u2 of channel c at the middle pixel of image 0
__global__ void __launch_bounds__(kBlk) wfb_pivot_kernel(const float* __restrict__ hid, const float* __restrict__ w1, const float* __restrict__ w2,
                                                         float* __restrict__ piv, int C, int h, int w) {
    const int c = blockIdx.x * kBlk + threadIdx.x;
    if (c >= C) return;
    const float* plane = hid + (size_t)c * h * w;
    const int y = h / 2, x = w / 2;
    float u = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) u = fmaf(w1[c * 9 + ky * 3 + kx], plane[(size_t)yy * w + xx], u);
        }
    piv[c] = u;
    piv[C + c] = w2[c] * plane[(size_t)y * w + x];
}

// partial[k][image * nblk + run][c], k = 0 .. 3: sum (u1 - p1), sum (u1 - p1)^2, sum (u2 - p2), sum (u2 - p2)^2 over the run's pixels
__global__ void __launch_bounds__(kBlk) wfb_stats_kernel(const float* __restrict__ hid, const float* __restrict__ w1, const float* __restrict__ w2,
                                                         const float* __restrict__ piv, float* __restrict__ partial, int C, int h, int w, int nblk,
                                                         int vec) {
    __shared__ float red[16];
    const int c = blockIdx.y, img = blockIdx.z;
    const float* plane = hid + ((size_t)img * C + c) * h * w;
    float k1[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k1[i] = w1[c * 9 + i];
    const float k2 = w2[c], p1 = piv[c], p2 = piv[C + c];
    const int wv = (w + 3) / 4, hr = (h + 3) / 4;
    int lo, hi;
    tile_run(wv * hr, nblk, &lo, &hi);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int it = lo + threadIdx.x; it < hi; it += kBlk) {
        const int x0 = (it % wv) * 4, y0 = (it / wv) * 4;
        float u[4][4], ctr[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p) u[r][p] = 0.f;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            float v[6];
            load_row6(plane, y0 + rr - 1, x0, h, w, vec, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ky = rr - r;
                if (ky >= 0 && ky < 3) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        u[r][p] = fmaf(k1[ky * 3 + 2], v[p + 2], fmaf(k1[ky * 3 + 1], v[p + 1], fmaf(k1[ky * 3], v[p], u[r][p])));
                        if (ky == 1) ctr[r][p] = v[p + 1];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (y0 + r < h && x0 + p < w) {
                    const float d1 = u[r][p] - p1, d2 = k2 * ctr[r][p] - p2;
                    s[0] += d1;
                    s[1] = fmaf(d1, d1, s[1]);
                    s[2] += d2;
                    s[3] = fmaf(d2, d2, s[3]);
                }
    }
    block_sums<4>(s, red);
    if (threadIdx.x == 0) {
        const size_t nrows = (size_t)gridDim.z * nblk, row = (size_t)img * nblk + blockIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) partial[(k * nrows + row) * C + c] = s[k];
    }
}

// Per channel: the slabs added in order (in double: the last step of the variance is a difference), stats = [mu1 | v1 | mu2 | v2];
// the fold into dwgate_kernel's first filter, wa [C][9] and ba [C] (wa == nullptr: none); nn.BatchNorm2d's update of the running
// statistics, with the UNBIASED variance (rm1 == nullptr: none)
struct StatsFinish {
    const float *partial, *piv;
    const float *w1, *w2, *g1, *b1, *g2, *b2;
    float *stats, *wa, *ba, *rm1, *rv1, *rm2, *rv2;
    int nrows, C;
    double N;
    float eps, momentum;
};

__global__ void __launch_bounds__(kBlk) wfb_stats_finish_kernel(StatsFinish q) {
    const int c = blockIdx.x * kBlk + threadIdx.x, C = q.C;
    if (c >= C) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int row = 0; row < q.nrows; ++row)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += (double)q.partial[((size_t)k * q.nrows + row) * C + c];
    const double m1 = s[0] / q.N, m2 = s[2] / q.N;
    double var1 = s[1] / q.N - m1 * m1, var2 = s[3] / q.N - m2 * m2;
    var1 = var1 > 0.0 ? var1 : 0.0;
    var2 = var2 > 0.0 ? var2 : 0.0;
    const float mu1 = (float)((double)q.piv[c] + m1), mu2 = (float)((double)q.piv[C + c] + m2), v1 = (float)var1, v2 = (float)var2;
    q.stats[c] = mu1;
    q.stats[C + c] = v1;
    q.stats[2 * C + c] = mu2;
    q.stats[3 * C + c] = v2;
    if (q.wa) {
        const float k1 = q.g1[c] / sqrtf(v1 + q.eps), k2 = q.g2[c] / sqrtf(v2 + q.eps);
#pragma unroll
        for (int i = 0; i < 9; ++i) q.wa[c * 9 + i] = i == 4 ? fmaf(k1, q.w1[c * 9 + 4], fmaf(k2, q.w2[c], 1.0f)) : k1 * q.w1[c * 9 + i];
        q.ba[c] = (q.b1[c] - mu1 * k1) + (q.b2[c] - mu2 * k2);
    }
    if (q.rm1) {
        const float keep = 1.0f - q.momentum, unb = (float)(q.N / (q.N - 1.0));
        q.rm1[c] = keep * q.rm1[c] + q.momentum * mu1;
        q.rv1[c] = keep * q.rv1[c] + q.momentum * (v1 * unb);
        q.rm2[c] = keep * q.rm2[c] + q.momentum * mu2;
        q.rv2[c] = keep * q.rv2[c] + q.momentum * (v2 * unb);
    }
}

// ---- the gate adjoint: a, g, u1 recomputed from hid; m, da, dg, uh1 written; partial[k][image * nblk + run][c], k = 0 .. 2:
// sum da, sum da uh1, sum da uh2
struct GateAdjoint {
    const float *hid, *dm;
    float *m, *da, *dg, *uh1, *partial;
    const float *w1, *w2, *wd, *bd, *g1, *b1, *g2, *b2;
    const float *mu1, *v1, *mu2, *v2;      // batch statistics (training) or the running ones (eval)
    float eps;
    int C, h, w, nblk, vec;
};

__global__ void __launch_bounds__(kBlk) wfb_gate_adjoint_kernel(GateAdjoint q) {
    __shared__ float red[12];
    const int c = blockIdx.y, img = blockIdx.z, h = q.h, w = q.w, vec = q.vec;
    const size_t off = ((size_t)img * q.C + c) * h * w;
    const float* plane = q.hid + off;
    float k1[9], kd[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { k1[i] = q.w1[c * 9 + i]; kd[i] = q.wd[c * 9 + i]; }
    const float k2 = q.w2[c], bd = q.bd[c], g1 = q.g1[c], g2 = q.g2[c], bsum = q.b1[c] + q.b2[c];
    const float mu1 = q.mu1[c], mu2 = q.mu2[c], rs1 = 1.0f / sqrtf(q.v1[c] + q.eps), rs2 = 1.0f / sqrtf(q.v2[c] + q.eps);
    const int wv = (w + 3) / 4, hr = (h + 3) / 4;
    int lo, hi;
    tile_run(wv * hr, q.nblk, &lo, &hi);
    float s[3] = {0.f, 0.f, 0.f};
    for (int it = lo + threadIdx.x; it < hi; it += kBlk) {
        const int x0 = (it % wv) * 4, y0 = (it / wv) * 4;
        float u[4][4], g[4][4], ctr[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p) { u[r][p] = 0.f; g[r][p] = bd; }
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            float v[6];
            load_row6(plane, y0 + rr - 1, x0, h, w, vec, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ky = rr - r;
                if (ky >= 0 && ky < 3) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        u[r][p] = fmaf(k1[ky * 3 + 2], v[p + 2], fmaf(k1[ky * 3 + 1], v[p + 1], fmaf(k1[ky * 3], v[p], u[r][p])));
                        g[r][p] = fmaf(kd[ky * 3 + 2], v[p + 2], fmaf(kd[ky * 3 + 1], v[p + 1], fmaf(kd[ky * 3], v[p], g[r][p])));
                        if (ky == 1) ctr[r][p] = v[p + 1];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + r;
            if (y >= h) continue;
            float dm[4], mo[4], da[4], dg[4], uh[4];
            load_row4(q.dm + off, y, x0, w, vec, dm);      // zero past the row's end: those lanes add nothing to the sums
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float uh1 = (u[r][p] - mu1) * rs1, uh2 = (k2 * ctr[r][p] - mu2) * rs2;
                const float a = ctr[r][p] + fmaf(g1, uh1, fmaf(g2, uh2, bsum)), gg = g[r][p];
                float fa, dfa, fg, dfg;
                gelu_pair(a, &fa, &dfa);
                gelu_pair(gg, &fg, &dfg);
                mo[p] = fg * a + fa * gg;
                da[p] = dm[p] * fmaf(dfa, gg, fg);
                dg[p] = dm[p] * fmaf(dfg, a, fa);
                uh[p] = uh1;
                s[0] += da[p];
                s[1] = fmaf(da[p], uh1, s[1]);
                s[2] = fmaf(da[p], uh2, s[2]);
            }
            store_row4(q.m + off, y, x0, w, vec, mo);
            store_row4(q.da + off, y, x0, w, vec, da);
            store_row4(q.dg + off, y, x0, w, vec, dg);
            store_row4(q.uh1 + off, y, x0, w, vec, uh);
        }
    }
    block_sums<3>(s, red);
    if (threadIdx.x == 0) {
        const size_t nrows = (size_t)gridDim.z * q.nblk, row = (size_t)img * q.nblk + blockIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) q.partial[(k * nrows + row) * q.C + c] = s[k];
    }
}

// ---- du1 (over uh1), t = da + w2 du2 (over da), partial[image * nblk + run][c] = sum du2 hid.  sums = [sum da | sum da uh1 | sum da uh2]
struct DuArgs {
    const float* hid;
    float *da, *uh1, *partial;
    const float *sums, *w2, *g1, *g2, *v1, *mu2, *v2;
    float eps, inv_n;      // inv_n = 1 / N in training mode, 0 in eval mode: the statistics are constants there
    int C, P, nblk;
};

template <int V>
__global__ void __launch_bounds__(kBlk) wfb_du_kernel(DuArgs q) {
    __shared__ float red[4];
    const int c = blockIdx.y, img = blockIdx.z, C = q.C;
    const size_t off = ((size_t)img * C + c) * q.P;
    const float* hid = q.hid + off;
    float *da = q.da + off, *uh1 = q.uh1 + off;
    const float k2w = q.w2[c], mu2 = q.mu2[c], rs2 = 1.0f / sqrtf(q.v2[c] + q.eps);
    const float k1 = q.g1[c] / sqrtf(q.v1[c] + q.eps), k2 = q.g2[c] * rs2;
    const float c0 = q.sums[c] * q.inv_n, c1 = q.sums[C + c] * q.inv_n, c2 = q.sums[2 * C + c] * q.inv_n;
    const int n = q.P / V, per = (n + q.nblk - 1) / q.nblk, lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    float s[1] = {0.f};
    for (int i = lo + threadIdx.x; i < hi; i += kBlk) {
        float hv[V], av[V], uv[V];
        if constexpr (V == 4) {
            const float4 a = *reinterpret_cast<const float4*>(hid + 4 * (size_t)i), b = *reinterpret_cast<const float4*>(da + 4 * (size_t)i),
                         d = *reinterpret_cast<const float4*>(uh1 + 4 * (size_t)i);
            hv[0] = a.x; hv[1] = a.y; hv[2] = a.z; hv[3] = a.w;
            av[0] = b.x; av[1] = b.y; av[2] = b.z; av[3] = b.w;
            uv[0] = d.x; uv[1] = d.y; uv[2] = d.z; uv[3] = d.w;
        } else {
            hv[0] = hid[i]; av[0] = da[i]; uv[0] = uh1[i];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float uh2 = (k2w * hv[e] - mu2) * rs2;
            const float du1 = k1 * (av[e] - c0 - uv[e] * c1), du2 = k2 * (av[e] - c0 - uh2 * c2);
            s[0] = fmaf(du2, hv[e], s[0]);
            uv[e] = du1;
            av[e] = fmaf(k2w, du2, av[e]);
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(da + 4 * (size_t)i) = make_float4(av[0], av[1], av[2], av[3]);
            *reinterpret_cast<float4*>(uh1 + 4 * (size_t)i) = make_float4(uv[0], uv[1], uv[2], uv[3]);
        } else {
            da[i] = av[0]; uh1[i] = uv[0];
        }
    }
    block_sums<1>(s, red);
    if (threadIdx.x == 0) q.partial[((size_t)img * q.nblk + blockIdx.x) * C + c] = s[0];
}

// ---- dhid = t + dw3x3^T(du1; w1) + dw3x3^T(dg; wd): the transposed stencils are the forward's with the taps flipped
__global__ void __launch_bounds__(kBlk) wfb_dhid_kernel(const float* __restrict__ t, const float* __restrict__ du1, const float* __restrict__ dg,
                                                        const float* __restrict__ w1, const float* __restrict__ wd, float* __restrict__ dhid, int C,
                                                        int h, int w, int nblk, int vec) {
    const int c = blockIdx.y, img = blockIdx.z;
    const size_t off = ((size_t)img * C + c) * h * w;
    float ka[9], kb[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { ka[i] = w1[c * 9 + 8 - i]; kb[i] = wd[c * 9 + 8 - i]; }
    const int wv = (w + 3) / 4, hr = (h + 3) / 4;
    int lo, hi;
    tile_run(wv * hr, nblk, &lo, &hi);
    for (int it = lo + threadIdx.x; it < hi; it += kBlk) {
        const int x0 = (it % wv) * 4, y0 = (it / wv) * 4;
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[r][p] = 0.f;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            float va[6], vb[6];
            load_row6(du1 + off, y0 + rr - 1, x0, h, w, vec, va);
            load_row6(dg + off, y0 + rr - 1, x0, h, w, vec, vb);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ky = rr - r;
                if (ky >= 0 && ky < 3) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        acc[r][p] = fmaf(ka[ky * 3 + 2], va[p + 2], fmaf(ka[ky * 3 + 1], va[p + 1], fmaf(ka[ky * 3], va[p], acc[r][p])));
                        acc[r][p] = fmaf(kb[ky * 3 + 2], vb[p + 2], fmaf(kb[ky * 3 + 1], vb[p + 1], fmaf(kb[ky * 3], vb[p], acc[r][p])));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + r;
            if (y >= h) continue;
            float tv[4];
            load_row4(t + off, y, x0, w, vec, tv);
#pragma unroll
            for (int p = 0; p < 4; ++p) tv[p] += acc[r][p];
            store_row4(dhid + off, y, x0, w, vec, tv);
        }
    }
}

// ---- host side
// workgroups per channel plane: one per 256 tiles of 4 x 4 pixels, at most kMaxRuns
int wfb_ffn_nblk(int h, int w) {
    const long long tiles = (long long)cdiv(h, 4) * cdiv(w, 4);
    const long long n = (tiles + kBlk - 1) / kBlk;
    return (int)(n > kMaxRuns ? kMaxRuns : n);
}

// the 12 parameters, then the 4 buffers, as ops.wfb_ff_param_shapes orders them
enum { kWin, kBin, kWd, kBd, kWout, kBout, kW1, kG1, kB1, kW2, kG2, kB2, kRm1, kRv1, kRm2, kRv2, kTensors };
constexpr int kParams = 12;

}  // namespace

// rf_grad.h declares this one: the block schedule of rf_wmb_block_bwd.hip checks ffn's tensors with it
size_t wfb_prm_floats(int i, int dim, int hidden) {
    const size_t D = dim, C = hidden;
    switch (i) {
        case kWin: case kWout: return D * C;
        case kBout: return D;
        case kWd: case kW1: return C * 9;
        default: return C;
    }
}

namespace {

int wfb_check_geometry(const char* who, int B, int dim, int hidden, int h, int w, bool training) {
    RF_CHECK_ARG(B > 0 && dim > 0 && hidden > 0 && h > 0 && w > 0, "%s: sizes must be positive (B %d, dim %d, hidden %d, %d x %d)", who, B, dim,
                 hidden, h, w);
    RF_CHECK_ARG(dim % 4 == 0 && hidden % 4 == 0, "%s: dim %d and hidden %d must be multiples of 4", who, dim, hidden);
    RF_CHECK_ARG(B <= 65535 && hidden <= 65535 && dim <= 65535 && (double)h * w < 6.0e7, "%s: B %d, dim %d, hidden %d or the plane %d x %d is too large",
                 who, B, dim, hidden, h, w);
    RF_CHECK_ARG(!training || (long long)B * h * w >= 2, "%s: batch statistics need more than one value per channel (B h w = %lld)", who,
                 (long long)B * h * w);
    return RF_OK;
}

size_t wfb_wpack_floats(int dim, int hidden) {
    const size_t a = packed1x1_floats(dim, hidden), b = packed1x1_floats(hidden, dim);
    return a > b ? a : b;
}

int launch_wfb_stats(const float* hid, const float* const* prm, float* piv, float* partial, float* stats, float* wa, float* ba, float* const* running,
                     int B, int C, int h, int w, float eps, float momentum, hipStream_t st) {
    const int nblk = wfb_ffn_nblk(h, w), vec = w % 4 == 0 && aligned16(hid);
    const double el = (double)B * C * h * w;
    ProfScope prof(st, "wfb_stats(3 kernels)", 26.0 * el, 4.0 * el);
    wfb_pivot_kernel<<<cdiv(C, kBlk), kBlk, 0, st>>>(hid, prm[kW1], prm[kW2], piv, C, h, w);
    wfb_stats_kernel<<<dim3((unsigned)nblk, (unsigned)C, (unsigned)B), kBlk, 0, st>>>(hid, prm[kW1], prm[kW2], piv, partial, C, h, w, nblk, vec);
    StatsFinish q{partial, piv, prm[kW1], prm[kW2], prm[kG1], prm[kB1], prm[kG2], prm[kB2], stats, wa, ba,
                  running ? running[0] : nullptr, running ? running[1] : nullptr, running ? running[2] : nullptr, running ? running[3] : nullptr,
                  B * nblk, C, (double)B * h * w, eps, momentum};
    wfb_stats_finish_kernel<<<cdiv(C, kBlk), kBlk, 0, st>>>(q);
    return check_launch("wfb_stats");
}

// ---- forward
struct WfbFwdPlan { size_t hid, gated, wpack, piv, partial, wa, ba, total; };

int wfb_fwd_plan(const char* who, int B, int dim, int hidden, int h, int w, WfbFwdPlan* p) {
    RF_TRY(wfb_check_geometry(who, B, dim, hidden, h, w, true));
    Bump b;
    const size_t U = (size_t)B * hidden * h * w, rows = (size_t)B * wfb_ffn_nblk(h, w);
    p->hid = b.off(U);
    p->gated = b.off(U);
    p->wpack = b.off(wfb_wpack_floats(dim, hidden));
    p->piv = b.off((size_t)2 * hidden);
    p->partial = b.off(4 * rows * hidden);
    p->wa = b.off((size_t)9 * hidden);
    p->ba = b.off((size_t)hidden);
    p->total = b.used;
    return RF_OK;
}

// ---- backward
struct WfbBwdPlan { size_t hid, m, dm, da, dg, uh1, dhid, wpack, piv, stats, sums, partial, wpart, wpart_cap, total; };

int wfb_bwd_plan(const char* who, int B, int dim, int hidden, int h, int w, bool training, WfbBwdPlan* p) {
    RF_TRY(wfb_check_geometry(who, B, dim, hidden, h, w, training));
    Bump b;
    const int P = h * w;
    const size_t U = (size_t)B * hidden * P, rows = (size_t)B * wfb_ffn_nblk(h, w);
    p->hid = b.off(U); p->m = b.off(U); p->dm = b.off(U); p->da = b.off(U); p->dg = b.off(U); p->uh1 = b.off(U); p->dhid = b.off(U);
    p->wpack = b.off(wfb_wpack_floats(dim, hidden));
    p->piv = b.off((size_t)2 * hidden);
    p->stats = b.off((size_t)4 * hidden);
    p->sums = b.off((size_t)3 * hidden);
    p->partial = b.off(4 * rows * hidden);
    size_t cap = 0;
    for (const size_t f : {wgrad1x1_partial_floats(B, dim, hidden, P, true), wgrad1x1_partial_floats(B, hidden, dim, P, true),
                           dw_wgrad_partial_floats(B, hidden, P)})
        cap = cap > f ? cap : f;
    p->wpart_cap = cap;
    p->wpart = b.off(cap);
    p->total = b.used;
    return RF_OK;
}

int run_wfb_backward(const WfbBwdPlan& p, const float* x, const float* dy, float* dx, const float* const* prm, float* const* grd, float* ws, int B,
                     int dim, int C, int h, int w, bool training, float eps, int acc, hipStream_t st) {
    const int P = h * w, nblk = wfb_ffn_nblk(h, w), rows = B * nblk, vec = w % 4 == 0;
    const double el = (double)B * C * P;
    float *hid = ws + p.hid, *m = ws + p.m, *dm = ws + p.dm, *da = ws + p.da, *dg = ws + p.dg, *uh1 = ws + p.uh1, *dhid = ws + p.dhid;
    float *wpack = ws + p.wpack, *stats = ws + p.stats, *sums = ws + p.sums, *partial = ws + p.partial;
    const Wgrad wg{"rf_wfb_ffn_backward", ws + p.wpart, p.wpart_cap, B, P, acc, st};
    const dim3 grid((unsigned)nblk, (unsigned)C, (unsigned)B);
    RF_TRY(conv1x1_raw(x, hid, prm[kWin], prm[kBin], nullptr, wpack, B, dim, C, P, 0, st));
    const float *mu1 = prm[kRm1], *v1 = prm[kRv1], *mu2 = prm[kRm2], *v2 = prm[kRv2];
    if (training) {
        RF_TRY(launch_wfb_stats(hid, prm, ws + p.piv, partial, stats, nullptr, nullptr, nullptr, B, C, h, w, eps, 0.f, st));
        mu1 = stats; v1 = stats + C; mu2 = stats + 2 * C; v2 = stats + 3 * C;
    }
    // project_out
    RF_TRY(dgrad1x1(dy, dim, prm[kWout], C, wpack, nullptr, dm, B, P, st));
    {
        ProfScope prof(st, "wfb_gate_adjoint_kernel", 120.0 * el, 24.0 * el);
        wfb_gate_adjoint_kernel<<<grid, kBlk, 0, st>>>(GateAdjoint{hid, dm, m, da, dg, uh1, partial, prm[kW1], prm[kW2], prm[kWd], prm[kBd], prm[kG1],
                                                                  prm[kB1], prm[kG2], prm[kB2], mu1, v1, mu2, v2, eps, C, h, w, nblk, vec});
        RF_TRY(check_launch("wfb_gate_adjoint"));
    }
    RF_TRY(wgrad1x1(wg, dy, dim, m, C, grd[kWout], grd[kBout]));
    // the BatchNorm affines: sums = [sum da | sum da uh1 | sum da uh2]
    const size_t slab = (size_t)rows * C;
    for (int k = 0; k < 3; ++k) RF_TRY(reduce_rows(partial + k * slab, sums + k * C, rows, (size_t)C, 0, st));
    RF_TRY(reduce_rows(partial, grd[kB1], rows, (size_t)C, acc, st));
    RF_TRY(reduce_rows(partial, grd[kB2], rows, (size_t)C, acc, st));
    RF_TRY(reduce_rows(partial + slab, grd[kG1], rows, (size_t)C, acc, st));
    RF_TRY(reduce_rows(partial + 2 * slab, grd[kG2], rows, (size_t)C, acc, st));
    // through the normalisation; d rep_conv2.c.weight
    {
        const DuArgs q{hid, da, uh1, partial, sums, prm[kW2], prm[kG1], prm[kG2], v1, mu2, v2, eps, training ? (float)(1.0 / ((double)B * P)) : 0.f,
                       C, P, nblk};
        ProfScope prof(st, "wfb_du_kernel", 14.0 * el, 20.0 * el);
        if (P % 4 == 0) wfb_du_kernel<4><<<grid, kBlk, 0, st>>>(q);
        else wfb_du_kernel<1><<<grid, kBlk, 0, st>>>(q);
        RF_TRY(check_launch("wfb_du"));
    }
    RF_TRY(reduce_rows(partial, grd[kW2], rows, (size_t)C, acc, st));
    float *du1 = uh1, *t = da;
    RF_TRY(launch_dw_wgrad(hid, du1, grd[kW1], nullptr, ws + p.wpart, B, C, h, w, acc, st));
    RF_TRY(launch_dw_wgrad(hid, dg, grd[kWd], grd[kBd], ws + p.wpart, B, C, h, w, acc, st));
    {
        ProfScope prof(st, "wfb_dhid_kernel", 37.0 * el, 16.0 * el);
        wfb_dhid_kernel<<<grid, kBlk, 0, st>>>(t, du1, dg, prm[kW1], prm[kWd], dhid, C, h, w, nblk, vec);
        RF_TRY(check_launch("wfb_dhid"));
    }
    // project_in and the identity
    RF_TRY(wgrad1x1(wg, dhid, C, x, dim, grd[kWin], grd[kBin]));
    return dgrad1x1(dhid, C, prm[kWin], dim, wpack, dy, dx, B, P, st);
}

}  // namespace
}  // namespace rf

using namespace rf;

extern "C" {

int rf_wfb_ffn_nblk(int h, int w) {
    RF_CHECK_ARG(h > 0 && w > 0, "rf_wfb_ffn_nblk: %d x %d", h, w);
    return wfb_ffn_nblk(h, w);
}

long long rf_wfb_ffn_train_workspace_bytes(int B, int dim, int hidden, int h, int w) {
    WfbFwdPlan p;
    const int rc = wfb_fwd_plan("rf_wfb_ffn_train_workspace_bytes", B, dim, hidden, h, w, &p);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_wfb_ffn_train_forward(const float* in, float* out, float* const* prm, float* batch_stats, void* workspace, size_t workspace_bytes, int B, int dim,
                             int hidden, int h, int w, float eps, float momentum, int update_running, void* stream) {
    const char* who = "rf_wfb_ffn_train_forward";
    WfbFwdPlan p;
    RF_TRY(wfb_fwd_plan(who, B, dim, hidden, h, w, &p));
    RF_CHECK_ARG(in && out && prm && batch_stats && workspace && aligned16(in) && aligned16(out) && aligned16(batch_stats) && aligned16(workspace),
                 "%s: in, out, prm, batch_stats and workspace must be non-null and 16-byte aligned", who);
    const size_t need = p.total * sizeof(float), plane = (size_t)B * dim * h * w * sizeof(float);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
        return RF_E_NOMEM;
    }
    for (int i = 0; i < kTensors; ++i) RF_CHECK_ARG(prm[i] != nullptr, "%s: parameter or buffer %d is null", who, i);
    // written: out, batch_stats, the workspace and (update_running) the four buffers; read: in, the parameters, the buffers otherwise
    std::vector<Span> outs{{out, plane}, {batch_stats, (size_t)4 * hidden * sizeof(float)}, {workspace, need}}, ins{{in, plane}};
    for (int i = 0; i < kTensors; ++i) (i >= kParams && update_running ? outs : ins).push_back({prm[i], wfb_prm_floats(i, dim, hidden) * sizeof(float)});
    int a, b;
    const int hit = first_alias(outs.data(), (int)outs.size(), ins.data(), (int)ins.size(), &a, &b);
    RF_CHECK_ARG(hit != 1, "%s: output %d (out, batch_stats, workspace, then the running statistics) may not alias input %d (in, then the parameters)", who,
                 a, b);
    RF_CHECK_ARG(hit != 2, "%s: outputs %d and %d (out, batch_stats, workspace, then the running statistics) may not alias each other", who, a, b);
    const hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int P = h * w;
    RF_TRY(conv1x1_raw(in, ws + p.hid, prm[kWin], prm[kBin], nullptr, ws + p.wpack, B, dim, hidden, P, 0, st));
    RF_TRY(launch_wfb_stats(ws + p.hid, prm, ws + p.piv, ws + p.partial, batch_stats, ws + p.wa, ws + p.ba, update_running ? prm + kRm1 : nullptr, B,
                            hidden, h, w, eps, momentum, st));
    RF_TRY(launch_dwgate3x3(ws + p.hid, ws + p.gated, ws + p.wa, ws + p.ba, prm[kWd], prm[kBd], B, hidden, h, w, st));
    return conv1x1_raw(ws + p.gated, out, prm[kWout], prm[kBout], in, ws + p.wpack, B, hidden, dim, P, 0, st);
}

long long rf_wfb_ffn_backward_workspace_bytes(int B, int dim, int hidden, int h, int w) {
    WfbBwdPlan p;
    const int rc = wfb_bwd_plan("rf_wfb_ffn_backward_workspace_bytes", B, dim, hidden, h, w, false, &p);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_wfb_ffn_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                        size_t workspace_bytes, int B, int dim, int hidden, int h, int w, int training, float eps, int accumulate, void* stream) {
    WfbBwdPlan p;
    RF_TRY(wfb_bwd_plan("rf_wfb_ffn_backward", B, dim, hidden, h, w, training != 0, &p));
    Span buffers[kTensors - kParams];
    if (prm)
        for (int i = kParams; i < kTensors; ++i) buffers[i - kParams] = {prm[i], (size_t)hidden * sizeof(float)};
    RF_TRY(check_backward_args({"rf_wfb_ffn_backward", in, grad_out, grad_in, (size_t)B * dim * h * w * sizeof(float), prm, grad_prm, kParams, workspace,
                                workspace_bytes, p.total * sizeof(float), buffers, kTensors - kParams},
                               [=](int i) { return wfb_prm_floats(i, dim, hidden); }));
    return run_wfb_backward(p, in, grad_out, grad_in, prm, grad_prm, (float*)workspace, B, dim, hidden, h, w, training != 0, eps, accumulate,
                            (hipStream_t)stream);
}

}  // extern "C"
