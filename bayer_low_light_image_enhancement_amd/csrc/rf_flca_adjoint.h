// Device code the FLCA kernels share (internal; device code only, no host declarations):
//   * the steps of the MFMA tap contraction of a spatial-gate adjoint, G[c][tap] = sum_p ds[c][p] plane[p + tap], for
//     flca_bwd_fused_kernel (rf_flca_bwd.hip, 4 guidance planes) and pyr_spatial_bwd_vec_kernel (rf_flca_pyramid_bwd.hip, 2): the
//     B operand, a row of the guidance neighbourhood, the fold of the accumulator tiles over the four waves.  The kernels keep
//     their own prologue, gate arithmetic and partial layout.  The helpers take the lane's coordinates (r, kq, wave, tdy, tdx), the
//     row test of neighbour_row and the fold's destination (a by-value lambda) from the kernel: hipcc simplifies a helper on its
//     own before it inlines it, and in this form neighbour_row compiles to the code of its loop written out in place and
//     fold_tap_tiles to that code less one dead scalar instruction; with the row test inside, or a by-reference lambda, the
//     kernels' whole schedule moved.  tap_operand moves register numbers in every form tried;
//   * the squeeze-excite MLP of one image, mean -> relu hidden -> sigmoid gate, and its adjoint, for flca_se_kernel (rf_flca.hip),
//     flca_se_bwd_kernel (rf_flca_bwd.hip) and pyr_se_kernel (rf_flca_pyramid.hip).  Every fmaf chain and every sum runs in one
//     fixed order: two runs give the same bits.
#pragma once
#include "rf_common.h"

namespace rf {
namespace {

// ---- tap contraction.  Lane (r = lane & 15, kq = lane >> 4) of wave `wave` owns channel 16 ti + r and 4 adjacent pixels at (y, x).

// B operand: tap (tdy, tdx) = tap r of each of NPL adjacent planes (P floats apart) at the lane's 4 pixels; zero outside the
// plane, for B rows 9 .. 15 and where the lane has no pixels (!ok)
template <int NPL>
__device__ __forceinline__ void tap_operand(const float* gpl, int P, int h, int w, int y, int x, int r, int tdy, int tdx, bool ok, float (&bv)[NPL][4]) {
    const int yy = y + tdy;
    const bool rowok = ok && r < 9 && yy >= 0 && yy < h;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int xx = x + m + tdx;
        const bool in = rowok && xx >= 0 && xx < w;
        const size_t off = in ? (size_t)yy * w + xx : 0;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) { const float v = gpl[(size_t)pl * P + off]; bv[pl][m] = in ? v : 0.f; }
    }
}

// Row yy of the 3 x 6 neighbourhood of the lane's 4 pixels in each plane: nb[pl][0 .. 5] = columns x - 1 .. x + 4, zero outside
// the plane (x % 4 == 0 and w % 4 == 0: the middle four are one 16-byte load).  rok = 0 <= yy < h, evaluated by the caller (file header)
template <int NPL>
__device__ __forceinline__ void neighbour_row(const float* gpl, int P, int w, int x, int yy, bool rok, float (&nb)[NPL][6]) {
    const size_t rowoff = (size_t)(rok ? yy : 0) * w + x;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
        const float* row = gpl + (size_t)pl * P + rowoff;
        const float4 t = ld4(row);
        const float lft = row[x > 0 ? -1 : 0], rgt = row[x + 4 < w ? 4 : 0];
        nb[pl][0] = (rok && x > 0) ? lft : 0.f;
        nb[pl][1] = rok ? t.x : 0.f; nb[pl][2] = rok ? t.y : 0.f; nb[pl][3] = rok ? t.z : 0.f; nb[pl][4] = rok ? t.w : 0.f;
        nb[pl][5] = (rok && x + 4 < w) ? rgt : 0.f;
    }
}

// The NT accumulator tiles [16 channels][16 taps] of the four waves added in wave order ((0 + 1) + 2) + 3 through red; thread
// (i = tid >> 4, jj = tid & 15) writes tap jj < 9 of channel 16 ti + i < C of tile t to *dst(t, channel, jj)
template <int NT, typename Dst>
__device__ __forceinline__ void fold_tap_tiles(const f32x4 (&acc)[NT], float (&red)[4][16][17], int wave, int kq, int r, int ti, int C, Dst dst) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][4 * kq + q][r] = acc[t][q];
        __syncthreads();
        const int i = threadIdx.x >> 4, jj = threadIdx.x & 15;
        const int gi = 16 * ti + i;
        if (gi < C && jj < 9) *dst(t, gi, jj) = ((red[0][i][jj] + red[1][i][jj]) + red[2][i][jj]) + red[3][i][jj];
    }
}

// ---- squeeze-excite of one image, one workgroup of 256 threads; mean, ds3 [C <= 512] and hv, dh [hid <= 64] are LDS.

// Column sums of image b's table in tables [B][nblk][C]: store(c, sum of column c) for every c < C.  cw channels x nsl row slices
// per pass, all 256 threads busy, 8 loads in flight per thread; a slice adds its rows in order, the slices are added in order.
// part: 256 floats of LDS.  (Handing in the image's table as a pointer costs flca_se_kernel 14 VGPRs.)
template <typename Store>
__device__ __forceinline__ void se_column_sums(const float* __restrict__ tables, size_t b, int nblk, int C, float* part, Store store) {
    const int cw = C < 256 ? C : 256, nsl = 256 / cw;
    for (int c0 = 0; c0 < C; c0 += cw) {
        const int c = c0 + threadIdx.x % cw, sl = threadIdx.x / cw;
        float s = 0.f;
        if (sl < nsl && c < C) {
            const float* src = tables + b * nblk * C + c;
            int k = sl;
            for (; k + 7 * nsl < nblk; k += 8 * nsl) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = src[(size_t)(k + u * nsl) * C];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += t[u];
            }
            for (; k < nblk; k += nsl) s += src[(size_t)k * C];
        }
        part[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x < cw && c0 + threadIdx.x < C) {
            float t = 0.f;
            for (int q = 0; q < nsl; ++q) t += part[q * cw + threadIdx.x];
            store(c0 + threadIdx.x, t);
        }
        __syncthreads();
    }
}

// hv = relu(W1 mean + b1), visible to the workgroup on return
__device__ __forceinline__ void se_hidden(const float* __restrict__ w1, const float* __restrict__ b1, const float* mean, float* hv, int C, int hid) {
    for (int m = threadIdx.x; m < hid; m += 256) {
        float s = b1[m];
        for (int c = 0; c < C; ++c) s = fmaf(w1[m * C + c], mean[c], s);
        hv[m] = fmaxf(s, 0.f);
    }
    __syncthreads();
}

// the gate of channel c: sigmoid(W3 hv + b3)
__device__ __forceinline__ float se_gate(const float* __restrict__ w3, const float* __restrict__ b3, const float* hv, int c, int hid) {
    float s = b3[c];
    for (int m = 0; m < hid; ++m) s = fmaf(w3[c * hid + m], hv[m], s);
    return sigm(s);
}

// The adjoint from ds3[c] = dch[c] ch[c] (1 - ch[c]) (written by the caller, no barrier yet):  dh = (W3^T ds3) [hv > 0], the image's
// share of the gradients of se.1.weight [hid][C], se.1.bias, se.3.weight [C][hid], se.3.bias, and dmP = W1^T dh / P
__device__ __forceinline__ void se_adjoint(const float* __restrict__ w1, const float* __restrict__ w3, const float* mean, const float* hv, const float* ds3,
                                           float* dh, float* __restrict__ g_w1, float* __restrict__ g_b1, float* __restrict__ g_w3,
                                           float* __restrict__ g_b3, float* __restrict__ dmP, int C, int hid, int P) {
    __syncthreads();
    for (int m = threadIdx.x; m < hid; m += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(w3[c * hid + m], ds3[c], s);
        dh[m] = hv[m] > 0.f ? s : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < hid * C; e += 256) g_w1[e] = dh[e / C] * mean[e % C];
    for (int m = threadIdx.x; m < hid; m += 256) g_b1[m] = dh[m];
    for (int e = threadIdx.x; e < C * hid; e += 256) g_w3[e] = ds3[e / hid] * hv[e % hid];
    for (int c = threadIdx.x; c < C; c += 256) {
        g_b3[c] = ds3[c];
        float s = 0.f;
        for (int m = 0; m < hid; ++m) s = fmaf(w1[m * C + c], dh[m], s);
        dmP[c] = s / (float)P;
    }
}

}  // namespace
}  // namespace rf
