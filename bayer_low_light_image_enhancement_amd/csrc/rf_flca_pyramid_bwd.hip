// Adjoint of FLCA_Pyramid (rf_flca_pyramid.hip) and of the multi-level output corrections (rf_multilvl.hip, ml_tail).
//
// Block.  Forward, s = 0 .. L, x_0 = feat:
//   m = x_s S_s;  t = relu(W0 m + b0);  r = W2 t + b2;  x_{s+1} = x_s + 0.2 tanh(r);   z = x_{L+1} ch,  ch = squeeze-excite(mean_p x_{L+1})
//   S_s = g0 sigmoid(conv3(y_low_s; w_low_s)) + g1 tanh(conv3(y_high_s; w_high_s)),  (g0, g1) = sigmoid(freq_gate_head_s(means))   s < L
//   S_L = gamma sigmoid(conv3([cr, cb]; w_chr)),  gamma = sigmoid(chroma_gate(mean sqrt(cr^2 + cb^2 + 1e-8)))
// Nothing is kept from a forward call: pyr_forward_steps recomputes x_1 .. x_{L+1} (and the guidance, which carries no gradient),
// then, with dz = dL/dz:
//   squeeze-excite   dch = sum_p dz x_{L+1} (launch_flca_dch, rf_flca_bwd.hip) -> pyr_se_kernel's adjoint -> dmean / P and the four se gradients;
//                    dx = dz ch + dmean / P (pyr_dx_kernel), kept in grad_in from here on
//   for s = L .. 0   m, t, r again (pyr_step_mtr);  dr = 0.2 (1 - tanh^2 r) dx in place of r (pyr_dtanh_kernel)
//                    dW2, db2 += wgrad1x1(dr, t);  dpre = (W2^T dr) [t > 0];  dW0, db0 += wgrad1x1(dpre, m);  dm = W0^T dpre
//                    pyr_spatial_bwd: dx += dm S_s in place; with dS = dm x_s the tap sums of the step's 18 weights per channel
//                    and the gate sums sum dS a_l, sum dS a_h per image go to per-workgroup slabs
//                    reduce_rows adds the tap slabs into the weight gradients and the gate slabs into [B][2] sums, to which
//                    pyr_gate_bwd_kernel applies the gate head's adjoint
// res_proj's gradients are the sum over the L + 1 steps: the steps add up in the workspace and the total goes to (or, with
// accumulate, is added to) the caller's tensors once, so an accumulating call adds exactly what a plain call writes.  The backward
// recomputes its gates with expf / tanhf, not the forward's fast forms.
//
// pyr_spatial_bwd has two forms over one slab layout and one prologue (PyrSpLane).  w % 4 == 0: the MFMA tap contraction of
// rf_flca_adjoint.h, which flca_bwd_fused_kernel (rf_flca_bwd.hip) runs on four planes -- a lane owns one channel of a 16-channel
// tile and 4 pixels, recomputes the gate there from the two guidance planes with the channel's 18 weights in registers, and feeds
// the two d(conv output) values into 16x16x4 MFMAs whose B rows are the taps.  Any other width:
// a thread owns one channel and every 16th pixel of the slab and keeps the 18 tap sums in registers.  dm, x_s and dx are read
// once and dx written once.  Slabs are pixel ranges of one image (pyr_slabs).
//
// Tail.  ml_tail is affine in the image: out' = out + 0.12 (in_mean - mean_p out), then out'' = out' + 0.03 (up(LL2) - luma(out')) on
// all three channels.  Its adjoint, last map first, with G = sum_c g_c and w = (0.299, 0.587, 0.114):
//   g1_c = g_c - 0.03 w_c G;   grad_c = g1_c - 0.12 mean_p(g1_c)
// ml_tail_bwd_sums_kernel leaves per-block sums of g1_c, ml_tail_bwd_apply_kernel adds them in block order and applies.
// No float atomics anywhere: two calls give the same bits.
#include "rf_flca_adjoint.h"
#include "rf_grad.h"

namespace rf {

namespace {

constexpr int kMeans = 8;            // floats per image in ml_means's table (rf_multilvl.hip): 2 l, 2 l + 1 the level's, 6 the chroma magnitude's
constexpr int kTailSumBlocks = 256;  // most workgroups per image of ml_tail_bwd_sums_kernel (= partial sums per channel)
constexpr int kTailApplyBlocks = 1024;   // ... of ml_tail_bwd_apply_kernel

// dx = dz ch[b][c] + dmP[b][c];  PX = 4: P % 4 == 0, 16 bytes per lane
template <int PX>
__global__ void __launch_bounds__(256) pyr_dx_kernel(const float* __restrict__ dz, const float* __restrict__ ch, const float* __restrict__ dmP,
                                                     float* __restrict__ dx, int P, size_t n) {
    const size_t i = (blockIdx.x * 256ull + threadIdx.x) * PX;
    if (i >= n) return;
    const size_t bc = i / P;
    const float s = ch[bc], d = dmP[bc];
    if constexpr (PX == 4) {
        const float4 v = ld4(dz + i);
        *reinterpret_cast<float4*>(dx + i) = make_float4(fmaf(v.x, s, d), fmaf(v.y, s, d), fmaf(v.z, s, d), fmaf(v.w, s, d));
    } else {
        dx[i] = fmaf(dz[i], s, d);
    }
}

// r <- 0.2 (1 - tanh^2 r) dx
template <int PX>
__global__ void __launch_bounds__(256) pyr_dtanh_kernel(float* __restrict__ r, const float* __restrict__ dx, size_t n) {
    const size_t i = (blockIdx.x * 256ull + threadIdx.x) * PX;
    if (i >= n) return;
    if constexpr (PX == 4) {
        const float4 a = ld4(r + i), g = ld4(dx + i);
        const float t0 = tanhf(a.x), t1 = tanhf(a.y), t2 = tanhf(a.z), t3 = tanhf(a.w);
        *reinterpret_cast<float4*>(r + i) = make_float4(0.2f * (1.0f - t0 * t0) * g.x, 0.2f * (1.0f - t1 * t1) * g.y,
                                                        0.2f * (1.0f - t2 * t2) * g.z, 0.2f * (1.0f - t3 * t3) * g.w);
    } else {
        const float t = tanhf(r[i]);
        r[i] = 0.2f * (1.0f - t * t) * dx[i];
    }
}

struct PyrSpArgs {
    const float* dm; const float* x; float* dx;     // [B][C][P]
    const float* planes; int64_t plane_bstride;     // the step's two guidance planes of image 0 (adjacent); floats between images
    const float* w_a; const float* w_b;             // level: low_attn / high_attn [C][9]; chroma: chroma_attn [C][18], w_b unused
    const float* means; const float* gate_w; const float* gate_b;
    int level;
    float* taps;                                    // level: [2][nslab][C][9] (low, then high); chroma: [nslab][C][18]
    float* gsum;                                    // [slabs per image][gridDim.y][B][2]: rows of one value per image and gate for reduce_rows
    int C, h, w, slab_px, per_image, nslab;
};

// the gate heads of this step for one image (wave-uniform)
template <bool CHROMA>
__device__ __forceinline__ void step_gates(const PyrSpArgs& a, size_t img, float& g0, float& g1) {
    const float* mn = a.means + img * kMeans;
    if constexpr (CHROMA) {
        g0 = sigm(fmaf(a.gate_w[0], mn[6], a.gate_b[0]));
        g1 = 0.f;
    } else {
        const float lo = mn[2 * a.level], hi = mn[2 * a.level + 1];
        g0 = sigm(fmaf(a.gate_w[1], hi, fmaf(a.gate_w[0], lo, a.gate_b[0])));
        g1 = sigm(fmaf(a.gate_w[3], hi, fmaf(a.gate_w[2], lo, a.gate_b[1])));
    }
}

// From the two convolution sums of one pixel and dS = dm x: the gate S, the gradients at the two sums, and the gate sums
template <bool CHROMA>
__device__ __forceinline__ void gate_adjoint(float s_a, float s_b, float g0, float g1, float dS, float& S, float& ds0, float& ds1, float& sa,
                                             float& sb) {
    if constexpr (CHROMA) {
        const float a_c = sigm(s_a + s_b);
        S = g0 * a_c;
        ds0 = ds1 = g0 * dS * a_c * (1.0f - a_c);
        sa = fmaf(dS, a_c, sa);
    } else {
        const float a_l = sigm(s_a), a_h = tanhf(s_b);
        S = fmaf(g0, a_l, g1 * a_h);
        ds0 = g0 * dS * a_l * (1.0f - a_l);
        ds1 = g1 * dS * (1.0f - a_h * a_h);
        sa = fmaf(dS, a_l, sa);
        sb = fmaf(dS, a_h, sb);
    }
}

template <bool CHROMA>
__device__ __forceinline__ size_t tap_index(const PyrSpArgs& a, int slab, int c, int plane, int tap) {
    return CHROMA ? ((size_t)slab * a.C + c) * 18 + 9 * plane + tap : (((size_t)plane * a.nslab + slab) * a.C + c) * 9 + tap;
}

// What both tap kernels set up for a thread that owns channel 16 ti + r (clamped to C - 1, cvalid = false, past the last) of the
// workgroup's slab: the slab's pixel range [n_lo, n_hi) of image img, the channel's 18 weights, the step's gates, its rows
template <bool CHROMA>
struct PyrSpLane {
    int slab, ti, img, sl, h, w, P, C, n_lo, n_hi, c;
    bool cvalid;
    float wa[9], wb[9], g0, g1;
    const float *dmr, *xr, *gpl;
    float* dxr;
    __device__ __forceinline__ PyrSpLane(const PyrSpArgs& a, int r) {
        slab = blockIdx.x; ti = blockIdx.y;
        img = slab / a.per_image; sl = slab - img * a.per_image;
        h = a.h; w = a.w; P = h * w; C = a.C;
        n_lo = sl * a.slab_px; n_hi = (n_lo + a.slab_px < P) ? n_lo + a.slab_px : P;
        cvalid = 16 * ti + r < C;
        c = cvalid ? 16 * ti + r : C - 1;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            wa[t] = CHROMA ? a.w_a[c * 18 + t] : a.w_a[c * 9 + t];
            wb[t] = CHROMA ? a.w_a[c * 18 + 9 + t] : a.w_b[c * 9 + t];
        }
        step_gates<CHROMA>(a, (size_t)img, g0, g1);
        const size_t row = ((size_t)img * C + c) * P;
        dmr = a.dm + row; xr = a.x + row; dxr = a.dx + row;
        gpl = a.planes + (size_t)img * a.plane_bstride;
    }
};

// the workgroup's two gate sums -> its row of a.gsum; lds: 8 floats no thread still reads
__device__ __forceinline__ void store_gate_sums(const PyrSpArgs& a, int sl, int ti, int img, float sa, float sb, float* lds) {
    float gs[2] = {sa, sb};
    block_sums<2>(gs, lds);
    if (threadIdx.x == 0) {
        float* o = a.gsum + (((size_t)sl * gridDim.y + ti) * (a.nslab / a.per_image) + img) * 2;
        o[0] = gs[0];
        o[1] = gs[1];
    }
}

// w % 4 == 0.  Workgroup (slab, 16-channel tile); lane (r = lane & 15, kq = lane >> 4) owns channel 16 ti + r and, per trip of
// its wave, pixels n0 + 4 kq .. + 3: the A-operand layout of the tap contraction G[c][tap] = sum_p ds[c][p] plane[p + tap], whose B
// operand is tap r of the plane at the lane's 4 pixels (rows 9 .. 15 zero), one accumulator tile per plane.  The steps of the
// contraction are rf_flca_adjoint.h's, as in flca_bwd_fused_kernel; the gate arithmetic (expf / tanhf) is this kernel's.
template <bool CHROMA>
__global__ void __launch_bounds__(256) pyr_spatial_bwd_vec_kernel(PyrSpArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const PyrSpLane<CHROMA> L(a, r);
    const int h = L.h, w = L.w, P = L.P;
    const int tdy = r < 9 ? r / 3 - 1 : 0, tdx = r < 9 ? r % 3 - 1 : 0;      // this lane's tap
    f32x4 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float sa = 0.f, sb = 0.f;
    for (int n0 = L.n_lo + wave * 16; n0 < L.n_hi; n0 += 64) {
        const int nn = n0 + 4 * kq;
        const bool ok = nn < L.n_hi;
        const int n = ok ? nn : L.n_lo;
        const int y = n / w, x = n - y * w;
        const float4 dm4 = ld4(L.dmr + n), x4 = ld4(L.xr + n), d4 = ld4(L.dxr + n);
        float bv[2][4];
        tap_operand<2>(L.gpl, P, h, w, y, x, r, tdy, tdx, ok, bv);
        float s_a[4] = {0.f, 0.f, 0.f, 0.f}, s_b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int yy = y + dy - 1;
            float nb[2][6];
            neighbour_row<2>(L.gpl, P, w, x, yy, yy >= 0 && yy < h, nb);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float k0 = L.wa[dy * 3 + dx], k1 = L.wb[dy * 3 + dx];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s_a[q] = fmaf(k0, nb[0][q + dx], s_a[q]);
                    s_b[q] = fmaf(k1, nb[1][q + dx], s_b[q]);
                }
            }
        }
        const float dmv[4] = {dm4.x, dm4.y, dm4.z, dm4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
        const float live = (ok && L.cvalid) ? 1.0f : 0.f;
        float ds0[4], ds1[4], o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float dmq = live * dmv[q];
            float S;
            gate_adjoint<CHROMA>(s_a[q], s_b[q], L.g0, L.g1, dmq * xv[q], S, ds0[q], ds1[q], sa, sb);
            o[q] = fmaf(dmq, S, dv[q]);
        }
        if (ok && L.cvalid) *reinterpret_cast<float4*>(L.dxr + n) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds0[m], bv[0][m], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds1[m], bv[1][m], acc[1], 0, 0, 0);
        }
    }
    __shared__ float red[4][16][17];
    const int slab = L.slab;
    fold_tap_tiles<2>(acc, red, wave, kq, r, L.ti, L.C, [=](int t, int gi, int jj) { return a.taps + tap_index<CHROMA>(a, slab, gi, t, jj); });
    __syncthreads();      // red is free again
    store_gate_sums(a, L.sl, L.ti, L.img, sa, sb, &red[0][0][0]);
}

// Any width.  Workgroup (slab, 16-channel tile); thread (r = tid >> 4, q = tid & 15) owns channel 16 ti + r and pixels
// n_lo + q, + 16, ..: its 18 tap sums stay in registers and are added over the 16 threads of the channel by shuffles at the end.
template <bool CHROMA>
__global__ void __launch_bounds__(256) pyr_spatial_bwd_kernel(PyrSpArgs a) {
    const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
    const PyrSpLane<CHROMA> L(a, r);
    const int h = L.h, w = L.w, P = L.P;
    float ta[9], tb[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) { ta[t] = 0.f; tb[t] = 0.f; }
    float sa = 0.f, sb = 0.f;
    for (int n = L.n_lo + q; n < L.n_hi; n += 16) {
        const int y = n / w, x = n - y * w;
        float nb[2][9];
        float s_a = 0.f, s_b = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
                const size_t off = in ? (size_t)yy * w + xx : 0;
                const float v0 = L.gpl[off], v1 = L.gpl[(size_t)P + off];
                nb[0][dy * 3 + dx] = in ? v0 : 0.f;
                nb[1][dy * 3 + dx] = in ? v1 : 0.f;
                s_a = fmaf(L.wa[dy * 3 + dx], nb[0][dy * 3 + dx], s_a);
                s_b = fmaf(L.wb[dy * 3 + dx], nb[1][dy * 3 + dx], s_b);
            }
        const float dmq = L.cvalid ? L.dmr[n] : 0.f;
        float S, ds0, ds1;
        gate_adjoint<CHROMA>(s_a, s_b, L.g0, L.g1, dmq * L.xr[n], S, ds0, ds1, sa, sb);
        if (L.cvalid) L.dxr[n] = fmaf(dmq, S, L.dxr[n]);
#pragma unroll
        for (int t = 0; t < 9; ++t) { ta[t] = fmaf(ds0, nb[0][t], ta[t]); tb[t] = fmaf(ds1, nb[1][t], tb[t]); }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { ta[t] += __shfl_xor(ta[t], o, 64); tb[t] += __shfl_xor(tb[t], o, 64); }
    }
    if (q == 0 && L.cvalid) {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            a.taps[tap_index<CHROMA>(a, L.slab, L.c, 0, t)] = ta[t];
            a.taps[tap_index<CHROMA>(a, L.slab, L.c, 1, t)] = tb[t];
        }
    }
    __shared__ float red[8];
    store_gate_sums(a, L.sl, L.ti, L.img, sa, sb, red);
}

// The gate sums of every image, dg [B][2] = (sum dS a_l, sum dS a_h) or (sum dS a_c, -), through the gate head's sigmoid:
//   level:  du_k = dg_k g_k (1 - g_k);  dW[k][0] = sum_b du_k mean_low_b,  dW[k][1] = sum_b du_k mean_high_b,  db[k] = sum_b du_k
//   chroma: one scalar gate on the mean chroma magnitude
// One workgroup; a thread walks images tid, tid + 256, .. in order, block_sums adds the threads.
template <bool CHROMA>
__global__ void __launch_bounds__(256) pyr_gate_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ means,
                                                           const float* __restrict__ gate_w, const float* __restrict__ gate_b, int level,
                                                           float* __restrict__ dgw, float* __restrict__ dgb, int B, int accumulate) {
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 256) {
        const float d0 = dg[2 * b], d1 = dg[2 * b + 1];
        const float* mn = means + (size_t)b * kMeans;
        if constexpr (CHROMA) {
            const float g = sigm(fmaf(gate_w[0], mn[6], gate_b[0])), du = d0 * g * (1.0f - g);
            s[0] = fmaf(du, mn[6], s[0]);
            s[1] += du;
        } else {
            const float lo = mn[2 * level], hi = mn[2 * level + 1];
            const float g0 = sigm(fmaf(gate_w[1], hi, fmaf(gate_w[0], lo, gate_b[0]))), g1 = sigm(fmaf(gate_w[3], hi, fmaf(gate_w[2], lo, gate_b[1])));
            const float du0 = d0 * g0 * (1.0f - g0), du1 = d1 * g1 * (1.0f - g1);
            s[0] = fmaf(du0, lo, s[0]); s[1] = fmaf(du0, hi, s[1]); s[2] = fmaf(du1, lo, s[2]); s[3] = fmaf(du1, hi, s[3]);
            s[4] += du0; s[5] += du1;
        }
    }
    __shared__ float red[24];
    block_sums<6>(s, red);
    if (threadIdx.x == 0) {
        const int nw = CHROMA ? 1 : 4, nb = CHROMA ? 1 : 2;
        for (int k = 0; k < nw; ++k) dgw[k] = accumulate ? dgw[k] + s[k] : s[k];
        for (int k = 0; k < nb; ++k) dgb[k] = accumulate ? dgb[k] + s[nw + k] : s[nw + k];
    }
}

// ---- the tail.  partial[(b * gridDim.x + blk) * 4 + c] = sum over the block's pixels of g1_c;  PX = 4: w2 % 4 == 0
__device__ __forceinline__ void tail_g1(float r, float g, float b, float& r1, float& g1, float& b1) {
    const float G = 0.03f * ((r + g) + b);
    r1 = fmaf(-0.299f, G, r);
    g1 = fmaf(-0.587f, G, g);
    b1 = fmaf(-0.114f, G, b);
}

template <int PX>
__global__ void __launch_bounds__(256) ml_tail_bwd_sums_kernel(const float* __restrict__ g, float* __restrict__ partial, size_t P) {
    const size_t b = blockIdx.y;
    const float* gb = g + b * 3 * P;
    float acc[3] = {0.f, 0.f, 0.f};
    for (size_t i = (blockIdx.x * 256ull + threadIdx.x) * PX; i < P; i += (size_t)gridDim.x * 256 * PX) {
        float rv[PX], gv[PX], bv[PX];
        if constexpr (PX == 4) {
            const float4 r4 = ld4(gb + i), g4 = ld4(gb + P + i), b4 = ld4(gb + 2 * P + i);
            rv[0] = r4.x; rv[1] = r4.y; rv[2] = r4.z; rv[3] = r4.w;
            gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
            bv[0] = b4.x; bv[1] = b4.y; bv[2] = b4.z; bv[3] = b4.w;
        } else {
            rv[0] = gb[i]; gv[0] = gb[P + i]; bv[0] = gb[2 * P + i];
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            float r1, g1, b1;
            tail_g1(rv[k], gv[k], bv[k], r1, g1, b1);
            acc[0] += r1; acc[1] += g1; acc[2] += b1;
        }
    }
    __shared__ float red[12];
    block_sums<3>(acc, red);
    if (threadIdx.x == 0) {
        float* o = partial + (b * gridDim.x + blockIdx.x) * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

// every workgroup adds the image's nblk <= 256 partials in the same order, then grad_c = g1_c - 0.12 mean_p(g1_c)
template <int PX>
__global__ void __launch_bounds__(256) ml_tail_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ partial, int nblk,
                                                                float* __restrict__ out, size_t P) {
    const size_t b = blockIdx.y;
    float m[3] = {0.f, 0.f, 0.f};
    if ((int)threadIdx.x < nblk) {
        const float* s = partial + (b * nblk + threadIdx.x) * 4;
        m[0] = s[0]; m[1] = s[1]; m[2] = s[2];
    }
    __shared__ float red[12];
    block_sums<3>(m, red);
    const float k = 0.12f / (float)P;
    const float d0 = k * m[0], d1 = k * m[1], d2 = k * m[2];
    const float* gb = g + b * 3 * P;
    float* ob = out + b * 3 * P;
    for (size_t i = (blockIdx.x * 256ull + threadIdx.x) * PX; i < P; i += (size_t)gridDim.x * 256 * PX) {
        if constexpr (PX == 4) {
            const float4 r4 = ld4(gb + i), g4 = ld4(gb + P + i), b4 = ld4(gb + 2 * P + i);
            const float rv[4] = {r4.x, r4.y, r4.z, r4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            float ro[4], go[4], bo[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                tail_g1(rv[q], gv[q], bv[q], ro[q], go[q], bo[q]);
                ro[q] -= d0; go[q] -= d1; bo[q] -= d2;
            }
            *reinterpret_cast<float4*>(ob + i) = make_float4(ro[0], ro[1], ro[2], ro[3]);
            *reinterpret_cast<float4*>(ob + P + i) = make_float4(go[0], go[1], go[2], go[3]);
            *reinterpret_cast<float4*>(ob + 2 * P + i) = make_float4(bo[0], bo[1], bo[2], bo[3]);
        } else {
            float r1, g1, b1;
            tail_g1(gb[i], gb[P + i], gb[2 * P + i], r1, g1, b1);
            ob[i] = r1 - d0; ob[P + i] = g1 - d1; ob[2 * P + i] = b1 - d2;
        }
    }
}

int tail_bwd_nblk(size_t P, int px, int cap) {
    const size_t n = (P / px + 255) / 256;
    return n > (size_t)cap ? cap : n < 1 ? 1 : (int)n;
}

// ---- the block's schedule
int pyr_dch_nblk(int P) { const int n = cdiv(P, 2048); return n > 16 ? 16 : n; }

// Pixel slabs of pyr_spatial_bwd: a multiple of 64 pixels, at least 512 where the image has as many, about 1024 workgroups in all.
// A slab costs its workgroup 18 weight loads, two block reductions and a row of C x 18 partial sums for reduce_rows to add; its
// pixels cost a trip of 64 each.  Measured on the MI355X at (4, 32, 256, 256), per step: slabs of 2048 pixels (256 workgroups)
// 76 us, of 512 (1024 workgroups) 45 us, of 256 (2048 workgroups) 46 us; the five tap reductions of a call took about 25, 105 and 170 us
// ("FLCA_Pyramid backward").
void pyr_slabs(int B, int P, int nti, int* slab_px, int* per_image) {
    int per = cdiv(1024, B * nti);
    if (per > cdiv(P, 512)) per = cdiv(P, 512);
    *slab_px = cdiv(cdiv(P, per), 64) * 64;
    *per_image = cdiv(P, *slab_px);
}

// The workspace as float offsets: the one layout behind the size query and the run.
struct PyrBwdPlan {
    PyrFwdPlan f;                        // guidance, one step's m, t, r / dr, the res_proj packs, pooling sums, ch
    int dnblk, hid, nti;                 // flca_dch_kernel's pixel blocks (pyr_dch_nblk); squeeze-excite hidden width; 16-channel tiles
    int slab_px, per_image, nslab;       // pixel slabs of pyr_spatial_bwd (pyr_slabs)
    size_t xs;                           // [L + 1][B][C][P]   x_1 .. x_{L+1}  (x_0 is feat)
    size_t d;                            // [B][C][P]          dpre; dm lands in f.t, dead by then
    size_t wt;                           // the transposed pack of the data gradient at hand
    size_t wpart, wpart_cap;             // weight-gradient partials
    size_t rsum[4];                      // res_proj.0.weight, .0.bias, .2.weight, .2.bias: their gradients summed over the steps
    size_t dch_part, dmP, se_contrib;    // [B][dnblk][C], [B][C], [B][2 C hid + hid + C]
    size_t taps, gsum, dg;               // [nslab][C][18], [per_image][nti][B][2], [B][2]
};

int pyr_bwd_plan(const char* who, int B, int C, int h, int w, int H, int W, int levels, PyrBwdPlan* p, Bump* b) {
    RF_TRY(pyr_fwd_plan(who, B, C, h, w, H, W, levels, true, &p->f, b));
    const int P = h * w;
    const size_t el = (size_t)B * C * P;
    p->dnblk = pyr_dch_nblk(P); p->hid = flca_hidden(C); p->nti = cdiv(C, 16);
    pyr_slabs(B, P, p->nti, &p->slab_px, &p->per_image);
    p->nslab = B * p->per_image;
    p->xs = b->off((size_t)(levels + 1) * el);
    p->d = b->off(el);
    p->wt = b->off(packed1x1_floats(C, C));
    p->wpart_cap = wgrad1x1_partial_floats(B, C, C, P, true);
    p->wpart = b->off(p->wpart_cap);
    for (int i = 0; i < 4; ++i) p->rsum[i] = b->off(i % 2 ? (size_t)C : (size_t)C * C);
    p->dch_part = b->off((size_t)B * p->dnblk * C);
    p->dmP = b->off((size_t)B * C);
    p->se_contrib = b->off((size_t)B * ((size_t)2 * C * p->hid + p->hid + C));
    p->taps = b->off((size_t)p->nslab * C * 18);
    p->gsum = b->off((size_t)p->nslab * p->nti * 2);
    p->dg = b->off((size_t)B * 2);
    return RF_OK;
}

// dx += dm S_s in place, the tap and gate slabs of step s, then their last sums into the step's four (chroma: three) gradients
int pyr_spatial_bwd(const PyrBwdPlan& p, float* ws, const float* dm, const float* x, float* dx, int s, const PyrGroup<const float*>& prm,
                    const PyrGroup<float*>& grd, const float* means, int B, int C, int h, int w, int levels, int acc, hipStream_t st) {
    const bool chroma = s == levels;
    const size_t P = (size_t)h * w;
    PyrSpArgs a{};
    a.dm = dm; a.x = x; a.dx = dx;
    a.planes = ws + p.f.guide + (size_t)2 * s * P; a.plane_bstride = (int64_t)(2 * levels + 2) * P;
    a.w_a = chroma ? prm.chr_w : prm.low[s]; a.w_b = chroma ? nullptr : prm.high[s];
    a.means = means; a.gate_w = chroma ? prm.cgate_w : prm.gate_w[s]; a.gate_b = chroma ? prm.cgate_b : prm.gate_b[s]; a.level = s;
    a.taps = ws + p.taps; a.gsum = ws + p.gsum;
    a.C = C; a.h = h; a.w = w; a.slab_px = p.slab_px; a.per_image = p.per_image; a.nslab = p.nslab;
    const dim3 grid((unsigned)p.nslab, (unsigned)p.nti);
    const double el = (double)B * C * P;
    {
        ProfScope prof(st, "pyr_spatial_bwd_kernel", (2.0 * 36 + 120.0) * el, 16.0 * el);
        if (w % 4 == 0) {
            if (chroma) pyr_spatial_bwd_vec_kernel<true><<<grid, 256, 0, st>>>(a);
            else pyr_spatial_bwd_vec_kernel<false><<<grid, 256, 0, st>>>(a);
        } else {
            if (chroma) pyr_spatial_bwd_kernel<true><<<grid, 256, 0, st>>>(a);
            else pyr_spatial_bwd_kernel<false><<<grid, 256, 0, st>>>(a);
        }
        RF_TRY(check_launch("pyr_spatial_bwd"));
    }
    float* dg = ws + p.dg;
    RF_TRY(reduce_rows(a.gsum, dg, p.per_image * p.nti, (size_t)B * 2, 0, st));
    if (chroma) {
        pyr_gate_bwd_kernel<true><<<1, 256, 0, st>>>(dg, means, a.gate_w, a.gate_b, s, grd.cgate_w, grd.cgate_b, B, acc);
        RF_TRY(check_launch("pyr_gate_bwd"));
        return reduce_rows(a.taps, grd.chr_w, p.nslab, (size_t)C * 18, acc, st);
    }
    pyr_gate_bwd_kernel<false><<<1, 256, 0, st>>>(dg, means, a.gate_w, a.gate_b, s, grd.gate_w[s], grd.gate_b[s], B, acc);
    RF_TRY(check_launch("pyr_gate_bwd"));
    RF_TRY(reduce_rows(a.taps, grd.low[s], p.nslab, (size_t)C * 9, acc, st));
    return reduce_rows(a.taps + (size_t)p.nslab * C * 9, grd.high[s], p.nslab, (size_t)C * 9, acc, st);
}

int run_pyr_backward(const PyrBwdPlan& p, const float* feat, const float* packed, const float* dz, float* dx, const float* const* prm_, float* const* grd_,
                     float* ws, int B, int C, int h, int w, int H, int W, int levels, int acc, hipStream_t st) {
    const char* const who = "rf_flca_pyramid_backward";
    const int P = h * w;
    const size_t el = (size_t)B * C * P;
    const PyrGroup<const float*> prm = pyr_group(prm_, levels);
    const PyrGroup<float*> grd = pyr_group(grd_, levels);
    float* x_next[4];
    for (int s = 0; s <= levels; ++s) x_next[s] = ws + p.xs + (size_t)s * el;
    RF_TRY(pyr_forward_steps(p.f, ws, feat, packed, x_next, prm, B, C, h, w, H, W, levels, st));
    const float* means = pyr_means(p.f, ws, B, H, W, levels);
    float *m = ws + p.f.m, *t = ws + p.f.t, *r = ws + p.f.r, *d = ws + p.d, *ch = ws + p.f.ch, *dmP = ws + p.dmP, *contrib = ws + p.se_contrib;
    const bool vec = P % 4 == 0;      // (every buffer is 16-byte aligned: check_backward_args, Bump)
    const unsigned gv = (unsigned)((el / 4 + 255) / 256), gsc = (unsigned)((el + 255) / 256);

    // squeeze-excite: dch -> the MLP adjoint per image -> dmean / P and the four gradients; dx = dz ch + dmean / P
    {
        ProfScope prof(st, "pyr_dch_kernel", 2.0 * el, 8.0 * el);
        RF_TRY(launch_flca_dch(dz, (int64_t)C * P, x_next[levels], ws + p.dch_part, p.dnblk, B, C, P, st));
    }
    RF_TRY(launch_pyr_se(ws + p.f.pool, p.f.nblk, P, prm.se, ch, ws + p.dch_part, p.dnblk, dmP, contrib, B, C, st));
    const size_t n1 = (size_t)p.hid * C;
    RF_TRY(reduce_rows(contrib, grd.se.se1_w, B, n1, acc, st));
    RF_TRY(reduce_rows(contrib + B * n1, grd.se.se1_b, B, (size_t)p.hid, acc, st));
    RF_TRY(reduce_rows(contrib + B * (n1 + p.hid), grd.se.se3_w, B, n1, acc, st));
    RF_TRY(reduce_rows(contrib + B * (2 * n1 + p.hid), grd.se.se3_b, B, (size_t)C, acc, st));
    {
        ProfScope prof(st, "pyr_dx_kernel", 2.0 * el, 8.0 * el);
        if (vec) pyr_dx_kernel<4><<<gv, 256, 0, st>>>(dz, ch, dmP, dx, P, el);
        else pyr_dx_kernel<1><<<gsc, 256, 0, st>>>(dz, ch, dmP, dx, P, el);
        RF_TRY(check_launch("pyr_dx"));
    }

    for (int s = levels; s >= 0; --s) {
        const float* xs = s == 0 ? feat : x_next[s - 1];
        const Wgrad wg{who, ws + p.wpart, p.wpart_cap, B, P, s != levels, st};      // res_proj: the sum over the steps, in rsum
        RF_TRY(pyr_step_mtr(p.f, ws, xs, s, prm, s == levels && p.f.fused, B, C, h, w, H, W, levels, st));
        {
            ProfScope prof(st, "pyr_dtanh_kernel", 12.0 * el, 12.0 * el);
            if (vec) pyr_dtanh_kernel<4><<<gv, 256, 0, st>>>(r, dx, el);
            else pyr_dtanh_kernel<1><<<gsc, 256, 0, st>>>(r, dx, el);
            RF_TRY(check_launch("pyr_dtanh"));
        }
        RF_TRY(wgrad1x1(wg, r, C, t, C, ws + p.rsum[2], ws + p.rsum[3]));
        RF_TRY(dgrad1x1(r, C, prm.r2_w, C, ws + p.wt, nullptr, d, B, P, st));
        RF_TRY(launch_ewise(d, t, d, el, EW_LRELU_GRAD, 0.f, st));                      // ReLU: dpre where t > 0, else 0
        RF_TRY(wgrad1x1(wg, d, C, m, C, ws + p.rsum[0], ws + p.rsum[1]));
        RF_TRY(dgrad1x1(d, C, prm.r0_w, C, ws + p.wt, nullptr, t, B, P, st));           // dm
        RF_TRY(pyr_spatial_bwd(p, ws, t, xs, dx, s, prm, grd, means, B, C, h, w, levels, acc, st));
    }
    float* const res[4] = {grd.r0_w, grd.r0_b, grd.r2_w, grd.r2_b};
    for (int i = 0; i < 4; ++i) RF_TRY(reduce_rows(ws + p.rsum[i], res[i], 1, i % 2 ? (size_t)C : (size_t)C * C, acc, st));
    return RF_OK;
}

}  // namespace

}  // namespace rf

using namespace rf;

extern "C" {

long long rf_flca_pyramid_backward_workspace_bytes(int B, int C, int h, int w, int H, int W, int levels) {
    PyrBwdPlan p;
    Bump b;
    const int rc = pyr_bwd_plan("rf_flca_pyramid_backward_workspace_bytes", B, C, h, w, H, W, levels, &p, &b);
    return rc ? rc : (long long)(b.used * sizeof(float));
}

int rf_flca_pyramid_backward(const float* feat, const float* packed, const float* grad_out, float* grad_in, const float* const* prm,
                             float* const* grad_prm, void* workspace, size_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                             int levels, int accumulate, void* stream) {
    const char* const who = "rf_flca_pyramid_backward";
    PyrBwdPlan p;
    Bump b;
    RF_TRY(pyr_bwd_plan(who, B, C, h, w, H, W, levels, &p, &b));
    const Span frame{packed, (size_t)B * 4 * H * W * sizeof(float)};
    BackwardArgs c{who, feat, grad_out, grad_in, (size_t)B * C * h * w * sizeof(float), prm, grad_prm, 4 * levels + 11, workspace,
                   workspace_bytes, b.used * sizeof(float)};
    c.buffers = &frame; c.nbuffers = 1;
    RF_TRY(check_backward_args(c, [=](int i) { return pyr_prm_floats(i, C, levels); }));
    RF_CHECK_ARG(aligned16(packed), "%s: packed must be 16-byte aligned", who);
    return run_pyr_backward(p, feat, packed, grad_out, grad_in, prm, grad_prm, (float*)workspace, B, C, h, w, H, W, levels, accumulate,
                            (hipStream_t)stream);
}

long long rf_ml_corrections_backward_workspace_bytes(int B, int h2, int w2) {
    if (!(B >= 1 && B <= 65535 && h2 >= 1 && w2 >= 1 && (size_t)h2 * w2 <= ((size_t)1 << 30))) {
        set_error("rf_ml_corrections_backward_workspace_bytes: B=%d h2=%d w2=%d: every size must be positive, B <= 65535 and h2 w2 <= 2^30", B, h2, w2);
        return RF_E_INVALID;
    }
    return (long long)(align_up((size_t)B * kTailSumBlocks * 4, 64) * sizeof(float));
}

int rf_ml_corrections_backward(const float* grad_out, float* grad_image, void* workspace, size_t workspace_bytes, int B, int h2, int w2,
                        void* stream) {
    const char* const who = "rf_ml_corrections_backward";
    RF_CHECK_ARG(B >= 1 && B <= 65535 && h2 >= 1 && w2 >= 1 && (size_t)h2 * w2 <= ((size_t)1 << 30),
                 "%s: B=%d h2=%d w2=%d: every size must be positive, B <= 65535 and h2 w2 <= 2^30", who, B, h2, w2);
    RF_CHECK_ARG(grad_out && grad_image && workspace && aligned16(grad_out) && aligned16(grad_image) && aligned16(workspace),
                 "%s: grad_out, grad_image and workspace must be non-null and 16-byte aligned", who);
    const size_t need = align_up((size_t)B * kTailSumBlocks * 4, 64) * sizeof(float), P = (size_t)h2 * w2, bytes = (size_t)B * 3 * P * sizeof(float);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
        return RF_E_NOMEM;
    }
    RF_CHECK_ARG(!overlaps(grad_image, bytes, grad_out, bytes) && !overlaps(workspace, need, grad_out, bytes) && !overlaps(workspace, need, grad_image, bytes),
                 "%s: grad_image and the workspace may not alias grad_out or each other", who);
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const bool vec = w2 % 4 == 0;
    const int px = vec ? 4 : 1, nblk = tail_bwd_nblk(P, px, kTailSumBlocks), gx = tail_bwd_nblk(P, px, kTailApplyBlocks);
    const double el = (double)B * 3 * P;
    {
        ProfScope prof(st, "ml_tail_bwd_sums_kernel", 8.0 * el, 4.0 * el);
        if (vec) ml_tail_bwd_sums_kernel<4><<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(grad_out, partial, P);
        else ml_tail_bwd_sums_kernel<1><<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(grad_out, partial, P);
        RF_TRY(check_launch("ml_tail_bwd_sums"));
    }
    ProfScope prof(st, "ml_tail_bwd_apply_kernel", 9.0 * el, 8.0 * el);
    if (vec) ml_tail_bwd_apply_kernel<4><<<dim3((unsigned)gx, (unsigned)B), 256, 0, st>>>(grad_out, partial, nblk, grad_image, P);
    else ml_tail_bwd_apply_kernel<1><<<dim3((unsigned)gx, (unsigned)B), 256, 0, st>>>(grad_out, partial, nblk, grad_image, P);
    return check_launch("ml_tail_bwd_apply");
}

}  // extern "C"
