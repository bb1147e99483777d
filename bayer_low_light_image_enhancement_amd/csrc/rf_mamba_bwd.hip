// Adjoint of the Mamba module of rf_mamba.hip: (u, dL/dout, parameters) -> dL/du and the nine parameter gradients.
//
// Nothing is kept from a forward call.  mamba_forward_front (rf_mamba.hip) recomputes xz, xc, [dt ; Bm ; Cm], delta and the
// state every chunk starts from; the rest, with g = dL/dout, everything channel-major [image][channel][L]:
//
//   dyg = W_out^T g                                      dgrad1x1 (rf_grad.hip): launch_conv1x1 on a transposed pack
//   reverse scan (below)                                 -> yg = y silu(z), dz, dx (scan part + D dy), dpre, dBm / dCm slabs,
//                                                           per-chunk partials of dA_log and dD
//   dW_out = sum g (x) yg, dD, dA_log                    wgrad1x1 (rf_grad.hip), reduce_rows
//   d dt_proj.bias = sum dpre, d dt_proj.weight = sum dpre (x) dt,  d dt = W_dt^T dpre
//   dBm, dCm = slabs summed over the channel tiles       mamba_bc_reduce_kernel (fixed order)
//   dW_x = sum d[dt;Bm;Cm] (x) xc,  dxc = dx + W_x^T d[dt;Bm;Cm]
//   conv1d + SiLU adjoint (the pre-activation is recomputed from xz; taps before token 0 are neither read nor written)
//   dW_in = sum [dx;dz] (x) u,  du = W_in^T [dx;dz]
//
// Reverse scan.  With e_t = exp(delta_t A) the adjoint of the state obeys  a_t = Cm_t dy_t + b_{t+1},  b_t = e_t a_t,  b_L = 0,
// the mirror image of the forward recurrence, and it is chunked the same way (kLc tokens):
//   phase 1  mamba_adj_kernel<false>   every chunk but the first, in parallel: b at the chunk's first token from a ZERO end, and
//                                      the chunk's sum of delta
//   phase 2  mamba_adj_carry_kernel    one thread per (d, n) walks the chunks from the last to the first:
//                                      G = exp(A S_c) G + E_c;  E_c <- G  = the adjoint chunk c - 1 ends with
//   phase 3  mamba_adj_kernel<true>    every chunk again from its incoming adjoint; emits all of the above
// Phase 3 needs h_{t-1} next to a_t, i.e. the forward states in REVERSE order.  They are recomputed, never reconstructed by
// dividing by e_t (which underflows to 0): a wave first walks its chunk forward from the chunk's incoming state and keeps the
// state at every tile boundary in LDS (kLc / kT checkpoints), then takes the tiles last to first; inside a tile it takes
// kTb tokens at a time, later ones first: forward from the tile's checkpoint once more with the kTb states-before-the-token
// held in registers, and then backward.
//
// Mapping: a one-wave workgroup owns 16 channels of one chunk; a lane owns one channel and 8 of its 32 states (lane = 16 g + c:
// channel c, states 8 g .. 8 g + 7), so the kTb x 8 state history is 64 registers.  Sums over the states (y, dx, ddelta) are two
// __shfl_xor steps over the four lanes of a channel; the sums over the 16 channels of dBm_t[n], dCm_t[n] are four steps, all in
// a fixed order.  Across channel tiles dBm / dCm are written as slabs [image][tile][64][L] and summed in tile order.
// No atomics anywhere: two runs give the same bits.
#include "rf_grad.h"
#include "rf_mamba.h"

namespace rf {

static constexpr int kCw = 16;                // channels per wave
static constexpr int kS = kN / 4;             // states per lane
static constexpr int kNck = kLc / kT;         // tile-boundary checkpoints per chunk
static constexpr int kTb = 8;                 // tokens whose states-before-the-token a lane holds at once
static constexpr float kLn2 = 0.69314718055994530942f;
static_assert(kNck * 64 * kS * 4 + 4 * kCw * (kT + 1) * 4 + 2 * kT * kBrow * 4 <= 65536, "the reverse scan keeps at most 64 KB of LDS");

struct AdjArgs {
    const float* delta;    // [B][Di][L]
    const float* x;        // [B][Di][L]   conv + SiLU output
    const float* z;        // z half of in_proj's output; z_bstride floats between images
    int64_t z_bstride;
    const float* bm;       // row R of x_proj's output [B][NR][L]; Cm = row R + 32
    int64_t bc_bstride;
    const float* A_log;    // [Di][32]
    const float* Dp;       // [Di]
    const float* state;    // [B][nchunk - 1][Di][32]  the state chunk c + 1 starts from (forward phases 1-2)
    float* yg;             // [B][Di][L]   in: W_out^T g;  out: y silu(z)
    float* dpre;           // [B][Di][L]   gradient at dt_proj's output
    float* dx;             // [B][Di][L]   the scan's own part of the gradient at xc
    float* dz;             // z half of d[x ; z]; z_bstride floats between images
    float* slab;           // [B][ceil(Di / 16)][64][L]   dBm (rows 0..31) and dCm (rows 32..63) of one channel tile
    float* adj;            // [B][nchunk - 1][Di][32]  phase 1: local b; after phase 2: the adjoint chunk c ends with
    float* adj_s;          // [B][nchunk - 1][Di]      sum of delta over chunk c + 1
    float* dA_part;        // [B][nchunk][Di][32]      A dA of one chunk
    float* dD_part;        // [B][nchunk][Di]
    int Di, L, nchunk;
};

template <bool EMIT>
__global__ void __launch_bounds__(64) mamba_adj_kernel(AdjArgs a) {
    __shared__ float sd[kCw][kT + 1], sz[kCw][kT + 1], sg[kCw][kT + 1], sx[EMIT ? kCw : 1][kT + 1];
    __shared__ __attribute__((aligned(16))) float sB[EMIT ? kT : 1][kBrow];
    __shared__ __attribute__((aligned(16))) float sC[kT][kBrow];
    __shared__ __attribute__((aligned(16))) float ck[EMIT ? kNck : 1][64][kS];
    const int lane = threadIdx.x, cl = lane & 15, g8 = (lane >> 4) * kS;
    const int chunk = EMIT ? (int)blockIdx.x : (int)blockIdx.x + 1, ct = blockIdx.y, d0 = ct * kCw, d = d0 + cl;
    const size_t img = blockIdx.z;
    const int Di = a.Di, L = a.L, ns = a.nchunk - 1;
    const bool live = d < Di;
    float A2[kS], b[kS], h[kS], dA[kS];
#pragma unroll
    for (int s = 0; s < kS; ++s) {
        A2[s] = live ? -expf(a.A_log[(size_t)d * kN + g8 + s]) * kLog2e : 0.f;
        b[s] = (EMIT && live && chunk < ns) ? a.adj[((img * ns + chunk) * Di + d) * kN + g8 + s] : 0.f;
        h[s] = (EMIT && live && chunk > 0) ? a.state[((img * ns + chunk - 1) * Di + d) * kN + g8 + s] : 0.f;
        dA[s] = 0.f;
    }
    const float Dp = (EMIT && live) ? a.Dp[d] : 0.f;
    const size_t plane = img * Di * (size_t)L;
    const float* dg = a.delta + plane;
    const float* xg = a.x + plane;
    const float* zg = a.z + img * a.z_bstride;
    const float* bg = a.bm + img * a.bc_bstride;
    const float* cg = bg + (size_t)kN * L;
    float* yg = a.yg + plane;
    const int t_begin = chunk * kLc, t_end = min(L, t_begin + kLc), ntile = (t_end - t_begin + kT - 1) / kT;

    if constexpr (EMIT) {
        // forward over the chunk: the state at every tile boundary (a lane reads back only what it wrote)
        for (int k = 0; k < ntile; ++k) {
            *reinterpret_cast<float4*>(&ck[k][lane][0]) = make_float4(h[0], h[1], h[2], h[3]);
            *reinterpret_cast<float4*>(&ck[k][lane][4]) = make_float4(h[4], h[5], h[6], h[7]);
            if (k == ntile - 1) break;
            const int t0 = t_begin + k * kT;                   // a whole tile: only the chunk's last one can be partial
#pragma unroll
            for (int q = 0; q < kCw * kT / 64; ++q) {
                const int idx = lane + 64 * q, r = idx / kT, j = idx % kT;
                const bool ok = d0 + r < Di;
                const size_t o = (size_t)(d0 + r) * L + t0 + j;
                sd[r][j] = ok ? dg[o] : 0.f;
                sx[r][j] = ok ? xg[o] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < kT * kN / 64; ++q) {
                const int idx = lane + 64 * q, n = idx / kT, j = idx % kT;
                sB[j][n] = bg[(size_t)n * L + t0 + j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kT; ++j) {
                const float dl = sd[cl][j], dxv = dl * sx[cl][j];
                const float4 b0 = *reinterpret_cast<const float4*>(&sB[j][g8]), b1 = *reinterpret_cast<const float4*>(&sB[j][g8 + 4]);
                const float bb[kS] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int s = 0; s < kS; ++s) h[s] = fmaf(__builtin_amdgcn_exp2f(dl * A2[s]), h[s], dxv * bb[s]);
            }
            __syncthreads();
        }
    }

    float sdl = 0.f, dD = 0.f;
    for (int k = ntile - 1; k >= 0; --k) {
        const int t0 = t_begin + k * kT;
#pragma unroll
        for (int q = 0; q < kCw * kT / 64; ++q) {            // 16 channels x kT tokens: kT consecutive lanes per channel row
            const int idx = lane + 64 * q, r = idx / kT, j = idx % kT;
            const bool ok = d0 + r < Di && t0 + j < t_end;
            const size_t o = (size_t)(d0 + r) * L + t0 + j;
            sd[r][j] = ok ? dg[o] : 0.f;
            sz[r][j] = ok ? zg[o] : 0.f;
            sg[r][j] = ok ? yg[o] : 0.f;
            if constexpr (EMIT) sx[r][j] = ok ? xg[o] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kT * kN / 64; ++q) {             // 32 state rows x kT tokens, stored token-major
            const int idx = lane + 64 * q, n = idx / kT, j = idx % kT;
            const bool ok = t0 + j < t_end;
            const size_t o = (size_t)n * L + t0 + j;
            sC[j][n] = ok ? cg[o] : 0.f;
            if constexpr (EMIT) sB[j][n] = ok ? bg[o] : 0.f;
        }
        __syncthreads();
        // a token past the end has delta = x = g = Bm = Cm = 0: it leaves h, a and every sum as they are
        if constexpr (!EMIT) {
#pragma unroll
            for (int j = kT - 1; j >= 0; --j) {
                const float dl = sd[cl][j], zv = sz[cl][j];
                const float dy = sg[cl][j] * (zv / (1.0f + expf(-zv)));
                const float4 c0 = *reinterpret_cast<const float4*>(&sC[j][g8]), c1 = *reinterpret_cast<const float4*>(&sC[j][g8 + 4]);
                const float cc[kS] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
                for (int s = 0; s < kS; ++s) b[s] = __builtin_amdgcn_exp2f(dl * A2[s]) * fmaf(cc[s], dy, b[s]);
                sdl += dl;
            }
        } else {
#pragma unroll 1
            for (int part = kT / kTb - 1; part >= 0; --part) {
            const int j0 = part * kTb;
            const float4 h0 = *reinterpret_cast<const float4*>(&ck[k][lane][0]), h1 = *reinterpret_cast<const float4*>(&ck[k][lane][4]);
            h[0] = h0.x; h[1] = h0.y; h[2] = h0.z; h[3] = h0.w; h[4] = h1.x; h[5] = h1.y; h[6] = h1.z; h[7] = h1.w;
            float hist[kTb][kS];                               // the state BEFORE token j0 + jj
#pragma unroll 1
            for (int j = 0; j < j0; ++j) {                     // from the tile's checkpoint up to this part
                const float dl = sd[cl][j], dxv = dl * sx[cl][j];
                const float4 b0 = *reinterpret_cast<const float4*>(&sB[j][g8]), b1 = *reinterpret_cast<const float4*>(&sB[j][g8 + 4]);
                const float bb[kS] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int s = 0; s < kS; ++s) h[s] = fmaf(__builtin_amdgcn_exp2f(dl * A2[s]), h[s], dxv * bb[s]);
            }
#pragma unroll
            for (int jj = 0; jj < kTb; ++jj) {
                const int j = j0 + jj;
                const float dl = sd[cl][j], dxv = dl * sx[cl][j];
                const float4 b0 = *reinterpret_cast<const float4*>(&sB[j][g8]), b1 = *reinterpret_cast<const float4*>(&sB[j][g8 + 4]);
                const float bb[kS] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int s = 0; s < kS; ++s) {
                    hist[jj][s] = h[s];
                    h[s] = fmaf(__builtin_amdgcn_exp2f(dl * A2[s]), h[s], dxv * bb[s]);
                }
            }
#pragma unroll
            for (int jj = kTb - 1; jj >= 0; --jj) {
                const int j = j0 + jj;
                const float dl = sd[cl][j], xv = sx[cl][j], zv = sz[cl][j], gv = sg[cl][j];
                const float sig = 1.0f / (1.0f + expf(-zv)), silu = zv * sig, dy = gv * silu, dxv = dl * xv;
                const float4 b0 = *reinterpret_cast<const float4*>(&sB[j][g8]), b1 = *reinterpret_cast<const float4*>(&sB[j][g8 + 4]);
                const float4 c0 = *reinterpret_cast<const float4*>(&sC[j][g8]), c1 = *reinterpret_cast<const float4*>(&sC[j][g8 + 4]);
                const float bb[kS] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                const float cc[kS] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                float dBv[kS], dCv[kS], y = 0.f, dxs = 0.f, dds = 0.f;
#pragma unroll
                for (int s = 0; s < kS; ++s) {
                    const float e = __builtin_amdgcn_exp2f(dl * A2[s]);
                    const float eh = e * hist[jj][s];                    // exp(delta A) h_{t-1}
                    const float ht = fmaf(dxv, bb[s], eh);              // h_t
                    const float av = fmaf(cc[s], dy, b[s]);             // a_t
                    y = fmaf(cc[s], ht, y);
                    dCv[s] = dy * ht;
                    dBv[s] = av * dxv;
                    dxs = fmaf(av, bb[s], dxs);
                    dds = fmaf(av, fmaf(A2[s] * kLn2, eh, bb[s] * xv), dds);
                    dA[s] = fmaf(av * dl, eh, dA[s]);
                    b[s] = e * av;
                }
#pragma unroll
                for (int m = 16; m <= 32; m <<= 1) {                    // over the four lanes of a channel
                    y += __shfl_xor(y, m, 64);
                    dxs += __shfl_xor(dxs, m, 64);
                    dds += __shfl_xor(dds, m, 64);
                }
#pragma unroll
                for (int m = 1; m <= 8; m <<= 1) {                      // over the 16 channels of the tile
#pragma unroll
                    for (int s = 0; s < kS; ++s) {
                        dBv[s] += __shfl_xor(dBv[s], m, 64);
                        dCv[s] += __shfl_xor(dCv[s], m, 64);
                    }
                }
                y = fmaf(Dp, xv, y);
                dD = fmaf(dy, xv, dD);
                // The slots of token j become its outputs with no barrier in between: the workgroup is ONE wave
                // (__launch_bounds__(64), a 64-thread launch), so every lane's reads of slot j precede these writes in the one
                // instruction stream.  A wider workgroup would need barriers here.
                if (lane < kCw) {
                    sd[cl][j] = dds * -expm1f(-dl);                     // softplus'(pre) = 1 - exp(-delta); 1 exactly where pre > 20
                    sx[cl][j] = fmaf(dl, dxs, Dp * dy);
                    sz[cl][j] = gv * y * (sig * fmaf(zv, 1.0f - sig, 1.0f));
                    sg[cl][j] = y * silu;
                }
                if (cl == 0) {
                    *reinterpret_cast<float4*>(&sB[j][g8]) = make_float4(dBv[0], dBv[1], dBv[2], dBv[3]);
                    *reinterpret_cast<float4*>(&sB[j][g8 + 4]) = make_float4(dBv[4], dBv[5], dBv[6], dBv[7]);
                    *reinterpret_cast<float4*>(&sC[j][g8]) = make_float4(dCv[0], dCv[1], dCv[2], dCv[3]);
                    *reinterpret_cast<float4*>(&sC[j][g8 + 4]) = make_float4(dCv[4], dCv[5], dCv[6], dCv[7]);
                }
            }
            }
            __syncthreads();
            float* pg = a.dpre + plane;
            float* xo = a.dx + plane;
            float* zo = a.dz + img * a.z_bstride;
#pragma unroll
            for (int q = 0; q < kCw * kT / 64; ++q) {
                const int idx = lane + 64 * q, r = idx / kT, j = idx % kT;
                if (d0 + r < Di && t0 + j < t_end) {
                    const size_t o = (size_t)(d0 + r) * L + t0 + j;
                    pg[o] = sd[r][j];
                    xo[o] = sx[r][j];
                    zo[o] = sz[r][j];
                    yg[o] = sg[r][j];
                }
            }
            float* so = a.slab + (img * gridDim.y + ct) * (size_t)(2 * kN) * L;
#pragma unroll
            for (int q = 0; q < kT * kN / 64; ++q) {
                const int idx = lane + 64 * q, n = idx / kT, j = idx % kT;
                if (t0 + j < t_end) {
                    so[(size_t)n * L + t0 + j] = sB[j][n];
                    so[(size_t)(kN + n) * L + t0 + j] = sC[j][n];
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if constexpr (EMIT) {
        float* ap = a.dA_part + ((img * a.nchunk + chunk) * Di + d) * kN + g8;
#pragma unroll
        for (int s = 0; s < kS; ++s) ap[s] = dA[s] * (A2[s] * kLn2);    // dA_log = dA A
        if (lane < kCw) a.dD_part[(img * a.nchunk + chunk) * Di + d] = dD;
    } else {
        float* ap = a.adj + ((img * ns + chunk - 1) * Di + d) * kN + g8;
#pragma unroll
        for (int s = 0; s < kS; ++s) ap[s] = b[s];
        if (lane < kCw) a.adj_s[(img * ns + chunk - 1) * Di + d] = sdl;
    }
}

// phase 2: adj[j] holds b at the first token of chunk j + 1 from a zero end; afterwards the adjoint chunk j ends with.  One
// thread per (d, n), from the last chunk to the first; eight chunks are loaded ahead of the eight dependent steps.
__global__ void __launch_bounds__(256) mamba_adj_carry_kernel(float* __restrict__ adj, const float* __restrict__ adj_s,
                                                              const float* __restrict__ A_log, int Di, int ns) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= Di * kN) return;
    const float A2 = -expf(A_log[gid]) * kLog2e;
    const size_t plane = (size_t)Di * kN;
    float* st = adj + (size_t)blockIdx.y * ns * plane + gid;
    const float* sp = adj_s + (size_t)blockIdx.y * ns * Di + gid / kN;
    float G = 0.f;
    for (int c0 = ns - 1; c0 >= 0; c0 -= 8) {
        float e[8], s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool ok = c0 - u >= 0;
            e[u] = ok ? st[(size_t)(c0 - u) * plane] : 0.f;
            s[u] = ok ? sp[(size_t)(c0 - u) * Di] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            G = fmaf(__builtin_amdgcn_exp2f(A2 * s[u]), G, e[u]);
            e[u] = G;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 - u >= 0) st[(size_t)(c0 - u) * plane] = e[u];
    }
}

// d[dt ; Bm ; Cm] rows R .. R + 63 = the slabs summed over the channel tiles in tile order; rows NR .. NRp - 1 (the padding to a
// multiple of 4 channels that the data-gradient GEMM reads) = 0.  Rows 0 .. R - 1 are written by the dt_proj data gradient.
__global__ void __launch_bounds__(256) mamba_bc_reduce_kernel(const float* __restrict__ slab, float* __restrict__ ddbc, int nct, int R, int NRp, int L) {
    const int t = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (t >= L) return;
    float s = 0.f;
    if (row < 2 * kN) {
        const float* sp = slab + ((size_t)blockIdx.z * nct * 2 * kN + row) * L + t;
        for (int c = 0; c < nct; ++c) s += sp[(size_t)c * 2 * kN * L];
    }
    ddbc[((size_t)blockIdx.z * NRp + R + row) * L + t] = s;
}

// dc = dxc silu'(c) with c = the convolution's pre-activation, recomputed from the x half of xz (mamba_conv_kernel's expression)
__global__ void __launch_bounds__(256) mamba_conv_act_bwd_kernel(const float* __restrict__ xz, float* __restrict__ dxc, const float* __restrict__ w,
                                                                 const float* __restrict__ b, int Di, int L, size_t total) {
    for (size_t idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int t = (int)(idx % (size_t)L);
        const size_t row = idx / (size_t)L;
        const int d = (int)(row % (size_t)Di);
        const size_t img = row / (size_t)Di;
        const float* xr = xz + (img * 2 * Di + d) * (size_t)L;
        float acc = b[d];
#pragma unroll
        for (int k = 0; k < kDc; ++k) {
            const int tt = t - (kDc - 1) + k;
            if (tt >= 0) acc = fmaf(w[d * kDc + k], xr[tt], acc);
        }
        const float sig = 1.0f / (1.0f + expf(-acc));
        dxc[idx] = dxc[idx] * (sig * fmaf(acc, 1.0f - sig, 1.0f));
    }
}

// One workgroup per (channel, image): dx_s = sum_k w[k] dc_{s + 3 - k} (tokens up to L - 1 only) into the x half of d[x ; z], and
// the row's sums  dw[k] = sum_t dc_t x_{t - 3 + k} (t - 3 + k >= 0),  db = sum_t dc_t  as partials [image][Di][4] and [image][Di].
__global__ void __launch_bounds__(256) mamba_conv_bwd_kernel(const float* __restrict__ xz, const float* __restrict__ dc, float* __restrict__ dxz,
                                                             const float* __restrict__ w, float* __restrict__ dw_part, float* __restrict__ db_part,
                                                             int Di, int L) {
    const int d = blockIdx.x;
    const size_t img = blockIdx.y;
    const float* xr = xz + (img * 2 * Di + d) * (size_t)L;
    const float* cr = dc + (img * Di + d) * (size_t)L;
    float* xo = dxz + (img * 2 * Di + d) * (size_t)L;
    float wk[kDc], acc[kDc + 1];
#pragma unroll
    for (int k = 0; k < kDc; ++k) { wk[k] = w[d * kDc + k]; acc[k] = 0.f; }
    acc[kDc] = 0.f;
    for (int t = threadIdx.x; t < L; t += 256) {
        const float c = cr[t];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kDc; ++k) {
            const int tf = t + (kDc - 1) - k, tb = t - (kDc - 1) + k;
            if (tf < L) s = fmaf(wk[k], cr[tf], s);
            if (tb >= 0) acc[k] = fmaf(c, xr[tb], acc[k]);
        }
        acc[kDc] += c;
        xo[t] = s;
    }
    __shared__ float part[4][kDc + 1];
#pragma unroll
    for (int k = 0; k <= kDc; ++k) {
        float v = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x <= kDc) {
        const int k = threadIdx.x;
        const float v = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
        if (k < kDc) dw_part[(img * Di + d) * kDc + k] = v;
        else db_part[img * Di + d] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
int mamba_bwd_plan(const char* who, int B, int L, int D, int N, int K, int E, MambaBwdPlan* p, Bump* b) {
    RF_TRY(mamba_plan(who, B, L, D, N, K, E, &p->m, b));
    const int Di = p->m.Di, R = p->m.R, NR = p->m.NR, nchunk = p->m.nchunk;
    p->NRp = (NR + 3) / 4 * 4;
    p->nct = cdiv(Di, kCw);
    const size_t plane = (size_t)B * L;
    p->u = b->off(plane * D);
    p->g = b->off(plane * D);
    p->gu = b->off(plane * D);
    p->yg = b->off(plane * Di);
    p->dpre = b->off(plane * Di);
    p->dx = b->off(plane * Di);
    p->dxc = b->off(plane * Di);
    p->dxz = b->off(plane * 2 * Di);
    p->ddbc = b->off(plane * p->NRp);
    p->slab = b->off(plane * p->nct * 2 * kN);
    p->adj = b->off((size_t)B * (nchunk - 1) * Di * kN);
    p->adj_s = b->off((size_t)B * (nchunk - 1) * Di);
    p->dA = b->off((size_t)B * nchunk * Di * kN);
    p->dD = b->off((size_t)B * nchunk * Di);
    p->cw = b->off((size_t)B * Di * kDc);
    p->cb = b->off((size_t)B * Di);
    p->csum = b->off((size_t)B * chan_sum_nblk(L) * Di);
    size_t cap = 0;                                                         // dW_out, d dt_proj.weight, dW_x, dW_in: no bias sums
    for (const size_t c : {wgrad1x1_partial_floats(B, D, Di, L, false), wgrad1x1_partial_floats(B, Di, R, L, false),
                           wgrad1x1_partial_floats(B, NR, Di, L, false), wgrad1x1_partial_floats(B, 2 * Di, D, L, false)})
        cap = cap > c ? cap : c;
    p->wpart_cap = cap;
    p->wpart = b->off(cap);
    p->t_in = b->off(packed1x1_floats(2 * Di, D));
    p->t_in3 = b->off(packed1x1_b3_floats(2 * Di, D));
    p->t_x = b->off(packed1x1_floats(p->NRp, Di));
    p->t_x3 = b->off(packed1x1_b3_floats(p->NRp, Di));
    p->t_dt = b->off(packed1x1_floats(Di, R));
    p->t_dt3 = b->off(packed1x1_b3_floats(Di, R));
    p->t_out = b->off(packed1x1_floats(D, Di));
    p->t_out3 = b->off(packed1x1_b3_floats(D, Di));
    return RF_OK;
}

// channel-major: u, g, du [B][D][L]
int run_mamba_backward(const MambaBwdPlan& p, const float* u, const float* g, float* du, const float* const* prm, float* const* grd,
                              float* ws, int B, int L, int acc, hipStream_t st) {
    const MambaPlan& m = p.m;
    const int D = m.D, Di = m.Di, R = m.R, NR = m.NR, NRp = p.NRp, nchunk = m.nchunk, ns = nchunk - 1;
    const float *w_in = prm[0], *w_conv = prm[1], *b_conv = prm[2], *w_x = prm[3], *w_dt = prm[4], *A_log = prm[6], *w_out = prm[8];
    float *xz = ws + m.xz, *xc = ws + m.xc, *dbc = ws + m.dbc, *yg = ws + p.yg, *dpre = ws + p.dpre, *dxc = ws + p.dxc, *dxz = ws + p.dxz,
          *ddbc = ws + p.ddbc, *wpart = ws + p.wpart;
    const int64_t iDi = (int64_t)Di * L, iD = (int64_t)D * L;
    const double el = (double)B * Di * L, bc = 4.0 * B * kN * (double)L;
    const Wgrad wg{"rf_mamba_backward", wpart, p.wpart_cap, B, L, acc, st};
    // data gradient of a projection W [K][Cout]: out = W^T x (+ res) on the bf16x3 GEMM, x [B][Kp >= K][L] with rows K .. Kp - 1 zero
    auto dgrad = [&](const float* x, int K, int Kp, const float* w, size_t t, size_t t3, const float* res, float* out, int64_t out_bstride, int Cout) {
        return dgrad1x1(Dgrad1x1{x, K, Kp, (int64_t)Kp * L, w, ws + t, ws + t3, res, out, out_bstride, Cout, B, L}, st);
    };
    RF_TRY(mamba_forward_front(m, u, prm, ws, B, L, st));
    // dyg = W_out^T g, into the buffer the scan turns into yg
    RF_TRY(dgrad(g, D, D, w_out, p.t_out, p.t_out3, nullptr, yg, iDi, Di));
    AdjArgs a{};
    a.delta = ws + m.delta; a.x = xc; a.z = xz + (size_t)Di * L; a.z_bstride = 2 * iDi;
    a.bm = dbc + (size_t)R * L; a.bc_bstride = (int64_t)NR * L; a.A_log = A_log; a.Dp = prm[7]; a.state = ws + m.state;
    a.yg = yg; a.dpre = dpre; a.dx = ws + p.dx; a.dz = dxz + (size_t)Di * L; a.slab = ws + p.slab;
    a.adj = ws + p.adj; a.adj_s = ws + p.adj_s; a.dA_part = ws + p.dA; a.dD_part = ws + p.dD;
    a.Di = Di; a.L = L; a.nchunk = nchunk;
    if (ns > 0) {
        {
            ProfScope prof(st, "mamba_adj_kernel<false>", 4.0 * kN * el, 12.0 * el + bc);
            mamba_adj_kernel<false><<<dim3((unsigned)ns, (unsigned)p.nct, (unsigned)B), 64, 0, st>>>(a);
            RF_TRY(check_launch("mamba_adj<false>"));
        }
        ProfScope prof(st, "mamba_adj_carry_kernel", 0.0, 8.0 * B * ns * (double)Di * kN);
        mamba_adj_carry_kernel<<<dim3((unsigned)cdiv(Di * kN, 256), (unsigned)B), 256, 0, st>>>(a.adj, a.adj_s, A_log, Di, ns);
        RF_TRY(check_launch("mamba_adj_carry"));
    }
    {
        // algorithmic HBM bytes: read delta, x, z, dyg, Bm, Cm; write yg, dz, dx, dpre and the dBm / dCm slabs
        ProfScope prof(st, "mamba_adj_kernel<true>", 26.0 * kN * el, 32.0 * el + 2.0 * bc + 2.0 * bc * p.nct);
        mamba_adj_kernel<true><<<dim3((unsigned)nchunk, (unsigned)p.nct, (unsigned)B), 64, 0, st>>>(a);
        RF_TRY(check_launch("mamba_adj<true>"));
    }
    RF_TRY(reduce_rows(a.dA_part, grd[6], B * nchunk, (size_t)Di * kN, acc, st));
    RF_TRY(reduce_rows(a.dD_part, grd[7], B * nchunk, (size_t)Di, acc, st));
    RF_TRY(wgrad1x1(wg, g, iD, D, yg, iDi, Di, grd[8], nullptr));                                                // dW_out
    // dt_proj
    {
        ProfScope prof(st, "chan_sum_kernel", el, 4.0 * el);
        RF_TRY(launch_chan_sum(dpre, iDi, grd[5], ws + p.csum, B, Di, L, acc, st));
    }
    RF_TRY(wgrad1x1(wg, dpre, iDi, Di, dbc, (int64_t)NR * L, R, grd[4], nullptr));
    RF_TRY(dgrad(dpre, Di, Di, w_dt, p.t_dt, p.t_dt3, nullptr, ddbc, (int64_t)NRp * L, R));
    {
        const int rows = 2 * kN + NRp - NR;
        ProfScope prof(st, "mamba_bc_reduce_kernel", 2.0 * kN * p.nct * (double)B * L, 2.0 * bc * (p.nct + 1));
        mamba_bc_reduce_kernel<<<dim3((unsigned)cdiv(L, 256), (unsigned)rows, (unsigned)B), 256, 0, st>>>(a.slab, ddbc, p.nct, R, NRp, L);
        RF_TRY(check_launch("mamba_bc_reduce"));
    }
    // x_proj
    RF_TRY(wgrad1x1(wg, ddbc, (int64_t)NRp * L, NR, xc, iDi, Di, grd[3], nullptr));
    RF_TRY(dgrad(ddbc, NR, NRp, w_x, p.t_x, p.t_x3, a.dx, dxc, iDi, Di));
    // conv1d + SiLU
    {
        const size_t total = (size_t)B * Di * L;
        size_t gx = (total + 255) / 256;
        if (gx > 16384) gx = 16384;
        ProfScope prof(st, "mamba_conv_act_bwd_kernel", 16.0 * el, 12.0 * el);
        mamba_conv_act_bwd_kernel<<<dim3((unsigned)gx), 256, 0, st>>>(xz, dxc, w_conv, b_conv, Di, L, total);
        RF_TRY(check_launch("mamba_conv_act_bwd"));
    }
    {
        ProfScope prof(st, "mamba_conv_bwd_kernel", 17.0 * el, 12.0 * el);
        mamba_conv_bwd_kernel<<<dim3((unsigned)Di, (unsigned)B), 256, 0, st>>>(xz, dxc, dxz, w_conv, ws + p.cw, ws + p.cb, Di, L);
        RF_TRY(check_launch("mamba_conv_bwd"));
    }
    RF_TRY(reduce_rows(ws + p.cw, grd[1], B, (size_t)Di * kDc, acc, st));
    RF_TRY(reduce_rows(ws + p.cb, grd[2], B, (size_t)Di, acc, st));
    // in_proj
    RF_TRY(wgrad1x1(wg, dxz, 2 * iDi, 2 * Di, u, iD, D, grd[0], nullptr));
    return dgrad(dxz, 2 * Di, 2 * Di, w_in, p.t_in, p.t_in3, nullptr, du, iD, D);
}

size_t mamba_prm_floats(int i, int D, int N, int K, int E) {
    const size_t Di = (size_t)E * D, R = cdiv(D, 16);
    const size_t floats[9] = {2 * Di * D, Di * K, Di, (R + 2 * N) * Di, Di * R, Di, Di * N, Di, D * Di};
    return floats[i];
}

}  // namespace rf

using namespace rf;

extern "C" {

long long rf_mamba_backward_workspace_bytes(int B, int L, int d_model, int d_state, int d_conv, int expand) {
    MambaBwdPlan p;
    Bump b;
    const int rc = mamba_bwd_plan("rf_mamba_backward_workspace_bytes", B, L, d_model, d_state, d_conv, expand, &p, &b);
    return rc ? rc : (long long)(b.used * sizeof(float));
}

int rf_mamba_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm,
                      void* workspace, size_t workspace_bytes, int B, int L, int d_model, int d_state, int d_conv, int expand,
                      int channel_major, int accumulate, void* stream) {
    MambaBwdPlan p;
    Bump b;
    RF_TRY(mamba_bwd_plan("rf_mamba_backward", B, L, d_model, d_state, d_conv, expand, &p, &b));
    // the workspace counts as an output whole: it holds the token-major call's u, g and gu copies too
    RF_TRY(check_backward_args({"rf_mamba_backward", in, grad_out, grad_in, (size_t)B * L * d_model * sizeof(float), prm, grad_prm, 9, workspace,
                                workspace_bytes, b.used * sizeof(float)},
                               [=](int i) { return mamba_prm_floats(i, d_model, d_state, d_conv, expand); }));
    RF_CHECK_ARG(in != grad_out, "rf_mamba_backward: in, grad_out and grad_in may not alias each other");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (channel_major) return run_mamba_backward(p, in, grad_out, grad_in, prm, grad_prm, ws, B, L, accumulate, st);
    RF_TRY(launch_tok_transpose(in, nullptr, ws + p.u, nullptr, nullptr, B, L, d_model, st));
    RF_TRY(launch_tok_transpose(grad_out, nullptr, ws + p.g, nullptr, nullptr, B, L, d_model, st));
    RF_TRY(run_mamba_backward(p, ws + p.u, ws + p.g, ws + p.gu, prm, grad_prm, ws, B, L, accumulate, st));
    return launch_tok_transpose(ws + p.gu, nullptr, grad_in, nullptr, nullptr, B, d_model, L, st);
}

}  // extern "C"
