// 1x1 convolution = per-image GEMM  out[co][p] = sum_k W[co][k] * x[k][p]  on the f32 matrix
// cores (v_mfma_f32_16x16x4_f32: exact f32 fmaf chain, so RawFormer keeps reference numerics).
//
// Operand mapping (one wave = 64 pixels):
//   * B: lane (j = l & 15, kq = l >> 4) reads ONE float4 = pixels p0 + 4j .. 4j+3 of channel
//     4s + kq: 16 lanes cover 256 contiguous bytes of a channel row, one wave instruction 1 KiB.
//     Component g of that float4 is the B operand of MFMA g, so x never goes through LDS (each
//     element is used by exactly one wave) and every HBM byte of x is fetched once.
//   * A: one float per lane from the lane-ordered packed weights, staged in LDS per workgroup
//     together with the bias and the LayerNorm scale/shift.
//   * D: lane holds channels 16t + 4kq + r of its 4 pixels -> 16-byte stores, 256 B per 16 lanes.
// Addresses are (wave-uniform channel base) + (one per-lane 32-bit offset).
//
// gfx950 has ONE in-order counter (vmcnt) for loads and stores: a load that is waited for drags
// every older store with it.  The kernels therefore issue every global load a tile needs
// (next tile's input, this tile's residual) BEFORE the tile's stores, keep loads branch-free
// (clamped addresses instead of predicates, so the compiler emits counted waits), and read all
// small operands (bias, gamma, beta, weights) from LDS, which has its own counter.
//
// Five kernels.  plan_conv1x1 (at the end of this file) is the single statement of the rule that picks between them and of
// their template arguments and grids; it applies the rule in this order:
//   1. conv1x1_scalar_kernel  any ragged shape (P % 4 != 0, unaligned operands, odd width in ConvTranspose mode), a residual
//                             with Cout % 16 != 0: plain FMA loop, correctness only.
//   2. conv1x1_b3_ln_kernel   b3 weights present, LayerNorm, K = 64 / 128 / 256, Cout % 64 == 0, one source, no residual
//                             (qkv and pw1 of levels 1-3): bf16 matrix pipe with three-piece operands; a workgroup normalises
//                             and splits its 64 pixels ONCE and its waves split the output tiles.
//   3. conv1x1_b3_kernel      b3 weights present, K >= 128, sources cut at multiples of 32 channels (up to three): the
//                             streaming form on the bf16 pipe, accumulators resident, K in blocks of 32; LayerNorm prologue
//                             (K = 512) at 4 tiles per workgroup only; without LayerNorm two output groups may share a
//                             512-thread workgroup and the x it fetches (PAIR) where the launch still fills the CUs.  With a
//                             Conv1x1Dw3 descriptor, one output group of four tiles and a large enough launch, the form whose
//                             third source is stencilled on the fly (conv1x1_b3_dw3_kernel, rf_gemm1x1_dw3.hip).
//   4. conv1x1_res_kernel     K <= 64, or K <= 128 without LayerNorm and residual (U-Net levels 0-1, HBM-bound): persistent
//                             workgroups; a wave keeps its whole [K x 64 px] input tile in registers, computes exact two-pass
//                             LayerNorm statistics on it, then sweeps ALL output-channel groups over the resident tile (x is
//                             read from HBM once whatever Cout is) while the next tile's loads are already in flight (K <= 64).
//   5. conv1x1_stream_kernel  everything else (K = 96 .. 128 with LayerNorm or a residual, K > 128 without b3 weights or
//                             with sources not cut at 8 / 32 channels): f32 MFMA, accumulators resident, K streamed in chunks;
//                             the next chunk's x (registers) and weights (registers -> LDS double buffer) are fetched while the
//                             current one is in the matrix pipe; one barrier per chunk.
// Fused: LayerNorm prologue (a4), second source (torch.cat without the copy), bias, residual,
// LeakyReLU, ConvTranspose2d(k=2,s=2) scatter (a9), per-image weights (wp_bstride != 0) for the
// attention / squeeze-excite matrices folded into the projection.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "rf_gemm1x1_tile.h"   // ldv, b3_split_pair, epilogue, stage_bias, b3_load_x_block: shared with rf_gemm1x1_dw3.hip

namespace rf {

// wave-uniform base of the 4-channel k-set s (channels 4s .. 4s+3 come from one source)
__device__ __forceinline__ const float* kset_base(const Conv1x1Args& a, int b, int s) {
    const int k = 4 * s;
    const bool first = k < a.C1;                       // selects, not branches: a branch around the loads that use this
    const float* src = first ? a.x1 : a.x2;            // base makes hipcc close each block with s_waitcnt vmcnt(0)
    const size_t off = (size_t)b * (size_t)(first ? a.x1_bstride : a.x2_bstride) + (size_t)(first ? k : k - a.C1) * (size_t)a.P;
    return src + off;
}

// ---- pieces the kernels share (operands by value or by reference-to-array: see the note at b3_load_x_block's call site)
template <int NCO>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NCO][4]) {
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------------------------
// Resident-input kernel.  KS = k-sets held in registers (K <= 4 * KS; missing k-sets are
// duplicates of the last one against zero weights).  A workgroup is persistent over the
// 256-pixel tiles of ONE image; its weight slice (output tiles [grp*ntw, grp*ntw+ntw), padded to
// a multiple of NCO = 2) sits in LDS as [KS][tpad][64] floats.  LDS map:
//   [0, KS*tpad*64) weights | tpad*16 bias | 4*KS gamma | 4*KS beta
// ---------------------------------------------------------------------------------------------
template <int KS, bool LN, int RT, bool DBUF>   // RT = residual tiles prefetched per workgroup (0, 2 or 4)
__global__ void __launch_bounds__(256, (KS <= 8 ? 3 : 2)) conv1x1_res_kernel(Conv1x1Args a, int ntw, int ngroups) {
    constexpr int NCO = 2;
    constexpr bool RES = RT > 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int grp = blockIdx.x % ngroups;
    const int wg = blockIdx.x / ngroups, nwg = gridDim.x / ngroups;
    const int b = blockIdx.y;
    const int P = a.P;
    const int K = a.C1 + a.C2;
    const int NS = K >> 2;
    const int NT = (a.Cout + 15) >> 4;
    const int tbeg = grp * ntw;
    const int tcnt = (NT - tbeg < ntw) ? NT - tbeg : ntw;
    const int tpad = (tcnt + NCO - 1) / NCO * NCO;
    const int ntiles = (P + 255) >> 8;
    float* lds_w = lds;
    float* bias_l = lds + KS * tpad * 64;
    float* gam_l = bias_l + tpad * 16;
    float* bet_l = gam_l + 4 * KS;

    // branch-free tile load: dead lanes (p0 >= P) read pixel 0, missing k-sets re-read the last one
    auto load_tile = [&](int tile, float4 (&dst)[KS]) {
        const int p0 = (tile * 4 + wave) * 64 + 4 * j;
        const unsigned voff = (unsigned)kq * (unsigned)P + (unsigned)(p0 < P ? p0 : 0);
#pragma unroll
        for (int s = 0; s < KS; ++s) dst[s] = ldv(kset_base(a, b, s < NS ? s : NS - 1), voff);
    };

    float4 xr[KS], xn[DBUF ? KS : 1];
    int tile = wg;
    load_tile(tile < ntiles ? tile : 0, xr);
    {   // weights, bias, LayerNorm affine -> LDS, once per workgroup (overlaps the first tile's loads)
        const float* wp = a.wp + (size_t)b * a.wp_bstride;
        const int n4 = KS * tpad * 16;
        for (int idx = tid; idx < n4; idx += 256) {
            const int l4 = idx & 15;
            const int t = (idx >> 4) % tpad;
            const int s = (idx >> 4) / tpad;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < tcnt && s < NS) v = *reinterpret_cast<const float4*>(wp + ((size_t)s * NT + tbeg + t) * 64 + l4 * 4);
            *reinterpret_cast<float4*>(lds_w + ((size_t)s * tpad + t) * 64 + l4 * 4) = v;
        }
        stage_bias(a, bias_l, tbeg, tpad, tid);
        if constexpr (LN) {
            for (int i = tid; i < 4 * KS; i += 256) {
                gam_l[i] = i < K ? a.ln_w[i] : 0.f;
                bet_l[i] = (a.ln_b && i < K) ? a.ln_b[i] : 0.f;
            }
        }
    }
    __syncthreads();

    for (; tile < ntiles; tile += nwg) {
        const int p0 = (tile * 4 + wave) * 64 + 4 * j;
        const bool live = p0 < P;
        const int tnext = tile + nwg;
        // ---- every global load this iteration needs is issued here, ahead of the tile's stores
        if constexpr (DBUF) {
            load_tile(tnext < ntiles ? tnext : tile, xn);
        }
        float4 res[RES ? RT * 4 : 1];   // residual rows of this workgroup's output tiles (Cout % 16 == 0 here)
        if constexpr (RES) {
            const float* resb = a.res + (size_t)b * a.res_bstride;
            const unsigned voff = (unsigned)(4 * kq) * (unsigned)P + (unsigned)(live ? p0 : 0);
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)   // tiles past tcnt re-read the last one: loads stay branch-free
                    res[t * 4 + r] = ldv(resb + (size_t)(16 * (tbeg + (t < tcnt ? t : tcnt - 1)) + r) * P, voff);
        }
        // ---- LayerNorm on the resident tile: exact two-pass statistics over the K channels
        if constexpr (LN) {
            float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (s < NS) { sum[0] += xr[s].x; sum[1] += xr[s].y; sum[2] += xr[s].z; sum[3] += xr[s].w; }
            const float invK = 1.0f / (float)K;
            float mu[4], var[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                sum[g] += __shfl_xor(sum[g], 16);
                sum[g] += __shfl_xor(sum[g], 32);
                mu[g] = sum[g] * invK;
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < NS) {
                    const float d0 = xr[s].x - mu[0], d1 = xr[s].y - mu[1], d2 = xr[s].z - mu[2], d3 = xr[s].w - mu[3];
                    var[0] = fmaf(d0, d0, var[0]); var[1] = fmaf(d1, d1, var[1]);
                    var[2] = fmaf(d2, d2, var[2]); var[3] = fmaf(d3, d3, var[3]);
                }
            }
            float rstd[4], sh[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                var[g] += __shfl_xor(var[g], 16);
                var[g] += __shfl_xor(var[g], 32);
                rstd[g] = 1.0f / sqrtf(var[g] * invK + a.ln_eps);
                sh[g] = a.ln_b ? mu[g] : 0.f;   // BiasFree_LayerNorm keeps the mean in the numerator
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float gk = gam_l[4 * s + kq], bk = bet_l[4 * s + kq];
                xr[s].x = fmaf((xr[s].x - sh[0]) * rstd[0], gk, bk);
                xr[s].y = fmaf((xr[s].y - sh[1]) * rstd[1], gk, bk);
                xr[s].z = fmaf((xr[s].z - sh[2]) * rstd[2], gk, bk);
                xr[s].w = fmaf((xr[s].w - sh[3]) * rstd[3], gk, bk);
            }
        }
        // ---- sweep the output-channel groups over the resident tile
        auto do_group = [&](int tg, const float4* resp) {
            f32x4 acc[NCO][4];
            zero_acc(acc);
            const float* wl = lds_w + (size_t)tg * 64 + lane;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float xb[4] = {xr[s].x, xr[s].y, xr[s].z, xr[s].w};
#pragma unroll
                for (int t = 0; t < NCO; ++t) {
                    const float av = wl[((size_t)s * tpad + t) * 64];
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[g], acc[t][g], 0, 0, 0);
                }
            }
            epilogue<NCO, RES>(a, acc, tbeg + tg, tcnt - tg, bias_l + (a.mode == 0 ? 16 : 4) * tg, resp, b, p0, kq, live);
        };
        if constexpr (RES) {   // at most two groups, unrolled so the residual registers are indexed statically
            do_group(0, &res[0]);
            if constexpr (RT > NCO) {
                if (tpad > NCO) do_group(NCO, &res[NCO * 4]);
            }
        } else {
#pragma unroll 1
            for (int tg = 0; tg < tpad; tg += NCO) do_group(tg, res);
        }
        if constexpr (DBUF) {
#pragma unroll
            for (int s = 0; s < KS; ++s) xr[s] = xn[s];
        } else {
            if (tnext < ntiles) load_tile(tnext, xr);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Streaming kernel: accumulators for NCO tiles resident, K in chunks of KCH k-sets.
// ---------------------------------------------------------------------------------------------
static constexpr int kStreamLnMaxK = 1024;   // LayerNorm gamma/beta staged in LDS (RawFormer-L level 3 has K = 512)

template <int NCO, int KCH, bool LN>
__global__ void __launch_bounds__(256, 2) conv1x1_stream_kernel(Conv1x1Args a, int ngroups) {
    __shared__ __attribute__((aligned(16))) float lds_w[2][KCH * NCO * 64];
    __shared__ float bias_l[NCO * 16];
    __shared__ float gam_l[LN ? kStreamLnMaxK : 4], bet_l[LN ? kStreamLnMaxK : 4];
    constexpr int WPT = KCH * NCO * 16 / 256;   // float4 of weights each thread moves per chunk
    static_assert(KCH * NCO * 16 % 256 == 0, "weight chunk must split evenly over the workgroup");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int grp = blockIdx.x % ngroups;
    const int tile = blockIdx.x / ngroups;
    const int b = blockIdx.y;
    const int P = a.P;
    const int K = a.C1 + a.C2;
    const int NS = K >> 2;
    const int NT = (a.Cout + 15) >> 4;
    const int t0 = grp * NCO;
    const int tcnt = (NT - t0 < NCO) ? NT - t0 : NCO;
    const int nch = (NS + KCH - 1) / KCH;
    const int p0 = (tile * 4 + wave) * 64 + 4 * j;
    const bool live = p0 < P;
    const unsigned voff = (unsigned)kq * (unsigned)P + (unsigned)(live ? p0 : 0);
    const float* wp = a.wp + (size_t)b * a.wp_bstride;
    stage_bias(a, bias_l, t0, NCO, tid);
    if constexpr (LN) {
        for (int i = tid; i < 4 * nch * KCH; i += 256) {          // zero beyond K: those k-sets meet zero weights anyway
            gam_l[i] = i < K ? a.ln_w[i] : 0.f;
            bet_l[i] = (a.ln_b && i < K) ? a.ln_b[i] : 0.f;
        }
    }

    // The residual initialises the accumulators: its loads travel with the first chunk's (one exposed
    // round trip instead of two) and the epilogue stays store-only.
    f32x4 acc[NCO][4];
    zero_acc(acc);
    if (a.res && a.mode == 0) {   // (wave-uniform)
        // branch-free: a conditional block around each load would be closed with s_waitcnt vmcnt(0), i.e. 32
        // serialised round trips to HBM; rows that do not exist read row 0 of the image and are masked to zero
        // (conv1x1_b3_kernel has the same loop: as a shared function it changes that kernel's code)
        const float* resb = a.res + (size_t)b * a.res_bstride;
        const unsigned vo = (unsigned)(live ? p0 : 0);
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (t0 + t) + 4 * kq + r;
                const bool ok = live && t < tcnt && co < a.Cout;
                const float4 rv = ldv(resb + (size_t)(ok ? co : 0) * P, vo);
                acc[t][0][r] = ok ? rv.x : 0.f; acc[t][1][r] = ok ? rv.y : 0.f;
                acc[t][2][r] = ok ? rv.z : 0.f; acc[t][3][r] = ok ? rv.w : 0.f;
            }
    }

    // LayerNorm statistics (shifted single pass; lanes kq = 0..3 split the channels)
    float lnA[4] = {1.f, 1.f, 1.f, 1.f}, lnB[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (LN) {
        const float4 s4 = ldv(kset_base(a, b, 0), (unsigned)(live ? p0 : 0));
        const float sh[4] = {s4.x, s4.y, s4.z, s4.w};
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
        for (int s = 0; s < NS; ++s) {
            const float4 t = ldv(kset_base(a, b, s), voff);
            const float d[4] = {t.x - sh[0], t.y - sh[1], t.z - sh[2], t.w - sh[3]};
#pragma unroll
            for (int g = 0; g < 4; ++g) { s1[g] += d[g]; s2[g] = fmaf(d[g], d[g], s2[g]); }
        }
        const float invK = 1.0f / (float)K;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            s1[g] += __shfl_xor(s1[g], 16); s1[g] += __shfl_xor(s1[g], 32);
            s2[g] += __shfl_xor(s2[g], 16); s2[g] += __shfl_xor(s2[g], 32);
            const float md = s1[g] * invK;
            const float var = fmaxf(fmaf(-md, md, s2[g] * invK), 0.f);
            const float rstd = 1.0f / sqrtf(var + a.ln_eps);
            lnA[g] = rstd;
            lnB[g] = a.ln_b ? -(sh[g] + md) * rstd : 0.f;
        }
    }

    float4 xa[KCH], xb_[KCH], wr[WPT];
    auto load_x_chunk = [&](int c, float4 (&dst)[KCH]) {
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int s = c * KCH + i;
            dst[i] = ldv(kset_base(a, b, s < NS ? s : NS - 1), voff);   // k-sets past K meet zero weights
        }
    };
    auto load_w_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int idx = tid + 256 * i;
            const int l4 = idx & 15, t = (idx >> 4) % NCO, s = c * KCH + (idx >> 4) / NCO;
            const bool ok = s < NS && t < tcnt;
            const float4 v = *reinterpret_cast<const float4*>(wp + ((size_t)(ok ? s : 0) * NT + t0 + (ok ? t : 0)) * 64 + l4 * 4);
            wr[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_w_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) *reinterpret_cast<float4*>(&lds_w[buf][(tid + 256 * i) * 4]) = wr[i];
    };
    // one chunk: the next chunk's x goes into the OTHER register set (no copies), its weights into the other LDS buffer
    auto chunk = [&](int c, float4 (&xc)[KCH], float4 (&xn)[KCH]) {
        if (c + 1 < nch) {   // next chunk in flight while this one computes
            load_x_chunk(c + 1, xn);
            load_w_chunk(c + 1);
        }
        const float* wl = &lds_w[c & 1][lane];
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            float xv[4] = {xc[i].x, xc[i].y, xc[i].z, xc[i].w};
            if constexpr (LN) {
                const int k = 4 * (c * KCH + i) + kq;
                const float gk = gam_l[k], bk = bet_l[k];
#pragma unroll
                for (int g = 0; g < 4; ++g) xv[g] = fmaf(fmaf(xv[g], lnA[g], lnB[g]), gk, bk);
            }
            // (reading the A operands one k-set ahead, pinned with sched_barrier, was measured: no gain -- the LDS
            // latency is already covered by the other wave of the SIMD)
#pragma unroll
            for (int t = 0; t < NCO; ++t) {
                const float av = wl[(i * NCO + t) * 64];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xv[g], acc[t][g], 0, 0, 0);
            }
        }
        if (c + 1 < nch) store_w_chunk((c + 1) & 1);
        __syncthreads();
    };

    load_x_chunk(0, xa);
    load_w_chunk(0);
    store_w_chunk(0);
    __syncthreads();
    for (int c = 0; c < nch; c += 2) {
        chunk(c, xa, xb_);
        if (c + 1 < nch) chunk(c + 1, xb_, xa);
    }
    epilogue<NCO, false>(a, acc, t0, tcnt, bias_l, nullptr, b, p0, kq, live);
}


// ---------------------------------------------------------------------------------------------
// b3 streaming kernel: the same GEMM on the bf16 matrix pipe with three-piece operands (rf_common.h).
// K is streamed in blocks of 32 channels = one v_mfma_f32_16x16x32_bf16 K extent.  Lane (j, kq) loads, for i = 0..7,
// one float4 = pixels p0 + 4j .. 4j+3 of channel 32c + 8kq + i; component g of those eight registers is -- after the
// split -- the B operand of pixel group g (the D layout, and with it the epilogue, is that of the f32 kernels).
// Per block and wave: 176 VALU for the split of 32 values x 4 pixels, 3 * NCO ds_read_b128 for the weight pieces,
// 24 * NCO MFMAs of 17 cycles (f32 form: 32 * NCO MFMAs of 33 cycles).  The next block's x is loaded into the registers
// the split has just vacated, its weights go registers -> LDS behind the MFMAs; one barrier per block.
// ---------------------------------------------------------------------------------------------
// PAIR (launch_conv1x1: no LayerNorm, more than one output group, a launch that still gives every CU a workgroup): the output
// groups of a pixel tile share the x they fetch.  A workgroup is 512 threads = two halves of four waves; half h runs output group
// 2 gp + h of the SAME 256 pixels with its own bias and double-buffered weight slice, so wave w and wave w + 4 issue the same x
// loads at the same time and the second one is served on the CU.  The pairs gp of a pixel tile get workgroup ids 8 apart
// (conv1x1_group_map, rf_common.h): they run back to back on one XCD and its L2 serves what the first pair fetched.  The grid
// is flat (images x pixel tiles x pairs, padded to whole chunks; the padding exits at once).  An odd group count leaves the last
// pair's second half without output tiles: it loads x, multiplies zero weights and stores nothing (at 3 groups a third more
// matrix work per pixel tile than the unpaired form; no layer of RawFormer-S / B / L has an odd count).  Per output the k order, the
// six-term chains and the epilogue are those of the unpaired form: same bits.
template <int NCO, bool LN, bool PAIR = false>
__global__ void __launch_bounds__(PAIR ? 512 : 256, 2) conv1x1_b3_kernel(Conv1x1Args a, int ngroups) {
    static_assert(!(PAIR && LN), "the paired form has no LayerNorm prologue");
    constexpr int NH = PAIR ? 2 : 1;
    __shared__ __attribute__((aligned(16))) u32x4 lds_w[NH * 2][NCO * 3 * 64];   // [half][buffer]
    __shared__ float bias_l[NH * NCO * 16];
    __shared__ float gam_l[LN ? kStreamLnMaxK : 4], bet_l[LN ? kStreamLnMaxK : 4];
    constexpr int WPT = (NCO * 3 * 64 + 255) / 256;   // 16-byte weight elements each thread moves per block
    const int tid = PAIR ? threadIdx.x & 255 : threadIdx.x;       // inside the half
    const int half = PAIR ? threadIdx.x >> 8 : 0;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    unsigned unit = 0, gp = 0, utiles = 1;
    if constexpr (PAIR) {
        utiles = (unsigned)(a.P + 255) >> 8;
        if (!conv1x1_group_map(blockIdx.x, (unsigned)a.B * utiles, (unsigned)(ngroups + 1) >> 1, &unit, &gp)) return;   // (whole workgroup)
    }
    const int grp = PAIR ? 2 * (int)gp + half : blockIdx.x % ngroups;
    const int tile = PAIR ? unit % utiles : blockIdx.x / ngroups;
    const int b = PAIR ? unit / utiles : blockIdx.y;
    const int P = a.P;
    const int K = a.C1 + a.C2 + a.C3;
    const int NB = (K + 31) >> 5;
    const int NT = (a.Cout + 15) >> 4;
    const bool idle = PAIR && grp >= ngroups;           // the second half of the last pair of an odd group count: reads tile 0, writes nothing
    const int t0 = idle ? 0 : grp * NCO;
    const int tcnt = idle ? 0 : (NT - t0 < NCO) ? NT - t0 : NCO;
    const int p0 = (tile * 4 + wave) * 64 + 4 * j;
    const bool live = p0 < P;
    const unsigned pl = (unsigned)(live ? p0 : 0);
    const u32x4* wp3 = reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(a.wp3) + (size_t)b * a.wp3_bstride);
    stage_bias(a, bias_l + half * NCO * 16, t0, NCO, tid);
    if constexpr (LN) {
        for (int i = tid; i < 32 * NB; i += 256) {
            gam_l[i] = i < K ? a.ln_w[i] : 0.f;
            bet_l[i] = (a.ln_b && i < K) ? a.ln_b[i] : 0.f;
        }
    }

    f32x4 acc[NCO][4];
#pragma unroll
    for (int t = 0; t < NCO; ++t)      // (zero_acc here moves the zeroing ahead of the branch below)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.res && a.mode == 0) {   // the residual initialises the accumulators (branch-free loads, see conv1x1_stream_kernel)
        const float* resb = a.res + (size_t)b * a.res_bstride;
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (t0 + t) + 4 * kq + r;
                const bool ok = live && t < tcnt && co < a.Cout;
                const float4 rv = ldv(resb + (size_t)(ok ? co : 0) * P, pl);
                acc[t][0][r] = ok ? rv.x : 0.f; acc[t][1][r] = ok ? rv.y : 0.f;
                acc[t][2][r] = ok ? rv.z : 0.f; acc[t][3][r] = ok ? rv.w : 0.f;
            }
    }

    // LayerNorm statistics (shifted single pass; lanes kq = 0..3 split the channels)
    float lnA[4] = {1.f, 1.f, 1.f, 1.f}, lnB[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (LN) {
        const unsigned voff = (unsigned)kq * (unsigned)P + pl;
        const float4 s4 = ldv(kset_base(a, b, 0), pl);
        const float sh[4] = {s4.x, s4.y, s4.z, s4.w};
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
        for (int s = 0; s < (K >> 2); ++s) {
            const float4 t = ldv(kset_base(a, b, s), voff);
            const float d[4] = {t.x - sh[0], t.y - sh[1], t.z - sh[2], t.w - sh[3]};
#pragma unroll
            for (int g = 0; g < 4; ++g) { s1[g] += d[g]; s2[g] = fmaf(d[g], d[g], s2[g]); }
        }
        const float invK = 1.0f / (float)K;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            s1[g] += __shfl_xor(s1[g], 16); s1[g] += __shfl_xor(s1[g], 32);
            s2[g] += __shfl_xor(s2[g], 16); s2[g] += __shfl_xor(s2[g], 32);
            const float md = s1[g] * invK;
            const float var = fmaxf(fmaf(-md, md, s2[g] * invK), 0.f);
            const float rstd = 1.0f / sqrtf(var + a.ln_eps);
            lnA[g] = rstd;
            lnB[g] = a.ln_b ? -(sh[g] + md) * rstd : 0.f;
        }
    }

    float4 xr[8];
    u32x4 wr[WPT];
    // channel 32c + 8kq + i of block c: sources are cut at multiples of 32 channels (launch_conv1x1 checks), channels past K
    // re-read the last one (their weights are zero)
    // (the sources are passed BY VALUE to a function: a conditional between two variables captured by a lambda is a conditional
    // between two addresses of its closure, and hipcc then keeps the closure -- and the xr registers it refers to -- in scratch)
    const float* const xb1 = a.x1 + (size_t)b * (size_t)a.x1_bstride;
    const float* const xb2 = a.x2 + (size_t)b * (size_t)a.x2_bstride;      // only dereferenced when C2 / C3 > 0
    const float* const xb3 = a.x3 + (size_t)b * (size_t)a.x3_bstride;
    auto load_x_block = [&](int c) { b3_load_x_block(xr, xb1, xb2, xb3, a.C1, a.C2, a.C3, c, kq, (unsigned)P, pl); };
    auto load_w_block = [&](int c) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int idx = tid + 256 * i;                       // (t, piece, lane) of this workgroup's slice
            const int t = idx / 192, rem = idx - t * 192;
            const bool ok = idx < NCO * 192 && t < tcnt;
            const u32x4 v = wp3[((size_t)c * NT + t0 + (ok ? t : 0)) * 192 + (ok ? rem : 0)];
            wr[i] = ok ? v : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_w_block = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i)
            if (tid + 256 * i < NCO * 192) lds_w[2 * half + buf][tid + 256 * i] = wr[i];
    };

    load_x_block(0);
    load_w_block(0);
    store_w_block(0);
    __syncthreads();
    for (int c = 0; c < NB; ++c) {
        // ---- LayerNorm + three-piece split of this block's 8 channels x 4 pixels
        u32x4 bp[4][3];
#pragma unroll
        for (int hp = 0; hp < 4; ++hp) {          // channel pair (2 hp, 2 hp + 1) -> dword hp of every operand
            float xa[4] = {xr[2 * hp].x, xr[2 * hp].y, xr[2 * hp].z, xr[2 * hp].w};
            float xb[4] = {xr[2 * hp + 1].x, xr[2 * hp + 1].y, xr[2 * hp + 1].z, xr[2 * hp + 1].w};
            if constexpr (LN) {
                const int k = 32 * c + 8 * kq + 2 * hp;
                const float ga = gam_l[k], ba = bet_l[k], gb = gam_l[k + 1], bb = bet_l[k + 1];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    xa[g] = fmaf(fmaf(xa[g], lnA[g], lnB[g]), ga, ba);
                    xb[g] = fmaf(fmaf(xb[g], lnA[g], lnB[g]), gb, bb);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) b3_split_pair(xa[g], xb[g], bp, g, hp);
        }
        if (c + 1 < NB) {   // next block in flight while this one is in the matrix pipe (x into the registers just vacated)
            load_x_block(c + 1);
            load_w_block(c + 1);
        }
        const u32x4* wl = &lds_w[2 * half + (c & 1)][lane];
#pragma unroll
        for (int t = 0; t < NCO; ++t) {
            const u32x4 ap[3] = {wl[(t * 3 + 0) * 64], wl[(t * 3 + 1) * 64], wl[(t * 3 + 2) * 64]};
            b3_mfma4(ap, bp, acc[t]);
        }
        if (c + 1 < NB) store_w_block((c + 1) & 1);
        __syncthreads();
    }
    epilogue<NCO, false>(a, acc, t0, tcnt, bias_l + half * NCO * 16, nullptr, b, p0, kq, live);
}

// ---------------------------------------------------------------------------------------------
// LayerNorm + 1x1 at levels 2-3 (K = 128 / 256, Cout = 2K or 3K): the input tile is normalised and split ONCE.
//   conv1x1_b3_kernel gives every workgroup 4-6 output tiles and re-reads, re-normalises and re-splits its 256 pixels for
//   each of the Cout / 64 output groups (6 passes over x for the level-2 qkv).  Here a workgroup owns 64 pixels and ALL
//   output tiles: the four waves load K / 4 channels each, reduce the two-pass statistics through LDS, write the three
//   bf16 pieces of the normalised tile to LDS in B-operand order ([K block][pixel q][piece][lane], 12 KB per 32 channels),
//   and then split the OUTPUT tiles: wave w computes tiles [w tpw, (w + 1) tpw) in chunks of NCO, reading the shared B
//   pieces from LDS (double-buffered per K block) and its A pieces straight from L2 (each weight element is used by exactly
//   one wave of the workgroup).
//
//   Inside the pixel-tile loop no wait at the START of a chunk covers an output store, and no wait of the GEMM phase the
//   next tile's input.  With the one in-order vmcnt that takes three things:
//   * every load is OLDER than the stores that follow it.  A chunk's stores come last in the chunk; ahead of them go the A
//     pieces of the first RING - 1 steps of the NEXT chunk (after a tile's last chunk: of the next tile's first chunk, the
//     same weights), into the ring registers the finished chunk has vacated, and, in the tile's last chunk, the next
//     tile's x (behind the chunk's last A load, so no wait for a ring slot covers it either).  A wave whose output tiles
//     are ONE chunk (RESIDENT: tpw == NCO at K = 64, every level-1 launch) keeps the A pieces of all KB NCO steps in
//     registers for all its pixel tiles instead, and its tile loop has x loads and stores only.  What one in-order counter
//     leaves: a ring load issued INSIDE a chunk is younger than the stores of the chunk before, so from step RING - 1 on a
//     chunk's waits cover those stores, RING - 1 steps after they were issued.
//   * the loop holds no other load: gamma and beta sit in registers from before the loop (not at K = 128, see LNREG).
//   * the stores are straight-line code.  A store under a lane condition is a block hipcc may branch around, and at the
//     join its wait counts assume the path without the store: every later wait for an older load then drains the stores
//     as well.  So every lane stores: the lanes past the end of a ragged last tile carry the tile's FIRST pixel group
//     (the same loads, the same arithmetic, the same bits as lanes j = 0) and store it to the same addresses in the same
//     instruction.  For the same reason the load of the next tile's x is unconditional: behind the last tile it reads 16
//     bytes at the start of the image per instruction.
//   The listing is the proof, not the source order (tools/loop_waits.py; profiles/b3ln_waits.md).
// ---------------------------------------------------------------------------------------------
template <int KB, int NCO, bool RESIDENT>
__device__ __forceinline__ void b3_ln_tiles(const Conv1x1Args& a, const int tpw, u32x4* __restrict__ Bl, float* __restrict__ red,
                                            const float* __restrict__ bias_l) {
    constexpr int KPW = KB >= 4 ? KB / 4 : 1; // K blocks each wave loads ...
    constexpr int CPT = KB >= 4 ? 8 : 4;      // ... and channels of a block per lane: K = 64 splits each block over two waves
    constexpr int K = 32 * KB;
    // A pieces straight from L2: RESIDENT all STEPS (K block, tile) steps of the wave's one chunk; otherwise a ring of RING
    // steps, a step's three 16-byte loads issued RING - 1 steps (x 24 MFMAs = 408 cycles each) before their use
    constexpr int STEPS = KB * NCO, RING = RESIDENT ? STEPS : KB > 4 ? 12 : (STEPS < 5 ? STEPS : 5);
    constexpr int AHEAD = RESIDENT ? STEPS : RING - 1;       // steps whose A pieces are loaded before their chunk begins
    // the step of a tile's last chunk at which the next tile's x is loaded: behind the chunk's last A load -- except <4, 3>, two
    // workgroups per CU with 60 ring and 96 B-piece registers: there x waits for the last K block, whose steps leave the
    // other B buffer free
    constexpr int XSTEP = (KB == 4 && NCO == 3) ? STEPS - NCO : STEPS - RING;
    // The wave index lives in a scalar register, so every address below is (scalar base) + (ONE per-lane offset that the tile
    // loop computes where it is used): left per-lane, each row and weight address is a loop-invariant register pair that
    // hipcc hoists out of the tile loop, and together they do not fit next to the ring.
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, P = a.P;
    const int NT = a.Cout >> 4;
    const int ntile = (P + 63) >> 6;
    const int tw0 = ((int)blockIdx.z * 4 + wave) * tpw;                   // this wave's first output tile (blockIdx.z: output-channel split of small launches)
    const float* xb = a.x1 + (size_t)b * a.x1_bstride;
    float* outb = a.out + (size_t)b * a.out_bstride;
    const char* wp3 = reinterpret_cast<const char*>(reinterpret_cast<const float*>(a.wp3) + (size_t)b * a.wp3_bstride);
    const unsigned aoff = 16u * (unsigned)lane;                           // the lane's 16 bytes of a 64-lane weight piece

    // ---- input tile: wave w holds K blocks [w KPW, (w + 1) KPW), lane (j, kq) channels 8 kq .. 8 kq + 7 of each, 4 pixels.
    // Persistent over pixel tiles with the next tile's x in flight behind the GEMM of this one (without that the kernel ran
    // at HBM time + MFMA time: all workgroups load, then all multiply).
    const int kb0 = KB >= 4 ? wave * KPW : wave >> 1;                     // this wave's first K block
    const int cwave = KB >= 4 ? 0 : 4 * (wave & 1);                       // the wave's part of ...
    const int cbase = 8 * kq + cwave;                                     // ... the first of the lane's CPT channels inside a block
    float4 xr[KPW][CPT];
    auto load_x = [&](int tile, bool exists) {      // lanes past the end of the image take the tile's first pixel group
        const int q0 = tile * 64 + 4 * j;
        size_t xoff = exists ? (size_t)(8 * kq) * (size_t)P + (size_t)(q0 < P ? q0 : tile * 64) : (size_t)0;
        asm volatile("" : "+v"(xoff));              // computed here, once per tile
#pragma unroll
        for (int i = 0; i < KPW; ++i)
#pragma unroll
            for (int c = 0; c < CPT; ++c) xr[i][c] = *reinterpret_cast<const float4*>(xb + (size_t)(32 * (kb0 + i) + cwave + c) * (size_t)P + xoff);
    };
    u32x4 A[RING][3];
    auto load_a = [&](int slot, int step, int t0) {
        const int kb = step / NCO, t = step - kb * NCO;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
            A[slot][pc] = *reinterpret_cast<const u32x4*>(wp3 + (((size_t)kb * NT + t0 + t) * 192 + pc * 64) * 16 + aoff);
    };
    load_x(blockIdx.x, true);
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) load_a(i, i, tw0);
    // gamma and beta of the lane's channels, in registers for all tiles -- except at K = 128, where 16 more registers next
    // to the ring spill: there every tile loads them again after its statistics, and THAT wait covers the stores of the
    // tile before (issued two barriers earlier)
    constexpr bool LNREG = KB != 4;
    float gam[LNREG ? KPW : 1][CPT], bet[LNREG ? KPW : 1][CPT];
    if constexpr (LNREG) {
#pragma unroll
        for (int i = 0; i < KPW; ++i)
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                const int k = 32 * (kb0 + i) + cbase + c;
                gam[i][c] = a.ln_w[k];
                bet[i][c] = a.ln_b ? a.ln_b[k] : 0.f;
            }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);    // vmcnt(0): the loop is entered with nothing of the prologue pending, as from its own back edge

    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int tnext = tile + (int)gridDim.x;
    const bool more = tnext < ntile;
    const int q0 = tile * 64 + 4 * j;
    const int p0 = q0 < P ? q0 : tile * 64;
    // two-pass statistics: lanes, then waves (fixed order)
    float mean[4], rstd[4];
    {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KPW; ++i)
#pragma unroll
            for (int c = 0; c < CPT; ++c) { s[0] += xr[i][c].x; s[1] += xr[i][c].y; s[2] += xr[i][c].z; s[3] += xr[i][c].w; }
#pragma unroll
        for (int g = 0; g < 4; ++g) { s[g] += __shfl_xor(s[g], 16); s[g] += __shfl_xor(s[g], 32); }
        if (kq == 0) *reinterpret_cast<float4*>(red + wave * 64 + 4 * j) = make_float4(s[0], s[1], s[2], s[3]);
        __syncthreads();
        const float4 r0 = *reinterpret_cast<const float4*>(red + 4 * j), r1 = *reinterpret_cast<const float4*>(red + 64 + 4 * j);
        const float4 r2 = *reinterpret_cast<const float4*>(red + 128 + 4 * j), r3 = *reinterpret_cast<const float4*>(red + 192 + 4 * j);
        mean[0] = (((r0.x + r1.x) + r2.x) + r3.x) * (1.0f / K); mean[1] = (((r0.y + r1.y) + r2.y) + r3.y) * (1.0f / K);
        mean[2] = (((r0.z + r1.z) + r2.z) + r3.z) * (1.0f / K); mean[3] = (((r0.w + r1.w) + r2.w) + r3.w) * (1.0f / K);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KPW; ++i)
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                const float d0 = xr[i][c].x - mean[0], d1 = xr[i][c].y - mean[1], d2 = xr[i][c].z - mean[2], d3 = xr[i][c].w - mean[3];
                v[0] = fmaf(d0, d0, v[0]); v[1] = fmaf(d1, d1, v[1]); v[2] = fmaf(d2, d2, v[2]); v[3] = fmaf(d3, d3, v[3]);
            }
#pragma unroll
        for (int g = 0; g < 4; ++g) { v[g] += __shfl_xor(v[g], 16); v[g] += __shfl_xor(v[g], 32); }
        if (kq == 0) *reinterpret_cast<float4*>(red + 256 + wave * 64 + 4 * j) = make_float4(v[0], v[1], v[2], v[3]);
        __syncthreads();
        const float4 q0 = *reinterpret_cast<const float4*>(red + 256 + 4 * j), q1 = *reinterpret_cast<const float4*>(red + 320 + 4 * j);
        const float4 q2 = *reinterpret_cast<const float4*>(red + 384 + 4 * j), q3 = *reinterpret_cast<const float4*>(red + 448 + 4 * j);
        rstd[0] = 1.0f / sqrtf((((q0.x + q1.x) + q2.x) + q3.x) * (1.0f / K) + a.ln_eps);
        rstd[1] = 1.0f / sqrtf((((q0.y + q1.y) + q2.y) + q3.y) * (1.0f / K) + a.ln_eps);
        rstd[2] = 1.0f / sqrtf((((q0.z + q1.z) + q2.z) + q3.z) * (1.0f / K) + a.ln_eps);
        rstd[3] = 1.0f / sqrtf((((q0.w + q1.w) + q2.w) + q3.w) * (1.0f / K) + a.ln_eps);
    }
    // normalise, split into three bf16 pieces, publish in B-operand order
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const int kb = kb0 + i;
        unsigned bpd[4][3][CPT / 2];              // [pixel][piece][channel pair]
#pragma unroll
        for (int hp = 0; hp < CPT / 2; ++hp) {
            const int k = 32 * kb + cbase + 2 * hp;
            const float ga = LNREG ? gam[LNREG ? i : 0][2 * hp] : a.ln_w[k], gb = LNREG ? gam[LNREG ? i : 0][2 * hp + 1] : a.ln_w[k + 1];
            const float ba = LNREG ? bet[LNREG ? i : 0][2 * hp] : a.ln_b ? a.ln_b[k] : 0.f, bb = LNREG ? bet[LNREG ? i : 0][2 * hp + 1] : a.ln_b ? a.ln_b[k + 1] : 0.f;
            const float xa[4] = {xr[i][2 * hp].x, xr[i][2 * hp].y, xr[i][2 * hp].z, xr[i][2 * hp].w};
            const float xc[4] = {xr[i][2 * hp + 1].x, xr[i][2 * hp + 1].y, xr[i][2 * hp + 1].z, xr[i][2 * hp + 1].w};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float mu = a.ln_b ? mean[g] : 0.f;     // BiasFree_LayerNorm scales x, not x - mean
                b3_split_pair(fmaf((xa[g] - mu) * rstd[g], ga, ba), fmaf((xc[g] - mu) * rstd[g], gb, bb), bpd, g, hp);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) {
                u32x4* dst = &Bl[((kb * 4 + g) * 3 + pc) * 64 + lane];
                if constexpr (CPT == 8) *dst = (u32x4){bpd[g][pc][0], bpd[g][pc][1], bpd[g][pc][2], bpd[g][pc][3]};
                else reinterpret_cast<uint2*>(dst)[wave & 1] = make_uint2(bpd[g][pc][0], bpd[g][pc][1]);   // this wave's half of the element
            }
    }
    __syncthreads();
    if constexpr (RESIDENT) load_x(tnext, more);
    unsigned soff = 4u * ((unsigned)(4 * kq) * (unsigned)P + (unsigned)p0);     // channel 4 kq of an output tile, the lane's pixels: bytes
    asm volatile("" : "+v"(soff));

    // ---- output tiles of this wave, one chunk of NCO at a time; LAST: the tile's last chunk, which also fetches for the next tile
    auto run_chunk = [&](const int t0, auto last_chunk) {
        constexpr bool LAST = decltype(last_chunk)::value;
        f32x4 acc[NCO][4];
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // B pieces from LDS, double-buffered per K block: the 12 reads of block kb + 1 are spread over the NCO steps of block kb
        u32x4 bp[2][4][3];
        auto load_b = [&](int buf, int kb, int first, int last) {
#pragma unroll
            for (int i = first; i < last; ++i) bp[buf][i / 3][i % 3] = Bl[(kb * 12 + i) * 64 + lane];
        };
        load_b(0, 0, 0, 12);
#pragma unroll
        for (int step = 0; step < STEPS; ++step) {
            const int kb = step / NCO, t = step % NCO;
            if constexpr (!RESIDENT) {
                if (step + RING - 1 < STEPS) load_a((step + RING - 1) % RING, step + RING - 1, t0);
                if (LAST && step == XSTEP) {
                    __builtin_amdgcn_sched_barrier(0);
                    load_x(tnext, more);
                }
            }
            if (kb + 1 < KB) load_b((kb + 1) & 1, kb + 1, 12 * t / NCO, 12 * (t + 1) / NCO);
            b3_mfma4(A[step % RING], bp[kb & 1], acc[t]);
            __builtin_amdgcn_sched_barrier(0);      // keep the ring: without it hipcc hoists every load to the top and spills
        }
        if constexpr (!RESIDENT) {                  // loads before stores: the ring and both B buffers are dead here
#pragma unroll
            for (int i = 0; i < RING - 1; ++i) load_a(i, i, LAST ? tw0 : t0 + NCO);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the stores (epilogue<NCO, false>'s arithmetic in mode 0; every channel exists: Cout % 64 == 0), every lane, straight-line:
        // the row in scalar registers + the lane's byte offset (at most 52 P: plan_conv1x1 keeps 64 P below 4e9)
#pragma unroll
        for (int t = 0; t < NCO; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float bs = bias_l[16 * (t0 + t) + 4 * kq + r];
                float v[4] = {acc[t][0][r] + bs, acc[t][1][r] + bs, acc[t][2][r] + bs, acc[t][3][r] + bs};
                if (a.act == 1 || a.act == 3) {
                    const float slope = a.act == 1 ? 0.2f : 0.1f;
#pragma unroll
                    for (int g = 0; g < 4; ++g) v[g] = v[g] > 0.f ? v[g] : slope * v[g];
                } else if (a.act == 2) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) v[g] = fmaxf(v[g], 0.f);
                } else if (a.act == 4) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) v[g] = fminf(fmaxf(v[g], 0.f), 1e4f);
                }
                *reinterpret_cast<float4*>(reinterpret_cast<char*>(outb + (size_t)(16 * (t0 + t) + r) * (size_t)P) + soff) = make_float4(v[0], v[1], v[2], v[3]);
            }
    };
    if constexpr (!RESIDENT)
        for (int t0 = tw0; t0 + NCO < tw0 + tpw; t0 += NCO) run_chunk(t0, std::false_type{});
    run_chunk(tw0 + tpw - NCO, std::true_type{});
    }   // pixel tiles (the first barrier of the next tile's statistics also frees Bl)
}

template <int KB, int NCO>
__global__ void __launch_bounds__(256, KB <= 4 ? 2 : 1) conv1x1_b3_ln_kernel(Conv1x1Args a, int tpw) {
    __shared__ __attribute__((aligned(16))) u32x4 Bl[KB * 768];
    __shared__ __attribute__((aligned(16))) float red[2 * 4 * 64];
    __shared__ float bias_l[1024];
    for (int i = threadIdx.x; i < a.Cout; i += 256) bias_l[i] = a.bias ? a.bias[i] : 0.f;
    if constexpr (KB == 2) {     // tpw is wave-uniform (a kernel argument)
        if (tpw == NCO) return b3_ln_tiles<KB, NCO, true>(a, tpw, Bl, red, bias_l);
    }
    b3_ln_tiles<KB, NCO, false>(a, tpw, Bl, red, bias_l);
}

// ---------------------------------------------------------------------------------------------
// Ragged shapes (P % 4 != 0, unaligned views): one thread per output pixel and channel, plain
// FMA over K with a two-pass LayerNorm.  Correctness path only: tiny odd test frames (a RawFormer level always has
// an even width and a pixel count divisible by 4 except at 1-2 pixel extents).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv1x1_scalar_kernel(Conv1x1Args a) {
    const int P = a.P, K = a.C1 + a.C2, NT = (a.Cout + 15) >> 4;
    const int b = blockIdx.y;
    const float* wp = a.wp + (size_t)b * a.wp_bstride;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
        auto xat = [&](int k) {
            return (k < a.C1) ? a.x1[(size_t)b * a.x1_bstride + (size_t)k * P + p]
                              : a.x2[(size_t)b * a.x2_bstride + (size_t)(k - a.C1) * P + p];
        };
        float mu = 0.f, rstd = 1.f;
        if (a.ln_w) {
            for (int k = 0; k < K; ++k) mu += xat(k);
            mu /= (float)K;
            float var = 0.f;
            for (int k = 0; k < K; ++k) { const float d = xat(k) - mu; var = fmaf(d, d, var); }
            rstd = 1.0f / sqrtf(var / (float)K + a.ln_eps);
            if (!a.ln_b) mu = 0.f;
        }
        for (int co = 0; co < a.Cout; ++co) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) {
                float xv = xat(k);
                if (a.ln_w) xv = fmaf((xv - mu) * rstd, a.ln_w[k], a.ln_b ? a.ln_b[k] : 0.f);
                s = fmaf(wp[((size_t)(k >> 2) * NT + (co >> 4)) * 64 + (co & 15) + 16 * (k & 3)], xv, s);
            }
            if (a.mode == 0) {
                s += a.bias ? a.bias[co] : 0.f;
                if (a.res) s += a.res[(size_t)b * a.res_bstride + (size_t)co * P + p];
                if (a.act == 1) s = s > 0.f ? s : 0.2f * s;
                else if (a.act == 2) s = fmaxf(s, 0.f);
                else if (a.act == 3) s = s > 0.f ? s : 0.1f * s;
                else if (a.act == 4) s = fminf(fmaxf(s, 0.f), 1e4f);
                a.out[(size_t)b * a.out_bstride + (size_t)co * P + p] = s;
            } else {
                const int o = co >> 2, y = p / a.w, x = p - y * a.w;
                s += a.bias ? a.bias[o] : 0.f;
                a.out[(size_t)b * a.out_bstride + (size_t)o * 4 * P + (size_t)(2 * y + ((co >> 1) & 1)) * (2 * a.w) + 2 * x + (co & 1)] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host side.  Every instantiation that can be launched is one row of kInst: the row's text is both the launch and the
// profiler key (= the kernel name a trace shows), so the two cannot drift apart.
enum { kScalar, kRes, kStream, kB3, kB3Ln };
struct Conv1x1Inst {
    const char* key;
    int family, targ[4];     // the template arguments as integers, in order (absent ones zero)
    unsigned block;
    void (*launch)(const Conv1x1Args&, const Conv1x1Plan&, hipStream_t);
};
#define RF_GRID dim3(p.grid[0], p.grid[1], p.grid[2]), p.block, p.lds, st
#define RF_INST(FAMILY, BLOCK, KERNEL, KARGS, ...)                                      \
    {#KERNEL "<" #__VA_ARGS__ ">", FAMILY, {__VA_ARGS__}, BLOCK,                        \
     [](const Conv1x1Args& a, const Conv1x1Plan& p, hipStream_t st) { KERNEL<__VA_ARGS__><<<RF_GRID>>> KARGS; }}
#define RF_RES(...) RF_INST(kRes, 256, conv1x1_res_kernel, (a, p.karg[0], p.karg[1]), __VA_ARGS__)          // <KS, LN, RT, DBUF>(ntw, ngroups)
#define RF_RES6(KS, DBUF4) /* K <= 64: LayerNorm or not, 0 / 2 / 4 residual tiles in registers */             \
    RF_RES(KS, true, 4, DBUF4), RF_RES(KS, false, 4, DBUF4), RF_RES(KS, true, 2, true), RF_RES(KS, false, 2, true), RF_RES(KS, true, 0, true), RF_RES(KS, false, 0, true)
#define RF_STREAM(...) RF_INST(kStream, 256, conv1x1_stream_kernel, (a, p.karg[0]), __VA_ARGS__)            // <NCO, KCH, LN>(ngroups)
#define RF_B3(BLOCK, ...) RF_INST(kB3, BLOCK, conv1x1_b3_kernel, (a, p.karg[0]), __VA_ARGS__)               // <NCO, LN[, PAIR]>(ngroups)
#define RF_B3LN(...) RF_INST(kB3Ln, 256, conv1x1_b3_ln_kernel, (a, p.karg[0]), __VA_ARGS__)                 // <KB, NCO>(tpw)
// (rows in the order the code object has always held its kernels)
static const Conv1x1Inst kInst[] = {
    {"conv1x1_scalar_kernel", kScalar, {}, 256, [](const Conv1x1Args& a, const Conv1x1Plan& p, hipStream_t st) { conv1x1_scalar_kernel<<<RF_GRID>>>(a); }},
    RF_B3LN(2, 3), RF_B3LN(2, 2), RF_B3LN(4, 3), RF_B3LN(4, 2), RF_B3LN(8, 4), RF_B3LN(8, 3), RF_B3LN(8, 2),
    // the unpaired key names the family by its first two arguments (bench.py's lookup covers <.., false, false> with it); the
    // paired form has a key of its own, so a profile shows which form a launch took
    RF_B3(512, 6, false, true), RF_B3(512, 4, false, true), RF_B3(256, 6, false), RF_B3(256, 2, false), RF_B3(256, 4, true), RF_B3(256, 4, false),
    // four residual tiles next to a whole [K x 64 px] tile in flight do not fit at K > 32: those load the next tile late (no
    // DBUF).  With K <= 32 or a LayerNorm prologue the four-tile forms spill and plan_conv1x1 never asks for them; they stay
    // in the table (and in the code object) as they were.
    RF_RES6(4, true), RF_RES6(8, true), RF_RES6(12, false), RF_RES6(16, false),
    RF_RES(24, false, 0, false), RF_RES(32, false, 0, false),
    RF_STREAM(8, 4, true), RF_STREAM(8, 4, false), RF_STREAM(4, 8, true), RF_STREAM(4, 8, false),
};
#undef RF_GRID

// the row of `family` whose first template arguments are t0, t1, t2 (-1: any); a kernel that is not there is an error
static int find_inst(int family, int t0, int t1, int t2, Conv1x1Plan* p) {
    const int want[3] = {t0, t1, t2};
    for (const Conv1x1Inst& r : kInst) {
        bool ok = r.family == family;
        for (int k = 0; k < 3; ++k) ok = ok && (want[k] < 0 || want[k] == r.targ[k]);
        if (ok) { p->inst = (int)(&r - kInst); p->key = r.key; p->block = r.block; return RF_OK; }
    }
    RF_CHECK_ARG(false, "conv1x1: no kernel instantiation for family %d <%d, %d, %d>", family, t0, t1, t2);
}

static bool b3_ln_supported(const Conv1x1Args& a, int* nco) {
    const int K = a.C1 + a.C2;
    if (!(a.ln_w && a.wp3 && a.C2 == 0 && (K == 64 || K == 128 || K == 256) && a.mode == 0 && !a.res && a.Cout % 64 == 0 && a.Cout <= 1024 &&
          aligned16(a.wp3) && a.wp3_bstride % 4 == 0))
        return false;
    const int tpw = a.Cout / 64;
    // K = 128 runs two workgroups per CU (256 registers): 4 tiles at once plus the next pixel tile in flight would spill
    *nco = (K == 256 && tpw % 4 == 0) ? 4 : tpw % 3 == 0 ? 3 : tpw % 2 == 0 ? 2 : 0;
    return *nco != 0;
}

// shapes the b3 kernel takes: K-blocks of 32 channels must not straddle the two sources; K < 128 stays on the resident-input
// f32 kernels, which read x once whatever Cout is and are HBM-bound there (measured per shape with tools/kbench.py:
// b3 wins 1.05-1.4 x from K = 128 up, loses 0.75-0.95 x at K = 64)
static bool b3_supported(const Conv1x1Args& a) {
    const int K = a.C1 + a.C2 + a.C3;
    return K >= 128 && a.C1 % 8 == 0 && a.C2 % 8 == 0 && a.C3 % 8 == 0 && (a.C2 + a.C3 == 0 || a.C1 % 32 == 0) &&
           (a.C3 == 0 || a.C2 % 32 == 0) && (!a.ln_w || (K <= kStreamLnMaxK && a.C3 == 0)) && aligned16(a.wp3) && (a.wp3_bstride % 4 == 0);
}

// THE selection rule (summary at the top of this file): argument checks, then the family in the order scalar, b3_ln, b3, res,
// stream, and inside a family the template arguments and the grid.  No HIP call, no launch; a plan exists only for arguments
// launch_conv1x1 accepts.
int plan_conv1x1(const Conv1x1Args& a, Conv1x1Plan* p, const Conv1x1Dw3* dw3) {
    bool b3_ok = a.wp3 != nullptr;
    int force_pair = -1;      // -1: by launch size
    int force_dw3 = -1;
#ifdef RF_DIAG   // diagnostic build only (build.py --diag): RF_NO_B3 forces the f32 MFMA kernels; RF_B3_PAIR=1 takes the paired form at any launch size, =0 never; RF_TAIL_DW likewise for the on-the-fly third source
    if (getenv("RF_NO_B3")) b3_ok = false;
    if (const char* e = getenv("RF_B3_PAIR")) force_pair = e[0] != '0';
    if (const char* e = getenv("RF_TAIL_DW")) force_dw3 = e[0] != '0';
#endif
    RF_CHECK_ARG(a.B > 0 && a.P > 0 && a.C1 > 0 && a.C2 >= 0 && a.Cout > 0, "conv1x1: bad sizes B=%d P=%d C1=%d C2=%d Cout=%d",
                 a.B, a.P, a.C1, a.C2, a.Cout);
    RF_CHECK_ARG(a.C1 % 4 == 0 && a.C2 % 4 == 0, "conv1x1: input channel counts (%d, %d) must be multiples of 4", a.C1, a.C2);
    RF_CHECK_ARG(a.C2 == 0 || a.x2 != nullptr, "conv1x1: second source missing");
    RF_CHECK_ARG(a.C3 >= 0 && a.C3 % 4 == 0 && (a.C3 == 0 || (a.x3 != nullptr && a.C2 > 0)), "conv1x1: bad third source (C3 = %d)", a.C3);
    RF_CHECK_ARG(a.mode == 0 || (a.Cout % 4 == 0 && a.w > 0 && a.P % a.w == 0 && !a.res), "conv1x1: bad ConvTranspose geometry");
    RF_CHECK_ARG(a.B <= 65535 && (double)a.P * 4.0 * 16.0 < 4.0e9, "conv1x1: batch %d / plane %d too large", a.B, a.P);
    const int K = a.C1 + a.C2 + a.C3;
    const int NS = K / 4, NT = cdiv(a.Cout, 16);
    const int ptiles = cdiv(a.P, 256);                    // 256-pixel tiles of an image
    const long units = (long)ptiles * a.B;
    bool vec = (a.P % 4 == 0) && aligned16(a.x1) && aligned16(a.out) && (a.x1_bstride % 4 == 0) && (a.out_bstride % 4 == 0);
    if (a.x2) vec = vec && aligned16(a.x2) && (a.x2_bstride % 4 == 0);
    if (a.C3) vec = vec && aligned16(a.x3) && (a.x3_bstride % 4 == 0);
    if (a.res) vec = vec && aligned16(a.res) && (a.res_bstride % 4 == 0);
    if (a.mode == 1) vec = vec && (a.w % 2 == 0);
    const bool ln = a.ln_w != nullptr;
    const double px = (double)a.B * a.P;
    *p = Conv1x1Plan{};
    p->flops = 2.0 * K * a.Cout * px;
    p->bytes = 4.0 * px * (K + a.Cout + (a.res ? a.Cout : 0));
    p->grid[1] = (unsigned)a.B; p->grid[2] = 1;
    int nco_ln = 0;
    const bool ln_once = b3_ln_supported(a, &nco_ln);      // the split-once bf16x3 kernel takes this shape
    // Does the LayerNorm prologue read x once?  Yes on the split-once bf16x3 kernel and on the resident-input kernels (K <= 64).
    // The streaming kernels re-read and re-normalise their pixels once per group of 64-96 output channels (RawFormer-L level 3,
    // K = 512 -> 1536: 24 passes, 0.77 ms for a 0.2 ms product; every level of RawFormer-B): their callers run layernorm2d first
    // and the plain GEMM on its output (rf_block.hip).  A property of the shape: the same on ragged frames and under RF_NO_B3.
    p->ln_single_pass = !ln || a.C1 + a.C2 <= 64 || ln_once;
    const bool use_b3 = b3_ok && b3_supported(a);
    // three sources exist for the bf16x3 streaming kernel only (its caller checks the shape; there is no slower form to fall to)
    RF_CHECK_ARG(a.C3 == 0 || (use_b3 && vec && !a.ln_w && !(a.res && a.Cout % 16 != 0)), "conv1x1: three sources need the bf16x3 kernel (K = %d, P = %d)", K, a.P);
    if (!vec || (a.res && a.Cout % 16 != 0) || (ln && K > kStreamLnMaxK)) {
        p->grid[0] = (unsigned)(cdiv(a.P, 256) < 4096 ? cdiv(a.P, 256) : 4096);
        return find_inst(kScalar, -1, -1, -1, p);
    }
    if (b3_ok && ln_once) {
        const int kb = K / 32;
        int tpw = a.Cout / 64;
        const int slots = (kb <= 4 ? 2 : 1) * 256;                // resident workgroups (LDS: 31 / 55 / 104 KB; registers: 2 per CU)
        int gx = slots / a.B;
        gx = gx < 1 ? 1 : gx;
        gx = gx < cdiv(a.P, 64) ? gx : cdiv(a.P, 64);
        // one small frame (levels 2-3: 4-64 pixel tiles): a workgroup's waves walk tpw / NCO chunks of output tiles one after the
        // other, each a chain of K-block steps -- split the output channels over blockIdx.z (every workgroup normalises its
        // 64 pixels again: K x 64 values) until the launch has a few hundred workgroups.  Same arithmetic per output: same bits.
        int zs = 1;
        if ((long)gx * a.B < 128)
            for (int z = tpw / nco_ln; z > 1; --z)
                if ((tpw / nco_ln) % z == 0 && (long)gx * a.B * z <= 512) { zs = z; break; }
        p->grid[0] = (unsigned)gx; p->grid[2] = (unsigned)zs;
        p->karg[0] = tpw / zs;
        return find_inst(kB3Ln, kb, nco_ln, -1, p);
    }
    if (use_b3) {
        // 6 tiles per workgroup where that divides the output evenly; never with the LayerNorm prologue (that instantiation
        // needs 2 registers more than the 256 a wave has at two waves per SIMD)
        int nco = (!ln && (NT % 6 == 0 || (NT % 4 != 0 && NT > 8))) ? 6 : 4;
        // Third source on the fly (conv1x1_b3_dw3_kernel): ONE output group of four tiles (two groups would both repeat the
        // stencil), workgroups of 4 rows x 64 columns that tile the image exactly, and a launch of at least 512 such units: a
        // smaller one leaves CUs idle either way and has no HBM time to save (RF_TAIL_DW=1: any size the kernel supports).
        if (dw3 && force_dw3 != 0 && !ln && !a.res && a.mode == 0 && nco == 4 && NT == 4 && a.Cout == 64 && a.C3 > 0 && a.C3 <= kDw3MaxC3 &&
            a.C1 % 32 == 0 && a.C2 % 32 == 0 && a.C3 % 32 == 0 && dw3->w && dw3->h > 0 && dw3->w_ > 0 && (long)dw3->h * dw3->w_ == a.P &&
            dw3->w_ % 64 == 0 && dw3->h % 4 == 0 && (double)a.C3 * a.P < 4.0e9 && (force_dw3 == 1 || units >= 512)) {
            p->dw3 = true;
            p->inst = -1; p->key = "conv1x1_b3_kernel<4, false, dw3>"; p->block = 256;
            p->grid[0] = (unsigned)ptiles;
            p->flops += 18.0 * a.C3 * px;      // the stencil, counted as launch_dwconv3x3 counts it; bytes: every source once, as above
            return RF_OK;
        }
        // Paired form (two output groups per 512-thread workgroup, the pairs of a pixel tile on one XCD): x is fetched once per
        // pixel tile instead of once per group.  It halves the workgroup count, so it is taken where every CU still gets one;
        // smaller launches keep the unpaired form and the rule below.
        const bool pair = !ln && cdiv(NT, nco) > 1 && (force_pair >= 0 ? force_pair != 0 : units * cdiv(cdiv(NT, nco), 2) >= 256);
        // one frame at levels 2-3: fewer than 256 workgroups -- two output tiles per workgroup instead of four fills more CUs
        if (!pair && !ln && nco == 4 && NT % 2 == 0 && units * cdiv(NT, 4) < 256) nco = 2;
        const int ngroups = cdiv(NT, nco);
        // the flat grid of the paired form: whole chunks of 8 units x pairs (conv1x1_group_grid), as one 32-bit workgroup id
        const long pair_ids = (units + 7) / 8 * 8 * cdiv(ngroups, 2);
        RF_CHECK_ARG(!pair || pair_ids < (1L << 31), "conv1x1: %ld pixel tiles x %d output groups is too large a grid", units, ngroups);
        p->karg[0] = ngroups;
        if (pair) { p->grid[0] = conv1x1_group_grid((unsigned)units, (unsigned)cdiv(ngroups, 2)); p->grid[1] = 1; }
        else p->grid[0] = (unsigned)(ptiles * ngroups);
        return find_inst(kB3, nco, ln, pair, p);
    }
    if (NS <= 16 || (NS <= 32 && !ln && !a.res)) {
        const int ks = NS <= 4 ? 4 : NS <= 8 ? 8 : NS <= 12 ? 12 : NS <= 16 ? 16 : NS <= 24 ? 24 : 32;
        // output tiles per workgroup: weight slice <= ~60 KB, and <= 8 tiles when the residual rows
        // are prefetched into registers
        int cap = (240 / ks) & ~1;
        if (a.res && cap > 4) cap = 4;
        // the four-residual-tile instantiations with K <= 32 or a LayerNorm prologue spill (28-296 bytes of scratch) next to
        // their prefetched loads: such shapes (no layer of RawFormer; reachable through rf_conv1x1) take two tiles per workgroup
        if (a.res && (ks <= 8 || ln) && cap > 2) cap = 2;
        const int ntw = NT < cap ? NT : cap;
        const int ngroups = cdiv(NT, ntw);
        const int tpad = cdiv(ntw, 2) * 2;
        p->lds = ((size_t)ks * tpad * 64 + tpad * 16 + 8 * ks) * sizeof(float);
        // persistent workgroups: enough to fill every CU at this kernel's occupancy, split over the images
        const int slots = 256 * (ks <= 8 ? 3 : 2);
        int wgs = cdiv(slots, a.B * ngroups);
        if (wgs > ptiles) wgs = ptiles;
        p->grid[0] = (unsigned)(wgs * ngroups);
        p->karg[0] = ntw; p->karg[1] = ngroups;
        return find_inst(kRes, ks, ln, a.res ? (ntw > 2 ? 4 : 2) : 0, p);      // residual tiles held in registers
    }
    // accumulator tiles per workgroup: 8 (128 channels) unless that would be mostly padding -- or unless the grid
    // would fill the 512 resident workgroup slots badly (level 3 of config 2: 256 or 768 workgroups = half-empty
    // rounds); 4 tiles per workgroup double the grid.  The k order per output is the same either way (same bits).
    int nco = (NT % 8 == 0 || NT > 12) ? 8 : 4;
    if (nco == 8) {
        const long cost8 = ((units * cdiv(NT, 8) + 511) / 512) * 8, cost4 = ((units * cdiv(NT, 4) + 511) / 512) * 4;
        if (cost4 < cost8) nco = 4;
    }
    p->karg[0] = cdiv(NT, nco);
    p->grid[0] = (unsigned)(ptiles * p->karg[0]);
    return find_inst(kStream, nco, -1, ln, p);
}

bool conv1x1_ln_single_pass(const Conv1x1Args& a) {
    Conv1x1Plan p;
    return plan_conv1x1(a, &p) != RF_OK || p.ln_single_pass;      // arguments without a plan: launch_conv1x1 reports them
}

int launch_conv1x1(const Conv1x1Args& a, hipStream_t st, const Conv1x1Dw3* dw3) {
    Conv1x1Plan p;
    RF_TRY(plan_conv1x1(a, &p, dw3));
    // no other kernel applies the stencil: the caller asks the plan first and runs launch_dwconv3x3 itself where this is false
    RF_CHECK_ARG(!dw3 || p.dw3, "conv1x1: no kernel produces source 3 on the fly for this shape (K = %d, Cout = %d, P = %d)", a.C1 + a.C2 + a.C3, a.Cout, a.P);
    {
        ProfScope prof(st, p.key, p.flops, p.bytes);
        if (p.dw3) RF_TRY(launch_conv1x1_b3_dw3(a, *dw3, p, st));
        else kInst[p.inst].launch(a, p, st);
    }
    return check_launch("conv1x1");
}

}  // namespace rf
