// Fused transformer-block kernels for U-Net levels 0-2.  Built: ffn_fused_kernel<32, false> and attn_front_kernel<32> (four
// waves, level 0 of RawFormer-S), ffn_fused8_kernel<48> / <64> (eight waves; <64> is built and tested but never dispatched, see
// fused_ffn_supported); attn_mid_kernel<64> / <128> (levels 1-2, where the qkv 1x1 stays a separate GEMM) is built by
// rf_attn_mid.hip.  The three kernels with a phase A (both FFN kernels and attn_front) share group_geom, split_step,
// phase_a_step_b3 and tile_range; all four share stencil4, and ffn_fused8_kernel and attn_front_kernel tile_origin.  Every helper is __forceinline__, and tools/isa_same.py shows whether an edit to one
// of them left the compiled code alone.  The helpers and ffn_fused_kernel live in rf_fused_tile.h: rf_fused_tail.hip builds the
// second instantiation, ffn_fused_kernel<32, true>, which a whole-model stage uses at level 0 -- the FFN with the stage's
// channel_reduce on top (FfnTail, rf_common.h), launched from here by launch_ffn_fused; rf_fused_proj.hip the third,
// <32, true, FfnProj>, with the attention projection ahead of it (FfnProj; fused_ffn_proj_rule).  rf_attn_front_tall.hip builds
// attn_front_tall_kernel<32>, attn_front on tiles of 12 rows and eight waves, which launch_attn_front takes above 256 x 256.
//
// Un-fused, one TransformerBlock moves ~26 C floats per pixel through HBM (qkv 1x1: C in / 3C out,
// depthwise 3x3: 3C/3C, Gram: 2C, ...; ffn: C/2C, 2C/2C, 2C+C/C).  Here the wide intermediates
// (qkv before/after the depthwise conv, the FFN hidden tensor) never leave the CU:
//
//   ffn_fused_kernel    x1 -> LN2 -> 1x1 (C->2C) -> dw3x3 -> GELU -> 1x1 (2C->C) + x1      reads C, writes C
//     ... <32, true>    the same, then channel_reduce(cat(xs, .)): [xs ; x1 ; g] x [Wa' | Wb | Wb W2]    reads 2C, writes C
//     ... <32, true, FfnProj>   the same on x1 = x + Wf v + b, formed per tile (the attention projection)     reads 3C, writes C
//   attn_front_kernel   x  -> LN1 -> 1x1 (C->3C) -> dw3x3 -> { Gram partials of q,k ; v }   reads C, writes C
//
// Tile = 4 rows x 64 px per workgroup (4 waves, one output row each) plus a 1-pixel halo, held as
// 6 rows x 72 columns (columns x0-4 .. x0+67, so every 4-pixel group is 16-byte aligned in HBM and
// either wholly inside or wholly outside the image).
//   Phase A (per part of 32 intermediate channels): each wave owns 27 of the 108 halo'd pixel
//     groups as two MFMA steps; its LayerNorm'd input (C x 64 px per step) stays in registers for
//     all parts (the resident-input GEMM of rf_gemm1x1.hip), D tiles go to LDS (+bias, zero outside
//     the image: the depthwise conv pads ITS input, i.e. the 1x1 output).
//   Phase B: a lane reads the 3x6 neighbourhood of its 4 pixels from LDS, runs the 9-tap stencil
//     in registers and feeds the result straight into the next MFMA as B operand (FFN: second 1x1;
//     attention: q k^T, q q^T, k k^T with the pixel axis as K) or stores it (v).
// Weights of the current part are staged in LDS in MFMA lane order.  All cross-workgroup
// reductions go through fixed-order partials (bitwise reproducible).
#include <cstdio>
#include <cstdlib>
#include "rf_common.h"
#ifdef RF_STAMP
namespace rf { __device__ unsigned long long g_stamp[16]; }      // STAMP_FLUSH (rf_fused_tile.h) adds into it
#endif
#include "rf_fused_tile.h"

namespace rf {

// ================================================================================================
// The same FFN for C = 48 and C = 64 (level 0 of RawFormer-B / -L, level 1 of RawFormer-S) on EIGHT-wave workgroups, one per CU.
// Two steps of b3 pieces per wave (the C = 32 kernel) would need 192 registers at C = 64; here the 108 halo'd pixel groups are
// spread over eight waves -- 14 each, ONE phase-A step and 96 registers of pieces per wave -- and phase B splits the K dimension
// of the second GEMM instead of the pixels: waves 0-3 and 4-7 own the same four output rows, wave half `hf` runs the
// depthwise stencil + GELU and the MFMAs of k-steps [4 hf, 4 hf + 4) of every part (no stencil is evaluated twice), and the two
// partial accumulator sets are added through LDS once per tile (64 KB = the `mid` planes, free by then).  K of the first GEMM
// is padded to a multiple of 32 with zero pieces (C = 48: the packed weight is zero-padded the same way).
// LDS at C = 64: 64 KB mid / reduction + 48 KB W1 (b3) + 32 KB W2 + 6 KB of vectors = 150 KB.
// ================================================================================================
// input of one step, K padded to KP: lane (j, kq) holds channels 32 kb + 8 kq + i; channels >= C are zeros (loaded from a
// clamped address, selected away: the loads stay branch-free)
template <int C, int KP>
__device__ __forceinline__ void load_step_b3p(const float* __restrict__ xb, int P, int kq, const GroupGeom& g, float4 (&xh)[KP / 4]) {
#pragma unroll
    for (int s = 0; s < KP / 4; ++s) {
        const int ch = 32 * (s >> 3) + 8 * kq + (s & 7);
        xh[s] = *reinterpret_cast<const float4*>(xb + (size_t)(ch < C ? ch : 0) * P + (unsigned)g.goff);
    }
}

template <int C, int KP>
__device__ __forceinline__ void ln_step_b3p(int kq, const float* __restrict__ gam_l, const float* __restrict__ bet_l, float eps, float4 (&xh)[KP / 4]) {
    constexpr int NS = KP / 4;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bool ok = 32 * (s >> 3) + 8 * kq + (s & 7) < C;
        if (!ok) xh[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        sum[0] += xh[s].x; sum[1] += xh[s].y; sum[2] += xh[s].z; sum[3] += xh[s].w;
    }
    float mu[4], var[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum[q] += __shfl_xor(sum[q], 16);
        sum[q] += __shfl_xor(sum[q], 32);
        mu[q] = sum[q] * (1.0f / C);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float m = (32 * (s >> 3) + 8 * kq + (s & 7) < C) ? 1.0f : 0.f;
        const float d0 = m * (xh[s].x - mu[0]), d1 = m * (xh[s].y - mu[1]), d2 = m * (xh[s].z - mu[2]), d3 = m * (xh[s].w - mu[3]);
        var[0] = fmaf(d0, d0, var[0]); var[1] = fmaf(d1, d1, var[1]);
        var[2] = fmaf(d2, d2, var[2]); var[3] = fmaf(d3, d3, var[3]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        var[q] += __shfl_xor(var[q], 16);
        var[q] += __shfl_xor(var[q], 32);
        rstd[q] = 1.0f / sqrtf(var[q] * (1.0f / C) + eps);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int ch = 32 * (s >> 3) + 8 * kq + (s & 7);
        const bool ok = ch < C;
        const float gk = gam_l[ok ? ch : 0], bk = bet_l[ok ? ch : 0];
        xh[s].x = ok ? fmaf((xh[s].x - mu[0]) * rstd[0], gk, bk) : 0.f;
        xh[s].y = ok ? fmaf((xh[s].y - mu[1]) * rstd[1], gk, bk) : 0.f;
        xh[s].z = ok ? fmaf((xh[s].z - mu[2]) * rstd[2], gk, bk) : 0.f;
        xh[s].w = ok ? fmaf((xh[s].w - mu[3]) * rstd[3], gk, bk) : 0.f;
    }
}

template <int C>
__global__ void __launch_bounds__(512, 1) ffn_fused8_kernel(FfnArgs a) {
    using namespace fused;
    const int ro[3] = {0, HC, 2 * HC};   // a tile's halo'd rows are contiguous in LDS
    constexpr int KP = (C + 31) / 32 * 32; // K of the first GEMM, padded
    constexpr int NT1 = 2 * C / 16;      // output tiles of the first GEMM (hidden)
    constexpr int NTO = C / 16;          // output tiles of the second GEMM
    constexpr int NPART = 2 * C / PART;  // parts of 32 hidden channels
    constexpr int PS = 448;
    constexpr int MIDF = (PART * PS + 8 > NTO * 4 * 256 * 4) ? PART * PS + 8 : NTO * 4 * 256 * 4;      // planes, or the K-split reduction
    __shared__ __attribute__((aligned(16))) float mid[MIDF];
    __shared__ __attribute__((aligned(16))) u32x4 w1_l[(KP / 32) * NT1 * 192];
    __shared__ __attribute__((aligned(16))) float w2_l[(2 * C / 4) * NTO * 64];
    __shared__ float wd_l[2 * C * 9], bd_l[2 * C], b1_l[2 * C], b2_l[C], gam_l[C], bet_l[C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = wave & 3, hf = wave >> 2;
    const int b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    const float* xb = a.x + (size_t)b * C * P;
    float* ob = a.out + (size_t)b * C * P;

    for (int i = tid; i < (KP / 32) * NT1 * 192; i += 512) w1_l[i] = reinterpret_cast<const u32x4*>(a.w1p)[i];
    for (int i = tid; i < (2 * C / 4) * NTO * 16; i += 512) *reinterpret_cast<float4*>(w2_l + i * 4) = *reinterpret_cast<const float4*>(a.w2p + i * 4);
    for (int i = tid; i < 2 * C * 9; i += 512) wd_l[i] = a.wd[i];
    for (int i = tid; i < 2 * C; i += 512) { bd_l[i] = a.bd[i]; b1_l[i] = a.b1[i]; }
    for (int i = tid; i < C; i += 512) { gam_l[i] = a.ln_w[i]; bet_l[i] = a.ln_b[i]; b2_l[i] = a.b2[i]; }
    __syncthreads();

    const TileRange tr = tile_range(a.ntiles, a.tiles_x, (int)gridDim.x, blockIdx.x);
    const int j0 = lane & 15, kq0 = lane >> 4, lane0 = lane;
    for (int tile = tr.begin; tile < tr.end; ++tile) {
        const int2 o = tile_origin(tile, tr.tiles_y);
        const int x0 = o.x, y0 = o.y;
        // the lane coordinates are made opaque once per tile: everything derived from them (LDS plane / weight / stencil addresses)
        // would otherwise be hoisted out of the tile loop into long-lived registers and spilled (112 of them)
        int j = j0, kq = kq0, lane = lane0;
        asm volatile("" : "+v"(j), "+v"(kq), "+v"(lane));
        const GroupGeom gw = group_geom<GPW8>(wave, 0, j, y0, x0, h, w);
        u32x4 bp[KP / 32][4][3];
        {
            float4 xh[KP / 4];
            load_step_b3p<C, KP>(xb, P, kq, gw, xh);
            ln_step_b3p<C, KP>(kq, gam_l, bet_l, 1e-5f, xh);
            split_step<KP>(xh, bp);
        }
        const int yo = y0 + row, xo = x0 + 4 * j;            // this lane's 4 output pixels (both wave halves)
        const bool live = yo < h && xo < w;
        const unsigned voff = (unsigned)(4 * kq) * (unsigned)P + (unsigned)(live ? yo * w + xo : 0);
        f32x4 acc[NTO][4];
#pragma unroll
        for (int t = 0; t < NTO; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
        for (int part = 0; part < NPART; ++part) {
            lds_barrier();                                 // previous phase B (or the previous tile's reduction) is done with mid
            phase_a_step_b3<KP, NT1>(bp, w1_l + lane, 2 * part, 2 * part + 1, b1_l + part * PART, b1_l + part * PART + 16, mid, PS, kq, gw);
            lds_barrier();
            // ---- phase B: this wave half's four k-steps of the part (not unrolled: hoisted stencil loads would spill)
#pragma unroll 1
            for (int s4 = 0; s4 < PART / 8; ++s4) {
                const int s = 4 * hf + s4, hc = 4 * s + kq;
                float v[4];
                stencil4<Edge::Dpp>(mid + hc * PS + row * HC + 4 * j + 4, ro, j, wd_l + (part * PART + hc) * 9, bd_l[part * PART + hc], v);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = gelu_fast(v[q]);
#pragma unroll
                for (int t = 0; t < NTO; ++t) {
                    const float av = w2_l[((part * (PART / 4) + s) * NTO + t) * 64 + lane];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v[q], acc[t][q], 0, 0, 0);
                }
            }
        }
        // ---- the two K halves: waves 4-7 hand their accumulators to waves 0-3 through LDS (mid is free after the barrier)
        lds_barrier();
        float4* red = reinterpret_cast<float4*>(mid);
        if (hf == 1) {
#pragma unroll
            for (int t = 0; t < NTO; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[(t * 4 + q) * 256 + row * 64 + lane] = make_float4(acc[t][q][0], acc[t][q][1], acc[t][q][2], acc[t][q][3]);
        }
        float4 resv[NTO * 4];
        if (hf == 0) {                                     // residual rows, in flight across the barrier
#pragma unroll
            for (int t = 0; t < NTO; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) resv[t * 4 + r] = *reinterpret_cast<const float4*>(xb + (size_t)(16 * t + r) * P + voff);
        }
        lds_barrier();
        if (hf == 0) {
#pragma unroll
            for (int t = 0; t < NTO; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 o = red[(t * 4 + q) * 256 + row * 64 + lane];
                    acc[t][q][0] += o.x; acc[t][q][1] += o.y; acc[t][q][2] += o.z; acc[t][q][3] += o.w;
                }
            if (live) {
#pragma unroll
                for (int t = 0; t < NTO; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int cu = 16 * t + r;
                        const float bs = b2_l[cu + 4 * kq];
                        const float4 rv = resv[t * 4 + r];
                        *reinterpret_cast<float4*>(ob + (size_t)cu * P + voff) =
                            make_float4(acc[t][0][r] + bs + rv.x, acc[t][1][r] + bs + rv.y, acc[t][2][r] + bs + rv.z, acc[t][3][r] + bs + rv.w);
                    }
            }
        }
    }
}

// C = 64 is built and tested (diagnostic twin: RF_FFN8_64=1) but NOT dispatched: measured on MI355X the eight-wave kernel ties the
// op-by-op chain there (RawFormer-L level 0, 3 M pixels: 1.98 ms against 1.85 ms; RawFormer-S level 1: 0.33 against 0.30 ms) --
// at 64 channels the kernel is bound by MFMA + VALU issue (they do not overlap on this chip) where the chain is bound by HBM,
// and both take the same time.  C = 48 (RawFormer-B level 0) gains 8 % of its FFN.
static bool ffn_shape_ok(int C, int hidden, int h, int w, bool diag64) {
    return (C == 32 || C == 48 || (diag64 && C == 64)) && hidden == 2 * C && (w % 4 == 0) && ((double)C * h * w * 4.0 < 4.0e9);
}
static bool ffn_diag64() {
#ifdef RF_DIAG
    return getenv("RF_FFN8_64") != nullptr;
#else
    return false;
#endif
}
bool fused_ffn_supported(int C, int hidden, int h, int w) { return ffn_shape_ok(C, hidden, h, w, ffn_diag64()); }
bool fused_ffn_tail_supported(int C) { return C == 32; }      // the four-wave kernel only

// The projection form (ffn_fused_kernel<32, true, FfnProj>, rf_fused_proj.hip) of a stage with the fused tail: at level 0, in the size
// class of the tall attention front (attn_front_tall_slabs: above 256 tiles of 4 x 64, i.e. 256 x 256 packed).  From the level and
// (h, w) alone -- never from B: the two forms round differently, and an image's result must not depend on its neighbours
// (fused_attn_plan).  Both extra conditions keep the two-launch path in use, and thereby tested: every dim-32 frame of the launch
// census (tests/golden/forward_launches.json) is at most 64 x 72 packed, and its 1032 x 1024 frame at dim 16 reaches the fused tail
// with C = 32 at LEVEL 1 (516 x 512), where the projection GEMM stays a launch of its own.
bool fused_ffn_proj_rule(int lvl, int h, int w) {
#ifdef RF_DIAG   // diagnostic build only: the projection launch at any size
    if (getenv("RF_NO_FUSE_PROJ")) return false;
#endif
    return lvl == 0 && cdiv(w, fused::TW) * cdiv(h, fused::TH) > 256;
}

int launch_ffn_fused(FfnArgs a, int C, hipStream_t st, FfnTail tail, const FfnProj* proj) {
    const int B = a.B, h = a.h, w = a.w;
    RF_CHECK_ARG(ffn_shape_ok(C, 2 * C, h, w, ffn_diag64()) && B <= 65535, "ffn_fused: unsupported shape C=%d %dx%d", C, h, w);
    RF_CHECK_ARG(aligned16(a.x) && aligned16(a.out) && aligned16(a.w1p), "ffn_fused: buffers must be 16-byte aligned");
    RF_CHECK_ARG(!tail.xs || (fused_ffn_tail_supported(C) && tail.wp && aligned16(tail.xs) && aligned16(tail.wp) && tail.wp_bstride % 4 == 0),
                 "ffn_fused: the stage tail needs C = 32 and 16-byte aligned operands (C = %d)", C);
    RF_CHECK_ARG(!proj || (tail.xs && proj->v && proj->wf3 && proj->bias && aligned16(proj->v) && aligned16(proj->wf3) && proj->v_bstride % 4 == 0),
                 "ffn_fused: the projection form needs the stage tail and 16-byte aligned operands (C = %d)", C);
    a.tiles_x = cdiv(w, fused::TW);
    a.ntiles = a.tiles_x * cdiv(h, fused::TH);
    int wgs = cdiv(512, B);                       // persistent: two workgroups per CU over the whole batch
    if (wgs > a.ntiles) wgs = a.ntiles;
    const dim3 grid((unsigned)wgs, (unsigned)B);
    const double px = (double)B * h * w;
    if (C != 32) {
        // eight-wave form: one workgroup per CU, persistent over the whole batch
        int wg8 = cdiv(256, B);
        if (wg8 > a.ntiles) wg8 = a.ntiles;
        const dim3 grid8((unsigned)wg8, (unsigned)B);
        ProfScope prof(st, C == 64 ? "ffn_fused8_kernel<64>" : "ffn_fused8_kernel<48>", px * (8.0 * C * C + 36.0 * C), px * 8.0 * C);
        if (C == 64) ffn_fused8_kernel<64><<<grid8, 512, 0, st>>>(a);
        else ffn_fused8_kernel<48><<<grid8, 512, 0, st>>>(a);
        return check_launch("ffn_fused8");
    }
    if (proj) {      // four tensors of C floats per pixel: x, v and xs in, out
        ProfScope prof(st, "ffn_fused_kernel<32, true, proj>", px * (8.0 * C * C + 36.0 * C + 2.0 * 2 * C * C + 2.0 * C * C), px * 4.0 * 4 * C);
        return launch_ffn_fused_proj32(a, tail, *proj, grid, st);
    }
    if (tail.xs) {
        ProfScope prof(st, "ffn_fused_kernel<32, true>", px * (8.0 * C * C + 36.0 * C + 2.0 * 2 * C * C), px * 4.0 * 3 * C);
        return launch_ffn_fused_tail32(a, tail, grid, st);
    }
    ProfScope prof(st, "ffn_fused_kernel<32>", px * (8.0 * C * C + 36.0 * C), px * 8.0 * C);
    ffn_fused_kernel<32, false><<<grid, 256, 0, st>>>(a, tail);
    return check_launch("ffn_fused");
}

// ================================================================================================
// Attention front:  qkv = dw3x3(Wqkv LN1(x) + b);  Gram partials of (q, k) per head;  v -> HBM          (AttnFrontArgs: rf_common.h)
// ================================================================================================
template <int C>
__global__ void __launch_bounds__(256, 2) attn_front_kernel(AttnFrontArgs a) {
    using namespace fused;
    const int ro[3] = {0, HC, 2 * HC};   // a tile's halo'd rows are contiguous in LDS
    constexpr int NS = C / 4;
    constexpr int NQT = C / 16;          // q (and k) tiles = Gram rounds
    constexpr int NVP = C / PART;        // v parts
    constexpr int NT3 = 3 * C / 16;      // tiles of the qkv weight
    constexpr int PSG = fused::PSG;      // plane stride for the Gram rounds (see fused::PSG)
    constexpr int PSV = 448;             // plane stride for the v parts: lanes run along pixels
    constexpr int ROWW = 4 * 16 + 2;     // partial row width of rf_attn.hip (kMaxBand * 16 + 2)
    __shared__ __attribute__((aligned(16))) float mid[PART * PSG + 8];
    __shared__ __attribute__((aligned(16))) u32x4 w_l[(C / 32) * NT3 * 192];     // whole qkv weight (b3), resident
    __shared__ float wd_l[3 * C * 9], bd_l[3 * C], bq_l[3 * C], gam_l[C], bet_l[C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int slab = blockIdx.x, b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    const float* xb = a.x + (size_t)b * C * P;
    float* vb = a.v + (size_t)b * C * P;

    for (int i = tid; i < (C / 32) * NT3 * 192; i += 256) w_l[i] = reinterpret_cast<const u32x4*>(a.wp)[i];
    for (int i = tid; i < 3 * C * 9; i += 256) wd_l[i] = a.wd[i];
    for (int i = tid; i < 3 * C; i += 256) { bd_l[i] = a.bd[i]; bq_l[i] = a.bq[i]; }
    for (int i = tid; i < C; i += 256) { gam_l[i] = a.ln_w[i]; bet_l[i] = a.ln_b[i]; }

    // |q_j|^2 and |k_j|^2 are plain per-lane sums of squares (2 VALU per value): as the diagonals of q q^T and k k^T on the matrix
    // pipe they cost eight 33-cycle MFMAs per step for 32 useful numbers -- and MFMA time and VALU time add up on this chip
    f32x4 gq[NQT];
    float nq[NQT], nk[NQT];
#pragma unroll
    for (int r = 0; r < NQT; ++r) { gq[r] = (f32x4){0.f, 0.f, 0.f, 0.f}; nq[r] = 0.f; nk[r] = 0.f; }
    STAMP_DECL

    const TileRange tr = tile_range(a.ntiles, a.tiles_x, a.nslab, slab);
    for (int tile = tr.begin; tile < tr.end; ++tile) {
        const int2 o = tile_origin(tile, tr.tiles_y);
        const int x0 = o.x, y0 = o.y;
        // The input tile is loaded here, not a tile ahead: the b3 pieces (96 registers) already fill the budget that the
        // f32 kernel of round 1 spent on the next tile's raw values.  The loads are issued before the barrier so that their
        // latency overlaps the wait (throw-away loads warming L2 for the next tile were measured: 3 % slower).
        const GroupGeom g0 = group_geom<GPW>(wave, 0, j, y0, x0, h, w), g1 = group_geom<GPW>(wave, 1, j, y0, x0, h, w);
        float4 xh0[NS], xh1[NS];
        load_step_b3<C>(xb, P, kq, g0, xh0);
        load_step_b3<C>(xb, P, kq, g1, xh1);
        lds_barrier();                                   // weights visible; previous tile finished with mid
        STAMP(0);
        ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh0);
        ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh1);
        u32x4 bp0[C / 32][4][3], bp1[C / 32][4][3];
        split_step<C>(xh0, bp0);
        split_step<C>(xh1, bp1);
        const int yo = y0 + wave;
        STAMP(1);

        // ---- Gram rounds: q tile r (plane 0-15) with k tile r (planes 16-31); heads never straddle a tile here
#pragma unroll
        for (int r = 0; r < NQT; ++r) {
            if (r) lds_barrier();
            STAMP(0);
            phase_a_step_b3<C, NT3>(bp0, w_l + lane, r, NQT + r, bq_l + 16 * r, bq_l + C + 16 * r, mid, PSG, kq, g0);
            phase_a_step_b3<C, NT3>(bp1, w_l + lane, r, NQT + r, bq_l + 16 * r, bq_l + C + 16 * r, mid, PSG, kq, g1);
            STAMP(2);
            lds_barrier();
            STAMP(0);
            // phase B: lane (i = j, kq) owns channel i of the q tile and of the k tile at pixels x0 + 16*st + 4*kq + m
            const int cq = 16 * r + j, ck = C + 16 * r + j;
#pragma unroll 1                                         // unrolled, the hoisted stencil loads push the kernel into scratch
            for (int st = 0; st < 4; ++st) {
                const int xo = x0 + 16 * st + 4 * kq;
                const bool ok = yo >= a.ylo && yo < a.yhi && xo >= a.xlo && xo < a.xhi;
                float qa[4], kb[4];
                stencil4<Edge::Wide>(mid + j * PSG + wave * HC + 16 * st + 4 * kq + 4, ro, j, wd_l + cq * 9, bd_l[cq], qa);
                stencil4<Edge::Wide>(mid + (16 + j) * PSG + wave * HC + 16 * st + 4 * kq + 4, ro, j, wd_l + ck * 9, bd_l[ck], kb);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float qv = ok ? qa[m] : 0.f, kv = ok ? kb[m] : 0.f;
                    gq[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(qv, kv, gq[r], 0, 0, 0);
                    nq[r] = fmaf(qv, qv, nq[r]);
                    nk[r] = fmaf(kv, kv, nk[r]);
                }
            }
            STAMP(3);
        }
        // ---- v parts: 1x1 -> LDS -> depthwise -> HBM
#pragma unroll
        for (int vp = 0; vp < NVP; ++vp) {
            lds_barrier();
            STAMP(0);
            const int t0 = 2 * NQT + 2 * vp;
            phase_a_step_b3<C, NT3>(bp0, w_l + lane, t0, t0 + 1, bq_l + 2 * C + vp * PART, bq_l + 2 * C + vp * PART + 16, mid, PSV, kq, g0);
            phase_a_step_b3<C, NT3>(bp1, w_l + lane, t0, t0 + 1, bq_l + 2 * C + vp * PART, bq_l + 2 * C + vp * PART + 16, mid, PSV, kq, g1);
            STAMP(2);
            lds_barrier();
            STAMP(0);
            const int xo = x0 + 4 * j;
            if (yo < h && xo < w) {
#pragma unroll
                for (int s = 0; s < PART / 4; ++s) {
                    const int hc = 4 * s + kq, cv = 2 * C + vp * PART + hc;
                    float v[4];
                    stencil4<Edge::Dpp>(mid + hc * PSV + wave * HC + 4 * j + 4, ro, j, wd_l + cv * 9, bd_l[cv], v);
                    // uniform base + 32-bit lane offset (C P < 2^30 elements, checked by fused_attn_supported): no 64-bit per-lane pointer to keep
                    *reinterpret_cast<float4*>(vb + (unsigned)((vp * PART + hc) * P + yo * w + xo)) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
            STAMP(4);
        }
    }
    STAMP_FLUSH;
    // ---- cross-wave reduction of the Gram tiles in a fixed order, one partial per workgroup.
    // The zero key tiles of a partial row are written by their own strided loop, not next to the Gram values: hipcc 7.2 paired
    // `rr[j] = g; rr[16 + j] = 0; rr[32 + j] = 0; rr[48 + j] = 0` into ds_write2_b32 with offset0 4 instead of 16 when the
    // accumulators sat in AGPRs (seen with __launch_bounds__(256, 1)), i.e. zeros over the neighbouring Gram columns.
    __syncthreads();
    float* red = mid;                                      // [4 waves][16][ROWW] floats = 4224 <= PART * PSG
#pragma unroll
    for (int r = 0; r < NQT; ++r) {
        for (int i = tid; i < 64 * 48; i += 256) red[(i / 48) * ROWW + 16 + i % 48] = 0.f;
        // channel j's sums of squares: the four kq lanes of a channel hold disjoint pixels
        float nqt = nq[r], nkt = nk[r];
        nqt += __shfl_xor(nqt, 16); nqt += __shfl_xor(nqt, 32);
        nkt += __shfl_xor(nkt, 16); nkt += __shfl_xor(nkt, 32);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 4 * kq + q;
            float* rr = red + (wave * 16 + row) * ROWW;
            rr[j] = gq[r][q];
            if (row == j) { rr[64] = nqt; rr[65] = nkt; }
        }
        __syncthreads();
        float* dst = a.partial + (((size_t)b * a.nslab + slab) * NQT + r) * 16 * ROWW;
        for (int i = tid; i < 16 * ROWW; i += 256)
            dst[i] = ((red[i] + red[16 * ROWW + i]) + red[2 * 16 * ROWW + i]) + red[3 * 16 * ROWW + i];
        __syncthreads();
    }
}

static bool attn_front_shape_ok(int C, int h, int w) { return C == 32 && (w % 4 == 0) && ((double)C * h * w * 4.0 < 4.0e9); }
bool fused_attn_supported(int C, int heads, int h, int w) { return heads_fit_tiles(C, heads) && attn_front_shape_ok(C, h, w); }

// Which form runs, from (h, w) alone -- never from B: an image's reduction order is batch-invariant.  The 12-row kernel on eight
// waves (rf_attn_front_tall.hip) takes over where the 4-row plan puts several tiles into a workgroup, i.e. above 256 x 256 packed,
// with TWO tall tiles (1536 px), consecutive down a column, per workgroup.  Measured on MI355X (DESIGN sections 5 and 7; ms per
// step of the whole forward on one box, the 4-row kernel at 7.67 - 7.71 for 8 images of 512 x 512 and 1.710 - 1.714 for one):
// one tile 7.58 | 1.71 - 1.73, two 7.52 - 7.53 | 1.692 - 1.694, three 7.50 - 7.52 | 1.693 - 1.700, four 7.53 - 7.54 | 1.74.  A
// workgroup pays its start, the 18 KB of weights and the reduction once, with no second workgroup on the CU to hide them, so one
// tile is too few; from four on a single frame leaves CUs idle (344 tiles: 86 workgroups).  Unequal shares (one or two tiles:
// the 4-row plan's workgroup count) lost to every equal split: 7.75.
static int attn_front_tall_slabs(int h, int w) {      // workgroups per image; 0: the 4-row kernel
    const int ntall = cdiv(w, fused::TW) * cdiv(h, fused::TH_TALL);
    if (cdiv(w, fused::TW) * cdiv(h, fused::TH) <= 256) return 0;
    int per = 2;
#ifdef RF_DIAG   // diagnostic build only: RF_ATTN_TALL=0 keeps the 4-row kernel everywhere, =T gives a workgroup T tall tiles
    if (const char* e = getenv("RF_ATTN_TALL")) per = atoi(e);
    if (per <= 0) return 0;
#endif
    return cdiv(ntall, per);
}

int fused_attn_plan(int h, int w, int* nslab, size_t* partial_floats, int B, int C, int* tall_form, size_t* reserve_floats) {
    const int ntiles = cdiv(w, fused::TW) * cdiv(h, fused::TH);
    int ns = cdiv(ntiles, 4);                   // the 4-row kernel above 256 tiles (now the diagnostic build's RF_ATTN_TALL=0 only):
                                                // 4 tiles (1024 px) per workgroup: ONE 1024x1024 frame gives the chip 256 workgroups
                                                // (8 tiles: 131 us per launch for one frame, 4 tiles: 75 us; a batch of 8 pays
                                                // 0.6 %); depends on the image only, never on B: an image's reduction order is
                                                // batch-invariant
    if (ntiles <= 256) ns = ntiles;             // frames up to 256 x 256 packed: one tile per workgroup (a workgroup's tiles are a
                                                // chain of ~15 us each: 62 -> 25 us per launch for one 128 x 128 frame)
                                                // (two tiles per workgroup at 512 x 512: -17 % for one frame, +11 % for a batch of 8)
    if (ns < 1) ns = 1;
    const int ns4 = ns, tall = attn_front_tall_slabs(h, w);
    if (tall) ns = tall;
    *nslab = ns;
    *partial_floats = (size_t)B * ns * (C / 16) * 16 * 66;
    if (tall_form) *tall_form = tall > 0;
    // what the scratch layouts set aside: the larger of the two forms' buffers, i.e. what the 4-row plan always took (the tall form
    // writes fewer partials), so no scratch or workspace size moves with the form
    if (reserve_floats) *reserve_floats = (size_t)B * (ns > ns4 ? ns : ns4) * (C / 16) * 16 * 66;
    return RF_OK;
}

int launch_attn_front(AttnFrontArgs a, int C, hipStream_t st) {
    const int B = a.B, h = a.h, w = a.w;
    RF_CHECK_ARG(attn_front_shape_ok(C, h, w) && B <= 65535, "attn_front: unsupported shape C=%d %dx%d", C, h, w);
    RF_CHECK_ARG(aligned16(a.x) && aligned16(a.v), "attn_front: buffers must be 16-byte aligned");
    int nslab = 0, tall = 0;
    size_t pf = 0;
    fused_attn_plan(h, w, &nslab, &pf, B, C, &tall);
    RF_CHECK_ARG(a.nslab == nslab, "attn_front: %d slabs, the plan for %dx%d has %d", a.nslab, h, w, nslab);
    a.tiles_x = cdiv(w, fused::TW);
    a.ntiles = a.tiles_x * cdiv(h, tall ? fused::TH_TALL : fused::TH);
    if (!(a.yhi > 0 && a.yhi < h)) a.yhi = h;
    if (!(a.xhi > 0 && a.xhi < w)) a.xhi = w;
    const double px = (double)B * h * w;
    ProfScope prof(st, "attn_front_kernel<32>", px * (6.0 * C * C + 54.0 * C + 4.0 * C * 16), px * 8.0 * C);
    const dim3 grid((unsigned)a.nslab, (unsigned)B);
    if (tall) return launch_attn_front_tall32(a, grid, st);
    attn_front_kernel<32><<<grid, 256, 0, st>>>(a);
    return check_launch("attn_front");
}

#ifdef RF_STAMP
extern "C" int rf_debug_stamps(unsigned long long* out8) {   // diagnostic build only: read and reset the phase cycle sums
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_stamp), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace rf
