// attn_front_kernel (rf_fused.hip) on a TALL tile: 12 output rows x 64 px per workgroup of EIGHT waves, one workgroup per CU.
// In a translation unit of its own: hipcc compiles a unit's kernels together, and an instantiation added to rf_fused.hip changes
// the code of its neighbours (tools/isa_same.py; rf_fused_tail.hip exists for the same reason).
//
// Why taller: phase A -- input loads, LayerNorm, the three-piece split, the qkv GEMM, bias + LDS write -- is paid per HALO'D pixel
// group.  The 4-row tile computes 6 x 18 = 108 groups in 128 slots (4 waves x 2 MFMA steps) for 64 output groups; this one
// 14 x 18 = 252 groups in 256 slots (8 waves x 2 steps) for 192: a third less phase A per output pixel.  The b3 pieces per wave
// (96 registers) and the waves per CU (eight) are those of two co-resident 4-row workgroups.
//   LDS: mid 32 planes x 1032 floats = 129 KB, the resident qkv weight 18 KB, stencil weights and vectors 4.4 KB: 155 008 B of
//   160 KB, one 512-thread workgroup per CU (as ffn_fused8_kernel runs).  hipcc 7.2: 244 VGPRs, no scratch, 2 waves per SIMD.
// Phase B keeps no per-pixel accumulator, so the 12 rows spread over 8 waves by units:
//   Gram rounds   48 units (row, column step of 16 px): wave wv takes column step wv % 4 of rows 6 (wv / 4) .. + 6
//   v parts       96 units (row, channel step of 4):    wave wv takes channel step wv of all 12 rows
// A wave's units are thus ONE strip of consecutive rows, and the depthwise stencil rolls down it (roll_row, rf_fused_tile.h): every
// input row is read from LDS once instead of three times and the nine weights stay in registers, with stencil4's values bit for
// bit.  This is what the form lives on: with a single workgroup on the CU all eight waves are in phase B together, nobody's phase A
// covers their LDS time, and with stencil4 per row the kernel only tied the 4-row one.
// The Gram tile and the norms are sums over pixels in any order; the eight waves' sums are added in a fixed order into ONE partial
// per workgroup, in the layout of the 4-row kernel ([B][nslab][C/16][16][66]): attn_fold_kernel does not know the difference.
#include "rf_common.h"
#include "rf_fused_tile.h"

namespace rf {

template <int C>
__global__ void __launch_bounds__(512, 1) attn_front_tall_kernel(AttnFrontArgs a) {
    using namespace fused;
    constexpr int NW = 8;                // waves
    constexpr int NS = C / 4;
    constexpr int NQT = C / 16;          // q (and k) tiles = Gram rounds
    constexpr int NVP = C / PART;        // v parts
    constexpr int NT3 = 3 * C / 16;      // tiles of the qkv weight
    constexpr int PSG = PSG_TALL, PSV = PSV_TALL;
    constexpr int ROWW = 4 * 16 + 2;     // partial row width of rf_attn.hip (kMaxBand * 16 + 2)
    static_assert(NW * GPW_TALL >= HR_TALL * (HC / 4) && HR_TALL * HC <= PSV && PSV <= PSG, "the halo'd tile fits the slots and the planes");
    static_assert(TH_TALL * 4 % NW == 0 && PART / 4 == NW, "phase B units divide over the waves");
    static_assert(NW * 16 * ROWW <= PART * PSG, "the cross-wave reduction fits mid");
    __shared__ __attribute__((aligned(16))) float mid[PART * PSG];
    __shared__ __attribute__((aligned(16))) u32x4 w_l[(C / 32) * NT3 * 192];     // whole qkv weight (b3), resident
    __shared__ float wd_l[3 * C * 9], bd_l[3 * C], bq_l[3 * C], gam_l[C], bet_l[C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int slab = blockIdx.x, b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    const float* xb = a.x + (size_t)b * C * P;
    float* vb = a.v + (size_t)b * C * P;

    for (int i = tid; i < (C / 32) * NT3 * 192; i += 64 * NW) w_l[i] = reinterpret_cast<const u32x4*>(a.wp)[i];
    for (int i = tid; i < 3 * C * 9; i += 64 * NW) wd_l[i] = a.wd[i];
    for (int i = tid; i < 3 * C; i += 64 * NW) { bd_l[i] = a.bd[i]; bq_l[i] = a.bq[i]; }
    for (int i = tid; i < C; i += 64 * NW) { gam_l[i] = a.ln_w[i]; bet_l[i] = a.ln_b[i]; }

    f32x4 gq[NQT];
    float nq[NQT], nk[NQT];              // sums of squares on the VALU (see attn_front_kernel)
#pragma unroll
    for (int r = 0; r < NQT; ++r) { gq[r] = (f32x4){0.f, 0.f, 0.f, 0.f}; nq[r] = 0.f; nk[r] = 0.f; }

    constexpr int GROWS = TH_TALL * 4 / NW;                                 // rows of a wave's Gram units
    const int gst = wave & 3, grow = GROWS * (wave >> 2);                   // ... their column step and first row

    // this workgroup's tiles: consecutive down the columns of the tile grid (see tile_range: successive tiles share two halo'd rows,
    // still in L2), an even split of the ntiles over the nslab workgroups: [slab ntiles / nslab, (slab + 1) ntiles / nslab)
    const int tiles_y = a.ntiles / a.tiles_x;
    const int tbegin = (int)((long long)slab * a.ntiles / a.nslab), tend = (int)((long long)(slab + 1) * a.ntiles / a.nslab);
    GroupGeom g0, g1;
    float4 xh0[NS], xh1[NS];
    auto fetch = [&](int tile) {                         // a tile's geometry and its raw input, two MFMA steps per wave
        const int2 o = tile_origin<TH_TALL>(tile, tiles_y);
        g0 = group_geom<GPW_TALL, HR_TALL>(wave, 0, j, o.y, o.x, h, w);
        g1 = group_geom<GPW_TALL, HR_TALL>(wave, 1, j, o.y, o.x, h, w);
        load_step_b3<C>(xb, P, kq, g0, xh0);
        load_step_b3<C>(xb, P, kq, g1, xh1);
    };
    for (int tile = tbegin; tile < tend; ++tile) {
        const int2 o = tile_origin<TH_TALL>(tile, tiles_y);
        const int x0 = o.x, y0 = o.y;
        fetch(tile);                                     // loads ahead of the barrier, as in the 4-row kernel
        lds_barrier();                                   // weights visible; previous tile finished with mid
        ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh0);
        ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh1);
        u32x4 bp0[C / 32][4][3], bp1[C / 32][4][3];
        split_step<C>(xh0, bp0);
        split_step<C>(xh1, bp1);

        // ---- Gram rounds: q tile r (planes 0-15) with k tile r (planes 16-31); heads never straddle a tile here
#pragma unroll
        for (int r = 0; r < NQT; ++r) {
            if (r) lds_barrier();
            phase_a_step_b3<C, NT3>(bp0, w_l + lane, r, NQT + r, bq_l + 16 * r, bq_l + C + 16 * r, mid, PSG, kq, g0);
            phase_a_step_b3<C, NT3>(bp1, w_l + lane, r, NQT + r, bq_l + 16 * r, bq_l + C + 16 * r, mid, PSG, kq, g1);
            lds_barrier();
            // phase B: lane (i = j, kq) owns channel i of the q tile and of the k tile at pixels x0 + 16 gst + 4 kq + m of six rows
            const int cq = 16 * r + j, ck = C + 16 * r + j;
            const int xo = x0 + 16 * gst + 4 * kq;
            const bool okx = xo >= a.xlo && xo < a.xhi;
            // the wave's six rows are one strip: eight input rows, each read once, the stencil weights in registers
            float wq[9], wk[9], aq[3][4] = {}, ak[3][4] = {};
#pragma unroll
            for (int t = 0; t < 9; ++t) { wq[t] = wd_l[cq * 9 + t]; wk[t] = wd_l[ck * 9 + t]; }
            const float bdq = bd_l[cq], bdk = bd_l[ck];
            const float* sq = mid + j * PSG + grow * HC + 16 * gst + 4 * kq + 4;
#pragma unroll 1
            for (int ir = 0; ir < GROWS + 2; ++ir) {
                float tq[6], tk[6];
                row_taps<Edge::Wide>(sq + ir * HC, j, tq);
                row_taps<Edge::Wide>(sq + 16 * PSG + ir * HC, j, tk);
                roll_row(tq, wq, bdq, aq);
                roll_row(tk, wk, bdk, ak);
                if (ir >= 2) {
                    const int yo = y0 + grow + ir - 2;
                    const bool ok = okx && yo >= a.ylo && yo < a.yhi;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float qv = ok ? aq[0][m] : 0.f, kv = ok ? ak[0][m] : 0.f;
                        gq[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(qv, kv, gq[r], 0, 0, 0);
                        nq[r] = fmaf(qv, qv, nq[r]);
                        nk[r] = fmaf(kv, kv, nk[r]);
                    }
                }
                roll_shift(aq);
                roll_shift(ak);
            }
        }
        // ---- v parts: 1x1 -> LDS -> depthwise -> HBM
#pragma unroll
        for (int vp = 0; vp < NVP; ++vp) {
            lds_barrier();
            const int t0 = 2 * NQT + 2 * vp;
            phase_a_step_b3<C, NT3>(bp0, w_l + lane, t0, t0 + 1, bq_l + 2 * C + vp * PART, bq_l + 2 * C + vp * PART + 16, mid, PSV, kq, g0);
            phase_a_step_b3<C, NT3>(bp1, w_l + lane, t0, t0 + 1, bq_l + 2 * C + vp * PART, bq_l + 2 * C + vp * PART + 16, mid, PSV, kq, g1);
            lds_barrier();
            const int xo = x0 + 4 * j;
            const int hc = 4 * wave + kq, cv = 2 * C + vp * PART + hc;
            if (xo < w) {
                // all twelve rows of the wave's four channels: one strip, fourteen input rows (fewer in a ragged last tile)
                float wv[9], av[3][4] = {};
#pragma unroll
                for (int t = 0; t < 9; ++t) wv[t] = wd_l[cv * 9 + t];
                const float bdv = bd_l[cv];
                const float* sv = mid + hc * PSV + 4 * j + 4;
                // uniform base + 32-bit lane offset (C P < 2^30 elements, checked by fused_attn_supported)
                unsigned voff = (unsigned)((vp * PART + hc) * P + y0 * w + xo);
                const int nrow = h - y0 < TH_TALL ? h - y0 : TH_TALL;
#pragma unroll 1
                for (int ir = 0; ir < nrow + 2; ++ir) {
                    float tv[6];
                    row_taps<Edge::Dpp>(sv + ir * HC, j, tv);
                    roll_row(tv, wv, bdv, av);
                    if (ir >= 2) {
                        *reinterpret_cast<float4*>(vb + voff) = make_float4(av[0][0], av[0][1], av[0][2], av[0][3]);
                        voff += (unsigned)w;
                    }
                    roll_shift(av);
                }
            }
        }
    }
    // ---- cross-wave reduction of the Gram tiles in a fixed order, one partial per workgroup (the zero key tiles of a partial row
    // are written by their own strided loop: see attn_front_kernel)
    __syncthreads();
    float* red = mid;                                      // [8 waves][16][ROWW] floats
#pragma unroll
    for (int r = 0; r < NQT; ++r) {
        for (int i = tid; i < NW * 16 * 48; i += 64 * NW) red[(i / 48) * ROWW + 16 + i % 48] = 0.f;
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
        for (int i = tid; i < 16 * ROWW; i += 64 * NW) {
            float s = red[i];
#pragma unroll
            for (int wv = 1; wv < NW; ++wv) s += red[wv * 16 * ROWW + i];
            dst[i] = s;
        }
        __syncthreads();
    }
}

int launch_attn_front_tall32(const AttnFrontArgs& a, dim3 grid, hipStream_t st) {
    attn_front_tall_kernel<32><<<grid, 512, 0, st>>>(a);
    return check_launch("attn_front_tall");
}

}  // namespace rf
