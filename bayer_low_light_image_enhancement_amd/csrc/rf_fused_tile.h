// The tile machinery of the fused transformer-block kernels (rf_fused.hip has the overview) and ffn_fused_kernel itself, in a
// header because the kernel is instantiated in three translation units: rf_fused.hip builds <32, false>, rf_fused_tail.hip
// <32, true>, rf_fused_proj.hip <32, true, FfnProj>.  hipcc compiles a translation unit's kernels together, and a second
// instantiation beside the first changed the code of the first AND of attn_front_kernel / attn_mid_kernel (tools/isa_same.py); on
// its own each compiles as before.
#pragma once
#include "rf_common.h"

namespace rf {

#ifdef RF_STAMP
// Diagnostic build only (python -m ...build --stamp): per-phase cycle sums of wave 0 lanes into g_stamp (rf_fused.hip), read back
// with rf_debug_stamps().  Never compiled into the shipped library.
#define STAMP_DECL unsigned long long st_prev = __builtin_amdgcn_s_memtime(), st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_prev; st_prev = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_FLUSH do { if ((threadIdx.x & 63) == 0) for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_stamp[i_], st_acc[i_]); } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#endif

// Workgroup barrier that orders LDS traffic only.  __syncthreads() makes hipcc drain vmcnt(0) first,
// which would stall every wave on the next tile's prefetch loads that are deliberately in flight.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// heads that never straddle a 16-channel tile: what attn_front_kernel (rf_fused.hip) and attn_mid_kernel (rf_attn_mid.hip) need
static inline bool heads_fit_tiles(int C, int heads) {
    const int c = heads > 0 ? C / heads : 0;
    return c > 0 && C % heads == 0 && c <= 16 && 16 % c == 0;
}

namespace fused {
constexpr int TH = 4, TW = 64;          // output tile
constexpr int HR = TH + 2;              // halo'd rows
constexpr int HC = 72;                  // halo'd columns held (18 groups of 4 px)
constexpr int NG = HR * (HC / 4);       // 108 pixel groups per tile
constexpr int GPW = NG / 4;             // 27 groups per wave in phase A (two MFMA steps: 16 + 11)
constexpr int GPW8 = 14;                // ... of the eight-wave kernel: one step (8 x 14 = 112 >= 108)
constexpr int PART = 32;                // intermediate channels per part
// Plane stride of the Gram rounds, where lane (j, kq) reads 16 bytes at plane j, column 4 kq (+ 16 st): a ds_read_b128 is
// served in four groups of 16 lanes, each holding every j once with two different kq (MI355X_MICROARCH.md, LDS), so the
// groups are conflict-free iff (PSG j + 4 kq) mod 64 are 16 distinct multiples of 4: PSG = 8 mod 64.  (452 = 4 mod 64 made
// lanes (j, 1) and (j + 1, 0) collide: SQ_LDS_BANK_CONFLICT was 55 % of the LDS-active cycles of attn_front.)
constexpr int PSG = 456;
// The tall attention tile (rf_attn_front_tall.hip): 12 output rows on eight waves, 14 halo'd rows x 18 groups = 252 groups as two
// MFMA steps per wave (8 x 32 = 256 slots).  Plane strides: 14 x 72 = 1008 floats, padded to 8 mod 64 for the Gram rounds (see PSG)
// and to a multiple of 64 for the v parts.
constexpr int TH_TALL = 12, HR_TALL = TH_TALL + 2, GPW_TALL = 32;
constexpr int PSG_TALL = 1032, PSV_TALL = 1024;
}  // namespace fused

// ---- shared phase-A machinery ------------------------------------------------------------------
// A wave's share of the halo'd pixel groups, G of them in steps of 16 (G <= 16: step 0 only; the last wave's share may then run
// past the tile): geometry of step st for lane j.  ROWS = halo'd rows of the tile (fused::HR; the tall attention tile: 14).
struct GroupGeom {
    int lds_off;     // row * HC + 4 * cg
    int goff;        // y * w + x  (clamped to 0 when outside)
    bool valid;
};
template <int G, int ROWS = fused::HR>
__device__ __forceinline__ GroupGeom group_geom(int wave, int st, int j, int y0, int x0, int h, int w) {
    using namespace fused;
    constexpr int NG = ROWS * (HC / 4);
    GroupGeom g;
    const int gi = wave * G + st * 16 + j;
    const bool in_step = j < G - st * 16 && (NG % G == 0 || gi < NG);
    const int row = gi / (HC / 4), cg = gi % (HC / 4);
    const int y = y0 - 1 + row, x = x0 - 4 + 4 * cg;
    g.valid = in_step && y >= 0 && y < h && x >= 0 && x < w;
    g.lds_off = in_step ? row * HC + 4 * cg : -1;
    g.goff = g.valid ? y * w + x : 0;
    return g;
}

// A persistent workgroup's tiles: CONSECUTIVE and numbered down the columns of the tile grid (ty fastest), so successive tiles
// share two of their six halo'd rows, which are then still in L2 (strided tiles, numbered along x, re-fetched every halo row
// from HBM).  `wg` of `nwg` workgroups owns [begin, end); WG keeps the caller's signedness of the product wg * per.
struct TileRange { int tiles_y, begin, end; };
template <typename WG>
__device__ __forceinline__ TileRange tile_range(int ntiles, int tiles_x, int nwg, WG wg) {
    const int tiles_y = ntiles / tiles_x;
    const int per = (ntiles + nwg - 1) / nwg;
    const int begin = wg * per, end = (begin + per < ntiles) ? begin + per : ntiles;
    return {tiles_y, begin, end};
}
template <int ROWS = fused::TH>                                           // output rows of a tile
__device__ __forceinline__ int2 tile_origin(int tile, int tiles_y) {      // (x0, y0) of a tile
    const int tx = tile / tiles_y, ty = tile % tiles_y;
    return make_int2(tx * fused::TW, ty * ROWS);
}

// ---- phase-A helpers in b3 form (rf_common.h): lane (j, kq) holds channels 32 kb + 8 kq + i, i = 0..7 ------------------------
// Input tile of one step: raw loads (issue early: the next tile is fetched behind the current phase B) ...
template <int C>
__device__ __forceinline__ void load_step_b3(const float* __restrict__ xb, int P, int kq, const GroupGeom& g, float4 (&xh)[C / 4]) {
    const unsigned voff = (unsigned)(8 * kq) * (unsigned)P + (unsigned)g.goff;
#pragma unroll
    for (int s = 0; s < C / 4; ++s) xh[s] = *reinterpret_cast<const float4*>(xb + (size_t)(32 * (s >> 3) + (s & 7)) * P + voff);
}

// ... and the exact two-pass LayerNorm over channels, in place.
template <int C>
__device__ __forceinline__ void ln_step_b3(int kq, const float* __restrict__ gam_l, const float* __restrict__ bet_l, float eps, float4 (&xh)[C / 4]) {
    constexpr int NS = C / 4;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) { sum[0] += xh[s].x; sum[1] += xh[s].y; sum[2] += xh[s].z; sum[3] += xh[s].w; }
    float mu[4], var[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum[q] += __shfl_xor(sum[q], 16);
        sum[q] += __shfl_xor(sum[q], 32);
        mu[q] = sum[q] * (1.0f / C);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float d0 = xh[s].x - mu[0], d1 = xh[s].y - mu[1], d2 = xh[s].z - mu[2], d3 = xh[s].w - mu[3];
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
        const float gk = gam_l[ch], bk = bet_l[ch];
        xh[s].x = fmaf((xh[s].x - mu[0]) * rstd[0], gk, bk);
        xh[s].y = fmaf((xh[s].y - mu[1]) * rstd[1], gk, bk);
        xh[s].z = fmaf((xh[s].z - mu[2]) * rstd[2], gk, bk);
        xh[s].w = fmaf((xh[s].w - mu[3]) * rstd[3], gk, bk);
    }
}

template <int C>
__device__ __forceinline__ void split_step(const float4 (&xh)[C / 4], u32x4 (&bp)[C / 32][4][3]) {
#pragma unroll
    for (int kb = 0; kb < C / 32; ++kb)
#pragma unroll
        for (int hp = 0; hp < 4; ++hp) {
            const float4 va = xh[8 * kb + 2 * hp], vb = xh[8 * kb + 2 * hp + 1];
            const float xa[4] = {va.x, va.y, va.z, va.w}, xc[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                unsigned a0, a1, a2, b0, b1, b2;
                b3_split(xa[g], a0, a1, a2);
                b3_split(xc[g], b0, b1, b2);
                bp[kb][g][0][hp] = b3_pack(a0, b0);
                bp[kb][g][1][hp] = b3_pack(a1, b1);
                bp[kb][g][2][hp] = b3_pack(a2, b2);
            }
        }
}

template <int C, int WT>
__device__ __forceinline__ void phase_a_step_b3(const u32x4 (&bp)[C / 32][4][3], const u32x4* __restrict__ wl,
                                                int tile0, int tile1, const float* __restrict__ bias0, const float* __restrict__ bias1,
                                                float* __restrict__ mid, int PS, int kq, const GroupGeom& g) {
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < C / 32; ++kb) {
        const u32x4* w0 = wl + (size_t)(kb * WT + tile0) * 192;
        const u32x4* w1 = wl + (size_t)(kb * WT + tile1) * 192;
        const u32x4 a0[3] = {w0[0], w0[64], w0[128]}, a1[3] = {w1[0], w1[64], w1[128]};
        b3_mfma4(a0, bp[kb], acc[0]);
        b3_mfma4(a1, bp[kb], acc[1]);
    }
    if (g.lds_off >= 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float bs = (t ? bias1 : bias0)[4 * kq + r];
                float4 v = make_float4(acc[t][0][r] + bs, acc[t][1][r] + bs, acc[t][2][r] + bs, acc[t][3][r] + bs);
                if (!g.valid) v = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(mid + (16 * t + 4 * kq + r) * PS + g.lds_off) = v;
            }
    }
}

// 3x3 depthwise stencil for 4 consecutive pixels from an LDS plane: `p` points at the plane's column of the first pixel,
// 16-byte aligned, and the three rows (output row - 1 ..) lie at p + ro[dy]: {0, HC, 2 HC} in a contiguous tile, anything in
// the circular row window of attn_mid_kernel.  The two edge taps of every row must not be scalar LDS reads (lanes 4 floats
// apart are a 4-way bank conflict on ds_read_b32: measured 58 % of all LDS cycles), so:
//   Edge::Dpp   lanes j-1 / j+1 of the same 16-lane row hold the neighbouring 4-pixel groups:
//               edges come over DPP row shifts; only lanes 0 and 15 read their outer tap.
//   Edge::Wide  neighbouring groups are not in this wave's registers: three aligned
//               ds_read_b128 per row (conflict-free with the plane stride used there).
__device__ __forceinline__ float dpp_row_shr1(float keep, float v) {   // lane i <- lane i-1 (i % 16 == 0 keeps `keep`)
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(keep), __float_as_int(v), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_row_shl1(float keep, float v) {   // lane i <- lane i+1 (i % 16 == 15 keeps `keep`)
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(keep), __float_as_int(v), 0x101, 0xf, 0xf, false));
}

enum class Edge { Dpp, Wide };
// the six taps of one row: the pixel left of the four, the four, the pixel right of them
template <Edge E>
__device__ __forceinline__ void row_taps(const float* __restrict__ row, int j, float (&v)[6]) {
    float4 m;
    float vl, vr;                                    // the taps left and right of m
    if constexpr (E == Edge::Dpp) {
        m = *reinterpret_cast<const float4*>(row);
        float el = 0.f, er = 0.f;
        if (j == 0) el = row[-1];
        if (j == 15) er = row[4];
        vl = dpp_row_shr1(el, m.w);
        vr = dpp_row_shl1(er, m.x);
    } else {
        const float4 lft = *reinterpret_cast<const float4*>(row - 4);
        m = *reinterpret_cast<const float4*>(row);
        const float4 rgt = *reinterpret_cast<const float4*>(row + 4);
        vl = lft.w;
        vr = rgt.x;
    }
    v[0] = vl; v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w; v[5] = vr;
}
template <Edge E>
__device__ __forceinline__ void stencil4(const float* __restrict__ p, const int (&ro)[3], int j, const float* __restrict__ k9, float bias, float (&out)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = bias;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        float v[6];
        row_taps<E>(p + ro[dy], j, v);
        const float k0 = k9[dy * 3], k1 = k9[dy * 3 + 1], k2 = k9[dy * 3 + 2];
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = fmaf(k2, v[q + 2], fmaf(k1, v[q + 1], fmaf(k0, v[q], out[q])));
    }
}

// The same stencil down a strip of consecutive rows, each input row read ONCE: input row i feeds output rows i - 2, i - 1 and i
// (numbered by their first input row) with kernel rows 2, 1 and 0.  acc[0] is the output row that this input row completes,
// acc[1] and acc[2] the two still open; the caller consumes acc[0] (from the third input row on) and calls roll_shift.  Every
// output is the fmaf chain of stencil4 in stencil4's order -- bias, kernel row 0, 1, 2 -- so the values are the same bit for bit.
__device__ __forceinline__ void roll_row(const float (&v)[6], const float (&k)[9], float bias, float (&acc)[3][4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[0][q] = fmaf(k[8], v[q + 2], fmaf(k[7], v[q + 1], fmaf(k[6], v[q], acc[0][q])));
        acc[1][q] = fmaf(k[5], v[q + 2], fmaf(k[4], v[q + 1], fmaf(k[3], v[q], acc[1][q])));
        acc[2][q] = fmaf(k[2], v[q + 2], fmaf(k[1], v[q + 1], fmaf(k[0], v[q], bias)));
    }
}
__device__ __forceinline__ void roll_shift(float (&acc)[3][4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { acc[0][q] = acc[1][q]; acc[1][q] = acc[2][q]; }
}

// ---- the attention projection ahead of the FFN (ffn_fused_kernel<32, true, FfnProj>; FfnProj: rf_common.h) -----------------------
// x1 = x + Wf v + b of one step, into the registers that hold x.  One b3 GEMM step against the image's folded weights `wa` (two
// output tiles of three pieces).  The MFMA leaves lane (j, kq) with output rows 16 t + 4 kq + r of its group; ln_step_b3 wants
// channel 8 kq + s in xh[s].  attn_fold_kernel wrote row 16 t + 4 a + r as channel 8 a + 4 t + r (fold_row_perm32), so
// acc[t][.][r] IS channel 8 kq + 4 t + r = xh[4 t + r]: no shuffle.  The bias is read by true channel.
template <int C>
__device__ __forceinline__ void proj_step_b3(const float4 (&vh)[C / 4], const u32x4 (&wa)[2][3], const float* __restrict__ bias, int kq, float4 (&xh)[C / 4]) {
    static_assert(C == 32, "one k-block, two output tiles");
    u32x4 bv[1][4][3];
    split_step<C>(vh, bv);
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        b3_mfma4(wa[t], bv[0], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = 4 * t + r;
            const float bs = bias[8 * kq + s];
            xh[s].x += acc[t][0][r] + bs; xh[s].y += acc[t][1][r] + bs;
            xh[s].z += acc[t][2][r] + bs; xh[s].w += acc[t][3][r] + bs;
        }
}
// ... and x1 of the step's groups into the LDS planes, at the offsets phase A uses (a group outside the image holds what offset 0
// gave: phase A zero-fills ITS output there, and the interior tile reads such a group only into lanes that never store)
template <int C>
__device__ __forceinline__ void stage_step(const float4 (&xh)[C / 4], float* __restrict__ mid, int PS, int kq, const GroupGeom& g) {
    if (g.lds_off >= 0) {
#pragma unroll
        for (int s = 0; s < C / 4; ++s) *reinterpret_cast<float4*>(mid + (32 * (s >> 3) + 8 * kq + (s & 7)) * PS + g.lds_off) = xh[s];
    }
}

// ================================================================================================
// FFN:  out = x1 + W2 gelu(dw3x3(W1 LN2(x1) + b1) + bd) + b2          (FfnArgs: rf_common.h)
// TAIL: the stage's channel_reduce on top,  out = Wa'_b xs + Wb x1 + (Wb W2) g + (Wb b2 + b_cr)  with g = gelu(..): Wb W2 takes
// the place of W2 in LDS (per image: a workgroup serves one), the composed bias that of b2, and x1 and xs enter as 16 more
// k-steps of the second GEMM.  Their B operands are the interior 4 x 64 tile in the lane map of the 1x1 kernels (lane (j, kq):
// one float4 of channel 4 s + kq), loaded where the tail-less kernel loads its residual rows -- behind the last phase A, when
// the b3 pieces are dead, and ahead of the tile's stores -- together with their A operands, which come from L2 (no LDS left for
// them); the MFMAs follow the last phase B.  No residual add: x1 arrives through Wb.
// PROJ (with TAIL): the attention projection on top, x1 = x + Wf_b v + b_proj per halo'd step ahead of LayerNorm (proj_step_b3), so
// x1 never exists in HBM: a.x is the block's input.  The interior x1 of the tail's k-steps is then not loadable: the lanes pass
// x1 of their groups through `mid` (free until part 0's phase A), every wave reads its row in the tail's lane map and issues the
// Wb x1 k-steps first, into the still-zero accumulators; only xs is loaded behind the last phase A.
// ================================================================================================
// Its operands (FfnProj) are a parameter pack, empty in the two other forms: their kernel arguments, and with them their code, are
// what they were without it (through a shared __device__ body, or with an empty third argument, they were not: tools/isa_same.py).
__device__ __forceinline__ FfnProj ffn_proj_of() { return FfnProj{nullptr, 0, nullptr, nullptr}; }
__device__ __forceinline__ FfnProj ffn_proj_of(const FfnProj& pj) { return pj; }
template <int C, bool TAIL, typename... PJ>
__global__ void __launch_bounds__(256, 2) ffn_fused_kernel(FfnArgs a, FfnTail tl, PJ... pjs) {
    constexpr bool PROJ = sizeof...(PJ) == 1;
    static_assert(sizeof...(PJ) <= 1 && (TAIL || !PROJ), "the projection form carries the stage tail");
    const FfnProj pj = ffn_proj_of(pjs...);
    using namespace fused;
    const int ro[3] = {0, HC, 2 * HC};   // a tile's halo'd rows are contiguous in LDS
    constexpr int NS = C / 4;            // k-sets of the first GEMM
    constexpr int NT1 = 2 * C / 16;      // output tiles of the first GEMM (hidden)
    constexpr int NTO = C / 16;          // output tiles of the second GEMM
    constexpr int NPART = 2 * C / PART;  // parts of 32 hidden channels
    constexpr int PS = 448;              // LDS plane stride (multiple of 64: kq planes on disjoint slots)
    // all weights live in LDS for the lifetime of the (persistent) workgroup
    __shared__ __attribute__((aligned(16))) float mid[PART * PS + 8];
    __shared__ __attribute__((aligned(16))) u32x4 w1_l[(C / 32) * NT1 * 192];      // b3 form (phase A runs on the bf16 instruction)
    __shared__ __attribute__((aligned(16))) float w2_l[(2 * C / 4) * NTO * 64];
    __shared__ float wd_l[2 * C * 9], bd_l[2 * C], b1_l[2 * C], b2_l[C], gam_l[C], bet_l[C];

    const int tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6;
    const int j0 = lane0 & 15, kq0 = lane0 >> 4;
    const int b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    const float* xb = a.x + (size_t)b * C * P;
    float* ob = a.out + (size_t)b * C * P;

    for (int i = tid; i < (C / 32) * NT1 * 192; i += 256) w1_l[i] = reinterpret_cast<const u32x4*>(a.w1p)[i];
    // TAIL: this image's [Wa' | Wb | Wb W2], k-sets [0, C/4) for xs, [C/4, 2C/4) for x1, the rest for g
    const float* tw = TAIL ? tl.wp + (size_t)b * tl.wp_bstride : nullptr;
    const float* w2src = TAIL ? tw + (2 * C / 4) * NTO * 64 : a.w2p;
    for (int i = tid; i < (2 * C / 4) * NTO * 16; i += 256) *reinterpret_cast<float4*>(w2_l + i * 4) = *reinterpret_cast<const float4*>(w2src + i * 4);
    for (int i = tid; i < 2 * C * 9; i += 256) wd_l[i] = a.wd[i];
    for (int i = tid; i < 2 * C; i += 256) { bd_l[i] = a.bd[i]; b1_l[i] = a.b1[i]; }
    for (int i = tid; i < C; i += 256) { gam_l[i] = a.ln_w[i]; bet_l[i] = a.ln_b[i]; b2_l[i] = a.b2[i]; }
    __syncthreads();
    STAMP_DECL
    const float* xsb = TAIL ? tl.xs + (size_t)b * C * P : nullptr;
    const float* vb = PROJ ? pj.v + (size_t)b * pj.v_bstride : nullptr;
    const u32x4* wf = PROJ ? reinterpret_cast<const u32x4*>(pj.wf3) + (size_t)b * (2 * 192) : nullptr;

    const TileRange tr = tile_range(a.ntiles, a.tiles_x, (int)gridDim.x, blockIdx.x);
    for (int tile = tr.begin; tile < tr.end; ++tile) {
        const int tx = tile / tr.tiles_y, ty = tile % tr.tiles_y;      // tile_origin, spelled out: through the helper this kernel's
        const int x0 = tx * TW, y0 = ty * TH;                          // prologue is scheduled differently (tools/isa_same.py)
        // PROJ: the lane coordinates are made opaque once per tile, as in ffn_fused8_kernel -- everything derived from them (LDS plane,
        // weight and stencil addresses: some 40 registers) is otherwise hoisted out of the tile loop, and with the projection's
        // operands on top of the parent's 226 registers 22 of them were spilled
        int j = j0, kq = kq0, lane = lane0;
        if constexpr (PROJ) asm volatile("" : "+v"(j), "+v"(kq), "+v"(lane));
        STAMP(0);
        // input tile, loaded here (see attn_front_kernel: the b3 pieces take the registers a tile in flight would need):
        // LayerNorm in registers, then the three-piece split that both parts of phase A reuse
        const GroupGeom gw0 = group_geom<GPW>(wave, 0, j, y0, x0, h, w), gw1 = group_geom<GPW>(wave, 1, j, y0, x0, h, w);
        u32x4 bp0[C / 32][4][3], bp1[C / 32][4][3];
        f32x4 accp[PROJ ? NTO : 1][4];                     // PROJ: Wb x1, the tile's first k-steps
        {
            float4 xh0[NS], xh1[NS];
            load_step_b3<C>(xb, P, kq, gw0, xh0);
            load_step_b3<C>(xb, P, kq, gw1, xh1);
            if constexpr (PROJ) {
                // v goes where x goes and is dead after its split; the folded weights come from L2 like the tail's A operands
                float4 vh0[NS], vh1[NS];
                load_step_b3<C>(vb, P, kq, gw0, vh0);
                load_step_b3<C>(vb, P, kq, gw1, vh1);
                const unsigned lo = (unsigned)lane;
                u32x4 wa[2][3];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) wa[t][pc] = (wf + (t * 3 + pc) * 64)[lo];
                proj_step_b3<C>(vh0, wa, pj.bias, kq, xh0);
                proj_step_b3<C>(vh1, wa, pj.bias, kq, xh1);
                // interior x1 in the lane map of the tail's k-steps (lane (j, kq): one float4 of channel 4 s + kq), through mid
                lds_barrier();                             // the previous tile's last phase B is done with mid
                stage_step<C>(xh0, mid, PS, kq, gw0);
                stage_step<C>(xh1, mid, PS, kq, gw1);
                lds_barrier();
#pragma unroll
                for (int t = 0; t < NTO; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) accp[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                float4 t1[C / 4];
                float a1[C / 4][NTO];
#pragma unroll
                for (int s = 0; s < C / 4; ++s) {
                    t1[s] = *reinterpret_cast<const float4*>(mid + (4 * s + kq) * PS + (wave + 1) * HC + 4 * j + 4);
#pragma unroll
                    for (int t = 0; t < NTO; ++t) a1[s][t] = (tw + ((C / 4 + s) * NTO + t) * 64)[lo];
                }
#pragma unroll
                for (int s = 0; s < C / 4; ++s) {
                    const float v[4] = {t1[s].x, t1[s].y, t1[s].z, t1[s].w};
#pragma unroll
                    for (int t = 0; t < NTO; ++t)
#pragma unroll
                        for (int q = 0; q < 4; ++q) accp[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s][t], v[q], accp[t][q], 0, 0, 0);
                }
                // (the barrier at the top of the part loop keeps phase A off mid until every wave has read its row)
            }
            ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh0);
            ln_step_b3<C>(kq, gam_l, bet_l, 1e-5f, xh1);
            split_step<C>(xh0, bp0);
            split_step<C>(xh1, bp1);
        }
        STAMP(1);

        const int yo = y0 + wave, xo = x0 + 4 * j;          // this lane's 4 output pixels
        const bool live = yo < h && xo < w;
        const unsigned voff = (unsigned)(4 * kq) * (unsigned)P + (unsigned)(live ? yo * w + xo : 0);
        float4 resv[NTO * 4];
        float4 tb[TAIL ? 2 * C / 4 : 1];                   // TAIL: B operands, k-steps of xs then of x1 ...
        float ta[TAIL ? 2 * C / 4 : 1][NTO];               // ... and their A operands
        f32x4 acc[NTO][4];
#pragma unroll
        for (int t = 0; t < NTO; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (PROJ) acc[t][q] = accp[t][q];
                else acc[t][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }

#pragma unroll
        for (int part = 0; part < NPART; ++part) {
            lds_barrier();                                 // previous phase B is done with mid
            STAMP(0);
            // ---- phase A: hidden[32 of part][halo tile] = W1 x^ + b1 -> LDS
            phase_a_step_b3<C, NT1>(bp0, w1_l + lane, 2 * part, 2 * part + 1, b1_l + part * PART, b1_l + part * PART + 16, mid, PS, kq, gw0);
            phase_a_step_b3<C, NT1>(bp1, w1_l + lane, 2 * part, 2 * part + 1, b1_l + part * PART, b1_l + part * PART + 16, mid, PS, kq, gw1);
            STAMP(2);
            if (part == NPART - 1) {
                if constexpr (TAIL) {
                    // this tile's xs and x1 rows and their weights, behind the last phase B (issued before this tile's stores)
                    const unsigned voffb = (unsigned)kq * (unsigned)P + (unsigned)(live ? yo * w + xo : 0);
#pragma unroll
                    for (int s = 0; s < C / 4; ++s) {
                        tb[s] = *reinterpret_cast<const float4*>(xsb + (size_t)(4 * s) * P + voffb);
                        if constexpr (!PROJ) tb[C / 4 + s] = *reinterpret_cast<const float4*>(xb + (size_t)(4 * s) * P + voffb);
                    }
                } else {
                // this tile's residual rows, behind the last phase B (issued before this tile's stores)
#pragma unroll
                for (int t = 0; t < NTO; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) resv[t * 4 + r] = *reinterpret_cast<const float4*>(xb + (size_t)(16 * t + r) * P + voff);
                }
            }
            lds_barrier();
            STAMP(0);
            // ---- phase B: depthwise 3x3 + GELU in registers, straight into the second GEMM
#pragma unroll
            for (int s = 0; s < PART / 4; ++s) {
                const int hc = 4 * s + kq;
                float v[4];
                stencil4<Edge::Dpp>(mid + hc * PS + wave * HC + 4 * j + 4, ro, j, wd_l + (part * PART + hc) * 9, bd_l[part * PART + hc], v);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = gelu_fast(v[q]);
#pragma unroll
                for (int t = 0; t < NTO; ++t) {
                    const float av = w2_l[((part * (PART / 4) + s) * NTO + t) * 64 + lane];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v[q], acc[t][q], 0, 0, 0);
                }
            }
            STAMP(3);
        }
        if constexpr (TAIL) {
            // uniform base + 32-bit lane offset, the lane made opaque per tile: per-lane 64-bit pointers to the 8 KB of weights would
            // be hoisted out of the tile loop and spilled
            constexpr int KT = PROJ ? C / 4 : 2 * C / 4;      // PROJ: the x1 k-steps went first
            unsigned lo = (unsigned)lane;
            asm volatile("" : "+v"(lo));
#pragma unroll
            for (int s = 0; s < KT; ++s)
#pragma unroll
                for (int t = 0; t < NTO; ++t) ta[s][t] = (tw + (s * NTO + t) * 64)[lo];
            // ---- the stage tail's k-steps: [Wa' | Wb] [xs ; x1] (a dead lane's columns hold whatever offset 0 gave: never stored)
#pragma unroll
            for (int s = 0; s < KT; ++s) {
                const float v[4] = {tb[s].x, tb[s].y, tb[s].z, tb[s].w};
#pragma unroll
                for (int t = 0; t < NTO; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta[s][t], v[q], acc[t][q], 0, 0, 0);
            }
            // ---- epilogue: + composed bias
            if (live) {
#pragma unroll
                for (int t = 0; t < NTO; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int cu = 16 * t + r;
                        const float bs = b2_l[cu + 4 * kq];
                        *reinterpret_cast<float4*>(ob + (size_t)cu * P + voff) =
                            make_float4(acc[t][0][r] + bs, acc[t][1][r] + bs, acc[t][2][r] + bs, acc[t][3][r] + bs);
                    }
            }
        } else {
        // ---- epilogue: + b2 + residual
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
        STAMP(4);
    }
    STAMP_FLUSH;
}

}  // namespace rf
