// conv1x1_b3_dw3_kernel: the bf16x3 streaming GEMM (conv1x1_b3_kernel<4, false, false>, rf_gemm1x1.hip) whose THIRD source is
// produced on the fly -- x3 holds the FFN's hidden tensor before its depthwise 3x3 + GELU, and a K block that lies in source 3
// is stencilled and activated in registers instead of loaded.  The composed stage tail of level 1 (rf_model.hip, run_stage) then
// needs no dwconv3x3 launch, and the hidden tensor crosses HBM twice (written by the LayerNorm GEMM, read here) instead of
// four times.  In a translation unit of its own so that the kernels of rf_gemm1x1.hip compile exactly as they do without it.
//
// Pixel map: a workgroup's four waves own four consecutive rows of a 64-pixel column strip, p0 = (4 ty + wave) w + 64 tx + 4 j
// with ty fastest over the workgroup ids (w % 64 == 0, h % 4 == 0: every lane is live).  Six hidden rows then serve four output
// rows, and the rows that the waves of a workgroup share come from L1.  A wave is ONE image row, so the row masks of the stencil
// are scalar conditions.
//
// A hidden K block: lane (j, kq) owns channels 8 kq + i and pixels 4 j .. 4 j + 3 as in every other block.  Per channel it loads
// rows y - 1, y, y + 1 of its four pixels (three 16-byte loads, row addresses clamped, rows outside the image zero) and ONE dword
// per row for the edge taps: lane 0 the pixel left of the strip, lane 15 the pixel right of it (clamped, zero at the image
// border); every other lane takes its edge taps from lanes j - 1 / j + 1 over DPP and loads a word of a line it fetches anyway.
// The values then run through stencil4's chain (bias, kernel rows 0, 1, 2, each fmaf(k2, v[q + 2], fmaf(k1, v[q + 1],
// fmaf(k0, v[q], acc)))) and gelu_fast -- dwconv3x3_halo_kernel's operations in its order, so g has its bits -- and enter the split
// as channel pairs.  The loads of channel pair hp + 1 (of the next block's first pair behind the last one) are in flight while
// pair hp is in the VALU; the next block's weights are requested BEFORE that prefetch, so the wait that moves them to LDS does not
// cover it.  The K order, the six-term chains and the epilogue are those of conv1x1_b3_kernel: same bits per output.
#undef RF_STAMP
#include <type_traits>
#include "rf_gemm1x1_tile.h"
#include "rf_fused_tile.h"      // dpp_row_shr1 / dpp_row_shl1

namespace rf {

// keeps hipcc from moving the loads of later stages up (every stage would be in flight at once, in registers that do not exist)
#define RF_DW3_FENCE __builtin_amdgcn_sched_barrier(0)

struct Dw3Chan {           // one hidden channel of a block, raw: rows y - 1, y, y + 1
    float4 m[3];           // the lane's four pixels
    float e[3];            // lane 0: the pixel left of them; lane 15: the pixel right of them
};

template <int NCO>
__global__ void __launch_bounds__(256, 2) conv1x1_b3_dw3_kernel(Conv1x1Args a, Conv1x1Dw3 d) {
    __shared__ __attribute__((aligned(16))) u32x4 lds_w[2][NCO * 3 * 64];
    __shared__ float bias_l[NCO * 16];
    __shared__ float wd_l[kDw3MaxC3 * 9], bd_l[kDw3MaxC3];
    constexpr int WPT = (NCO * 3 * 64 + 255) / 256;   // 16-byte weight elements each thread moves per block
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y;
    const int P = a.P, w = d.w_, h = d.h;
    const int C12 = a.C1 + a.C2;
    const int NB12 = C12 >> 5, NB = (C12 + a.C3) >> 5;      // blocks of sources 1-2 (>= 2), all blocks (> NB12)
    const int NT = (a.Cout + 15) >> 4;
    const int tcnt = NT < NCO ? NT : NCO;
    const int th = h >> 2;
    const int ty = (int)blockIdx.x % th, tx = (int)blockIdx.x / th;
    const int y = 4 * ty + wave, x0 = 64 * tx + 4 * j;
    const int p0 = y * w + x0;
    const unsigned pl = (unsigned)p0;
    const u32x4* wp3 = reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(a.wp3) + (size_t)b * a.wp3_bstride);
    stage_bias(a, bias_l, 0, NCO, tid);
    for (int i = tid; i < 9 * a.C3; i += 256) wd_l[i] = d.w[i];
    for (int i = tid; i < a.C3; i += 256) bd_l[i] = d.bias ? d.bias[i] : 0.f;

    f32x4 acc[NCO][4];
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- stencil geometry: rows are wave-uniform, the edge column is the lane's
    const bool up_ok = y > 0, dn_ok = y + 1 < h;
    const unsigned rowoff[3] = {(unsigned)((up_ok ? y - 1 : 0) * w), (unsigned)(y * w), (unsigned)((dn_ok ? y + 1 : y) * w)};
    const bool right = j == 15;
    const bool e_ok = right ? x0 + 4 < w : x0 > 0;                       // lanes 0 and 15: the edge pixel exists
    const unsigned ex = (unsigned)(right ? (x0 + 4 < w ? x0 + 4 : x0) : (x0 > 0 ? x0 - 1 : 0));
    unsigned mo[3], eo[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { mo[r] = rowoff[r] + (unsigned)x0; eo[r] = rowoff[r] + ex; }

    float4 xr[8];
    u32x4 wr[WPT];
    const float* const xb1 = a.x1 + (size_t)b * (size_t)a.x1_bstride;
    const float* const xb2 = a.x2 + (size_t)b * (size_t)a.x2_bstride;
    const float* const xb3 = a.x3 + (size_t)b * (size_t)a.x3_bstride;      // the hidden tensor before the stencil
    auto load_x_block = [&](int c) { b3_load_x_block(xr, xb1, xb2, xb2, a.C1, a.C2, 0, c, kq, (unsigned)P, pl); };      // c < NB12
    auto load_w_block = [&](int c) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int idx = tid + 256 * i;                       // (t, piece, lane) of this workgroup's slice
            const int t = idx / 192, rem = idx - t * 192;
            const bool ok = idx < NCO * 192 && t < tcnt;
            const u32x4 v = wp3[((size_t)c * NT + (ok ? t : 0)) * 192 + (ok ? rem : 0)];
            wr[i] = ok ? v : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_w_block = [&](int buf) {
#pragma unroll
        for (int i = 0; i < WPT; ++i)
            if (tid + 256 * i < NCO * 192) lds_w[buf][tid + 256 * i] = wr[i];
    };
    // the three-piece split of a block of sources 1-2 (conv1x1_b3_kernel without LayerNorm)
    auto split_x = [&](u32x4 (&bp)[4][3]) {
#pragma unroll
        for (int hp = 0; hp < 4; ++hp) {
            const float xa[4] = {xr[2 * hp].x, xr[2 * hp].y, xr[2 * hp].z, xr[2 * hp].w};
            const float xb[4] = {xr[2 * hp + 1].x, xr[2 * hp + 1].y, xr[2 * hp + 1].z, xr[2 * hp + 1].w};
#pragma unroll
            for (int g = 0; g < 4; ++g) b3_split_pair(xa[g], xb[g], bp, g, hp);
        }
    };
    auto mma = [&](int c, const u32x4 (&bp)[4][3]) {
        const u32x4* wl = &lds_w[c & 1][lane];
#pragma unroll
        for (int t = 0; t < NCO; ++t) {
            const u32x4 ap[3] = {wl[(t * 3 + 0) * 64], wl[(t * 3 + 1) * 64], wl[(t * 3 + 2) * 64]};
            b3_mfma4(ap, bp, acc[t]);
        }
    };
    // hidden channel 32 (c - NB12) + 8 kq + i: three 16-byte loads and three dwords, branch-free
    auto load_chan = [&](int c, int i, Dw3Chan& r) {
        unsigned ch = (unsigned)(32 * (c - NB12) + 8 * kq + i);
        asm volatile("" : "+v"(ch));      // computed here: left to hipcc, the 48 offsets of a block become loop-carried registers
        const unsigned cb = ch * (unsigned)P;
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            r.m[row] = ldv(xb3, cb + mo[row]);
            r.e[row] = xb3[cb + eo[row]];
        }
    };
    // stencil + GELU of the channel's four pixels
    auto stencil_chan = [&](int c, int i, const Dw3Chan& r, float (&g)[4]) {
        const int ch = 32 * (c - NB12) + 8 * kq + i;
        const float* k9 = wd_l + 9 * ch;
        const float bias = bd_l[ch];
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = bias;
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            const bool rok = row == 0 ? up_ok : row == 2 ? dn_ok : true;
            const float4 m = r.m[row];
            const float e = e_ok ? r.e[row] : 0.f;
            const float vl = dpp_row_shr1(e, m.w), vr = dpp_row_shl1(e, m.x);
            const float v[6] = {rok ? vl : 0.f, rok ? m.x : 0.f, rok ? m.y : 0.f, rok ? m.z : 0.f, rok ? m.w : 0.f, rok ? vr : 0.f};
            const float k0 = k9[3 * row], k1 = k9[3 * row + 1], k2 = k9[3 * row + 2];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = fmaf(k2, v[q + 2], fmaf(k1, v[q + 1], fmaf(k0, v[q], g[q])));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = gelu_fast(g[q]);
        // the channel is finished HERE, ahead of the next load_chan (volatile statements keep their order): left alone, hipcc
        // sinks the arithmetic of all eight channels below the last load, and their raw rows are live together
        asm volatile("" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]));
    };
    // One hidden block: even channels arrive in ra, odd ones in rb, channel i + 1 in flight while channel i is in the VALU; a
    // pair of channels is dword hp of every operand of the block.  Behind the last channel's loads go the next block's weights
    // and then its first channel (LAST: nothing).
    Dw3Chan ra, rb;
    auto hidden_block = [&](int c, auto last, u32x4 (&bp)[4][3]) {
#pragma unroll
        for (int hp = 0; hp < 4; ++hp) {
            float g0[4], g1[4];
            load_chan(c, 2 * hp + 1, rb); RF_DW3_FENCE;
            stencil_chan(c, 2 * hp, ra, g0); RF_DW3_FENCE;
            if (hp < 3) {
                load_chan(c, 2 * hp + 2, ra); RF_DW3_FENCE;
            } else if constexpr (!decltype(last)::value) {
                load_w_block(c + 1);
                load_chan(c + 1, 0, ra); RF_DW3_FENCE;
            }
            stencil_chan(c, 2 * hp + 1, rb, g1); RF_DW3_FENCE;
#pragma unroll
            for (int q = 0; q < 4; ++q) b3_split_pair(g0[q], g1[q], bp, q, hp);
        }
    };

    load_x_block(0);
    load_w_block(0);
    store_w_block(0);
    __syncthreads();
    // ---- sources 1 and 2: the blocks of conv1x1_b3_kernel; the last one requests the first hidden channel instead of a next x
    for (int c = 0; c < NB12 - 1; ++c) {
        u32x4 bp[4][3];
        split_x(bp);
        load_x_block(c + 1);
        load_w_block(c + 1);
        mma(c, bp);
        store_w_block((c + 1) & 1);
        __syncthreads();
    }
    {
        const int c = NB12 - 1;
        u32x4 bp[4][3];
        split_x(bp);
        load_w_block(c + 1);
        load_chan(c + 1, 0, ra); RF_DW3_FENCE;
        mma(c, bp);
        store_w_block((c + 1) & 1);
        __syncthreads();
    }
    // ---- source 3
    for (int c = NB12; c < NB - 1; ++c) {
        u32x4 bp[4][3];
        hidden_block(c, std::false_type{}, bp);
        mma(c, bp);
        store_w_block((c + 1) & 1);
        __syncthreads();
    }
    {
        u32x4 bp[4][3];
        hidden_block(NB - 1, std::true_type{}, bp);
        mma(NB - 1, bp);
    }
    epilogue<NCO, false>(a, acc, 0, tcnt, bias_l, nullptr, b, p0, kq, true);
}

int launch_conv1x1_b3_dw3(const Conv1x1Args& a, const Conv1x1Dw3& d, const Conv1x1Plan& p, hipStream_t st) {
    RF_CHECK_ARG(p.dw3 && a.C3 > 0 && a.C3 <= kDw3MaxC3 && (a.C1 + a.C2) >= 32 && a.P == d.h * d.w_ && d.w_ % 64 == 0 && d.h % 4 == 0 &&
                 p.grid[0] == (unsigned)(a.P / 256), "conv1x1 (third source on the fly): not planned for these arguments");
    conv1x1_b3_dw3_kernel<4><<<dim3(p.grid[0], p.grid[1], 1), 256, 0, st>>>(a, d);
    return RF_OK;
}

}  // namespace rf
