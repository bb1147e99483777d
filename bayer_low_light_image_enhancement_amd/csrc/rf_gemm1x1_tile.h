// Pieces of the 1x1 GEMM kernels (rf_gemm1x1.hip has the overview) that a second translation unit needs: rf_gemm1x1_dw3.hip
// builds the bf16x3 streaming kernel whose third source is produced on the fly.  Every function is __forceinline__, and
// tools/isa_same.py shows that rf_gemm1x1.hip compiles to the code it had when they stood in it.
#pragma once
#include "rf_common.h"

namespace rf {

__device__ __forceinline__ float4 ldv(const float* __restrict__ base, unsigned off) {
    return *reinterpret_cast<const float4*>(base + off);
}

// channel pair (2 hp, 2 hp + 1) of pixel g -> dword hp of the three bf16 pieces of that pixel's B operand, bp[g][piece][hp]
template <class BP>
__device__ __forceinline__ void b3_split_pair(float xa, float xb, BP& bp, int g, int hp) {
    unsigned a0, a1, a2, b0, b1, b2;
    b3_split(xa, a0, a1, a2);
    b3_split(xb, b0, b1, b2);
    bp[g][0][hp] = b3_pack(a0, b0);
    bp[g][1][hp] = b3_pack(a1, b1);
    bp[g][2][hp] = b3_pack(a2, b2);
}

// Store NCO accumulator tiles.  bias_l: LDS bias of the first tile; res: prefetched residual rows
// (RES) laid out [tile][r] as float4.
template <int NCO, bool RES>
__device__ __forceinline__ void epilogue(const Conv1x1Args& a, f32x4 (&acc)[NCO][4], int tfirst, int ntiles,
                                         const float* __restrict__ bias_l, const float4* res,
                                         int b, int p0, int kq, bool live) {
    const int P = a.P;
    float* outb = a.out + (size_t)b * a.out_bstride;
    if (a.mode == 0) {
        const unsigned voff = (unsigned)(4 * kq) * (unsigned)P + (unsigned)p0;   // channel 4kq of a tile
#pragma unroll
        for (int t = 0; t < NCO; ++t) {
            if (t >= ntiles) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cu = 16 * (tfirst + t) + r;                  // wave-uniform part of the channel
                const float bs = bias_l[16 * t + 4 * kq + r];
                float v[4] = {acc[t][0][r] + bs, acc[t][1][r] + bs, acc[t][2][r] + bs, acc[t][3][r] + bs};
                if constexpr (RES) {
                    const float4 rv = res[t * 4 + r];
                    v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
                }
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
                if (live && cu + 4 * kq < a.Cout)
                    *reinterpret_cast<float4*>(outb + (size_t)cu * P + voff) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    } else {
        // ConvTranspose2d(k=2, s=2): GEMM row 4*o + 2*i + jj is output channel o at sub-position
        // (i, jj); the lane holds the whole 2x2 patch of each of its pixels for channel o.  The width only has to be
        // even: pixels (p0, p0+1) and (p0+2, p0+3) are each inside one row (p0 % 4 == 0), so every pixel PAIR is one
        // aligned 16-byte store per output row (at w = 266, level 3 of a 1424x2128 frame, the two pairs of a lane may
        // sit in different rows).
        const int w = a.w, w2 = 2 * a.w;
        const int ya = p0 / w, xa = p0 - ya * w;
        const int yb = (p0 + 2) / w, xb = (p0 + 2) - yb * w;
#pragma unroll
        for (int t = 0; t < NCO; ++t) {
            if (t >= ntiles) break;
            const int co = 16 * (tfirst + t) + 4 * kq;
            const int o = co >> 2;
            const float bs = bias_l[4 * t + kq];      // bias per real output channel o (staged as [NT*4])
            float* op = outb + (size_t)o * 4 * P;
            if (live && co < a.Cout) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    *reinterpret_cast<float4*>(op + (size_t)(2 * ya + i) * w2 + 2 * xa) =
                        make_float4(acc[t][0][2 * i] + bs, acc[t][0][2 * i + 1] + bs, acc[t][1][2 * i] + bs, acc[t][1][2 * i + 1] + bs);
                    *reinterpret_cast<float4*>(op + (size_t)(2 * yb + i) * w2 + 2 * xb) =
                        make_float4(acc[t][2][2 * i] + bs, acc[t][2][2 * i + 1] + bs, acc[t][3][2 * i] + bs, acc[t][3][2 * i + 1] + bs);
                }
            }
        }
    }
}

// bias (or zeros) for tiles [tbeg, tbeg + tpad) into LDS; mode 1 stores one value per output channel o
__device__ __forceinline__ void stage_bias(const Conv1x1Args& a, float* bias_l, int tbeg, int tpad, int tid) {
    if (a.mode == 0) {
        for (int i = tid; i < tpad * 16; i += 256) {
            const int co = 16 * tbeg + i;
            bias_l[i] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
        }
    } else {
        for (int i = tid; i < tpad * 4; i += 256) {
            const int o = 4 * tbeg + i;
            bias_l[i] = (a.bias && 4 * o < a.Cout) ? a.bias[o] : 0.f;
        }
    }
}

// channels 32c + 8kq + i (i = 0..7) of K block c, 4 pixels each: the block lies in ONE of up to three sources (launch_conv1x1
// checks that they are cut at multiples of 32 channels); selects, not branches (see kset_base)
__device__ __forceinline__ void b3_load_x_block(float4 (&xr)[8], const float* xb1, const float* xb2, const float* xb3, int C1, int C2, int C3,
                                                int c, int kq, unsigned P, unsigned pl) {
    const int cb = 32 * c;
    const bool first = cb < C1, third = cb >= C1 + C2;
    const float* src = first ? xb1 : third ? xb3 : xb2;
    const int cloc = first ? cb : third ? cb - C1 - C2 : cb - C1, cmax = (first ? C1 : third ? C3 : C2) - 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int ch = cloc + 8 * kq + i;
        ch = ch < cmax ? ch : cmax;
        xr[i] = ldv(src, (unsigned)ch * P + pl);
    }
}

}  // namespace rf
