// Device code the forward guidance and gate kernels share -- rf_flca.hip (base FLCA), rf_truecolor.hip (TrueColor), rf_multilvl.hip
// (multi-level FLCA), and rf_flca_bwd.hip for the fast sigmoid -- and the pyramid descriptor their host schedules lay out:
//   * the reference's conventions, one statement each: the packed-or-mosaic Bayer read (packed_at), F.interpolate's bilinear
//     sampling with align_corners=False (bilerp), one Haar step of a 2x2 block (haar_ll_mag), the per-image luma maximum
//     (block_max_atomic);
//   * the fast sigmoid / tanh of the forward's spatial gates;
//   * the steps of a gate kernel: the zero-padded guidance neighbourhood of a lane's pixels (guide_nb), the FLCA_Pyramid gate
//     heads (ml_gate_heads), a lane's PX pixels of a feature row (load_px / store_px).
// Every fmaf chain and every sum keeps the order it had written out in the kernels: the bits are those of
// tests/golden/guidance_parent.json.  Which kernels compile to the same gfx950 code as before and which do not: DESIGN.md section 4.
#pragma once
#include "rf_common.h"

namespace rf {

// Haar pyramid of the luma below an H x W frame: LL and high-band magnitude of level i, [B][lh[i]][lw[i]].  The tail of
// TcGuideSrc and MlGuideSrc (kernel arguments) and of the two scratch layouts.
struct GuidePyramid {
    float* ll[3]; float* mag[3];
    int lh[3], lw[3];
    int levels;
};
// Levels first .. levels - 1 on `b`, each half the size (rounded up) of the one above; h x w is the plane above level `first`.
// Returns the floats of the planes themselves (the Bump rounds each up).
inline size_t pyramid_layout(GuidePyramid& p, Bump& b, int B, int h, int w, int first, int levels) {
    size_t floats = 0;
    for (int i = first; i < levels; ++i) {
        h = (h + 1) / 2; w = (w + 1) / 2;
        p.lh[i] = h; p.lw[i] = w;
        p.ll[i] = b.take((size_t)B * h * w); p.mag[i] = b.take((size_t)B * h * w);
        floats += 2 * (size_t)B * h * w;
    }
    p.levels = levels;
    return floats;
}

#ifdef __HIPCC__
namespace {

// ---- scalar helpers

// sigmoid / tanh on v_exp_f32 + v_rcp_f32 (about 1 ulp each, far below the parity budget); the accurate forms are sigm / tanhf
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// channel ch of packed pixel (y, x) of image b: from packed RGGB [B][4][H][W] or from the mosaic [B][2H][2W] itself
__device__ __forceinline__ float packed_at(const float* in, int mosaic, int clamp_in, size_t b, int ch, int y, int x, int H, int W) {
    float v = mosaic ? in[(b * 2 * H + 2 * y + (ch >> 1)) * (size_t)(2 * W) + 2 * x + (ch & 1)]
                     : in[((b * 4 + ch) * H + y) * (size_t)W + x];
    return clamp_in ? fminf(fmaxf(v, 0.f), 1.f) : v;
}

// F.interpolate(mode='bilinear', align_corners=False): half-pixel offset, source coordinate clamped at 0, index at the last
__device__ __forceinline__ float bilerp(const float* __restrict__ src, int hi, int wi, int ho, int wo, int y, int x) {
    const float sy = fmaxf(((float)y + 0.5f) * ((float)hi / (float)ho) - 0.5f, 0.f);
    const float sx = fmaxf(((float)x + 0.5f) * ((float)wi / (float)wo) - 0.5f, 0.f);
    int y0 = (int)sy, x0 = (int)sx;
    if (y0 > hi - 1) y0 = hi - 1;
    if (x0 > wi - 1) x0 = wi - 1;
    const int y1 = y0 + (y0 < hi - 1), x1 = x0 + (x0 < wi - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float top = src[(size_t)y0 * wi + x0] * (1.f - lx) + src[(size_t)y0 * wi + x1] * lx;
    const float bot = src[(size_t)y1 * wi + x0] * (1.f - lx) + src[(size_t)y1 * wi + x1] * lx;
    return top * (1.f - ly) + bot * ly;
}

// one Haar step of the 2x2 block v = (top left, top right, bottom left, bottom right): LL and the high-band magnitude
__device__ __forceinline__ void haar_ll_mag(const float (&v)[4], float& ll, float& mag) {
    ll = (v[0] + v[1] + v[2] + v[3]) * 0.5f;
    const float lh = (v[0] - v[1] + v[2] - v[3]) * 0.5f, hl = (v[0] + v[1] - v[2] - v[3]) * 0.5f, hh = (v[0] - v[1] - v[2] + v[3]) * 0.5f;
    mag = sqrtf(lh * lh + hl * hl + hh * hh + 1e-8f);
}

// ---- per-image maximum: amax[b] holds the bit pattern of a float, -inf before the first atomic (launch_guide_init, rf_flca.hip)
__device__ __forceinline__ void atomic_max_float(int* addr, float v) {
    if (v >= 0.f) atomicMax(addr, __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// maximum of m over a workgroup of 256 threads, then one atomic per workgroup: all of an image's atomics hit one address
__device__ __forceinline__ void block_max_atomic(float m, int* addr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        if (m > -INFINITY) atomic_max_float(addr, m);
    }
}

// ---- steps of a gate kernel.  A lane owns PX consecutive pixels of row y, starting at column x, of an h x w plane (P = h w).

// nb[pl][dy][dx] = plane pl (P floats apart) at (y + dy - 1, x + dx - 1), zero outside the plane and where the lane has no pixels
template <int PL, int PX>
__device__ __forceinline__ void guide_nb(float (&nb)[PL][3][PX + 2], const float* planes, int P, int y, int x, int h, int w, bool live) {
#pragma unroll
    for (int pl = 0; pl < PL; ++pl)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < PX + 2; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                const bool ok = live && yy >= 0 && yy < h && xx >= 0 && xx < w;
                nb[pl][dy][dx] = ok ? planes[(size_t)pl * P + (size_t)yy * w + xx] : 0.f;
            }
}

// The gate heads of one FLCA_Pyramid step from the image's means table mn (wave-uniform).  Level form: g0, g1 = sigmoid of the
// 2 -> 2 affine map freq_gate_head[level] of (mean y_low, mean y_high); chroma form: g0 = sigmoid(chroma_gate(mean magnitude))
template <bool CHROMA>
__device__ __forceinline__ void ml_gate_heads(const float* mn, const float* gate_w, const float* gate_b, int level, float& g0, float& g1) {
    if constexpr (CHROMA) {
        g0 = fast_sigmoid(fmaf(gate_w[0], mn[6], gate_b[0]));
    } else {
        const float lo = mn[2 * level], hi = mn[2 * level + 1];
        g0 = fast_sigmoid(fmaf(gate_w[1], hi, fmaf(gate_w[0], lo, gate_b[0])));
        g1 = fast_sigmoid(fmaf(gate_w[3], hi, fmaf(gate_w[2], lo, gate_b[1])));
    }
}

// the lane's PX pixels of a feature row: one float4 (PX = 4, p 16-byte aligned) or one float
template <int PX>
__device__ __forceinline__ void load_px(const float* p, float (&v)[PX]) {
    if constexpr (PX == 4) {
        const float4 f4 = *reinterpret_cast<const float4*>(p);
        v[0] = f4.x; v[1] = f4.y; v[2] = f4.z; v[3] = f4.w;
    } else {
        v[0] = p[0];
    }
}
template <int PX>
__device__ __forceinline__ void store_px(float* p, const float (&v)[PX]) {
    if constexpr (PX == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

}  // namespace
#endif

}  // namespace rf
