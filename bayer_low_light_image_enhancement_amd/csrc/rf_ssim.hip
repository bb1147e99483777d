// SSIM of uint8 HWC images on the device (test.py:124, structural_similarity(a, b, channel_axis=-1)): 7x7 uniform window,
// K1 = 0.01, K2 = 0.03, data range 255, sample covariance, mean over the (h-6)(w-6) fully covered window positions.
//
// The inputs are bytes, so the five window sums Sx, Sy, Sxx, Syy, Sxy are exact integers (<= 49 * 255^2 = 3 186 225) and with
// n = 49, C1 = (K1 255)^2, C2 = (K2 255)^2 the value at a window position is
//   ((2 Sx Sy + C1 n^2) (2 (n Sxy - Sx Sy) + C2 n (n-1))) / ((Sx^2 + Sy^2 + C1 n^2) (n Sxx - Sx^2 + n Syy - Sy^2 + C2 n (n-1)))
// where every integer sub-expression fits int32: the four factors are one float64 rounding each from exact, then two products and
// one quotient.  What is left to rounding after that is the sum over positions, which is taken in a FIXED order (no float atomics).
//
// Layout: an HWC row is w*C interleaved bytes ("elements"); the horizontal window of element j is the taps j, j+C, .., j+6C, so the
// image is never deinterleaved.  A workgroup owns kSeg consecutive elements of a band of kBand output rows and walks down the band:
//   stage    each thread loads ONE aligned dword of the row per image (unconditional, address clamped into the buffer: the row need
//            not start on a dword, nor w*C be a multiple of 4) into a double-buffered LDS row; the loads of row i+1 are issued
//            before the arithmetic of row i and land in registers across the barrier
//   across   a thread owns 4 consecutive elements: 8 LDS dwords per image, shifted to its first element with v_alignbyte, bytes
//            picked at compile-time positions (the kernel is a template over C); Sx and Sy row sums share a dword
//   down     integer running sums: add the newest row's horizontal sums, subtract the row seven back, kept in a ring of seven rows
//            in registers (the row loop is unrolled by seven so that the ring is indexed statically: no scratch)
//   value    from the eighth row of the band on, one quotient per element per row, added to a per-element float64 accumulator
// At the end the workgroup adds its accumulators per channel in a fixed tree and writes C partials; u8_ssim_reduce_kernel adds the
// partials of an image in index order.  The partition depends on (h, w, C) only, so an image's sums are bitwise the same alone or
// in a batch and from run to run.
#include "rf_common.h"

namespace rf {

constexpr int kSsimWin = 7;
constexpr int kSsimThreads = 256;
constexpr int kSsimSeg = 4 * (kSsimThreads - 8);   // output elements per workgroup: 256 staged dwords = 1024 bytes >= 3 (row misalignment) + kSeg + 6 * 4 (halo)
constexpr int kSsimBand = 64;                      // output rows per workgroup (kBand + 6 rows read)
constexpr int kSsimRowDw = kSsimThreads + 8;       // LDS dwords per staged row: the last threads read (and discard) up to 7 past their own

struct SsimPlan { int nseg, nband; };
static inline SsimPlan ssim_plan(int C, int h, int w) {
    return {cdiv((w - (kSsimWin - 1)) * C, kSsimSeg), cdiv(h - (kSsimWin - 1), kSsimBand)};
}

template <int C>
__global__ void __launch_bounds__(kSsimThreads) u8_ssim_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                              double* __restrict__ partial, int h, int w, size_t total_bytes,
                                                              double c1, double c2) {
    constexpr int NB = 4 + 6 * C;             // bytes a thread's 4 elements reach
    constexpr int ND = (NB + 3) / 4;          // ... as dwords from its first element
    __shared__ __align__(16) unsigned rows[2][2][kSsimRowDw];

    const int tid = threadIdx.x;
    const int wb = w * C;                                   // bytes per row
    const int seg0 = blockIdx.x * kSsimSeg;                 // first element of the segment
    const int y0 = blockIdx.y * kSsimBand;                  // first output row of the band
    const int hout = h - (kSsimWin - 1);
    const int nin = min(kSsimBand, hout - y0) + (kSsimWin - 1);   // rows read
    const size_t img = (size_t)blockIdx.z * h * wb;

    // aligned-dword view of the two buffers; a row's dword index is clamped to the last dword holding a byte of the buffer
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    const unsigned* __restrict__ da = reinterpret_cast<const unsigned*>(a - (pa & 3));   // (derived from the argument: stays a global pointer)
    const unsigned* __restrict__ db = reinterpret_cast<const unsigned*>(b - (pb & 3));
    const size_t last_a = ((pa & 3) + total_bytes - 1) >> 2, last_b = ((pb & 3) + total_bytes - 1) >> 2;

    if (tid < 2 * 2 * 8) rows[tid >> 4][(tid >> 3) & 1][kSsimThreads + (tid & 7)] = 0;   // the tail no load writes

    bool ok[4];                                             // element inside the segment and inside the (w-6) C output elements
#pragma unroll
    for (int e = 0; e < 4; ++e) ok[e] = 4 * tid + e < kSsimSeg && seg0 + 4 * tid + e < (w - (kSsimWin - 1)) * C;

    unsigned ring[kSsimWin][4][4] = {};                     // [row mod 7][element][Sx | Sy << 16, Sxx, Syy, Sxy] horizontal sums
    unsigned run[4][4] = {};                                // the same summed over the last seven rows
    double acc[4] = {0.0, 0.0, 0.0, 0.0};

    size_t ra = (pa & 3) + img + (size_t)y0 * wb + seg0, rb = (pb & 3) + img + (size_t)y0 * wb + seg0;   // byte offsets of the row from da / db
    unsigned ga = da[min((ra >> 2) + tid, last_a)], gb = db[min((rb >> 2) + tid, last_b)];

#pragma unroll 1
    for (int base = 0; base < nin; base += kSsimWin) {
#pragma unroll
        for (int k = 0; k < kSsimWin; ++k) {
            const int i = base + k;
            if (i >= nin) break;
            const int buf = i & 1;
            const unsigned sha = (unsigned)ra & 3, shb = (unsigned)rb & 3;
            rows[buf][0][tid] = ga;
            rows[buf][1][tid] = gb;
            // next row's loads in flight over the barrier and this row's arithmetic (the last iteration reloads its own row)
            if (i + 1 < nin) { ra += wb; rb += wb; }
            ga = da[min((ra >> 2) + tid, last_a)];
            gb = db[min((rb >> 2) + tid, last_b)];
            __syncthreads();   // one barrier per row: buffer `buf` is next written two rows on, after the barrier of row i + 1

            unsigned xa[ND + 1], xb[ND + 1];
#pragma unroll
            for (int d = 0; d <= ND; ++d) { xa[d] = rows[buf][0][tid + d]; xb[d] = rows[buf][1][tid + d]; }
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                xa[d] = __builtin_amdgcn_alignbyte(xa[d + 1], xa[d], sha);
                xb[d] = __builtin_amdgcn_alignbyte(xb[d + 1], xb[d], shb);
            }
            unsigned x[NB], y[NB], xy[NB];
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                x[p] = (xa[p >> 2] >> (8 * (p & 3))) & 0xffu;
                y[p] = (xb[p >> 2] >> (8 * (p & 3))) & 0xffu;
                xy[p] = x[p] | (y[p] << 16);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
                for (int t = 0; t < kSsimWin; ++t) {
                    const int p = e + t * C;
                    s0 += xy[p];
                    s1 += x[p] * x[p];
                    s2 += y[p] * y[p];
                    s3 += x[p] * y[p];
                }
                run[e][0] += s0 - ring[k][e][0]; ring[k][e][0] = s0;
                run[e][1] += s1 - ring[k][e][1]; ring[k][e][1] = s1;
                run[e][2] += s2 - ring[k][e][2]; ring[k][e][2] = s2;
                run[e][3] += s3 - ring[k][e][3]; ring[k][e][3] = s3;
            }
            if (i >= kSsimWin - 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int sx = (int)(run[e][0] & 0xffffu), sy = (int)(run[e][0] >> 16);
                    const int sxx = (int)run[e][1], syy = (int)run[e][2], sxy = (int)run[e][3];
                    const int sxsy = sx * sy, sq = sx * sx + sy * sy;
                    const double a1 = (double)(2 * sxsy) + c1;
                    const double a2 = (double)(2 * (49 * sxy - sxsy)) + c2;
                    const double b1 = (double)sq + c1;
                    const double b2 = (double)(49 * (sxx + syy) - sq) + c2;
                    const double v = (a1 * a2) / (b1 * b2);
                    acc[e] += ok[e] ? v : 0.0;
                }
            }
        }
    }

    // per-channel sum of the workgroup in a fixed tree: lane, wave (xor butterfly), the four waves in order
    __syncthreads();
    double* wsum = reinterpret_cast<double*>(&rows[0][0][0]);   // [4 waves][C]
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (seg0 + 4 * tid + e) % C == c ? acc[e] : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) wsum[(tid >> 6) * C + c] = s;
    }
    __syncthreads();
    if (tid < C) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[wg * 4 + tid] = ((wsum[tid] + wsum[C + tid]) + wsum[2 * C + tid]) + wsum[3 * C + tid];
    }
}

// sums[image * C + c] = the image's workgroup partials of channel c: lane l adds partials l, l + 64, .. in order, then a butterfly
__global__ void __launch_bounds__(64) u8_ssim_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sums, int nwg, int C) {
    const int image = blockIdx.x / C, c = blockIdx.x % C;
    const double* p = partial + (size_t)image * nwg * 4 + c;
    double s = 0.0;
    for (int i = threadIdx.x; i < nwg; i += 64) s += p[(size_t)i * 4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

static int ssim_check_shape(int B, int C, int h, int w) {
    RF_CHECK_ARG(C >= 1 && C <= 4, "u8_ssim: %d channels (1..4 supported)", C);
    RF_CHECK_ARG(B >= 1 && B <= 65535, "u8_ssim: batch %d outside 1..65535", B);
    RF_CHECK_ARG(h >= kSsimWin && w >= kSsimWin, "u8_ssim: image %dx%d is smaller than the 7x7 window", h, w);
    const SsimPlan p = ssim_plan(C, h, w);
    RF_CHECK_ARG(p.nband <= 65535, "u8_ssim: image height %d too large", h);
    return RF_OK;
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_u8_ssim_scratch_bytes(int B, int C, int h, int w, size_t* bytes) {
    RF_CHECK_ARG(bytes, "u8_ssim_scratch_bytes: null output");
    RF_TRY(ssim_check_shape(B, C, h, w));
    const SsimPlan p = ssim_plan(C, h, w);
    *bytes = (size_t)B * p.nband * p.nseg * 4 * sizeof(double);
    return RF_OK;
}

int rf_u8_ssim(const unsigned char* a, const unsigned char* b, double* ssim_sums, void* scratch, int B, int C, int h, int w, void* stream) {
    RF_TRY(ssim_check_shape(B, C, h, w));
    RF_CHECK_ARG(a && b && ssim_sums && scratch, "u8_ssim: null pointer");
    RF_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(ssim_sums) & 7) == 0,
                 "u8_ssim: scratch and ssim_sums must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const SsimPlan p = ssim_plan(C, h, w);
    const dim3 grid((unsigned)p.nseg, (unsigned)p.nband, (unsigned)B);
    const size_t total = (size_t)B * h * w * C;
    const double n = kSsimWin * kSsimWin;
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0) * n * n, c2 = (0.03 * 255.0) * (0.03 * 255.0) * n * (n - 1.0);
    double* part = static_cast<double*>(scratch);
    {
        ProfScope prof(st, "u8_ssim_kernel", 0.0, 2.0 * total);
        switch (C) {
            case 1: u8_ssim_kernel<1><<<grid, kSsimThreads, 0, st>>>(a, b, part, h, w, total, c1, c2); break;
            case 2: u8_ssim_kernel<2><<<grid, kSsimThreads, 0, st>>>(a, b, part, h, w, total, c1, c2); break;
            case 3: u8_ssim_kernel<3><<<grid, kSsimThreads, 0, st>>>(a, b, part, h, w, total, c1, c2); break;
            default: u8_ssim_kernel<4><<<grid, kSsimThreads, 0, st>>>(a, b, part, h, w, total, c1, c2); break;
        }
        RF_TRY(check_launch("u8_ssim"));
    }
    u8_ssim_reduce_kernel<<<B * C, 64, 0, st>>>(part, ssim_sums, p.nband * p.nseg, C);
    return check_launch("u8_ssim_reduce");
}
}  // extern "C"
