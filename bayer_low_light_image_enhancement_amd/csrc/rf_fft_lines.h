// The line transform both FFT files stand on (rf_fft.hip: rfft2 / irfft2 of FEB; rf_ffab_bwd.hip: their adjoints).
//
// A line of length n lives in LDS as n complex values.  n = 2^k: radix-2 decimation in time (bit-reversed load, k in-place stages,
// one barrier each).  Any other n: direct O(n^2) DFT out of the same LDS line with an exact twiddle index (j k mod n).  Twiddles
// come from sincospif (rf_fft.hip's header has the error account).
#pragma once
#include "rf_common.h"

namespace rf {

namespace {

constexpr int kMaxLine = 4096;          // longest line held in LDS (32 KB as float2)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__device__ __forceinline__ float2 twiddle(int k, int n, bool inverse) {   // exp(-+ 2 pi i k / n)
    float s, c;
    sincospif(2.0f * (float)k / (float)n, &s, &c);
    return make_float2(c, inverse ? s : -s);
}

// In-place transform of L independent lines of length n held in `buf` (line l at buf + l * n); `tmp` (same size) is
// only used by the generic path.  All 256 threads take part; ends with a barrier.  Unscaled.
__device__ void lds_fft_lines(float2* __restrict__ buf, float2* __restrict__ tmp, int n, int log2n, int L, bool inverse) {
    const int tid = threadIdx.x;
    if (log2n >= 0) {
        // bit reversal (in place: swap pairs once)
        for (int i = tid; i < L * n; i += 256) {
            const int l = i / n, k = i - l * n;
            const int r = (int)(__brev((unsigned)k) >> (32 - log2n));
            if (log2n > 0 && r > k) {
                float2* b = buf + l * n;
                const float2 t = b[k];
                b[k] = b[r];
                b[r] = t;
            }
        }
        __syncthreads();
        for (int s = 0; s < log2n; ++s) {
            const int half = 1 << s;
            for (int i = tid; i < L * (n >> 1); i += 256) {
                const int l = i / (n >> 1), q = i - l * (n >> 1);
                const int j = q & (half - 1), base = ((q >> s) << (s + 1)) + j;
                float2* b = buf + l * n;
                const float2 w = twiddle(j << (log2n - 1 - s), n, inverse);   // exp(-+2 pi i j / (2 half))
                const float2 u = b[base], v = cmul(b[base + half], w);
                b[base] = make_float2(u.x + v.x, u.y + v.y);
                b[base + half] = make_float2(u.x - v.x, u.y - v.y);
            }
            __syncthreads();
        }
    } else {
        for (int i = tid; i < L * n; i += 256) {
            const int l = i / n, k = i - l * n;
            const float2* b = buf + l * n;
            float2 acc = make_float2(0.f, 0.f);
            int jk = 0;                                   // j * k mod n, exact
            for (int j = 0; j < n; ++j) {
                const float2 w = twiddle(jk, n, inverse);
                const float2 v = b[j];
                acc.x = fmaf(v.x, w.x, fmaf(-v.y, w.y, acc.x));
                acc.y = fmaf(v.x, w.y, fmaf(v.y, w.x, acc.y));
                jk += k;
                if (jk >= n) jk -= n;
            }
            tmp[i] = acc;
        }
        __syncthreads();
        for (int i = tid; i < L * n; i += 256) buf[i] = tmp[i];
        __syncthreads();
    }
}

}  // namespace

}  // namespace rf
