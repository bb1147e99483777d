// FEB / FFAB (RawFomer_WFB_FFAB/blocks.py:11-92): the frequency block of the WFB variant.
//
//   FEB(x) = clamp( irfft2( polar( clamp(MLP1(|F| + 1e-6), 0, 1e4), MLP2(angle F) ) ) + clamp(x) ),  F = rfft2(fpre(clamp x))
//
// with norm='ortho' transforms over the last two axes.  Both transforms are hand-written, line-in-LDS kernels:
//
//   rfft2  = [row pass]    real row of length w  -> half spectrum (wf = w/2 + 1 complex), scaled 1/sqrt(w)
//            [column pass] complex FFT of length h over every one of the wf columns, scaled 1/sqrt(h); its epilogue
//                          turns the spectrum into the two REAL planes the MLPs read: |F| + 1e-6 and atan2(Im, Re)
//   irfft2 = [column pass] its prologue turns (mag, pha) into mag cos(pha) + i mag sin(pha); inverse FFT of length h
//            [row pass]    Hermitian half spectrum -> real row (Im of the DC / Nyquist bins ignored, as pocketfft's c2r
//                          does); epilogue: + clamp(x, -10, 10), clamp(-10, 10)
//
// (lds_fft_lines lives in rf_fft_lines.h, shared with the adjoints of rf_ffab_bwd.hip.)
// A line of length n lives in LDS as n complex values.  n = 2^k: radix-2 decimation in time (bit-reversed load, k
// in-place stages, one barrier each).  Any other n (e.g. 712 x 1072 = the LL band of a packed 1424 x 2144 frame, a SID frame
// padded to the multiple of 32 variant='wfb' asks of the width): direct O(n^2) DFT out of the same LDS line with an exact
// twiddle index (j k mod n) -- a correctness path, ~n/log2(n) times the work.
// Twiddles come from sincospif.  Its argument 2 k / n is exact in float only for a power of two n, where the error
// growth matches a table-driven host FFT (pocketfft in the reference: O(1e-7 log n) relative); for any other n the quotient is
// rounded once, a phase error of at most 2^-24 * 2 pi per twiddle (tests/test_fft_lines.py measures what the n terms add up to).
//
// The four bins of a real 2-D transform that are real by symmetry -- (0|h/2, 0|w/2) -- get Im = +0 exactly, as the
// reference produces them: angle() of a negative real must be +pi, not -pi (it feeds a 1x1 MLP, i.e. is NOT 2 pi
// periodic downstream).  Elsewhere a phase within rounding of the +-pi cut is ill-conditioned in the reference too;
// tests state their tolerance accordingly.
#include <climits>
#include "rf_fft_lines.h"

namespace rf {

namespace {

static int ilog2_exact(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return (1 << l) == n ? l : -1;
}

// ---- forward row pass: real rows [rows][w] -> half spectrum [rows][wf] complex, scaled by `scale`
__global__ void __launch_bounds__(256) fft_rows_r2c_kernel(const float* __restrict__ in, float2* __restrict__ out, int rows, int w,
                                                           int log2w, int L, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;
    float2* tmp = fft_lds + L * w;
    const int wf = w / 2 + 1;
    for (int r0 = blockIdx.x * L; r0 < rows; r0 += gridDim.x * L) {
        const int nl = rows - r0 < L ? rows - r0 : L;
        for (int i = threadIdx.x; i < L * w; i += 256) {
            const int l = i / w, k = i - l * w;
            buf[i] = make_float2(l < nl ? in[(size_t)(r0 + l) * w + k] : 0.f, 0.f);
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, w, log2w, L, false);
        for (int i = threadIdx.x; i < nl * wf; i += 256) {
            const int l = i / wf, k = i - l * wf;
            float2 v = buf[l * w + k];
            v.x *= scale; v.y *= scale;
            if (k == 0 || 2 * k == w) v.y = 0.f;          // real by symmetry
            out[(size_t)(r0 + l) * wf + k] = v;
        }
        __syncthreads();
    }
}

// ---- column passes.  One workgroup owns TC consecutive columns of one [h][wf] plane: line c is column c0 + c.
// forward: complex in -> FFT -> (|F| + 1e-6, angle F) planes.   inverse: (mag, pha) planes -> polar -> inverse FFT -> complex out
template <bool INVERSE>
__global__ void __launch_bounds__(256) fft_cols_kernel(const float2* __restrict__ cin, float2* __restrict__ cout_, const float* __restrict__ mag_in,
                                                       const float* __restrict__ pha_in, float* __restrict__ mag_out, float* __restrict__ pha_out,
                                                       int planes, int h, int wf, int w_even_nyq, int log2h, int TC, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;                    // [TC][h]
    float2* tmp = fft_lds + TC * h;
    const int ctiles = (wf + TC - 1) / TC;
    for (int unit = blockIdx.x; unit < planes * ctiles; unit += gridDim.x) {
        const int pl = unit / ctiles, c0 = (unit - pl * ctiles) * TC;
        const size_t pbase = (size_t)pl * h * wf;
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;          // consecutive threads read consecutive columns of a row
            float2 v = make_float2(0.f, 0.f);
            if (c0 + c < wf) {
                const size_t g = pbase + (size_t)y * wf + c0 + c;
                if constexpr (INVERSE) {
                    const float m = mag_in[g], p = pha_in[g];
                    float s, co;
                    sincosf(p, &s, &co);
                    v = make_float2(m * co, m * s);
                } else {
                    v = cin[g];
                }
            }
            buf[c * h + y] = v;
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, h, log2h, TC, INVERSE);
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;
            if (c0 + c >= wf) continue;
            float2 v = buf[c * h + y];
            v.x *= scale; v.y *= scale;
            const size_t g = pbase + (size_t)y * wf + c0 + c;
            if constexpr (INVERSE) {
                cout_[g] = v;
            } else {
                const int k2 = c0 + c;
                if ((k2 == 0 || k2 == w_even_nyq) && (y == 0 || 2 * y == h)) v.y = 0.f;     // the four real bins: Im = +0
                mag_out[g] = sqrtf(v.x * v.x + v.y * v.y) + 1e-6f;
                pha_out[g] = atan2f(v.y, v.x);
            }
        }
        __syncthreads();
    }
}

// ---- inverse row pass: half spectrum [rows][wf] -> real rows [rows][w]; out = clamp(scale * x + clamp(res))
__global__ void __launch_bounds__(256) fft_rows_c2r_kernel(const float2* __restrict__ in, const float* __restrict__ res, float* __restrict__ out,
                                                           int rows, int w, int log2w, int L, float scale, float lim) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;
    float2* tmp = fft_lds + L * w;
    const int wf = w / 2 + 1;
    for (int r0 = blockIdx.x * L; r0 < rows; r0 += gridDim.x * L) {
        const int nl = rows - r0 < L ? rows - r0 : L;
        for (int i = threadIdx.x; i < L * w; i += 256) {
            const int l = i / w, k = i - l * w;
            float2 v = make_float2(0.f, 0.f);
            if (l < nl) {
                if (k < wf) {
                    v = in[(size_t)(r0 + l) * wf + k];
                    if (k == 0 || 2 * k == w) v.y = 0.f;                   // c2r ignores Im of DC / Nyquist
                } else {
                    v = in[(size_t)(r0 + l) * wf + (w - k)];
                    v.y = -v.y;                                            // Hermitian extension
                }
            }
            buf[i] = v;
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, w, log2w, L, true);
        for (int i = threadIdx.x; i < nl * w; i += 256) {
            const int l = i / w, k = i - l * w;
            const size_t g = (size_t)(r0 + l) * w + k;
            float v = buf[l * w + k].x * scale;
            if (res) v += fminf(fmaxf(res[g], -lim), lim);
            out[g] = fminf(fmaxf(v, -lim), lim);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) clamp_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, float lo, float hi) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = fminf(fmaxf(in[i], lo), hi);
}

}  // namespace

static int fft_geometry(int n, const char* what, int* log2n) {
    RF_CHECK_ARG(n >= 2 && n <= kMaxLine, "%s: transform length %d outside [2, %d]", what, n, kMaxLine);
    *log2n = ilog2_exact(n);
    RF_CHECK_ARG(*log2n >= 0 || n <= 2048, "%s: non-power-of-two length %d > 2048 not supported", what, n);
    return RF_OK;
}

int plan_fft(const char* what, int planes, int h, int w, FftPlan* p) {
    RF_CHECK_ARG(w % 2 == 0, "%s: width %d must be even (irfft2 with s=(H,W) inverts rfft2 only then)", what, w);
    if (int rc = fft_geometry(w, what, &p->log2w)) return rc;
    if (int rc = fft_geometry(h, what, &p->log2h)) return rc;
    p->wf = w / 2 + 1;
    // the kernels count lines and column tiles in int, and step past the last one by up to a grid of them
    RF_CHECK_ARG(planes >= 1 && (int64_t)planes * h <= INT_MAX / 2 && (int64_t)planes * p->wf <= INT_MAX / 2,
                 "%s: %d planes of %d x %d: more than 2^30 lines", what, planes, h, w);
    p->rows = planes * h;
    p->L = 2048 / w; if (p->L < 1) p->L = 1;
    p->TC = 2048 / h; if (p->TC < 1) p->TC = 1; if (p->TC > 16) p->TC = 16;
    p->units = planes * cdiv(p->wf, p->TC);
    const int groups = cdiv(p->rows, p->L);
    p->gx = groups > 4096 ? 4096 : groups;
    p->gy = p->units > 4096 ? 4096 : p->units;
    // the line and the direct path's `tmp` line of the same size: 64 KB at n = 4096, the most a launch gets without opting in
    p->lds_rows = (size_t)2 * p->L * w * sizeof(float2);
    p->lds_cols = (size_t)2 * p->TC * h * sizeof(float2);
    return RF_OK;
}

// rfft2 (ortho) of [planes][h][w] followed by |.| + 1e-6 and angle: mag / pha are [planes][h][w/2 + 1]; `cscratch` holds
// planes * h * (w/2 + 1) complex values
int launch_rfft2_polar(const float* in, float* mag, float* pha, float2* cscratch, int planes, int h, int w, hipStream_t st) {
    FftPlan p;
    RF_TRY(plan_fft("rfft2", planes, h, w, &p));
    ProfScope prof(st, "rfft2_polar(2 kernels)", 0.0, 4.0 * planes * ((double)h * w + 6.0 * h * p.wf));
    fft_rows_r2c_kernel<<<p.gx, 256, p.lds_rows, st>>>(in, cscratch, p.rows, w, p.log2w, p.L, 1.0f / sqrtf((float)w));
    fft_cols_kernel<false><<<p.gy, 256, p.lds_cols, st>>>(cscratch, nullptr, nullptr, nullptr, mag, pha, planes, h, p.wf, w / 2, p.log2h, p.TC,
                                                          1.0f / sqrtf((float)h));
    return check_launch("rfft2_polar");
}

// the row pass of launch_rfft2_polar alone: the half spectrum of every row, scaled 1/sqrt(w), into `cscratch` (the backward's
// column kernel transforms it again, rf_ffab_bwd.hip)
int launch_rfft_rows(const float* in, float2* cscratch, int planes, int h, int w, hipStream_t st) {
    FftPlan p;
    RF_TRY(plan_fft("rfft2", planes, h, w, &p));
    ProfScope prof(st, "rfft_rows", 0.0, 4.0 * planes * ((double)h * w + 2.0 * h * p.wf));
    fft_rows_r2c_kernel<<<p.gx, 256, p.lds_rows, st>>>(in, cscratch, p.rows, w, p.log2w, p.L, 1.0f / sqrtf((float)w));
    return check_launch("rfft_rows");
}

// irfft2 (ortho, s = (h, w)) of mag * exp(i pha), then out = clamp(. + clamp(res, +-lim), +-lim)   (res may be null)
int launch_polar_irfft2(const float* mag, const float* pha, const float* res, float* out, float2* cscratch, int planes, int h, int w,
                        float lim, hipStream_t st) {
    FftPlan p;
    RF_TRY(plan_fft("irfft2", planes, h, w, &p));
    ProfScope prof(st, "polar_irfft2(2 kernels)", 0.0, 4.0 * planes * (2.0 * h * w + 6.0 * h * p.wf));
    fft_cols_kernel<true><<<p.gy, 256, p.lds_cols, st>>>(nullptr, cscratch, mag, pha, nullptr, nullptr, planes, h, p.wf, w / 2, p.log2h, p.TC,
                                                         1.0f / sqrtf((float)h));
    fft_rows_c2r_kernel<<<p.gx, 256, p.lds_rows, st>>>(cscratch, res, out, p.rows, w, p.log2w, p.L, 1.0f / sqrtf((float)w), lim);
    return check_launch("polar_irfft2");
}

int launch_clamp(const float* in, float* out, size_t n, float lo, float hi, hipStream_t st) {
    int gx = (int)((n + 255) / 256); if (gx > 4096) gx = 4096;
    clamp_kernel<<<gx, 256, 0, st>>>(in, out, n, lo, hi);
    return check_launch("clamp");
}

}  // namespace rf
