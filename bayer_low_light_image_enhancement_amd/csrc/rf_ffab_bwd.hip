// Adjoint of FEB / ProcessBlock / FFAB (rf_ffab.hip, rf_fft.hip; RawFomer_WFB_FFAB/blocks.py:11-92): (x, dL/dout, parameters) ->
// dL/dx and the parameter gradients.  Nothing is kept from a forward call.  With the forward
//
//   xc = clamp(x, +-10),  y = fpre(xc),  F = rfft2(y),  mag = |F| + 1e-6,  pha = angle F
//   t1 = lrelu(process1.0(mag)),  a = process1.2(t1),  m = clamp(a, 0, 1e4)
//   t2 = lrelu(process2.0(pha)),  p = process2.2(t2)
//   s = irfft2(m e^{i p}) + xc,   out = clamp(s, +-10)
//
// recomputed by the forward's own kernels (s: polar_irfft2 with the residual and an unbounded clamp), the backward of one FEB is
//
//   gs        = g where -10 <= s <= 10                                  mask_range_kernel
//   gm, gp    = adjoint of polar + irfft2 at (m, p) of gs               adj_rows_r2c_kernel, adj_cols_polar_kernel
//   ga        = gm where 0 <= a <= 1e4
//   process1  dW, db = wgrad(ga, t1);  gt = W^T ga, times lrelu'(t1);  dW, db = wgrad(gt, mag);  gmag = W^T gt
//   process2  the same from gp through t2 and pha to gpha
//   gy        = adjoint of rfft2 + polar at F of (gmag, gpha)           launch_rfft_rows, adj_cols_rfft_kernel, adj_rows_c2r_kernel
//   fpre      dW, db = wgrad(gy, xc);  gx = (W^T gy + gs) where -10 <= x <= 10
//
// wgrad = wgrad1x1 (rf_grad.hip): launch_gram2 with one tap where the plane's pixel count is a multiple of 4, else wgrad1x1_kernel;
// W^T g = dgrad1x1: launch_conv1x1 on a transposed pack.  Both transforms are norm='ortho' and linear, so their adjoints are
// transforms of the other direction over the same lines in LDS (rf_fft_lines.h); what differs from irfft2 / rfft2 is the treatment
// of the half spectrum:
//
//   adjoint of rfft2:   the half spectrum G (wf = w/2 + 1 columns) is zero-extended, NOT Hermitian-extended, and nothing is
//                       doubled:  gy[x] = Re sum_{k < wf} G_k e^{+2 pi i k x / w} / sqrt(w)
//   adjoint of irfft2:  c2r reads columns 1 .. w/2 - 1 twice (once conjugated) and ignores Im of columns 0 and w/2, so the
//                       forward-direction row spectrum of gs is doubled on the interior columns and loses Im on the two others.
//
// Every sum over pixels goes to per-workgroup slabs that a second kernel adds in a fixed order: no atomics, two runs give the same bits.
#include <cmath>
#include "rf_fft_lines.h"
#include "rf_grad.h"

namespace rf {

namespace {

// ---- adjoint of fft_rows_c2r_kernel: real rows [rows][w] -> forward-direction half spectrum [rows][wf], scaled; interior columns
// doubled, Im of columns 0 and w/2 dropped
__global__ void __launch_bounds__(256) adj_rows_r2c_kernel(const float* __restrict__ in, float2* __restrict__ out, int rows, int w, int log2w,
                                                           int L, float scale) {
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
            if (k == 0 || 2 * k == w) {
                v.x *= scale; v.y = 0.f;
            } else {
                v.x *= 2.0f * scale; v.y *= 2.0f * scale;
            }
            out[(size_t)(r0 + l) * wf + k] = v;
        }
        __syncthreads();
    }
}

// ---- adjoint of fft_cols_kernel<true>: complex [h][wf] planes -> forward column FFT, scaled -> (gm, gp) at the polar point (m, p)
__global__ void __launch_bounds__(256) adj_cols_polar_kernel(const float2* __restrict__ cin, const float* __restrict__ mag, const float* __restrict__ pha,
                                                             float* __restrict__ gmag, float* __restrict__ gpha, int planes, int h, int wf, int log2h,
                                                             int TC, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;                    // [TC][h]
    float2* tmp = fft_lds + TC * h;
    const int ctiles = (wf + TC - 1) / TC;
    for (int unit = blockIdx.x; unit < planes * ctiles; unit += gridDim.x) {
        const int pl = unit / ctiles, c0 = (unit - pl * ctiles) * TC;
        const size_t pbase = (size_t)pl * h * wf;
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;
            buf[c * h + y] = c0 + c < wf ? cin[pbase + (size_t)y * wf + c0 + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, h, log2h, TC, false);
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;
            if (c0 + c >= wf) continue;
            const float2 v = buf[c * h + y];
            const size_t g = pbase + (size_t)y * wf + c0 + c;
            const float m = mag[g];
            float s, co;
            sincosf(pha[g], &s, &co);
            const float gr = v.x * scale, gi = v.y * scale;
            gmag[g] = gr * co + gi * s;
            gpha[g] = m * (gi * co - gr * s);
        }
        __syncthreads();
    }
}

// ---- adjoint of fft_cols_kernel<false>: the row spectrum `cin` of the forward is transformed again to F (the forward's arithmetic),
// G = gmag F/|F| + gpha (-Im F, Re F)/|F|^2 (0 where F = 0; no Im at the four bins the forward forces real), then the
// inverse-direction column transform, scaled.  cout_ may be cin: a workgroup reads its tile whole before it writes it.
__global__ void __launch_bounds__(256) adj_cols_rfft_kernel(const float2* cin, const float* __restrict__ gmag, const float* __restrict__ gpha,
                                                            float2* cout_, int planes, int h, int wf, int w_even_nyq, int log2h, int TC,
                                                            float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;                    // [TC][h]
    float2* tmp = fft_lds + TC * h;
    const int ctiles = (wf + TC - 1) / TC;
    for (int unit = blockIdx.x; unit < planes * ctiles; unit += gridDim.x) {
        const int pl = unit / ctiles, c0 = (unit - pl * ctiles) * TC;
        const size_t pbase = (size_t)pl * h * wf;
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;
            buf[c * h + y] = c0 + c < wf ? cin[pbase + (size_t)y * wf + c0 + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, h, log2h, TC, false);
        for (int i = threadIdx.x; i < TC * h; i += 256) {       // each thread rewrites the elements it reads: no barrier in between
            const int y = i / TC, c = i - y * TC;
            float2 G = make_float2(0.f, 0.f);
            if (c0 + c < wf) {
                float2 v = buf[c * h + y];
                v.x *= scale; v.y *= scale;
                const int k2 = c0 + c;
                const bool real_bin = (k2 == 0 || k2 == w_even_nyq) && (y == 0 || 2 * y == h);
                if (real_bin) v.y = 0.f;
                const float r = sqrtf(v.x * v.x + v.y * v.y);
                if (r > 0.f) {
                    const size_t g = pbase + (size_t)y * wf + k2;
                    const float ux = v.x / r, uy = v.y / r, gm = gmag[g], gq = gpha[g] / r;
                    G = make_float2(gm * ux - gq * uy, real_bin ? 0.f : gm * uy + gq * ux);
                }
            }
            buf[c * h + y] = G;
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, h, log2h, TC, true);
        for (int i = threadIdx.x; i < TC * h; i += 256) {
            const int y = i / TC, c = i - y * TC;
            if (c0 + c >= wf) continue;
            float2 v = buf[c * h + y];
            v.x *= scale; v.y *= scale;
            cout_[pbase + (size_t)y * wf + c0 + c] = v;
        }
        __syncthreads();
    }
}

// ---- adjoint of fft_rows_r2c_kernel: half spectrum [rows][wf], zero-extended to w -> inverse-direction transform -> real part, scaled
__global__ void __launch_bounds__(256) adj_rows_c2r_kernel(const float2* __restrict__ in, float* __restrict__ out, int rows, int w, int log2w,
                                                           int L, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    float2* buf = fft_lds;
    float2* tmp = fft_lds + L * w;
    const int wf = w / 2 + 1;
    for (int r0 = blockIdx.x * L; r0 < rows; r0 += gridDim.x * L) {
        const int nl = rows - r0 < L ? rows - r0 : L;
        for (int i = threadIdx.x; i < L * w; i += 256) {
            const int l = i / w, k = i - l * w;
            buf[i] = (l < nl && k < wf) ? in[(size_t)(r0 + l) * wf + k] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        lds_fft_lines(buf, tmp, w, log2w, L, true);
        for (int i = threadIdx.x; i < nl * w; i += 256) {
            const int l = i / w, k = i - l * w;
            out[(size_t)(r0 + l) * w + k] = buf[l * w + k].x * scale;
        }
        __syncthreads();
    }
}

// out = (g where lo <= v <= hi, else 0) [+ add]: torch.clamp's backward at the pre-clamp value v.  out may be g, v or add.
__global__ void __launch_bounds__(256) mask_range_kernel(const float* g, const float* v, const float* add, float* out, size_t n, float lo, float hi) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float x = v[i];
        float r = (x >= lo && x <= hi) ? g[i] : 0.f;
        if (add) r += add[i];
        out[i] = r;
    }
}

int launch_mask_range(const float* g, const float* v, const float* add, float* out, size_t n, float lo, float hi, hipStream_t st) {
    ProfScope prof(st, "mask_range_kernel", 0.0, (add ? 16.0 : 12.0) * n);
    mask_range_kernel<<<grid1d(n), 256, 0, st>>>(g, v, add, out, n, lo, hi);
    return check_launch("mask_range");
}

}  // namespace

// (mag, pha, grad_out) -> (grad_mag, grad_pha): the adjoint of launch_polar_irfft2 without residual and clamp
int launch_polar_irfft2_backward(const float* mag, const float* pha, const float* gout, float* gmag, float* gpha, float2* cscratch, int planes,
                                 int h, int w, hipStream_t st) {
    FftPlan p;
    RF_TRY(plan_fft("irfft2 backward", planes, h, w, &p));
    ProfScope prof(st, "polar_irfft2_backward(2 kernels)", 0.0, 4.0 * planes * ((double)h * w + 8.0 * h * p.wf));
    adj_rows_r2c_kernel<<<p.gx, 256, p.lds_rows, st>>>(gout, cscratch, p.rows, w, p.log2w, p.L, 1.0f / sqrtf((float)w));
    adj_cols_polar_kernel<<<p.gy, 256, p.lds_cols, st>>>(cscratch, mag, pha, gmag, gpha, planes, h, p.wf, p.log2h, p.TC, 1.0f / sqrtf((float)h));
    return check_launch("polar_irfft2_backward");
}

// (in, grad_mag, grad_pha) -> grad_in: the adjoint of launch_rfft2_polar; the spectrum of `in` is recomputed
int launch_rfft2_polar_backward(const float* in, const float* gmag, const float* gpha, float* gin, float2* cscratch, int planes, int h, int w,
                                hipStream_t st) {
    FftPlan p;
    RF_TRY(plan_fft("rfft2 backward", planes, h, w, &p));
    RF_TRY(launch_rfft_rows(in, cscratch, planes, h, w, st));
    ProfScope prof(st, "rfft2_polar_backward(2 kernels)", 0.0, 4.0 * planes * ((double)h * w + 8.0 * h * p.wf));
    adj_cols_rfft_kernel<<<p.gy, 256, p.lds_cols, st>>>(cscratch, gmag, gpha, cscratch, planes, h, p.wf, w / 2, p.log2h, p.TC, 1.0f / sqrtf((float)h));
    adj_rows_c2r_kernel<<<p.gx, 256, p.lds_rows, st>>>(cscratch, gin, p.rows, w, p.log2w, p.L, 1.0f / sqrtf((float)w));
    return check_launch("rfft2_polar_backward");
}

namespace {

// ---- one FEB
struct FebBwdBufs {
    float *xc, *y, *s, *gy;                                              // [B][nc][P]
    float *mag, *pha, *t1, *a, *m, *t2, *p, *gm, *gp, *gt, *gmag, *gpha;  // [B][nc][Pf]
    float2* cplx;
    float *wpack, *wpart;
    size_t wpart_cap;
};

void feb_bwd_plan(Bump& b, FebBwdBufs& f, int B, int nc, int h, int w, size_t wpart_cap) {
    const size_t U = (size_t)B * nc * h * w, Uf = (size_t)B * nc * h * (w / 2 + 1);
    f.xc = b.take(U); f.y = b.take(U); f.s = b.take(U); f.gy = b.take(U);
    f.mag = b.take(Uf); f.pha = b.take(Uf); f.t1 = b.take(Uf); f.a = b.take(Uf); f.m = b.take(Uf); f.t2 = b.take(Uf); f.p = b.take(Uf);
    f.gm = b.take(Uf); f.gp = b.take(Uf); f.gt = b.take(Uf); f.gmag = b.take(Uf); f.gpha = b.take(Uf);
    f.cplx = reinterpret_cast<float2*>(b.take(2 * Uf));
    f.wpack = b.take(packed1x1_floats(nc, nc));
    const size_t c1 = wgrad1x1_partial_floats(B, nc, nc, h * w, true), c2 = wgrad1x1_partial_floats(B, nc, nc, h * (w / 2 + 1), true);
    f.wpart_cap = wpart_cap > c1 ? wpart_cap : c1;
    if (f.wpart_cap < c2) f.wpart_cap = c2;
    f.wpart = b.take(f.wpart_cap);
}

// the forward with everything the backward reads kept: f.s is the sum the output clamp sees
int feb_recompute(const float* x, const float* const* p, const FebBwdBufs& f, int B, int nc, int h, int w, hipStream_t st) {
    const int P = h * w, Pf = h * (w / 2 + 1);
    RF_TRY(launch_clamp(x, f.xc, (size_t)B * nc * P, -10.f, 10.f, st));
    RF_TRY(conv1x1_raw(f.xc, f.y, p[0], p[1], nullptr, f.wpack, B, nc, nc, P, 0, st));
    RF_TRY(launch_rfft2_polar(f.y, f.mag, f.pha, f.cplx, B * nc, h, w, st));
    RF_TRY(conv1x1_raw(f.mag, f.t1, p[2], p[3], nullptr, f.wpack, B, nc, nc, Pf, 3, st));
    RF_TRY(conv1x1_raw(f.t1, f.a, p[4], p[5], nullptr, f.wpack, B, nc, nc, Pf, 0, st));
    RF_TRY(launch_clamp(f.a, f.m, (size_t)B * nc * Pf, 0.f, 1e4f, st));
    RF_TRY(conv1x1_raw(f.pha, f.t2, p[6], p[7], nullptr, f.wpack, B, nc, nc, Pf, 3, st));
    RF_TRY(conv1x1_raw(f.t2, f.p, p[8], p[9], nullptr, f.wpack, B, nc, nc, Pf, 0, st));
    return launch_polar_irfft2(f.m, f.p, f.xc, f.s, f.cplx, B * nc, h, w, INFINITY, st);
}

// after feb_recompute: gx = dL/dx (+ add), the ten parameter gradients (+)= ; g = dL/d FEB(x).  f.s is overwritten by gs.
int feb_adjoint(const float* x, const float* g, const float* add, float* gx, const float* const* p, float* const* d, const FebBwdBufs& f, int B,
                int nc, int h, int w, int acc, hipStream_t st) {
    const int P = h * w, Pf = h * (w / 2 + 1);
    const size_t U = (size_t)B * nc * P, Uf = (size_t)B * nc * Pf;
    const Wgrad wp{"ffab backward", f.wpart, f.wpart_cap, B, P, acc, st}, wf{"ffab backward", f.wpart, f.wpart_cap, B, Pf, acc, st};
    float* gs = f.s;
    RF_TRY(launch_mask_range(g, f.s, nullptr, gs, U, -10.f, 10.f, st));
    RF_TRY(launch_polar_irfft2_backward(f.m, f.p, gs, f.gm, f.gp, f.cplx, B * nc, h, w, st));
    // magnitude MLP
    RF_TRY(launch_mask_range(f.gm, f.a, nullptr, f.gm, Uf, 0.f, 1e4f, st));
    RF_TRY(wgrad1x1(wf, f.gm, nc, f.t1, nc, d[4], d[5]));
    RF_TRY(dgrad1x1(f.gm, nc, p[4], nc, f.wpack, nullptr, f.gt, B, Pf, st));
    RF_TRY(launch_ewise(f.gt, f.t1, f.gt, Uf, EW_LRELU_GRAD, 0.1f, st));               // LeakyReLU(0.1): t1 has the sign of its input
    RF_TRY(wgrad1x1(wf, f.gt, nc, f.mag, nc, d[2], d[3]));
    RF_TRY(dgrad1x1(f.gt, nc, p[2], nc, f.wpack, nullptr, f.gmag, B, Pf, st));
    // phase MLP
    RF_TRY(wgrad1x1(wf, f.gp, nc, f.t2, nc, d[8], d[9]));
    RF_TRY(dgrad1x1(f.gp, nc, p[8], nc, f.wpack, nullptr, f.gt, B, Pf, st));
    RF_TRY(launch_ewise(f.gt, f.t2, f.gt, Uf, EW_LRELU_GRAD, 0.1f, st));
    RF_TRY(wgrad1x1(wf, f.gt, nc, f.pha, nc, d[6], d[7]));
    RF_TRY(dgrad1x1(f.gt, nc, p[6], nc, f.wpack, nullptr, f.gpha, B, Pf, st));
    // rfft2 + polar, fpre, the residual and the input clamp
    RF_TRY(launch_rfft2_polar_backward(f.y, f.gmag, f.gpha, f.gy, f.cplx, B * nc, h, w, st));
    RF_TRY(wgrad1x1(wp, f.gy, nc, f.xc, nc, d[0], d[1]));
    RF_TRY(dgrad1x1(f.gy, nc, p[0], nc, f.wpack, gs, gx, B, P, st));
    return launch_mask_range(gx, x, add, gx, U, -10.f, 10.f, st);
}

// ---- one ProcessBlock: out = cat(FEB(x)) + x.  p / d: its 12 tensors
struct BlockBufs { float *feb_out, *gfeb; };

int block_recompute(const float* x, float* out, const float* const* p, const FebBwdBufs& f, const BlockBufs& k, int B, int nc, int h, int w,
                    hipStream_t st) {
    RF_TRY(feb_recompute(x, p, f, B, nc, h, w, st));
    RF_TRY(launch_clamp(f.s, k.feb_out, (size_t)B * nc * h * w, -10.f, 10.f, st));
    return out ? conv1x1_raw(k.feb_out, out, p[10], p[11], x, f.wpack, B, nc, nc, h * w, 0, st) : RF_OK;
}

int block_backward(const float* x, const float* g, float* gx, const float* const* p, float* const* d, const FebBwdBufs& f, const BlockBufs& k,
                   int B, int nc, int h, int w, int acc, hipStream_t st) {
    const int P = h * w;
    RF_TRY(block_recompute(x, nullptr, p, f, k, B, nc, h, w, st));
    RF_TRY(wgrad1x1(Wgrad{"ffab backward", f.wpart, f.wpart_cap, B, P, acc, st}, g, nc, k.feb_out, nc, d[10], d[11]));
    RF_TRY(dgrad1x1(g, nc, p[10], nc, f.wpack, nullptr, k.gfeb, B, P, st));
    return feb_adjoint(x, k.gfeb, g, gx, p, d, f, B, nc, h, w, acc, st);
}

// ---- FFAB
struct FfabBwdPlan {
    float *x0, *x, *x1, *x2, *xt;             // [B][nc][P]: conv0.0's output, the blocks' outputs x .. x2, one of x3 / x4 / x5 at a time
    float *cat[3], *pb[3];                    // [B][2 nc][P]: the inputs and outputs of the three 2 nc blocks (conv4, conv5, convout)
    float *gpb, *gcat;                        // [B][2 nc][P]
    float *gax, *gax1, *gax2, *gh, *gt, *gc;  // [B][nc][P]: the first halves of the three gcat (x, x1, x2), a second half, block results, sums
    BlockBufs k;
    FebBwdBufs f;
    size_t total;
};

int ffab_bwd_plan(const char* who, float* base, FfabBwdPlan& p, int B, int nc, int h, int w) {
    RF_TRY(ffab_check_geometry(who, B, nc, h, w));
    FftPlan fp;
    RF_TRY(plan_fft(who, B * 2 * nc, h, w, &fp));
    Bump b{base};
    const size_t U = (size_t)B * nc * h * w;
    p.x0 = b.take(U); p.x = b.take(U); p.x1 = b.take(U); p.x2 = b.take(U); p.xt = b.take(U);
    for (int i = 0; i < 3; ++i) { p.cat[i] = b.take(2 * U); p.pb[i] = b.take(2 * U); }
    p.gpb = b.take(2 * U); p.gcat = b.take(2 * U);
    p.gax = b.take(U); p.gax1 = b.take(U); p.gax2 = b.take(U); p.gh = b.take(U); p.gt = b.take(U); p.gc = b.take(U);
    p.k.feb_out = b.take(2 * U); p.k.gfeb = b.take(2 * U);
    const size_t c1 = wgrad1x1_partial_floats(B, nc, 2 * nc, h * w, true), c2 = wgrad1x1_partial_floats(B, nc, nc, h * w, true),
                 c3 = wgrad1x1_partial_floats(B, nc, nc, h * (w / 2 + 1), true);
    size_t cap = c1 > c2 ? c1 : c2;
    if (cap < c3) cap = c3;
    feb_bwd_plan(b, p.f, B, 2 * nc, h, w, cap);
    p.total = b.used;
    return RF_OK;
}

int run_ffab_backward(const FfabBwdPlan& q, const float* in, const float* g, float* gin, const float* const* prm, float* const* grd, int B, int nc,
                      int h, int w, int acc, hipStream_t st) {
    const int P = h * w;
    const size_t U = (size_t)B * nc * P, per = (size_t)nc * P;
    const FebBwdBufs& f = q.f;
    const Wgrad wg{"ffab backward", f.wpart, f.wpart_cap, B, P, acc, st};
    // state_dict order (rf_ffab.hip): conv0.0 at 0; the nc blocks conv0.1, conv1, conv2, conv3 at 2, 14, 26, 38; the 2 nc blocks and
    // their 1x1 back to nc: conv4 at 50 / 62, conv5 at 64 / 76, convout at 78 / 90
    const int tail_at[3] = {50, 64, 78};
    // forward: the inputs of the seven blocks and the outputs of the three wide ones
    RF_TRY(conv1x1_raw(in, q.x0, prm[0], prm[1], nullptr, f.wpack, B, nc, nc, P, 0, st));
    RF_TRY(block_recompute(q.x0, q.x, prm + 2, f, q.k, B, nc, h, w, st));
    RF_TRY(block_recompute(q.x, q.x1, prm + 14, f, q.k, B, nc, h, w, st));
    RF_TRY(block_recompute(q.x1, q.x2, prm + 26, f, q.k, B, nc, h, w, st));
    RF_TRY(block_recompute(q.x2, q.xt, prm + 38, f, q.k, B, nc, h, w, st));
    const float* first[3] = {q.x2, q.x1, q.x};
    for (int i = 0; i < 3; ++i) {
        const int at = tail_at[i];
        RF_TRY(launch_cat2(first[i], q.xt, q.cat[i], B, per, st));
        RF_TRY(block_recompute(q.cat[i], q.pb[i], prm + at, f, q.k, B, 2 * nc, h, w, st));
        if (i < 2) RF_TRY(conv1x1_raw(q.pb[i], q.xt, prm[at + 12], prm[at + 13], nullptr, f.wpack, B, 2 * nc, nc, P, 0, st));
    }
    // backward: convout, conv5, conv4; each leaves the first half of its concatenation's gradient for x / x1 / x2 and hands the second on
    float* const first_half[3] = {q.gax2, q.gax1, q.gax};
    const float* gtail = g;
    for (int i = 2; i >= 0; --i) {
        const int at = tail_at[i];
        RF_TRY(wgrad1x1(wg, gtail, nc, q.pb[i], 2 * nc, grd[at + 12], grd[at + 13]));
        RF_TRY(dgrad1x1(gtail, nc, prm[at + 12], 2 * nc, f.wpack, nullptr, q.gpb, B, P, st));
        RF_TRY(block_backward(q.cat[i], q.gpb, q.gcat, prm + at, grd + at, f, q.k, B, 2 * nc, h, w, acc, st));
        RF_TRY(launch_split_halves(q.gcat, first_half[i], q.gh, B, nc, P, st));
        gtail = q.gh;
    }
    // conv3 .. conv0.1: x2, x1 and x each have two consumers, summed as (concatenation half) + (next block)
    RF_TRY(block_backward(q.x2, q.gh, q.gt, prm + 38, grd + 38, f, q.k, B, nc, h, w, acc, st));
    RF_TRY(launch_ewise(q.gax2, q.gt, q.gc, U, EW_ADD, 0.f, st));
    RF_TRY(block_backward(q.x1, q.gc, q.gt, prm + 26, grd + 26, f, q.k, B, nc, h, w, acc, st));
    RF_TRY(launch_ewise(q.gax1, q.gt, q.gh, U, EW_ADD, 0.f, st));
    RF_TRY(block_backward(q.x, q.gh, q.gt, prm + 14, grd + 14, f, q.k, B, nc, h, w, acc, st));
    RF_TRY(launch_ewise(q.gax, q.gt, q.gc, U, EW_ADD, 0.f, st));
    RF_TRY(block_backward(q.x0, q.gc, q.gt, prm + 2, grd + 2, f, q.k, B, nc, h, w, acc, st));
    RF_TRY(wgrad1x1(wg, q.gt, nc, in, nc, grd[0], grd[1]));
    return dgrad1x1(q.gt, nc, prm[0], nc, f.wpack, nullptr, gin, B, P, st);
}

struct FebBwdPlan { FebBwdBufs f; size_t total; };

int feb_bwd_whole_plan(const char* who, float* base, FebBwdPlan& p, int B, int nc, int h, int w) {
    RF_TRY(ffab_check_geometry(who, B, nc, h, w));
    FftPlan fp;
    RF_TRY(plan_fft(who, B * nc, h, w, &fp));
    Bump b{base};
    feb_bwd_plan(b, p.f, B, nc, h, w, 0);
    p.total = b.used;
    return RF_OK;
}

long long fft_bwd_scratch(const char* who, int planes, int h, int w) {
    FftPlan p;
    if (planes <= 0) {
        set_error("%s: %d planes", who, planes);
        return RF_E_INVALID;
    }
    const int rc = plan_fft(who, planes, h, w, &p);
    return rc ? rc : (long long)((size_t)planes * h * p.wf * sizeof(float2));
}

}  // namespace

// floats of tensor i of the pointer arrays (state_dict order: weight, bias, weight, bias, ...)
static size_t feb_prm_floats(int i, int nc) { return i % 2 == 0 ? (size_t)nc * nc : (size_t)nc; }

size_t ffab_prm_floats(int i, int nc) {
    if (i < 50) return feb_prm_floats(i, nc);                 // conv0.0 and the four nc blocks
    const int j = (i - 50) % 14;                              // conv4 / conv5 / convout: a 2 nc block, then the 1x1 back to nc
    return j < 12 ? feb_prm_floats(j, 2 * nc) : j == 12 ? (size_t)2 * nc * nc : (size_t)nc;
}

}  // namespace rf

using namespace rf;

extern "C" {

long long rf_rfft2_polar_backward_scratch_bytes(int planes, int h, int w) { return fft_bwd_scratch("rf_rfft2_polar_backward_scratch_bytes", planes, h, w); }

int rf_rfft2_polar_backward(const float* in, const float* grad_mag, const float* grad_pha, float* grad_in, void* scratch, int planes, int h, int w,
                            void* stream) {
    const long long need = fft_bwd_scratch("rf_rfft2_polar_backward", planes, h, w);
    if (need < 0) return (int)need;
    RF_CHECK_ARG(in && grad_mag && grad_pha && grad_in && scratch && aligned16(in) && aligned16(grad_mag) && aligned16(grad_pha) &&
                     aligned16(grad_in) && aligned16(scratch),
                 "rf_rfft2_polar_backward: in, grad_mag, grad_pha, grad_in and scratch must be non-null and 16-byte aligned");
    const size_t nb = (size_t)planes * h * w * sizeof(float), nf = (size_t)planes * h * (w / 2 + 1) * sizeof(float);
    const Span outs[] = {{grad_in, nb}, {scratch, (size_t)need}}, ins[] = {{in, nb}, {grad_mag, nf}, {grad_pha, nf}};
    int a, b;
    RF_CHECK_ARG(!first_alias(outs, 2, ins, 3, &a, &b), "rf_rfft2_polar_backward: grad_in and scratch may not alias an input or each other");
    return launch_rfft2_polar_backward(in, grad_mag, grad_pha, grad_in, (float2*)scratch, planes, h, w, (hipStream_t)stream);
}

long long rf_polar_irfft2_backward_scratch_bytes(int planes, int h, int w) { return fft_bwd_scratch("rf_polar_irfft2_backward_scratch_bytes", planes, h, w); }

int rf_polar_irfft2_backward(const float* mag, const float* pha, const float* grad_out, float* grad_mag, float* grad_pha, void* scratch, int planes,
                             int h, int w, void* stream) {
    const long long need = fft_bwd_scratch("rf_polar_irfft2_backward", planes, h, w);
    if (need < 0) return (int)need;
    RF_CHECK_ARG(mag && pha && grad_out && grad_mag && grad_pha && scratch && aligned16(mag) && aligned16(pha) && aligned16(grad_out) &&
                     aligned16(grad_mag) && aligned16(grad_pha) && aligned16(scratch),
                 "rf_polar_irfft2_backward: mag, pha, grad_out, grad_mag, grad_pha and scratch must be non-null and 16-byte aligned");
    const size_t nb = (size_t)planes * h * w * sizeof(float), nf = (size_t)planes * h * (w / 2 + 1) * sizeof(float);
    const Span outs[] = {{grad_mag, nf}, {grad_pha, nf}, {scratch, (size_t)need}}, ins[] = {{mag, nf}, {pha, nf}, {grad_out, nb}};
    int a, b;
    RF_CHECK_ARG(!first_alias(outs, 3, ins, 3, &a, &b), "rf_polar_irfft2_backward: grad_mag, grad_pha and scratch may not alias an input or each other");
    return launch_polar_irfft2_backward(mag, pha, grad_out, grad_mag, grad_pha, (float2*)scratch, planes, h, w, (hipStream_t)stream);
}

long long rf_feb_backward_workspace_bytes(int B, int nc, int h, int w) {
    FebBwdPlan p;
    const int rc = feb_bwd_whole_plan("rf_feb_backward_workspace_bytes", nullptr, p, B, nc, h, w);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_feb_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                    size_t workspace_bytes, int B, int nc, int h, int w, int accumulate, void* stream) {
    FebBwdPlan p;
    RF_TRY(feb_bwd_whole_plan("rf_feb_backward", (float*)workspace, p, B, nc, h, w));
    RF_TRY(check_backward_args({"rf_feb_backward", in, grad_out, grad_in, (size_t)B * nc * h * w * sizeof(float), prm, grad_prm, 10, workspace,
                                workspace_bytes, p.total * sizeof(float)},
                               [=](int i) { return feb_prm_floats(i, nc); }));
    const hipStream_t st = (hipStream_t)stream;
    RF_TRY(feb_recompute(in, prm, p.f, B, nc, h, w, st));
    return feb_adjoint(in, grad_out, nullptr, grad_in, prm, grad_prm, p.f, B, nc, h, w, accumulate, st);
}

long long rf_ffab_backward_workspace_bytes(int B, int nc, int h, int w) {
    FfabBwdPlan p;
    const int rc = ffab_bwd_plan("rf_ffab_backward_workspace_bytes", nullptr, p, B, nc, h, w);
    return rc ? rc : (long long)(p.total * sizeof(float));
}

int rf_ffab_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                     size_t workspace_bytes, int B, int nc, int h, int w, int accumulate, void* stream) {
    FfabBwdPlan p;
    RF_TRY(ffab_bwd_plan("rf_ffab_backward", (float*)workspace, p, B, nc, h, w));
    RF_TRY(check_backward_args({"rf_ffab_backward", in, grad_out, grad_in, (size_t)B * nc * h * w * sizeof(float), prm, grad_prm, 92, workspace,
                                workspace_bytes, p.total * sizeof(float)},
                               [=](int i) { return ffab_prm_floats(i, nc); }));
    return run_ffab_backward(p, in, grad_out, grad_in, prm, grad_prm, B, nc, h, w, accumulate, (hipStream_t)stream);
}

}  // extern "C"
