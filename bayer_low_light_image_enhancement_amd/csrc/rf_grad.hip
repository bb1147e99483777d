// The gradient pieces of rf_grad.h.
#include <vector>
#include "rf_grad.h"

namespace rf {

namespace {

// Weight (and, BIAS, bias) gradient of a 1x1 convolution for planes launch_gram2 does not take (P % 4 != 0: rows that are not
// 16-byte aligned): partial[(image, slab)][i][j] = sum over the slab's pixels of a[i][t] b[j][t], bias_partial[(image, slab)][i] =
// sum of a[i][t]; a workgroup owns a 16 x 16 tile of (i, j) and adds its pixels in order.  The instance without the bias sum has
// an empty last argument: it does no work for it and finds its other (and the launch's hidden) arguments where they lie without one.
template <bool BIAS> struct BiasPartial { float* p; };
template <> struct BiasPartial<false> {};

template <bool BIAS>
__global__ void __launch_bounds__(256) wgrad1x1_kernel(const float* __restrict__ a, int64_t a_bstride, int Ca, const float* __restrict__ b,
                                                       int64_t b_bstride, int Cb, float* __restrict__ partial, int P, int slab_len, int ntj,
                                                       BiasPartial<BIAS> bias_partial) {
    __shared__ float sa[16][65], sb[16][65];
    const int i0 = ((int)blockIdx.x / ntj) * 16, j0 = ((int)blockIdx.x % ntj) * 16, ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    const float* ag = a + (size_t)blockIdx.z * a_bstride;
    const float* bg = b + (size_t)blockIdx.z * b_bstride;
    const int lo = blockIdx.y * slab_len, hi = min(P, lo + slab_len);
    float acc = 0.f, accb = 0.f;
    for (int t0 = lo; t0 < hi; t0 += 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = threadIdx.x + 256 * q, r = idx >> 6, c = idx & 63;
            const bool ok = t0 + c < hi;
            sa[r][c] = (ok && i0 + r < Ca) ? ag[(size_t)(i0 + r) * P + t0 + c] : 0.f;
            sb[r][c] = (ok && j0 + r < Cb) ? bg[(size_t)(j0 + r) * P + t0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 16
        for (int c = 0; c < 64; ++c) {
            acc = fmaf(sa[ti][c], sb[tj][c], acc);
            if constexpr (BIAS) accb += sa[ti][c];
        }
        __syncthreads();
    }
    if (i0 + ti < Ca && j0 + tj < Cb)
        partial[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * Ca + i0 + ti) * Cb + j0 + tj] = acc;
    if constexpr (BIAS)
        if (j0 == 0 && tj == 0 && i0 + ti < Ca) bias_partial.p[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * Ca + i0 + ti] = accb;
}

// 3x3 weight and bias gradient for the widths launch_gram2 does not take (w % 4 != 0: the small bands of the deep levels):
//   dW[co][ci][dy][dx] = sum over images and pixels of a[co][y][x] b[ci][y + dy - 1][x + dx - 1],   db[co] = sum of a[co]
// A thread owns one (ci, tap) of one output channel and one slab of `slab_px` consecutive pixels of the batch (images laid end
// to end) and adds them in order; every thread of the workgroup reads the same a value (one broadcast load).  The partials have
// the layout of the result, [slab][Ca][Cb][9] and [slab][Ca].
__global__ void __launch_bounds__(256) conv3x3_wgrad_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ partial,
                                                            float* __restrict__ bias_partial, int Ca, int Cb, int h, int w, long long total,
                                                            long long slab_px) {
    const int co = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= Cb * 9) return;
    const int ci = e / 9, tap = e - 9 * ci, sy = tap / 3 - 1, sx = tap % 3 - 1;
    const int P = h * w;
    const long long q0 = (long long)blockIdx.z * slab_px, q1 = q0 + slab_px < total ? q0 + slab_px : total;
    long long img = q0 / P;
    int p = (int)(q0 - img * P);
    float s = 0.f, sb = 0.f;
    for (long long q = q0; q < q1; ++q) {
        const float av = a[((size_t)img * Ca + co) * P + p];
        const int y = p / w, x = p - y * w, yy = y + sy, xx = x + sx;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) s = fmaf(av, b[((size_t)img * Cb + ci) * P + yy * w + xx], s);
        sb += av;
        if (++p == P) {
            p = 0;
            ++img;
        }
    }
    partial[((size_t)blockIdx.z * Ca + co) * Cb * 9 + e] = s;
    if (e == 0) bias_partial[(size_t)blockIdx.z * Ca + co] = sb;
}

// slabs per image of wgrad1x1_kernel and their length: a multiple of 64 pixels, at least 1024, at most 16 slabs
int wgrad1x1_slabs(int P, int* slab_len) {
    int len = cdiv(cdiv(P, 16), 64) * 64;
    if (len < 1024) len = 1024;
    *slab_len = len;
    return cdiv(P, len);
}

int wgrad3x3_slabs(int B, int P, long long* slab_px) {
    const long long total = (long long)B * P;
    long long px = (total + 32767) / 32768;
    if (px < 4096) px = 4096;
    *slab_px = px;
    return (int)((total + px - 1) / px);
}

}  // namespace

Gram2Launch gram2_of(const Wgrad& q, const float* a, int64_t a_bstride, int Ca, const float* b, int64_t b_bstride, int Cb, float* dW, int ld,
                     float* db, int w, int ntap) {
    Gram2Launch g{};
    g.a = a; g.a_bstride = a_bstride; g.Ca = Ca; g.b = b; g.b_bstride = b_bstride; g.Cb = Cb;
    g.out = dW; g.ld = ld; g.partial = q.partial; g.partial_cap = q.cap; g.B = q.B; g.h = q.P / w; g.w = w; g.ntap = ntap;
    g.accumulate = q.acc != 0; g.db = db;
    return g;
}

int reduce_rows(const float* partial, float* out, int nrows, size_t n, int accumulate, hipStream_t st) {
    ProfScope prof(st, "reduce_partials_kernel", (double)nrows * n, 4.0 * (nrows + 1.0) * n);
    return launch_reduce_rows(partial, out, nrows, n, accumulate, st);
}

size_t wgrad1x1_partial_floats(int B, int Ca, int Cb, int P, bool with_bias) {
    if (P % 4 == 0) return gram2_partial_floats(B, Ca, Cb, 1, P, 1);
    int len;
    return (size_t)B * wgrad1x1_slabs(P, &len) * ((size_t)Ca * Cb + (with_bias ? Ca : 0));
}

int wgrad1x1(const Wgrad& q, const float* a, int64_t a_bstride, int Ca, const float* b, int64_t b_bstride, int Cb, float* dW, float* db) {
    const int B = q.B, P = q.P;
    if (P % 4 == 0) {
        return launch_gram2(gram2_of(q, a, a_bstride, Ca, b, b_bstride, Cb, dW, Cb, db, P, 1), q.st);
    }
    int len;
    const int nslab = wgrad1x1_slabs(P, &len), ntj = cdiv(Cb, 16);
    const size_t n = (size_t)Ca * Cb;
    RF_CHECK_ARG((size_t)B * nslab * (n + (db ? Ca : 0)) <= q.cap, "%s: the weight-gradient partials exceed their buffer", q.who);
    float* bias_partial = db ? q.partial + (size_t)B * nslab * n : nullptr;
    {
        ProfScope prof(q.st, "wgrad1x1_kernel", 2.0 * Ca * Cb * (double)B * P, 4.0 * (double)B * P * (Ca + Cb));
        const dim3 grid((unsigned)(cdiv(Ca, 16) * ntj), (unsigned)nslab, (unsigned)B);
        if (db) wgrad1x1_kernel<true><<<grid, 256, 0, q.st>>>(a, a_bstride, Ca, b, b_bstride, Cb, q.partial, P, len, ntj, {bias_partial});
        else wgrad1x1_kernel<false><<<grid, 256, 0, q.st>>>(a, a_bstride, Ca, b, b_bstride, Cb, q.partial, P, len, ntj, {});
        RF_TRY(check_launch("wgrad1x1"));
    }
    RF_TRY(reduce_rows(q.partial, dW, B * nslab, n, q.acc, q.st));
    return db ? reduce_rows(bias_partial, db, B * nslab, (size_t)Ca, q.acc, q.st) : RF_OK;
}

size_t wgrad3x3_partial_floats(int B, int Ca, int Cb, int h, int w) {
    if (w % 4 == 0) return gram2_partial_floats(B, Ca, Cb, h, w, 9);
    long long px;
    return (size_t)wgrad3x3_slabs(B, h * w, &px) * ((size_t)9 * Ca * Cb + Ca);
}

int wgrad3x3(const Wgrad& q, const float* a, int Ca, const float* b, int Cb, float* dW, float* db, int w) {
    const int B = q.B, P = q.P, h = P / w;
    if (w % 4 == 0) {
        return launch_gram2(gram2_of(q, a, (int64_t)Ca * P, Ca, b, (int64_t)Cb * P, Cb, dW, Cb, db, w, 9), q.st);
    }
    long long px;
    const int nslab = wgrad3x3_slabs(B, P, &px);
    const size_t n = (size_t)9 * Ca * Cb;
    RF_CHECK_ARG((size_t)nslab * (n + Ca) <= q.cap, "%s: the weight-gradient partials exceed their buffer", q.who);
    float* bias_partial = q.partial + (size_t)nslab * n;
    {
        const double px_all = (double)B * P;
        ProfScope prof(q.st, "conv3x3_wgrad_kernel", 18.0 * Ca * Cb * px_all, 4.0 * px_all * (Ca + Cb));
        conv3x3_wgrad_kernel<<<dim3((unsigned)Ca, (unsigned)cdiv(Cb * 9, 256), (unsigned)nslab), 256, 0, q.st>>>(a, b, q.partial, bias_partial, Ca, Cb,
                                                                                                                 h, w, (long long)B * P, px);
        RF_TRY(check_launch("conv3x3_wgrad"));
    }
    RF_TRY(reduce_rows(q.partial, dW, nslab, n, q.acc, q.st));
    return reduce_rows(bias_partial, db, nslab, (size_t)Ca, q.acc, q.st);
}

int dgrad1x1(const Dgrad1x1& d, hipStream_t st) {
    RF_TRY(pack_1x1(d.w, d.wp, d.Cout, d.K, 1, d.Cout, st));
    if (d.wp3) RF_TRY(pack_1x1_b3(d.w, d.wp3, d.Cout, d.K, 1, d.Cout, st));
    Conv1x1Args a{};
    a.x1 = d.x; a.C1 = d.Kp; a.x1_bstride = d.x_bstride; a.wp = d.wp; a.wp3 = d.wp3;
    a.res = d.res; a.res_bstride = (int64_t)d.Cout * d.P;
    a.out = d.out; a.out_bstride = d.out_bstride; a.Cout = d.Cout; a.B = d.B; a.P = d.P; a.w = d.P;
    return launch_conv1x1(a, st);
}

bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}

int first_alias(const Span* outs, int nout, const Span* ins, int nin, int* a, int* b) {
    for (*a = 0; *a < nout; ++*a) {
        const Span& o = outs[*a];
        for (*b = 0; *b < nin; ++*b)
            if (overlaps(o.p, o.bytes, ins[*b].p, ins[*b].bytes)) return 1;
        for (*b = *a + 1; *b < nout; ++*b)
            if (overlaps(o.p, o.bytes, outs[*b].p, outs[*b].bytes)) return 2;
    }
    return 0;
}

int check_backward_args(const BackwardArgs& c, const std::function<size_t(int)>& prm_floats) {
    const int n = c.n;
    RF_CHECK_ARG(c.in && c.grad_out && c.grad_in && c.prm && c.grad_prm && c.workspace && aligned16(c.in) && aligned16(c.grad_out) &&
                     aligned16(c.grad_in) && aligned16(c.workspace),
                 "%s: in, grad_out, grad_in, prm, grad_prm and workspace must be non-null and 16-byte aligned", c.who);
    if (c.workspace_bytes < c.need_bytes) {
        set_error("%s: workspace of %zu bytes, %zu needed", c.who, c.workspace_bytes, c.need_bytes);
        return RF_E_NOMEM;
    }
    for (int i = 0; i < n; ++i) RF_CHECK_ARG(c.prm[i] != nullptr && c.grad_prm[i] != nullptr, "%s: parameter or gradient %d is null", c.who, i);
    for (int i = 0; i < c.nbuffers; ++i) RF_CHECK_ARG(c.buffers[i].p != nullptr, "%s: buffer %d is null", c.who, i);
    std::vector<Span> outs(n + 2), ins(n + 2);              // tensors 0 .. n - 1, then grad_in | in, then the workspace | grad_out
    ins.insert(ins.end(), c.buffers, c.buffers + c.nbuffers);      // ... and the read-only buffers behind the inputs
    for (int i = 0; i < n; ++i) {
        const size_t bytes = prm_floats(i) * sizeof(float);
        outs[i] = {c.grad_prm[i], bytes};
        ins[i] = {c.prm[i], bytes};
    }
    outs[n] = {c.grad_in, c.plane_bytes};
    outs[n + 1] = {c.workspace, c.need_bytes};
    ins[n] = {c.in, c.plane_bytes};
    ins[n + 1] = {c.grad_out, c.plane_bytes};
    int a, b;
    const int hit = first_alias(outs.data(), n + 2, ins.data(), n + 2 + c.nbuffers, &a, &b);
    RF_CHECK_ARG(hit != 1 || b < n + 2, "%s: an output (gradient %d; %d = grad_in, %d = workspace) may not alias read-only buffer %d", c.who, a, n, n + 1,
                 b - n - 2);
    RF_CHECK_ARG(hit != 1, "%s: an output (gradient %d; %d = grad_in, %d = workspace) may not alias an input (parameter %d; %d = in, %d = grad_out)",
                 c.who, a, n, n + 1, b, n, n + 1);
    RF_CHECK_ARG(hit != 2, "%s: outputs may not alias each other (gradients %d and %d; %d = grad_in, %d = workspace)", c.who, a, b, n, n + 1);
    return RF_OK;
}

}  // namespace rf
