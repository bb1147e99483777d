// Adjoint of the WM block of rf_mamba.hip (RawFomer_WFB_FFAB/model.py:138-172): (x, dL/dout, parameters) -> dL/dx and the 17
// parameter gradients.  With
//   a1 = relu(convb.0(x)),  r = convb.2(a1) + x,  tok = LN(rows of r) stored channel-major [n][c][L],  y = mamba(tok),  out = smooth(y)
// nothing is kept from a forward call: wm_forward_front (rf_mamba.hip) recomputes a1, convb.2(a1), tok and y; then, with g = dL/dout:
//
//   smooth    dW, db = wgrad(g, y);            g_y  = conv3x3(g, smooth^T with flipped taps)
//   Mamba     g_tok, nine gradients            run_mamba_backward (rf_mamba_bwd.hip) on (tok, g_y), channel-major
//   LN        g_r, d ln.weight, d ln.bias      wm_ln_bwd_kernel (below): the adjoint of tok_transpose_kernel<true>
//   convb.2   dW, db = wgrad(g_r, a1);         g_a1 = conv3x3(g_r, W2^T flipped) masked by a1 > 0
//   convb.0   dW, db = wgrad(g_a1, x);         dL/dx = g_r + conv3x3(g_a1, W0^T flipped)
//
// wgrad = wgrad3x3 (rf_grad.hip): launch_gram2 with nine taps where w % 4 == 0, else conv3x3_wgrad_kernel.  The three transposed, tap-flipped
// packs are written by one launch_pack_batch.  Every sum over pixels or rows goes to per-workgroup slabs that a second kernel adds
// in a fixed order: no atomics, two runs give the same bits.
#include "rf_grad.h"
#include "rf_mamba.h"

namespace rf {

// ---------------------------------------------------------------------------------------------------------------------------
// Adjoint of tok_transpose_kernel<true>.  in (+ add) [rows][cols] per image is the LayerNorm input, row i a run of cols floats;
// g [cols][rows] the gradient at the kernel's channel-major output.  Per row, with mean and rstd recomputed as the forward does,
// xh = (v - mean) rstd and dyh[k] = g[k] gamma[k]:
//   dx[k] = rstd (dyh[k] - mean_k(dyh) - xh[k] mean_k(dyh xh))
// and per column  dgamma[k] = sum_rows g xh,  dbeta[k] = sum_rows g.
// As in the forward a workgroup owns 32 rows at a time: its four waves reduce 8 rows each for mean / rstd, then g is read in
// 32 x 32 tiles that turn round in LDS (both global sides move 128-byte runs) twice: once for the two row means, once more (L2)
// for dx.  The row sums end in shuffles over the 32 lanes of a row, in a fixed order.  Thread (ty, tx) alone owns the column
// sums acc[.][ty][k = tx mod 32]; they stay in LDS over all the row groups the workgroup walks and leave as one slab per
// workgroup, summed over ty in order (launch_reduce_rows adds the slabs).
__global__ void __launch_bounds__(256) wm_ln_bwd_kernel(const float* __restrict__ in, const float* __restrict__ add, const float* __restrict__ g,
                                                        const float* __restrict__ lw, float* __restrict__ dx, float* __restrict__ dgam,
                                                        float* __restrict__ dbet, float eps, int rows, int cols) {
    __shared__ float tile[32][33];
    __shared__ float smean[32], srstd[32], sm1[32], sm2[32];
    __shared__ float acc[2][8][512];
    const size_t img = (size_t)blockIdx.y * rows * cols;
    in += img;
    add += img;
    g += img;
    dx += img;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = tx; k < cols; k += 32) {
        acc[0][ty][k] = 0.f;
        acc[1][ty][k] = 0.f;
    }
    const float inv = 1.0f / (float)cols;
    const int ngroups = (rows + 31) / 32;
    for (int rg = blockIdx.x; rg < ngroups; rg += gridDim.x) {
        const int r0 = rg * 32;
        tok_row_stats([&](size_t o) { return in[o] + add[o]; }, r0, rows, cols, eps, smean, srstd);   // the forward's mean and rstd
        __syncthreads();
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < cols; c0 += 32) {                // pass 1: row means of dyh and dyh xh, column sums
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = ty + 8 * i, k = c0 + kk, r = r0 + tx;
                tile[kk][tx] = (k < cols && r < rows) ? g[(size_t)k * rows + r] : 0.f;
            }
            __syncthreads();
            const int k = c0 + tx;
            if (k < cols) {
                const float gam = lw[k];
                float cg = 0.f, cb = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = ty + 8 * i, r = r0 + rr;
                    if (r < rows) {
                        const size_t o = (size_t)r * cols + k;
                        const float xh = (in[o] + add[o] - smean[rr]) * srstd[rr], gt = tile[tx][rr], dy = gt * gam;
                        s1[i] += dy;
                        s2[i] = fmaf(dy, xh, s2[i]);
                        cg = fmaf(gt, xh, cg);
                        cb += gt;
                    }
                }
                acc[0][ty][k] += cg;
                acc[1][ty][k] += cb;
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int m = 16; m > 0; m >>= 1) {
                s1[i] += __shfl_xor(s1[i], m, 64);
                s2[i] += __shfl_xor(s2[i], m, 64);
            }
            if (tx == 0) {
                sm1[ty + 8 * i] = s1[i] * inv;
                sm2[ty + 8 * i] = s2[i] * inv;
            }
        }
        __syncthreads();
        for (int c0 = 0; c0 < cols; c0 += 32) {                // pass 2: dx
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = ty + 8 * i, k = c0 + kk, r = r0 + tx;
                tile[kk][tx] = (k < cols && r < rows) ? g[(size_t)k * rows + r] : 0.f;
            }
            __syncthreads();
            const int k = c0 + tx;
            if (k < cols) {
                const float gam = lw[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = ty + 8 * i, r = r0 + rr;
                    if (r < rows) {
                        const size_t o = (size_t)r * cols + k;
                        const float xh = (in[o] + add[o] - smean[rr]) * srstd[rr], dy = tile[tx][rr] * gam;
                        dx[o] = srstd[rr] * (dy - sm1[rr] - xh * sm2[rr]);
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const size_t slab = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * cols;
    for (int k = threadIdx.x; k < cols; k += 256) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            a += acc[0][t][k];
            b += acc[1][t][k];
        }
        dgam[slab + k] = a;
        dbet[slab + k] = b;
    }
}

// workgroups per image: one per 32 rows up to about 2048 in all (a workgroup walks the row groups it owns in order)
static int wm_ln_bwd_nblk(int B, int rows) {
    const int ng = cdiv(rows, 32), cap = cdiv(2048, B);
    return ng < cap ? ng : cap;
}

// partial: 2 B nblk cols floats
static int launch_wm_ln_bwd(const float* in, const float* add, const float* g, const float* lw, float* dx, float* dlw, float* dlb, float* partial,
                            int B, int rows, int cols, int accumulate, hipStream_t st) {
    const int nblk = wm_ln_bwd_nblk(B, rows);
    float *dgam = partial, *dbet = partial + (size_t)B * nblk * cols;
    {
        const double el = (double)B * rows * cols;
        ProfScope prof(st, "wm_ln_bwd_kernel", 20.0 * el, 12.0 * el);
        wm_ln_bwd_kernel<<<dim3((unsigned)nblk, (unsigned)B), 256, 0, st>>>(in, add, g, lw, dx, dgam, dbet, 1e-5f, rows, cols);
        RF_TRY(check_launch("wm_ln_bwd"));
    }
    RF_TRY(reduce_rows(dgam, dlw, B * nblk, (size_t)cols, accumulate, st));
    return reduce_rows(dbet, dlb, B * nblk, (size_t)cols, accumulate, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
struct WmBwdPlan {
    MambaBwdPlan mb;                      // its u, g and gu buffers hold tok, g_y and g_tok
    size_t w0, w2;                        // packed convb.0 / convb.2 (forward)
    size_t t0, t2, ts;                    // transposed, tap-flipped packs of convb.0, convb.2, smooth
    size_t a1, r, y, ga1;                 // [n][2c][P], [n][c][P] (convb.2's output without the skip), [n][c][P] (y, then g_r), [n][2c][P]
    size_t lnp, wpart, wpart_cap;         // LayerNorm slabs; weight-gradient partials and their capacity
    size_t ks, ks_floats;                 // scratch of the 3x3 convolutions' input-channel split (small launches only, else 0 floats)
};

static int wm_bwd_plan(const char* who, int n, int c, int h, int w, WmBwdPlan* p, Bump* b) {
    RF_TRY(wm_check_shape(who, n, c, h, w));
    RF_TRY(mamba_bwd_plan(who, n, h * w, c, kN, kDc, 2, &p->mb, b));
    const size_t plane = (size_t)n * h * w;
    p->w0 = b->off(packed3x3_floats(c, 2 * c));
    p->w2 = b->off(packed3x3_floats(2 * c, c));
    p->t0 = b->off(packed3x3_floats(2 * c, c));
    p->t2 = b->off(packed3x3_floats(c, 2 * c));
    p->ts = b->off(packed3x3_floats(c, c));
    p->a1 = b->off(plane * 2 * c);
    p->r = b->off(plane * c);
    p->y = b->off(plane * c);
    p->ga1 = b->off(plane * 2 * c);
    p->lnp = b->off((size_t)2 * n * wm_ln_bwd_nblk(n, h * w) * c);
    size_t cap = 0;                                                       // convb.0, convb.2, smooth
    for (const size_t f : {wgrad3x3_partial_floats(n, 2 * c, c, h, w), wgrad3x3_partial_floats(n, c, 2 * c, h, w), wgrad3x3_partial_floats(n, c, c, h, w)})
        cap = cap > f ? cap : f;
    p->wpart_cap = cap;
    p->wpart = b->off(cap);
    p->ks_floats = conv3x3_ksplit_floats(n, 2 * c, h, w);                // the widest output of the five convolutions
    p->ks = b->off(p->ks_floats);
    return RF_OK;
}

// floats of tensor i of the 17 of the pointer arrays, in ops.wm_param_shapes' order
size_t wm_prm_floats(int i, int c) {
    if (i >= 6 && i < 15) return mamba_prm_floats(i - 6, c, kN, kDc, 2);                           // model1
    const size_t C = c, floats[6] = {2 * C * C * 9, 2 * C, C * 2 * C * 9, C, C, C};                // convb.0, convb.2, ln
    return i < 6 ? floats[i] : i == 15 ? C * C * 9 : C;                                            // smooth
}

static int wm_dgrad3x3(const float* dy, const float* wp, float* dx, float* ks, size_t ks_floats, int n, int cout, int cin, int h, int w,
                       hipStream_t st) {
    Conv3x3Args a = conv3x3_dense(dy, wp, nullptr, dx, n, cout, cin, h, w, 0);
    a.ks_scratch = ks; a.ks_floats = ks_floats;
    return launch_conv3x3(a, st);
}

static int run_wm_backward(const WmBwdPlan& p, const float* x, const float* g, float* dx, const float* const* prm, float* const* grd, float* ws,
                           int n, int c, int h, int w, int acc, hipStream_t st) {
    const int L = h * w;
    const size_t el = (size_t)n * c * L;
    float *a1 = ws + p.a1, *r = ws + p.r, *y = ws + p.y, *ga1 = ws + p.ga1, *tok = ws + p.mb.u, *gy = ws + p.mb.g, *gtok = ws + p.mb.gu;
    const Wgrad wg{"rf_wm_backward", ws + p.wpart, p.wpart_cap, n, L, acc, st};
    float* gr = y;                                                          // y is dead once smooth's weight gradient is taken
    // dX weights of a 3x3 convolution [Cout][Cin][3][3]: rows and columns exchanged, taps flipped
    const PackDesc packs[3] = {{prm[0], ws + p.t0, 1, c, 2 * c, 9, (int64_t)c * 9, 1},
                               {prm[2], ws + p.t2, 1, 2 * c, c, 9, (int64_t)2 * c * 9, 1},
                               {prm[15], ws + p.ts, 1, c, c, 9, (int64_t)c * 9, 1}};
    RF_TRY(launch_pack_batch(packs, 3, st));
    // Launches of at most 64 workgroups (single frames of the deep levels) split their input channels over up to eight workgroups:
    // a chain of 64 chunk barriers becomes eight of 8, and the accumulation runs over an eighth of the 9 Cin products before the
    // partial tiles are added in split order, which also shortens the rounding chain ("WM backward").  Deterministic.
    float* ks = p.ks_floats ? ws + p.ks : nullptr;
    if (ks) RF_TRY(check_hip(hipMemsetAsync(ks, 0, conv3x3_ksplit_counter_bytes(), st), "rf_wm_backward: memset"));
    WmFrontBufs fb{ws + p.w0, ws + p.w2, a1, r, tok, y};
    fb.ks = ks; fb.ks_floats = p.ks_floats;
    RF_TRY(wm_forward_front(p.mb.m, x, prm, nullptr, ws, fb, n, c, h, w, st));
    // smooth
    RF_TRY(wgrad3x3(wg, g, c, y, c, grd[15], grd[16], w));
    RF_TRY(wm_dgrad3x3(g, ws + p.ts, gy, ks, p.ks_floats, n, c, c, h, w, st));
    // Mamba, channel-major
    RF_TRY(run_mamba_backward(p.mb, tok, gy, gtok, prm + 6, grd + 6, ws, n, L, acc, st));
    // LayerNorm over the runs of c floats + the transposition
    RF_TRY(launch_wm_ln_bwd(r, x, gtok, prm[4], gr, grd[4], grd[5], ws + p.lnp, n, L, c, acc, st));
    // convb.2
    RF_TRY(wgrad3x3(wg, gr, c, a1, 2 * c, grd[2], grd[3], w));
    RF_TRY(wm_dgrad3x3(gr, ws + p.t2, ga1, ks, p.ks_floats, n, c, 2 * c, h, w, st));
    RF_TRY(launch_ewise(ga1, a1, ga1, 2 * el, EW_LRELU_GRAD, 0.f, st));                 // ReLU: g_a1 where a1 > 0, else 0
    // convb.0 and the skip
    RF_TRY(wgrad3x3(wg, ga1, 2 * c, x, c, grd[0], grd[1], w));
    RF_TRY(wm_dgrad3x3(ga1, ws + p.t0, dx, ks, p.ks_floats, n, 2 * c, c, h, w, st));
    return launch_ewise(dx, gr, dx, el, EW_ADD, 0.f, st);
}

}  // namespace rf

using namespace rf;

extern "C" {

long long rf_wm_backward_workspace_bytes(int n, int c, int h, int w) {
    WmBwdPlan p;
    Bump b;
    const int rc = wm_bwd_plan("rf_wm_backward_workspace_bytes", n, c, h, w, &p, &b);
    return rc ? rc : (long long)(b.used * sizeof(float));
}

int rf_wm_backward(const float* in, const float* grad_out, float* grad_in, const float* const* prm, float* const* grad_prm, void* workspace,
                   size_t workspace_bytes, int n, int c, int h, int w, int accumulate, void* stream) {
    WmBwdPlan p;
    Bump b;
    RF_TRY(wm_bwd_plan("rf_wm_backward", n, c, h, w, &p, &b));
    RF_TRY(check_backward_args({"rf_wm_backward", in, grad_out, grad_in, (size_t)n * c * h * w * sizeof(float), prm, grad_prm, 17, workspace,
                                workspace_bytes, b.used * sizeof(float)},
                               [=](int i) { return wm_prm_floats(i, c); }));
    RF_CHECK_ARG(in != grad_out, "rf_wm_backward: in, grad_out and grad_in may not alias each other");
    return run_wm_backward(p, in, grad_out, grad_in, prm, grad_prm, (float*)workspace, n, c, h, w, accumulate, (hipStream_t)stream);
}

}  // extern "C"
