// Mamba selective scan and the WM block of the WFB variant (RawFomer_WFB_FFAB/model.py:138-172), inference only.
//
//   Mamba(d_model = D, d_state = 32, d_conv = 4, expand = E), Di = E D, R = ceil(D / 16), on u [B, L, D]:
//     [x ; z] = in_proj(u);  x = silu(conv1d(x));  [dt ; Bm ; Cm] = x_proj(x);  delta = softplus(dt_proj(dt) + bias)
//     h_t = exp(delta_t A) h_{t-1} + delta_t Bm_t x_t;  y_t = Cm_t . h_t + D x_t;  out = out_proj(y silu(z))
//
// Layout: every intermediate is channel-major, [image][channel][L] with L contiguous -- the layout of launch_conv1x1, so
// in_proj, x_proj and out_proj are calls of that launcher with P = L, and out_proj's result already is the
// permute(0,2,1).reshape(n,c,h,w) tensor WM's `smooth` convolution reads.  Token-major tensors ([B, L, D], and WM's raw
// reshape of NCHW memory into runs of c floats) pass through tok_transpose_kernel once, which also carries WM's LayerNorm.
//
// The scan is a recurrence over up to 65 536 tokens; it is cut into chunks of kLc tokens.  The decay of a whole chunk is
// exp(A[d,n] sum_{t in chunk} delta_t[d]), so a chunk is summarised by its end state from a ZERO start and one sum per channel:
//   phase 1  mamba_scan_kernel<false>   every chunk but the last, in parallel: local end state E_c[d,n] and S_c[d]
//   phase 2  mamba_carry_kernel         one thread per (d, n) walks the chunks in order:  H = exp(A S_c) H + E_c;  E_c <- H
//   phase 3  mamba_scan_kernel<true>    every chunk again from its incoming state E_{c-1}; emits (C . h + D x) silu(z)
// A lane owns one channel d and keeps h[32] and A[32] (times log2 e) in registers: Bm_t / Cm_t are wave-uniform (LDS
// broadcast reads) and the sum over n is a chain of FMAs in the lane, no cross-lane step.  A wave handles 64 channels of one
// chunk; delta, x, z tiles of 64 channels x kT tokens go through LDS so that global accesses run along L.  No atomics, fixed
// summation orders: two runs give the same bits.
#include "rf_mamba.h"

namespace rf {

// ---------------------------------------------------------------------------------------------------------------------------
// in [rows][cols] (+ add, same layout) -> out [cols][rows] per image, with an optional LayerNorm along cols (cols <= 512).
// Token-major -> channel-major: rows = L, cols = channels; the way back: rows = channels, cols = L, no LayerNorm.
// A workgroup owns 32 rows: its four waves first reduce 8 rows each (two passes over values held in registers), then the
// rows are read again (L2) in 32 x 32 tiles that turn round in LDS; both global sides move 128-byte runs.
template <bool LN>
__global__ void __launch_bounds__(256) tok_transpose_kernel(const float* __restrict__ in, const float* __restrict__ add,
                                                            float* __restrict__ out, const float* __restrict__ lw,
                                                            const float* __restrict__ lb, float eps, int rows, int cols) {
    __shared__ float tile[32][33];
    __shared__ float smean[32], srstd[32];
    const size_t img = (size_t)blockIdx.y * rows * cols;
    in += img;
    out += img;
    if (add) add += img;
    const int r0 = blockIdx.x * 32;
    if constexpr (LN) {
        tok_row_stats([&](size_t o) { return add ? in[o] + add[o] : in[o]; }, r0, rows, cols, eps, smean, srstd);
        __syncthreads();
    }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int c0 = 0; c0 < cols; c0 += 32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = ty + 8 * i, r = r0 + rr, k = c0 + tx;
            float v = 0.f;
            if (r < rows && k < cols) {
                const size_t o = (size_t)r * cols + k;
                v = add ? in[o] + add[o] : in[o];
                if constexpr (LN) v = (v - smean[rr]) * srstd[rr] * lw[k] + lb[k];
            }
            tile[rr][tx] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = ty + 8 * i, k = c0 + kk, r = r0 + tx;
            if (k < cols && r < rows) out[(size_t)k * rows + r] = tile[tx][kk];
        }
        __syncthreads();
    }
}

// causal depthwise conv1d along L + bias + SiLU on the x half of in_proj's output [B][2 Di][L] -> xc [B][Di][L].
// Tap k of token t reads token t - 3 + k of the SAME row; a tap before token 0 is the zero padding and is never loaded, so
// no lane reaches into the previous channel row or image.
__global__ void __launch_bounds__(256) mamba_conv_kernel(const float* __restrict__ xz, float* __restrict__ xc, const float* __restrict__ w,
                                                         const float* __restrict__ b, int Di, int L, size_t total) {
    for (size_t idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int t = (int)(idx % (size_t)L);
        const size_t row = idx / (size_t)L;
        const int d = (int)(row % (size_t)Di);
        const size_t img = row / (size_t)Di;
        const float* xr = xz + (img * 2 * Di + d) * (size_t)L;
        float acc = b[d];
#pragma unroll
        for (int k = 0; k < kDc; ++k) {
            const int tt = t - (kDc - 1) + k;
            if (tt >= 0) acc = fmaf(w[d * kDc + k], xr[tt], acc);
        }
        xc[idx] = acc / (1.0f + expf(-acc));
    }
}

// delta[d][t] = softplus(dt_proj.weight[d][:] . dt[:][t] + dt_proj.bias[d]) with dt = rows 0..R-1 of x_proj's output
// [B][R + 2N][L]; a thread owns 4 channels of one token (the dt values are loaded once for the four).
__global__ void __launch_bounds__(256) mamba_delta_kernel(const float* __restrict__ dbc, float* __restrict__ delta, const float* __restrict__ wdt,
                                                          const float* __restrict__ bdt, int Di, int R, int NR, int L) {
    const int t = blockIdx.x * 256 + threadIdx.x, d0 = blockIdx.y * 4;
    if (t >= L) return;
    const float* dr = dbc + (size_t)blockIdx.z * NR * L + t;
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bdt[d0 + j];
    for (int r = 0; r < R; ++r) {
        const float v = dr[(size_t)r * L];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(wdt[(d0 + j) * R + r], v, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        delta[((size_t)blockIdx.z * Di + d0 + j) * L + t] = acc[j] > 20.0f ? acc[j] : log1pf(expf(acc[j]));   // torch softplus
}

// The kernels take this struct by value.  y may be the delta buffer itself: a wave reads a tile of delta before it writes the
// same tile of y, and no other wave touches that tile.
struct ScanArgs {
    const float* delta;    // [B][Di][L]
    const float* x;        // [B][Di][L]   conv + SiLU output
    const float* z;        // z half of in_proj's output; z_bstride floats between images
    int64_t z_bstride;
    const float* bm;       // row R of x_proj's output [B][NR][L]; Cm = row R + 32
    int64_t bc_bstride;
    const float* A_log;    // [Di][32]
    const float* Dp;       // [Di]
    float* y;              // [B][Di][L]
    float* state;          // [B][nchunk - 1][Di][32]
    float* sdelta;         // [B][nchunk - 1][Di]
    int Di, L, nchunk;
};

template <bool EMIT>
__global__ void __launch_bounds__(64) mamba_scan_kernel(ScanArgs a) {
    __shared__ float sd[64][kT + 1], sx[64][kT + 1], sz[EMIT ? 64 : 1][kT + 1];
    __shared__ __attribute__((aligned(16))) float sB[kT][kBrow];
    __shared__ __attribute__((aligned(16))) float sC[EMIT ? kT : 1][kBrow];
    const int lane = threadIdx.x, chunk = blockIdx.x, d0 = blockIdx.y * 64, d = d0 + lane;
    const size_t img = blockIdx.z;
    const int Di = a.Di, L = a.L, ns = a.nchunk - 1;
    const bool live = d < Di;
    float A2[kN], h[kN];
#pragma unroll
    for (int q = 0; q < kN / 4; ++q) {
        float4 al = make_float4(0.f, 0.f, 0.f, 0.f), hv = al;
        if (live) {
            al = *reinterpret_cast<const float4*>(a.A_log + (size_t)d * kN + 4 * q);
            al = make_float4(-expf(al.x) * kLog2e, -expf(al.y) * kLog2e, -expf(al.z) * kLog2e, -expf(al.w) * kLog2e);
            if (EMIT && chunk > 0) hv = *reinterpret_cast<const float4*>(a.state + ((img * ns + chunk - 1) * Di + d) * kN + 4 * q);
        }
        A2[4 * q] = al.x; A2[4 * q + 1] = al.y; A2[4 * q + 2] = al.z; A2[4 * q + 3] = al.w;
        h[4 * q] = hv.x; h[4 * q + 1] = hv.y; h[4 * q + 2] = hv.z; h[4 * q + 3] = hv.w;
    }
    const float Dp = (EMIT && live) ? a.Dp[d] : 0.f;
    const float* dg = a.delta + img * Di * (size_t)L;
    const float* xg = a.x + img * Di * (size_t)L;
    const float* zg = a.z + img * a.z_bstride;
    const float* bg = a.bm + img * a.bc_bstride;
    const float* cg = bg + (size_t)kN * L;
    float* yg = a.y + img * Di * (size_t)L;
    const int t_end = min(L, (chunk + 1) * kLc);
    float sdl = 0.f;
    for (int t0 = chunk * kLc; t0 < t_end; t0 += kT) {
#pragma unroll
        for (int k = 0; k < kT; ++k) {                       // 64 channels x kT tokens: kT consecutive lanes per channel row
            const int idx = lane + 64 * k, r = idx / kT, j = idx % kT;
            const bool ok = d0 + r < Di && t0 + j < t_end;
            const size_t o = (size_t)(d0 + r) * L + t0 + j;
            sd[r][j] = ok ? dg[o] : 0.f;
            sx[r][j] = ok ? xg[o] : 0.f;
            if constexpr (EMIT) sz[r][j] = ok ? zg[o] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kT * kN / 64; ++k) {             // 32 state rows x kT tokens, stored token-major for the broadcast reads
            const int idx = lane + 64 * k, n = idx / kT, j = idx % kT;
            const bool ok = t0 + j < t_end;
            const size_t o = (size_t)n * L + t0 + j;
            sB[j][n] = ok ? bg[o] : 0.f;
            if constexpr (EMIT) sC[j][n] = ok ? cg[o] : 0.f;
        }
        __syncthreads();
        const int nt = min(kT, t_end - t0);
        for (int j = 0; j < nt; ++j) {
            const float dl = sd[lane][j], xv = sx[lane][j], dx = dl * xv;
            float y = 0.f;
#pragma unroll
            for (int q = 0; q < kN / 4; ++q) {
                const float4 b4 = *reinterpret_cast<const float4*>(&sB[j][4 * q]);
                const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
                float cc[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (EMIT) {
                    const float4 c4 = *reinterpret_cast<const float4*>(&sC[j][4 * q]);
                    cc[0] = c4.x; cc[1] = c4.y; cc[2] = c4.z; cc[3] = c4.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = 4 * q + e;
                    h[n] = fmaf(__builtin_amdgcn_exp2f(dl * A2[n]), h[n], dx * bb[e]);
                    if constexpr (EMIT) y = fmaf(cc[e], h[n], y);
                }
            }
            if constexpr (EMIT) {
                const float zv = sz[lane][j];
                sd[lane][j] = fmaf(Dp, xv, y) * (zv / (1.0f + expf(-zv)));     // the lane's own slot: y replaces delta
            } else {
                sdl += dl;
            }
        }
        __syncthreads();
        if constexpr (EMIT) {
#pragma unroll
            for (int k = 0; k < kT; ++k) {
                const int idx = lane + 64 * k, r = idx / kT, j = idx % kT;
                if (d0 + r < Di && t0 + j < t_end) yg[(size_t)(d0 + r) * L + t0 + j] = sd[r][j];
            }
            __syncthreads();
        }
    }
    if constexpr (!EMIT) {
        if (live) {
            float* sp = a.state + ((img * ns + chunk) * Di + d) * kN;
#pragma unroll
            for (int q = 0; q < kN / 4; ++q)
                *reinterpret_cast<float4*>(sp + 4 * q) = make_float4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
            a.sdelta[(img * ns + chunk) * Di + d] = sdl;
        }
    }
}

// phase 2: state[c] holds chunk c's end state from a zero start; afterwards the state at the end of chunk c = what chunk c + 1
// starts from.  One thread per (d, n); eight chunks are loaded ahead of the eight dependent steps that consume them.
__global__ void __launch_bounds__(256) mamba_carry_kernel(float* __restrict__ state, const float* __restrict__ sdelta,
                                                          const float* __restrict__ A_log, int Di, int ns) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= Di * kN) return;
    const float A2 = -expf(A_log[gid]) * kLog2e;
    const size_t plane = (size_t)Di * kN;
    float* st = state + (size_t)blockIdx.y * ns * plane + gid;
    const float* sp = sdelta + (size_t)blockIdx.y * ns * Di + gid / kN;
    float H = 0.f;
    for (int c0 = 0; c0 < ns; c0 += 8) {
        float e[8], s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool ok = c0 + u < ns;
            e[u] = ok ? st[(size_t)(c0 + u) * plane] : 0.f;
            s[u] = ok ? sp[(size_t)(c0 + u) * Di] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            H = fmaf(__builtin_amdgcn_exp2f(A2 * s[u]), H, e[u]);
            e[u] = H;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + u < ns) st[(size_t)(c0 + u) * plane] = e[u];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// every refusal names the argument; nothing is launched or dereferenced before this returns RF_OK
int mamba_plan(const char* who, int B, int L, int D, int N, int K, int E, MambaPlan* p, Bump* bump) {
    RF_CHECK_ARG(N == kN, "%s: d_state %d is not supported (d_state must be %d)", who, N, kN);
    RF_CHECK_ARG(K == kDc, "%s: d_conv %d is not supported (d_conv must be %d)", who, K, kDc);
    RF_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 512, "%s: d_model %d must be a positive multiple of 4, at most 512", who, D);
    RF_CHECK_ARG(E >= 1 && (long)E * D <= 4096, "%s: expand %d gives %ld inner channels (1 .. 4096 are supported)", who, E, (long)E * D);
    RF_CHECK_ARG(L >= 1 && L <= (1 << 24), "%s: L %d must be between 1 and 2^24 tokens", who, L);
    RF_CHECK_ARG(B >= 1 && B <= 65535, "%s: B %d must be between 1 and 65535", who, B);
    p->D = D;
    p->Di = E * D;
    p->R = cdiv(D, 16);
    p->NR = p->R + 2 * kN;
    p->nchunk = cdiv(L, kLc);
    const size_t plane = (size_t)B * L;
    p->xz = bump->off(plane * 2 * p->Di);
    p->xc = bump->off(plane * p->Di);
    p->dbc = bump->off(plane * p->NR);
    p->delta = bump->off(plane * p->Di);
    p->state = bump->off((size_t)B * (p->nchunk - 1) * p->Di * kN);
    p->sdelta = bump->off((size_t)B * (p->nchunk - 1) * p->Di);
    p->w_in = bump->off(packed1x1_floats(D, 2 * p->Di));
    p->w_in3 = bump->off(packed1x1_b3_floats(D, 2 * p->Di));
    p->w_x = bump->off(packed1x1_floats(p->Di, p->NR));
    p->w_x3 = bump->off(packed1x1_b3_floats(p->Di, p->NR));
    p->w_out = bump->off(packed1x1_floats(p->Di, D));
    p->w_out3 = bump->off(packed1x1_b3_floats(p->Di, D));
    p->floats = bump->used;
    return RF_OK;
}

// w == nullptr: wp and wp3 already hold the packed forms (the WFB handle's, rf_pack_params) and are only read
int mamba_gemm(const float* x, int K, const float* w, float* wp, float* wp3, float* out, int Cout, int B, int L, hipStream_t st) {
    if (w) {
        RF_TRY(pack_1x1(w, wp, Cout, K, K, 1, st));
        RF_TRY(pack_1x1_b3(w, wp3, Cout, K, K, 1, st));
    }
    Conv1x1Args a{};
    a.x1 = x; a.C1 = K; a.x1_bstride = (int64_t)K * L; a.wp = wp; a.wp3 = wp3; a.ln_eps = 1e-5f;
    a.out = out; a.out_bstride = (int64_t)Cout * L; a.Cout = Cout; a.B = B; a.P = L; a.w = L;
    return launch_conv1x1(a, st);
}

int launch_tok_transpose(const float* in, const float* add, float* out, const float* lw, const float* lb, int B, int rows, int cols,
                         hipStream_t st) {
    const dim3 grid((unsigned)cdiv(rows, 32), (unsigned)B);
    const double el = (double)B * rows * cols;
    ProfScope prof(st, lw ? "tok_transpose_kernel<true>" : "tok_transpose_kernel<false>", 0.0, (add ? 12.0 : 8.0) * el);
    if (lw) tok_transpose_kernel<true><<<grid, 256, 0, st>>>(in, add, out, lw, lb, 1e-5f, rows, cols);
    else tok_transpose_kernel<false><<<grid, 256, 0, st>>>(in, add, out, nullptr, nullptr, 0.f, rows, cols);
    return check_launch("tok_transpose");
}

static ScanArgs scan_args(const MambaPlan& p, const float* const* prm, float* ws, int L) {
    float *xz = ws + p.xz, *dbc = ws + p.dbc, *delta = ws + p.delta;
    ScanArgs a{};
    a.delta = delta; a.x = ws + p.xc; a.z = xz + (size_t)p.Di * L; a.z_bstride = (int64_t)2 * p.Di * L;
    a.bm = dbc + (size_t)p.R * L; a.bc_bstride = (int64_t)p.NR * L; a.A_log = prm[6]; a.Dp = prm[7];
    a.y = delta; a.state = ws + p.state; a.sdelta = ws + p.sdelta; a.Di = p.Di; a.L = L; a.nchunk = p.nchunk;
    return a;
}

// one of the module's three projections: packed per call into the plan's buffers, or read from the handle's packed forms
static int mamba_proj(const MambaPlan& p, const float* x, int K, const float* w, size_t o, size_t o3, const float* pw, const void* pw3, bool packed,
                      float* dst, int Cout, float* ws, int B, int L, hipStream_t st) {
    if (packed) return mamba_gemm(x, K, nullptr, const_cast<float*>(pw), static_cast<float*>(const_cast<void*>(pw3)), dst, Cout, B, L, st);
    return mamba_gemm(x, K, w, ws + o, ws + o3, dst, Cout, B, L, st);
}

int mamba_forward_front(const MambaPlan& p, const float* u, const float* const* prm, float* ws, int B, int L, hipStream_t st, const WmPacked* pk) {
    const float *w_in = prm[0], *w_conv = prm[1], *b_conv = prm[2], *w_x = prm[3], *w_dt = prm[4], *b_dt = prm[5], *A_log = prm[6];
    const int D = p.D, Di = p.Di;
    float *xz = ws + p.xz, *xc = ws + p.xc, *dbc = ws + p.dbc, *delta = ws + p.delta;
    auto gemm = [&](const float* x, int K, const float* w, size_t o, size_t o3, const float* pw, const void* pw3, float* dst, int Cout) {
        return mamba_proj(p, x, K, w, o, o3, pw, pw3, pk != nullptr, dst, Cout, ws, B, L, st);
    };
    RF_TRY(gemm(u, D, w_in, p.w_in, p.w_in3, pk ? pk->in_proj : nullptr, pk ? pk->in_proj3 : nullptr, xz, 2 * Di));
    const double el = (double)B * Di * L;
    {
        const size_t total = (size_t)B * Di * L;
        size_t gx = (total + 255) / 256;
        if (gx > 16384) gx = 16384;
        ProfScope prof(st, "mamba_conv_kernel", 10.0 * el, 8.0 * el);
        mamba_conv_kernel<<<dim3((unsigned)gx), 256, 0, st>>>(xz, xc, w_conv, b_conv, Di, L, total);
        RF_TRY(check_launch("mamba_conv"));
    }
    RF_TRY(gemm(xc, Di, w_x, p.w_x, p.w_x3, pk ? pk->x_proj : nullptr, pk ? pk->x_proj3 : nullptr, dbc, p.NR));
    {
        ProfScope prof(st, "mamba_delta_kernel", 2.0 * p.R * el, 4.0 * el + 4.0 * B * p.R * (double)L);
        mamba_delta_kernel<<<dim3((unsigned)cdiv(L, 256), (unsigned)(Di / 4), (unsigned)B), 256, 0, st>>>(dbc, delta, w_dt, b_dt, Di, p.R, p.NR, L);
        RF_TRY(check_launch("mamba_delta"));
    }
    const ScanArgs a = scan_args(p, prm, ws, L);
    const int ns = p.nchunk - 1;
    const double bc = 4.0 * B * kN * (double)L;
    if (ns > 0) {
        {
            ProfScope prof(st, "mamba_scan_kernel<false>", 4.0 * kN * el, 8.0 * el + bc);
            mamba_scan_kernel<false><<<dim3((unsigned)ns, (unsigned)cdiv(Di, 64), (unsigned)B), 64, 0, st>>>(a);
            RF_TRY(check_launch("mamba_scan<false>"));
        }
        ProfScope prof(st, "mamba_carry_kernel", 0.0, 8.0 * B * ns * (double)Di * kN);
        mamba_carry_kernel<<<dim3((unsigned)cdiv(Di * kN, 256), (unsigned)B), 256, 0, st>>>(a.state, a.sdelta, A_log, Di, ns);
        RF_TRY(check_launch("mamba_carry"));
    }
    return RF_OK;
}

// channel-major Mamba: u, out [B][D][L]; ws = the plan's buffers.  prm: the nine tensors in the header's order.
static int run_mamba(const MambaPlan& p, const float* u, float* out, const float* const* prm, float* ws, int B, int L, hipStream_t st,
                     const WmPacked* pk = nullptr) {
    RF_TRY(mamba_forward_front(p, u, prm, ws, B, L, st, pk));
    const int Di = p.Di;
    const ScanArgs a = scan_args(p, prm, ws, L);
    const double el = (double)B * Di * L, bc = 4.0 * B * kN * (double)L;
    {
        // algorithmic HBM bytes of the scan: read delta, x, z, Bm, Cm, write y
        ProfScope prof(st, "mamba_scan_kernel<true>", 6.0 * kN * el, 16.0 * el + 2.0 * bc);
        mamba_scan_kernel<true><<<dim3((unsigned)p.nchunk, (unsigned)cdiv(Di, 64), (unsigned)B), 64, 0, st>>>(a);
        RF_TRY(check_launch("mamba_scan<true>"));
    }
    return mamba_proj(p, ws + p.delta, Di, prm[8], p.w_out, p.w_out3, pk ? pk->out_proj : nullptr, pk ? pk->out_proj3 : nullptr, pk != nullptr, out,
                      p.D, ws, B, L, st);
}

struct WmPlan {
    MambaPlan m;
    size_t w0, w2, ws_, t1, t2;   // packed 3x3 weights (convb.0, convb.2, smooth); [n][2c][P] and [n][c][P]
    size_t floats;
};

int wm_check_shape(const char* who, int n, int c, int h, int w) {
    RF_CHECK_ARG(h >= 1 && w >= 1 && (double)h * w <= (double)(1 << 24), "%s: h x w = %d x %d must be between 1 and 2^24 pixels", who, h, w);
    RF_CHECK_ARG(c > 0 && c % 4 == 0 && c <= 512, "%s: c %d must be a positive multiple of 4, at most 512", who, c);
    RF_CHECK_ARG(n >= 1 && n <= 65535, "%s: n %d must be between 1 and 65535", who, n);
    RF_CHECK_ARG(8.0 * c * h * w < 2.0e9, "%s: an image of 2c x h x w = %d x %d x %d floats is too large for the 3x3 convolutions", who, 2 * c, h, w);
    return RF_OK;
}

static int wm_plan(const char* who, int n, int c, int h, int w, WmPlan* p) {
    RF_TRY(wm_check_shape(who, n, c, h, w));
    Bump b;
    RF_TRY(mamba_plan(who, n, h * w, c, kN, kDc, 2, &p->m, &b));
    p->w0 = b.off(packed3x3_floats(c, 2 * c));
    p->w2 = b.off(packed3x3_floats(2 * c, c));
    p->ws_ = b.off(packed3x3_floats(c, c));
    p->t1 = b.off((size_t)n * 2 * c * h * w);
    p->t2 = b.off((size_t)n * c * h * w);
    p->floats = b.used;
    return RF_OK;
}

// wgt == nullptr: wp already holds the packed weight
static int wm_conv(const float* x, const float* wgt, const float* wp, const float* bias, float* out, int act, int n, int cin, int cout, int h, int w,
                   hipStream_t st, float* ks = nullptr, size_t ks_floats = 0) {
    if (wgt) RF_TRY(pack_3x3(wgt, const_cast<float*>(wp), cout, cin, st));
    Conv3x3Args a{};
    a.x = x; a.x_bstride = (int64_t)cin * h * w; a.wp = wp; a.bias = bias; a.out = out; a.out_bstride = (int64_t)cout * h * w;
    a.B = n; a.Cin = cin; a.Cout = cout; a.h = h; a.w = w; a.act = act; a.ks_scratch = ks; a.ks_floats = ks_floats;
    return launch_conv3x3(a, st);
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_mamba_chunk_len(void) { return kLc; }

long long rf_mamba_workspace_bytes(int B, int L, int d_model, int d_state, int d_conv, int expand) {
    MambaPlan p;
    Bump b;
    const int rc = mamba_plan("rf_mamba_workspace_bytes", B, L, d_model, d_state, d_conv, expand, &p, &b);
    if (rc) return rc;
    b.off((size_t)B * L * d_model);   // the channel-major copy of a token-major input, then of the output
    return (long long)(b.used * sizeof(float));
}

int rf_mamba_forward(const float* in, float* out, const float* const* prm, void* workspace, size_t workspace_bytes,
                     int B, int L, int d_model, int d_state, int d_conv, int expand, int channel_major, void* stream) {
    MambaPlan p;
    Bump b;
    RF_TRY(mamba_plan("rf_mamba_forward", B, L, d_model, d_state, d_conv, expand, &p, &b));
    const size_t xn = b.off((size_t)B * L * d_model);
    RF_CHECK_ARG(in && out && prm && workspace && aligned16(in) && aligned16(out) && aligned16(workspace),
                 "rf_mamba_forward: in, out, prm and workspace must be non-null and 16-byte aligned");
    if (workspace_bytes < b.used * sizeof(float)) {
        set_error("rf_mamba_forward: workspace of %zu bytes, %zu needed", workspace_bytes, b.used * sizeof(float));
        return RF_E_NOMEM;
    }
    for (int i = 0; i < 9; ++i) RF_CHECK_ARG(prm[i] != nullptr, "rf_mamba_forward: parameter %d is null", i);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (channel_major) return run_mamba(p, in, out, prm, ws, B, L, st);
    RF_TRY(launch_tok_transpose(in, nullptr, ws + xn, nullptr, nullptr, B, L, d_model, st));
    RF_TRY(run_mamba(p, ws + xn, ws + xn, prm, ws, B, L, st));      // in_proj has consumed the buffer long before out_proj writes it
    return launch_tok_transpose(ws + xn, nullptr, out, nullptr, nullptr, B, d_model, L, st);
}

long long rf_wm_workspace_bytes(int n, int c, int h, int w) {
    WmPlan p;
    const int rc = wm_plan("rf_wm_workspace_bytes", n, c, h, w, &p);
    return rc ? rc : (long long)(p.floats * sizeof(float));
}

int rf_wm_forward(const float* in, float* out, const float* const* prm, void* workspace, size_t workspace_bytes,
                  int n, int c, int h, int w, void* stream) {
    WmPlan p;
    RF_TRY(wm_plan("rf_wm_forward", n, c, h, w, &p));
    RF_CHECK_ARG(in && out && prm && workspace && aligned16(in) && aligned16(out) && aligned16(workspace),
                 "rf_wm_forward: in, out, prm and workspace must be non-null and 16-byte aligned");
    if (workspace_bytes < p.floats * sizeof(float)) {
        set_error("rf_wm_forward: workspace of %zu bytes, %zu needed", workspace_bytes, p.floats * sizeof(float));
        return RF_E_NOMEM;
    }
    for (int i = 0; i < 17; ++i) RF_CHECK_ARG(prm[i] != nullptr, "rf_wm_forward: parameter %d is null", i);
    return wm_forward(in, out, prm, nullptr, (float*)workspace, n, c, h, w, (hipStream_t)stream);
}

}  // extern "C"

namespace rf {

int wm_workspace_floats(const char* who, int n, int c, int h, int w, size_t* floats) {
    WmPlan p;
    RF_TRY(wm_plan(who, n, c, h, w, &p));
    *floats = p.floats;
    return RF_OK;
}

int wm_forward_front(const MambaPlan& m, const float* in, const float* const* prm, const WmPacked* pk, float* ws, const WmFrontBufs& b, int n,
                     int c, int h, int w, hipStream_t st) {
    const int L = h * w;
    RF_TRY(wm_conv(in, pk ? nullptr : prm[0], pk ? pk->convb0 : b.w0, prm[1], b.a1, 2 /* ReLU */, n, c, 2 * c, h, w, st, b.ks, b.ks_floats));
    RF_TRY(wm_conv(b.a1, pk ? nullptr : prm[2], pk ? pk->convb2 : b.w2, prm[3], b.r, 0, n, 2 * c, c, h, w, st, b.ks, b.ks_floats));
    // tokens = LayerNorm((convb(x) + x) as runs of c floats), stored channel-major
    RF_TRY(launch_tok_transpose(b.r, in, b.tok, prm[4], prm[5], n, L, c, st));
    return run_mamba(m, b.tok, b.y, prm + 6, ws, n, L, st, pk);      // [n][c][L] = permute(0,2,1).reshape(n,c,h,w)
}

int wm_forward(const float* in, float* out, const float* const* prm, const WmPacked* pk, float* ws, int n, int c, int h, int w,
               hipStream_t st) {
    WmPlan p;
    RF_TRY(wm_plan("wm_forward", n, c, h, w, &p));
    float *t1 = ws + p.t1, *t2 = ws + p.t2;
    // the tokens go over t1, which is dead by then, and Mamba's output over t2
    const WmFrontBufs b{ws + p.w0, ws + p.w2, t1, t2, t1, t2};
    RF_TRY(wm_forward_front(p.m, in, prm, pk, ws, b, n, c, h, w, st));
    return wm_conv(t2, pk ? nullptr : prm[15], pk ? pk->smooth : ws + p.ws_, prm[16], out, 0, n, c, c, h, w, st);
}

}  // namespace rf
