// What the Mamba forward (rf_mamba.hip) and its adjoint (rf_mamba_bwd.hip) share: the geometry of the chunked scan, the
// workspace plan of the forward intermediates and the host steps that fill them.
#pragma once
#include "rf_common.h"

namespace rf {

static constexpr int kN = 32;     // d_state
static constexpr int kDc = 4;     // d_conv
#ifndef RF_MAMBA_LC               // build-time only: tools/kbench.py compares libraries built with other values
#define RF_MAMBA_LC 128
#endif
static constexpr int kLc = RF_MAMBA_LC;   // tokens per chunk
static constexpr int kT = 16;             // tokens per LDS tile
static constexpr int kBrow = kN + 4;      // floats per token row of the Bm / Cm tiles: 16-byte aligned rows, writes 2-way at worst
static_assert(kLc % kT == 0 && kLc > kDc, "a chunk is a whole number of tiles and longer than the convolution");
static constexpr float kLog2e = 1.44269504088896340736f;

struct MambaPlan {
    int D, Di, R, NR, nchunk;
    size_t xz, xc, dbc, delta, state, sdelta, w_in, w_in3, w_x, w_x3, w_out, w_out3;   // float offsets
    size_t floats;
};

// every refusal names the argument; nothing is launched or dereferenced before this returns RF_OK
int mamba_plan(const char* who, int B, int L, int D, int N, int K, int E, MambaPlan* p, Bump* bump);
// w == nullptr: wp and wp3 already hold the packed forms and are only read
int mamba_gemm(const float* x, int K, const float* w, float* wp, float* wp3, float* out, int Cout, int B, int L, hipStream_t st);
int launch_tok_transpose(const float* in, const float* add, float* out, const float* lw, const float* lb, int B, int rows, int cols,
                         hipStream_t st);
// The forward up to the carry pass on channel-major u [B][D][L]: afterwards the plan's xz, xc, dbc and delta buffers hold
// in_proj(u), silu(conv1d(x)), x_proj(xc) and softplus(dt_proj(dt)), `state` the state every chunk but the first starts from and
// `sdelta` the sums of delta over every chunk but the last.
int mamba_forward_front(const MambaPlan& p, const float* u, const float* const* prm, float* ws, int B, int L, hipStream_t st,
                        const WmPacked* pk = nullptr);

// ---- the adjoint schedule of rf_mamba_bwd.hip, as rf_mamba_backward and the WM backward (rf_wm_bwd.hip) call it
struct MambaBwdPlan {
    MambaPlan m;
    int NRp, nct;
    size_t u, g, gu, yg, dpre, dx, dxc, dxz, ddbc, slab, adj, adj_s, dA, dD, cw, cb, csum, wpart, wpart_cap;   // float offsets
    size_t t_in, t_in3, t_x, t_x3, t_dt, t_dt3, t_out, t_out3;                                                 // transposed packs
};
// floats of tensor i of the nine of the pointer arrays, in ops.mamba_param_shapes' order
size_t mamba_prm_floats(int i, int D, int N, int K, int E);
// the forward plan first (same offsets as mamba_plan on a fresh Bump), then the adjoint's buffers
int mamba_bwd_plan(const char* who, int B, int L, int D, int N, int K, int E, MambaBwdPlan* p, Bump* b);
// channel-major: u, g, du [B][D][L]; grd: the nine gradients in the order of prm, written or (acc) added to.  The plan's u, g and
// gu buffers are not touched: they are the caller's (rf_mamba_backward's token-major copies, WM's tok / g_y / g_tok).
int run_mamba_backward(const MambaBwdPlan& p, const float* u, const float* g, float* du, const float* const* prm, float* const* grd,
                       float* ws, int B, int L, int acc, hipStream_t st);

// ---- the row LayerNorm of tok_transpose_kernel<true> and its adjoint wm_ln_bwd_kernel (rf_wm_bwd.hip): mean and rstd of the 32 rows
// r0 .. r0 + 31 of [rows][cols], cols <= 512, into smean / srstd [32].  Each of the four waves of the workgroup takes 8 rows, a row's
// values in registers over both passes; val(o) is the element at offset o (the forward's optional `add` included).  The caller
// synchronises before it reads the two arrays.
template <class V>
__device__ __forceinline__ void tok_row_stats(V&& val, int r0, int rows, int cols, float eps, float* smean, float* srstd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < 8; ++i) {
        const int r = r0 + wave * 8 + i;
        float v[8], s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = lane + 64 * j;
            v[j] = (r < rows && k < cols) ? val((size_t)r * cols + k) : 0.f;
            s += v[j];
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
        const float mean = s / (float)cols;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dv = lane + 64 * j < cols ? v[j] - mean : 0.f;
            q = fmaf(dv, dv, q);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) q += __shfl_xor(q, m, 64);
        if (lane == 0) {
            smean[wave * 8 + i] = mean;
            srstd[wave * 8 + i] = 1.0f / sqrtf(q / (float)cols + eps);
        }
    }
}

// ---- WM (rf_mamba.hip): what rf_wm_forward and the WM backward share
int wm_check_shape(const char* who, int n, int c, int h, int w);      // the refusals of rf_wm_forward, each naming its argument
struct WmFrontBufs {
    float *w0, *w2;            // packed convb.0 / convb.2 weights, written here unless the caller passes WmPacked
    float *a1;                 // [n][2c][P]  relu(convb.0(x))
    float *r;                  // [n][c][P]   convb.2(a1), WITHOUT the skip: the transposition pass adds x on the fly
    float *tok;                // [n][c][L]   LayerNorm(rows of r + x), channel-major (may be a1: dead by then)
    float *y;                  // [n][c][L]   mamba(tok) (may be r)
    // optional scratch of launch_conv3x3's input-channel split (Conv3x3Args::ks_scratch: its counters zero on entry).  The forward
    // passes none and keeps its bits; the backward's small launches run a chain 1/S as long and add the S partial tiles in order
    float *ks = nullptr;
    size_t ks_floats = 0;
};
// WM's forward up to `smooth`, on the forward's own launchers in the forward's order; ws: the buffers of the Mamba plan `m`
int wm_forward_front(const MambaPlan& m, const float* in, const float* const* prm, const WmPacked* pk, float* ws, const WmFrontBufs& b, int n,
                     int c, int h, int w, hipStream_t st);

}  // namespace rf
