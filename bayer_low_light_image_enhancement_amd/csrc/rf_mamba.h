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

}  // namespace rf
