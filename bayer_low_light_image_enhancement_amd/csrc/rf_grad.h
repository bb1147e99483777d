// What the block backward operators (rf_mamba_bwd.hip, rf_wm_bwd.hip, rf_ffab_bwd.hip) share: the weight and data gradients of
// the 1x1 and 3x3 convolutions and the argument checks of their entry points (rf_grad.hip).  Every sum over pixels goes to
// per-workgroup slabs that a second kernel adds in a fixed order: no atomics, two runs give the same bits.
#pragma once
#include <functional>
#include "rf_common.h"

namespace rf {

// launch_reduce_rows inside a profiler bracket: out[e] (+)= sum over rows of partial[row][e]
int reduce_rows(const float* partial, float* out, int nrows, size_t n, int accumulate, hipStream_t st);

// ---- weight gradients.  `who` prefixes the refusal of a partial buffer that is too small; B images of P pixels (tokens)
struct Wgrad { const char* who; float* partial; size_t cap; int B, P, acc; hipStream_t st; };

// The launch_gram2 call for "the weight gradient of this layer": dW [Ca][ld][ntap] and db [Ca] (nullptr: none) (+)= the gradient
// for output gradient a and input b, planes of h = q.P / w rows.  Builds the launch only: the caller adds a second input, if any,
// and launches on the stream of its choice.
Gram2Launch gram2_of(const Wgrad& q, const float* a, int64_t a_bstride, int Ca, const float* b, int64_t b_bstride, int Cb, float* dW, int ld,
                     float* db, int w, int ntap);

// dW [Ca][Cb] and db [Ca] (nullptr: none) (+)= the gradient of a 1x1 convolution with output gradient a (rows i of image n at
// a + n a_bstride + i P) and input b: launch_gram2 with one tap where P % 4 == 0, else wgrad1x1_kernel (16-byte alignment is
// launch_gram2's condition) and reduce_rows.  wgrad1x1_partial_floats: the floats of `partial` the path taken needs.
size_t wgrad1x1_partial_floats(int B, int Ca, int Cb, int P, bool with_bias);
int wgrad1x1(const Wgrad& q, const float* a, int64_t a_bstride, int Ca, const float* b, int64_t b_bstride, int Cb, float* dW, float* db);
// dense planes a [B][Ca][P], b [B][Cb][P]
inline int wgrad1x1(const Wgrad& q, const float* a, int Ca, const float* b, int Cb, float* dW, float* db) {
    return wgrad1x1(q, a, (int64_t)Ca * q.P, Ca, b, (int64_t)Cb * q.P, Cb, dW, db);
}

// dW [Ca][Cb][3][3] and db [Ca] (+)= the gradient of a 3x3 convolution with output gradient a [B][Ca][h][w] and input
// b [B][Cb][h][w], h = q.P / w: launch_gram2 with nine taps where w % 4 == 0, else conv3x3_wgrad_kernel and reduce_rows
size_t wgrad3x3_partial_floats(int B, int Ca, int Cb, int h, int w);
int wgrad3x3(const Wgrad& q, const float* a, int Ca, const float* b, int Cb, float* dW, float* db, int w);

// ---- data gradient of a 1x1 convolution: out [B][Cout][P] = W^T x (+ res, dense [B][Cout][P]) for W [K][Cout] row-major and
// x [B][Kp >= K][P] whose rows K .. Kp - 1 are zero.  The transpose is packed into wp (packed1x1_floats(Kp, Cout)) and, where wp3
// is given (packed1x1_b3_floats(Kp, Cout)), in bf16x3 form too, which selects launch_conv1x1's bf16x3 kernels.
struct Dgrad1x1 {
    const float* x; int K, Kp; int64_t x_bstride;
    const float* w; float* wp; float* wp3;
    const float* res;
    float* out; int64_t out_bstride; int Cout;
    int B, P;
};
int dgrad1x1(const Dgrad1x1& d, hipStream_t st);
// dense planes, f32 GEMM: out [B][cin][P] = W^T g (+ res) for a layer's weight W [cout][cin] and output gradient g [B][cout][P]
inline int dgrad1x1(const float* g, int cout, const float* w, int cin, float* wpack, const float* res, float* out, int B, int P, hipStream_t st) {
    return dgrad1x1(Dgrad1x1{g, cout, cout, (int64_t)cout * P, w, wpack, nullptr, res, out, (int64_t)cin * P, cin, B, P}, st);
}

// ---- the preamble of a block backward entry point  f(in, grad_out, grad_in, prm, grad_prm, workspace, workspace_bytes, ...)
struct Span { const void* p; size_t bytes; };
bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes);
// 0: every output is disjoint from every input and from every other output; 1: outs[*a] overlaps ins[*b]; 2: outs[*a] overlaps outs[*b]
int first_alias(const Span* outs, int nout, const Span* ins, int nin, int* a, int* b);

struct BackwardArgs {
    const char* who;                                 // the entry point: prefixes every refusal
    const float *in, *grad_out; float* grad_in;      // plane_bytes each
    size_t plane_bytes;
    const float* const* prm; float* const* grad_prm; // n tensors each
    int n;
    const void* workspace; size_t workspace_bytes, need_bytes;
    const Span* buffers = nullptr; int nbuffers = 0; // what the call reads besides (BatchNorm's running statistics): no gradient
};
// In this order: in, grad_out, grad_in, prm, grad_prm and workspace non-null and (the arrays apart) 16-byte aligned; the workspace
// large enough (RF_E_NOMEM); no null tensor; then, with prm_floats(i) the floats of tensor i: everything the call writes (grad_in,
// the n gradients, need_bytes of workspace) disjoint from everything it reads (in, grad_out, the n parameters, the buffers) and
// from everything else it writes.  Inputs may overlap each other.  Nothing is dereferenced but the two pointer arrays.
int check_backward_args(const BackwardArgs& c, const std::function<size_t(int)>& prm_floats);

// floats of tensor i of an operator's pointer arrays, in the order of its ops.*_param_shapes: what a schedule over several
// operators (rf_wmb_block_bwd.hip) hands to check_backward_args for the tensors of all of them
size_t ffab_prm_floats(int i, int nc);                        // 92
size_t wm_prm_floats(int i, int c);                           // 17
size_t wfb_prm_floats(int i, int dim, int hidden);            // 12 parameters, then the 4 BatchNorm buffers
size_t illu_prm_floats(int i, int C, int Cm, int Co);         // 6

}  // namespace rf
