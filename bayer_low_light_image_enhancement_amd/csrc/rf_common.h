// Shared declarations for the gfx950 RawFormer kernels (internal; the public ABI is
// include/rawformer_hip.h).  Everything here is written for CDNA4 only: 64-lane waves,
// v_mfma_f32_16x16x4_f32, 160 KB LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/rawformer_hip.h"

namespace rf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

void set_error(const char* fmt, ...);
int check_hip(hipError_t e, const char* what);
int check_launch(const char* what);

#define RF_CHECK_ARG(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            rf::set_error(__VA_ARGS__);    \
            return RF_E_INVALID;           \
        }                                  \
    } while (0)

#define RF_TRY(expr)            \
    do {                        \
        const int rc_ = (expr); \
        if (rc_) return rc_;    \
    } while (0)

// Optional per-launch HIP-event bracket (rf_profile_begin / rf_profile_end in the C ABI):
// bench.py uses it to time each kernel class on the stream it is launched on.
struct ProfScope {
    ProfScope(hipStream_t st, const char* key, double flops, double bytes);
    ~ProfScope();
    hipStream_t st_;
    int rec_;
};
bool profiling_active();   // between rf_profile_begin and rf_profile_end: schedules stay on ONE stream so the brackets mean what they say

// GELU(v) = v/2 (1 + erf(v/sqrt 2)) with erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7), arranged for the fewest
// VALU operations (this sits next to MFMAs, and f32 VALU time adds to f32 MFMA time): with h = v/2 and
// q = 1 - erf(|v|/sqrt 2) = poly(t) t exp(-v^2/2), t = 1 / (1 + p |v|/sqrt 2):
//   GELU = h + |h| (1 - q) = h + fma(-|h|, q, |h|)            (no sign transfer: h sign(v) = |h|)
// 11 plain operations + v_rcp_f32 + v_exp_f32.
__device__ __forceinline__ float gelu_fast(float v) {
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752440f, fabsf(v), 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float ex = __builtin_amdgcn_exp2f((v * v) * (-0.5f * 1.44269504088896340736f));   // exp(-v^2 / 2)
    const float q = (p * t) * ex;
    const float h = 0.5f * v;
    return h + fmaf(-fabsf(h), q, fabsf(h));
}
// the accurate sigmoid (expf) of the gradient kernels and the squeeze-excite gates; the forward's spatial gates use fast_sigmoid /
// fast_tanh (rf_guidance.h)
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }   // p 16-byte aligned
// The exact Haar pair of RawFomer_WFB_FFAB/blocks.py: halve first, then the sums in the order Python evaluates them.  t / r: the 2x2
// quad, row then column.  dwt_init (blocks.py:104-113): x1 = (0,0), x2 = (1,0), x3 = (0,1), x4 = (1,1)
__device__ __forceinline__ void haar_analysis(float t00, float t01, float t10, float t11, float& ll, float& hl, float& lh, float& hh) {
    const float x1 = t00 / 2, x2 = t10 / 2, x3 = t01 / 2, x4 = t11 / 2;
    ll = ((x1 + x2) + x3) + x4;
    hl = ((-x1 - x2) + x3) + x4;
    lh = ((-x1 + x2) - x3) + x4;
    hh = ((x1 - x2) - x3) + x4;
}
// iwt_init (blocks.py:123-134)
__device__ __forceinline__ void haar_synthesis(float ll, float hl, float lh, float hh, float& r00, float& r01, float& r10, float& r11) {
    const float b1 = ll / 2, b2 = hl / 2, b3 = lh / 2, b4 = hh / 2;
    r00 = ((b1 - b2) - b3) + b4;
    r10 = ((b1 - b2) + b3) - b4;
    r01 = ((b1 + b2) - b3) - b4;
    r11 = ((b1 + b2) + b3) + b4;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
// workgroups of 256 threads for a grid-stride loop over n elements: at least one, at most cap
static inline int grid1d(size_t n, int cap = 4096) {
    const size_t g = (n + 255) / 256;
    return g > (size_t)cap ? cap : g < 1 ? 1 : (int)g;
}

// The one allocator behind every workspace / scratch layout: consecutive buffers, each rounded up to 64 floats (256-byte granules
// keep every buffer 16-byte aligned).  off() is the offset form and take() the pointer form of the same step; with a null base
// take() returns nullptr and `used` alone counts (the *_bytes entry points size their layouts that way).
struct Bump {
    float* base = nullptr;
    size_t used = 0;
    size_t off(size_t floats) { const size_t o = used; used += align_up(floats, 64); return o; }
    float* take(size_t floats) { const size_t o = off(floats); return base ? base + o : nullptr; }
};

// ---------------------------------------------------------------------------------------------
// MFMA operand packing.  All dense contractions use v_mfma_f32_16x16x4_f32:
//   A (weights)   lane l holds A[i = l & 15][k = l >> 4]
//   B (pixels)    lane l holds B[k = l >> 4][j = l & 15]
//   C/D           lane l, reg r holds D[row = 4 * (l >> 4) + r][col = l & 15]
// A packed weight matrix [Cout][K] is stored as tiles of 64 floats in lane order:
//   packed[(s * NT + t) * 64 + l] = W[16 t + (l & 15)][4 s + (l >> 4)]      (zero outside)
// with NT = ceil(Cout / 16) and s over ceil(K / 4) k-sets.  A 3x3 weight [Cout][Cin][3][3] is
//   packed[((s * TAPS + dy * TAPS/3 + j) * NT + t) * 64 + l] = u_j(W[16 t + (l & 15)][4 s + (l >> 4)][dy][0..2]),
// the Winograd transform G g of the three taps of kernel row dy (rf_pack.hip; TAPS = 18).
// ---------------------------------------------------------------------------------------------
static inline size_t packed1x1_floats(int K, int Cout) { return (size_t)cdiv(K, 4) * cdiv(Cout, 16) * 64; }
// 3x3 weights are packed in Winograd F(4,3) form along x: 18 transformed taps per k-set
static inline size_t packed3x3_floats(int Cin, int Cout) { return (size_t)cdiv(Cin, 8) * 2 * 18 * cdiv(Cout, 16) * 64; }

// ---------------------------------------------------------------------------------------------
// "b3" operands: an f32 value as the exact sum of three bf16 pieces (truncation split: x = p0 + p1 + p2, 8 significant
// bits each), contracted on the bf16 matrix pipe as six cross terms with f32 accumulation
//   a b ~= a2 b0 + a0 b2 + a1 b1 + a1 b0 + a0 b1 + a0 b0        (dropped: a1 b2, a2 b1, a2 b2 <= 2^-24 |a b|)
// Measured on MI355X (tools/ubench/bf16x3.hip, profiles/r02_ubench_*.txt): the error against an f64 reference equals
// the f32 MFMA chain's (7e-8 .. 6e-7 of sum |a b|, K = 32 .. 2304), and v_mfma_f32_16x16x32_bf16 issues every 17 cycles
// for K = 32 where v_mfma_f32_16x16x4_f32 needs 8 x 33: 6 x 17 = 102 cycles per 16x16x32 block instead of 264.
// (The f32 MFMA runs at the f32 VECTOR rate and is mutually exclusive with VALU work on its SIMD -- tools/ubench/
// mfma_valu.hip -- so it buys operand reuse, not throughput.)
//   v_mfma_f32_16x16x32_bf16:  A lane l holds A[i = l & 15][k = 8 (l >> 4) + e], e = 0..7 (16 bytes, e = ushort index)
//                              B lane l holds B[k = 8 (l >> 4) + e][j = l & 15];   C/D as for the f32 instruction
// A packed b3 weight matrix [Cout][K]: per (k-block s32 of 32 channels, output tile t of 16) three 1 KiB pieces
//   packed3[(((s32 * NT + t) * 3 + piece) * 64 + l) * 8 + e] = piece(W[16 t + (l & 15)][32 s32 + 8 (l >> 4) + e])   (ushort)
// ---------------------------------------------------------------------------------------------
static inline size_t packed1x1_b3_floats(int K, int Cout) { return (size_t)cdiv(K, 32) * cdiv(Cout, 16) * 768; }
int pack_1x1_b3(const float* w, void* packed3, int Cout, int K, int64_t row_stride, int64_t col_stride, hipStream_t st);
// device helpers shared by every producer / consumer of b3 operands
#ifdef __HIPCC__
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void b3_split(float x, unsigned& p0, unsigned& p1, unsigned& p2) {   // pieces = HIGH halves of p0, p1, p2
    p0 = __float_as_uint(x);
    const float r1 = x - __uint_as_float(p0 & 0xffff0000u);
    p1 = __float_as_uint(r1);
    p2 = __float_as_uint(r1 - __uint_as_float(p1 & 0xffff0000u));
}
__device__ __forceinline__ unsigned b3_pack(unsigned even_elem, unsigned odd_elem) {   // high halves -> one dword (element e at ushort e)
    return __builtin_amdgcn_perm(odd_elem, even_elem, 0x07060302u);
}
__device__ __forceinline__ size_t b3_index(int NT, int co, int k, int piece) {   // ushort index of W[co][k]'s piece
    const int lane = (co & 15) + 16 * ((k & 31) >> 3);
    return ((((size_t)(k >> 5) * NT + (co >> 4)) * 3 + piece) * 64 + lane) * 8 + (k & 7);
}
__device__ __forceinline__ void b3_store(unsigned short* dst, int NT, int co, int k, float v) {
    unsigned p0, p1, p2;
    b3_split(v, p0, p1, p2);
    dst[b3_index(NT, co, k, 0)] = (unsigned short)(p0 >> 16);
    dst[b3_index(NT, co, k, 1)] = (unsigned short)(p1 >> 16);
    dst[b3_index(NT, co, k, 2)] = (unsigned short)(p2 >> 16);
}
// six cross terms, smallest first
__device__ __forceinline__ f32x4 b3_mfma(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 c) {
#define RF_B3(x) __builtin_bit_cast(bf16x8, x)
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[2]), RF_B3(b[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[0]), RF_B3(b[2]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[1]), RF_B3(b[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[1]), RF_B3(b[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[0]), RF_B3(b[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[0]), RF_B3(b[0]), c, 0, 0, 0);
#undef RF_B3
    return c;
}
// The same six terms for the four pixel sub-groups of a lane, term-major: an accumulator's six MFMAs form a dependent chain, and
// a dependent v_mfma_f32_16x16x32_bf16 issued straight after its producer waits out the producer's 8 passes (measured: chains
// issued one after the other run at half the 17-cycle issue rate).  Interleaved, three independent MFMAs sit between an
// accumulator's consecutive terms.  Every accumulator still sees its terms in b3_mfma's order: the results are bit-identical.
__device__ __forceinline__ void b3_mfma4(const u32x4 (&a)[3], const u32x4 (&b)[4][3], f32x4 (&c)[4]) {
#define RF_B3(x) __builtin_bit_cast(bf16x8, x)
#define RF_B3_TERM(ia, ib)                                                                                     \
    _Pragma("unroll") for (int g = 0; g < 4; ++g)                                                              \
        c[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(RF_B3(a[ia]), RF_B3(b[g][ib]), c[g], 0, 0, 0);
    RF_B3_TERM(2, 0) RF_B3_TERM(0, 2) RF_B3_TERM(1, 1) RF_B3_TERM(1, 0) RF_B3_TERM(0, 1) RF_B3_TERM(0, 0)
#undef RF_B3_TERM
#undef RF_B3
}
#endif

// ---- weight repacking (rf_pack.hip)
// 1x1: W[Cout][K] row-major -> packed.  `row_stride`/`col_stride` let the source be a
// ConvTranspose2d weight [Cin][Cout][2][2] viewed as rows (o,i,j) x cols k.
int pack_1x1(const float* w, float* packed, int Cout, int K, int64_t row_stride, int64_t col_stride, hipStream_t st);
int pack_3x3(const float* w, float* packed, int Cout, int Cin, hipStream_t st);
int pack_convT(const float* w, float* packed, int Cin, int Cout, hipStream_t st);

// ---- batched weight packing (rf_pack.hip; the training step packs every weight form it needs in a few launches)
struct PackDesc {
    const float* src; float* dst;
    int kind;              // 0: 1x1 generic strides, 1: 3x3 Winograd generic strides (+ tap flip), 2: depthwise taps flipped, 3: 1x1 in b3 form
    int rows, cols;        // of the packed matrix (rows = its output channels)
    int64_t rs, cs;        // floats between rows / columns of src
    int flip;
};
constexpr int kPackBatch = 48;
struct PackBatch { PackDesc d[kPackBatch]; };
size_t pack_desc_floats(const PackDesc& d);
int launch_pack_batch(const PackDesc* d, int n, hipStream_t st);

// ---- decoder step ConvTranspose2d(2C,C,2,2) + cat skip + Conv2d(2C,C,1) on composed weights (rf_upcat.hip)
size_t upcat_packed_floats(int C);
int pack_upcat(const float* up_w, const float* up_b, const float* cr_w, const float* cr_b, float* packed, int C, hipStream_t st);
bool upcat_supported(int C, int h, int w, const void* x, const void* skip, const void* out);
int launch_upcat(const float* x, const float* skip, float* out, const float* packed, int B, int C, int h, int w, hipStream_t st);

// ---- conv1x1 (rf_gemm1x1.hip)
struct Conv1x1Args {
    const float* x1;       // first source, channel 0 of image 0
    const float* x2;       // second source or nullptr
    int C1, C2;            // channels taken from each source (K = C1 + C2)
    int64_t x1_bstride;    // floats between images in source 1
    int64_t x2_bstride;
    const float* x3;       // third source (bf16x3 streaming kernel only: the composed Conv_Transformer tail, rf_model.hip) or nullptr
    int C3;                // K = C1 + C2 + C3
    int64_t x3_bstride;
    const float* wp;       // packed weights
    int64_t wp_bstride;    // floats between per-image weight sets (0 = shared)
    const void* wp3;       // the same weights in b3 form (packed1x1_b3_floats) or nullptr: selects the bf16x3 kernels
    int64_t wp3_bstride;   // floats between per-image b3 weight sets (0 = shared)
    const float* bias;     // [Cout] or nullptr
    const float* ln_w;     // LayerNorm prologue over the K channels (nullptr = none)
    const float* ln_b;
    float ln_eps;
    const float* res;      // residual, same layout as out (nullptr = none)
    int64_t res_bstride;
    float* out;
    int64_t out_bstride;
    int Cout;              // rows of W (for mode 1: 4 * output channels)
    int B, P;              // images, pixels per image
    int w;                 // image width (mode 1 only)
    int mode;              // 0: out[co][p]; 1: ConvTranspose2d 2x2 scatter, row co = 4*o + 2*i + j
    int act;               // 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 LeakyReLU(0.1), 4 clamp to [0, 1e4] (FEB, blocks.py:14-30)
};
// What launch_conv1x1 will launch for `a`, decided on the host alone (no HIP call): plan_conv1x1 in rf_gemm1x1.hip is the single
// statement of the selection rule.
struct Conv1x1Plan {
    int inst;              // row of rf_gemm1x1.hip's instantiation table: the kernel and its template arguments
    const char* key;       // that row's name: the profiler key, and the kernel name a trace shows
    unsigned grid[3], block;
    size_t lds;            // dynamic LDS bytes
    int karg[2];           // the kernel's integer arguments: (ntw, ngroups) resident-input | (ngroups) streaming, b3 | (tpw) b3_ln
    double flops, bytes;   // of the whole launch, for ProfScope
    bool ln_single_pass;   // the LayerNorm prologue (if any) reads x once: see conv1x1_ln_single_pass
    bool dw3;              // the form whose third source is produced on the fly (rf_gemm1x1_dw3.hip): `inst` is unset
};
// Optional descriptor of source 3: x3 holds the tensor BEFORE a depthwise 3x3 (padding 1) + GELU, and the GEMM applies both while
// it reads (conv1x1_b3_dw3_kernel; the composed stage tail of levels 1-3, whose hidden tensor then crosses HBM twice instead of
// four times).  It travels beside Conv1x1Args and not inside it: that struct is the by-value parameter of every 1x1 kernel, and
// a member more moves the kernels' trailing arguments, i.e. changes the code of all of them.
struct Conv1x1Dw3 {
    const float* w;        // depthwise weights [C3][9]
    const float* bias;     // [C3] or nullptr
    int h, w_;             // the image: h * w_ == P
};
constexpr int kDw3MaxC3 = 256;      // depthwise weights and bias of all C3 channels are staged in LDS
// RF_E_INVALID (and the error text) for arguments launch_conv1x1 refuses; `dw3` is honoured only where the plan takes the new
// form (p->dw3) -- everywhere else x3 must hold the finished source, and the caller asks the plan which it is
int plan_conv1x1(const Conv1x1Args& a, Conv1x1Plan* p, const Conv1x1Dw3* dw3 = nullptr);
int launch_conv1x1(const Conv1x1Args& a, hipStream_t st, const Conv1x1Dw3* dw3 = nullptr);
int launch_conv1x1_b3_dw3(const Conv1x1Args& a, const Conv1x1Dw3& d, const Conv1x1Plan& p, hipStream_t st);      // rf_gemm1x1_dw3.hip; called by launch_conv1x1
// one dense NCHW source and a dense destination (batch strides C1 P / Cout P); everything else zero
inline Conv1x1Args conv1x1_dense(const float* x1, int C1, const float* wp, const void* wp3, const float* bias, float* out, int Cout, int B, int P, int w) {
    Conv1x1Args a{};
    a.x1 = x1; a.C1 = C1; a.x1_bstride = (int64_t)C1 * P; a.wp = wp; a.wp3 = wp3; a.bias = bias;
    a.out = out; a.out_bstride = (int64_t)Cout * P; a.Cout = Cout; a.B = B; a.P = P; a.w = w;
    return a;
}
// Workgroup id -> (unit, grp) for `ngroups` workgroups per unit that read the same input (conv1x1_b3_kernel's paired form: a unit
// is one pixel tile of one image, a group one pair of output groups).  The hardware deals consecutive ids round-robin over the 8
// XCDs (one L2 each), so the groups of a unit get ids 8 apart: the same XCD, one after the other in its dispatch order, and the
// L2 serves the re-reads.  Ids come in chunks of 8 units x ngroups; ids [0, units * ngroups) alone cannot do this when
// units % 8 != 0 (one unit with two groups would own ids 0 and 1), so the grid is conv1x1_group_grid(units, ngroups) ids, the
// last chunk padded to 8 units, and the ids of the missing units return false (at most 7 * ngroups of them).  The ids that
// return true map one to one onto the (unit, grp) pairs.
__host__ __device__ inline bool conv1x1_group_map(unsigned id, unsigned units, unsigned ngroups, unsigned* unit, unsigned* grp) {
    const unsigned chunk = id / (8u * ngroups), r = id - chunk * 8u * ngroups;
    *unit = 8u * chunk + (r & 7u);
    *grp = r >> 3;
    return *unit < units;
}
inline unsigned conv1x1_group_grid(unsigned units, unsigned ngroups) { return (units + 7u) / 8u * 8u * ngroups; }
bool conv1x1_ln_single_pass(const Conv1x1Args& a);   // false: cheaper as layernorm2d + the plain GEMM (the prologue would re-read x per output group)

// ---- conv3x3 (rf_conv3x3.hip)
struct Conv3x3Args {
    const float* x;        // [B][Cin][h][w]; with unshuffle_in: mosaic [B][Cin/4][2h][2w]
    int64_t x_bstride;
    const float* wp;       // packed 3x3 weights
    const float* bias;     // [Cout] or nullptr
    float* out;
    int64_t out_bstride;
    int B, Cin, Cout, h, w;
    int act;               // 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 GELU, 4 tanh (EnhancedBayerProcessor, BayerTORGBColorMultiLvl.py:86-98)
    int store;             // 0 plain, 1 pixel-unshuffle, 2 pixel-shuffle
    int unshuffle_in;      // read the input through the Bayer pack (a1)
    int clamp_in;          // clamp input to [0,1] while loading
    int clamp_out;         // clamp output to [0,1] before storing
    // optional scratch for the input-channel split of small launches (rf_conv3x3.hip, KS): conv3x3_ksplit_floats() floats whose
    // first 4096 are zero before the first launch (the kernels leave them zero); nullptr = never split.  One launch at a time.
    float* ks_scratch = nullptr;
    size_t ks_floats = 0;
};
// What launch_conv3x3 will launch for `a`, decided on the host alone (no HIP call): plan_conv3x3 in rf_conv3x3.hip is the single
// statement of the selection rule.
struct Conv3x3Plan {
    int nco, log2_rw, rpw, nwv, ks, l0;    // the template arguments of conv3x3_kernel (ks: ksplit > 1)
    int ngroups, tiles_x, ntiles, vec;     // the kernel's integer arguments
    dim3 grid;                             // grid.z = ksplit
    unsigned block;
    int ksplit;                            // workgroups that share the input channels of a tile (1: no split); above 1 only where
                                           // every workgroup has exactly one tile, grid.x == ngroups * ntiles
    char key[64];                          // the profiler key: the instantiation's name (a split launch: the unsplit kernel's)
    double flops, bytes;                   // of the whole launch, for ProfScope
};
int plan_conv3x3(const Conv3x3Args& a, Conv3x3Plan* p);    // RF_E_INVALID (and the error text) for arguments launch_conv3x3 refuses
int launch_conv3x3(const Conv3x3Args& a, hipStream_t st);
// dense NCHW source and destination (batch strides Cin h w / Cout h w, also through a pixel (un)shuffle); everything else zero
inline Conv3x3Args conv3x3_dense(const float* x, const float* wp, const float* bias, float* out, int B, int Cin, int Cout, int h, int w, int act) {
    Conv3x3Args a{};
    a.x = x; a.x_bstride = (int64_t)Cin * h * w; a.wp = wp; a.bias = bias; a.out = out; a.out_bstride = (int64_t)Cout * h * w;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.h = h; a.w = w; a.act = act;
    return a;
}
size_t conv3x3_ksplit_floats(int B, int Cout, int h, int w);   // 0: launches of this size never split
size_t conv3x3_ksplit_counter_bytes();

// ---- named parameter groups: one struct per group, over the element type -- int: registry indices (rf_handle.h), const float*:
// device pointers, float*: gradients.  Field order = registration order = the reference's state_dict order.
template <class T> struct SeGroup { T se1_w, se1_b, se3_w, se3_b; };      // squeeze-excite: se.1 and se.3, weight and bias
template <class T> struct FlcaGroup {                                     // FLCA branch of a stage
    T alpha, beta, gamma;                 // scalars
    T w_low, w_high, w_chr;               // low_attn.0 / high_attn.0 [C][1][3][3], chroma_attn.0 [C][2][3][3]
    SeGroup<T> se;
};
typedef SeGroup<const float*> SePrm;
typedef FlcaGroup<const float*> FlcaPrm;
typedef FlcaGroup<float*> FlcaGrad;
static inline int flca_hidden(int C) { return C / 8 > 8 ? C / 8 : 8; }   // width of the squeeze-excite hidden layer

// ---- memory-bound ops (rf_pointwise.hip)
int launch_layernorm2d(const float* in, float* out, const float* w, const float* b, float eps,
                       int B, int C, int P, hipStream_t st);
struct DwConvArgs {
    const float* x; int64_t x_bstride;
    float* out; int64_t out_bstride;
    const float* w;        // [C][9]
    const float* bias;     // [C] or nullptr
    int B, C, h, w_;
    int gelu;
    float* out2 = nullptr; // training forward: out keeps the pre-activation, out2 (layout of out) receives GELU(out) with the exact erf
};
int launch_dwconv3x3(const DwConvArgs& a, hipStream_t st);
int launch_pixel_unshuffle2(const float* in, float* out, int B, int C, int h, int w, hipStream_t st);
int launch_pixel_shuffle2(const float* in, float* out, int B, int C, int h, int w, hipStream_t st);
// 2x2 analysis/synthesis with an arbitrary 4x4 matrix.  layout 0: bands on the batch axis
// (dwt_init), 1: band-major channels (CustomDWT), 2: four separate [B,C,h,w] planes (HaarDWT).
// exact_haar selects the reference's summation order for dwt_init / iwt_init (bit-exact).
int launch_dwt2x2(const float* in, float* out, const float k[16], int layout, int exact_haar,
                  int B, int C, int h, int w, int hin, int win, hipStream_t st);
int launch_idwt2x2(const float* in, float* out, const float k[16], int layout, int exact_haar,
                   int B, int C, int h, int w, hipStream_t st);

// ---- channel attention (rf_attn.hip)
struct GramArgs {
    const float* q; const float* k;   // channel 0 of image 0 for q and k
    int64_t bstride;                  // floats between images
    int B, C, heads, P;
    float* partial;                   // [B][nslab][C][bandw + 2]  (see gram_partial_floats)
    int nslab, slab;
    int p_lo = 0, p_hi = 0;           // pixels [p_lo, p_hi) enter the statistics (p_hi = 0: all); see rf_set_shard
    int w = 0, x_lo = 0, x_hi = 0;    // ... and of those only columns [x_lo, x_hi) of the w-wide image (x_hi = 0: all); rf_set_shard_grid
};
int gram_plan(int B, int C, int heads, int P, int* nslab, int* slab, size_t* partial_floats);
int launch_gram(const GramArgs& a, hipStream_t st);
// softmax + fold into project_out: wp_out[b] = pack(W_out * blockdiag(attn_b))
// wp_out == nullptr: the b3 form only.  perm (C = 32): the b3 form's rows in the order the fused FFN kernel's projection step
// wants them (fold_row_perm32).
int launch_attn_fold(const float* partial, int nslab, const float* temperature, const float* w_out,
                     float* wp_out /* or nullptr */, void* wp3_out /* b3 form too, or nullptr */, int B, int C, int heads, hipStream_t st,
                     int log_temperature = 0, bool perm = false);
// Row of the folded 32 x 32 projection that holds output channel `co` in the permuted b3 form: row 16 t + 4 a + r <-> channel
// 8 a + 4 t + r, so that the MFMA's output rows 16 t + 4 kq + r of lane (j, kq) are its LayerNorm channels 8 kq + (4 t + r)
// (proj_step_b3, rf_fused_tile.h)
__host__ __device__ static inline int fold_row_perm32(int co) { return 16 * ((co >> 2) & 1) + 4 * (co >> 3) + (co & 3); }

// ---- fused transformer-block kernels (rf_fused.hip).  The kernels take these structs by value: their layout is the kernels'.
// The caller fills the tensors, B / h / w, nslab (from the plan) and the shard window; the launcher fills tiles_x, ntiles and
// rgroups and clamps yhi / xhi.
struct FfnArgs {           // out = x + W2 gelu(dw3x3(W1 LN2(x) + b1) + bd) + b2, for C = 32 / 48
    const float* x;        // [B][C][h][w] block input (also the residual)
    float* out;            // [B][C][h][w]
    const float* ln_w; const float* ln_b;
    const void* w1p;       // b3-packed pw1 weight [C/32][2C/16][3][64] 16-byte elements
    const float* b1;       // [2C]
    const float* wd;       // [2C][9]
    const float* bd;       // [2C]
    const float* w2p;      // packed [2C/4][C/16][64]
    const float* b2;       // [C]
    int B, h, w, tiles_x, ntiles;
};
// Stage tail (C = 32 only, fused_ffn_tail_supported): with one the kernel writes channel_reduce(cat(xs, x + ffn(x)))
//   out = Wa'_b xs + Wb x + (Wb W2) g + (Wb b2 + b_cr)       (g = the GELU output; composition: rf_flca.hip pack_tail)
// FfnArgs.b2 is then the composed bias and FfnArgs.w2p is not read: Wb W2 is the last 2C/4 k-sets of `wp`.
struct FfnTail {
    const float* xs;           // [B][C][h][w] branch output; nullptr: no tail
    const float* wp;           // [Wa' | Wb | Wb W2] in f32 MFMA operand order [(2C + 2C)/4][C/16][64] (flca_fold_kernel's wp_out)
    int64_t wp_bstride;        // floats between the images' sets (0: one static set)
};
// The attention projection inside the kernel too (with a tail only): FfnArgs.x is then the BLOCK's input and the kernel forms
//   x1 = x + Wf_b v + bias       per halo'd tile, in place of reading it,
// so the projection GEMM's launch and x1's trip through HBM go.  Carried beside FfnArgs / FfnTail: their layout is the kernels'.
struct FfnProj {
    const float* v;            // [B][C][h][w] at v_bstride floats per image: the attention front's depthwise-convolved v
    int64_t v_bstride;
    const void* wf3;           // [B] folded projection weights, b3 form with permuted rows (launch_attn_fold, perm)
    const float* bias;         // [C] project_out's bias
};
bool fused_ffn_supported(int C, int hidden, int h, int w);
bool fused_ffn_tail_supported(int C);
// Does a level-`lvl` stage with the fused tail take the projection form?  From the level and (h, w) alone, never from B (the
// two forms round differently: see fused_attn_plan).
bool fused_ffn_proj_rule(int lvl, int h, int w);
int launch_ffn_fused(FfnArgs a, int C, hipStream_t st, FfnTail tail = FfnTail{nullptr, nullptr, 0}, const FfnProj* proj = nullptr);
int launch_ffn_fused_proj32(const FfnArgs& a, const FfnTail& tail, const FfnProj& pj, dim3 grid, hipStream_t st);   // rf_fused_proj.hip; called by launch_ffn_fused
int launch_ffn_fused_tail32(const FfnArgs& a, const FfnTail& tail, dim3 grid, hipStream_t st);   // rf_fused_tail.hip; called by launch_ffn_fused

struct AttnFrontArgs {     // LN1 -> qkv 1x1 -> depthwise 3x3 -> Gram partials of (q, k) + v, for C = 32
    const float* x;        // [B][C][h][w]
    float* v;              // [B][C][h][w]  depthwise-convolved v
    float* partial;        // [B][nslab][C/16][16][66]  (layout of rf_attn.hip: band of one k tile)
    const float* ln_w; const float* ln_b;
    const void* wp;        // b3-packed qkv weight [C/32][3C/16][3][64] 16-byte elements
    const float* bq;       // [3C]
    const float* wd;       // [3C][9]
    const float* bd;       // [3C]
    int B, h, w, tiles_x, ntiles, nslab;
    int ylo, yhi;          // rows [ylo, yhi) enter the Gram statistics (a spatial shard's interior); yhi = 0: all
    int xlo, xhi;          // ... and columns [xlo, xhi) of them, both multiples of 4 or xhi = w: whole 4-pixel groups; xhi = 0: all
};
bool fused_attn_supported(int C, int heads, int h, int w);
// The one statement of the launch geometry, from (h, w) alone: the workgroups per image (= partials), the floats of partials they
// write, in *tall_form whether the eight-wave kernel on 12-row tiles runs (above 256 x 256 packed) or the 4-row kernel, and in
// *reserve_floats what a scratch layout sets aside for the partial buffer (>= *partial_floats; the same for either form).
int fused_attn_plan(int h, int w, int* nslab, size_t* partial_floats, int B, int C, int* tall_form = nullptr, size_t* reserve_floats = nullptr);
int launch_attn_front(AttnFrontArgs a, int C, hipStream_t st);
int launch_attn_front_tall32(const AttnFrontArgs& a, dim3 grid, hipStream_t st);      // rf_attn_front_tall.hip; called by launch_attn_front

struct AttnMidArgs {       // qkv [B,3C,h,w] -> depthwise 3x3 -> Gram partials of (q, k) + v, for C = 64 / 128
    const float* qkv;      // [B][3C][h][w]
    float* v;              // [B][C][h][w]  depthwise-convolved v
    float* partial;        // [B][nslab][C/16][16][66]  (layout of attn_front_kernel / rf_attn.hip)
    const float* wd;       // [3C][9]
    const float* bd;       // [3C]
    int B, h, w, tiles_x, ntiles, nslab;
    int ylo, yhi;          // as AttnFrontArgs
    int xlo, xhi;
    int rgroups;           // gridDim.z: the rounds (Gram tiles, then v parts) are split over this many workgroups per slab
};
bool attn_mid_supported(int C, int heads, int h, int w);
int attn_mid_plan(int h, int w, int* nslab, size_t* partial_floats, int B, int C);
int launch_attn_mid(AttnMidArgs a, int C, hipStream_t st);

// ---- TransformerBlock schedule (rf_block.hip)
struct TbParams {
    const float *ln1_w, *ln1_b, *temperature;
    const float *qkv_wp /* packed */, *qkv_b, *qkv_dw_w, *qkv_dw_b, *proj_w /* raw [C][C] */, *proj_b;
    const float *ln2_w, *ln2_b, *pw1_wp /* packed */, *pw1_b, *dw_w, *dw_b, *pw2_wp /* packed */, *pw2_b;
    const void *qkv_wp3, *pw1_wp3, *pw2_wp3;   // b3 forms of the three packed weights (nullptr: f32 kernels only)
    int log_temperature;                       // `temperature` holds log T (TrueColorRawFormer, BayerTORGBColorMultiLvl.py:331,344)
    // spatial shard (rf_set_shard / rf_set_shard_grid): rows [ylo, yhi) and columns [xlo, xhi) (xhi = 0: all) of this level
    // enter the Gram statistics, and `allreduce` sums the
    // slab partials over the ranks before the softmax (nullptr: single device)
    int ylo = 0, yhi = 0, xlo = 0, xhi = 0;
    void (*allreduce)(void* user, float* buf, size_t n, int op, void* stream) = nullptr;
    void* allreduce_user = nullptr;
    // composed stage tail: on the op-by-op FFN path stop after depthwise 3x3 + GELU -- x + attn(..) stays in the x1 buffer, the
    // hidden tensor in bufB, `out` is not written; the caller's channel_reduce GEMM applies pointwise2 (transformer_ffn_is_fused
    // tells it which path runs)
    bool defer_pw2 = false;
    // ... and stop one launch earlier still, after pointwise1: the hidden tensor stays in bufA before its depthwise 3x3 + GELU, which
    // the caller's GEMM applies as it reads (Conv1x1Dw3; the caller has asked plan_conv1x1).  Only with defer_pw2.
    bool defer_dw = false;
    // fused stage tail: on the fused FFN path (C = 32) the kernel applies the caller's channel_reduce too, `out` receives
    // channel_reduce(cat(tail.xs, block output)); tail_bias = the composed bias
    FfnTail tail{nullptr, nullptr, 0};
    const float* tail_bias = nullptr;
};
bool transformer_ffn_is_fused(const TbParams& p, int C, int hc, int hh, int ww);
struct TbBufOffsets { size_t bufA, bufB, x1, partial, wfold, wfold3; };   // float offsets into one scratch area
size_t transformer_scratch_floats(int B, int C, int heads, int hc, int h, int w, TbBufOffsets* o);
int run_transformer(const TbParams& p, const float* in, float* out, float* ws, const TbBufOffsets& o,
                    int B, int C, int heads, int hc, int hh, int ww, hipStream_t st);
// its two halves: x1 = in + attn(LN1(in)) into the x1 buffer, then out = x1 + ffn(LN2(x1)) (a caller may order other work
// between them: run_stage joins the branch there when the FFN kernel carries the stage tail)
// `proj` (run_stage, where fused_ffn_proj_rule holds): the attention half stops after the fold and says there what the FFN kernel
// needs to apply the projection itself; the FFN half then reads `proj_in`, the block's input, and x1 is never written.
int run_transformer_attn(const TbParams& p, const float* in, float* ws, const TbBufOffsets& o, int B, int C, int heads, int hh, int ww,
                         hipStream_t st, FfnProj* proj = nullptr);
int run_transformer_ffn(const TbParams& p, float* out, float* ws, const TbBufOffsets& o, int B, int C, int hc, int hh, int ww, hipStream_t st,
                        const float* proj_in = nullptr, const FfnProj* proj = nullptr);
// The attention half of the block, also the whole of rf_chan_attn:  out = [in +] W_out softmax(T q^ k^T) v + b  with
// q, k, v = depthwise3x3(W_qkv [LN1](in)).  Reads the attention fields of `p`; p.ln1_w == nullptr: no LayerNorm (and never the
// attn_front kernel, which has one built in).  The no_fuse switches are the diagnostic build's (run_transformer sets them).
struct AttnBufs {
    float *pre, *qkv;     // [B][3C][P] each: the qkv GEMM's output and the depthwise convolution's (or v alone, [B][C][P])
    float *partial;       // Gram partials: the largest of gram_plan / fused_attn_plan / attn_mid_plan for the shape
    float *wfold;         // [B] packed1x1_floats(C, C)
    void* wfold3;         // [B] packed1x1_b3_floats(C, C)
};
int run_chan_attn(const TbParams& p, const float* in, float* out, bool residual, const AttnBufs& buf, int B, int C, int heads, int hh, int ww,
                  hipStream_t st, bool no_fuse = false, bool no_fuse_attn = false, FfnProj* proj = nullptr);

// ---- rfft2 / irfft2 with the polar maps of FEB (rf_fft.hip); cscratch: planes * h * (w/2 + 1) complex values
// What both launchers launch for [planes][h][w], decided on the host alone (no HIP call): plan_fft is the single statement of the
// geometry and of the argument checks.  A row workgroup takes L rows at a time and a column workgroup TC columns of one plane.
struct FftPlan {
    int log2w, log2h;          // per axis: log2 of the line length (radix 2), or -1 (direct DFT)
    int L, TC;
    int wf, rows, units;       // w/2 + 1;  planes * h lines for the row kernels;  planes * ceil(wf / TC) column tiles
    unsigned gx, gy;           // grids of the row and the column kernel: row groups / column tiles, capped (persistent loops)
    size_t lds_rows, lds_cols; // dynamic LDS bytes
};
int plan_fft(const char* what, int planes, int h, int w, FftPlan* p);    // RF_E_INVALID (and the error text) for sizes the launchers refuse
int launch_rfft2_polar(const float* in, float* mag, float* pha, float2* cscratch, int planes, int h, int w, hipStream_t st);
int launch_polar_irfft2(const float* mag, const float* pha, const float* res, float* out, float2* cscratch, int planes, int h, int w,
                        float lim, hipStream_t st);
int launch_clamp(const float* in, float* out, size_t n, float lo, float hi, hipStream_t st);
int launch_rfft_rows(const float* in, float2* cscratch, int planes, int h, int w, hipStream_t st);   // the row pass of launch_rfft2_polar alone
// their adjoints (rf_ffab_bwd.hip): (mag, pha, dL/dout) -> (dL/dmag, dL/dpha);  (in, dL/dmag, dL/dpha) -> dL/din, the spectrum recomputed
int launch_polar_irfft2_backward(const float* mag, const float* pha, const float* gout, float* gmag, float* gpha, float2* cscratch, int planes,
                                 int h, int w, hipStream_t st);
int launch_rfft2_polar_backward(const float* in, const float* gmag, const float* gpha, float* gin, float2* cscratch, int planes, int h, int w,
                                hipStream_t st);

// ---- TrueColorRawFormer extras (rf_truecolor.hip)
size_t tc_front_scratch_floats(int B, int H, int W, int levels);
int launch_tc_front(const float* in, int mosaic, const float* wb_gains, const float* color_matrix, const float* wp_c0, const float* b_c0,
                    const float* wp_c2, const float* b_c2, const float* wp_d0, const float* b_d0, const float* wp_d2, const float* b_d2,
                    float* scratch, int B, int H, int W, int levels, hipStream_t st);
int launch_tc_guide_level(const float* scratch, float* guide, int B, int H, int W, int levels, int hf, int wf, hipStream_t st);
int tc_front_outputs(const float* scratch, const float** y, const float** crcb, const float** rgb, int B, int H, int W, int levels);
int tc_nblk(int h, int w);
int launch_tc_spatial(const float* feat, float* xs, const float* guide, const float* w_col, const float* b_col, const float* w_low,
                      const float* b_low, const float* w_high, const float* b_high, int B, int C, int h, int w, hipStream_t st);
int launch_tc_residual(const float* xs, const float* r, float* x2, float* partial, int B, int C, int h, int w, hipStream_t st);
int launch_tc_color_head(float* x, const float* const* prm, int B, size_t P, hipStream_t st);
int launch_tc_pyramid(const float* src, float* ll, float* mag, int B, int hs, int ws, hipStream_t st);
int check_gate_shape(const char* who, int B, int C, int h, int w);   // the shape checks the rf_tc_* and rf_ml_* entry points share

// ---- multi-level FLCA RawFormer extras (rf_multilvl.hip): guidance pyramid, per-stage planes and pooled means, the gated
// modulation of one residual step (step = pyramid level, or `levels` for the chroma form), the output corrections
size_t ml_scratch_floats(int B, int H, int W, int levels);
int launch_ml_guidance(const float* in, int mosaic, float* scratch, int B, int H, int W, int levels, hipStream_t st);
int launch_ml_guide_level(float* scratch, float* guide, int lvl, int B, int H, int W, int levels, int hf, int wf, hipStream_t st);
const float* ml_level_means(const float* scratch, int lvl, int B, int H, int W, int levels);
int launch_ml_modulate(const float* x, float* out, const float* guide, const float* means, int step, int levels, const float* w_a,
                       const float* w_b, const float* gate_w, const float* gate_b, int B, int C, int h, int w, hipStream_t st);
int launch_ml_residual(const float* x, const float* r, float* out, int B, int C, int h, int w, hipStream_t st);
bool ml_step_fused_supported(int C, int h, int w);
int launch_ml_step_fused(const float* x, float* out, const float* guide, const float* means, int step, int levels, const float* w_a,
                         const float* w_b, const float* gate_w, const float* gate_b, const float* w0, const float* b0, const float* w2,
                         const float* b2, float* partial, int B, int C, int h, int w, hipStream_t st);
int launch_ml_tail(float* out, const float* in, int mosaic, float* scratch, int B, int H, int W, int levels, hipStream_t st);

// ---- FLCA_Pyramid as an operator (rf_flca_pyramid.hip): what rf_flca_pyramid_forward and the backward (rf_flca_pyramid_bwd.hip)
// share.  PyrGroup: the 4 L + 11 tensors of the block in state_dict order (= the C ABI's pointer arrays), by name.
template <class T> struct PyrGroup {
    T low[3], high[3], gate_w[3], gate_b[3];      // low_attn.<l>.0 / high_attn.<l>.0 [C][1][3][3], freq_gate_head.<l> [2][2], [2]
    T chr_w, cgate_w, cgate_b;                    // chroma_attn.0 [C][2][3][3], chroma_gate [1], [1]
    SeGroup<T> se;
    T r0_w, r0_b, r2_w, r2_b;                     // res_proj.0 / .2: [C][C], [C]
};
template <class T> PyrGroup<T> pyr_group(T const* a, int L) {
    PyrGroup<T> g{};
    for (int l = 0; l < L; ++l) { g.low[l] = a[l]; g.high[l] = a[L + l]; g.gate_w[l] = a[2 * L + 2 * l]; g.gate_b[l] = a[2 * L + 2 * l + 1]; }
    a += 4 * L;
    g.chr_w = a[0]; g.cgate_w = a[1]; g.cgate_b = a[2];
    g.se = {a[3], a[4], a[5], a[6]};
    g.r0_w = a[7]; g.r0_b = a[8]; g.r2_w = a[9]; g.r2_b = a[10];
    return g;
}
size_t pyr_prm_floats(int i, int C, int levels);  // floats of tensor i of the pointer arrays
// Float offsets of what the forward schedule uses, at the head of either entry point's workspace.  m, t, r and the two packed
// matrices exist where a step is composed, and for the backward, which composes every step it differentiates.
struct PyrFwdPlan {
    bool fused;                                   // the steps run as launch_ml_step_fused
    int nblk;                                     // pooling blocks per image: tc_nblk(h, w), the layout both step forms leave
    size_t gscratch, guide, m, t, r, wp0, wp2, pool, ch;
};
// the shape checks of both entry points (`who` prefixes the refusal), then the layout
int pyr_fwd_plan(const char* who, int B, int C, int h, int w, int H, int W, int levels, bool backward, PyrFwdPlan* p, Bump* b);
// guidance and means at (h, w), then x_{s+1} -> x_next[s] for s = 0 .. levels (x_next[s] may be x_next[s - 1]: a step runs in
// place); leaves the pooling sums of x_{levels+1} in ws + p.pool
int pyr_forward_steps(const PyrFwdPlan& p, float* ws, const float* feat, const float* packed, float* const* x_next,
                      const PyrGroup<const float*>& prm, int B, int C, int h, int w, int H, int W, int levels, hipStream_t st);
// one residual step's m = x S_s, t = relu(W0 m + b0), r = W2 t + b2 into ws + p.m / p.t / p.r (the packs in p.wp0 / p.wp2 are
// pyr_forward_steps's or, with `pack`, written first)
int pyr_step_mtr(const PyrFwdPlan& p, float* ws, const float* x, int step, const PyrGroup<const float*>& prm, bool pack, int B, int C,
                 int h, int w, int H, int W, int levels, hipStream_t st);
const float* pyr_means(const PyrFwdPlan& p, const float* ws, int B, int H, int W, int levels);   // [B][8] at (h, w): ml_means's table
// Squeeze-excite gate of every image from the pooling sums: ch [B][C].  With dch_part ([B][dnblk][C], per-block sums of dz x) also
// its adjoint: dmP [B][C] = (gradient of the pooled mean) / P and contrib, each image's share of the gradients of se.1.weight,
// se.1.bias, se.3.weight, se.3.bias as four arrays back to back: [B][hid C], [B][hid], [B][C hid], [B][C]
int launch_pyr_se(const float* pool, int nblk, int P, const SePrm& se, float* ch, const float* dch_part, int dnblk, float* dmP, float* contrib,
                  int B, int C, hipStream_t st);

// ---- training kernels (rf_train.hip)
#ifdef __HIPCC__
// s[k] <- the sum of s[k] over a workgroup of 256 threads, in a fixed order: lanes by shuffles, then the four waves.  What a kernel
// calls before it writes its slab
template <int N>
__device__ __forceinline__ void block_sums(float (&s)[N], float* lds /* [N][4] */) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
        if ((threadIdx.x & 63) == 0) lds[k * 4 + (threadIdx.x >> 6)] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = (lds[k * 4] + lds[k * 4 + 1]) + (lds[k * 4 + 2] + lds[k * 4 + 3]);
}
#endif
// pixel slabs of a contraction over pixels with `tiles` workgroups per slab: pixels per slab a multiple of 64, about 1024
// workgroups in flight
void gram2_slabs(int B, int P, int tiles, int* slab_px, int* per_image);
size_t gram2_partial_floats(int B, int Ca, int Cb, int h, int w, int ntap);
// out[(i * ld + j) * ntap + tap] (+)= sum over images and pixels of a[i][p] b[j][p + tap shift]: the weight gradient [Ca][ld >= Cb][ntap]
// of a convolution with a = dOut and b = the layer's input
struct Gram2Launch {
    const float* a; int64_t a_bstride; int Ca;        // dOut  [B][Ca][h][w], floats between images
    const float* b; int64_t b_bstride; int Cb;        // input [B][Cb][h][w]
    const float* b2; int64_t b2_bstride; int Cb2;     // optional: the input is cat(b, b2) along channels, read in place (Cb2 = 0: none)
    float* out; int ld;
    size_t out_istride;                               // per_image: out[image * out_istride + ...]
    float* partial; size_t partial_cap;               // slab partials, floats available there (slabs x (ntap Ca Cb + Ca when db): checked)
    int B, h, w;
    int ntap;                                         // 1, or 9 = the 3x3 window in (dy, dx) row-major order
    bool per_image;                                   // no sum over images
    bool accumulate;                                  // add to out (and db)
    float* db;                                        // [Ca] (+)= row sums of a over all images and pixels: the bias gradient of the same layer; or nullptr
};
int launch_gram2(const Gram2Launch& g, hipStream_t st);
int launch_reduce_rows(const float* partial, float* out, int nrows, size_t n, int accumulate, hipStream_t st);
int chan_sum_nblk(int P);
int launch_chan_sum(const float* x, int64_t bstride, float* out, float* partial, int B, int C, int P, int accumulate, hipStream_t st);
size_t ln_bwd_partial_floats(int B, int C, int P);
bool ln_bwd_fused_shape(int C, int P);   // true: launch_ln_bwd takes a strided residual for this shape
int launch_ln_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgb, float* partial,
                  int B, int C, int P, float eps, int accumulate_dx, int accumulate_w, hipStream_t st,
                  const float* res = nullptr, int64_t res_bstride = 0);
size_t dw_wgrad_partial_floats(int B, int C, int P);
int launch_dw_wgrad(const float* x, const float* dy, float* dw, float* db, float* partial, int B, int C, int h, int w, int accumulate, hipStream_t st);
// out = a + b | a gelu'(b) (a = dy, b = x) | a (b > 0 ? 1 : slope) (a = dy, b = y) | a | clamp(a, 0, 1).  ewise_kernel takes the
// mode as a runtime argument: the values are part of what callers pass
enum EwiseMode { EW_ADD = 0, EW_GELU_GRAD = 1, EW_LRELU_GRAD = 2, EW_COPY = 5, EW_CLAMP01 = 6 };
int launch_ewise(const float* a, const float* b, float* out, size_t n, EwiseMode mode, float slope, hipStream_t st);
int launch_split_halves(const float* src, float* a, float* b, int B, int C, int P, hipStream_t st);
int loss_nblk();
int launch_loss(const float* pred, const float* gt, float* grad, float* loss_out, float* partial, size_t n, int mode, float eps, int clamp, hipStream_t st);
int launch_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, float wd, int decoupled,
                int step, float gscale, hipStream_t st);

// softmax of the forward's Gram partials and its adjoint, per (head, image): packed A and A^T, and unless fwd_only the packed M2
// with d[q;k] = M2 [q;k] and the per-image dT partials (rf_trainstep.hip, header)
struct AttnSmall {
    const float* partial; int nslab;       // Gram partials of the forward (rf_attn.hip layout, kRowW = 66)
    const float* temperature;
    const float* dA; size_t dA_istride;    // [B][C][C]
    float* m2; size_t m2_istride;          // packed [2C x 2C], zero-filled by the caller
    float* at; float* ap; size_t a_istride;   // packed A^T and A [C x C], zero-filled by the caller
    float* dT_part;                        // [B][heads]
    int C, heads, fwd_only;
};
int launch_attn_small(const AttnSmall& a, int B, hipStream_t st);

// ---- FLCA branch, backward (rf_flca_bwd.hip)
size_t flca_bwd_scratch_floats(int B, int C, int h, int w);
// partial[(b * nblk + blk) * C + c] = sum over pixel block blk of dz x: dz with dz_bstride floats between images, x [B][C][P].  nblk
// fixes the order of the sum and is the caller's (chan_sum_nblk here, pyr_dch_nblk in rf_flca_pyramid_bwd.hip)
int launch_flca_dch(const float* dz, int64_t dz_bstride, const float* x, float* partial, int nblk, int B, int C, int P, hipStream_t st);
// prm / grd: the FLCA parameters and their gradients (grd.se: four tensors adjacent in the flat gradient buffer, checked)
int launch_flca_backward(const float* feat, const float* guide, const float* xs, const float* dz, int64_t dz_bstride, const float* ch,
                         const float* pool_partial, int pool_nblk, const FlcaPrm& prm, const FlcaGrad& grd, float* dfeat, int accumulate,
                         float* scratch, size_t scratch_floats, int B, int C, int h, int w, hipStream_t st);

// ---- FLCA (rf_flca.hip)
size_t guidance_scratch_floats(int B, int H, int W);
// packed-or-mosaic input -> base planes in scratch (y, cr, cb at HxW; LL, mag at H/2 x W/2)
int launch_guidance_base(const float* in, int mosaic, int clamp_in, float* scratch, int B, int H, int W, hipStream_t st,
                         void (*allreduce)(void*, float*, size_t, int, void*) = nullptr, void* allreduce_user = nullptr);
int launch_guidance_level(const float* scratch, float* guide, int B, int H, int W, int hf, int wf, hipStream_t st);
void guidance_planes(float* scratch, int B, int H, int W, float** y, float** cr, float** cb, float** ll, float** mag);
void launch_guide_init(int* amax, int B, hipStream_t st);   // amax[0 .. B) = -inf: before the first block_max_atomic (rf_guidance.h)
struct FlcaSpatialArgs {
    const float* feat; float* xs; const float* guide;   // feat/xs [B][C][P], guide [B][4][h][w]
    const float* w_low; const float* w_high; const float* w_chr;   // [C][1][3][3], [C][1][3][3], [C][2][3][3]
    const float* alpha; const float* beta; const float* gamma;     // device scalars
    float* partial;                                      // [B][nblk][C] per-block channel sums
    int B, C, h, w, nblk;
    int ylo = 0, yhi = 0;                                // rows [ylo, yhi) enter the channel sums (yhi = 0: all); see rf_set_shard
    int xlo = 0, xhi = 0;                                // ... and columns [xlo, xhi) of them (xhi = 0: all); see rf_set_shard_grid
    void set_params(const FlcaPrm& p) {                  // (the kernels take this struct by value: its layout is theirs)
        w_low = p.w_low; w_high = p.w_high; w_chr = p.w_chr;
        alpha = p.alpha; beta = p.beta; gamma = p.gamma;
    }
};
int flca_nblk(int h, int w);
int launch_flca_spatial(const FlcaSpatialArgs& a, hipStream_t st);
// squeeze-excite gate only: ch_out[b][c]
int launch_flca_se(const float* partial, int nblk, int P, const SePrm& se, float* ch_out, int B, int C, hipStream_t st);
// x[b][c][:] *= ch[b][c]   (operator-level FLCA output; the forward folds the gate into the next 1x1 instead)
int launch_scale_channels(float* x, const float* ch, int B, int C, int P, hipStream_t st);
int launch_scale_channels_to(const float* in, float* out, const float* ch, int B, int C, int P, hipStream_t st);   // out = in * ch (in == out allowed)
// SE + fold into channel_reduce: wp_out[b] = pack([Wa * diag(ch_b) | Wb])
int launch_flca_se_fold(const float* partial, int nblk, int P, const SePrm& se, const float* w_cr, float* wp_out,
                        void* wp3_out /* b3 form too, or nullptr */, float* ch_out, int B, int C, hipStream_t st,
                        const float* composed = nullptr /* pack_tail: emit [Wa diag(ch_b) | Wb | Wb W2], in whichever of the two forms has
                                                           a pointer (wp_out then holds packed1x1_floats(2C + hc, C) per image) */,
                        int hc = 0);
// Composed stage tail (rf_model.hip run_stage): channel_reduce(cat(xs, x1 + W2 g + b2)) as ONE GEMM over [xs ; x1 ; g].
// pack_tail writes Wb W2 ([C][hc]) and the composed bias ([C]) once per parameter load; launch_tail_fold the weights, in b3 form
// (the GEMM of levels 1-3) and / or in f32 operand order (wp_out: the fused FFN kernel's tail at level 0).
size_t tail_composed_floats(int C, int hc);
int pack_tail(const float* w_cr, const float* b_cr, const float* w2, const float* b2, float* composed, int C, int hc, hipStream_t st);
int launch_tail_fold(const float* w_cr, const float* ch /* [B][C] gate or nullptr */, const float* composed, void* wp3_out, int B, int C, int hc,
                     hipStream_t st, float* wp_out = nullptr);

// ---- FFAB and WM as the WFB handle calls them (rf_ffab.hip, rf_mamba.hip): the schedules of rf_ffab / rf_wm_forward.
// prepacked: every 1x1 / 3x3 / projection weight pointer of `prm` already is the packed form (rf_pack_params), nothing is packed
// per call.  WM's three projections need both forms, so those travel in WmPacked (prm keeps the raw pointers, unused then).
size_t ffab_scratch_floats(int B, int nc, int h, int w);
int ffab_check_geometry(const char* what, int B, int nc, int h, int w);
// one nn.Conv2d(cin, cout, 1) on [B, cin, P] planes, the raw weight packed into `wpack` first (nullptr: `w` is the packed form)
int conv1x1_raw(const float* x, float* out, const float* w, const float* bias, const float* res, float* wpack, int B, int cin, int cout,
                int P, int act, hipStream_t st);
int launch_cat2(const float* a, const float* b, float* out, int B, size_t per_image, hipStream_t st);   // torch.cat((a, b), dim=1), per_image floats each
int ffab_forward(const float* in, float* out, const float* const* prm, bool prepacked, float* scratch, int B, int nc, int h, int w,
                 hipStream_t st);
struct WmPacked { const float *convb0, *convb2, *smooth, *in_proj, *x_proj, *out_proj; const void *in_proj3, *x_proj3, *out_proj3; };
int wm_workspace_floats(const char* who, int n, int c, int h, int w, size_t* floats);
int wm_forward(const float* in, float* out, const float* const* prm, const WmPacked* pk, float* ws, int n, int c, int h, int w,
               hipStream_t st);
int launch_dwgate3x3(const float* in, float* out, const float* wa, const float* ba, const float* wb, const float* bb, int B, int C, int h,
                     int w, hipStream_t st);
int launch_dwconv5x5(const float* in, float* out, const float* weight, const float* bias, int B, int C, int h, int w, hipStream_t st);

// ---- the WMB block's own kernels and pack-time folds (rf_wmb.hip)
int launch_wmb_front(const float* x, float* t, float* bands, const float* w2, const float* b2, int B, int C, int h, int w, hipStream_t st);
int launch_wmb_back(const float* bands, const float* t, float* out, int B, int C, int h, int w, hipStream_t st);
int launch_wmb_ffn_tail(const float* t, const float* y, float* out, const float* ln_w, const float* ln_b, int B, int C, int h, int w,
                        hipStream_t st);
// folds of one block, written once per parameter load: [2 w | 2 b - 1] of norm1 (2C floats); rep_conv1 + BN, rep_conv2 + BN and
// the identity as one depthwise 3x3 weight [hid][9] and bias [hid]; illu.conv1 with the channel mean folded in, [C][C] row-major
int launch_wmb_fold(const float* ln_w, const float* ln_b, float* ln2, const float* rep1_w, const float* const* bn1, const float* rep2_w,
                    const float* const* bn2, float* rep_w, float* rep_b, const float* illu_w, float* illu_fold, int C, int hid, hipStream_t st);

// ---- the adjoints of the front and back pass (rf_wmb_bwd.hip).  front: dx = the LayerNorm adjoint of g = gt + iwt_init(gb) (g is
// never stored); partial [B * wmb_front_bwd_nblk][2][C]: the slabs of d w2 and d b2 times gscale, for reduce_rows.  back:
// gbands = dwt_init(m go / 2), m the forward's clamp mask recomputed from bands
int wmb_front_bwd_nblk(int B, int C, int h, int w);
int launch_wmb_front_bwd(const float* x, const float* gt, const float* gb, const float* gamma, float* dx, float* partial, float gscale, int B, int C,
                         int h, int w, hipStream_t st);
int launch_wmb_back_bwd(const float* bands, const float* go, float* gbands, int B, int C, int h, int w, hipStream_t st);

}  // namespace rf
