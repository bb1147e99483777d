// Training batch assembly from a device-resident SID set (RawFomer_WFB_FFAB/load_dataset.py:53-95, load_data_SID.__getitem__):
// random crop, left-right / up-down flip, normalisation and HWC -> CHW, one pass, 8 bytes read and 16 bytes written per pixel.
//   x  = ((clip((float)raw, black, white) - black) / (float)(white - black + 1e-6)) * amp     float32, every operation rounded (:88-89)
//   gt = (float)((double)v / 65535.0)                                                         float64 quotient rounded once (:90, :93)
// The crop offsets are even (:63-64), so with an even frame width a row segment of the mosaic and its 3-halfword-per-pixel
// ground-truth segment both start on a dword: a lane owns 4 pixels = 2 dwords of raw and 6 dwords of ground truth, and stores
// one float4 into the input plane and one into each colour plane.  The flips are applied on the store index (the left-right
// flip mirrors the lane's group and the order inside it).  As in the reference the flip is of the MOSAIC, so it changes the
// CFA phase of the patch.  No LDS, no scratch.
#include "rf_common.h"

namespace rf {

constexpr int kSampleLanes = 128;       // one workgroup = a row segment of 512 pixels

struct SidSampleArgs {
    const unsigned short* raw;          // [N, H, W]
    const unsigned short* gt;           // [N, H, W, 3]
    const float* amp;                   // [N]
    const int* desc;                    // [B, 4]: frame, i, j, flips (bit 0 left-right, bit 1 up-down)
    float* x_out;                       // [B, 1, ph, pw]
    float* gt_out;                      // [B, 3, ph, pw]
    int N, H, W, ph, pw;
    float black, white, denom;
};

__device__ __forceinline__ float sid_input(unsigned v, const SidSampleArgs& a, float amp) {
    const float c = fminf(fmaxf((float)v, a.black), a.white);
    return (c - a.black) / a.denom * amp;
}
__device__ __forceinline__ float sid_truth(unsigned v) { return (float)((double)v / 65535.0); }

__global__ void __launch_bounds__(kSampleLanes) sid_sample_kernel(const SidSampleArgs a) {
    const int b = blockIdx.z, r = blockIdx.y, q = blockIdx.x * kSampleLanes + threadIdx.x, groups = a.pw / 4;
    const int f = a.desc[4 * b], i = a.desc[4 * b + 1], j = a.desc[4 * b + 2], flips = a.desc[4 * b + 3];
    // a descriptor the host wrapper would have refused: skip the patch, never read or write outside the buffers
    if (f < 0 || f >= a.N || i < 0 || j < 0 || ((i | j) & 1) || i > a.H - a.ph || j > a.W - a.pw) return;
    if (q >= groups) return;
    const size_t pix = ((size_t)f * a.H + (i + r)) * a.W + j + 4 * q;        // even: dword-aligned in both arrays
    const unsigned* rp = reinterpret_cast<const unsigned*>(a.raw + pix);
    const unsigned* gp = reinterpret_cast<const unsigned*>(a.gt + 3 * pix);
    const unsigned r0 = rp[0], r1 = rp[1];
    unsigned g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = gp[k];
    const float amp = a.amp[f];
    float x[4] = {sid_input(r0 & 0xffffu, a, amp), sid_input(r0 >> 16, a, amp), sid_input(r1 & 0xffffu, a, amp), sid_input(r1 >> 16, a, amp)};
    float t[12];                        // halfword 3 k + c = colour c of pixel k
#pragma unroll
    for (int k = 0; k < 6; ++k) { t[2 * k] = sid_truth(g[k] & 0xffffu); t[2 * k + 1] = sid_truth(g[k] >> 16); }
    const bool lr = flips & 1, ud = flips & 2;
    const int row = ud ? a.ph - 1 - r : r, grp = lr ? groups - 1 - q : q;
    const size_t plane = (size_t)a.ph * a.pw, at = (size_t)row * a.pw + 4 * grp;
    float* xo = a.x_out + (size_t)b * plane + at;
    float* go = a.gt_out + (size_t)b * 3 * plane + at;
    if (lr) {
        *reinterpret_cast<float4*>(xo) = make_float4(x[3], x[2], x[1], x[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(go + c * plane) = make_float4(t[9 + c], t[6 + c], t[3 + c], t[c]);
    } else {
        *reinterpret_cast<float4*>(xo) = make_float4(x[0], x[1], x[2], x[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(go + c * plane) = make_float4(t[c], t[3 + c], t[6 + c], t[9 + c]);
    }
}

// ---- MCR (load_data_MCR.__getitem__, RawFomer_WFB_FFAB/load_dataset.py:136-179): the same launch shape over uint8 sources, 4 bytes read
// and 16 written per pixel.
//   x  = (float)(((double)v / 255.0) * amp[f])      float64 quotient, float64 product, ONE rounding to float32 (:151); amp is float64
//   gt = (float)((double)v / 255.0)                 (:152)
// The reference normalises the frame and then crops and flips; both act per pixel, so the order does not show.
// Alignment: pix is even and not more, so a lane's 4 raw bytes and its 12 ground-truth bytes (at 3 pix) start on a HALFWORD; which
// half of a dword changes with j mod 4, with the row when W = 2 (mod 4) and with the frame when H W = 2 (mod 4).  The kernel reads
// halfwords: 2 of raw and 6 of ground truth per lane, each naturally aligned given 2-byte-aligned sources (all that the entry point
// asks of them), never a dword at a halfword address.  The compiler would fuse neighbouring halfword loads into exactly such dwords
// (gfx950 permits them), so every halfword index passes through an empty asm that hides its value (mcr_half): the loads stay
// global_load_ushort.  Every halfword read holds two bytes of the lane's own 4 pixels, and a patch that passed the guard lies
// inside its frame, so the kernel reads no byte outside the patches -- none before the first byte of `raw` / `gt`, none past
// their last -- by construction; there is no trailing load to clamp.  No LDS, no scratch.
struct McrSampleArgs {
    const unsigned short* raw;          // [N, H, W] bytes, viewed as halfwords
    const unsigned short* gt;           // [N, H, W, 3] bytes (HWC), viewed as halfwords
    const double* amp;                  // [N]
    const int* desc;                    // [B, 4]: frame, i, j, flips (bit 0 left-right, bit 1 up-down)
    float* x_out;                       // [B, 1, ph, pw]
    float* gt_out;                      // [B, 3, ph, pw]
    int N, H, W, ph, pw;
};

__device__ __forceinline__ unsigned mcr_half(const unsigned short* base, size_t k) {
    asm("" : "+v"(k));                  // the index, not the pointer: the load stays a global one
    return base[k];
}
__device__ __forceinline__ float mcr_input(unsigned v, double amp) { return (float)(((double)v / 255.0) * amp); }
__device__ __forceinline__ float mcr_truth(unsigned v) { return (float)((double)v / 255.0); }

__global__ void __launch_bounds__(kSampleLanes) mcr_sample_kernel(const McrSampleArgs a) {
    const int b = blockIdx.z, r = blockIdx.y, q = blockIdx.x * kSampleLanes + threadIdx.x, groups = a.pw / 4;
    const int f = a.desc[4 * b], i = a.desc[4 * b + 1], j = a.desc[4 * b + 2], flips = a.desc[4 * b + 3];
    // a descriptor the host wrapper would have refused: skip the patch, never read or write outside the buffers
    if (f < 0 || f >= a.N || i < 0 || j < 0 || ((i | j) & 1) || i > a.H - a.ph || j > a.W - a.pw) return;
    if (q >= groups) return;
    const size_t pix = ((size_t)f * a.H + (i + r)) * a.W + j + 4 * q;        // even: halfword-aligned in both arrays
    const size_t hw = pix / 2;                                               // halfword index in raw; 3 hw in gt
    const unsigned r0 = mcr_half(a.raw, hw), r1 = mcr_half(a.raw, hw + 1);
    unsigned g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = mcr_half(a.gt, 3 * hw + k);
    const double amp = a.amp[f];
    float x[4] = {mcr_input(r0 & 0xffu, amp), mcr_input(r0 >> 8, amp), mcr_input(r1 & 0xffu, amp), mcr_input(r1 >> 8, amp)};
    float t[12];                        // byte 3 k + c = colour c of pixel k
#pragma unroll
    for (int k = 0; k < 6; ++k) { t[2 * k] = mcr_truth(g[k] & 0xffu); t[2 * k + 1] = mcr_truth(g[k] >> 8); }
    const bool lr = flips & 1, ud = flips & 2;
    const int row = ud ? a.ph - 1 - r : r, grp = lr ? groups - 1 - q : q;
    const size_t plane = (size_t)a.ph * a.pw, at = (size_t)row * a.pw + 4 * grp;
    float* xo = a.x_out + (size_t)b * plane + at;
    float* go = a.gt_out + (size_t)b * 3 * plane + at;
    if (lr) {
        *reinterpret_cast<float4*>(xo) = make_float4(x[3], x[2], x[1], x[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(go + c * plane) = make_float4(t[9 + c], t[6 + c], t[3 + c], t[c]);
    } else {
        *reinterpret_cast<float4*>(xo) = make_float4(x[0], x[1], x[2], x[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(go + c * plane) = make_float4(t[c], t[3 + c], t[6 + c], t[9 + c]);
    }
}

}  // namespace rf

using namespace rf;

extern "C" {

int rf_sid_check_desc(const int* desc_host, int N, int H, int W, int B, int ph, int pw) {
    RF_CHECK_ARG(desc_host && N > 0 && H > 0 && W > 0 && B > 0 && ph > 0 && pw > 0, "rf_sid_check_desc: bad arguments");
    for (int b = 0; b < B; ++b) {
        const int f = desc_host[4 * b], i = desc_host[4 * b + 1], j = desc_host[4 * b + 2], flips = desc_host[4 * b + 3];
        RF_CHECK_ARG(f >= 0 && f < N, "rf_sid_check_desc: patch %d: frame index %d out of range (%d frames)", b, f, N);
        RF_CHECK_ARG(i >= 0 && j >= 0 && !((i | j) & 1), "rf_sid_check_desc: patch %d: offset (%d, %d) must be even and not negative", b, i, j);
        RF_CHECK_ARG(i <= H - ph && j <= W - pw, "rf_sid_check_desc: patch %d: %dx%d at (%d, %d) leaves the %dx%d frame", b, ph, pw, i, j, H, W);
        RF_CHECK_ARG(flips >= 0 && flips <= 3, "rf_sid_check_desc: patch %d: flips %d (bit 0 left-right, bit 1 up-down)", b, flips);
    }
    return RF_OK;
}

int rf_sid_sample(const unsigned short* raw, const unsigned short* gt, const float* amp, const int* desc, float* x_out, float* gt_out,
                  int N, int H, int W, int B, int ph, int pw, int black, int white, void* stream) {
    RF_CHECK_ARG(raw && gt && amp && desc && x_out && gt_out, "rf_sid_sample: null argument");
    RF_CHECK_ARG(N > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && ph > 0 && ph <= 65535 && pw > 0,
                 "rf_sid_sample: N = %d frames of %dx%d, B = %d patches of %dx%d", N, H, W, B, ph, pw);
    RF_CHECK_ARG(pw % 4 == 0, "rf_sid_sample: patch width %d is not a multiple of 4", pw);
    RF_CHECK_ARG(W % 2 == 0, "rf_sid_sample: frame width %d is odd", W);
    RF_CHECK_ARG(ph <= H && pw <= W, "rf_sid_sample: a %dx%d patch does not fit a %dx%d frame", ph, pw, H, W);
    RF_CHECK_ARG(white > black && black >= 0, "rf_sid_sample: white level %d <= black level %d", white, black);
    RF_CHECK_ARG((reinterpret_cast<uintptr_t>(raw) & 3) == 0 && (reinterpret_cast<uintptr_t>(gt) & 3) == 0 && aligned16(x_out) && aligned16(gt_out),
                 "rf_sid_sample: the frames must be 4-byte aligned and the outputs 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    SidSampleArgs a{raw, gt, amp, desc, x_out, gt_out, N, H, W, ph, pw, (float)black, (float)white, (float)((double)(white - black) + 1e-6)};
    const int groups = pw / 4;
    ProfScope prof(st, "sid_sample_kernel", 0.0, 24.0 * B * ph * pw);
    sid_sample_kernel<<<dim3((unsigned)((groups + kSampleLanes - 1) / kSampleLanes), (unsigned)ph, (unsigned)B), kSampleLanes, 0, st>>>(a);
    return check_launch("sid_sample");
}

int rf_mcr_sample(const unsigned char* raw, const unsigned char* gt, const double* amp, const int* desc, float* x_out, float* gt_out,
                  int N, int H, int W, int B, int ph, int pw, void* stream) {
    RF_CHECK_ARG(raw && gt && amp && desc && x_out && gt_out, "rf_mcr_sample: null argument");
    RF_CHECK_ARG(N > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && ph > 0 && ph <= 65535 && pw > 0,
                 "rf_mcr_sample: N = %d frames of %dx%d, B = %d patches of %dx%d", N, H, W, B, ph, pw);
    RF_CHECK_ARG(pw % 4 == 0, "rf_mcr_sample: patch width %d is not a multiple of 4", pw);
    RF_CHECK_ARG(W % 2 == 0, "rf_mcr_sample: frame width %d is odd", W);
    RF_CHECK_ARG(ph <= H && pw <= W, "rf_mcr_sample: a %dx%d patch does not fit a %dx%d frame", ph, pw, H, W);
    RF_CHECK_ARG((reinterpret_cast<uintptr_t>(raw) & 1) == 0 && (reinterpret_cast<uintptr_t>(gt) & 1) == 0 &&
                 (reinterpret_cast<uintptr_t>(amp) & 7) == 0 && (reinterpret_cast<uintptr_t>(desc) & 3) == 0 && aligned16(x_out) && aligned16(gt_out),
                 "rf_mcr_sample: the frames must be 2-byte aligned, amp 8-byte, the table 4-byte and the outputs 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    McrSampleArgs a{reinterpret_cast<const unsigned short*>(raw), reinterpret_cast<const unsigned short*>(gt), amp, desc, x_out, gt_out, N, H, W, ph, pw};
    const int groups = pw / 4;
    ProfScope prof(st, "mcr_sample_kernel", 0.0, 20.0 * B * ph * pw);
    mcr_sample_kernel<<<dim3((unsigned)((groups + kSampleLanes - 1) / kSampleLanes), (unsigned)ph, (unsigned)B), kSampleLanes, 0, st>>>(a);
    return check_launch("mcr_sample");
}

}  // extern "C"
