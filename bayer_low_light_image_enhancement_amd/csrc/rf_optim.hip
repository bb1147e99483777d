// The guarded optimiser step (include/rawformer_hip.h, "guarded optimiser step"): what torch.cuda.amp.GradScaler.step and
// torch.nn.utils.clip_grad_norm_ do around optimizer.step() in the reference's loops (training.py:233,251-253,
// RawFomer_WFB_FFAB/train.py:139,183-190), decided ON THE DEVICE: no host read between the statistics and the update.
//
//   grad_stats_kernel          per chunk of kChunk floats of ONE segment of the flat gradient buffer: sum of g^2 and the number
//                              of non-finite elements -> partial[chunk].  Chunks never cross a segment's end, so the floats
//                              between segments (the 16-byte alignment gaps) are never read.
//   optim_control_kernel       one workgroup: the chunks of every segment added in chunk order, the segments in a fixed order;
//                              <true> also takes the decision (rf_optim_control: norm, clip coefficient, skip, step counters,
//                              the two bias corrections)
//   adam_guarded_kernel        adam_kernel (rf_train.hip) with skip, bias corrections and the gradient factor read from the
//                              control block; the gradient buffer is only read
//
// House rules of rf_train.hip: no float atomics, no tickets or fences between workgroups; partials go to memory and are added in
// an order that depends on the segment table alone (the chunk size is a constant, the grid only decides which workgroup computes
// which chunk): two runs give the same bits.  Squares and sums are float64: the square of a float32 is exact there, so a finite
// gradient cannot overflow the norm.
#include <cmath>
#include <vector>
#include "rf_common.h"

namespace rf {

namespace {

constexpr int kChunk = 4096;          // floats per chunk: 4 x 16 bytes per thread of a workgroup
constexpr int kStatsGridCap = 1024;   // workgroups of the statistics pass; more chunks than this take further grid-stride passes

struct alignas(8) OptimSeg { int chunk0, nchunks; };
struct alignas(16) OptimChunk { long long begin; int len; };      // floats [begin, begin + len) of the buffer, inside one segment
struct alignas(16) OptimPartial { double sumsq; long long nonfinite; };
static_assert(sizeof(rf_optim_control) == 80 && sizeof(rf_optim_segment) == 16 && sizeof(OptimChunk) == 16 && sizeof(OptimPartial) == 16, "device state layout");

// Device state: rf_optim_control | rf_optim_segment[nseg] | OptimSeg[nseg] | OptimChunk[max_chunks] | OptimPartial[max_chunks],
// every part on a 16-byte boundary.  max_chunks bounds sum(ceil(count_i / kChunk)) from n and nseg alone.
struct OptimLayout {
    size_t seg_result, seg_table, chunk_table, partial, total;
    int max_chunks;
};
OptimLayout optim_layout(int nseg, size_t n) {
    OptimLayout L;
    L.max_chunks = (int)(n / kChunk) + nseg;
    L.seg_result = align_up(sizeof(rf_optim_control), 16);
    L.seg_table = L.seg_result + (size_t)nseg * sizeof(rf_optim_segment);
    L.chunk_table = align_up(L.seg_table + (size_t)nseg * sizeof(OptimSeg), 16);
    L.partial = L.chunk_table + (size_t)L.max_chunks * sizeof(OptimChunk);
    L.total = L.partial + (size_t)L.max_chunks * sizeof(OptimPartial);
    return L;
}
constexpr size_t kMaxFloats = (size_t)1 << 40;     // keeps the chunk count an int with room to spare

// s, c <- their sums over the 256 threads, in a fixed order: lanes by shuffles, then the four waves (block_sums in float64)
__device__ __forceinline__ void block_sums_f64(double& s, long long& c, double* lds_s, long long* lds_c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { lds_s[threadIdx.x >> 6] = s; lds_c[threadIdx.x >> 6] = c; }
    __syncthreads();
    s = (lds_s[0] + lds_s[1]) + (lds_s[2] + lds_s[3]);
    c = (lds_c[0] + lds_c[1]) + (lds_c[2] + lds_c[3]);
    __syncthreads();           // the arrays are written again by the caller's next round
}

__device__ __forceinline__ void stat_add(float x, double& s, long long& c) {
    const double d = (double)x;
    s += d * d;
    c += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;       // exponent all ones: inf or NaN
}

// thread t of the workgroup takes elements 4 (t + 256 j) + q of its chunk, j outer, q inner: a full chunk by four 16-byte loads
// issued together, the last chunk of a segment element by element up to the segment's end
__global__ void __launch_bounds__(256) grad_stats_kernel(const float* __restrict__ g, size_t n, const rf_optim_control* __restrict__ ctl,
                                                         const OptimChunk* __restrict__ chunks, OptimPartial* __restrict__ partial, int max_chunks) {
    __shared__ double lds_s[4];
    __shared__ long long lds_c[4];
    const int nchunks = ctl->nchunks < max_chunks ? ctl->nchunks : max_chunks;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptimChunk ch = chunks[c];
        // a table that does not belong to this buffer reads nothing
        const int len = (ch.begin >= 0 && ch.len >= 0 && ch.len <= kChunk && (size_t)ch.begin + (size_t)ch.len <= n) ? ch.len : 0;
        const float* p = g + (len ? ch.begin : 0);
        double s = 0.0;
        long long k = 0;
        if (len == kChunk) {
            float4 v[kChunk / 1024];
#pragma unroll
            for (int j = 0; j < kChunk / 1024; ++j) v[j] = *reinterpret_cast<const float4*>(p + 4 * (threadIdx.x + 256 * j));
#pragma unroll
            for (int j = 0; j < kChunk / 1024; ++j) { stat_add(v[j].x, s, k); stat_add(v[j].y, s, k); stat_add(v[j].z, s, k); stat_add(v[j].w, s, k); }
        } else {
            for (int j = 0; j < kChunk / 1024; ++j)
                for (int q = 0; q < 4; ++q) {
                    const int e = 4 * ((int)threadIdx.x + 256 * j) + q;
                    if (e < len) stat_add(p[e], s, k);
                }
        }
        block_sums_f64(s, k, lds_s, lds_c);
        if (threadIdx.x == 0) { partial[c].sumsq = s; partial[c].nonfinite = k; }
    }
}

__device__ __forceinline__ double powi_f64(double b, long long k) {      // b^k by squaring
    double r = 1.0;
    for (; k > 0; k >>= 1) { if (k & 1) r *= b; b *= b; }
    return r;
}

struct ControlArgs { float grad_scale, max_norm, beta1, beta2; int skip_nonfinite; };

// One workgroup.  Thread t adds the chunk partials of segments t, t + 256, ... in chunk order and these segments in that order;
// the 256 thread sums are added by block_sums_f64.
template <bool DECIDE>
__global__ void __launch_bounds__(256) optim_control_kernel(rf_optim_control* __restrict__ ctl, const OptimSeg* __restrict__ segs,
                                                            const OptimPartial* __restrict__ partial, rf_optim_segment* __restrict__ seg_out,
                                                            int nseg, int max_chunks, ControlArgs a) {
    __shared__ double lds_s[4];
    __shared__ long long lds_c[4];
    double ts = 0.0;
    long long tk = 0;
    for (int i = threadIdx.x; i < nseg; i += 256) {
        const OptimSeg sg = segs[i];
        const bool ok = sg.chunk0 >= 0 && sg.nchunks >= 0 && sg.chunk0 <= max_chunks - sg.nchunks;
        const int c0 = ok ? sg.chunk0 : 0, c1 = ok ? sg.chunk0 + sg.nchunks : 0;
        double s = 0.0;
        long long k = 0;
#pragma unroll 8
        for (int c = c0; c < c1; ++c) { s += partial[c].sumsq; k += partial[c].nonfinite; }
        seg_out[i].sumsq = s;
        seg_out[i].nonfinite = k;
        ts += s;
        tk += k;
    }
    block_sums_f64(ts, tk, lds_s, lds_c);
    if (threadIdx.x != 0) return;
    ctl->grad_sumsq = ts;
    ctl->nonfinite = tk;
    if constexpr (DECIDE) {
        const double gn = (double)a.grad_scale * sqrt(ts);
        double coef = 1.0;
        if (a.max_norm < INFINITY) {                  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
            const double c = (double)a.max_norm / (gn + 1e-6);
            coef = c < 1.0 ? c : 1.0;                 // a NaN norm leaves the gradient as it is: nothing to rescue
        }
        const int skip = a.skip_nonfinite && tk > 0;
        ctl->grad_norm = gn;
        ctl->clip_coef = coef;
        ctl->grad_mul = (float)((double)a.grad_scale * coef);
        ctl->skip = skip;
        if (skip) {
            ctl->steps_skipped += 1;
        } else {
            const long long k = ctl->steps_applied + 1;
            ctl->steps_applied = k;
            ctl->bias_corr1 = (float)(1.0 - powi_f64((double)a.beta1, k));
            ctl->bias_corr2 = (float)(1.0 - powi_f64((double)a.beta2, k));
        }
    }
}

// adam_kernel (rf_train.hip), element for element; bc1, bc2 and the gradient factor come from the control block, and a skipped
// step leaves before anything is read or written -- the decoupled weight decay included: GradScaler.step does not call
// optimizer.step() at all.  g is const: clipping happens on the way into the update.
__global__ void __launch_bounds__(256) adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                                                           float lr, float b1, float b2, float eps, float wd, int decoupled,
                                                           const rf_optim_control* __restrict__ ctl) {
    if (ctl->skip) return;
    const float bc1 = ctl->bias_corr1, bc2 = ctl->bias_corr2, gscale = ctl->grad_mul;
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float gi = g[i] * gscale, pi = p[i];
        if (wd != 0.f) { if (decoupled) pi *= 1.0f - lr * wd; else gi = fmaf(wd, pi, gi); }
        const float mi = fmaf(b1, m[i], (1.0f - b1) * gi);
        const float vi = fmaf(b2, v[i], (1.0f - b2) * gi * gi);
        m[i] = mi; v[i] = vi;
        p[i] = pi - lr / bc1 * mi / (sqrtf(vi) / sqrtf(bc2) + eps);
    }
}

__global__ void optim_set_steps_kernel(rf_optim_control* ctl, long long steps_applied) { ctl->steps_applied = steps_applied; }

struct OptimState {
    rf_optim_control* ctl;
    rf_optim_segment* seg_result;
    OptimSeg* segs;
    OptimChunk* chunks;
    OptimPartial* partial;
    int max_chunks;
};

// the checks every entry point shares, and the parts of the state
int optim_state(const char* who, void* state, size_t state_bytes, int nseg, size_t n, OptimState* s) {
    RF_CHECK_ARG(nseg > 0, "%s: nseg = %d, need at least one segment", who, nseg);
    RF_CHECK_ARG(n > 0 && n <= kMaxFloats && (size_t)nseg <= n, "%s: n = %zu floats for %d segments", who, n, nseg);
    RF_CHECK_ARG(state && aligned16(state), "%s: null or misaligned state buffer (16 bytes)", who);
    const OptimLayout L = optim_layout(nseg, n);
    RF_CHECK_ARG(state_bytes >= L.total, "%s: state buffer of %zu bytes is too small, rf_optim_state_bytes asks for %zu", who, state_bytes, L.total);
    char* b = static_cast<char*>(state);
    s->ctl = reinterpret_cast<rf_optim_control*>(b);
    s->seg_result = reinterpret_cast<rf_optim_segment*>(b + L.seg_result);
    s->segs = reinterpret_cast<OptimSeg*>(b + L.seg_table);
    s->chunks = reinterpret_cast<OptimChunk*>(b + L.chunk_table);
    s->partial = reinterpret_cast<OptimPartial*>(b + L.partial);
    s->max_chunks = L.max_chunks;
    return RF_OK;
}

}  // namespace

}  // namespace rf

using namespace rf;

extern "C" {

int rf_optim_state_bytes(int nseg, size_t n, size_t* bytes) {
    RF_CHECK_ARG(bytes, "rf_optim_state_bytes: null result pointer");
    RF_CHECK_ARG(nseg > 0, "rf_optim_state_bytes: nseg = %d, need at least one segment", nseg);
    RF_CHECK_ARG(n > 0 && n <= kMaxFloats && (size_t)nseg <= n, "rf_optim_state_bytes: n = %zu floats for %d segments", n, nseg);
    *bytes = optim_layout(nseg, n).total;
    return RF_OK;
}

int rf_optim_init(const size_t* offsets, const size_t* counts, int nseg, size_t n, void* state, size_t state_bytes, void* stream) {
    RF_CHECK_ARG(offsets && counts, "rf_optim_init: null segment table");
    OptimState s;
    RF_TRY(optim_state("rf_optim_init", state, state_bytes, nseg, n, &s));
    size_t end = 0;
    for (int i = 0; i < nseg; ++i) {
        RF_CHECK_ARG(offsets[i] % 4 == 0, "rf_optim_init: segment %d starts at float %zu, not on a 16-byte boundary", i, offsets[i]);
        RF_CHECK_ARG(offsets[i] <= n && counts[i] <= n - offsets[i], "rf_optim_init: segment %d = [%zu, %zu + %zu) passes the buffer's %zu floats", i,
                     offsets[i], offsets[i], counts[i], n);
        RF_CHECK_ARG(offsets[i] >= end, "rf_optim_init: segment %d starts at float %zu, inside or before its predecessor (ends at %zu)", i, offsets[i], end);
        end = offsets[i] + counts[i];
    }
    // the whole state in front of the partials as one host image: zeroed control block and results, the two tables
    const OptimLayout L = optim_layout(nseg, n);
    std::vector<char> img(L.partial, 0);
    OptimSeg* segs = reinterpret_cast<OptimSeg*>(img.data() + L.seg_table);
    OptimChunk* chunks = reinterpret_cast<OptimChunk*>(img.data() + L.chunk_table);
    int nchunks = 0;
    for (int i = 0; i < nseg; ++i) {
        segs[i].chunk0 = nchunks;
        for (size_t lo = 0; lo < counts[i]; lo += kChunk) {
            const size_t len = counts[i] - lo < (size_t)kChunk ? counts[i] - lo : (size_t)kChunk;
            chunks[nchunks].begin = (long long)(offsets[i] + lo);
            chunks[nchunks].len = (int)len;
            ++nchunks;
        }
        segs[i].nchunks = nchunks - segs[i].chunk0;
    }
    rf_optim_control* ctl = reinterpret_cast<rf_optim_control*>(img.data());
    ctl->clip_coef = 1.0;
    ctl->n = (long long)n;
    ctl->nseg = nseg;
    ctl->nchunks = nchunks;
    hipStream_t st = (hipStream_t)stream;
    RF_TRY(check_hip(hipMemcpyAsync(state, img.data(), img.size(), hipMemcpyHostToDevice, st), "rf_optim_init: copy of the tables"));
    return check_hip(hipStreamSynchronize(st), "rf_optim_init");      // the host image goes away with this call
}

int rf_grad_stats(const float* grads, size_t n, int nseg, void* state, size_t state_bytes, void* stream) {
    RF_CHECK_ARG(grads && aligned16(grads), "rf_grad_stats: null or misaligned gradient buffer (16 bytes)");
    OptimState s;
    RF_TRY(optim_state("rf_grad_stats", state, state_bytes, nseg, n, &s));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope prof(st, "grad_stats_kernel", 2.0 * n, 4.0 * n);
        const int grid = s.max_chunks < kStatsGridCap ? s.max_chunks : kStatsGridCap;
        grad_stats_kernel<<<grid, 256, 0, st>>>(grads, n, s.ctl, s.chunks, s.partial, s.max_chunks);
    }
    ProfScope prof(st, "optim_control_kernel", 0.0, 16.0 * s.max_chunks);
    optim_control_kernel<false><<<1, 256, 0, st>>>(s.ctl, s.segs, s.partial, s.seg_result, nseg, s.max_chunks, ControlArgs{});
    return check_launch("rf_grad_stats");
}

int rf_adam_step_guarded(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int decoupled, float grad_scale, float max_norm, int skip_nonfinite, int nseg, void* state,
                         size_t state_bytes, void* stream) {
    RF_CHECK_ARG(params && grads && m && v, "rf_adam_step_guarded: null parameter, gradient or moment buffer");
    RF_CHECK_ARG(max_norm > 0.f, "rf_adam_step_guarded: max_norm = %g, need a positive number (+inf: no clipping)", (double)max_norm);
    OptimState s;
    RF_TRY(optim_state("rf_adam_step_guarded", state, state_bytes, nseg, n, &s));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope prof(st, "optim_control_kernel", 0.0, 16.0 * s.max_chunks);
        const ControlArgs a{grad_scale, max_norm, beta1, beta2, skip_nonfinite != 0};
        optim_control_kernel<true><<<1, 256, 0, st>>>(s.ctl, s.segs, s.partial, s.seg_result, nseg, s.max_chunks, a);
    }
    ProfScope prof(st, "adam_guarded_kernel", 12.0 * n, 28.0 * n);
    adam_guarded_kernel<<<grid1d(n), 256, 0, st>>>(params, grads, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, s.ctl);
    return check_launch("rf_adam_step_guarded");
}

int rf_optim_set_steps(void* state, size_t state_bytes, long long steps_applied, void* stream) {
    RF_CHECK_ARG(state && aligned16(state) && state_bytes >= sizeof(rf_optim_control), "rf_optim_set_steps: null, misaligned or too small state buffer");
    RF_CHECK_ARG(steps_applied >= 0, "rf_optim_set_steps: steps_applied = %lld", steps_applied);
    optim_set_steps_kernel<<<1, 1, 0, (hipStream_t)stream>>>(static_cast<rf_optim_control*>(state), steps_applied);
    return check_launch("rf_optim_set_steps");
}

}  // extern "C"
