// C-ABI operator entry points (include/rawformer_hip.h) and error plumbing.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "rf_common.h"

namespace rf {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return RF_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return RF_E_DEVICE;
}

int check_launch(const char* what) { return check_hip(hipGetLastError(), what); }

// ---- per-launch event profiler (single-threaded diagnostic; off by default)
struct ProfRec {
    std::string key;
    double flops, bytes;
    hipEvent_t e0, e1;
};
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;

ProfScope::ProfScope(hipStream_t st, const char* key, double flops, double bytes) : st_(st), rec_(-1) {
    if (!g_prof_on) return;
    ProfRec r;
    r.key = key;
    r.flops = flops;
    r.bytes = bytes;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
    (void)hipEventRecord(r.e0, st);
    rec_ = (int)g_prof.size();
    g_prof.push_back(r);
}

bool profiling_active() { return g_prof_on; }

ProfScope::~ProfScope() {
    if (rec_ >= 0) (void)hipEventRecord(g_prof[rec_].e1, st_);
}

static const float kHaarInit[16] = {   // dwt_init / iwt_init, taps t = 2*row + col, bands LL,HL,LH,HH
    0.5f, 0.5f, 0.5f, 0.5f, -0.5f, 0.5f, -0.5f, 0.5f, -0.5f, -0.5f, 0.5f, 0.5f, 0.5f, -0.5f, -0.5f, 0.5f};
static const float kHaarOrtho[16] = {  // HaarDWT, bands LL,LH,HL,HH
    0.5f, 0.5f, 0.5f, 0.5f, 0.5f, -0.5f, 0.5f, -0.5f, 0.5f, 0.5f, -0.5f, -0.5f, 0.5f, -0.5f, -0.5f, 0.5f};

}  // namespace rf

using namespace rf;

extern "C" {

const char* rf_last_error(void) { return g_err; }
int rf_version(void) { return 1; }

int rf_profile_begin(void) {
    for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_prof.clear();
    g_prof_on = true;
    return RF_OK;
}

int rf_profile_end(char* json, size_t len) {
    g_prof_on = false;
    struct Agg { long n = 0; double ms = 0, flops = 0, bytes = 0; };
    std::map<std::string, Agg> agg;
    int rc = RF_OK;
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) rc = RF_E_DEVICE;
        Agg& a = agg[r.key];
        a.n += 1; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_prof.clear();
    if (rc) { set_error("rf_profile_end: event timing failed"); return rc; }
    std::string out = "[";
    bool first = true;
    for (auto& kv : agg) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s{\"kernel\": \"%s\", \"launches\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.flops, kv.second.bytes);
        out += buf;
        first = false;
    }
    out += "]";
    RF_CHECK_ARG(json && out.size() + 1 <= len, "rf_profile_end: buffer of %zu bytes too small (need %zu)", len, out.size() + 1);
    memcpy(json, out.c_str(), out.size() + 1);
    return RF_OK;
}

int rf_pixel_unshuffle2(const float* in, float* out, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && B > 0 && C > 0 && h > 0 && w > 0, "pixel_unshuffle2: bad arguments");
    return launch_pixel_unshuffle2(in, out, B, C, h, w, (hipStream_t)stream);
}

int rf_pixel_shuffle2(const float* in, float* out, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && B > 0 && C > 0 && h > 0 && w > 0, "pixel_shuffle2: bad arguments");
    return launch_pixel_shuffle2(in, out, B, C, h, w, (hipStream_t)stream);
}

int rf_dwt_haar(const float* in, float* out, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && B > 0 && C > 0 && h > 0 && w > 0, "dwt_haar: bad arguments");
    return launch_dwt2x2(in, out, kHaarInit, 0, 1, B, C, h, w, 2 * h, 2 * w, (hipStream_t)stream);
}

int rf_idwt_haar(const float* in, float* out, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && B > 0 && C > 0 && h > 0 && w > 0, "idwt_haar: bad arguments");
    return launch_idwt2x2(in, out, kHaarInit, 0, 1, B, C, h, w, (hipStream_t)stream);
}

static void scaled_kernel(const float* k16, int norm, float out[16]) {
    for (int i = 0; i < 16; ++i) out[i] = norm ? k16[i] / 2.0f : k16[i];
}

int rf_dwt_custom(const float* in, float* out, const float* k16, int norm, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && k16 && B > 0 && C > 0 && h > 0 && w > 0, "dwt_custom: bad arguments");
    float k[16];
    scaled_kernel(k16, norm, k);
    return launch_dwt2x2(in, out, k, 1, 0, B, C, h, w, 2 * h, 2 * w, (hipStream_t)stream);
}

int rf_idwt_custom(const float* in, float* out, const float* k16, int norm, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && k16 && B > 0 && C > 0 && h > 0 && w > 0, "idwt_custom: bad arguments");
    float k[16];
    scaled_kernel(k16, norm, k);
    return launch_idwt2x2(in, out, k, 1, 0, B, C, h, w, (hipStream_t)stream);
}

int rf_haar_dwt(const float* in, float* out, int B, int C, int hin, int win, void* stream) {
    RF_CHECK_ARG(in && out && B > 0 && C > 0 && hin > 1 && win > 1, "haar_dwt: bad arguments");
    return launch_dwt2x2(in, out, kHaarOrtho, 0, 0, B, C, (hin + 1) / 2, (win + 1) / 2, hin, win, (hipStream_t)stream);
}

int rf_layernorm2d(const float* in, float* out, const float* weight, const float* bias, float eps,
                   int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && weight && B > 0 && C > 0 && h > 0 && w > 0, "layernorm2d: bad arguments");
    return launch_layernorm2d(in, out, weight, bias, eps, B, C, h * w, (hipStream_t)stream);
}

int rf_conv1x1_scratch_bytes(int Cin_total, int Cout, size_t* bytes) {
    RF_CHECK_ARG(bytes && Cin_total > 0 && Cout > 0, "conv1x1_scratch_bytes: bad arguments");
    *bytes = (align_up(packed1x1_floats(Cin_total, Cout), 64) + packed1x1_b3_floats(Cin_total, Cout)) * sizeof(float);
    return RF_OK;
}

int rf_conv1x1_group_grid(int units, int ngroups, int* ids) {
    RF_CHECK_ARG(ids && units > 0 && ngroups > 0 && (long)units * ngroups < (1L << 30), "conv1x1_group_grid: bad arguments");
    *ids = (int)conv1x1_group_grid((unsigned)units, (unsigned)ngroups);
    return RF_OK;
}

int rf_conv1x1_group_map(int units, int ngroups, int id, int* unit, int* group) {
    RF_CHECK_ARG(unit && group && units > 0 && ngroups > 0 && (long)units * ngroups < (1L << 30) && id >= 0 &&
                 (unsigned)id < conv1x1_group_grid((unsigned)units, (unsigned)ngroups), "conv1x1_group_map: bad arguments");
    unsigned u, g;
    const bool ok = conv1x1_group_map((unsigned)id, (unsigned)units, (unsigned)ngroups, &u, &g);
    *unit = ok ? (int)u : -1;
    *group = ok ? (int)g : -1;
    return RF_OK;
}

// the GEMM of rf_conv1x1 on packed weights wp / wp3
static Conv1x1Args conv1x1_api_args(const float* in, const float* in2, float* out, const float* wp, const void* wp3, const float* bias,
                                    const float* ln_w, const float* ln_b, const float* res, int B, int C1, int C2, int Cout, int h, int w) {
    Conv1x1Args a{};
    a.x1 = in; a.C1 = C1; a.x1_bstride = (int64_t)C1 * h * w;
    a.x2 = C2 ? in2 : nullptr; a.C2 = C2; a.x2_bstride = (int64_t)C2 * h * w;
    a.wp = wp; a.wp3 = wp3; a.bias = bias; a.ln_w = ln_w; a.ln_b = ln_b; a.ln_eps = 1e-5f;
    a.res = res; a.res_bstride = (int64_t)Cout * h * w;
    a.out = out; a.out_bstride = (int64_t)Cout * h * w; a.Cout = Cout; a.B = B; a.P = h * w; a.w = w;
    return a;
}

int rf_conv1x1(const float* in, const float* in2, float* out, const float* weight, const float* bias,
               const float* ln_w, const float* ln_b, const float* res, void* scratch,
               int B, int C1, int C2, int Cout, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && weight && scratch && aligned16(scratch), "conv1x1: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int K = C1 + C2;
    RF_TRY(pack_1x1(weight, (float*)scratch, Cout, K, K, 1, st));
    float* w3 = (float*)scratch + align_up(packed1x1_floats(K, Cout), 64);
    RF_TRY(pack_1x1_b3(weight, w3, Cout, K, K, 1, st));
    return launch_conv1x1(conv1x1_api_args(in, in2, out, (const float*)scratch, w3, bias, ln_w, ln_b, res, B, C1, C2, Cout, h, w), st);
}

int rf_dwconv3x3(const float* in, float* out, const float* weight, const float* bias, int gelu,
                 int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && weight && B > 0 && C > 0 && h > 0 && w > 0, "dwconv3x3: bad arguments");
    DwConvArgs a{};
    a.x = in; a.x_bstride = (int64_t)C * h * w; a.out = out; a.out_bstride = (int64_t)C * h * w;
    a.w = weight; a.bias = bias; a.B = B; a.C = C; a.h = h; a.w_ = w; a.gelu = gelu;
    return launch_dwconv3x3(a, (hipStream_t)stream);
}

int rf_conv3x3_scratch_bytes(int Cin, int Cout, size_t* bytes) {
    RF_CHECK_ARG(bytes && Cin > 0 && Cout > 0, "conv3x3_scratch_bytes: bad arguments");
    *bytes = packed3x3_floats(Cin, Cout) * sizeof(float);
    return RF_OK;
}

int rf_conv3x3(const float* in, float* out, const float* weight, const float* bias, void* scratch,
               int act, int store, int B, int Cin, int Cout, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && weight && scratch && aligned16(scratch), "conv3x3: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    RF_TRY(pack_3x3(weight, (float*)scratch, Cout, Cin, st));
    Conv3x3Args a{};
    a.x = in; a.x_bstride = (int64_t)Cin * h * w; a.wp = (const float*)scratch; a.bias = bias;
    a.out = out; a.out_bstride = (int64_t)Cout * h * w; a.B = B; a.Cin = Cin; a.Cout = Cout; a.h = h; a.w = w;
    a.act = act; a.store = store;
    return launch_conv3x3(a, st);
}

int rf_conv3x3_plan(int B, int Cin, int Cout, int h, int w, int store, int unshuffle_in, int aligned, size_t ks_floats,
                    char* key, size_t key_len, int* grid, int* block, int* ksplit, int* level0) {
    RF_CHECK_ARG(key && key_len > 0 && grid && block && ksplit && level0, "conv3x3_plan: bad arguments");
    alignas(16) static float any[8];      // stands for every operand: a plan looks at presence and alignment only
    float* buf = aligned ? any : any + 1;
    Conv3x3Args a = conv3x3_dense(buf, any, any, buf, B, Cin, Cout, h, w, 0);
    a.store = store; a.unshuffle_in = unshuffle_in;
    a.ks_scratch = ks_floats ? buf : nullptr; a.ks_floats = ks_floats;
    Conv3x3Plan p;
    RF_TRY(plan_conv3x3(a, &p));
    snprintf(key, key_len, "%s", p.key);
    grid[0] = (int)p.grid.x; grid[1] = (int)p.grid.y; grid[2] = (int)p.grid.z;
    *block = (int)p.block;
    *ksplit = p.ksplit;
    *level0 = p.l0 != 0;
    return RF_OK;
}

int rf_convT2x2_scratch_bytes(int Cin, int Cout, size_t* bytes) {
    RF_CHECK_ARG(bytes && Cin > 0 && Cout > 0, "convT2x2_scratch_bytes: bad arguments");
    *bytes = packed1x1_floats(Cin, 4 * Cout) * sizeof(float);
    return RF_OK;
}

// the GEMM of rf_convT2x2 on packed weights wp
static Conv1x1Args convT2x2_api_args(const float* in, float* out, const float* wp, const float* bias, int B, int Cin, int Cout, int h, int w) {
    Conv1x1Args a{};
    a.x1 = in; a.C1 = Cin; a.x1_bstride = (int64_t)Cin * h * w; a.wp = wp; a.bias = bias;
    a.out = out; a.out_bstride = (int64_t)Cout * 4 * h * w; a.Cout = 4 * Cout; a.B = B; a.P = h * w; a.w = w; a.mode = 1;
    return a;
}

int rf_convT2x2(const float* in, float* out, const float* weight, const float* bias, void* scratch,
                int B, int Cin, int Cout, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && weight && scratch && aligned16(scratch), "convT2x2: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    RF_TRY(pack_convT(weight, (float*)scratch, Cin, Cout, st));
    return launch_conv1x1(convT2x2_api_args(in, out, (const float*)scratch, bias, B, Cin, Cout, h, w), st);
}

int rf_conv1x1_plan(int B, int C1, int C2, int Cout, int h, int w, int ln, int res, int transposed, int b3_weights,
                    char* key, size_t key_len, int* grid, int* block, size_t* lds_bytes, int* ln_single_pass) {
    RF_CHECK_ARG(key && key_len > 0 && grid && block && lds_bytes && ln_single_pass, "conv1x1_plan: bad arguments");
    RF_CHECK_ARG(!transposed || (!ln && !res && C2 == 0 && !b3_weights), "conv1x1_plan: rf_convT2x2 has one source, no LayerNorm, no residual and no b3 weights");
    alignas(16) static float any[4];      // stands for every operand: a plan looks at presence and alignment only
    const Conv1x1Args a = transposed ? convT2x2_api_args(any, any, any, any, B, C1, Cout, h, w)
                                     : conv1x1_api_args(any, any, any, any, b3_weights ? any : nullptr, any, ln ? any : nullptr, ln ? any : nullptr,
                                                        res ? any : nullptr, B, C1, C2, Cout, h, w);
    Conv1x1Plan p;
    RF_TRY(plan_conv1x1(a, &p));
    snprintf(key, key_len, "%s", p.key);
    grid[0] = (int)p.grid[0]; grid[1] = (int)p.grid[1]; grid[2] = (int)p.grid[2];
    *block = (int)p.block;
    *lds_bytes = p.lds;
    *ln_single_pass = p.ln_single_pass;
    return RF_OK;
}

int rf_conv1x1_dw3_plan(int B, int C, int hc, int h, int w, char* key, size_t key_len, int* grid, int* block, int* on_the_fly) {
    RF_CHECK_ARG(key && key_len > 0 && grid && block && on_the_fly && C > 0 && hc > 0 && h > 0 && w > 0, "conv1x1_dw3_plan: bad arguments");
    alignas(16) static float any[4];      // stands for every operand: a plan looks at presence and alignment only
    Conv1x1Args a = conv1x1_api_args(any, any, any, nullptr, any, any, nullptr, nullptr, nullptr, B, C, C, C, h, w);
    a.x3 = any; a.C3 = hc; a.x3_bstride = (int64_t)hc * h * w;
    const Conv1x1Dw3 d{any, any, h, w};
    Conv1x1Plan p;
    RF_TRY(plan_conv1x1(a, &p, &d));
    snprintf(key, key_len, "%s", p.key);
    grid[0] = (int)p.grid[0]; grid[1] = (int)p.grid[1]; grid[2] = (int)p.grid[2];
    *block = (int)p.block;
    *on_the_fly = p.dw3;
    return RF_OK;
}

int rf_fft_plan(int planes, int h, int w, int out[10]) {
    RF_CHECK_ARG(out, "fft_plan: bad arguments");
    FftPlan p;
    RF_TRY(plan_fft("fft_plan", planes, h, w, &p));
    const int plan[10] = {p.log2w, p.log2h, p.L, p.TC, (int)p.gx, (int)p.gy, cdiv(cdiv(p.rows, p.L), (int)p.gx), cdiv(p.units, (int)p.gy),
                          (int)p.lds_rows, (int)p.lds_cols};
    for (int i = 0; i < 10; ++i) out[i] = plan[i];
    return RF_OK;
}

// scratch layout of rf_chan_attn: packed qkv weights | qkv_pre | qkv | gram partials | folded weights
struct AttnScratch {
    size_t wqkv, wqkv3, pre, qkv, partial, wfold, wfold3, total;
};
static int attn_scratch(int B, int C, int heads, int h, int w, AttnScratch* s) {
    const int P = h * w;
    int ns, sl;
    size_t pf;
    RF_TRY(gram_plan(B, C, heads, P, &ns, &sl, &pf));
    if (attn_mid_supported(C, heads, h, w)) {
        size_t pf2;
        attn_mid_plan(h, w, &ns, &pf2, B, C);
        if (pf2 > pf) pf = pf2;
    }
    Bump b;
    s->wqkv = b.off(packed1x1_floats(C, 3 * C));
    s->wqkv3 = b.off(packed1x1_b3_floats(C, 3 * C));
    s->pre = b.off((size_t)B * 3 * C * P);
    s->qkv = b.off((size_t)B * 3 * C * P);
    s->partial = b.off(pf);
    s->wfold = b.off((size_t)B * packed1x1_floats(C, C));
    s->wfold3 = b.off((size_t)B * packed1x1_b3_floats(C, C));
    s->total = b.used;
    return RF_OK;
}

int rf_chan_attn_scratch_bytes(int B, int C, int heads, int h, int w, size_t* bytes) {
    RF_CHECK_ARG(bytes && B > 0 && C > 0 && heads > 0 && h > 0 && w > 0, "chan_attn_scratch_bytes: bad arguments");
    AttnScratch s;
    RF_TRY(attn_scratch(B, C, heads, h, w, &s));
    *bytes = s.total * sizeof(float);
    return RF_OK;
}

int rf_chan_attn(const float* in, float* out, const float* qkv_w, const float* qkv_b,
                 const float* dw_w, const float* dw_b, const float* temperature,
                 const float* proj_w, const float* proj_b, void* scratch,
                 int B, int C, int heads, int h, int w, void* stream) {
    RF_CHECK_ARG(in && out && qkv_w && dw_w && temperature && proj_w && scratch && aligned16(scratch), "chan_attn: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    AttnScratch s;
    RF_TRY(attn_scratch(B, C, heads, h, w, &s));      // gram_plan's checks of the head layout
    // launch_attn_fold's and launch_gram's own checks, made here as well: they run after the qkv GEMM and the depthwise filter
    RF_CHECK_ARG(B > 0 && B <= 65535 && h > 0 && w > 0 && C % 4 == 0, "chan_attn: unsupported shape B=%d C=%d heads=%d %dx%d", B, C, heads, h, w);
    float* ws = (float*)scratch;
    RF_TRY(pack_1x1(qkv_w, ws + s.wqkv, 3 * C, C, C, 1, st));
    RF_TRY(pack_1x1_b3(qkv_w, ws + s.wqkv3, 3 * C, C, C, 1, st));
    // the block's attention schedule (rf_block.hip) without its LayerNorm and residual
    TbParams p{};
    p.qkv_wp = ws + s.wqkv; p.qkv_wp3 = ws + s.wqkv3; p.qkv_b = qkv_b; p.qkv_dw_w = dw_w; p.qkv_dw_b = dw_b;
    p.temperature = temperature; p.proj_w = proj_w; p.proj_b = proj_b;
    return run_chan_attn(p, in, out, false, AttnBufs{ws + s.pre, ws + s.qkv, ws + s.partial, ws + s.wfold, ws + s.wfold3}, B, C, heads, h, w, st);
}

// scratch layout of rf_transformer_block: packed qkv | packed pw1 | packed pw2 | run_transformer buffers
struct TbScratch { size_t wqkv, w1, w2, wqkv3, w13, w23, bufs, total; TbBufOffsets o; };
static void tb_scratch(int B, int C, int heads, int hc, int h, int w, TbScratch* s) {
    Bump b;
    s->wqkv = b.off(packed1x1_floats(C, 3 * C));
    s->w1 = b.off(packed1x1_floats(C, hc));
    s->w2 = b.off(packed1x1_floats(hc, C));
    s->wqkv3 = b.off(packed1x1_b3_floats(C, 3 * C));
    s->w13 = b.off(packed1x1_b3_floats(C, hc));
    s->w23 = b.off(packed1x1_b3_floats(hc, C));
    s->bufs = b.used;
    s->total = b.used + transformer_scratch_floats(B, C, heads, hc, h, w, &s->o);
}

int rf_attn_front_plan(int B, int C, int heads, int h, int w, long long out[4]) {
    RF_CHECK_ARG(out && B > 0 && heads > 0 && h > 0 && w > 0, "attn_front_plan: bad arguments");
    RF_CHECK_ARG(fused_attn_supported(C, heads, h, w), "attn_front_plan: attn_front does not run at C=%d heads=%d %dx%d", C, heads, h, w);
    int nslab = 0, tall = 0;
    size_t pf = 0, reserve = 0;
    RF_TRY(fused_attn_plan(h, w, &nslab, &pf, B, C, &tall, &reserve));
    out[0] = tall; out[1] = nslab; out[2] = (long long)pf; out[3] = (long long)reserve;
    return RF_OK;
}

int rf_transformer_block_scratch_bytes(int B, int C, int heads, int ffn_expansion, int h, int w, size_t* bytes) {
    RF_CHECK_ARG(bytes && B > 0 && C > 0 && heads > 0 && C % heads == 0 && ffn_expansion > 0 && h > 0 && w > 0, "transformer_block_scratch_bytes: bad arguments");
    { int ns, sl; size_t pf; RF_TRY(gram_plan(B, C, heads, h * w, &ns, &sl, &pf)); }
    TbScratch s;
    tb_scratch(B, C, heads, C * ffn_expansion, h, w, &s);
    *bytes = s.total * sizeof(float);
    return RF_OK;
}

int rf_transformer_block(const float* in, float* out, const float* const* prm, void* scratch,
                         int B, int C, int heads, int ffn_expansion, int h, int w, void* stream) {
    return rf_transformer_block_window(in, out, prm, scratch, B, C, heads, ffn_expansion, h, w, 0, 0, 0, 0, stream);
}

int rf_transformer_block_window(const float* in, float* out, const float* const* prm, void* scratch,
                                int B, int C, int heads, int ffn_expansion, int h, int w, int y_lo, int y_hi, int x_lo, int x_hi, void* stream) {
    RF_CHECK_ARG(in && out && prm && scratch && aligned16(scratch), "transformer_block: bad arguments");
    RF_CHECK_ARG((y_hi == 0 && y_lo == 0) || (0 <= y_lo && y_lo < y_hi && y_hi <= h), "transformer_block: interior rows [%d, %d) of %d", y_lo, y_hi, h);
    RF_CHECK_ARG((x_hi == 0 && x_lo == 0) || (y_hi > 0 && 0 <= x_lo && x_lo < x_hi && x_hi <= w && x_lo % 4 == 0 && (x_hi % 4 == 0 || x_hi == w)),
                 "transformer_block: interior columns [%d, %d) of %d: whole groups of 4, and interior rows with them", x_lo, x_hi, w);
    RF_CHECK_ARG(B > 0 && C % 4 == 0 && heads > 0 && C % heads == 0 && C / heads <= 64, "transformer_block: unsupported C=%d heads=%d", C, heads);
    for (int i = 0; i < 17; ++i) RF_CHECK_ARG(prm[i] != nullptr, "transformer_block: parameter %d is null", i);
    hipStream_t st = (hipStream_t)stream;
    const int hc = C * ffn_expansion;
    { int ns, sl; size_t pf; RF_TRY(gram_plan(B, C, heads, h * w, &ns, &sl, &pf)); }
    TbScratch s;
    tb_scratch(B, C, heads, hc, h, w, &s);
    float* ws = (float*)scratch;
    // prm, in state_dict order; the three GEMM weights enter packed
    TbParams p{};
    p.ln1_w = prm[0]; p.ln1_b = prm[1]; p.temperature = prm[2];
    const float* qkv_w = prm[3]; p.qkv_b = prm[4]; p.qkv_dw_w = prm[5]; p.qkv_dw_b = prm[6]; p.proj_w = prm[7]; p.proj_b = prm[8];
    p.ln2_w = prm[9]; p.ln2_b = prm[10];
    const float* pw1_w = prm[11]; p.pw1_b = prm[12]; p.dw_w = prm[13]; p.dw_b = prm[14];
    const float* pw2_w = prm[15]; p.pw2_b = prm[16];
    p.qkv_wp = ws + s.wqkv; p.pw1_wp = ws + s.w1; p.pw2_wp = ws + s.w2;
    p.qkv_wp3 = ws + s.wqkv3; p.pw1_wp3 = ws + s.w13; p.pw2_wp3 = ws + s.w23;
    RF_TRY(pack_1x1(qkv_w, ws + s.wqkv, 3 * C, C, C, 1, st));
    RF_TRY(pack_1x1(pw1_w, ws + s.w1, hc, C, C, 1, st));
    RF_TRY(pack_1x1(pw2_w, ws + s.w2, C, hc, hc, 1, st));
    RF_TRY(pack_1x1_b3(qkv_w, ws + s.wqkv3, 3 * C, C, C, 1, st));
    RF_TRY(pack_1x1_b3(pw1_w, ws + s.w13, hc, C, C, 1, st));
    RF_TRY(pack_1x1_b3(pw2_w, ws + s.w23, C, hc, hc, 1, st));
    p.ylo = y_lo; p.yhi = y_hi; p.xlo = x_lo; p.xhi = x_hi;
    return run_transformer(p, in, out, ws + s.bufs, s.o, B, C, heads, hc, h, w, st);
}

// scratch layout of rf_flca: per-block channel sums | the gate [B][C]
struct FlcaScratch { float *partial, *ch; size_t total; };
static FlcaScratch flca_scratch(float* base, int B, int C, int h, int w) {
    Bump b{base};
    FlcaScratch s;
    s.partial = b.take((size_t)B * flca_nblk(h, w) * C);
    s.ch = b.take((size_t)B * C);
    s.total = b.used;
    return s;
}

int rf_flca_scratch_bytes(int B, int C, int h, int w, size_t* bytes) {
    RF_CHECK_ARG(bytes && B > 0 && C > 0 && h > 0 && w > 0, "flca_scratch_bytes: bad arguments");
    *bytes = flca_scratch(nullptr, B, C, h, w).total * sizeof(float);
    return RF_OK;
}

int rf_flca(const float* feat, const float* guide, float* out, const float* const* prm, void* scratch,
            int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(feat && guide && out && prm && scratch && aligned16(scratch), "flca: bad arguments");
    for (int i = 0; i < 10; ++i) RF_CHECK_ARG(prm[i] != nullptr, "flca: parameter %d is null", i);
    // launch_flca_se's own check, made here as well: it runs after the spatial kernel, which would have written `out` by then
    RF_CHECK_ARG(B > 0 && B <= 65535 && h > 0 && w > 0 && C > 0 && C <= 512 && C % 8 == 0 && flca_hidden(C) <= 64,
                 "flca: unsupported shape B=%d C=%d %dx%d", B, C, h, w);
    hipStream_t st = (hipStream_t)stream;
    const FlcaPrm p{prm[0], prm[1], prm[2], prm[3], prm[4], prm[5], {prm[6], prm[7], prm[8], prm[9]}};   // state_dict order = FlcaGroup's
    const FlcaScratch s = flca_scratch((float*)scratch, B, C, h, w);
    FlcaSpatialArgs a{};
    a.feat = feat; a.xs = out; a.guide = guide;
    a.set_params(p);
    a.partial = s.partial; a.B = B; a.C = C; a.h = h; a.w = w; a.nblk = flca_nblk(h, w);
    RF_TRY(launch_flca_spatial(a, st));
    RF_TRY(launch_flca_se(s.partial, a.nblk, h * w, p.se, s.ch, B, C, st));
    return launch_scale_channels(out, s.ch, B, C, h * w, st);
}

int rf_guidance_scratch_bytes(int B, int H, int W, size_t* bytes) {
    RF_CHECK_ARG(bytes && B > 0 && H > 0 && W > 0, "guidance_scratch_bytes: bad arguments");
    *bytes = guidance_scratch_floats(B, H, W) * sizeof(float);
    return RF_OK;
}

int rf_flca_guidance(const float* packed, float* guide, void* scratch, int B, int H, int W, int hf, int wf, void* stream) {
    RF_CHECK_ARG(packed && guide && scratch && hf > 0 && wf > 0, "flca_guidance: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    RF_TRY(launch_guidance_base(packed, 0, 0, (float*)scratch, B, H, W, st));
    return launch_guidance_level((const float*)scratch, guide, B, H, W, hf, wf, st);
}

int rf_upcat_scratch_bytes(int C, size_t* bytes) {
    RF_CHECK_ARG(bytes && C > 0 && C % 4 == 0, "upcat_scratch_bytes: bad arguments");
    *bytes = upcat_packed_floats(C) * sizeof(float);
    return RF_OK;
}

int rf_upcat(const float* x, const float* skip, float* out, const float* up_w, const float* up_b, const float* cr_w, const float* cr_b,
             void* scratch, int B, int C, int h, int w, void* stream) {
    RF_CHECK_ARG(x && skip && out && up_w && cr_w && scratch && aligned16(scratch), "upcat: bad arguments");
    // launch_upcat's own check, made here as well: an unsupported shape is refused before pack_upcat launches anything
    RF_CHECK_ARG(upcat_supported(C, h, w, x, skip, out) && B > 0 && B <= 65535, "upcat: unsupported shape C=%d %dx%d", C, h, w);
    hipStream_t st = (hipStream_t)stream;
    RF_TRY(pack_upcat(up_w, up_b, cr_w, cr_b, (float*)scratch, C, st));
    return launch_upcat(x, skip, out, (const float*)scratch, B, C, h, w, st);
}
}  // extern "C"
