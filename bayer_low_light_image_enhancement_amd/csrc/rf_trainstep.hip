// Training step of RawFormer (SURVEY.md section 8 f3 / BASELINE configs[4]; reference: train.py:127-147 -- forward, loss,
// backward -- with torch.autograd replaced by an explicit adjoint schedule).  rf_train_step = forward with the activations
// the backward needs kept in the workspace, L1 / Charbonnier loss, backward; the gradient of every parameter lands in ONE
// flat buffer (rf_flat_offset) that the host all-reduces across ranks (RCCL) and hands to rf_adam_step together with the flat
// parameter buffer.  Host code only: kernels in rf_train.hip and the forward files.
//
// The forward here is the op-by-op schedule (the fused level-0 kernels keep their intermediates on chip, which is exactly what a
// backward pass cannot use).  Adjoints:
//   1x1 conv          dX = conv1x1(dY, W^T)                         dW = gram2(dY, X)          db = channel sums of dY
//   3x3 conv          dX = conv3x3(dY, W^T with flipped taps)       dW = gram2<9 taps>(dY, X)
//   depthwise 3x3     dX = dwconv(dY, flipped taps)                 dW, db = dw_wgrad
//   ConvTranspose2d   dX = conv1x1(unshuffle(dY), W as [Cin][4 Cout])   dW = gram2(X, unshuffle(dY))
//   PixelShuffle / downshuffle: each other's adjoint;  LayerNorm, GELU, LeakyReLU: rf_train.hip
//   channel attention (q^ k^T T -> softmax -> A v -> project_out), per image and head, with G = q k^T, rq = 1/|q|, rk = 1/|k|,
//   c = rq G rk (cosines), S = T c, A = softmax(S), o = A v:
//       do = W_out^T dOut;  dW_out = gram2(dOut, o);  dA = gram2(do, v) per image;  dv = A^T do;
//       dS = A (dA - rowsum(dA A));  dT = sum dS c;  dc = T dS;
//       dq = (rq dc rk) k - diag(rq^2 rowsum(dc c)) q;     dk = (rq dc rk)^T q - diag(rk^2 colsum(dc c)) k
//     i.e. d[q;k] = M2 [q;k] with a per-image 2C x 2C matrix and dv = blockdiag(A^T) do: two 1x1 GEMMs with per-image weights.
// Variants 'plain' (conv branch) and 'flca' (rf_flca_bwd.hip: launch_flca_backward).
//
// Schedule-level choices (round 3): every packed / transposed / tap-flipped weight form of the step is written by three batched
// launches before the forward (pack cache, laid out once by plan_training); bias gradients are row sums inside gram2; the depthwise 3x3 of the
// FFN writes its pre-activation and GELU(.) in one pass; the halves of a concatenated-input gradient are read in place through
// strides; both residual adds of a block ride on the LayerNorm adjoints; inside a stage every backward tensor has its own
// buffer so that the weight-gradient kernels run on a second stream beside the dX chain (fork before each, join at the end of
// the stage); finished ranges of the flat gradient buffer are announced to the caller (rf_set_grad_ready) from its end towards
// its start so that the gradient all-reduce overlaps the rest of the backward.
//
// Every tensor is reached through the handle's index table (rf_handle.h): raw pointers by registry index, packed forms at the
// offsets plan_training fixed at rf_create, gradients at the parameter's flat offset.
#include <vector>
#include "rf_handle.h"
#include "rf_grad.h"

using namespace rf;

namespace {

struct Stash {      // one Conv_Transformer stage
    const float* in;
    float *qkvp, *qkv, *partial, *x1, *f1, *f2, *g, *trans, *xs, *cr, *out;      // g = GELU(f2), written by the same kernel as f2
    float *xraw, *ch, *pool;           // FLCA: xs before the squeeze-excite gate, the gate [B][C], the pooling partial sums
    int nslab, slab;
};

struct TrainPlan {
    Stash st[8];                       // 1..7
    float *x4, *e, *down[3], *up[3], *catr[3], *pred;
    float *gscratch, *guide[4], *flca_scr;
    size_t flca_scr_floats;
    float *tA, *tB, *tC, *tD, *tE;     // backward temporaries (3 * U0 each)
    float *dskip[3], *dpred, *ga, *gb;
    float *pack_cache;                 // every packed weight form of the step (rf_handle::cache_packs), written at its start
    float *part;                       // reduction partials
    float *part_wg;                    // ... of the kernels on the weight-gradient stream
    size_t part_floats;                // capacity of each of part / part_wg (launch_gram2 checks its slab partials against it)
    // stage_backward's temporaries, one buffer per tensor (see there)
    float *d_pre, *d_cr, *d_cat, *d_f2, *d_f1, *ln2, *d_ln2, *d_x1, *o, *d_o, *d_qkv, *d_qkvp, *ln1, *d_ln1, *d_xs, *d_tr;
    float *small;                      // attention: per-image C x C matrices and packed per-image weights (SmallLayout)
    float *loss_part;
    size_t total;
};

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// TrainPlan::small in a stage's backward.  Per image: dA [C][C] (from gram2; 3 C^2 floats kept for it), then the packed M2
// (K = 2C, Cout = 2C), the packed A^T and the packed A (C x C each); after the B images the softmax adjoint's dT partials
// [B][heads].  (The forward keeps its per-image folded projection at the start of the same buffer.)
struct SmallLayout {
    size_t m2, at, ap;        // float offsets inside an image's block (dA at 0)
    size_t per, dT_part;      // floats per image = the image stride of all four; float offset of the dT partials
    size_t cleared, floats;   // floats stage_backward zero-fills before the attention adjoint; floats reserved
};
SmallLayout small_layout(int B, int C) {
    SmallLayout l;
    l.m2 = 3 * (size_t)C * C;
    l.at = l.m2 + packed1x1_floats(2 * C, 2 * C);
    l.ap = l.at + packed1x1_floats(C, C);
    l.per = l.ap + packed1x1_floats(C, C);
    l.dT_part = (size_t)B * l.per;
    l.cleared = (size_t)B * (l.per + 64);
    l.floats = l.cleared + 64;
    return l;
}

int make_train_plan(const rf_handle* h, float* base, int B, int H, int W, TrainPlan& p) {
    const rf_config& c = h->cfg;
    Bump b{base};
    const size_t U0 = (size_t)B * c.dim * H * W;
    const int hcx = c.ffn_expansion;
    p.x4 = b.take((size_t)B * 4 * H * W);
    p.e = b.take(U0);
    const bool flca = h->vt.branch == BR_FLCA;
    if (flca) {
        p.gscratch = b.take(guidance_scratch_floats(B, H, W));
        for (int l = 0; l < 4; ++l) p.guide[l] = b.take((size_t)B * 4 * (H >> l) * (W >> l));
    }
    size_t part = 0, small = 0, fscr = 0;
    auto stage = [&](int i, int lvl) -> int {
        const int C = c.dim << lvl, hh = H >> lvl, ww = W >> lvl;
        const size_t U = (size_t)B * C * hh * ww;
        Stash& s = p.st[i];
        s.qkvp = b.take(3 * U); s.qkv = b.take(3 * U); s.x1 = b.take(U); s.f1 = b.take(hcx * U); s.f2 = b.take(hcx * U); s.g = b.take(hcx * U);
        s.trans = b.take(U); s.xs = b.take(U); s.cr = b.take(U); s.out = b.take(U);
        if (flca) {
            s.xraw = b.take(U); s.ch = b.take((size_t)B * C); s.pool = b.take((size_t)B * flca_nblk(hh, ww) * C);
            fscr = max_sz(fscr, flca_bwd_scratch_floats(B, C, hh, ww));
        }
        size_t pf;
        RF_TRY(gram_plan(B, C, c.heads[lvl], hh * ww, &s.nslab, &s.slab, &pf));
        s.partial = b.take(pf);
        const int hc = C * hcx;
        part = max_sz(part, gram2_partial_floats(B, C, C, hh, ww, 9));
        part = max_sz(part, gram2_partial_floats(B, 3 * C, C, hh, ww, 1));
        part = max_sz(part, gram2_partial_floats(B, hc, hc, hh, ww, 1));
        part = max_sz(part, gram2_partial_floats(B, 2 * C, 4 * C, hh, ww, 1));
        part = max_sz(part, ln_bwd_partial_floats(B, C, hh * ww));
        part = max_sz(part, dw_wgrad_partial_floats(B, 3 * C > hc ? 3 * C : hc, hh * ww));
        small = max_sz(small, small_layout(B, C).floats);
        return RF_OK;
    };
    for (int i = 1; i <= 4; ++i) {
        RF_TRY(stage(i, i - 1));
        if (i <= 3) p.down[i - 1] = b.take(U0 >> i);
    }
    for (int i = 1; i <= 3; ++i) {
        const int lvl = 3 - i;
        p.up[i - 1] = b.take(U0 >> lvl);
        p.catr[i - 1] = b.take(U0 >> lvl);
        RF_TRY(stage(4 + i, lvl));
        p.dskip[lvl] = b.take(U0 >> lvl);
    }
    p.pred = b.take((size_t)B * c.out_channels * 4 * H * W);
    p.dpred = b.take((size_t)B * c.out_channels * 4 * H * W);
    const size_t T = max_sz(3, (size_t)hcx) * U0;
    p.tA = b.take(T); p.tB = b.take(T); p.tC = b.take(T); p.tD = b.take(T); p.tE = b.take(64);
    p.ga = b.take(U0); p.gb = b.take(U0);
    p.pack_cache = b.take(h->cache_floats);
    p.part_floats = max_sz(part, (size_t)B * 64 * 512);
    p.part = b.take(p.part_floats);
    p.part_wg = b.take(p.part_floats);
    p.d_pre = b.take(U0); p.d_cr = b.take(U0); p.d_cat = b.take(2 * U0); p.d_f2 = b.take(hcx * U0); p.d_f1 = b.take(hcx * U0);
    p.ln2 = b.take(U0); p.d_ln2 = b.take(U0); p.d_x1 = b.take(U0); p.o = b.take(U0); p.d_o = b.take(U0);
    p.d_qkv = b.take(3 * U0); p.d_qkvp = b.take(3 * U0); p.ln1 = b.take(U0); p.d_ln1 = b.take(U0); p.d_xs = b.take(U0); p.d_tr = b.take(U0);
    p.small = b.take(small);
    p.loss_part = b.take(4096);
    p.flca_scr = b.take(fscr);
    p.flca_scr_floats = fscr;
    p.total = b.used;
    return RF_OK;
}

struct Ctx {
    const rf_handle* h;
    TrainPlan* p;
    float* grads;      // flat gradient buffer
    int B;
    hipStream_t st;
    // weight-gradient stream: inside stage_backward (on its own copy of the Ctx) the side stream, where the dW kernels -- which
    // nothing downstream of the stage waits for -- run beside the dX chain; st everywhere else
    hipStream_t wg;
    SideStream* side;
    bool forked() const { return wg != st; }
    float* dw_part() const { return forked() ? p->part_wg : p->part; }
    float* G(int ix) const { return grads + h->flat_offset[ix]; }
    FlcaGrad flca_grad(const FlcaGroup<int>& x) const {
        return {G(x.alpha), G(x.beta), G(x.gamma), G(x.w_low), G(x.w_high), G(x.w_chr), {G(x.se.se1_w), G(x.se.se1_b), G(x.se.se3_w), G(x.se.se3_b)}};
    }
    // weight `ix` in pack-cache form `form`; the b3 forms are optional (nullptr: the f32 kernels), the others an error when missing
    const float* pk(int ix, int form) const {
        const size_t off = h->params[ix].cache[form];
        return off == kNotCached ? nullptr : p->pack_cache + off;
    }
    int pk(int ix, int form, const float** out) const {
        *out = pk(ix, form);
        if (*out) return RF_OK;
        static const char* const names[PF_COUNT] = {"PF_N", "PF_T", "PF_CTB", "PF_N3", "PF_T3", "PF_CTB3"};
        set_error("rf_train_step: the pack cache holds no %s form of '%s'", names[form], h->params[ix].name.c_str());
        return RF_E_INVALID;
    }
};

// ---- forward helpers (weights by registry index, packed forms from the pack cache) --------------------------------------
int f_conv1x1(const Ctx& c, const float* x1, int C1, const float* x2, int C2, int w, const float* bias, const float* ln_w, const float* ln_b,
              const float* res, float* out, int Cout, int P_) {
    Conv1x1Args a{};
    RF_TRY(c.pk(w, PF_N, &a.wp));
    a.wp3 = c.pk(w, PF_N3);
    a.x1 = x1; a.C1 = C1; a.x1_bstride = (int64_t)C1 * P_;
    a.x2 = x2; a.C2 = C2; a.x2_bstride = (int64_t)C2 * P_;
    a.bias = bias; a.ln_w = ln_w; a.ln_b = ln_b; a.ln_eps = 1e-5f;
    a.res = res; a.res_bstride = (int64_t)Cout * P_;
    a.out = out; a.out_bstride = (int64_t)Cout * P_; a.Cout = Cout; a.B = c.B; a.P = P_; a.w = P_;
    return launch_conv1x1(a, c.st);
}

// form PF_N: the forward conv; PF_T: its dX (b_conv3x3_dx)
int f_conv3x3(const Ctx& c, const float* x, int Cin, int w, const float* bias, float* out, int Cout, int hh, int ww, int act, int store,
              int form = PF_N) {
    Conv3x3Args a{};
    RF_TRY(c.pk(w, form, &a.wp));
    a.x = x; a.x_bstride = (int64_t)Cin * hh * ww; a.bias = bias; a.out = out;
    a.out_bstride = (int64_t)Cout * hh * ww; a.B = c.B; a.Cin = Cin; a.Cout = Cout; a.h = hh; a.w = ww; a.act = act; a.store = store;
    return launch_conv3x3(a, c.st);
}

int f_dw(const Ctx& c, const float* x, const float* w, const float* bias, float* out, int C, int hh, int ww, float* out_gelu = nullptr) {
    DwConvArgs d{};
    d.x = x; d.x_bstride = (int64_t)C * hh * ww; d.out = out; d.out_bstride = (int64_t)C * hh * ww; d.w = w; d.bias = bias;
    d.B = c.B; d.C = C; d.h = hh; d.w_ = ww; d.gelu = 0; d.out2 = out_gelu;
    return launch_dwconv3x3(d, c.st);
}

// ---- backward helpers ------------------------------------------------------------------------------------------------
// dX of a 1x1 conv with raw weight [Cout][K]: conv1x1 with W^T (out: K channels)
// (dy_bstride: floats between the images of dy when it is a channel slice of a wider tensor; 0 = contiguous)
int b_conv1x1_dx(const Ctx& c, const float* dy, int Cout, int w, int K, float* dx, int P_, const float* res = nullptr, int64_t dy_bstride = 0) {
    Conv1x1Args a{};
    RF_TRY(c.pk(w, PF_T, &a.wp));
    a.wp3 = c.pk(w, PF_T3);
    a.x1 = dy; a.C1 = Cout; a.x1_bstride = dy_bstride ? dy_bstride : (int64_t)Cout * P_;
    a.res = res; a.res_bstride = (int64_t)K * P_;
    a.out = dx; a.out_bstride = (int64_t)K * P_; a.Cout = K; a.B = c.B; a.P = P_; a.w = P_;
    return launch_conv1x1(a, c.st);
}

// dW of a convolution layer [Cout][ld][ntap] += gram2(dy, x) over all images, accumulated into the flat gradient buffer on the
// weight-gradient stream (launched on c.wg after c.side->fork): what gram2_of (rf_grad.h) takes for it
Wgrad wgrad(const Ctx& c, int P_) { return Wgrad{"rf_train_step", c.dw_part(), c.p->part_floats, c.B, P_, 1, c.wg}; }

// dW [Cout][ld] columns [col0, col0 + Cx) += gram2(dy, x);  db = channel sums of dy, taken in the same pass
// (x2 / Cx2: the layer's input is cat(x, x2) along channels, read in place)
int b_conv1x1_dw(const Ctx& c, const float* dy, int Cout, const float* x, int Cx, float* dW, int ld, int col0, float* db, int hh, int ww,
                 int64_t dy_bstride = 0, const float* x2 = nullptr, int Cx2 = 0) {
    RF_TRY(c.side->fork(c.st, c.wg));
    Gram2Launch g = gram2_of(wgrad(c, hh * ww), dy, dy_bstride ? dy_bstride : (int64_t)Cout * hh * ww, Cout, x, (int64_t)Cx * hh * ww, Cx,
                             dW + col0, ld, col0 == 0 ? db : nullptr, ww, 1);
    if (Cx2 && Cx % 16 != 0) {       // the two-source contraction cuts the inputs at a tile boundary: otherwise one pass per input
        RF_TRY(launch_gram2(g, c.wg));
        g.b = x2; g.b_bstride = (int64_t)Cx2 * hh * ww; g.Cb = Cx2; g.out = dW + col0 + Cx; g.db = nullptr;
    } else {
        g.b2 = x2; g.b2_bstride = (int64_t)Cx2 * hh * ww; g.Cb2 = Cx2;
    }
    return launch_gram2(g, c.wg);
}

int b_conv3x3_dx(const Ctx& c, const float* dy, int Cout, int w, int Cin, float* dx, int hh, int ww) {
    return f_conv3x3(c, dy, Cout, w, nullptr, dx, Cin, hh, ww, 0, 0, PF_T);
}

int b_conv3x3_dw(const Ctx& c, const float* dy, int Cout, const float* x, int Cin, float* dW, float* db, int hh, int ww) {
    RF_TRY(c.side->fork(c.st, c.wg));
    return launch_gram2(gram2_of(wgrad(c, hh * ww), dy, (int64_t)Cout * hh * ww, Cout, x, (int64_t)Cin * hh * ww, Cin, dW, Cin, db, ww, 9), c.wg);
}

// depthwise 3x3 with weight `w`: dW, db on the weight-gradient stream, dX = the forward kernel on the flipped taps
int b_dw(const Ctx& c, const float* dy, const float* x, int w, float* dx, float* dW, float* db, int C, int hh, int ww) {
    RF_TRY(c.side->fork(c.st, c.wg));
    RF_TRY(launch_dw_wgrad(x, dy, dW, db, c.dw_part(), c.B, C, hh, ww, 1, c.wg));
    const float* wf;
    RF_TRY(c.pk(w, PF_T, &wf));
    return f_dw(c, dy, wf, nullptr, dx, C, hh, ww);
}

// ---- attention, small per-(head, image) kernel (rf_train.hip: launch_attn_small) --------------------------------------
int attn_small(const Ctx& c, const Stash& s, const float* temperature, int C, int heads, int fwd_only, float* dT) {
    const SmallLayout l = small_layout(c.B, C);
    float* sm = c.p->small;
    AttnSmall a{};
    a.partial = s.partial; a.nslab = s.nslab; a.temperature = temperature;
    a.dA = sm; a.dA_istride = l.per;
    a.m2 = sm + l.m2; a.m2_istride = l.per;
    a.at = sm + l.at; a.ap = sm + l.ap; a.a_istride = l.per;
    a.dT_part = sm + l.dT_part;
    a.C = C; a.heads = heads; a.fwd_only = fwd_only;
    RF_TRY(launch_attn_small(a, c.B, c.st));
    if (!fwd_only && dT) RF_TRY(launch_reduce_rows(a.dT_part, dT, c.B, (size_t)heads, 1, c.st));   // dT[h] += sum over images, in order
    return RF_OK;
}

}  // namespace

// ---- the step ---------------------------------------------------------------------------------------------------------
namespace {

int stage_forward(const Ctx& c, int i, const float* in, int H, int W) {
    const rf_handle* h = c.h;
    const rf_config& cfg = h->cfg;
    const StageIx& x = h->stage[i];
    const int lvl = x.lvl, C = cfg.dim << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww, heads = cfg.heads[lvl], hc = C * cfg.ffn_expansion;
    Stash& s = c.p->st[i];
    s.in = in;
    RF_TRY(f_conv1x1(c, in, C, nullptr, 0, x.qkv_w, h->prm(x.qkv_b), h->prm(x.ln1_w), h->prm(x.ln1_b), nullptr, s.qkvp, 3 * C, Pn));
    RF_TRY(f_dw(c, s.qkvp, h->prm(x.qkv_dw_w), h->prm(x.qkv_dw_b), s.qkv, 3 * C, hh, ww));
    GramArgs g{};
    g.q = s.qkv; g.k = s.qkv + (size_t)C * Pn; g.bstride = (int64_t)3 * C * Pn; g.B = c.B; g.C = C; g.heads = heads; g.P = Pn;
    g.partial = s.partial; g.nslab = s.nslab; g.slab = s.slab;
    RF_TRY(launch_gram(g, c.st));
    // attention map -> per-image folded projection (forward only), x1 = in + W_out A v + b
    float* wfold = c.p->small;
    RF_TRY(launch_attn_fold(s.partial, s.nslab, h->prm(x.temperature), h->prm(x.proj_w), wfold, nullptr, c.B, C, heads, c.st));
    {
        Conv1x1Args a{};
        a.x1 = s.qkv + (size_t)2 * C * Pn; a.C1 = C; a.x1_bstride = (int64_t)3 * C * Pn; a.wp = wfold; a.wp_bstride = (int64_t)packed1x1_floats(C, C);
        a.bias = h->prm(x.proj_b); a.res = in; a.res_bstride = (int64_t)C * Pn;
        a.out = s.x1; a.out_bstride = (int64_t)C * Pn; a.Cout = C; a.B = c.B; a.P = Pn; a.w = ww;
        RF_TRY(launch_conv1x1(a, c.st));
    }
    RF_TRY(f_conv1x1(c, s.x1, C, nullptr, 0, x.pw1_w, h->prm(x.pw1_b), h->prm(x.ln2_w), h->prm(x.ln2_b), nullptr, s.f1, hc, Pn));
    RF_TRY(f_dw(c, s.f1, h->prm(x.dw_w), h->prm(x.dw_b), s.f2, hc, hh, ww, s.g));   // f2 and g = gelu(f2)
    RF_TRY(f_conv1x1(c, s.g, hc, nullptr, 0, x.pw2_w, h->prm(x.pw2_b), nullptr, nullptr, s.x1, s.trans, C, Pn));
    if (h->vt.branch == BR_FLCA) {
        const FlcaPrm fp = h->flca_prm(x.flca);
        FlcaSpatialArgs sa{};
        sa.feat = in; sa.xs = s.xraw; sa.guide = c.p->guide[lvl];
        sa.set_params(fp);
        sa.partial = s.pool; sa.B = c.B; sa.C = C; sa.h = hh; sa.w = ww; sa.nblk = flca_nblk(hh, ww);
        RF_TRY(launch_flca_spatial(sa, c.st));
        RF_TRY(launch_flca_se(s.pool, sa.nblk, Pn, fp.se, s.ch, c.B, C, c.st));
        RF_TRY(launch_scale_channels_to(s.xraw, s.xs, s.ch, c.B, C, Pn, c.st));                         // xs = branch output z
    } else {
        RF_TRY(f_conv3x3(c, in, C, x.conv_w, h->prm(x.conv_b), s.xs, C, hh, ww, cfg.branch_lrelu ? 1 : 0, 0));
    }
    RF_TRY(f_conv1x1(c, s.xs, C, s.trans, C, x.cr_w, h->prm(x.cr_b), nullptr, nullptr, nullptr, s.cr, C, Pn));
    RF_TRY(f_conv3x3(c, s.cr, C, x.out_w, h->prm(x.out_b), s.out, C, hh, ww, 1, 0));
    return RF_OK;
}

// dout: gradient w.r.t. the stage output (consumed); din: receives the gradient w.r.t. the stage input; wg: the stage's
// weight-gradient stream
int stage_backward(const Ctx& outer, hipStream_t wg, int i, float* dout, float* din, int H, int W) {
    Ctx c = outer;
    c.wg = wg;
    const rf_handle* h = c.h;
    const rf_config& cfg = h->cfg;
    const StageIx& x = h->stage[i];
    const int lvl = x.lvl, C = cfg.dim << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww, heads = cfg.heads[lvl], hc = C * cfg.ffn_expansion;
    const Stash& s = c.p->st[i];
    const size_t U = (size_t)c.B * C * Pn;
    // One buffer per tensor: the weight-gradient kernels read them from their own stream while the dX chain moves on, so nothing
    // is overwritten inside a stage; the stage ends with a join, after which the next stage reuses the buffers.
    const TrainPlan& t = *c.p;
    float *d_pre = t.d_pre, *d_cr = t.d_cr, *d_cat = t.d_cat, *d_f2 = t.d_f2, *d_f1 = t.d_f1, *ln2 = t.ln2, *d_ln2 = t.d_ln2, *d_x1 = t.d_x1, *o = t.o,
          *d_o = t.d_o, *d_qkv = t.d_qkv, *d_qkvp = t.d_qkvp, *ln1 = t.ln1, *d_ln1 = t.d_ln1, *d_xs = t.d_xs, *d_tr = t.d_tr;
    // Conv_out + LeakyReLU
    RF_TRY(launch_ewise(dout, s.out, d_pre, U, EW_LRELU_GRAD, 0.2f, c.st));                                      // d(pre-activation)
    RF_TRY(b_conv3x3_dw(c, d_pre, C, s.cr, C, c.G(x.out_w), c.G(x.out_b), hh, ww));
    RF_TRY(b_conv3x3_dx(c, d_pre, C, x.out_w, C, d_cr, hh, ww));
    // channel_reduce over cat[xs, trans]
    RF_TRY(b_conv1x1_dw(c, d_cr, C, s.xs, C, c.G(x.cr_w), 2 * C, 0, c.G(x.cr_b), hh, ww, 0, s.trans, C));
    RF_TRY(b_conv1x1_dx(c, d_cr, C, x.cr_w, 2 * C, d_cat, Pn));           // d_cat = [dxs ; dtrans] per image
    // dxs and dtrans are read in place as channel slices of d_cat (image stride 2C Pn) by the kernels that take a stride; only the
    // plain variant's element-wise LeakyReLU adjoint (and a LayerNorm shape without the fused kernel) needs contiguous halves
    const float* dxs = d_cat;
    const float* dtr = d_cat + (size_t)C * Pn;
    int64_t half_bs = (int64_t)2 * C * Pn;
    if (h->vt.branch != BR_FLCA || !ln_bwd_fused_shape(C, Pn)) {
        RF_TRY(launch_split_halves(d_cat, d_xs, d_tr, c.B, C, Pn, c.st));
        dxs = d_xs; dtr = d_tr; half_bs = (int64_t)C * Pn;
    }
    if (h->vt.branch == BR_FLCA) {
        RF_TRY(launch_flca_backward(s.in, c.p->guide[lvl], s.xraw, dxs, half_bs, s.ch, s.pool, flca_nblk(hh, ww), h->flca_prm(x.flca),
                                    c.flca_grad(x.flca), din, 0, c.p->flca_scr, c.p->flca_scr_floats, c.B, C, hh, ww, c.st));   // din = branch part
    } else {
        // conv branch
        if (cfg.branch_lrelu) RF_TRY(launch_ewise(d_xs, s.xs, d_xs, U, EW_LRELU_GRAD, 0.2f, c.st));
        RF_TRY(b_conv3x3_dw(c, d_xs, C, s.in, C, c.G(x.conv_w), c.G(x.conv_b), hh, ww));
        RF_TRY(b_conv3x3_dx(c, d_xs, C, x.conv_w, C, din, hh, ww));                  // din = branch part
    }
    // FFN:  trans = x1 + pw2(gelu(dw(pw1(LN2(x1)))))          dtr = dtrans (also the residual part of dx1)
    RF_TRY(b_conv1x1_dw(c, dtr, C, s.g, hc, c.G(x.pw2_w), hc, 0, c.G(x.pw2_b), hh, ww, half_bs));
    RF_TRY(b_conv1x1_dx(c, dtr, C, x.pw2_w, hc, d_f2, Pn, nullptr, half_bs));   // dg ...
    RF_TRY(launch_ewise(d_f2, s.f2, d_f2, (size_t)c.B * hc * Pn, EW_GELU_GRAD, 0.f, c.st));                      // ... -> df2, in place
    RF_TRY(b_dw(c, d_f2, s.f1, x.dw_w, d_f1, c.G(x.dw_w), c.G(x.dw_b), hc, hh, ww));
    RF_TRY(launch_layernorm2d(s.x1, ln2, h->prm(x.ln2_w), h->prm(x.ln2_b), 1e-5f, c.B, C, Pn, c.st));   // LN2(x1) again
    RF_TRY(b_conv1x1_dw(c, d_f1, hc, ln2, C, c.G(x.pw1_w), C, 0, c.G(x.pw1_b), hh, ww));
    RF_TRY(b_conv1x1_dx(c, d_f1, hc, x.pw1_w, C, d_ln2, Pn));               // d LN2 out
    // d_x1 = dtrans + (LayerNorm adjoint), dtrans read in place
    RF_TRY(launch_ln_bwd(s.x1, d_ln2, h->prm(x.ln2_w), d_x1, c.G(x.ln2_w), c.p->part, c.B, C, Pn, 1e-5f, 0, 1, c.st, dtr, half_bs));
    // attention:  x1 = in + W_out (A v) + b          (the residual din += dx1 rides on the last kernel of the stage)
    const SmallLayout sl = small_layout(c.B, C);
    RF_TRY(check_hip(hipMemsetAsync(c.p->small, 0, sl.cleared * sizeof(float), c.st), "memset"));
    RF_TRY(attn_small(c, s, h->prm(x.temperature), C, heads, 1, nullptr));                     // packed A, A^T
    float *m2 = c.p->small + sl.m2, *at = c.p->small + sl.at, *ap = c.p->small + sl.ap;
    const float* v = s.qkv + (size_t)2 * C * Pn;
    {   // o = blockdiag(A) v
        Conv1x1Args a{};
        a.x1 = v; a.C1 = C; a.x1_bstride = (int64_t)3 * C * Pn; a.wp = ap; a.wp_bstride = (int64_t)sl.per;
        a.out = o; a.out_bstride = (int64_t)C * Pn; a.Cout = C; a.B = c.B; a.P = Pn; a.w = ww;
        RF_TRY(launch_conv1x1(a, c.st));
    }
    RF_TRY(b_conv1x1_dw(c, d_x1, C, o, C, c.G(x.proj_w), C, 0, c.G(x.proj_b), hh, ww));
    RF_TRY(b_conv1x1_dx(c, d_x1, C, x.proj_w, C, d_o, Pn));
    // dA per image: on the dX chain (the softmax adjoint waits for it)
    Gram2Launch dA{};
    dA.a = d_o; dA.a_bstride = (int64_t)C * Pn; dA.Ca = C;
    dA.b = v; dA.b_bstride = (int64_t)3 * C * Pn; dA.Cb = C;
    dA.out = c.p->small; dA.ld = C; dA.per_image = true; dA.out_istride = sl.per;
    dA.partial = c.p->part; dA.partial_cap = c.p->part_floats; dA.B = c.B; dA.h = hh; dA.w = ww; dA.ntap = 1;
    RF_TRY(launch_gram2(dA, c.st));
    RF_TRY(attn_small(c, s, h->prm(x.temperature), C, heads, 0, c.G(x.temperature)));
    {   // d(qkv): [dq ; dk] = M2 [q ; k],  dv = blockdiag(A^T) do
        Conv1x1Args a{};
        a.x1 = s.qkv; a.C1 = 2 * C; a.x1_bstride = (int64_t)3 * C * Pn; a.wp = m2; a.wp_bstride = (int64_t)sl.per;
        a.out = d_qkv; a.out_bstride = (int64_t)3 * C * Pn; a.Cout = 2 * C; a.B = c.B; a.P = Pn; a.w = ww;
        RF_TRY(launch_conv1x1(a, c.st));
        Conv1x1Args d{};
        d.x1 = d_o; d.C1 = C; d.x1_bstride = (int64_t)C * Pn; d.wp = at; d.wp_bstride = (int64_t)sl.per;
        d.out = d_qkv + (size_t)2 * C * Pn; d.out_bstride = (int64_t)3 * C * Pn; d.Cout = C; d.B = c.B; d.P = Pn; d.w = ww;
        RF_TRY(launch_conv1x1(d, c.st));
    }
    RF_TRY(b_dw(c, d_qkv, s.qkvp, x.qkv_dw_w, d_qkvp, c.G(x.qkv_dw_w), c.G(x.qkv_dw_b), 3 * C, hh, ww));
    RF_TRY(launch_layernorm2d(s.in, ln1, h->prm(x.ln1_w), h->prm(x.ln1_b), 1e-5f, c.B, C, Pn, c.st));   // LN1(in) again
    RF_TRY(b_conv1x1_dw(c, d_qkvp, 3 * C, ln1, C, c.G(x.qkv_w), C, 0, c.G(x.qkv_b), hh, ww));
    RF_TRY(b_conv1x1_dx(c, d_qkvp, 3 * C, x.qkv_w, C, d_ln1, Pn));                // d LN1 out
    // din (branch part) += dx1 (residual of x1 = in + attention) + (LayerNorm adjoint)
    RF_TRY(launch_ln_bwd(s.in, d_ln1, h->prm(x.ln1_w), din, c.G(x.ln1_w), c.p->part, c.B, C, Pn, 1e-5f, 1, 1, c.st, d_x1, (int64_t)C * Pn));
    return c.side->join(c.st, c.wg);
}

}  // namespace

// ---- training layout, fixed by the registry (rf_create) -----------------------------------------------------------------
void plan_training(rf_handle* h) {
    // flat buffers: registry order, every tensor on a 16-byte boundary (a LayerNorm's weight and bias stay adjacent)
    for (const Param& q : h->params) {
        h->flat_offset.push_back(h->flat_floats);
        h->flat_floats += align_up(q.numel(), 4);
    }
    // Gradient ranges in the order they become final = reverse registry order of the modules (the registry is in forward
    // order): conv_out, conv_tran7, up3, conv_tran6, up2, conv_tran5, up1, conv_tran4 .. conv_tran1, embedding.  A range runs from
    // its module's first float to the previous one's, so channel_reduce<i> rides with up<i>, down<i> with conv_tran<i>, and
    // TrueColor's color_correction with conv_out.
    const int first[12] = {h->conv_out_w, h->stage[7].first, h->up_w[2], h->stage[6].first, h->up_w[1], h->stage[5].first, h->up_w[0],
                           h->stage[4].first, h->stage[3].first, h->stage[2].first, h->stage[1].first, h->embedding_w};
    size_t watermark = h->flat_floats;
    for (int ix : first) {
        h->grad_ranges.push_back({h->flat_offset[ix], watermark - h->flat_offset[ix]});
        watermark = h->flat_offset[ix];
    }
    // Pack cache: the forms of every weight the step multiplies by a GEMM / conv kernel, in registry order (the gate
    // convolutions of FLCA have their own kernels).  The step writes them with launch_pack_batch before its forward.
    for (size_t ix = 0; ix < h->params.size(); ++ix) {
        Param& q = h->params[ix];
        for (size_t& off : q.cache) off = kNotCached;
        if (q.ndim != 4 || q.name.find("FLCA.") != std::string::npos) continue;
        auto add = [&](int form, int kind, int rows, int cols, int64_t rs, int64_t cs, int flip) {
            const PackDesc d{nullptr, nullptr, kind, rows, cols, rs, cs, flip};
            q.cache[form] = h->cache_floats;
            h->cache_packs.push_back({(int)ix, h->cache_floats, d});
            h->cache_floats += align_up(pack_desc_floats(d), 64);
        };
        const int n0 = (int)q.shape[0], n1 = (int)q.shape[1], kh = (int)q.shape[2];
        if (kh == 1) {                                   // 1x1 conv [Cout][K]
            add(PF_N, 0, n0, n1, n1, 1, 0);
            add(PF_T, 0, n1, n0, 1, n1, 0);
            if (n1 >= 128) add(PF_N3, 3, n0, n1, n1, 1, 0);
            if (n0 >= 128) add(PF_T3, 3, n1, n0, 1, n1, 0);
        } else if (kh == 3 && n1 == 1) {                 // depthwise [C][1][3][3]: dX runs the forward kernel on flipped taps
            add(PF_T, 2, n0, 9, 9, 1, 0);
        } else if (kh == 3) {                            // 3x3 conv [Cout][Cin][3][3]
            add(PF_N, 1, n0, n1, (int64_t)n1 * 9, 9, 0);
            add(PF_T, 1, n1, n0, 9, (int64_t)n1 * 9, 1);
        } else if (kh == 2) {                            // ConvTranspose2d [Cin][Cout][2][2]: GEMM row 4 o + 2 i + j, column k (pack_convT)
            add(PF_N, 0, 4 * n1, n0, 1, (int64_t)4 * n1, 0);
            add(PF_CTB, 0, n0, 4 * n1, (int64_t)4 * n1, 1, 0);
            if (n0 >= 128) add(PF_N3, 3, 4 * n1, n0, 1, (int64_t)4 * n1, 0);
            if (4 * n1 >= 128) add(PF_CTB3, 3, n0, 4 * n1, (int64_t)4 * n1, 1, 0);
        }
    }
}

extern "C" {

int rf_set_grad_ready(rf_handle* h, rf_grad_ready_fn ready, void* user) {
    RF_CHECK_ARG(h, "rf_set_grad_ready: null handle");
    h->grad_ready = ready; h->grad_ready_user = ready ? user : nullptr;
    return RF_OK;
}

int rf_set_loss_clamp(rf_handle* h, int on) {
    RF_CHECK_ARG(h, "rf_set_loss_clamp: null handle");
    h->loss_clamp = on != 0;
    return RF_OK;
}

int rf_grad_range_count(const rf_handle* h, int* count) {
    RF_CHECK_ARG(h && count, "rf_grad_range_count: null argument");
    *count = (int)h->grad_ranges.size();
    return RF_OK;
}

int rf_grad_range(const rf_handle* h, int index, size_t* offset, size_t* count) {
    RF_CHECK_ARG(h && offset && count && index >= 0, "rf_grad_range: bad arguments");
    const int n = (int)h->grad_ranges.size();
    RF_CHECK_ARG(index < n, "rf_grad_range: index %d out of range (%d ranges)", index, n);
    *offset = h->grad_ranges[index].offset;
    *count = h->grad_ranges[index].count;
    return RF_OK;
}

int rf_flat_param_floats(const rf_handle* h, size_t* floats) {
    RF_CHECK_ARG(h && floats, "rf_flat_param_floats: null argument");
    *floats = h->flat_floats;
    return RF_OK;
}

int rf_flat_offset(const rf_handle* h, int index, size_t* offset) {
    RF_CHECK_ARG(h && offset && index >= 0 && index < (int)h->params.size(), "rf_flat_offset: index %d out of range", index);
    *offset = h->flat_offset[index];
    return RF_OK;
}

int rf_train_workspace_bytes(const rf_handle* h, int B, int H, int W, size_t* bytes) {
    RF_CHECK_ARG(h && bytes, "rf_train_workspace_bytes: null argument");
    RF_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0, "rf_train_workspace_bytes: B = %d, packed size %dx%d", B, H, W);
    RF_CHECK_ARG(H % 8 == 0, "rf_train_workspace_bytes: packed height %d is not a multiple of 8", H);
    RF_CHECK_ARG(W % 32 == 0, "rf_train_workspace_bytes: packed width %d is not a multiple of 32", W);
    TrainPlan p;
    RF_TRY(make_train_plan(h, nullptr, B, H, W, p));
    *bytes = p.total * sizeof(float);
    return RF_OK;
}

int rf_train_step(rf_handle* h, const float* in, const float* gt, float* grads, float* loss_out, float* pred_out, void* workspace,
                  size_t workspace_bytes, int B, int H, int W, int loss_mode, float loss_eps, void* stream) {
    RF_CHECK_ARG(h && in && gt && grads && loss_out && workspace && aligned16(workspace) && aligned16(grads), "rf_train_step: bad arguments");
    // clamp_io under the clamped criterion (rf_set_loss_clamp) is the criterion's own mask; the plain variant alone, whose input
    // clamp feeds nothing but the embedding
    const bool clamp_io = h->cfg.clamp_io && h->loss_clamp && h->cfg.variant == RF_VARIANT_PLAIN;
    RF_CHECK_ARG((h->cfg.variant == RF_VARIANT_PLAIN || h->cfg.variant == RF_VARIANT_FLCA) && (!h->cfg.clamp_io || clamp_io),
                 "rf_train_step: variants 'plain' and 'flca' without clamp_io have their adjoint so far");
    RF_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0, "rf_train_step: B = %d, packed size %dx%d", B, H, W);
    RF_CHECK_ARG(H % 8 == 0, "rf_train_step: packed height %d is not a multiple of 8", H);
    RF_CHECK_ARG(W % 32 == 0, "rf_train_step: packed width %d is not a multiple of 32", W);
    for (const Param& q : h->params) RF_CHECK_ARG(q.ptr, "rf_train_step: parameter '%s' not set", q.name.c_str());
    TrainPlan p;
    RF_TRY(make_train_plan(h, (float*)workspace, B, H, W, p));
    if (workspace_bytes < p.total * sizeof(float)) {
        set_error("rf_train_step: workspace of %zu bytes, need %zu", workspace_bytes, p.total * sizeof(float));
        return RF_E_NOMEM;
    }
    hipStream_t st = (hipStream_t)stream;
    const rf_config& cfg = h->cfg;
    const int d = cfg.dim, oc = cfg.out_channels;
    SideJoinGuard joined(h->side, st);
    Ctx c{h, &p, grads, B, st, st, &h->side};
    RF_TRY(check_hip(hipMemsetAsync(grads, 0, h->flat_floats * sizeof(float), st), "memset grads"));
    std::vector<PackDesc> packs;
    for (const CachePack& k : h->cache_packs) {
        packs.push_back(k.d);
        packs.back().src = h->prm(k.param);
        packs.back().dst = p.pack_cache + k.offset;
    }
    RF_TRY(launch_pack_batch(packs.data(), (int)packs.size(), st));
    const hipStream_t wg = h->side.get(st);      // the stages' weight-gradient stream

    // ------------------------------------------------------------------ forward
    RF_TRY(launch_pixel_unshuffle2(in, p.x4, B, 1, H, W, st));
    if (clamp_io) RF_TRY(launch_ewise(p.x4, nullptr, p.x4, (size_t)B * 4 * H * W, EW_CLAMP01, 0.f, st));      // model.py:475
    if (h->vt.branch == BR_FLCA) {
        RF_TRY(launch_guidance_base(p.x4, 0, 0, p.gscratch, B, H, W, st));
        for (int l = 0; l < 4; ++l) RF_TRY(launch_guidance_level(p.gscratch, p.guide[l], B, H, W, H >> l, W >> l, st));
    }
    RF_TRY(f_conv3x3(c, p.x4, 4, h->embedding_w, h->prm(h->embedding_b), p.e, d, H, W, 0, 0));
    const float* cur = p.e;
    for (int i = 1; i <= 3; ++i) {
        const int lvl = i - 1, C = d << lvl, hh = H >> lvl, ww = W >> lvl;
        RF_TRY(stage_forward(c, i, cur, H, W));
        RF_TRY(f_conv3x3(c, p.st[i].out, C, h->down_w[i - 1], nullptr, p.down[i - 1], C / 2, hh, ww, 0, 1));
        cur = p.down[i - 1];
    }
    RF_TRY(stage_forward(c, 4, cur, H, W));
    cur = p.st[4].out;
    for (int i = 1; i <= 3; ++i) {
        const int lvl = 3 - i, C = d << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww;
        Conv1x1Args up{};
        RF_TRY(c.pk(h->up_w[i - 1], PF_N, &up.wp));
        up.wp3 = c.pk(h->up_w[i - 1], PF_N3);
        up.x1 = cur; up.C1 = 2 * C; up.x1_bstride = (int64_t)2 * C * (Pn / 4); up.bias = h->prm(h->up_b[i - 1]);
        up.out = p.up[i - 1]; up.out_bstride = (int64_t)C * Pn; up.Cout = 4 * C; up.B = B; up.P = Pn / 4; up.w = ww / 2; up.mode = 1;
        RF_TRY(launch_conv1x1(up, st));
        RF_TRY(f_conv1x1(c, p.up[i - 1], C, p.st[lvl + 1].out, C, h->upcr_w[i - 1], h->prm(h->upcr_b[i - 1]), nullptr, nullptr, nullptr, p.catr[i - 1], C, Pn));
        RF_TRY(stage_forward(c, 4 + i, p.catr[i - 1], H, W));
        cur = p.st[4 + i].out;
    }
    RF_TRY(f_conv3x3(c, cur, d, h->conv_out_w, h->prm(h->conv_out_b), p.pred, 4 * oc, H, W, 1, 2));
    const size_t npred = (size_t)B * oc * 4 * H * W;
    if (pred_out && clamp_io) RF_TRY(launch_ewise(p.pred, nullptr, pred_out, npred, EW_CLAMP01, 0.f, st));    // model.py:508
    else if (pred_out) RF_TRY(check_hip(hipMemcpyAsync(pred_out, p.pred, npred * 4, hipMemcpyDeviceToDevice, st), "copy pred"));

    // ------------------------------------------------------------------ loss
    RF_TRY(launch_loss(p.pred, gt, p.dpred, loss_out, p.loss_part, npred, loss_mode, loss_eps, h->loss_clamp, st));

    // ------------------------------------------------------------------ backward
    float *tA = p.tA, *tB = p.tB;
    // conv_out + LeakyReLU + PixelShuffle
    RF_TRY(launch_pixel_unshuffle2(p.dpred, tA, B, oc, H, W, st));          // [B, 4 oc, H, W]
    RF_TRY(launch_pixel_unshuffle2(p.pred, tB, B, oc, H, W, st));
    RF_TRY(launch_ewise(tA, tB, tA, (size_t)B * 4 * oc * H * W, EW_LRELU_GRAD, 0.2f, st));
    RF_TRY(b_conv3x3_dw(c, tA, 4 * oc, p.st[7].out, d, c.G(h->conv_out_w), c.G(h->conv_out_b), H, W));
    // announce range k of h->grad_ranges (plan_training lists the order): final on st from here on
    auto ready = [&](int k) {
        if (h->grad_ready) h->grad_ready(h->grad_ready_user, h->grad_ranges[k].offset, h->grad_ranges[k].count, (void*)st);
    };
    ready(0);                                                                                  // conv_out
    float* tE_src = p.tC;
    RF_TRY(b_conv3x3_dx(c, tA, 4 * oc, h->conv_out_w, d, tE_src, H, W));    // d(stage 7 out)
    for (int l = 0; l < 3; ++l) RF_TRY(check_hip(hipMemsetAsync(p.dskip[l], 0, ((size_t)B * (d << l) * (H >> l) * (W >> l)) * 4, st), "memset dskip"));
    // ga: gradient w.r.t. the output of the stage about to be processed; gb receives the gradient w.r.t. its input
    float *ga = p.ga, *gb = p.gb;
    RF_TRY(check_hip(hipMemcpyAsync(ga, tE_src, (size_t)B * d * H * W * 4, hipMemcpyDeviceToDevice, st), "copy"));
    // decoder, top-down
    for (int i = 3; i >= 1; --i) {
        const int lvl = 3 - i, C = d << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww;
        RF_TRY(stage_backward(c, wg, 4 + i, ga, gb, H, W));                                   // gb = d(catr_i)
        ready(2 * (3 - i) + 1);                                                                // conv_tran<4 + i>
        // channel_reduce_i over cat[up, skip]
        RF_TRY(b_conv1x1_dw(c, gb, C, p.up[i - 1], C, c.G(h->upcr_w[i - 1]), 2 * C, 0, c.G(h->upcr_b[i - 1]), hh, ww, 0, p.st[lvl + 1].out, C));
        RF_TRY(b_conv1x1_dx(c, gb, C, h->upcr_w[i - 1], 2 * C, p.tC, Pn));                 // tC = [dup ; dskip]
        RF_TRY(launch_split_halves(p.tC, p.tA, p.dskip[lvl], B, C, Pn, st));
        // ConvTranspose2d(2C -> C): dX = conv1x1(unshuffle(dup), W as [2C][4C]);  dW = gram2(x, unshuffle(dup));  db = channel sums of dup
        RF_TRY(launch_chan_sum(p.tA, (int64_t)C * Pn, c.G(h->up_b[i - 1]), p.part, B, C, Pn, 1, st));
        RF_TRY(launch_pixel_unshuffle2(p.tA, p.tB, B, C, hh / 2, ww / 2, st));                 // [B, 4C, hh/2, ww/2]
        const float* xin = (i == 1) ? p.st[4].out : p.st[4 + i - 1].out;
        Gram2Launch g{};
        g.a = xin; g.a_bstride = (int64_t)2 * C * (Pn / 4); g.Ca = 2 * C;
        g.b = p.tB; g.b_bstride = (int64_t)4 * C * (Pn / 4); g.Cb = 4 * C;
        g.out = c.G(h->up_w[i - 1]); g.ld = 4 * C; g.accumulate = true;
        g.partial = p.part; g.partial_cap = p.part_floats; g.B = B; g.h = hh / 2; g.w = ww / 2; g.ntap = 1;
        RF_TRY(launch_gram2(g, st));
        Conv1x1Args a{};
        RF_TRY(c.pk(h->up_w[i - 1], PF_CTB, &a.wp));
        a.wp3 = c.pk(h->up_w[i - 1], PF_CTB3);
        a.x1 = p.tB; a.C1 = 4 * C; a.x1_bstride = (int64_t)4 * C * (Pn / 4);
        a.out = ga; a.out_bstride = (int64_t)2 * C * (Pn / 4); a.Cout = 2 * C; a.B = B; a.P = Pn / 4; a.w = ww / 2;
        RF_TRY(launch_conv1x1(a, st));                                                         // ga = d(previous stage out) [B, 2C, Pn/4]
        ready(2 * (3 - i) + 2);                                                                // up_i and channel_reduce_i
    }
    // bottleneck and encoder, bottom-up: ga = d(stage i out) on entry (for i <= 3 after the Downsample adjoint and the skip gradient)
    for (int i = 4; i >= 1; --i) {
        const int lvl = i - 1, C = d << lvl, hh = H >> lvl, ww = W >> lvl, Pn = hh * ww;
        if (i <= 3) {
            // gb = d(down_i output) [B, 2C, Pn/4] = d(stage i+1 input)
            RF_TRY(launch_pixel_shuffle2(gb, p.tA, B, C / 2, hh / 2, ww / 2, st));             // [B, C/2, hh, ww]
            RF_TRY(b_conv3x3_dw(c, p.tA, C / 2, p.st[i].out, C, c.G(h->down_w[i - 1]), nullptr, hh, ww));
            RF_TRY(b_conv3x3_dx(c, p.tA, C / 2, h->down_w[i - 1], C, ga, hh, ww));
            RF_TRY(launch_ewise(ga, p.dskip[lvl], ga, (size_t)B * C * Pn, EW_ADD, 0.f, st));
        }
        RF_TRY(stage_backward(c, wg, i, ga, gb, H, W));                                       // gb = d(stage i input)
        ready(11 - i);                                                                         // conv_tran<i> and down_i, whose gradient came first
    }
    float* dcur = gb;
    // embedding
    RF_TRY(b_conv3x3_dw(c, dcur, d, p.x4, 4, c.G(h->embedding_w), c.G(h->embedding_b), H, W));
    ready(11);                                                                                 // embedding: the buffer's first float
    return RF_OK;
}

int rf_adam_step(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int decoupled, int step, float grad_scale, void* stream) {
    RF_CHECK_ARG(params && grads && m && v && step >= 1, "rf_adam_step: bad arguments");
    return launch_adam(params, grads, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale, (hipStream_t)stream);
}

}  // extern "C"
