// FLCA branch of the training step, backward (FrequencyawareLumaChromaAttentionRAWFormer.py:103-162).  Forward:
//   S = 1 + alpha sigmoid(conv(g_low; w_low)) + beta tanh(conv(g_high; w_high)) + gamma sigmoid(conv(g_cr, g_cb; w_chr))
//   xs = feat S;   ch = sigmoid(W3 relu(W1 mean_p(xs) + b1) + b3) per image;   z = xs ch
// Backward of z w.r.t. feat and the 10 parameter tensors (the guidance planes carry no gradient: they come from the input):
//   dch[b][c] = sum_p dz xs           -> squeeze-excite MLP backward (tiny, per image) -> dm[b][c] (gradient of the pooled mean)
//   dxs = dz ch + dm / P;   dfeat = dxs S;   dS = dxs feat;   dalpha = sum dS a_low, ...;   d(conv outputs) -> tap sums
// Kernels: flca_dch_kernel (launch_flca_dch: FLCA_Pyramid's backward runs it too), flca_se_bwd_kernel (squeeze-excite part),
// flca_bwd_fused_kernel (spatial part and tap sums in one pass), flca_abg_kernel and flca_taps_scatter_kernel (the last step of
// their sums).  The squeeze-excite MLP and the steps of the MFMA tap contraction -- B operand, neighbourhood row, fold of the
// accumulator tiles -- are rf_flca_adjoint.h's, shared with rf_flca.hip and rf_flca_pyramid*.hip.  Slabs are split by gram2_slabs
// and added in order by launch_reduce_rows (rf_train.hip): two runs give the same bits.  FlcaBwdPlan is the scratch layout,
// launch_flca_backward the schedule.
#include "rf_flca_adjoint.h"
#include "rf_guidance.h"      // fast_sigmoid: the gates recomputed here are the forward's

namespace rf {
namespace {

// dch partial: partial[(b * nblk + blk) * C + c] = sum over the block's pixels of dz x.  dz has dz_bstride floats between images,
// x is [B][C][P]; the caller's nblk fixes the order of the sum
__global__ void __launch_bounds__(256) flca_dch_kernel(const float* __restrict__ dz, int64_t dz_bstride, const float* __restrict__ xs, float* __restrict__ partial,
                                                       int C, int P, int nblk) {
    const int blk = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float* d = dz + (size_t)b * dz_bstride + (size_t)c * P;
    const float* x = xs + ((size_t)b * C + c) * P;
    const int per = (P + nblk - 1) / nblk, lo = blk * per, hi = (lo + per < P) ? lo + per : P;
    float s[1] = {0.f};
    for (int p = lo + threadIdx.x; p < hi; p += 256) s[0] = fmaf(d[p], x[p], s[0]);
    __shared__ float red[4];
    block_sums<1>(s, red);
    if (threadIdx.x == 0) partial[((size_t)b * nblk + blk) * C + c] = s[0];
}

// squeeze-excite backward, one workgroup per image (a single workgroup walking the images in turn took 120 us per stage):
// in: pooled sums partial (forward: flca partial / P = mean), dch partials;  out: dm[b][c] / P and the image's CONTRIBUTION to the
// gradients of se.1.{w,b}, se.3.{w,b} in contrib[b][hid C | hid | C hid | C] (the order of the four tensors in the flat gradient
// buffer), summed over the images in order by reduce_partials_kernel: deterministic.  Both tables are summed the way the
// forward's flca_se_kernel sums its own (se_column_sums).
__global__ void __launch_bounds__(256) flca_se_bwd_kernel(const float* __restrict__ pool_partial, int pool_nblk, const float* __restrict__ dch_partial, int dch_nblk,
                                                          const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w3, const float* __restrict__ b3,
                                                          float* __restrict__ dmP, float* __restrict__ contrib, int C, int hid, int P) {
    __shared__ float mean[512], ds3[512], hv[64], dh[64], part[256];
    const size_t b = blockIdx.x;
    se_column_sums(pool_partial, b, pool_nblk, C, part, [&](int c, float t) { mean[c] = t / (float)P; });
    se_column_sums(dch_partial, b, dch_nblk, C, part, [&](int c, float t) { ds3[c] = t; });      // dch, until the gate is known
    se_hidden(w1, b1, mean, hv, C, hid);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float chv = se_gate(w3, b3, hv, c, hid);
        ds3[c] = ds3[c] * chv * (1.0f - chv);
    }
    float* gw1 = contrib + b * (size_t)(2 * C * hid + hid + C);
    float* gb1 = gw1 + (size_t)hid * C;
    float* gw3 = gb1 + hid;
    se_adjoint(w1, w3, mean, hv, ds3, dh, gw1, gb1, gw3, gw3 + (size_t)C * hid, dmP + b * C, C, hid, P);
}

struct FlcaBwdArgs {
    const float* feat; const float* guide; const float* dz; int64_t dz_bstride; const float* ch; const float* dmP;
    const float* w_low; const float* w_high; const float* w_chr; const float* alpha; const float* beta; const float* gamma;
    float* dfeat;
    float* abg_partial;             // [slab][A tile][3]
    int C, h, w, accumulate;
};

// Spatial part and tap sums in ONE kernel (w % 4 == 0):
//   dfeat = dxs S;   ds_low = alpha dS a_l (1 - a_l),  ds_high = beta dS (1 - a_h^2),  ds_chr = gamma dS a_c (1 - a_c)   (dS = dxs feat)
// and the tap sums dW[c][tap] = sum_p ds[c][p] g[p + tap], without the three ds tensors ever reaching memory.  A lane owns channel
// 16 ti + r and the 4 pixels of its pixel group kq -- the A-operand layout of the tap contraction below -- recomputes the three
// gates of its channel at those pixels from the guidance neighbourhood (36 weights of the channel in registers), writes dfeat,
// and feeds ds_low / ds_high / ds_chr straight into the MFMAs whose B rows are the TAPS: G[c][col] = sum_p ds_k[c][p] * plane_k[p + tap] is a contraction over pixels; lane (r, kq) of
// the B operand loads tap r of its plane at the lane's 4 pixels, four accumulator tiles per A tile: low x plane 0, high x plane 1,
// chroma x plane 2, chroma x plane 3 (columns 0-8 = the 3 x 3 window).  dz and feat are read once, dfeat written once, nothing
// else touches HBM (the guidance planes are cache resident).
// partial[(slab * C + c) * 36 + {low 0-8, high 9-17, chroma 18-35}], slabs reduced in order by reduce_partials_kernel;
// abg_partial[(slab * gridDim.y + ti) * 3 + k].
__global__ void __launch_bounds__(256) flca_bwd_fused_kernel(FlcaBwdArgs a, float* __restrict__ partial, int slab_px, int slabs_per_image) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int slab = blockIdx.x, ti = blockIdx.y;
    const int img = slab / slabs_per_image, sl = slab - img * slabs_per_image;
    const int h = a.h, w = a.w, P = h * w, C = a.C;
    const int n_lo = sl * slab_px, n_hi = (n_lo + slab_px < P) ? n_lo + slab_px : P;
    const bool cvalid = 16 * ti + r < C;
    const int c = cvalid ? 16 * ti + r : C - 1;
    float wl[9], wh[9], wc[18];
#pragma unroll
    for (int t = 0; t < 9; ++t) { wl[t] = a.w_low[c * 9 + t]; wh[t] = a.w_high[c * 9 + t]; wc[t] = a.w_chr[c * 18 + t]; wc[9 + t] = a.w_chr[c * 18 + 9 + t]; }
    const float al = *a.alpha, be = *a.beta, ga = *a.gamma;
    const float chv = a.ch[(size_t)img * C + c], dm = a.dmP[(size_t)img * C + c];
    const float* dzr = a.dz + (size_t)img * a.dz_bstride + (size_t)c * P;
    const float* fr = a.feat + ((size_t)img * C + c) * P;
    float* dfr = a.dfeat + ((size_t)img * C + c) * P;
    const float* gpl = a.guide + (size_t)img * 4 * P;
    const int tdy = r < 9 ? r / 3 - 1 : 0, tdx = r < 9 ? r % 3 - 1 : 0;      // this lane's tap (B operand rows 9-15 are zero)
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float sa = 0.f, sb = 0.f, sg = 0.f;
    for (int n0 = n_lo + wave * 16; n0 < n_hi; n0 += 64) {
        const int nn = n0 + 4 * kq;
        const bool ok = nn < n_hi;
        const int n = ok ? nn : n_lo;
        const int y = n / w, x = n - y * w;
        const float4 dz4 = ld4(dzr + n), f4 = ld4(fr + n);
        float bv[4][4];
        tap_operand<4>(gpl, P, h, w, y, x, r, tdy, tdx, ok, bv);
        // gates of the lane's channel at its 4 pixels: pre-activations from the 3 x 6 neighbourhood of each plane
        float s_l[4] = {0.f, 0.f, 0.f, 0.f}, s_h[4] = {0.f, 0.f, 0.f, 0.f}, s_c[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int yy = y + dy - 1;
            float nb[4][6];
            neighbour_row<4>(gpl, P, w, x, yy, yy >= 0 && yy < h, nb);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float k0 = wl[dy * 3 + dx], k1 = wh[dy * 3 + dx], k2 = wc[dy * 3 + dx], k3 = wc[9 + dy * 3 + dx];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s_l[q] = fmaf(k0, nb[0][q + dx], s_l[q]);
                    s_h[q] = fmaf(k1, nb[1][q + dx], s_h[q]);
                    s_c[q] = fmaf(k3, nb[3][q + dx], fmaf(k2, nb[2][q + dx], s_c[q]));
                }
            }
        }
        const float dzv[4] = {dz4.x, dz4.y, dz4.z, dz4.w}, fv[4] = {f4.x, f4.y, f4.z, f4.w};
        const float live = (ok && cvalid) ? 1.0f : 0.f;
        float dsl[4], dsh[4], dsc[4], df[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float a_l = fast_sigmoid(s_l[q]), a_h = 2.0f * fast_sigmoid(2.0f * s_h[q]) - 1.0f, a_c = fast_sigmoid(s_c[q]);
            const float dxs = live * fmaf(dzv[q], chv, dm);
            df[q] = dxs * (1.0f + al * a_l + be * a_h + ga * a_c);
            const float dS = dxs * fv[q];
            dsl[q] = al * dS * a_l * (1.0f - a_l);
            dsh[q] = be * dS * (1.0f - a_h * a_h);
            dsc[q] = ga * dS * a_c * (1.0f - a_c);
            sa = fmaf(dS, a_l, sa); sb = fmaf(dS, a_h, sb); sg = fmaf(dS, a_c, sg);
        }
        if (ok && cvalid) {
            float4 o = make_float4(df[0], df[1], df[2], df[3]);
            if (a.accumulate) { const float4 p = ld4(dfr + n); o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
            *reinterpret_cast<float4*>(dfr + n) = o;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsl[m], bv[0][m], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsh[m], bv[1][m], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsc[m], bv[2][m], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsc[m], bv[3][m], acc[3], 0, 0, 0);
        }
    }
    __shared__ float red[4][16][17];
    fold_tap_tiles<4>(acc, red, wave, kq, r, ti, C, [=](int t, int gi, int jj) { return partial + ((size_t)slab * C + gi) * 36 + 9 * t + jj; });
    // dalpha, dbeta, dgamma of the workgroup (red is free again after the barrier)
    __syncthreads();
    float abg[3] = {sa, sb, sg};
    block_sums<3>(abg, &red[0][0][0]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.abg_partial[((size_t)slab * gridDim.y + ti) * 3 + k] = abg[k];
    }
}

// the 36 tap sums of a channel -> the three weight gradients: low [C][9], high [C][9], chroma [C][2][9]
__global__ void __launch_bounds__(256) flca_taps_scatter_kernel(const float* __restrict__ sums, float* __restrict__ g_low, float* __restrict__ g_high,
                                                                float* __restrict__ g_chr, int C) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < C * 36; e += gridDim.x * 256) {
        const int c = e / 36, t = e % 36;
        if (t < 9) g_low[c * 9 + t] += sums[e];
        else if (t < 18) g_high[c * 9 + t - 9] += sums[e];
        else g_chr[c * 18 + t - 18] += sums[e];
    }
}

__global__ void __launch_bounds__(256) flca_abg_kernel(const float* __restrict__ partial, int nrec, float* __restrict__ ga, float* __restrict__ gb, float* __restrict__ gg) {
    __shared__ float part[3][256];
    float s[3] = {0.f, 0.f, 0.f};
    for (int k = threadIdx.x; k < nrec; k += 256) {
#pragma unroll
        for (int t = 0; t < 3; ++t) s[t] += partial[(size_t)k * 3 + t];
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) part[t][threadIdx.x] = s[t];
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = 0.f;
        for (int q = 0; q < 256; ++q) v += part[threadIdx.x][q];      // fixed order
        float* o = threadIdx.x == 0 ? ga : threadIdx.x == 1 ? gb : gg;
        *o += v;
    }
}

// The scratch of launch_flca_backward as float offsets: the one layout behind the size query and the run.
struct FlcaBwdPlan {
    int dnblk, hid, nti;                 // flca_dch_kernel's pixel blocks; squeeze-excite hidden width; 16-channel tiles
    int slab_px, per_image, nslab;       // pixel slabs of the fused kernel (gram2_slabs)
    size_t n_se;                         // floats of one image's contribution to the four squeeze-excite gradients
    size_t abg;                          // [nslab][nti][3]     dalpha, dbeta, dgamma of each workgroup of the fused kernel
    size_t dch_part;                     // [B][dnblk][C]
    size_t dmP;                          // [B][C]
    size_t se_contrib;                   // [B][n_se]
    size_t taps;                         // [nslab][C][36]      the tap sums of each slab
    size_t sums;                         // [C][36]             ... added over the slabs
    size_t floats;
};

FlcaBwdPlan flca_bwd_plan(int B, int C, int h, int w) {
    FlcaBwdPlan p;
    const int P = h * w;
    p.dnblk = chan_sum_nblk(P); p.hid = flca_hidden(C); p.nti = cdiv(C, 16);
    gram2_slabs(B, P, p.nti, &p.slab_px, &p.per_image);
    p.nslab = B * p.per_image;
    p.n_se = (size_t)2 * C * p.hid + p.hid + C;
    Bump b;
    p.abg = b.off((size_t)p.nslab * p.nti * 3);
    p.dch_part = b.off((size_t)B * p.dnblk * C);
    p.dmP = b.off((size_t)B * C);
    p.se_contrib = b.off((size_t)B * p.n_se);
    p.taps = b.off((size_t)p.nslab * C * 36);
    p.sums = b.off((size_t)C * 36);
    p.floats = b.used;
    return p;
}

}  // namespace

size_t flca_bwd_scratch_floats(int B, int C, int h, int w) { return flca_bwd_plan(B, C, h, w).floats; }

int launch_flca_dch(const float* dz, int64_t dz_bstride, const float* x, float* partial, int nblk, int B, int C, int P, hipStream_t st) {
    flca_dch_kernel<<<dim3((unsigned)nblk, (unsigned)C, (unsigned)B), 256, 0, st>>>(dz, dz_bstride, x, partial, C, P, nblk);
    return check_launch("flca_dch");
}

int launch_flca_backward(const float* feat, const float* guide, const float* xs, const float* dz, int64_t dz_bstride, const float* ch,
                         const float* pool_partial, int pool_nblk, const FlcaPrm& prm, const FlcaGrad& grd, float* dfeat, int accumulate,
                         float* scratch, size_t scratch_floats, int B, int C, int h, int w, hipStream_t st) {
    RF_CHECK_ARG(C <= 512 && B <= 65535 && w % 4 == 0, "flca backward: C=%d, w=%d unsupported", C, w);
    // the fused kernel moves 16 bytes per lane; the training step hands it nothing else (workspace granules, packed widths)
    const char* const misaligned = !aligned16(dz) ? "dz" : dz_bstride % 4 != 0 ? "the image stride of dz" : !aligned16(feat) ? "feat"
                                   : !aligned16(dfeat) ? "dfeat" : !aligned16(guide) ? "guide" : nullptr;
    RF_CHECK_ARG(!misaligned, "flca backward: %s is not 16-byte aligned", misaligned);
    const FlcaBwdPlan p = flca_bwd_plan(B, C, h, w);
    RF_CHECK_ARG(p.floats <= scratch_floats, "flca backward: scratch of %zu floats, %zu needed", scratch_floats, p.floats);
    const int P = h * w;
    float *abg = scratch + p.abg, *dch_part = scratch + p.dch_part, *dmP = scratch + p.dmP, *se_contrib = scratch + p.se_contrib,
          *taps = scratch + p.taps, *sums = scratch + p.sums;
    // the four squeeze-excite tensors follow each other in the flat gradient buffer (registry order, sizes multiples of 4)
    RF_CHECK_ARG(grd.se.se1_b == grd.se.se1_w + (size_t)p.hid * C && grd.se.se3_w == grd.se.se1_b + p.hid && grd.se.se3_b == grd.se.se3_w + (size_t)C * p.hid,
                 "flca backward: the gradients of se.1.weight, se.1.bias, se.3.weight, se.3.bias must be contiguous");
    ProfScope prof(st, "flca_backward(fused)", 2.0 * 36 * (double)B * C * P + 200.0 * B * C * P, 12.0 * (double)B * C * P + 8.0 * B * C * P);
    // squeeze-excite part: dch -> per-image MLP adjoint -> dm, the four se gradients (all four reduced at once)
    RF_TRY(launch_flca_dch(dz, dz_bstride, xs, dch_part, p.dnblk, B, C, P, st));
    flca_se_bwd_kernel<<<B, 256, 0, st>>>(pool_partial, pool_nblk, dch_part, p.dnblk, prm.se.se1_w, prm.se.se1_b, prm.se.se3_w, prm.se.se3_b, dmP,
                                          se_contrib, C, p.hid, P);
    RF_TRY(launch_reduce_rows(se_contrib, grd.se.se1_w, B, p.n_se, 1, st));
    // spatial part + tap sums in one kernel, then the last step of its sums
    FlcaBwdArgs a{feat, guide, dz, dz_bstride, ch, dmP, prm.w_low, prm.w_high, prm.w_chr, prm.alpha, prm.beta, prm.gamma, dfeat, abg, C, h, w, accumulate};
    flca_bwd_fused_kernel<<<dim3((unsigned)p.nslab, (unsigned)p.nti), 256, 0, st>>>(a, taps, p.slab_px, p.per_image);
    flca_abg_kernel<<<1, 256, 0, st>>>(abg, p.nslab * p.nti, grd.alpha, grd.beta, grd.gamma);
    RF_TRY(launch_reduce_rows(taps, sums, p.nslab, (size_t)C * 36, 0, st));
    flca_taps_scatter_kernel<<<cdiv(C * 36, 256), 256, 0, st>>>(sums, grd.w_low, grd.w_high, grd.w_chr, C);
    return check_launch("flca_backward (fused)");
}

}  // namespace rf

