// Attention middle for levels where the qkv 1x1 stays a separate GEMM (C = 64, 128), in a translation unit of its own: hipcc
// compiles a unit's kernels together, and an edit here must not move the registers of the other fused kernels (rf_fused.hip,
// rf_fused_tile.h; tools/isa_same.py --kernel shows it).
//   qkv [B,3C,h,w] (HBM) -> depthwise 3x3 -> { Gram partials of (q, k) per head ; v -> HBM }
// i.e. attn_front_kernel with phase A replaced by staging halo'd qkv tiles from HBM: the depthwise-convolved
// q and k never exist in memory (un-fused: dwconv writes 3C and the Gram kernel reads 2C of it back).
// Round r stages q tile r (planes 0-15) and k tile r (planes 16-31) -- heads never straddle a 16-channel tile
// here -- and the v rounds 32 channels each; a round's 16-byte loads are issued before the previous round's phase B
// and land in LDS after it (hardware zero fill outside the image, like rf_conv3x3.hip).
// (AttnMidArgs: rf_common.h)
#include <cstdio>
#include <cstdlib>
#include "rf_common.h"
#include "rf_fused_tile.h"

namespace rf {

// A workgroup's tiles are consecutive and run DOWN a column of the tile grid, and the six halo'd rows of a plane live in a
// circular window of LDS rows (image row y in slot (y + 1) mod 6): a tile directly below the previous one of the same round
// finds its first two rows already there and stages only the four new ones -- 4.5 instead of 6.75 floats read per pixel
// and channel (the measured HBM traffic of this kernel had been 2.1-2.3 x its algorithmic bytes).
//
// The staging plan is made ONCE per workgroup.  Tile origins are multiples of 4 rows, so the window turns by whole PAIRS of
// slots: pair p = slots {2p, 2p + 1} holds halo rows {rb, rb + 1} of a tile, rb = 2 ((p - k) mod 3) with k = (2 ty) mod 3, and
// a sliding tile keeps exactly the pair with rb = 0.  An element of the plan is therefore (plane, row of the pair, 4-pixel
// group): 32 x 2 x 18 = 1152 of them = 4.5 per thread, the same for all three pairs.  Per element and workgroup:
//     rel   byte offset of (row of the pair, group) + the plane, relative to the pair's first row at the tile's column x0 - 4;
//           bit 31 = outside the image in x (refreshed when the workgroup changes its tile column, i.e. hardly ever)
//     lp    its LDS address in pair 0 (the other pairs: + 2 HC, + 4 HC floats, an immediate offset)
// and per (round, tile) step nothing but wave-uniform scalars: the byte offset of each pair's first row and whether its two
// rows lie inside the image.  A load is `rel + that offset` -- one add -- and a store has no address arithmetic at all.
// Everything else a step or a round needs advances by adds as well: tile (tx, ty), k, the tile's byte offset, the wave's first
// stencil row in the window, the round's source planes, its weights, its v planes and its partial.  No integer multiply, divide
// or modulo is left in the round loop up to and including its tile steps (gfx950 listing: none between the round loop's header
// and the step loop's end).  What remains is the epilogue of a Gram round, once per round after its last tile: the row
// addresses of the cross-wave reduction (five v_mul_lo_u32 by ROWW and one v_mad_u64_u32), deliberately not hoisted -- they
// were spilled when they were.
template <int C>
__global__ void __launch_bounds__(256, 2) attn_mid_kernel(AttnMidArgs a) {
    using namespace fused;
    constexpr int NQT = C / 16;          // Gram rounds
    constexpr int NVP = C / PART;        // v rounds
    constexpr int NR = NQT + NVP;
    constexpr int PSG = fused::PSG, PSV = 448, ROWW = 4 * 16 + 2;
    constexpr int G4 = HC / 4;                           // 18 groups of 4 pixels per halo'd row
    constexpr int PE = PART * 2 * G4;                    // 16-byte elements of one slot pair (32 planes x 2 rows x 18)
    constexpr int KP = (PE + 255) / 256;                 // ... per thread: 4, and a fifth for waves 0-1
    static_assert(PE == 4 * 256 + 128 && KP == 5, "the last element of a pair belongs to waves 0 and 1");
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) float mid[PART * PSG + 8];
    __shared__ float wd_l[3 * C * 9], bd_l[3 * C];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int slab = blockIdx.x, b = blockIdx.y;
    const int h = a.h, w = a.w, P = h * w;
    const float* qb = a.qkv + (size_t)b * 3 * C * P;
    float* vb = a.v + (size_t)b * C * P;
    for (int i = tid; i < 3 * C * 9; i += 256) wd_l[i] = a.wd[i];
    for (int i = tid; i < 3 * C; i += 256) bd_l[i] = a.bd[i];

    const int tiles_y = a.ntiles / a.tiles_x;
    const int per = (a.ntiles + a.nslab - 1) / a.nslab;
    // Rounds are the OUTER loop and this workgroup's tiles the inner one, so one register set holds the Gram tile of the
    // round across all tiles (a round index into a register array would go to scratch); (round, tile) is one flattened
    // pipeline: the next step's loads are issued before this step's phase B.
    const int t_begin = slab * per;
    if (t_begin >= a.ntiles) {                             // (whole workgroup) no tiles: its Gram partials are zero
        if ((int)blockIdx.z == 0)
            for (int i = tid; i < NQT * 16 * ROWW; i += 256) a.partial[((size_t)b * a.nslab + slab) * NQT * 16 * ROWW + i] = 0.f;
        return;
    }
    const int ntw = (t_begin + per < a.ntiles) ? per : a.ntiles - t_begin;      // tiles of this workgroup: t_begin, t_begin + 1, ...
    // rounds of this workgroup: every round is independent (its own Gram partial or its own v channels), so a launch with few
    // slabs (one frame) spreads them over gridDim.z workgroups per slab -- same partials, same results
    const int rd_lo = (int)blockIdx.z * NR / a.rgroups, rd_hi = ((int)blockIdx.z + 1) * NR / a.rgroups;

    // ---- the plan (once): round rd < NQT stages q tile rd | k tile rd, C - 16 planes apart; rd >= NQT v channels 32 (rd - NQT) ..
    const unsigned w4 = (unsigned)w * 4u, w16 = w4 * 4u;                 // bytes of one image row / of a tile's four
    const unsigned kjump = (unsigned)((C - 16) * P) * 4u;                 // planes 16-31 of a Gram round are the k tile
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);             // the wave index in a scalar register
    const bool wave_lo = wave_u < 2;                                      // owns a fifth element
    unsigned rel[KP];
    float* lp[KP];
    int key[KP];              // group | plane << 5 | row of the pair << 10; group 31: no such element
    {
        const bool gram = rd_lo < NQT;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int e = tid + 256 * k;
            const int pl = e / (2 * G4), rem = e % (2 * G4), sub = rem / G4, g = rem % G4;
            const bool there = e < PE;
            key[k] = there ? g | (pl << 5) | (sub << 10) : 31;
            rel[k] = there ? (unsigned)sub * w4 + 16u * (unsigned)g + (unsigned)pl * (unsigned)P * 4u + (gram && pl >= 16 ? kjump : 0u) : 0u;
            lp[k] = mid + (there ? pl * (gram ? PSG : PSV) + sub * HC + 4 * g : 0);
        }
    }
    auto set_column = [&](int x0) {      // x = x0 - 4 + 4 g inside the image?  (w % 4 == 0: whole groups)
        const int glo = x0 == 0 ? 1 : 0, gtop = ((w - x0) >> 2) + 1, gn = (gtop < G4 ? gtop : G4) - glo;
#pragma unroll
        for (int k = 0; k < KP; ++k) rel[k] = (rel[k] & ~OOB) | ((unsigned)((key[k] & 31) - glo) < (unsigned)gn ? 0u : OOB);
    };
    auto to_v_rounds = [&]() {           // the Gram rounds are over: 32 adjacent planes at stride PSV
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int pl = (key[k] >> 5) & 31;
            rel[k] -= pl >= 16 ? kjump : 0u;
            lp[k] -= pl * (PSG - PSV);
        }
    };
    // first plane of a round's source, in floats: 16 rd P (Gram) or (2C + 32 (rd - NQT)) P (v); carried from round to round
    const size_t P16 = (size_t)16 * P, PV = (size_t)PART * P, base_v0 = (size_t)2 * C * P, span_g = (size_t)(C + 16) * P, total = (size_t)3 * C * P;
    size_t r_base = rd_lo < NQT ? (size_t)rd_lo * P16 : base_v0 + (size_t)(rd_lo - NQT) * PV;
    auto next_base = [&](int rd_next) { return rd_next < NQT ? r_base + P16 : rd_next == NQT ? base_v0 : r_base + PV; };
    auto round_rsrc = [&](size_t base, bool gram) {
        // num_records = the planes this round touches (q tile + k tile, C planes apart; or 32 v planes), never the rest of the
        // tensor: it must stay below the OOB offset 2^31 for the zero fill to work on large frames (3C planes of a 1424x2128
        // level are 2.3 GB)
        const size_t span = gram ? span_g : PV, rest = total - base;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qb) + base, 0, (int)((span < rest ? span : rest) * 4), 0x00020000);
    };

    // the tile in flight: its loads are issued one step ahead and stored at the top of its own step
    int n_tx = t_begin / tiles_y, n_ty = t_begin % tiles_y;
    const int tx0 = n_tx, ty0 = n_ty, k0 = (2 * ty0) % 3;
    const unsigned tb0 = ((unsigned)(ty0 * TH) * (unsigned)w + (unsigned)(tx0 * TW)) * 4u;
    int n_k = k0;             // (2 n_ty) mod 3: halo row 0 of the tile sits in slot 2 n_k
    unsigned n_tb = tb0;      // byte offset of pixel (y0, x0) inside a plane
    bool n_full = true;       // all six rows are staged (first tile of a round or of a column)
    int col_tx = n_tx;        // the tile column `rel` is valid for
    // LDS offset of this wave's first stencil row (halo row `wave` of the tile, slot (2 k + wave) mod 6): + 4 slots per tile down
    const int ro_top = wave_u * HC, ro_0 = ((2 * k0 + wave_u) % HR) * HC;
    int n_ro = ro_0;
    // what a lane adds to a tile's and a round's offsets, once: its v output pixels, its v weights, its Gram weights, its partial
    float* const v_lane = vb + (size_t)kq * P + (size_t)wave * w + 4 * j;
    const size_t P4 = (size_t)4 * P;
    size_t v_round = rd_lo > NQT ? (size_t)(rd_lo - NQT) * PV : 0;          // first plane of the round's 32 v channels
    int vw_off = (2 * C + (rd_lo > NQT ? (rd_lo - NQT) * PART : 0) + kq) * 9, vb_off = 2 * C + (rd_lo > NQT ? (rd_lo - NQT) * PART : 0) + kq;
    int gw_off = (16 * rd_lo + j) * 9;                                       // q channel 16 rd + j; its k channel: + 9 C
    float* dstp = a.partial + (((size_t)b * a.nslab + slab) * NQT + (rd_lo < NQT ? rd_lo : 0)) * 16 * ROWW;
    set_column(n_tx * TW);

    float4 stg[3][KP];
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    // an element this tile does not stage: its registers hold nothing from here on (no instruction; without it the old value
    // stays live around the step loop and every staging register is copied once per step)
    auto forget = [](float4& v) { asm volatile("" : "=v"(v.x), "=v"(v.y), "=v"(v.z), "=v"(v.w)); };
    auto load_tile = [&](const __amdgpu_buffer_rsrc_t rs) {      // the tile (n_*): every pair it does not find in LDS
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int d = p - n_k + (p < n_k ? 3 : 0);           // rb / 2
            if (n_full || d != 0) {
                const int ya = n_ty * TH - 1 + 2 * d;            // image row of the pair's first row
                const bool va = (unsigned)ya < (unsigned)h, vb2 = (unsigned)(ya + 1) < (unsigned)h;
                // byte offset of (ya, x0 - 4): the tile's, one row up, 0 / 2 / 4 rows down
                const unsigned rowbase = n_tb - w4 - 16u + (d == 0 ? 0u : d == 1 ? 2u * w4 : w16);
                if (va && vb2) {
#pragma unroll
                    for (int k = 0; k < KP; ++k)
                        if (k < KP - 1 || wave_lo) {      // (outside the image in x: bit 31 of rel, see the bound below)
                            const u32x4_t v4 = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(rel[k] + rowbase), 0, 0);
                            stg[p][k] = make_float4(__uint_as_float(v4.x), __uint_as_float(v4.y), __uint_as_float(v4.z), __uint_as_float(v4.w));
                        } else forget(stg[p][k]);
                } else {                                         // the image's first or last rows: zero fill by row
                    const unsigned ia = va ? 0u : OOB, ib = vb2 ? 0u : OOB;
#pragma unroll
                    for (int k = 0; k < KP; ++k)
                        if (k < KP - 1 || wave_lo) {
                            // an offset marked OOB is >= 2^31 - w4 - 16 (rowbase is at least -(w4 + 16), at the image's first
                            // row and column), and num_records < 2.0e9 (attn_mid_shape_ok) lies below that: zero fill
                            const unsigned off = (rel[k] | ((key[k] & 1024) ? ib : ia)) + rowbase;
                            const u32x4_t v4 = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
                            stg[p][k] = make_float4(__uint_as_float(v4.x), __uint_as_float(v4.y), __uint_as_float(v4.z), __uint_as_float(v4.w));
                        } else forget(stg[p][k]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < KP; ++k) forget(stg[p][k]);
            }
        }
    };

    const int ntw1 = ntw - 1;
    f32x4 gq = {0.f, 0.f, 0.f, 0.f};
    float nq = 0.f, nk = 0.f;                              // sums of squares on the VALU (see attn_front_kernel)
    load_tile(round_rsrc(r_base, rd_lo < NQT));
    __syncthreads();                                      // wd_l / bd_l visible
    for (int rd = rd_lo; rd < rd_hi; ++rd) {
        const __amdgpu_buffer_rsrc_t rs = round_rsrc(r_base, rd < NQT);
        // Gram round: lane (i = j, kq) owns channel j of the q tile and of the k tile for the whole round
        float wq[9], wk[9], bq = 0.f, bk = 0.f;
        if (rd < NQT) {
            const int cq = 16 * rd + j;
#pragma unroll
            for (int t = 0; t < 9; ++t) { wq[t] = wd_l[gw_off + t]; wk[t] = wd_l[gw_off + 9 * C + t]; }
            bq = bd_l[cq]; bk = bd_l[C + cq];
            gw_off += 16 * 9;
        } else {
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[t] = wk[t] = 0.f;
        }
        for (int ti = 0; ti < ntw; ++ti) {
            // this step's tile is the one in flight
            const int x0 = n_tx * TW, y0 = n_ty * TH;
            const int yo = y0 + wave;
            const int c_k = n_k, c_ro = n_ro;
            const bool c_full = n_full;
            const size_t c_px = n_tb >> 2;                // y0 w + x0
            lds_barrier();                                // everyone is done reading the previous step
#pragma unroll
            for (int p = 0; p < 3; ++p)                   // its rows into their slots (a sliding tile's first pair is already there)
                if (c_full || p != c_k) {
#pragma unroll
                    for (int k = 0; k < KP; ++k)
                        if (k < KP - 1 || wave_lo) *reinterpret_cast<float4*>(lp[k] + 2 * p * HC) = stg[p][k];
                }
            // LDS row offsets of this wave's three stencil rows (halo rows wave .. wave + 2 of this tile)
            int ro[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int r = c_ro + dy * HC;
                ro[dy] = r - (r >= HR * HC ? HR * HC : 0);
            }
            if (ti < ntw1) {                              // next step: same round, the tile below / on top of the next column
                ++n_ty; n_k = n_k == 0 ? 2 : n_k - 1; n_tb += w16; n_full = false;
                n_ro += 4 * HC; n_ro -= n_ro >= HR * HC ? HR * HC : 0;
                if (n_ty == tiles_y) { n_ty = 0; ++n_tx; n_k = 0; n_tb = (unsigned)(n_tx * TW) * 4u; n_full = true; n_ro = ro_top; }      // a new column starts with a full window
                if (n_tx != col_tx) { col_tx = n_tx; set_column(n_tx * TW); }
                load_tile(rs);
            } else if (rd + 1 < rd_hi) {                  // next round, first tile
                n_tx = tx0; n_ty = ty0; n_k = k0; n_tb = tb0; n_full = true; n_ro = ro_0;
                if (n_tx != col_tx) { col_tx = n_tx; set_column(n_tx * TW); }
                if (rd + 1 == NQT) to_v_rounds();
                load_tile(round_rsrc(next_base(rd + 1), rd + 1 < NQT));
            }
            lds_barrier();
            if (rd < NQT) {
                // Gram: lane (i = j, kq) owns channel j of the q tile and of the k tile at pixels x0 + 16 st + 4 kq + m
#pragma unroll 1
                for (int st = 0; st < 4; ++st) {
                    const int xo = x0 + 16 * st + 4 * kq;
                    const bool ok = yo >= a.ylo && yo < a.yhi && xo >= a.xlo && xo < a.xhi;
                    float qa[4], kb[4];
                    stencil4<Edge::Wide>(mid + j * PSG + 16 * st + 4 * kq + 4, ro, j, wq, bq, qa);
                    stencil4<Edge::Wide>(mid + (16 + j) * PSG + 16 * st + 4 * kq + 4, ro, j, wk, bk, kb);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float qv = ok ? qa[m] : 0.f, kv = ok ? kb[m] : 0.f;
                        gq = __builtin_amdgcn_mfma_f32_16x16x4f32(qv, kv, gq, 0, 0, 0);
                        nq = fmaf(qv, qv, nq);
                        nk = fmaf(kv, kv, nk);
                    }
                }
            } else {
                const int xo = x0 + 4 * j;
                if (yo < h && xo < w) {
                    size_t so = v_round + c_px;           // channel 32 vp + 4 s (+ kq: v_lane), pixel (y0, x0) (+ wave, 4 j: v_lane)
#pragma unroll
                    for (int s = 0; s < PART / 4; ++s) {
                        const int hc = 4 * s + kq;
                        float v[4];
                        stencil4<Edge::Dpp>(mid + hc * PSV + 4 * j + 4, ro, j, wd_l + vw_off + 36 * s, bd_l[vb_off + 4 * s], v);
                        *reinterpret_cast<float4*>(v_lane + so) = make_float4(v[0], v[1], v[2], v[3]);
                        so += P4;
                    }
                }
            }
        }
        if (rd < NQT) {
            // ---- cross-wave reduction of this round's Gram tile in a fixed order, one partial per workgroup
            // (the next step's data is still in registers: mid is free between the two barriers)
            __syncthreads();
            float* red = mid;                 // [4 waves][16][ROWW]
            int kq_ = kq;                     // opaque here: the row addresses below were hoisted out of the round loop and SPILLED
            asm volatile("" : "+v"(kq_));     // (scratch traffic next to the prefetched loads of the next round)
            float nqt = nq, nkt = nk;         // channel j's sums of squares over the four kq lanes
            nqt += __shfl_xor(nqt, 16); nqt += __shfl_xor(nqt, 32);
            nkt += __shfl_xor(nkt, 16); nkt += __shfl_xor(nkt, 32);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 4 * kq_ + q;
                float* rr = red + (wave * 16 + row) * ROWW;
                rr[j] = gq[q];
                if (row == j) { rr[64] = nqt; rr[65] = nkt; }
            }
            __syncthreads();
            // a partial row = this q tile against its own k tile | three zero key tiles | the two sums of squares.  The zero
            // tiles are stored as zeros, not summed from zero-filled LDS: ((0 + 0) + 0) + 0 is the same +0, and the fill was a
            // 12-trip loop with two divisions per trip, every round
            float* dst = dstp;
            dstp += 16 * ROWW;
            auto sum4 = [&](int i) { return ((red[i] + red[16 * ROWW + i]) + red[2 * 16 * ROWW + i]) + red[3 * 16 * ROWW + i]; };
            int t_ = tid;
            asm volatile("" : "+v"(t_));      // opaque for the same reason
            const int ri = (t_ >> 4) * ROWW + (t_ & 15);
            dst[ri] = sum4(ri);
            dst[ri + 16] = 0.f; dst[ri + 32] = 0.f; dst[ri + 48] = 0.f;
            if (t_ < 32) {
                const int si = (t_ >> 1) * ROWW + 64 + (t_ & 1);
                dst[si] = sum4(si);
            }
            gq = (f32x4){0.f, 0.f, 0.f, 0.f}; nq = 0.f; nk = 0.f;
        } else {
            v_round += PV; vw_off += PART * 9; vb_off += PART;
        }
        r_base = next_base(rd + 1);
    }
}

// slabs of the image (= workgroups per image): enough of them to fill the chip at a batch of 8, at most 8 tiles each;
// a function of the image only (batch-invariant reduction order)
int attn_mid_plan(int h, int w, int* nslab, size_t* partial_floats, int B, int C) {
    const int ntiles = cdiv(w, fused::TW) * cdiv(h, fused::TH);
    int per = ntiles / 64;                      // (finer slabs -- ntiles / 128 -- are 40 % faster for ONE frame and 9 % slower for a
                                                // batch of 8: the tile loop is what hides this kernel's load latency)
    if (per < 1) per = 1;
    if (per > 8) per = 8;
    *nslab = cdiv(ntiles, per);
    *partial_floats = (size_t)B * *nslab * (C / 16) * 16 * 66;
    return RF_OK;
}

static bool attn_mid_shape_ok(int C, int h, int w) {
    return (C == 64 || C == 128) && (w % 4 == 0) && ((double)(C + 16) * h * w * 4.0 < 2.0e9);      // byte offsets inside one round's buffer window stay below 2^31
}
bool attn_mid_supported(int C, int heads, int h, int w) { return heads_fit_tiles(C, heads) && attn_mid_shape_ok(C, h, w); }

int launch_attn_mid(AttnMidArgs a, int C, hipStream_t st) {
    const int B = a.B, h = a.h, w = a.w;
    RF_CHECK_ARG(attn_mid_shape_ok(C, h, w) && B <= 65535, "attn_mid: unsupported shape C=%d %dx%d", C, h, w);
    RF_CHECK_ARG(aligned16(a.qkv) && aligned16(a.v), "attn_mid: buffers must be 16-byte aligned");
    a.tiles_x = cdiv(w, fused::TW);
    a.ntiles = a.tiles_x * cdiv(h, fused::TH);
    if (!(a.yhi > 0 && a.yhi < h)) a.yhi = h;
    if (!(a.xhi > 0 && a.xhi < w)) a.xhi = w;
    a.rgroups = ((long)a.nslab * B < 256) ? 3 : 1;          // C / 16 + C / 32 rounds: 6 (C = 64) or 12 (C = 128)
    const double px = (double)B * h * w;
    ProfScope prof(st, C == 64 ? "attn_mid_kernel<64>" : "attn_mid_kernel<128>", px * (54.0 * C + 4.0 * C * 16), px * 16.0 * C);
    const dim3 grid((unsigned)a.nslab, (unsigned)B, (unsigned)a.rgroups);
    if (C == 64) attn_mid_kernel<64><<<grid, 256, 0, st>>>(a);
    else attn_mid_kernel<128><<<grid, 256, 0, st>>>(a);
    return check_launch("attn_mid");
}

}  // namespace rf
