// Dense 3x3 convolution (padding 1) as an implicit GEMM on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32; K = 4 input channels per instruction), with the Winograd F(4,3) minimal filtering
// algorithm along x: the lane's 4 output pixels of one kernel row cost 6 products instead of 12,
//   m = (G g) * (B^T d),   y = A^T m
//   G g   = (g0/4, -(g0+g1+g2)/6, -(g0-g1+g2)/6, g0/24+g1/12+g2/6, g0/24-g1/12+g2/6, g2): done when the weights
//           are packed (rf_pack.hip), 18 taps per k-set instead of 9
//   B^T d = (4d0-5d2+d4, (d4-4d2)+(d3-4d1), (d4-4d2)-(d3-4d1), (d4-d2)+2(d3-d1), (d4-d2)-2(d3-d1), 4d1-5d3+d5):
//           12 VALU operations on the two ds_read_b128 of a (k-set, input row), next to 6*NCO MFMAs
//   A^T m = (m0+m1+m2+m3+m4, (m1-m2)+2(m3-m4), (m1+m2)+4(m3+m4), (m1-m2)+8(m3-m4)+m5): once per tile, in the epilogue
// A chunk takes half the MFMAs of the direct form.  Rounding error 2.2 x the direct form's (f32 simulated against
// f64: 5e-7 on O(0.2) outputs at Cin = 32, 1.3e-6 at Cin = 256), inside every parity tolerance.
//
// Workgroup = NWV waves; it owns a (NWV*RW*RPW rows) x (64/RW cols) pixel tile and NCO*16 output
// channels, and is persistent over several such tiles.  Per 8-input-channel chunk the halo'd input tile and the matching slice of the
// lane-ordered packed weights sit in LDS; every wave then walks 2 k-sets x 18 transformed taps.
//   * B operand: lane (kq, j) owns 4 consecutive pixels of one row.  Two ds_read_b128 per
//     (k-set, input row) fetch the 6 neighbours those pixels need; their transform B^T d is the operand of the
//     row's 6 taps, so one LDS read feeds 6 * NCO MFMAs per output row it reaches.  The plane stride (448 floats)
//     keeps the four kq planes on disjoint LDS slots.
//   * A operand: ds_read_b32, lane-linear (conflict-free).
//   * D: channels 16t + 4kq + r for the lane's 4 pixels -> 16-byte stores.
// Pipeline: LDS is double buffered; the global loads of chunk c+1 (input tile with zero
// padding, weight slice) are issued into registers before the MFMA block of chunk c and written
// to the other LDS buffer after it: one barrier per chunk, HBM/L2 latency hidden behind the
// matrix pipe.  Per-thread gather offsets are computed once, not per chunk.
// Fused: Bayer pack on the input side (a1, the embedding conv reads the mosaic directly),
// input/output clamps, bias, LeakyReLU(0.2), and the pixel-unshuffle (Downsample, a8) or
// pixel-shuffle (conv_out + PixelShuffle, a10) store.
#include <cstdio>
#include <cstdlib>
#include "rf_common.h"

namespace rf {

static constexpr int KC = 8;        // input channels per LDS chunk
static constexpr int kKsCounters = 4096;   // floats at the head of Conv3x3Args::ks_scratch that hold the tickets of a K-split launch
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// NWV = waves per workgroup: 8 on wide images (the 18-tap weight slice is shared by twice the waves, so that two
// waves per SIMD fit the 160 KB of LDS with one workgroup per CU), 4 for the narrow-image tile shapes.
// KS (small launches only, one tile per workgroup): the input-channel chunks are split over gridDim.z workgroups.  Each writes
// its partial tile (after the output transform, before bias and activation) to scratch; the LAST one to arrive -- a ticket per
// (image, tile, output group) -- adds the partials in split order (deterministic whatever the arrival order), applies bias /
// activation / clamp and stores.  One 16 x 16 frame at level 3 is a chain of 32 chunk barriers on 4 workgroups otherwise.
//
// L0 (wide level-0 launches with Cin <= 32, rows of whole aligned float4s; chosen by plan_conv3x3, nothing else changes):
//   bit 0: the output group's complete Winograd weight set (Cin/4 k-sets x 18 taps x NCO x 64 floats, at most 72 KB) is loaded
//          into LDS once per workgroup and stays there; the chunk loop stages input only.
//   bit 1: the halo'd input tile is staged by row segments: the 64 interior floats of a (channel, row) as 16-byte loads,
//          the two halo columns as dword loads (V4PT + 1 memory instructions per thread and chunk instead of EPT = 19 or 10,
//          and a tile plan of the same length).  The LDS layout, and with it every MFMA operand, is the generic path's.
template <int NCO, int LOG2_RW, int RPW, int NWV, bool KS = false, int L0 = 0>
__global__ void __launch_bounds__(64 * NWV, (NWV >= 8 || NCO >= 3) ? 1 : 2) conv3x3_kernel(Conv3x3Args a, int ngroups, int tiles_x, int ntiles, int vec) {
    constexpr int NTHR = 64 * NWV;
    constexpr int TAPS = 18;                 // transformed taps per k-set (3 kernel rows x 6)
    constexpr int NM = 6;                    // Winograd products per lane and output tile
    constexpr int RW = 1 << LOG2_RW;         // rows one MFMA pixel group spans (narrow images)
    constexpr int TW = 64 / RW;              // tile width
    constexpr int TH = NWV * RW * RPW;       // tile height: a wave owns RPW row groups (RPW = 2 for few output channels:
                                             // twice the MFMAs per barrier and per staged weight, 17 % less halo)
    static_assert(RPW == 1 || RW == 1, "two row groups per wave only with one row per group");
    constexpr int RS = TW + 8;               // LDS row stride
    constexpr int PS = ((TH + 2) * RS + 63) / 64 * 64;   // LDS plane stride in floats (multiple of 64)
    constexpr bool RESW = (L0 & 1) != 0, ROWS = (L0 & 2) != 0;
    static_assert(L0 == 0 || (!KS && LOG2_RW == 0), "the level-0 path: wide tiles, no input-channel split");
    constexpr int NIN = KC * (TH + 2) * (TW + 2);       // staged input elements per chunk
    constexpr int NV4 = KC * (TH + 2) * (TW / 4);       // ROWS: interior float4 per chunk ...
    constexpr int V4PT = ROWS ? (NV4 + NTHR - 1) / NTHR : 0;   // ... per thread; then one halo element per thread
    static_assert(!ROWS || 2 * KC * (TH + 2) <= NTHR, "one halo element per thread");
    constexpr int EPT = ROWS ? V4PT + 1 : (NIN + NTHR - 1) / NTHR;   // staged input items per thread
    constexpr int WSL = 2 * TAPS * NCO * 64;            // floats of one chunk's weight slice
    constexpr int NW4 = WSL / 4;                        // staged weight float4 per chunk
    constexpr int WPT = RESW ? 0 : (NW4 + NTHR - 1) / NTHR;
    constexpr int BUF = KC * PS + (RESW ? 0 : WSL);     // floats per LDS buffer
    constexpr int MAXCH = 32 / KC;                      // RESW: chunks whose weights are resident (Cin <= 32)
    __shared__ __attribute__((aligned(16))) float lds[2 * BUF + (RESW ? MAXCH * WSL : 0)];
    __shared__ __attribute__((aligned(16))) float bias_l[NCO * 16];       // the epilogue must not read global memory: a load there is followed by
                                             // s_waitcnt vmcnt(0), one exposed round trip per bias value and tile

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int rowj = j / (16 / RW), cg = j % (16 / RW);
    const int grp = blockIdx.x % ngroups;
    const int wg = blockIdx.x / ngroups;
    const int b = blockIdx.y;
    const int h = a.h, w = a.w;
    const int NT = (a.Cout + 15) >> 4;
    const int t0 = grp * NCO;
    const int nchunks_all = (a.Cin + KC - 1) / KC;
    const int ksplit = KS ? (int)gridDim.z : 1, kz = KS ? (int)blockIdx.z : 0;
    const int ch_lo = KS ? (int)((long)kz * nchunks_all / ksplit) : 0, ch_hi = KS ? (int)((long)(kz + 1) * nchunks_all / ksplit) : nchunks_all;
    const float* xb = a.x + (size_t)b * a.x_bstride;
    const size_t chunk_stride = a.unshuffle_in ? (size_t)(KC / 4) * 4 * h * w : (size_t)KC * h * w;

    // ---- staging plan.  Every per-chunk instruction of the staging path is a memory instruction with
    // precomputed operands: f32 MFMA time and VALU time add up on this hardware (measured: ~250 VALU per
    // chunk cost 10 %), so the chunk loop carries no address arithmetic, selects or masks.
    //   * input: buffer_load_dword through a per-chunk descriptor (base = first plane of the chunk,
    //     num_records = the planes that exist).  Zero padding, "no element" and channels beyond Cin
    //     are out-of-range offsets -> the hardware returns 0.
    //   * weights: buffer_load_dwordx4, same trick for output tiles beyond Cout.
    // Element i of this thread is halo'd-tile element idx = tid + NTHR i = (channel cl, row r, col c).
    constexpr unsigned OOB = 0x80000000u;   // > any num_records (images are < 2 GiB, checked by the launcher)
    int prc[EPT];             // (cl << 16) | (r << 8) | c, or -1 = no element
    short loff[EPT];          // LDS float offset inside a buffer ("no element" -> a spare slot in the plane padding,
                              // so the LDS writes need no predicate; 128 spare slots, 2 threads of different waves each)
    static_assert(PS - (TH + 2) * RS >= (ROWS ? 32 : 16), "plane padding holds the dummy slots");
    const int dummy = ROWS ? (tid & 7) * PS + (TH + 2) * RS + 4 * ((tid >> 3) & 7)    // four floats
                           : (tid & 7) * PS + (TH + 2) * RS + ((tid >> 3) & 15);   // shared only by threads of different waves
    if constexpr (ROWS) {
        // item i < V4PT: float4 q of halo'd row (cl, r), columns 1 + 4q .. 4 + 4q; item V4PT: column 0 or TW + 1 of row tid / 2
#pragma unroll
        for (int i = 0; i < V4PT; ++i) {
            const int idx = tid + NTHR * i;
            const int c = 1 + 4 * (idx % (TW / 4));
            const int r = (idx / (TW / 4)) % (TH + 2);
            const int cl = idx / ((TW / 4) * (TH + 2));
            prc[i] = idx < NV4 ? (cl << 16) | (r << 8) | c : -1;
            loff[i] = (short)(idx < NV4 ? cl * PS + r * RS + c : dummy);
        }
        const int c = (tid & 1) * (TW + 1), r = (tid >> 1) % (TH + 2), cl = (tid >> 1) / (TH + 2);
        prc[V4PT] = cl < KC ? (cl << 16) | (r << 8) | c : -1;
        loff[V4PT] = (short)(cl < KC ? cl * PS + r * RS + c : dummy);
    } else {
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int idx = tid + NTHR * i;
            const int c = idx % (TW + 2);
            const int r = (idx / (TW + 2)) % (TH + 2);
            const int cl = idx / ((TW + 2) * (TH + 2));
            prc[i] = idx < NIN ? (cl << 16) | (r << 8) | c : -1;
            loff[i] = (short)(idx < NIN ? cl * PS + r * RS + c : dummy);
        }
    }
    unsigned wvoff[WPT > 0 ? WPT : 1];      // weight byte offsets inside one chunk's packed slice
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int idx = tid + NTHR * i;
        const int l4 = idx % 16;
        const int t = (idx / 16) % NCO;
        const int kt = idx / (16 * NCO);          // ks * TAPS + dy * (TAPS / 3) + j
        const bool ok = idx < NW4 && t0 + t < NT;
        wvoff[i] = ok ? (unsigned)(((kt * NT + t0 + t) * 64 + l4 * 4) * 4) : OOB;
    }
    const int w_chunk_bytes = 2 * TAPS * NT * 64 * 4;
    const size_t plane_bytes = (size_t)h * w * 4;      // one packed-resolution plane

    unsigned voff[EPT];       // current tile: byte offset inside the chunk's planes, OOB = zero
    int x0 = 0, y0 = 0;       // origin of the tile the plan (and the loads in flight) belong to
    auto plan_tile = [&](int tile) {
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        x0 = tx * TW;
        y0 = ty * TH;
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            int e = prc[i];
            asm volatile("" : "+v"(e));   // opaque: nothing derived from the element id stays live across the MFMA blocks
            const int cl = e >> 16;
            const int y = y0 - 1 + ((e >> 8) & 255), x = x0 - 1 + (e & 255);
            const bool ok = e >= 0 && (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w;
            // packed channel cl = 2*i + jj of mosaic plane 0 lives at (2y+i, 2x+jj); KC = 8 covers 2 mosaic planes
            const int off_m = ((cl >> 2) * 2 * h + 2 * y + ((cl >> 1) & 1)) * (2 * w) + 2 * x + (cl & 1);
            const int off_p = (cl * h + y) * w + x;
            voff[i] = ok ? (unsigned)(4 * (a.unshuffle_in ? off_m : off_p)) : OOB;
        }
    };
    float xin[ROWS ? 1 : EPT];
    u32x4 xin4[ROWS ? V4PT : 1];          // ROWS: the interior float4s (xin[0] = the halo element)
    float4 win[WPT > 0 ? WPT : 1];
    auto load_chunk = [&](int ch) {
        // planes of this chunk that exist: min(KC, Cin - ch*KC) channel planes (mosaic input: 4 channels = 1 plane of 4hw)
        const int cl_lim = min(KC, a.Cin - ch * KC);
        const float* src = xb + (size_t)ch * chunk_stride;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(src), 0, (int)(a.unshuffle_in ? (size_t)(cl_lim / 4) * 4 * plane_bytes : (size_t)cl_lim * plane_bytes), 0x00020000);
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.wp) + (size_t)ch * (w_chunk_bytes / 4), 0, w_chunk_bytes, 0x00020000);
        if constexpr (ROWS) {
            // a float4 lies inside the image or outside it as a whole (w % 4 == 0, checked by the launcher), and so do the planes
#pragma unroll
            for (int i = 0; i < V4PT; ++i) xin4[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)voff[i], 0, 0);
            xin[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, (int)voff[V4PT], 0, 0));
        } else {
#pragma unroll
            for (int i = 0; i < EPT; ++i) xin[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, (int)voff[i], 0, 0));
        }
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)wvoff[i], 0, 0);
            win[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    };
    auto store_chunk = [&](int buf) {
        float* li = lds + buf * BUF;
        float* lw = li + KC * PS;
        if constexpr (ROWS) {
            // the interior starts at column 1 (the halo column in front of it is what the B-operand reads expect): dword writes
#pragma unroll
            for (int i = 0; i < V4PT; ++i) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float v = __uint_as_float(xin4[i][g]);
                    if (a.clamp_in) v = fminf(fmaxf(v, 0.f), 1.f);
                    li[loff[i] + g] = v;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < (ROWS ? 1 : EPT); ++i) {
            float v = xin[i];
            if (a.clamp_in) v = fminf(fmaxf(v, 0.f), 1.f);      // uniform; only the clamp_io embedding conv
            li[loff[ROWS ? V4PT : i]] = v;
        }
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int idx = tid + NTHR * i;
            if (idx < NW4) *reinterpret_cast<float4*>(lw + idx * 4) = win[i];   // [kt][t][64] is linear in idx
        }
    };

    f32x4 acc[RPW][NCO][NM];     // [row group][output tile][Winograd product m_0..5]

    // ---- persistent over a contiguous range of tiles: the first chunk of the next tile is prefetched
    // behind the last MFMA block of the current one, so only the very first load is exposed
    // (tiles wg, wg + nwg, ...: the workgroups running at one time cover a compact band of the image that moves
    // down it -- contiguous runs per workgroup put them 8 rows x 2^k bytes apart and lost 10 % at 512 x 512)
    const int nwg = gridDim.x / ngroups;
    int tile = wg;
    const int tile_end = ntiles;
    if (tile >= tile_end) return;
    if (tid < NCO * 16) {
        const int co = 16 * t0 + tid;
        bias_l[tid] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
    }
    plan_tile(tile);
    load_chunk(ch_lo);
    if constexpr (RESW) {
        // resident weights: chunk ch at lds + 2 BUF + ch WSL, laid out [kt][t][64] as the staged slice is
        float* lw = lds + 2 * BUF;
        const int n4 = nchunks_all * NW4;
        for (int idx = tid; idx < n4; idx += NTHR) {
            const int l4 = idx % 16, t = (idx / 16) % NCO, kt = idx / (16 * NCO);      // kt = (2 ch + ks) * TAPS + tap
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t0 + t < NT) v = *reinterpret_cast<const float4*>(a.wp + ((size_t)(kt * NT + t0 + t) * 64 + l4 * 4));
            *reinterpret_cast<float4*>(lw + idx * 4) = v;
        }
    }
    store_chunk(0);
    __syncthreads();
    int buf = 0;
    float* outb = a.out + (size_t)b * a.out_bstride;
    for (; tile < tile_end; tile += nwg) {
        const int ex0 = x0, ey0 = y0;                  // this tile's origin (the plan moves on before the epilogue)
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
            for (int t = 0; t < NCO; ++t)
#pragma unroll
                for (int g = 0; g < NM; ++g) acc[rr][t][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ch = ch_lo; ch < ch_hi; ++ch) {
            const bool last = ch + 1 == ch_hi;
            const bool more = !last || tile + nwg < tile_end;
            const int nch = last ? ch_lo : ch + 1;
            if (last && more) plan_tile(tile + nwg);
            if (more) load_chunk(nch);                  // in flight during the MFMA block below
            const float* lds_in = lds + buf * BUF;
            const float* lds_w = RESW ? lds + 2 * BUF + ch * WSL : lds_in + KC * PS;
            const int nks = (a.Cin - ch * KC > 4) ? 2 : 1;   // a 4-channel tail (the embedding conv) skips the empty k-set
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks >= nks) break;
                const float* lp = lds_in + (ks * 4 + kq) * PS + (wave * RW * RPW + rowj) * RS + 4 * cg;
#pragma unroll
                for (int ir = 0; ir < RPW + 2; ++ir) {          // input row group ir feeds output row groups ir-2 .. ir
                    const float4 lo = *reinterpret_cast<const float4*>(lp + ir * RS);
                    const float4 hi = *reinterpret_cast<const float4*>(lp + ir * RS + 4);
                    float d[NM];
                    {
                        const float p = fmaf(-4.f, lo.z, hi.x), q = fmaf(-4.f, lo.y, lo.w);      // d4 - 4 d2, d3 - 4 d1
                        const float c2 = hi.x - lo.z, e2 = lo.w - lo.y;                         // d4 - d2,   d3 - d1
                        d[0] = fmaf(4.f, lo.x, fmaf(-5.f, lo.z, hi.x));
                        d[1] = p + q; d[2] = p - q;
                        d[3] = fmaf(2.f, e2, c2); d[4] = fmaf(-2.f, e2, c2);
                        d[5] = fmaf(4.f, lo.y, fmaf(-5.f, lo.w, hi.y));
                    }
#pragma unroll
                    for (int rr = 0; rr < RPW; ++rr) {
                        const int dy = ir - rr;
                        if (dy < 0 || dy > 2) continue;
#pragma unroll
                        for (int j4 = 0; j4 < TAPS / 3; ++j4) {
                            const float* wl = lds_w + ((ks * TAPS + dy * (TAPS / 3) + j4) * NCO) * 64 + lane;
#pragma unroll
                            for (int t = 0; t < NCO; ++t) {
                                acc[rr][t][j4] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[t * 64], d[j4], acc[rr][t][j4], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            if (more) store_chunk(buf ^ 1);             // the other buffer: last read one barrier ago
            __syncthreads();
            buf ^= 1;
        }

        // ---- epilogue of this tile (its stores drain behind the next tile's first MFMA block)
        int kq_ = kq;                      // opaque per tile: keeps the bias values and output row pointers from being
        asm volatile("" : "+v"(kq_));      // hoisted out of the tile loop (they would stay live across every MFMA block)
        const int x = ex0 + 4 * cg;
        // output transform A^T m of the lane's F(4,3) tiles: u[r][g], channel 16 (t0 + t) + 4 kq + r, pixel x + g
        auto transform = [&](int rr, int t, float (&u)[4][4]) {
            const f32x4* mm = acc[rr][t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s12 = mm[1][r] + mm[2][r], d12 = mm[1][r] - mm[2][r], s34 = mm[3][r] + mm[4][r], d34 = mm[3][r] - mm[4][r];
                u[r][0] = (mm[0][r] + s12) + s34;
                u[r][1] = fmaf(2.f, d34, d12);
                u[r][2] = fmaf(4.f, s34, s12);
                u[r][3] = fmaf(8.f, d34, d12) + mm[5][r];
            }
        };
        // bias, activation, clamp.  The (uniform) choice of the activation is made once per 16 values: written per value it stayed
        // a chain of six scalar branches around every one of them, and the bias a ds_read_b32 + lgkmcnt(0) per channel.
        auto finish = [&](int t, float (&v)[4][4]) {
            const float4 b4 = *reinterpret_cast<const float4*>(bias_l + 16 * t + 4 * kq_);
            const float bs[4] = {b4.x, b4.y, b4.z, b4.w};
            auto each = [&](auto f) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int g = 0; g < 4; ++g) v[r][g] = f(v[r][g] + bs[r]);
            };
            if (a.act == 1) each([](float u) { return u > 0.f ? u : 0.2f * u; });
            else if (a.act == 2) each([](float u) { return fmaxf(u, 0.f); });
            else if (a.act == 3) each([](float u) { return gelu_fast(u); });
            else if (a.act == 4) each([](float u) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * u)); });      // tanh
            else each([](float u) { return u; });
            if (a.clamp_out) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int g = 0; g < 4; ++g) v[r][g] = fminf(fmaxf(v[r][g], 0.f), 1.f);
            }
        };
        auto store_tile = [&](int t, int y, const float (&v)[4][4]) {
            const int cobase = 16 * (t0 + t) + 4 * kq_;
            if (a.store == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = cobase + r;
                    if (co >= a.Cout) continue;
                    float* o = outb + ((size_t)co * h + y) * w + x;
                    if (vec) {
                        *reinterpret_cast<float4*>(o) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
                    } else {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            if (x + g < w) o[g] = v[r][g];
                    }
                }
            } else if (a.store == 1) {
                // Downsample: out[4*co + 2*(y&1) + (x&1)][y>>1][x>>1]
                const int h2 = h >> 1, w2 = w >> 1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = cobase + r;
                    if (co >= a.Cout) continue;
                    float* o = outb + (((size_t)(4 * co + 2 * (y & 1))) * h2 + (y >> 1)) * w2 + (x >> 1);
                    const size_t ps = (size_t)h2 * w2;
                    if (vec) {
                        *reinterpret_cast<float2*>(o) = make_float2(v[r][0], v[r][2]);
                        *reinterpret_cast<float2*>(o + ps) = make_float2(v[r][1], v[r][3]);
                    } else {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            if (x + g < w) o[(size_t)(g & 1) * ps + (g >> 1)] = v[r][g];
                    }
                }
            } else {
                // conv_out + PixelShuffle(2): GEMM row 4*c + 2*i + jj -> out[c][2y+i][2x+jj]
                if (cobase >= a.Cout) return;
                const int c = cobase >> 2;
                float* op = outb + (size_t)c * 4 * h * w;
                const int w2 = 2 * w;
                if (vec) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        float* row = op + (size_t)(2 * y + i) * w2 + 2 * x;
                        *reinterpret_cast<float4*>(row) = make_float4(v[2 * i][0], v[2 * i + 1][0], v[2 * i][1], v[2 * i + 1][1]);
                        *reinterpret_cast<float4*>(row + 4) = make_float4(v[2 * i][2], v[2 * i + 1][2], v[2 * i][3], v[2 * i + 1][3]);
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (x + g < w) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                op[(size_t)(2 * y + (r >> 1)) * w2 + 2 * (x + g) + (r & 1)] = v[r][g];
                        }
                }
            }
        };
        if constexpr (!KS) {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int y = ey0 + (wave * RPW + rr) * RW + rowj;
                if (y >= h || x >= w) continue;
#pragma unroll
                for (int t = 0; t < NCO; ++t) {
                    if (t0 + t >= NT) break;
                    float v[4][4];   // [r][g]
                    transform(rr, t, v);
                    finish(t, v);
                    store_tile(t, y, v);
                }
            }
        } else {
            // partial tiles [split][image][channel][y][x] (the launcher checks w % 4 == 0), then the ticket
            unsigned* counter = reinterpret_cast<unsigned*>(a.ks_scratch) + ((size_t)b * ntiles + tile) * ngroups + grp;
            float* part = a.ks_scratch + kKsCounters;
            const size_t split_stride = (size_t)a.B * a.Cout * h * w;
            float* mine = part + (size_t)kz * split_stride + (size_t)b * a.Cout * h * w;
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int y = ey0 + (wave * RPW + rr) * RW + rowj;
                if (y >= h || x >= w) continue;
#pragma unroll
                for (int t = 0; t < NCO; ++t) {
                    if (t0 + t >= NT) break;
                    float v[4][4];
                    transform(rr, t, v);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int co = 16 * (t0 + t) + 4 * kq_ + r;
                        if (co < a.Cout) *reinterpret_cast<float4*>(mine + ((size_t)co * h + y) * w + x) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
                    }
                }
            }
            __shared__ unsigned ticket;
            // release (every workgroup: its partial tile is written back before the ticket is taken) / acquire (the last workgroup
            // only: it must not read stale lines).  A full __threadfence() on both sides made EVERY workgroup invalidate its L2.
            // The returns below leave the tile loop for good.  That is sound because a split launch gives every workgroup exactly
            // one tile: plan_conv3x3 sets Conv3x3Plan::ksplit above 1 only where grid.x == ngroups * ntiles (nwg == ntiles).
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __syncthreads();
            if (tid == 0) ticket = atomicAdd(counter, 1u);
            __syncthreads();
            if (ticket != (unsigned)(ksplit - 1)) return;  // not the last split of this tile
            if (tid == 0) *counter = 0u;                   // ready for the next launch (stream order)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int y = ey0 + (wave * RPW + rr) * RW + rowj;
                if (y >= h || x >= w) continue;
#pragma unroll
                for (int t = 0; t < NCO; ++t) {
                    if (t0 + t >= NT) break;
                    float v[4][4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int co = 16 * (t0 + t) + 4 * kq_ + r;
                        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (co < a.Cout) {
                            const float* src = part + (size_t)b * a.Cout * h * w + ((size_t)co * h + y) * w + x;
                            for (int z = 0; z < ksplit; ++z) {          // split order, whatever the arrival order
                                const float4 pz = *reinterpret_cast<const float4*>(src + (size_t)z * split_stride);
                                sum.x += pz.x; sum.y += pz.y; sum.z += pz.z; sum.w += pz.w;
                            }
                        }
                        v[r][0] = sum.x; v[r][1] = sum.y; v[r][2] = sum.z; v[r][3] = sum.w;
                    }
                    finish(t, v);
                    store_tile(t, y, v);
                }
            }
            return;
        }
    }
}

size_t conv3x3_ksplit_counter_bytes() { return (size_t)kKsCounters * sizeof(float); }
size_t conv3x3_ksplit_floats(int B, int Cout, int h, int w) {
    return ((long)B * h * w <= 16384) ? (size_t)kKsCounters + (size_t)8 * B * Cout * h * w : 0;
}

// THE selection rule: argument checks, then the instantiation <NCO, LOG2_RW, RPW, NWV, KS, L0>, its geometry and its profiler key
// (the name of the unsplit kernel: a split launch differs in grid.z alone).  No HIP call, no launch; a plan exists only for
// arguments launch_conv3x3 accepts.
int plan_conv3x3(const Conv3x3Args& a, Conv3x3Plan* p) {
    RF_CHECK_ARG(a.B > 0 && a.B <= 65535 && a.Cin > 0 && a.Cout > 0 && a.h > 0 && a.w > 0, "conv3x3: bad sizes");
    RF_CHECK_ARG(a.store == 0 || (a.store == 1 && a.h % 2 == 0 && a.w % 2 == 0) || (a.store == 2 && a.Cout % 4 == 0),
                 "conv3x3: store mode %d incompatible with Cout=%d h=%d w=%d", a.store, a.Cout, a.h, a.w);
    RF_CHECK_ARG(!a.unshuffle_in || a.Cin == 4, "conv3x3: the packed-mosaic input path takes exactly 4 channels");
    RF_CHECK_ARG((double)a.Cin * a.h * a.w * 4.0 < 2.0e9, "conv3x3: image too large for 32-bit gather offsets");
    const int NT = cdiv(a.Cout, 16);
    int nco = 4;
    if (NT % 4 != 0) nco = (NT % 3 == 0) ? 3 : (NT % 2 == 0 ? 2 : (NT == 1 ? 1 : 4));
    // A launch that would put fewer than 128 workgroups on the 256 CUs (one frame at the deep levels: 8 tiles x 4 output
    // groups at level 3) trades per-workgroup efficiency for parallelism: 4x64 tiles on 4-wave workgroups and fewer output tiles
    // per workgroup.  Batches of 8 never come here (the grid already fills the chip).
    bool small = false;
    if (a.w > 32 && a.h >= 8) {
        const long big = (long)cdiv(a.w, 64) * cdiv(a.h, nco <= 2 ? 16 : 8) * cdiv(NT, nco) * a.B;
        if (big < 128) {
            small = true;
            const long t4 = (long)cdiv(a.w, 64) * cdiv(a.h, 4) * a.B;
            while (nco > 1 && t4 * cdiv(NT, nco) < 192) nco = (nco == 4 || nco == 2) ? nco / 2 : 1;
        }
    }
    *p = Conv3x3Plan{};
    p->nco = nco;
    p->ngroups = cdiv(NT, nco);
    p->vec = (a.w % 4 == 0) && aligned16(a.out) && (a.out_bstride % 4 == 0);
    // Wide images (w > 32): 8 waves share one 18-tap weight slice, one workgroup per CU; a wave owns one pixel row of 64, or two
    // where 16 rows exist and NCO = 2 (16x64 tile, 144 MFMAs per barrier).  One output tile: 16 waves of one row each (103 registers,
    // four waves per SIMD cover each other's LDS and barrier waits) beat 8 waves of two rows by 7 %; with NCO = 2 the same shape
    // spills at the 128-register cap.  Small launches (few pixels: one frame at levels 2-3) and images under 8 rows take 4-wave
    // workgroups on 4x64 tiles, more of them; narrow images 4-wave tiles of 8x32 or 16x16 pixels.
    p->log2_rw = a.w > 32 ? 0 : (a.w > 16 ? 1 : 2);
    const bool wide = p->log2_rw == 0 && !small && a.h >= 8, rows16 = wide && nco <= 2 && a.h >= 16;
    p->nwv = !wide ? 4 : (rows16 && nco == 1) ? 16 : 8;
    p->rpw = (rows16 && nco == 2) ? 2 : 1;
    // The level-0 path (template argument L0 of the kernel) for the 16-row tiles: all of Cin in at most four chunks (resident
    // weights) and input rows made of whole, 16-byte aligned float4s.  The mosaic input of the embedding conv is gathered element
    // by element and stays on the generic path.
    p->l0 = (rows16 && a.Cin <= 32 && !a.unshuffle_in && a.w % 4 == 0 && aligned16(a.x) && a.x_bstride % 4 == 0) ? 3 : 0;
    // workgroups are persistent over the tiles of one (image, output group): one resident workgroup per CU
    p->tiles_x = cdiv(a.w, 64 >> p->log2_rw);
    p->ntiles = p->tiles_x * cdiv(a.h, (p->nwv * p->rpw) << p->log2_rw);
    const long total = (long)p->ntiles * p->ngroups * a.B;
    p->grid = dim3((unsigned)(p->ngroups * cdiv(p->ntiles, (int)((total + 255) / 256))), (unsigned)a.B);
    p->block = 64u * p->nwv;
    // Input-channel split (KS) of a 4-wave launch whose every tile has its own workgroup, grid.x == ngroups * ntiles: the kernel's
    // split epilogue returns from its tile loop on the strength of that.  Only for launches of at most 64 workgroups, split into
    // at most 256: a 256-workgroup launch split three ways was 2.2-2.8 x SLOWER (46 -> 103 us with release / acquire fences, 129 us
    // with a full fence on both sides): the hand-over costs every workgroup an L2 write-back
    const int nchunks = cdiv(a.Cin, KC);
    p->ksplit = 1;
    if (p->nwv == 4 && a.ks_scratch && p->vec && aligned16(a.ks_scratch) && total <= 64 && nchunks >= 8 && (long)p->grid.x == (long)p->ngroups * p->ntiles) {
        int S = nchunks / 4 < 8 ? nchunks / 4 : 8;
        while (S > 1 && total * S > 256) --S;
        if (S >= 2 && (size_t)kKsCounters + (size_t)S * a.B * a.Cout * a.h * a.w <= a.ks_floats) p->ksplit = S;
    }
    static_assert(64 <= kKsCounters, "a ticket per workgroup of the unsplit launch");
    p->ks = p->ksplit > 1;
    p->grid.z = (unsigned)p->ksplit;
    snprintf(p->key, sizeof(p->key), "conv3x3_kernel<%d, %d, %d, %d%s>", p->nco, p->log2_rw, p->rpw, p->nwv, p->l0 ? ", false, 3" : "");
    const double px = (double)a.B * a.h * a.w;
    p->flops = 18.0 * a.Cin * a.Cout * px;
    p->bytes = 4.0 * px * (a.Cin + a.Cout);
    return RF_OK;
}

// Every instantiation there is, one row each: its template arguments and its launch.
struct Conv3x3Inst {
    int nco, log2_rw, rpw, nwv, ks, l0;
    void (*launch)(const Conv3x3Args&, const Conv3x3Plan&, hipStream_t);
};
template <int NCO, int LOG2_RW, int RPW, int NWV, bool KS, int L0>
static void launch_inst(const Conv3x3Args& a, const Conv3x3Plan& p, hipStream_t st) {
    conv3x3_kernel<NCO, LOG2_RW, RPW, NWV, KS, L0><<<p.grid, p.block, 0, st>>>(a, p.ngroups, p.tiles_x, p.ntiles, p.vec);
}
#define RF_INST(...) {__VA_ARGS__, launch_inst<__VA_ARGS__>}
#define RF_NWV4(NCO, KS) RF_INST(NCO, 0, 1, 4, KS, 0), RF_INST(NCO, 1, 1, 4, KS, 0), RF_INST(NCO, 2, 1, 4, KS, 0)     // 4x64, 8x32, 16x16 tiles
static const Conv3x3Inst kInst[] = {
    RF_NWV4(1, false), RF_NWV4(2, false), RF_NWV4(3, false), RF_NWV4(4, false),
    RF_NWV4(1, true), RF_NWV4(2, true), RF_NWV4(3, true), RF_NWV4(4, true),
    RF_INST(1, 0, 1, 8, false, 0), RF_INST(2, 0, 1, 8, false, 0), RF_INST(3, 0, 1, 8, false, 0), RF_INST(4, 0, 1, 8, false, 0),      // 8x64
    RF_INST(2, 0, 2, 8, false, 0), RF_INST(2, 0, 2, 8, false, 3), RF_INST(1, 0, 1, 16, false, 0), RF_INST(1, 0, 1, 16, false, 3),    // 16x64
};

int launch_conv3x3(const Conv3x3Args& a, hipStream_t st) {
    Conv3x3Plan p;
    RF_TRY(plan_conv3x3(a, &p));
    ProfScope prof(st, p.key, p.flops, p.bytes);
    for (const Conv3x3Inst& r : kInst)
        if (r.nco == p.nco && r.log2_rw == p.log2_rw && r.rpw == p.rpw && r.nwv == p.nwv && r.ks == p.ks && r.l0 == p.l0) {
            r.launch(a, p, st);
            return check_launch("conv3x3");
        }
    RF_CHECK_ARG(false, "conv3x3: no kernel instantiation %s (split %d)", p.key, p.ksplit);
}

}  // namespace rf
