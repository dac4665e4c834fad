// The fused conv pair (conv3x3_pair.hip: x_a = lrelu(conv_a([x..])), x_b = lrelu(conv_b([x.., x_a])), reference
// src/framewright/processors/aesrgan_face.py:184-187) as a SLIDING WINDOW down a column of tiles.
//
// conv3x3_pair.hip evaluates both convs on one 16x32 region and delivers its 14x30 interior: the one-pixel ring is
// recomputed by the neighbours (+22 % MFMA work).  Here the vertical part of that ring is gone: a workgroup walks DOWN a column
// with a step of 16 rows, conv_b runs ONE ROW BEHIND conv_a, and the two x_a rows a tile shares with the next one stay in LDS:
//
//   tile ty:   conv_a rows  A = [16 ty, 16 ty + 15]          -> x_a rows A
//              conv_b rows  B = [16 ty - 1, 16 ty + 14]      needs x_a rows [16 ty - 2, 16 ty + 15] = carry (2 rows) + A
//   input halo rows [16 ty - 2, 16 ty + 16] (19 rows): conv_a row r reads r-1..r+1, conv_b row r the same
//
// so a tile delivers 16 rows of x_a and 16 rows of x_b for 16 rows of conv_a and conv_b work (16/16 instead of 14/16; the
// horizontal ring stays: 30 of 32 columns).  Wave w owns conv_a rows 2w, 2w+1 and conv_b rows 2w-1, 2w of the tile: five
// halo rows (2w .. 2w+4) of B fragments instead of four, conv_a reading them one row lower than conv_b.
// The x_a tile keeps the standard 18-row halo format with row 0 = image row 16 ty - 2: rows 0,1 come from the carry buffer
// (wave 7 copies rows 16,17 of the tile there after the x_a item), rows 2..17 are this tile's conv_a.  A workgroup whose
// run starts in the middle of a column first computes the last two conv_a rows of the tile above it (the warm-up below: four
// input rows per chunk and conv_a's weights, all chunks in flight at once) to obtain the carry rows; at the top of a column
// the carry is zero (= conv_b's zero padding).
#include <cstdlib>
#include <type_traits>
#include "fw_internal.h"
#include "conv_pair_common.h"

#ifndef FW_DMA_SLOT_W
#define FW_DMA_SLOT_W 2
#define FW_DMA_SLOT_A 6
#endif

namespace fw {

constexpr int PS_TH = TILE_H;          // 16 rows per step
constexpr int PS_TW = TILE_W - 2;      // 30 valid pixels per tile row
constexpr int PS_HALO_H = TILE_H + 3;  // 19 input rows
constexpr int PS_PIECES = PS_HALO_H * ROW_PIECES;  // 2584
constexpr int PS_EXTRA = PS_PIECES - ACT_ITERS * NWAVES * 64;  // 24 pieces beyond the 40 batched KiB: one more DMA of wave 0
constexpr int PS_REGION = 41 * 64;     // pieces per activation stage
constexpr int PS_CARRY = 2 * ROW_PIECES;  // two x_a rows
// every row of a tile is a valid output, pixels 0 / 31 of the region are the recompute ring; x_a row cr is row cr + 2 of the x_a tile
using SlideGeom = PairGeom<0, TILE_H - 1, 1, PS_TW, 2, 1, ROW_PIECES>;

constexpr int PS_WARM_ROWS = 4;                           // input rows 16 ty - 3 .. 16 ty: what conv_a rows 16 ty - 2, 16 ty - 1 read
constexpr int PS_WARM_PIECES = PS_WARM_ROWS * ROW_PIECES;  // 544 per chunk
constexpr int PS_WARM_KIB = 9;                            // DMA instructions per chunk: a batch of 5 and a batch of 4 (32 pad pieces)
constexpr int PS_WARM_SLOT = PS_WARM_KIB * 64;            // pieces per chunk slot in the second activation stage
constexpr int PS_WARM_CHUNKS = 4;                         // chunk slots: a warm-up batch

struct SlideSmem {
    static constexpr int W_REGION = PAIR_W_REGION;
    static constexpr int W_BASE = 2 * PS_REGION;
    static constexpr int CARRY = W_BASE + 2 * W_REGION;
    static constexpr int BIAS = CARRY + PS_CARRY;  // 64 floats: bias_a, bias_b
    static constexpr int TOTAL = BIAS + 16;        // 10144 pieces = 162304 bytes
};
static_assert(PS_WARM_CHUNKS * PS_WARM_SLOT <= PS_REGION && 2 * PS_WARM_CHUNKS == NWAVES, "warm-up batch: two waves per chunk slot");

// Phase slots of the stamped build (-DFW_PAIR_STAMP; tools/pair_tile_phases.py prints them per tile): 16 per wave, which is all
// of stamp_buffer(0).  0 - 9: a tile of the run; 10 - 14: the warm-up; 15: the wave's lifetime in 100 MHz ticks.
enum {
    ST_BARRIER = 0, ST_SHARED = 1, ST_XA_ITEM = 2, ST_XA_LDS = 3, ST_SETUP = 4, ST_VMCNT = 5, ST_XA_EPI = 6, ST_XB_EPI = 7,
    ST_CARRY = 8, ST_FIRST = 9, ST_W_BARRIER = 10, ST_W_MFMA = 11, ST_W_DMA = 12, ST_W_EPI = 13, ST_W_SETUP = 14, ST_LIFE = 15
};
#ifdef FW_PAIR_STAMP
#undef FW_STAMP_INIT
#undef FW_STAMP_FLUSH
#define FW_STAMP_INIT()                                                                  \
    unsigned long long stamp_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long stamp_last = __builtin_amdgcn_s_memtime();                        \
    const unsigned long long stamp_rt0 = __builtin_amdgcn_s_memrealtime()
#define FW_STAMP_FLUSH(buf)                                                                                 \
    do {                                                                                                    \
        stamp_acc[ST_LIFE] = __builtin_amdgcn_s_memrealtime() - stamp_rt0;                                  \
        if ((threadIdx.x & 63) == 0 && (buf))                                                               \
            for (int k_ = 0; k_ < 16; ++k_) atomicAdd((buf) + (threadIdx.x >> 6) * 16 + k_, stamp_acc[k_]); \
    } while (0)
#endif
static_assert(NWAVES == 8 && RPW == 2 && PS_EXTRA > 0 && PS_EXTRA <= 64, "written for 8 waves of 2 rows");
static_assert(SlideSmem::TOTAL * 16 <= 160 * 1024, "LDS");

template <typename T>
__global__ __launch_bounds__(64 * NWAVES, WAVES_PER_SIMD) void conv3x3_pair_slide_kernel(const ConvPairParams p) {
    using SM = SlideSmem;
    __shared__ __attribute__((aligned(16))) uint4 lds[SM::TOTAL];
    constexpr int NW = 4;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int q = lane & 15;
    const int sl = lane >> 4;
    FW_STAMP_INIT();  // phase stamps: diagnostic builds only (-DFW_PAIR_STAMP, conv_common.h)

    const TileBand band;
    const int tiles_x = (p.W + PS_TW - 1) / PS_TW;
    const int tiles_y = (p.H + PS_TH) / PS_TH;  // the last conv_b row H - 1 = 16 ty + 14 at the latest
    const int ntiles = tiles_x * tiles_y;        // column-major: t = tx * tiles_y + ty
    int t_lo, t_hi;
    band.range(ntiles, &t_lo, &t_hi);
    if (t_lo >= t_hi) return;
#ifdef FW_PS_NOWARM   // timing only (wrong pixels in the first conv_b row of a run that starts mid-column): what the warm-up tiles cost
    const int needs_warm = 0;
#else
    const int needs_warm = (t_lo % tiles_y) != 0;  // the run starts below the top of a column: conv_a of the tile above first
#endif
    const int na = p.na;
    const int nitems = (t_hi - t_lo) * (na + 1);

    // ---- per-lane DMA plan: 2560 pieces as five batched KiB per "virtual wave" v, pieces 2560..2583 as one more DMA of wave 0.
    //      FW_DMA_OLD_ONLY: the older wave of every SIMD (waves 0-3) issues the batches of virtual waves 2w and 2w+1 and the
    //      younger ones none: the younger wave is the critical path of every item, the older one waits at the barrier a
    //      quarter of the time. -----------------------------------------------------------------------------------------------
#ifndef FW_DMA_OLD_ONLY
#define FW_DMA_OLD_ONLY 0
#endif
    constexpr int NBB = FW_DMA_OLD_ONLY ? 2 : 1;                       // batches per issuing wave
    const bool issuer = FW_DMA_OLD_ONLY ? wave < NWAVES / 2 : true;    // wave-uniform
    auto vwave = [&](int bt) { return FW_DMA_OLD_ONLY ? 2 * wave + bt : wave; };
    auto piece_idx = [&](int bt, int i) { return i < ACT_ITERS ? (ACT_ITERS * vwave(bt) + i) * 64 + lane : ACT_ITERS * NWAVES * 64 + lane; };
    unsigned relb[NBB][ACT_ITERS];
    unsigned relb_x = 0;
    auto piece_off = [&](int idx) { return halo_piece_off(idx, p.W, p.in_cstride); };
#pragma unroll
    for (int bt = 0; bt < NBB; ++bt)
#pragma unroll
        for (int i = 0; i < ACT_ITERS; ++i) relb[bt][i] = piece_off(piece_idx(bt, i)) + (unsigned)(4 - i) * 1024u;
    relb_x = piece_off(piece_idx(0, ACT_ITERS));
    const bool extra_lane = wave == 0 && lane < PS_EXTRA;
    const unsigned lds_base = (unsigned)(size_t)(lds_ptr_t)lds;
    const char* in = reinterpret_cast<const char*>(p.in);
    const char* wa_b = reinterpret_cast<const char*>(p.wpk_a);
    const char* wb_b = reinterpret_cast<const char*>(p.wpk_b);
    const unsigned lane16 = lane * 16;
    const long chunk_bytes = p.in_pstride * 2;

    // tile t: first conv_a row R0 and compute-region origin column ox (one pixel left of the first valid output)
    auto origin = [&](int t, int* R0, int* ox) {
        const int tx = t / tiles_y, ty = t - tx * tiles_y;
        *R0 = ty * PS_TH;
        *ox = tx * PS_TW - 1;
    };

    unsigned f_ok = 0;            // bit bt * ACT_ITERS + i: piece i of batch bt is inside the image; bit 2 * ACT_ITERS: the extra piece
    bool f_all = true;
    const char* f_src = nullptr;  // halo origin (image row R0 - 2, column ox - 1) of (tile f_t, chunk f_c)
    int f_t = t_lo, f_c = 0;
    auto plan_tile = [&]() {
        int R0, ox;
        origin(f_t, &R0, &ox);
        f_src = in + ((long)(R0 - 2) * p.W + (ox - 1)) * p.in_cstride * 2;
        f_ok = 0;
        auto inside = [&](int idx) {
            const HaloPiece h = halo_piece(idx);
            return idx < PS_PIECES && (unsigned)(R0 - 2 + h.row) < (unsigned)p.H && (unsigned)(ox - 1 + h.px) < (unsigned)p.W;
        };
#pragma unroll
        for (int bt = 0; bt < NBB; ++bt)
#pragma unroll
            for (int i = 0; i < ACT_ITERS; ++i)
                if (inside(piece_idx(bt, i))) f_ok |= 1u << (bt * ACT_ITERS + i);
        if (inside(piece_idx(0, ACT_ITERS))) f_ok |= 1u << (2 * ACT_ITERS);
        // the extra piece only counts on the lanes that issue it
        const unsigned need = ((1u << (NBB * ACT_ITERS)) - 1u) | (extra_lane ? 1u << (2 * ACT_ITERS) : 0u);
        f_all = __builtin_amdgcn_readfirstlane(__all((f_ok & need) == need)) != 0;
#ifdef FW_FORCE_SLOW_DMA  // timing experiment: every tile takes the per-piece border path
        f_all = false;
#endif
    };
    auto issue_act = [&](int stage) {
        if (f_c == 0) plan_tile();
        if (issuer) {
            const unsigned dst_x = lds_base + (unsigned)(stage * PS_REGION + ACT_ITERS * NWAVES * 64) * 16u;
#pragma unroll
            for (int bt = 0; bt < NBB; ++bt) {
                const unsigned dst = (unsigned)(stage * PS_REGION + ACT_ITERS * vwave(bt) * 64);
                if (f_all) {
                    glds16_batch_a(f_src, relb[bt], lds_base + (dst + 4 * 64) * 16u);
                } else {
#pragma unroll
                    for (int i = 0; i < ACT_ITERS; ++i)
                        glds16_v(((f_ok >> (bt * ACT_ITERS + i)) & 1u) ? f_src + (relb[bt][i] - (unsigned)(4 - i) * 1024u)
                                                                        : reinterpret_cast<const char*>(p.zeros),
                                 lds_base + (dst + i * 64) * 16u);
                }
            }
            if (extra_lane) {
                if (f_all)
                    glds16(f_src, relb_x, dst_x);
                else
                    glds16_v(((f_ok >> (2 * ACT_ITERS)) & 1u) ? f_src + relb_x : reinterpret_cast<const char*>(p.zeros), dst_x);
            }
        }
        if (++f_c == na) {
            f_c = 0;
            ++f_t;
        } else {
            f_src += chunk_bytes;
        }
    };
    const PairIssueW<SM::W_BASE> pair_w{na, wa_b, wb_b, lds_base, lane16};
    // halves: bit 0 = conv_a's fragments, bit 1 = conv_b's
    auto issue_w = [&](int j, int ws, int halves = 3) {
        if (!issuer) return;
#pragma unroll
        for (int bt = 0; bt < NBB; ++bt) {
            pair_w.template issue<true>(j, ws, vwave(bt), halves);
        }
    };

    int rd_off[3][2];  // [dx][ph]: piece index of (halo row 2 * wave, px 16*ph + q + dx, slot sl)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) rd_off[dx][ph] = halo_rd_off(RPW * wave, 16 * ph + q + dx, sl);
    const PairWIdx widx;

    f32x4 acc[RPW][NW][2];

    // ---- emit (conv_pair_common.h): columns 1..30 of the region are valid outputs; the wave's rows of x_a start at image row
    //      R0 + 2 * wave, those of x_b one row higher ---------------------------------------------------------------------------------
    const int ls = (sl & 1) ? 2 + (sl >> 1) : (sl >> 1);
    const unsigned st_off = (unsigned)((q * p.out_cstride + ls * 8) * 2);
    const PairEmit<SlideGeom, T> emit{p, wave, q, ls, st_off, acc};
    uint4* carry = lds + SM::CARRY;
    float* bias_l = reinterpret_cast<float*>(lds + SM::BIAS);  // [0, 32) bias_a, [32, 64) bias_b
    // Loaded ahead of every DMA and read by the tiles from LDS: a global load at the top of a tile would make hipcc wait for
    // vmcnt(0), that is for the x_b stores the wave has just issued, where the tile's first item does not wait at all.
    float bias_g = 0.f;
    if (tid < 64) bias_g = tid < 32 ? p.bias_a[tid] : p.bias_b[tid - 32];

    if (!needs_warm) {
        issue_w(0, 0);
        issue_act(0);
        if (tid < 64) bias_l[tid] = bias_g;
        __syncthreads();
        FW_STAMP(ST_SETUP);
    } else {
        // ---- warm-up: x_a rows R0 - 2, R0 - 1 of the tile above the run into the carry buffer.  They read input rows R0 - 3 .. R0
        //      and conv_a's weights only.  All chunks of a batch (up to four; the shapes of RRDBNet have two or four) are in flight
        //      at once: four rows of chunk b in slot b of the second activation stage, conv_a's fragments of chunk 0 where the
        //      first tile's item 0 wants them anyway (weight stage 0, first half), those of the others in the second weight
        //      stage and, with a fourth chunk, in the second half of stage 0 - conv_b's fragments of item 0 then follow the
        //      warm-up.  Waves 4 - 7 (one per SIMD) take one row x one pixel half each and both cout tiles, chunk by chunk
        //      and tap by tap in the item's order, so every accumulator sees the sums of conv_item_lag (conv_pair_common.h) in the same order.
        int R0, ox;
        origin(t_lo, &R0, &ox);
        const int wr0 = R0 - 3;
        const bool w_all = R0 < p.H && ox >= 1 && ox + TILE_W < p.W;  // rows wr0 .. R0, columns ox - 1 .. ox + 32 inside (uniform)
        const char* w_src = in + ((long)wr0 * p.W + (ox - 1)) * p.in_cstride * 2;
        const int w_slot = wave >> 1, w_hi = wave & 1;  // this wave's DMAs: KiB 0 .. 4 (even wave) or 5 .. 8 (odd) of chunk slot wave / 2
        unsigned w_rel[5];
        unsigned w_ok = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int li0 = (5 * w_hi + i) * 64 + lane;
            const int li = li0 < PS_WARM_PIECES ? li0 : PS_WARM_PIECES - 1;  // pad pieces: any piece of the chunk
            const HaloPiece h = halo_piece(li);
            w_rel[i] = piece_off(li);
            if ((unsigned)(wr0 + h.row) < (unsigned)p.H && (unsigned)(ox - 1 + h.px) < (unsigned)p.W) w_ok |= 1u << i;
        }
        auto warm_rows = [&](int b, int c) {  // chunk c -> slot b
            const char* src = w_src + (long)c * chunk_bytes;
            const unsigned dst = lds_base + (unsigned)(PS_REGION + b * PS_WARM_SLOT + 5 * w_hi * 64) * 16u;
            if (w_all) {
                unsigned vo[5];
                if (w_hi == 0) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) vo[i] = w_rel[i] + (unsigned)(4 - i) * 1024u;
                    glds16_batch_a(src, vo, dst + 4 * 1024u);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) vo[i] = w_rel[i] + (unsigned)(3 - i) * 1024u;
                    glds16_batch_a4(src, vo, dst + 3 * 1024u);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    if (5 * w_hi + i < PS_WARM_KIB)
                        glds16_v(((w_ok >> i) & 1u) ? src + w_rel[i] : reinterpret_cast<const char*>(p.zeros), dst + i * 1024u);
            }
        };
        // weight slot s of a batch: the two halves of weight stage 1, then the second half of stage 0
        auto w_slot_piece = [](int s) { return SM::W_BASE + (s < 2 ? SM::W_REGION + s * W_FRAGS * 64 : W_FRAGS * 64); };
        const bool wb_late = na >= PS_WARM_CHUNKS;  // the third weight slot is in use: conv_b's fragments of item 0 after the warm-up
        const int wrow = (wave >> 1) & 1, wph = wave & 1;
        f32x4 wacc[2] = {};  // (bias_a from LDS behind the first barrier: a global load here would have hipcc wait for the DMAs)
        for (int c0 = 0; c0 < na;) {
            const int rest = na - c0;
            const int nb = c0 == 0 ? (rest < PS_WARM_CHUNKS ? rest : PS_WARM_CHUNKS) : (rest < 3 ? rest : 3);
            const int wc0 = c0 == 0 ? 1 : c0;        // first chunk whose fragments go to a slot
            const int nws = c0 == 0 ? nb - 1 : nb;   // slots in use
            if (w_slot < nb) warm_rows(w_slot, c0 + w_slot);
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s < nws && (wave >> 2) == (s & 1))
                    issue_w_half(wa_b + (size_t)(wc0 + s) * (W_FRAGS * 1024), lds_base + (unsigned)w_slot_piece(s) * 16u, wave & 3, lane16);
            if (c0 == 0) {
                issue_w(0, 0, wb_late ? 1 : 3);
                if (tid < 64) bias_l[tid] = bias_g;
            }
            FW_STAMP(ST_W_SETUP);
            FW_WAIT_VMCNT(0);
            FW_STAMP(ST_W_DMA);
            if (c0 == 0) issue_act(0);  // the first tile's first stage lands behind the MFMAs below
            __syncthreads();
            FW_STAMP(ST_W_BARRIER);
            if (wave >= NWAVES / 2) {
                if (c0 == 0) {
#pragma unroll
                    for (int w = 0; w < 2; ++w) wacc[w] = *reinterpret_cast<const f32x4*>(bias_l + 16 * w + 4 * sl);
                }
                for (int b = 0; b < nb; ++b) {
                    const uint4* xw = lds + PS_REGION + b * PS_WARM_SLOT;
                    const uint4* wl = lds + (c0 + b == 0 ? SM::W_BASE : w_slot_piece(c0 + b - wc0)) + lane;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int px = 16 * wph + q + dx;
                        const int xo = px * 4 + (sl ^ halo_swz(px));
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy) {
                            const uint4 xv = xw[(wrow + dy) * ROW_PIECES + xo];
#pragma unroll
                            for (int w = 0; w < 2; ++w)
                                wacc[w] = Op<T>::mfma16(wl[widx(dy * 3 + dx, w) * 64], xv, wacc[w]);
                        }
                    }
                }
            }
            FW_STAMP(ST_W_MFMA);
            c0 += nb;
            if (c0 < na) {
                __syncthreads();  // the next batch overwrites the slots
                FW_STAMP(ST_W_BARRIER);
            }
        }
        if (wave >= NWAVES / 2) {
            // as convert() and write_xa() do for rows 16, 17 of the x_a tile, straight into the carry buffer
            uint4 v = pair16<T>(lrelu4(wacc[0]), lrelu4(wacc[1]));
            const int cp = 16 * wph + q, hp = cp + 1;
            if (!((unsigned)(R0 - 2 + wrow) < (unsigned)p.H && (unsigned)(ox + cp) < (unsigned)p.W)) v = make_uint4(0, 0, 0, 0);
            carry[(wrow * HALO_W + hp) * 4 + (ls ^ halo_swz(hp))] = v;
        }
        FW_STAMP(ST_W_EPI);
        if (wb_late) {
            __syncthreads();  // waves 4 - 7 are done with the fragments in the second half of weight stage 0
            FW_STAMP(ST_W_BARRIER);
            issue_w(0, 0, 2);
            FW_STAMP(ST_W_SETUP);
        }
    }

    int n = 0;   // item counter (weight stage = n & 1)
    int qd = 0;  // DMA'd chunks consumed
    for (int t = t_lo; t < t_hi; ++t) {
        int R0, ox;
        origin(t, &R0, &ox);
        const bool col_top = R0 == 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_l + 16 * w + 4 * sl);
#pragma unroll
            for (int row = 0; row < RPW; ++row)
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) acc[row][w][ph] = bv;
        }
        FW_STAMP(ST_SETUP);  // tile set-up
        const int ipt = na + 1;
        // kind: 0 = shared chunk with both convs, 2 = conv_b's x_a chunk
        auto run_item = [&](int j, auto kind_tag, bool wait_dma) {
            constexpr int KIND = decltype(kind_tag)::value;
            constexpr bool SHARED = KIND != 2;
            FW_STAMP(SHARED ? ST_SHARED : ST_XA_LDS);  // the previous phase ends
            if (wait_dma) FW_WAIT_VMCNT(0);
#ifdef FW_PAIR_STAMP
            if (j == 0) {
                __syncthreads();
                FW_STAMP(ST_FIRST);  // the wait for the tile's first stage
            } else {
                FW_STAMP(ST_VMCNT);
                __syncthreads();
                FW_STAMP(ST_BARRIER);
            }
#else
            __syncthreads();
#endif
            const bool more = n + 1 < nitems;
            const int jn = (j + 1 == ipt) ? 0 : j + 1;
            const bool fetch = SHARED && more && (j + 1 < na || t + 1 < t_hi);
            const int fetch_stage = (qd + 1) & 1;
            auto dma_slot = [&](int d) {
                if (d == FW_DMA_SLOT_W) {
                    if (more) issue_w(jn, (n + 1) & 1);
                } else if (d == FW_DMA_SLOT_A) {
                    if (fetch) issue_act(fetch_stage);
                }
            };
            const uint4* a = lds + ((SHARED ? qd : qd - 1) & 1) * PS_REGION;
            const uint4* wl = lds + SM::W_BASE + (n & 1) * SM::W_REGION + lane;
            auto& slot_fn = dma_slot;
            if constexpr (KIND == 0)
                conv_item_lag<ROW_PIECES, T, true>(acc, a, wl, rd_off, NoXCol{}, widx, slot_fn);
            else
                conv_item<T, NW, 2>(acc, a, wl, rd_off, widx, slot_fn, [](const uint4 (&)[RPW][2]) {}, [](int) {});
            if (SHARED) ++qd;
            ++n;
        };
        bool wait_dma = t == t_lo;
#pragma clang loop unroll(disable)
        for (int j = 0; j < na; ++j) {
            run_item(j, std::integral_constant<int, 0>{}, wait_dma);
            wait_dma = true;
        }
        FW_STAMP(ST_SHARED);
        // conv_a done for this wave; the DMAs in flight are an item old: wait ahead of the stores (vmcnt counts stores too)
        FW_WAIT_VMCNT(0);
        FW_STAMP(ST_VMCNT);
        // everything this tile reads, computes and stores inside the image?  (uniform)
        const bool interior = ox >= 0 && ox + TILE_W <= p.W && R0 >= 1 && R0 + TILE_H <= p.H;
        uint4 pk[RPW][2];
        emit.convert(0, pk);
        if (interior)
            emit.template store_out<true>(pk, R0, ox, reinterpret_cast<T*>(p.out_a));
        else
            emit.template store_out<false>(pk, R0, ox, reinterpret_cast<T*>(p.out_a));
        FW_STAMP(ST_XA_EPI);  // convert + stores of x_a
        __syncthreads();      // every wave is done with the last chunk's stage: it becomes the x_a tile
        FW_STAMP(ST_BARRIER);
        uint4* xa = lds + ((qd - 1) & 1) * PS_REGION;
        if (interior)
            emit.template write_xa<true>(pk, xa, R0, ox);
        else
            emit.template write_xa<false>(pk, xa, R0, ox);
        // x_a rows R0 - 2, R0 - 1 -> tile rows 0, 1: from the tile above (carry), zero at the top of a column
        if (lane < PS_CARRY / NWAVES) {
            const int i = wave * (PS_CARRY / NWAVES) + lane;
            xa[i] = col_top ? make_uint4(0, 0, 0, 0) : carry[i];
        }
        // (run_item's first stamp closes ST_XA_LDS: x_a tile, own rows + carry rows, into LDS)
        run_item(na, std::integral_constant<int, 2>{}, false);
        FW_STAMP(ST_XA_ITEM);
        // rows 16, 17 of the x_a tile (wave 7's own conv_a rows: its LDS writes are ordered before these reads) -> carry, after
        // the barrier that ends every wave's reading of the old carry
        if (wave == NWAVES - 1) {
#pragma unroll
            for (int k = 0; k < (PS_CARRY + 63) / 64; ++k) {
                const int i = k * 64 + lane;
                if (i < PS_CARRY) carry[i] = xa[16 * ROW_PIECES + i];
            }
        }
        FW_STAMP(ST_CARRY);  // carry rows
        // conv_b done for this wave: rows R0 - 1 + (2w, 2w + 1).  In flight: the x_a stores (an item old), the next weights.
        FW_WAIT_VMCNT(0);
        FW_STAMP(ST_VMCNT);
        emit.convert(2, pk);
        if (interior)
            emit.template store_out<true>(pk, R0 - 1, ox, reinterpret_cast<T*>(p.out_b));
        else
            emit.template store_out<false>(pk, R0 - 1, ox, reinterpret_cast<T*>(p.out_b));
        FW_STAMP(ST_XB_EPI);  // convert + stores of x_b
    }
    FW_STAMP_FLUSH(p.stamps);
}

// FW_PAIR_SLIDE=1 / 0 forces the sliding-window / the ring kernel; unset: the sliding window when a workgroup gets at least six
// tiles (its warm-up tile and the uneven last round weigh less and less: 0.9 % ahead at 720p, 3.5 % at 1080p; the ring kernel is
// 1.5 % ahead at 960x540, four tiles per workgroup).  Read per launch (a getenv is nothing next to a launch): tests flip it
// inside one process.
bool pair_slide_enabled(int H, int W, int num_cus) {
    if (const char* e = getenv("FW_PAIR_SLIDE")) return atoi(e) != 0;
    const long tiles = (long)((W + PS_TW - 1) / PS_TW) * ((H + PS_TH) / PS_TH);
    return tiles >= 6L * num_cus;
}

void launch_conv3x3_pair_slide(DType dt, const ConvPairParams& p, int num_cus, hipStream_t stream) {
    const int tiles = ((p.W + PS_TW - 1) / PS_TW) * ((p.H + PS_TH) / PS_TH);
    launch_pair_kernel(conv3x3_pair_slide_kernel<__bf16>, conv3x3_pair_slide_kernel<_Float16>, dt, tiles, num_cus, p, stream);
}

}  // namespace fw
