// What the three fused conv-pair kernels share: conv3x3_pair.hip (the ring kernel: both convs on one 16x32 region, 14x30 valid),
// conv3x3_pair_slide.hip (minus the vertical ring: 16x30 valid, conv_b one row behind conv_a) and conv3x3_pair_slide32.hip (minus
// the horizontal ring too: 16x32 valid).  A kernel states its geometry (PairGeom) and keeps its own DMA plan and tile loop; the
// weight stage, the emit, the x_a tile and the window kernels' item with conv_b one row behind conv_a are here once.  gfx950 only.
#pragma once
#include <type_traits>
#include "conv_common.h"

namespace fw {

constexpr int PAIR_W_REGION = 2 * W_FRAGS * 64;  // pieces of a weight stage: the chunk of conv_a (18 fragments) + of conv_b (18)

// What differs between the three kernels in where a wave's RPW x 32 accumulator pixels go.  Tile row cr = RPW*wave + row and
// region column cp = 16*ph + q are valid outputs inside [ROW_LO, ROW_HI] x [COL_LO, COL_HI]; x_a (cr, cp) sits at row cr + XA_ROW,
// px cp + XA_PX of the x_a tile, which has ROWP pieces per halo row.
template <int ROW_LO_, int ROW_HI_, int COL_LO_, int COL_HI_, int XA_ROW_, int XA_PX_, int ROWP_>
struct PairGeom {
    static constexpr int ROW_LO = ROW_LO_, ROW_HI = ROW_HI_, COL_LO = COL_LO_, COL_HI = COL_HI_, XA_ROW = XA_ROW_, XA_PX = XA_PX_, ROWP = ROWP_;
};

// weight fragment of (tap, accumulator tile w) inside a weight stage: tiles 0,1 = conv_a, 2,3 = conv_b
struct PairWIdx {
    __device__ __forceinline__ int operator()(int tap, int w) const { return w < 2 ? tap * 2 + w : W_FRAGS + tap * 2 + (w - 2); }
};

// The pieces below are closures written out by hand: structs of REFERENCES to the kernel's own variables, built once in the kernel
// body where the three kernels used to define the same lambdas.  (By reference on purpose: hipcc then sees what it saw with the
// lambdas and emits the same code; helpers that take the values instead shift its scalar prologue around.)

// Weights of item j of a tile -> weight stage ws (the stages start at piece W_BASE of the workgroup's LDS), the share of issuing
// wave v: fragments [0,18) = conv_a chunk j (waves 0-3: 5, 5, 5, 3 fragments), [18,36) = conv_b chunk j (waves 4-7); the last item
// (j == na) only has conv_b's chunk.  SELECT: only the halves named by `halves` (bit 0 = conv_a's fragments, bit 1 = conv_b's).
template <int W_BASE>
struct PairIssueW {
    const int& na;
    const char* const& wa_b;
    const char* const& wb_b;
    const unsigned& lds_base;
    const unsigned& lane16;
    template <bool SELECT = false>
    __device__ __forceinline__ void issue(int j, int ws, int v, int halves = 3) const {
        const int half = v / (NWAVES / 2), k = v % (NWAVES / 2);
        if ((!SELECT || ((halves >> half) & 1)) && (half == 1 || j < na))
            issue_w_half((half ? wb_b : wa_b) + (size_t)j * (W_FRAGS * 1024),
                         lds_base + (unsigned)(W_BASE + ws * PAIR_W_REGION + W_FRAGS * half * 64) * 16u, k, lane16);
    }
};

// ---- emit: accumulators -> LeakyReLU -> typed, without a transpose through LDS and BEFORE the barrier (pair16 in conv_common.h
// has the lane map).  Everything up to the LDS write of x_a needs no barrier: a wave converts and stores as soon as ITS last item
// is done - the older wave of a SIMD while the younger one still runs MFMAs, the younger one with the VALU to itself (with the
// convert behind the barrier both waves of a SIMD converted at the same time: 18 % of the kernel, phase stamps in DESIGN.md
// section 6).
template <typename G, typename T>
struct PairEmit {
    const ConvPairParams& p;
    const int& wave;
    const int& q;
    const int& ls;            // the 8-channel slot of its pixel that the lane holds after the permlane swap
    const unsigned& st_off;   // the lane's store offset from (row, region px 16*ph)
    f32x4 (&acc)[RPW][4][2];

    // tiles w0, w0 + 1 (0 = conv_a, 2 = conv_b) of the wave's pixels -> one 16-byte slot per pixel
    __device__ __forceinline__ void convert(int w0, uint4 (&pk)[RPW][2]) const {
#pragma unroll
        for (int row = 0; row < RPW; ++row)
#pragma unroll
            for (int ph = 0; ph < 2; ++ph)
                pk[row][ph] = pair16<T>(lrelu4(w0 ? acc[row][2][ph] : acc[row][0][ph]), lrelu4(w0 ? acc[row][3][ph] : acc[row][1][ph]));
    }
    // The valid part of the wave's pixels -> global plane.  y0 = image row of tile row 0, ox = image column of region column 0.
    // INTERIOR: the whole tile is inside the image.
    template <bool INTERIOR>
    __device__ __forceinline__ void store_out(const uint4 (&pk)[RPW][2], int y0, int ox, T* plane) const {
        constexpr bool ALL_ROWS = G::ROW_LO == 0 && G::ROW_HI == TILE_H - 1, ALL_COLS = G::COL_LO == 0 && G::COL_HI == TILE_W - 1;
        const int gy0 = y0 + RPW * wave;
#pragma unroll
        for (int row = 0; row < RPW; ++row) {
            const int cr = RPW * wave + row;
            const int gy = ALL_ROWS ? gy0 + row : y0 + cr;
            if constexpr (ALL_ROWS) {
                if (!INTERIOR && !((unsigned)gy < (unsigned)p.H)) continue;  // wave-uniform
            } else {
                const bool row_ok = cr >= G::ROW_LO && cr <= G::ROW_HI && (INTERIOR || (unsigned)gy < (unsigned)p.H);  // wave-uniform
                if (!row_ok) continue;
            }
            char* rowbase = reinterpret_cast<char*>(plane) + ((long)gy * p.W + ox) * p.out_cstride * 2;  // wave-uniform
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                const int cp = 16 * ph + q;
                if constexpr (ALL_COLS) {  // (region column 0 is a valid output: ox >= 0)
                    if (INTERIOR || ox + cp < p.W) store16(rowbase + (long)(16 * ph) * p.out_cstride * 2 + st_off, pk[row][ph]);
                } else {
                    if (cp >= G::COL_LO && cp <= G::COL_HI && (INTERIOR || (unsigned)(ox + cp) < (unsigned)p.W))
                        store16(rowbase + (long)(16 * ph) * p.out_cstride * 2 + st_off, pk[row][ph]);
                }
            }
        }
    }
    // x_a of the wave's pixels -> the x_a tile in LDS, in the halo format the LDS-DMA produces (zero outside the image = conv_b's
    // zero padding; border tiles only).  y0 = image row of tile row 0, ox = image column of region column 0.
    template <bool INTERIOR>
    __device__ __forceinline__ void write_xa(const uint4 (&pk)[RPW][2], uint4* xa, int y0, int ox) const {
#pragma unroll
        for (int row = 0; row < RPW; ++row) {
            const int cr = RPW * wave + row;
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                const int cp = 16 * ph + q, hp = cp + G::XA_PX;
                uint4 v = pk[row][ph];
                constexpr bool OX_GE_0 = G::COL_LO == 0;  // region column 0 is a valid output
                if (!INTERIOR && !((unsigned)(y0 + cr) < (unsigned)p.H && (OX_GE_0 ? ox + cp < p.W : (unsigned)(ox + cp) < (unsigned)p.W)))
                    v = make_uint4(0, 0, 0, 0);
                if constexpr (G::ROWP % 4 == 0)
                    xa[((cr + G::XA_ROW) * (G::ROWP / 4) + hp) * 4 + (ls ^ halo_swz(hp))] = v;
                else
                    xa[(cr + G::XA_ROW) * G::ROWP + hp * 4 + (ls ^ halo_swz(hp))] = v;
            }
        }
    }
};

// ---- the shared-chunk item of the two window kernels ------------------------------------------------------------------------------
// acc += A * B when `on` (wave-uniform) is non-zero, with the jump inside the statement: no control flow that hipcc can see.  The
// operands come from LDS reads (the compiler waits for them ahead of the statement) and the accumulator is next touched tiles later,
// so none of the MFMA's software wait states is at stake.
template <typename T>
__device__ __forceinline__ void mfma16_if(f32x4& acc, const uint4& a4, const uint4& b4, int on) {
    const nt_u32x4 a = {a4.x, a4.y, a4.z, a4.w}, b = {b4.x, b4.y, b4.z, b4.w};   // (a HIP uint4 is a struct: no register constraint takes it)
    on = __builtin_amdgcn_readfirstlane(on);   // provably scalar, even where hipcc has parked the flag in a vector register
    if constexpr (std::is_same<T, __bf16>::value)
        asm volatile("s_cmp_eq_u32 %3, 0\n\ts_cbranch_scc1 .Lfw_skip_%=\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n.Lfw_skip_%=:"
                     : "+v"(acc) : "v"(a), "v"(b), "s"(on) : "scc");
    else
        asm volatile("s_cmp_eq_u32 %3, 0\n\ts_cbranch_scc1 .Lfw_skip_%=\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n.Lfw_skip_%=:"
                     : "+v"(acc) : "v"(a), "v"(b), "s"(on) : "scc");
}

// One shared-chunk item with conv_b one row behind conv_a.  acc tiles 0,1 = conv_a rows (2w, 2w+1), 2,3 = conv_b rows
// (2w-1, 2w); xr[h] = halo row 2w + h.  conv_a row r, tap row dy reads xr[r + dy + 1], conv_b xr[r + dy].  Row h is last used
// at dy = min(h, 2): rows 0 / 1 are re-read for the next dx after dy = 0 / 1, row 2 after conv_b's tiles of dy = 2, rows 3, 4
// at the start of the next dx.  conv_b's tiles go first within a step so that the freshly read rows are needed last.
// ROWP = pieces per halo row of the stage (the 36-pixel stages of conv3x3_pair_slide32.hip: 145).
//
// x = NoXCol{} (the window kernel; the 32-column kernel's warm-up items), or the extra conv_a column of a wave of the 32-column
// kernel that owns one (XCol): its B fragment for tap (dy, dx) is piece off[dx] + dy * ROWP of the stage (16 rows of one halo
// pixel), its A fragment the one the row-shaped MFMAs of output-channel tile xct use at that tap.
// Only waves 0-3 own an extra column, and the item must not branch on that in a way hipcc sees: a wave-uniform branch per step made
// its waitcnt pass drain the LDS queue at every join (the item lost its read-ahead: +3.4 ms per frame), two whole variants of the
// item under one branch spilled 44-126 registers.  So the two fragment reads are predicated per lane (lane: true in every lane of
// waves 0-3 - to the compiler a divergent condition, i.e. an EXEC mask around one ds_read, no branch) and the MFMA sits in an asm
// statement that jumps over it when on == 0 (mfma16_if).  wl = the item's wl + 64 * xct: the extra column's own A fragment (tile
// xct of conv_a) is read a step ahead like the others, at a compile-time offset.  With NoXCol all of it is compiled out.
struct NoXCol {};
struct XCol {
    f32x4& acc;           // the column's accumulator: 16 rows x 16 output channels of tile xct
    const uint4* wl;      // wl + 64 * xct
    const int (&off)[3];  // [dx]: the lane's piece of (halo row q + 1, the column's px + dx)
    bool lane;            // == on in every lane, kept per lane
    int on;
};
template <int ROWP, typename T, bool WITH_B, typename X, typename WIdx, typename Slot>
__device__ __forceinline__ void conv_item_lag(f32x4 (&acc)[RPW][4][2], const uint4* a, const uint4* wl, const int (&rd_off)[3][2], X x, WIdx widx,
                                              Slot dma_slot) {
    constexpr bool XCODE = !std::is_same<X, NoXCol>::value;
    constexpr int NWU = WITH_B ? 4 : 2;
    constexpr int NK = 9 * NWU;
    constexpr int RING = 3;
    uint4 xr[5][2];
    uint4 wf[RING];
    uint4 xc = make_uint4(0, 0, 0, 0);   // the extra column's B fragment of the current tap: re-read once its MFMA has issued
    uint4 wx = make_uint4(0, 0, 0, 0);   // ... and its A fragment
    auto tile_of = [](int w) { return WITH_B ? ((w + 2) & 3) : w; };
    auto load_w = [&](int k) {
        const int t = k / NWU, w = k - t * NWU;
        const int dx = t / 3, dy = t - 3 * dx;
        wf[k % RING] = wl[widx(dy * 3 + dx, tile_of(w)) * 64];
    };
    auto load_row = [&](int h, int dx) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) xr[h][ph] = a[h * ROWP + rd_off[dx][ph]];
    };
#pragma unroll
    for (int h = 0; h < 5; ++h) load_row(h, 0);
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) load_w(k);
    if constexpr (XCODE) { if (x.lane) xc = a[x.off[0]]; }   // tap (dy 0, dx 0)
    FW_SB();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dx = t / 3, dy = t - 3 * dx;
        if (dx < 2 && dy == 1) load_row(0, dx + 1);
        if (dx < 2 && dy == 2) load_row(1, dx + 1);
        if (dx > 0 && dy == 0) {
            load_row(3, dx);
            load_row(4, dx);
        }
#pragma unroll
        for (int w = 0; w < NWU; ++w) {
            const int k = t * NWU + w;
            if (k + RING - 1 < NK) load_w(k + RING - 1);
            FW_SB();
            const int tile = tile_of(w);
            const int lag = tile >= 2 ? 0 : 1;
#pragma unroll
            for (int row = 0; row < RPW; ++row)
#pragma unroll
                for (int ph = 0; ph < 2; ++ph)
                    acc[row][tile][ph] = Op<T>::mfma16(wf[k % RING], xr[row + dy + lag][ph], acc[row][tile][ph]);
            if constexpr (XCODE) {
                if (w == 0) { if (x.lane) wx = x.wl[widx(dy * 3 + dx, 0) * 64]; }
                if (w == NWU - 1) mfma16_if<T>(x.acc, wx, xc, x.on);
            }
            FW_SB();
#pragma unroll
            for (int d = 0; d < 4 / NWU; ++d) dma_slot((t * NWU + w) * (4 / NWU) + d);
            FW_SB();
            if (dx < 2 && dy == 2 && w == (WITH_B ? 1 : 0)) load_row(2, dx + 1);
        }
        if (t + 1 < 9) {
            const int dxn = (t + 1) / 3, dyn = (t + 1) - 3 * dxn;
            if constexpr (XCODE) { if (x.lane) xc = a[x.off[dxn] + dyn * ROWP]; }
        }
    }
}

// ---- host side: conv3x3_pair.hip's launch_conv3x3_pair chooses among the three -------------------------------------------------
bool pair_slide_enabled(int H, int W, int num_cus);
void launch_conv3x3_pair_slide(DType dt, const ConvPairParams& p, int num_cus, hipStream_t stream);
bool pair_slide32_enabled();   // conv3x3_pair_slide32.hip: the window kernel with all 32 columns of a tile valid
void launch_conv3x3_pair_slide32(DType dt, const ConvPairParams& p, int num_cus, hipStream_t stream);

// One persistent workgroup per CU (or per tile, if there are fewer); k_bf16 / k_f16 = the kernel's two instances
inline void launch_pair_kernel(void (*k_bf16)(ConvPairParams), void (*k_f16)(ConvPairParams), DType dt, int tiles, int num_cus,
                               const ConvPairParams& p, hipStream_t stream) {
    dim3 grid(tiles < num_cus ? tiles : num_cus), block(64 * NWAVES);
    hipLaunchKernelGGL(dt == DT_BF16 ? k_bf16 : k_f16, grid, block, 0, stream, p);
    FW_HIP_CHECK(hipGetLastError());
}

}  // namespace fw
