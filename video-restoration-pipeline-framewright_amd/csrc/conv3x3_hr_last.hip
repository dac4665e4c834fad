// The tail of the RRDBNet in one launch: out = conv_last(lrelu(conv_hr(x))) (reference src/framewright/processors/aesrgan_face.py:268)
// without the 64-channel map h = lrelu(conv_hr(x)) ever leaving the chip.
//
// conv_hr is conv3x3_mfma_kernel<T, 2, EPI_STORE>'s K loop unchanged (same conv_item, same order of chunks and taps, accumulators
// started at the bias, same LDS-DMA plan), so h has the bits the two-launch form stores.  conv_last (64 -> 3 channels) is evaluated
// in scatter form from the registers that hold h:
//
//   pointwise step   z[dy][dx][c](y', x') = sum_ch W_last[c][ch][dy][dx] * h(y', x', ch)      a 1x1 conv 64 -> 27 on the matrix cores
//   shifted adds     r_dy(y', x) = (z[dy][0](y', x - 1) + z[dy][1](y', x)) + z[dy][2](y', x + 1)
//                    out(y, x)   = ((b + r_0(y - 1, x)) + r_1(y, x)) + r_2(y + 1, x)             fp32, the same order for every pixel
//
// After lrelu4 + pair16 a lane holds one 8-channel slot of its pixel: a B fragment of v_mfma_f32_16x16x32 with its k slots permuted
// (slot sl of the instruction = slot ls(sl) of the chunk); pack_conv_last_pointwise permutes the A fragments' k the same way.
// Fragment (dx, chunk): D row 4 dy + c, so the 16-lane group sl = dy of a wave ends up with colour j = c of its pixel for tap row dy and
// the three dx terms of a pixel's r_dy sit in three registers of lanes of ONE 16-lane row: the horizontal shifts stay inside the
// wave (the two 16-pixel halves of a row are two registers of the same lane), only r changes waves, through LDS.
//
// Geometry (the window kernel's, conv3x3_pair_slide.hip): the compute region is 16 x 32 pixels of h, columns 1..30 are valid outputs
// (the horizontal ring is recomputed by the neighbours), a workgroup walks DOWN a column in steps of 16 rows and the outputs run one
// row behind: step ty computes h rows [16 ty, 16 ty + 15] and emits out rows [16 ty - 1, 16 ty + 14].  Three rows of r stay in LDS
// from step to step (r_0 of tile rows 14 and 15, r_1 of row 15); they are zero at the top of a column.  A run that starts in the
// middle of a column first runs the step above it whole, with nothing stored: its only product is the carry.
// h outside the image is ZERO (conv_last's padding), not lrelu(bias): border tiles zero those fragments.
//
// LDS: Smem<2> (152 KiB) + 6 KiB pointwise fragments + 1.5 KiB carry + the two bias vectors.  The 24 KiB exchange of r lives in the
// activation stage the tile's last item has just freed: with two stages the next DMA into it is issued behind the next item's top
// barrier.  Nothing is loaded from global memory inside the tile loop.
#include "fw_internal.h"
#include "conv_common.h"

#ifndef FW_DMA_SLOT_W
#define FW_DMA_SLOT_W 2
#define FW_DMA_SLOT_A 6
#endif

namespace fw {

constexpr int HL_TW = TILE_W - 2;   // 30 valid columns per tile
constexpr int HL_FRAGS = 6;         // pointwise A fragments: [dx][chunk]

struct HrLastParams {
    ConvParams p;          // conv_hr's problem + the image outputs of EPI_IMAGE (out_u8 / out_u16 / out_rgb, img_H, img_W)
    const void* wlast;     // pack_conv_last_pointwise
    const float* blast;    // conv_last's bias, >= 3 floats
};

struct HrLastSmem {
    using SM = Smem<2>;
    static constexpr int FRAG = SM::TOTAL;              // 6 fragments of 64 pieces
    static constexpr int CARRY = FRAG + HL_FRAGS * 64;  // 3 rows x 32 px x float4
    static constexpr int BIAS = CARRY + 3 * TILE_W;     // 64 floats of conv_hr, then 4 of conv_last
    static constexpr int TOTAL = BIAS + 17;
};
static_assert(HrLastSmem::TOTAL * 16 <= 160 * 1024, "LDS");
static_assert(3 * TILE_H * TILE_W <= ACT_REGION, "the exchange of r fits an activation stage");
static_assert(NWAVES == 8 && RPW == 2, "written for 8 waves of 2 rows");

// v of the lane at byte address addr4 = 4 * lane.  v by value: a bit_cast straight from a vector ELEMENT reads element 0 of the vector.
__device__ __forceinline__ float lane_read(int addr4, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr4, __builtin_bit_cast(int, v)));
}

// lrelu4 (conv_common.h) with the max as a builtin; the values are the same.  Here the LeakyReLU of one pixel half runs between the
// pointwise MFMAs of the other, and only three of an MFMA's four result registers are used: hipcc hands the fourth to the next
// value at once, and an instruction inside an asm statement gets none of the wait states it puts between an MFMA and a VALU
// write of one of its result registers - the MFMA then overwrites the LeakyReLU value (seen on the device: one channel pair
// of the second pixel half wrong).
__device__ __forceinline__ f32x4 lrelu4_builtin(f32x4 v) {
    const f32x4 t = v * 0.2f;
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaxf(v[j], t[j]);
    return o;
}

template <typename T>
__global__ __launch_bounds__(64 * NWAVES, WAVES_PER_SIMD) void conv3x3_hr_last_kernel(const HrLastParams hp) {
    const ConvParams& p = hp.p;
    using SM = Smem<2>;
    using HS = HrLastSmem;
    __shared__ __attribute__((aligned(16))) uint4 lds[HS::TOTAL];
    constexpr int NA = SM::NA;
    constexpr int NW = 4;
    static_assert(NA == 2, "the exchange scratch relies on two activation stages");

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int q = lane & 15;
    const int sl = lane >> 4;

    // ---- persistent workgroup: a contiguous range of tiles, column-major (t = tx * tiles_y + ty) -----------------------------
    const TileBand band;
    const int tiles_x = (p.W + HL_TW - 1) / HL_TW;
    const int tiles_y = (p.H + TILE_H) / TILE_H;   // the last output row H - 1 = 16 ty + 14 at the latest
    const int ntiles = tiles_x * tiles_y;
    int t_lo, t_hi;
    band.range(ntiles, &t_lo, &t_hi);
    if (t_lo >= t_hi) return;
    const int t_first = t_lo - ((t_lo % tiles_y) != 0 ? 1 : 0);   // a run that starts mid-column: the step above it first, for the carry
    const int nch = p.cin_chunks;
    const int nitems = (t_hi - t_first) * nch;
    // tile t: first h row y0 and the image column x0 of region column 0 (one pixel left of the first valid output)
    auto origin = [&](int t, int* y0, int* x0) {
        const int tx = t / tiles_y, ty = t - tx * tiles_y;
        *y0 = ty * TILE_H;
        *x0 = tx * HL_TW - 1;
    };

    // ---- parameters into LDS, ahead of every DMA ---------------------------------------------------------------------------------
    float* bias_l = reinterpret_cast<float*>(lds + HS::BIAS);   // [0, 64) conv_hr, [64, 67) conv_last
    if (tid < HL_FRAGS * 64) lds[HS::FRAG + tid] = reinterpret_cast<const uint4*>(hp.wlast)[tid];
    if (tid < 64) bias_l[tid] = p.bias[tid];
    if (tid >= 64 && tid < 68) bias_l[tid] = tid < 67 ? hp.blast[tid - 64] : 0.f;
    __syncthreads();   // the first tile reads the bias ahead of its first barrier

    // ---- per-lane DMA plan (conv3x3_mfma.hip's, with the tile origin of this geometry) ---------------------------------------------
    unsigned relb[ACT_ITERS];
#pragma unroll
    for (int i = 0; i < ACT_ITERS; ++i) {
        const HaloPiece h = halo_piece((ACT_ITERS * wave + i) * 64 + lane);
        relb[i] = (unsigned)(((h.row * p.W + h.px) * p.in_cstride + h.s * 8) * 2) + (unsigned)(4 - i % 5) * 1024u;
    }
    const unsigned lds_base = (unsigned)(size_t)(lds_ptr_t)lds;
    const char* in = reinterpret_cast<const char*>(p.in);
    const char* w_b = reinterpret_cast<const char*>(p.wpk);
    const unsigned lane16 = lane * 16;
    const long chunk_bytes = p.in_pstride * 2;

    unsigned a_ok = 0;
    bool a_all = true;
    const char* a_src = nullptr;
    int a_n = 0, a_t = t_first, a_c = 0;
    auto plan_tile = [&]() {
        int ty0, tx0;
        origin(a_t, &ty0, &tx0);
        a_src = in + ((long)(ty0 - 1) * p.W + (tx0 - 1)) * p.in_cstride * 2;
        a_ok = 0;
#pragma unroll
        for (int i = 0; i < ACT_ITERS; ++i) {
            const int idx = (ACT_ITERS * wave + i) * 64 + lane;
            const HaloPiece h = halo_piece(idx);
            const int gy = ty0 - 1 + h.row;
            const int gx = tx0 - 1 + h.px;
            if (idx < ACT_PIECES && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) a_ok |= 1u << i;
        }
        a_all = __builtin_amdgcn_readfirstlane(__all(a_ok == (1u << ACT_ITERS) - 1u)) != 0;
    };
    auto issue_act = [&]() {
        if (a_c == 0) plan_tile();
        const unsigned dst = (unsigned)((a_n % NA) * ACT_REGION + ACT_ITERS * wave * 64);
        if (a_all) {
#pragma unroll
            for (int bt = 0; bt < ACT_ITERS / 5; ++bt) glds16_batch_a(a_src, relb + 5 * bt, lds_base + (dst + (5 * bt + 4) * 64) * 16u);
        } else {
#pragma unroll
            for (int i = 0; i < ACT_ITERS; ++i)
                glds16_v(((a_ok >> i) & 1u) ? a_src + (relb[i] - (unsigned)(4 - i % 5) * 1024u) : reinterpret_cast<const char*>(p.zeros),
                         lds_base + (dst + i * 64) * 16u);
        }
        ++a_n;
        if (++a_c == nch) {
            a_c = 0;
            ++a_t;
        } else {
            a_src += chunk_bytes;
        }
    };
    auto issue_w = [&](int c, int ws) {
        const int half = wave / (NWAVES / 2), k = wave % (NWAVES / 2);
        issue_w_half(w_b + (size_t)c * (W_FRAGS * 2 * 1024) + W_FRAGS * half * 1024,
                     lds_base + (unsigned)(SM::W_BASE + ws * SM::W_REGION + W_FRAGS * half * 64) * 16u, k, lane16);
    };

    int rd_off[3][2];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) rd_off[dx][ph] = halo_rd_off(RPW * wave, 16 * ph + q + dx, sl);

    // the lanes a lane takes its left / right neighbour pixel from (same 16-lane row, with wrap: the wrapped lane holds the
    // neighbour in the register of the other pixel half), as ds_bpermute byte addresses
    const int lane_l = ((lane & 48) | ((q + 15) & 15)) * 4;
    const int lane_r = ((lane & 48) | ((q + 1) & 15)) * 4;

    f32x4 acc[RPW][NW][2];

    issue_w(0, 0);
    issue_act();

    float4* carry = reinterpret_cast<float4*>(lds + HS::CARRY);   // [0] r_0 of tile row 14, [1] r_1 of row 15, [2] r_0 of row 15
    const uint4* frag = lds + HS::FRAG + lane;

    int n = 0;
    for (int t = t_first; t < t_hi; ++t) {
        int y0, x0;
        origin(t, &y0, &x0);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_l + 16 * w + 4 * sl);
#pragma unroll
            for (int row = 0; row < RPW; ++row)
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) acc[row][w][ph] = bv;
        }

        for (int c = 0; c < nch; ++c, ++n) {
            // (a tile's first item after an epilogue does not wait: its DMAs were waited for ahead of the epilogue's stores)
            if (c > 0 || t == t_first) FW_WAIT_VMCNT(0);
            __syncthreads();
            const bool do_w = n + 1 < nitems;
            const bool do_a = n + NA - 1 < nitems;
            const int c1 = (c + 1 == nch) ? 0 : c + 1;
            auto dma_slot = [&](int d) {
                if (d == FW_DMA_SLOT_W) {
                    if (do_w) issue_w(c1, (n + 1) & 1);
                } else if (d == FW_DMA_SLOT_A) {
                    if (do_a) issue_act();
                }
            };
            const uint4* a = lds + (n % NA) * ACT_REGION;
            const uint4* wl = lds + SM::W_BASE + (n & 1) * SM::W_REGION + lane;
            auto& slot_fn = dma_slot;
            conv_item<T, NW, 0>(
                acc, a, wl, rd_off, [](int tap, int w) { return tap * NW + w; }, slot_fn, [](const uint4 (&)[RPW][2]) {}, [](int) {});
        }

        // ---- epilogue (the DMA stream is already fetching the next tile) -------------------------------------------------------
        FW_WAIT_VMCNT(0);   // the next tile's first item has been in flight for an item: wait here, ahead of the stores
        const bool interior = x0 >= 0 && x0 + TILE_W <= p.W && y0 + TILE_H <= p.H;   // every h of the tile inside the image (uniform)
        f32x4 r[RPW][2];   // lanes of group sl = dy < 3: r_dy of (tile row RPW * wave + row, region column 16 * ph + q), colours 0..2
#pragma unroll
        for (int row = 0; row < RPW; ++row) {
            f32x4 z[3][2];
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                uint4 hk[2];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    hk[c2] = pair16<T>(lrelu4_builtin(acc[row][2 * c2][ph]), lrelu4_builtin(acc[row][2 * c2 + 1][ph]));
                    if (!interior && !(y0 + RPW * wave + row < p.H && (unsigned)(x0 + 16 * ph + q) < (unsigned)p.W))
                        hk[c2] = make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    f32x4 zz = {0.f, 0.f, 0.f, 0.f};
                    zz = Op<T>::mfma16(frag[(2 * dx) * 64], hk[0], zz);
                    zz = Op<T>::mfma16(frag[(2 * dx + 1) * 64], hk[1], zz);
                    z[dx][ph] = zz;
                }
            }
            // r(x) = (z[0](x - 1) + z[1](x)) + z[2](x + 1); region columns 0 and 31 are no outputs, what they sum is never read
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float zl[2], zr[2];
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) {
                    zl[ph] = lane_read(lane_l, z[0][ph][j]);
                    zr[ph] = lane_read(lane_r, z[2][ph][j]);
                }
                r[row][0][j] = (zl[0] + z[1][0][j]) + (q == 15 ? zr[1] : zr[0]);
                r[row][1][j] = ((q == 0 ? zl[0] : zl[1]) + z[1][1][j]) + zr[1];
            }
            r[row][0][3] = 0.f;
            r[row][1][3] = 0.f;
        }
        __syncthreads();   // every wave is done reading the last item's stage: it becomes the exchange of r
        float4* S = reinterpret_cast<float4*>(lds + ((n - 1) % NA) * ACT_REGION);   // [dy][tile row][region column]
        if (sl < 3) {
#pragma unroll
            for (int row = 0; row < RPW; ++row)
#pragma unroll
                for (int ph = 0; ph < 2; ++ph)
                    S[(sl * TILE_H + RPW * wave + row) * TILE_W + 16 * ph + q] =
                        make_float4(r[row][ph][0], r[row][ph][1], r[row][ph][2], 0.f);
        }
        __syncthreads();
        // one output pixel per thread: out row o of the step = image row y0 - 1 + o, region column cp
        {
            const int o = RPW * wave + (lane >> 5), cp = lane & 31;
            const bool col_top = y0 == 0;
            const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 a0, a1;
            if (wave == 0) {   // rows 0, 1 of the step: r_0 / r_1 of the step above
                const float4 c0 = carry[(o == 0 ? 0 : 2) * TILE_W + cp];
                const float4 c1 = o == 0 ? carry[TILE_W + cp] : S[(TILE_H + 0) * TILE_W + cp];
                a0 = col_top ? zero4 : c0;
                a1 = (col_top && o == 0) ? zero4 : c1;
            } else {
                a0 = S[(o - 2) * TILE_W + cp];
                a1 = S[(TILE_H + o - 1) * TILE_W + cp];
            }
            const float4 a2 = S[(2 * TILE_H + o) * TILE_W + cp];
            if (wave == 0) {   // the carry of the next step, behind this wave's reads of the old one
                carry[lane] = S[(lane < 32 ? 14 : TILE_H + 15) * TILE_W + cp];
                if (lane < 32) carry[2 * TILE_W + cp] = S[15 * TILE_W + cp];
            }
            const float cr = ((bias_l[64] + a0.x) + a1.x) + a2.x;
            const float cg = ((bias_l[65] + a0.y) + a1.y) + a2.y;
            const float cb = ((bias_l[66] + a0.z) + a1.z) + a2.z;
            const int y = y0 - 1 + o, x = x0 + cp;
            if (t >= t_lo && cp >= 1 && cp <= HL_TW && y >= 0 && y < p.H && x < p.W && y < p.img_H && x < p.img_W) {
                const size_t pix = (size_t)y * p.img_W + x;
                if (p.out_rgb) {
                    float* op = p.out_rgb + pix * 3;
                    op[0] = cr;
                    op[1] = cg;
                    op[2] = cb;
                }
                if (p.out_u16) {
                    uint16_t* op = p.out_u16 + pix * 3;
                    op[0] = (uint16_t)rintf(fminf(fmaxf(cb, 0.f), 1.f) * 65535.f);
                    op[1] = (uint16_t)rintf(fminf(fmaxf(cg, 0.f), 1.f) * 65535.f);
                    op[2] = (uint16_t)rintf(fminf(fmaxf(cr, 0.f), 1.f) * 65535.f);
                }
                if (p.out_u8) {
                    uint8_t* op = p.out_u8 + pix * 3;
                    op[0] = (uint8_t)rintf(fminf(fmaxf(cb, 0.f), 1.f) * 255.f);
                    op[1] = (uint8_t)rintf(fminf(fmaxf(cg, 0.f), 1.f) * 255.f);
                    op[2] = (uint8_t)rintf(fminf(fmaxf(cr, 0.f), 1.f) * 255.f);
                }
            }
        }
    }
}

// FW_RRDB_HR_LAST unset: fused when a workgroup gets at least six steps - a run's warm-up step and the uneven last round weigh
// less and less (the rule of pair_slide_enabled, conv3x3_pair_slide.hip)
bool hr_last_default(int H, int W) {
    const long tiles = (long)((W + HL_TW - 1) / HL_TW) * ((H + TILE_H) / TILE_H);
    return tiles >= 6L * conv_num_cus();
}

void launch_conv3x3_hr_last(DType dt, const ConvParams& hr, const void* wlast, const float* bias_last, hipStream_t stream) {
    HrLastParams hp{};
    hp.p = hr;
    hp.p.zeros = conv_zero_page();
    hp.wlast = wlast;
    hp.blast = bias_last;
    const ConvParams& p = hp.p;
    if (p.H <= 0 || p.W <= 0) throw Error(1, "conv3x3_hr_last: empty problem");
    if (p.cin_chunks != 2) throw Error(1, "conv3x3_hr_last: conv_hr contracts 64 channels");
    if (!p.in || !p.wpk || !p.bias || !wlast || !bias_last) throw Error(1, "conv3x3_hr_last: NULL argument");
    if (p.upsample2x || p.n_groups > 1 || p.out_f32 || p.res1 || p.res2 || p.out_lo || p.chan_scale)
        throw Error(1, "conv3x3_hr_last: unsupported conv_hr field");
    if (p.in_cstride < 32 || (p.in_cstride & 7) || p.in_pstride < 32 || (p.in_pstride & 7) ||
        (p.in_pstride == 32 && p.in_cstride < 64 && (long)p.H * p.W > 1))
        throw Error(1, "conv3x3_hr_last: bad input channel/plane stride");
    if (p.img_H <= 0 || p.img_W <= 0 || p.img_H > p.H || p.img_W > p.W) throw Error(1, "conv3x3_hr_last: bad image size");
    if (!p.out_u8 && !p.out_u16 && !p.out_rgb) throw Error(1, "conv3x3_hr_last: no output");
    const int tiles = ((p.W + HL_TW - 1) / HL_TW) * ((p.H + TILE_H) / TILE_H);
    const int ncu = conv_num_cus();
    dim3 grid(tiles < ncu ? tiles : ncu), block(64 * NWAVES);
    if (dt == DT_BF16)
        hipLaunchKernelGGL(conv3x3_hr_last_kernel<__bf16>, grid, block, 0, stream, hp);
    else
        hipLaunchKernelGGL(conv3x3_hr_last_kernel<_Float16>, grid, block, 0, stream, hp);
    FW_HIP_CHECK(hipGetLastError());
}

// conv_last's weights w[3][64][3][3] as the six A fragments of the pointwise step: [dx][chunk c2][lane][j], value =
//   w[c][ch = 32 c2 + 8 ls(lane >> 4) + j][dy][dx]   with D row lane & 15 = 4 dy + c (dy, c < 3; zero elsewhere)
// where ls(s) = s odd ? 2 + s / 2 : s / 2 is the slot of the chunk a lane of group s holds after pair16 (conv_common.h).
size_t pack_conv_last_pointwise(DType dt, const float* w, uint16_t* dst) {
    const size_t n = (size_t)HL_FRAGS * 64 * 8;
    if (!dst) return n;
    size_t o = 0;
    for (int dx = 0; dx < 3; ++dx)
        for (int c2 = 0; c2 < 2; ++c2)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int row = lane & 15, s = lane >> 4;
                    const int dy = row >> 2, c = row & 3;
                    const int ls = (s & 1) ? 2 + (s >> 1) : (s >> 1);
                    const int ch = 32 * c2 + 8 * ls + j;
                    float val = 0.f;
                    if (dy < 3 && c < 3) val = w[((size_t)c * 64 + ch) * 9 + dy * 3 + dx];
                    dst[o++] = f32_to_operand(dt, val);
                }
    return n;
}

}  // namespace fw
