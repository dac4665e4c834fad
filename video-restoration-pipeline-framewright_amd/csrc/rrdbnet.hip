// RRDBNet (Real-ESRGAN generator) forward on one MI355X: launch sequencing, workspace and weights.
//
// Architecture: basicsr RRDBNet as constructed by the reference at
// src/framewright/processors/pytorch_realesrgan.py:103-129; block arithmetic as spelled out in-tree at
// src/framewright/processors/aesrgan_face.py:171-204 (ResidualDenseBlock, RRDB) and :249-269 (trunk + tail).
// Data layout: the torch.cat([x, x1, x2, x3, x4]) of a residual dense block is never
// materialised by copying — each RDB owns a 192-channel NHWC "concat" buffer, conv k reads its first
// 64+32(k-1) channels and writes its 32 outputs into the next channel slice.  The residual trunk
// (x5*0.2 + x, and the RRDB-level *0.2 + x) is carried in fp32 side buffers so operand rounding does not
// accumulate over the 69 blocks.
#include <mutex>
#include <vector>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include "engine_common.h"

namespace fw {

struct ConvLayer {
    int cout = 0, cin = 0, ct = 0, chunks = 0;
    DevBuf d_w, d_b;            // packed weight fragments (pack_conv3x3_weights); fp32 bias, zero padded to 32 * ct
    DevBuf d_wphase;            // conv_up1 / conv_up2: the same weights as four 2x2 phase convolutions (conv_up2x_phase.hip)
    DevBuf d_wwino;             // conv5 of a dense block, f16: the same weights as row-wise Winograd fragments (conv3x3_wino.hip)
    DevBuf d_wlast;             // conv_last: the same weights as the pointwise fragments of the fused tail (conv3x3_hr_last.hip)
    bool set = false;
};

}  // namespace fw

using namespace fw;

struct fw_rrdbnet : fw::EngineBase {
    int num_block = 0;
    int scale = 4;
    DType dt = DT_BF16;
    ConvLayer conv_first, conv_body, conv_up1, conv_up2, conv_hr, conv_last;
    std::vector<ConvLayer> body;  // [num_block][3][5]
    int fuse_mask = 3;       // bit 0: conv1+conv2, bit 1: conv3+conv4 (FW_RRDB_FUSE_MASK, for A/B runs)
    bool fuse_pairs = true;  // conv1+conv2 / conv3+conv4 in one kernel (FW_RRDB_FUSE_PAIRS=0 disables, for A/B runs)
    // residual trunk as typed hi + typed lo planes (EPI_RESIDUAL_SPLIT): the residual adds run on the matrix cores as
    // identity chunks and conv5's epilogue loads nothing (FW_RRDB_SPLIT_TRUNK=0 selects the fp32 trunk, for A/B runs)
    bool split_trunk = true;
    // split trunk: lo planes only for the RRDB-level trunk (FW_RRDB_LO=0 keeps a lo plane pair behind every RDB, for A/B runs)
    bool rrdb_lo = true;
    // TIMING-ONLY ablation (wrong pixels): bit 0 - the pair kernels, bit 1 - conv5 read every input chunk from (almost) the same
    // plane, so their HBM reads collapse to about one plane at unchanged MACs: what a launch would cost if its inputs were
    // already on chip (FW_RRDB_ABL_ALIAS; DESIGN.md section 6 uses it to price fusions before building them)
    int abl_alias = 0;
    // conv_up1 / conv_up2 (nearest x2 + 3x3) as four 2x2 phase convolutions on the source grid: 4 instead of 9 taps per output pixel
    // (FW_RRDB_UP_PHASE=0 keeps the gathering nine-tap form, for A/B runs)
    bool up_phase = true;
    // conv5 as a row-wise Winograd F(2, 3): two thirds of the MFMAs (f16 only; conv3x3_wino.hip).  FW_RRDB_C5_WINO: 0 never, 1 (default)
    // rdb1 / rdb2 - no residual planes: 69.4 -> 67.6 ms per 1080p frame -, 2 rdb3 as well (its residual-plane variant spills 17 registers
    // and is 1 ms SLOWER than the direct kernel there: profiles/r03_ab/conv5_winograd_rows.txt)
    int c5_wino = 1;
    bool hr_wino = false;   // conv_hr at the output resolution in the same form (FW_RRDB_HR_WINO=1)
    // conv_hr + conv_last in one launch, the 64-channel map at the output resolution never stored (conv3x3_hr_last.hip).
    // FW_RRDB_HR_LAST: 0 never, 1 always, unset (-1): when a workgroup gets at least six steps (hr_last_default)
    int hr_last = -1;
    int abl_rdb3 = 0;   // TIMING-ONLY ablation of rdb3's conv5 (wrong pixels): 1 no lo write, 2 no R lo planes, 4 no R hi planes (FW_RRDB_ABL_RDB3)
    // hipGraph capture of the per-frame forward (BASELINE configs[4] "hipGraph-captured per-frame stages").  graph_mode: 0 never
    // (default), 1 always, 2 for frames of at most graph_max_px input pixels.  Off by default because it buys nothing here: the
    // launches of a forward run back to back at 1080p, and even a 48x64 frame through 3 blocks takes 0.61 ms either way (the
    // persistent 256-workgroup kernels, not the launches, set the floor) - tests/test_rrdbnet_gpu.py prints both.  One executable
    // graph per (frame size, sample bits, buffer pointers), rebuilt when the workspace moves.  FW_RRDB_GRAPH=0|1|2,
    // FW_RRDB_GRAPH_MAX_PX.
    int graph_mode = 0;
    long graph_max_px = 512L * 512L;
    bool warmed = false;
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    double prof_flops = 0;
    hipStream_t prof_stream = nullptr;
    ~fw_rrdbnet() {   // (destroy_engine: on the handle's device)
        for (auto e : ev_pool) (void)hipEventDestroy(e);
    }
};

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Trunk (low-resolution) size for an H x W input.
void trunk_size(const fw_rrdbnet* n, int H, int W, int* Ht, int* Wt) {
    if (n->scale == 2) {
        *Ht = (H + 1) / 2;
        *Wt = (W + 1) / 2;
    } else {
        *Ht = H;
        *Wt = W;
    }
}

struct Plan {
    size_t in_u8, out_u8, in32, cat0, cat1, cat2, F, R, tA, tB, U1, U2, U3, total;
};

Plan make_plan(const fw_rrdbnet* n, int H, int W) {
    int Ht, Wt;
    trunk_size(n, H, W, &Ht, &Wt);
    const size_t px = (size_t)Ht * Wt;
    const size_t s = (size_t)n->scale;
    Plan p{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += align_up(bytes, 256);
        return at;
    };
    p.in_u8 = take((size_t)H * W * 3 * 2);            // staging of host frames: up to 16 bits per sample
    p.out_u8 = take((size_t)H * W * 3 * s * s * 2);
    p.in32 = take(px * 32 * 2);
    // concat buffers: 6 planes of 32 channels (x, x1..x4); the split trunk adds planes 6-7 (lo part of x) and a third
    // buffer, which keeps the RRDB input alive until rdb3's second residual
    const size_t cat_bytes = px * (n->split_trunk ? 256 : 192) * 2;
    p.cat0 = take(cat_bytes);
    p.cat1 = take(cat_bytes);
    const size_t trunk = f32_native_elems(Ht, Wt, 2) * 4;  // fp32 trunk buffers, accumulator-native layout
    p.F = take(trunk);
    if (n->split_trunk) {
        p.cat2 = take(cat_bytes);
    } else {
        p.R = take(trunk);
        p.tA = take(trunk);
        p.tB = take(trunk);
    }
    p.U1 = take(px * 4 * 64 * 2);
    p.U2 = take(px * 16 * 64 * 2);
    p.U3 = take(px * 16 * 64 * 2);
    p.total = o;
    return p;
}

ConvLayer* find_layer(fw_rrdbnet* n, const std::string& key, int* want_cout, int* want_cin) {
    const int in_ch = n->scale == 2 ? 12 : 3;
    auto ret = [&](ConvLayer* l, int co, int ci) {
        *want_cout = co;
        *want_cin = ci;
        return l;
    };
    if (key == "conv_first") return ret(&n->conv_first, 64, in_ch);
    if (key == "conv_body") return ret(&n->conv_body, 64, 64);
    if (key == "conv_up1") return ret(&n->conv_up1, 64, 64);
    if (key == "conv_up2") return ret(&n->conv_up2, 64, 64);
    if (key == "conv_hr") return ret(&n->conv_hr, 64, 64);
    if (key == "conv_last") return ret(&n->conv_last, 3, 64);
    int b = -1, r = -1, c = -1;
    char tail = 0;
    if (sscanf(key.c_str(), "body.%d.rdb%d.conv%d%c", &b, &r, &c, &tail) == 3 && b >= 0 && b < n->num_block && r >= 1 &&
        r <= 3 && c >= 1 && c <= 5) {
        ConvLayer* l = &n->body[((size_t)b * 3 + (r - 1)) * 5 + (c - 1)];
        return ret(l, c == 5 ? 64 : 32, 64 + 32 * (c - 1));
    }
    return nullptr;
}

// one packed form of a layer's weights on the device: sized by the packer's nullptr call, packed on the host, uploaded
template <typename Pack>
void upload_packed(DevBuf& b, const float* weight, Pack&& pack) {
    std::vector<uint16_t> pk(pack(nullptr, nullptr));
    pack(weight, pk.data());
    upload(b, pk.data(), pk.size() * 2);
}

double conv_flops(const ConvLayer& l, size_t pixels) { return 2.0 * 9.0 * l.cin * l.cout * (double)pixels; }

// Runs `launch` on `st`; with profiling on, between two events of the pool and with its algorithmic `flops` added to the count
template <typename F>
void timed(fw_rrdbnet* n, hipStream_t st, double flops, F&& launch) {
    if (!n->profile) {
        launch();
        return;
    }
    if (n->ev_used + 2 > n->ev_pool.size()) {
        size_t old = n->ev_pool.size();
        n->ev_pool.resize(old + 1024);
        for (size_t i = old; i < n->ev_pool.size(); ++i) FW_HIP_CHECK(hipEventCreate(&n->ev_pool[i]));
    }
    FW_HIP_CHECK(hipEventRecord(n->ev_pool[n->ev_used++], st));
    launch();
    FW_HIP_CHECK(hipEventRecord(n->ev_pool[n->ev_used++], st));
    n->prof_flops += flops;
    n->prof_stream = st;
}

void run_conv(fw_rrdbnet* n, const ConvLayer& l, ConvEpilogue epi, ConvParams p, hipStream_t st) {
    p.cin_chunks = l.chunks;
    p.wpk = l.d_w.p;
    p.bias = (const float*)l.d_b.p;
    timed(n, st, conv_flops(l, (size_t)p.H * p.W), [&] { launch_conv3x3(n->dt, l.ct, epi, p, st); });
}

void run_pair(fw_rrdbnet* n, const ConvLayer& a, const ConvLayer& b, const ConvPairParams& q, hipStream_t st) {
    // algorithmic FLOPs, no recompute
    timed(n, st, conv_flops(a, (size_t)q.H * q.W) + conv_flops(b, (size_t)q.H * q.W), [&] { launch_conv3x3_pair(n->dt, q, st); });
}

// The trunk of a forward in the handle's workspace, as forward() and fw_rrdbnet_run_rrdbs see it
struct Trunk {
    int Ht = 0, Wt = 0;
    int ncat = 2;       // concat buffers in rotation: 3 on the split trunk (the RRDB input stays alive until rdb3's second residual)
    long PL = 0;        // elements of one plane: a 192-channel concat buffer is 6 planes of [Ht][Wt][32] (+ planes 6-7: the lo part of x)
    void* cat[3] = {};
    float *F = nullptr, *R = nullptr, *tA = nullptr, *tB = nullptr;   // fp32 trunk buffers, accumulator-native layout
    ConvParams base{};  // what every conv of the trunk starts from
};

void* plane(void* buf, int chunk, long pl) { return (void*)((char*)buf + (size_t)chunk * pl * 2); }

Trunk make_trunk(const fw_rrdbnet* n, const Plan& pl, int Ht, int Wt) {
    char* ws = (char*)n->ws.p;
    Trunk T;
    T.Ht = Ht;
    T.Wt = Wt;
    T.ncat = n->split_trunk ? 3 : 2;
    T.PL = (long)Ht * Wt * 32;
    T.cat[0] = ws + pl.cat0;
    T.cat[1] = ws + pl.cat1;
    T.cat[2] = ws + pl.cat2;
    T.F = (float*)(ws + pl.F);
    T.R = (float*)(ws + pl.R);
    T.tA = (float*)(ws + pl.tA);
    T.tB = (float*)(ws + pl.tB);
    T.base.H = Ht;
    T.base.W = Wt;
    T.base.s1 = 1.f;
    T.base.s2 = 1.f;
    T.base.in_cstride = 32;
    T.base.in_pstride = T.PL;
    T.base.out_cstride = 32;
    T.base.out_pstride = T.PL;
    T.base.f32_native = 1;
    return T;
}

// whether conv c + 1 and conv c + 2 of a dense block (c = 0, 2) run as one launch
bool pair_fused(const fw_rrdbnet* n, int c) { return n->fuse_pairs && (n->fuse_mask >> (c >> 1) & 1); }

// residual planes of rdb k's conv5 on the split trunk: x lo (unless the lo planes are kept at RRDB granularity) and, for rdb3, R hi + R lo
int c5_planes(const fw_rrdbnet* n, int k) { return n->rrdb_lo ? (k == 2 ? 4 : 0) : (k == 2 ? 6 : 2); }

// whether a conv5 with n_id residual planes takes the Winograd kernel: the one place that decides it, for run_rrdb and for
// fw_rrdbnet_block_paths
bool c5_on_wino(const fw_rrdbnet* n, int n_id, const ConvLayer& c5) {
    return n->c5_wino && n->dt == DT_F16 && (n_id == 0 || n->c5_wino >= 2) && c5.d_wwino.p && !(n->abl_alias & 2) && !n->abl_rdb3;
}

// RRDB b of the trunk.  cur: the concat buffer whose planes 0-1 (split trunk: + 6-7) hold its input, on return the one that holds its
// output; Rin: the fp32 trunk buffer of its input (fp32 trunk only; the output goes to R).
void run_rrdb(fw_rrdbnet* n, const Trunk& T, int b, const float* Rin, int& cur, hipStream_t st) {
    void* const* cat = T.cat;
    const int ncat = T.ncat, Ht = T.Ht, Wt = T.Wt;
    const long PL = T.PL;
    const ConvParams& base = T.base;
    float *R = T.R, *tA = T.tA, *tB = T.tB;
    const int rrdb_in = cur;  // split trunk: planes 0-1 of this buffer stay the RRDB input until rdb3 overwrites them
    for (int k = 0; k < 3; ++k) {
        const ConvLayer* L = &n->body[((size_t)b * 3 + k) * 5];
        // conv1..conv4: growth channels, LeakyReLU(0.2), written into the next plane    (:184-187);
        // fused in pairs (conv1+conv2, conv3+conv4): the shared input chunks leave HBM once per pair
        for (int c = 0; c < 4; c += 2) {
            if (pair_fused(n, c)) {
                ConvPairParams q{};
                q.in = cat[cur];
                q.in_cstride = 32;
                q.in_pstride = (n->abl_alias & 1) ? 40 : PL;
                q.na = 2 + c;
                q.H = Ht;
                q.W = Wt;
                q.wpk_a = L[c].d_w.p;
                q.bias_a = (const float*)L[c].d_b.p;
                q.wpk_b = L[c + 1].d_w.p;
                q.bias_b = (const float*)L[c + 1].d_b.p;
                q.out_a = plane(cat[cur], 2 + c, PL);
                q.out_b = plane(cat[cur], 3 + c, PL);
                q.out_cstride = 32;
                run_pair(n, L[c], L[c + 1], q, st);
            } else {
                for (int cc = c; cc < c + 2; ++cc) {
                    ConvParams p = base;
                    p.in = cat[cur];
                    p.out = plane(cat[cur], 2 + cc, PL);
                    p.act = 1;
                    run_conv(n, L[cc], EPI_STORE, p, st);
                }
            }
        }
        // conv5 + residual(s): x5*0.2 + x  (:188-189); after rdb3 additionally *0.2 + rrdb_in (:204)
        ConvParams p = base;
        const int nxt = (cur + 1) % ncat;
        p.in = cat[cur];
        p.out = cat[nxt];
        p.s1 = 0.2f;
        if (n->abl_alias & 2) p.in_pstride = 40;
        if (n->split_trunk) {
            // y = 0.2*conv5 + x           = 0.2  * (conv5 + 5*x)            x = planes 0,1 (hi) + 6,7 (lo) of cat[cur]
            // y = (0.2*conv5 + x)*0.2 + R = 0.04 * (conv5 + 5*x + 25*R)     R = the same planes of cat[rrdb_in]
            // x hi is added from conv chunks 0,1 while they sit in LDS; residual planes: x lo (6,7) [, R hi (0,1), R lo
            // (6,7)].  Each tile consumes its residual pixels before it stores, so rdb3 updates the RRDB input in place
            // (nxt == rrdb_in).
            const long PB = PL * 2;  // bytes per plane
            const long r_off = (char*)cat[rrdb_in] - (char*)cat[cur];
            p.in_id_scale = 5.f;
            if (n->rrdb_lo) {
                // lo planes at RRDB granularity: rdb1 / rdb2 carry their output as the typed planes alone (what they lose
                // - half an ulp of the operand type, once each - reaches the RRDB output scaled by 0.2), and only the
                // RRDB-level trunk R keeps hi + lo.  rdb1 takes its residual from R hi (the centre tap in LDS), rdb3
                // adds R hi + R lo and writes hi + lo.  Per RRDB 4 lo-plane transfers instead of 16; measured against
                // the fp32 oracle the f16 path moves from 3.0-3.7e-4 to 3.4-3.8e-4 max-abs.
                p.n_id = c5_planes(n, k);
                if (k == 2) {
                    p.out_lo = plane(cat[nxt], 6, PL);
                    p.chunk_off[0] = r_off;              // R hi
                    p.chunk_off[1] = r_off + PB;
                    p.chunk_off[2] = r_off + 6 * PB;     // R lo
                    p.chunk_off[3] = r_off + 7 * PB;
                    for (int i = 0; i < 4; ++i) p.id_scale[i] = 25.f;
                    if (n->abl_rdb3 & 1) {
                        p.out_lo = nullptr;
                    }
                    if (n->abl_rdb3 & 2) p.n_id = 2;
                    if ((n->abl_rdb3 & 6) == 6) p.n_id = 0;
                    else if (n->abl_rdb3 & 4) {
                        p.n_id = 2;
                        p.chunk_off[0] = p.chunk_off[2];
                        p.chunk_off[1] = p.chunk_off[3];
                    }
                }
            } else {
                p.out_lo = plane(cat[nxt], 6, PL);
                p.n_id = c5_planes(n, k);
                p.chunk_off[0] = 6 * PB;
                p.chunk_off[1] = 7 * PB;
                p.id_scale[0] = p.id_scale[1] = 5.f;
                if (k == 2) {
                    p.chunk_off[2] = r_off;              // R hi
                    p.chunk_off[3] = r_off + PB;
                    p.chunk_off[4] = r_off + 6 * PB;     // R lo
                    p.chunk_off[5] = r_off + 7 * PB;
                    for (int i = 2; i < 6; ++i) p.id_scale[i] = 25.f;
                }
            }
            p.s1 = (k == 2) ? 0.2f * 0.2f : 0.2f;
            if (c5_on_wino(n, p.n_id, L[4])) {
                p.cin_chunks = L[4].chunks;
                p.wpk = L[4].d_wwino.p;
                p.bias = (const float*)L[4].d_b.p;
                // algorithmic FLOPs: the nine-tap count
                timed(n, st, conv_flops(L[4], (size_t)p.H * p.W), [&] { launch_conv3x3_wino_split(p, st); });
            } else {
                run_conv(n, L[4], EPI_RESIDUAL_SPLIT, p, st);
            }
        } else {
            p.res1 = (k == 0) ? Rin : (k == 1 ? tA : tB);
            if (k == 2) {
                p.res2 = Rin;
                p.s2 = 0.2f;
                p.out_f32 = R;
            } else {
                p.out_f32 = (k == 0) ? tA : tB;
            }
            run_conv(n, L[4], EPI_RESIDUAL, p, st);
        }
        cur = nxt;
    }
}

// The two ends of a forward in the handle's workspace, as forward(), fw_rrdbnet_run_head and fw_rrdbnet_run_tail see them
struct Ends {
    void *in32 = nullptr, *U1 = nullptr, *U2 = nullptr, *U3 = nullptr;
};

Ends make_ends(const fw_rrdbnet* n, const Plan& pl) {
    char* ws = (char*)n->ws.p;
    Ends E;
    E.in32 = ws + pl.in32;
    E.U1 = ws + pl.U1;
    E.U2 = ws + pl.U2;
    E.U3 = ws + pl.U3;
    return E;
}

// whether an up-conv runs as four 2x2 phase convolutions, conv_hr in the Winograd form, and conv_hr + conv_last as one launch on a
// trunk of Ht x Wt pixels: the one place that decides each, for run_tail and for fw_rrdbnet_tail_paths
bool up_on_phase(const fw_rrdbnet* n, const ConvLayer& l) { return n->up_phase && l.d_wphase.p; }
bool hr_on_wino(const fw_rrdbnet* n) { return n->c5_wino && n->dt == DT_F16 && n->conv_hr.d_wwino.p && n->hr_wino; }
bool tail_fused(const fw_rrdbnet* n, int Ht, int Wt) {
    return !hr_on_wino(n) && (n->hr_last < 0 ? hr_last_default(4 * Ht, 4 * Wt) : n->hr_last != 0);
}

// The head of a forward: frame -> NHWC, conv_first -> concat buffer 0 [0:64] (split trunk: + its lo planes) and the fp32 trunk F.
// bits = 8: d_in is uint8 BGR; bits = 16: uint16 BGR (range 65535)
void run_head(fw_rrdbnet* n, const Trunk& T, const Ends& E, const void* d_in, int bits, int H, int W, hipStream_t st) {
    launch_frame_to_nhwc(n->dt, d_in, bits, H, W, E.in32, 32, n->scale == 2 ? 2 : 1, st);
    // conv_first -> concat buffer 0 [0:64] + fp32 trunk F          (aesrgan_face.py:250)
    ConvParams p = T.base;
    p.in = E.in32;
    p.out = T.cat[0];
    p.out_f32 = T.F;
    if (n->split_trunk) p.out_lo = plane(T.cat[0], 6, T.PL);
    run_conv(n, n->conv_first, EPI_STORE, p, st);
}

// The tail of a forward: from the trunk behind the last RRDB in concat buffer `cur` and conv_first's fp32 output F to the image of
// img_H x img_W pixels (bits = 8: d_out is uint8 BGR; bits = 16: uint16 BGR) and / or the float RGB plane.
void run_tail(fw_rrdbnet* n, const Trunk& T, const Ends& E, int cur, int bits, int img_H, int img_W, void* d_out, float* d_rgb, hipStream_t st) {
    void* const* cat = T.cat;
    const int ncat = T.ncat, Ht = T.Ht, Wt = T.Wt;
    const long PL = T.PL;
    const ConvParams& base = T.base;
    float* F = T.F;
    void *U1 = E.U1, *U2 = E.U2, *U3 = E.U3;
    // feat + conv_body(body_feat)                                                  (:256-257)
    {
        ConvParams p = base;
        p.in = cat[cur];
        p.out = cat[(cur + 1) % ncat];
        p.res1 = F;
        p.s1 = 1.f;
        run_conv(n, n->conv_body, EPI_RESIDUAL, p, st);
        cur = (cur + 1) % ncat;
    }
    // lrelu(conv_up1(nearest x2)), lrelu(conv_up2(nearest x2))                    (:260-266)
    auto run_up = [&](const ConvLayer& l, const void* src, long src_pstride, int Hs, int Ws, void* dst, long dst_pstride) {
        if (up_on_phase(n, l)) {
            ConvUpParams u{};
            u.in = src;
            u.in_cstride = 32;
            u.in_pstride = src_pstride;
            u.H = Hs;
            u.W = Ws;
            u.wpk = l.d_wphase.p;
            u.bias = (const float*)l.d_b.p;
            u.act = 1;
            u.out = dst;
            u.out_cstride = 32;
            u.out_pstride = dst_pstride;
            // algorithmic FLOPs: the nine-tap count of the reference's conv
            timed(n, st, conv_flops(l, (size_t)4 * Hs * Ws), [&] { launch_conv_up2x_phase(n->dt, u, st); });
        } else {
            ConvParams p = base;
            p.H = 2 * Hs;
            p.W = 2 * Ws;
            p.in = src;
            p.in_pstride = src_pstride;
            p.upsample2x = 1;
            p.out = dst;
            p.out_pstride = dst_pstride;
            p.act = 1;
            run_conv(n, l, EPI_STORE, p, st);
        }
    };
    run_up(n->conv_up1, cat[cur], PL, Ht, Wt, U1, 4 * PL);
    run_up(n->conv_up2, U1, 4 * PL, 2 * Ht, 2 * Wt, U2, 16 * PL);
    // conv_last(lrelu(conv_hr(feat)))                                              (:268)
    ConvParams hr = base;
    hr.H = 4 * Ht;
    hr.W = 4 * Wt;
    hr.in = U2;
    hr.in_pstride = 16 * PL;
    ConvParams img = base;
    img.H = 4 * Ht;
    img.W = 4 * Wt;
    if (bits == 16)
        img.out_u16 = (uint16_t*)d_out;
    else
        img.out_u8 = (uint8_t*)d_out;
    img.out_rgb = d_rgb;
    img.img_H = img_H;  // crops the mod-pad of the x2 model
    img.img_W = img_W;
    const bool hr_wino = hr_on_wino(n);
    if (tail_fused(n, Ht, Wt)) {
        // one launch, U3 never written: the algorithmic FLOPs of both convs
        ConvParams p = hr;
        p.out_u8 = img.out_u8;
        p.out_u16 = img.out_u16;
        p.out_rgb = img.out_rgb;
        p.img_H = img.img_H;
        p.img_W = img.img_W;
        p.cin_chunks = n->conv_hr.chunks;
        p.wpk = n->conv_hr.d_w.p;
        p.bias = (const float*)n->conv_hr.d_b.p;
        const size_t px = (size_t)p.H * p.W;
        timed(n, st, conv_flops(n->conv_hr, px) + conv_flops(n->conv_last, px),
              [&] { launch_conv3x3_hr_last(n->dt, p, n->conv_last.d_wlast.p, (const float*)n->conv_last.d_b.p, st); });
        return;
    }
    {
        ConvParams p = hr;
        p.out = U3;
        p.out_pstride = 16 * PL;
        p.act = 1;
        if (hr_wino) {
            p.cin_chunks = n->conv_hr.chunks;
            p.wpk = n->conv_hr.d_wwino.p;
            p.bias = (const float*)n->conv_hr.d_b.p;
            timed(n, st, conv_flops(n->conv_hr, (size_t)p.H * p.W), [&] { launch_conv3x3_wino_store(p, st); });
        } else {
            run_conv(n, n->conv_hr, EPI_STORE, p, st);
        }
    }
    {
        ConvParams p = img;
        p.in = U3;
        p.in_pstride = 16 * PL;
        run_conv(n, n->conv_last, EPI_IMAGE, p, st);
    }
}

// bits = 8: d_in / d_out are uint8 BGR; bits = 16: uint16 BGR (range 65535)
void forward(fw_rrdbnet* n, const void* d_in, int bits, int H, int W, void* d_out, float* d_rgb, hipStream_t st) {
    int Ht, Wt;
    trunk_size(n, H, W, &Ht, &Wt);
    const Plan pl = make_plan(n, H, W);
    const Trunk T = make_trunk(n, pl, Ht, Wt);
    const Ends E = make_ends(n, pl);
    run_head(n, T, E, d_in, bits, H, W, st);
    int cur = 0;
    for (int b = 0; b < n->num_block; ++b) run_rrdb(n, T, b, b == 0 ? T.F : T.R, cur, st);
    run_tail(n, T, E, cur, bits, n->scale * H, n->scale * W, d_out, d_rgb, st);
}

}  // namespace

extern "C" {

int fw_rrdbnet_create(int device_id, int num_block, int scale, int dtype, fw_rrdbnet** out) {
    if (!out) return fail(FW_ERR_INVALID, "fw_rrdbnet_create: out is NULL");
    *out = nullptr;
    if (num_block < 1 || num_block > 64) return fail(FW_ERR_INVALID, "fw_rrdbnet_create: num_block out of range");
    if (scale != 2 && scale != 4) return fail(FW_ERR_INVALID, "fw_rrdbnet_create: scale must be 2 or 4");
    if (dtype != FW_DTYPE_BF16 && dtype != FW_DTYPE_F16) return fail(FW_ERR_INVALID, "fw_rrdbnet_create: bad dtype");
    return guarded([&] {
        int ndev = 0;
        FW_HIP_CHECK(hipGetDeviceCount(&ndev));
        if (device_id < 0 || device_id >= ndev) throw Error(FW_ERR_INVALID, "fw_rrdbnet_create: no such device");
        auto n = std::make_unique<fw_rrdbnet>();
        n->device = device_id;
        n->num_block = num_block;
        n->scale = scale;
        n->dt = (DType)dtype;
        n->body.resize((size_t)num_block * 15);
        if (const char* e = getenv("FW_RRDB_FUSE_PAIRS")) n->fuse_pairs = atoi(e) != 0;
        if (const char* e = getenv("FW_RRDB_FUSE_MASK")) n->fuse_mask = atoi(e) & 3;
        if (const char* e = getenv("FW_RRDB_GRAPH")) n->graph_mode = atoi(e);
        if (const char* e = getenv("FW_RRDB_GRAPH_MAX_PX")) n->graph_max_px = atol(e);
        if (const char* e = getenv("FW_RRDB_SPLIT_TRUNK")) n->split_trunk = atoi(e) != 0;
        if (const char* e = getenv("FW_RRDB_LO")) n->rrdb_lo = atoi(e) != 0;
        if (const char* e = getenv("FW_RRDB_ABL_ALIAS")) n->abl_alias = atoi(e);
        if (const char* e = getenv("FW_RRDB_UP_PHASE")) n->up_phase = atoi(e) != 0;
        if (const char* e = getenv("FW_RRDB_ABL_RDB3")) n->abl_rdb3 = atoi(e);
        if (const char* e = getenv("FW_RRDB_C5_WINO")) n->c5_wino = atoi(e);
        if (const char* e = getenv("FW_RRDB_HR_WINO")) n->hr_wino = atoi(e) != 0;
        if (const char* e = getenv("FW_RRDB_HR_LAST")) n->hr_last = atoi(e) != 0;
        *out = n.release();
    });
}

int fw_rrdbnet_set_conv(fw_rrdbnet* n, const char* key, const float* weight, const float* bias, int cout, int cin) {
    if (!n || !key || !weight || !bias) return fail(FW_ERR_INVALID, "fw_rrdbnet_set_conv: NULL argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(n->mu);
        int wco = 0, wci = 0;
        ConvLayer* l = find_layer(n, key, &wco, &wci);
        if (!l) throw Error(FW_ERR_INVALID, std::string("fw_rrdbnet_set_conv: unknown key '") + key + "'");
        if (cout != wco || cin != wci)
            throw Error(FW_ERR_INVALID, std::string("fw_rrdbnet_set_conv: shape mismatch for '") + key + "': got [" +
                                            std::to_string(cout) + "," + std::to_string(cin) + ",3,3], expected [" +
                                            std::to_string(wco) + "," + std::to_string(wci) + ",3,3]");
        DevGuard dg(n->device);
        *l = ConvLayer();   // a layer set again: its previous buffers go first
        l->cout = cout;
        l->cin = cin;
        l->ct = (cout + 31) / 32;
        l->chunks = (cin + 31) / 32;
        const DType dt = n->dt;
        upload_packed(l->d_w, weight, [&](const float* w, uint16_t* dst) { return pack_conv3x3_weights(dt, w, cout, cin, l->ct, l->chunks, dst); });
        std::vector<float> b(32 * l->ct, 0.f);
        for (int i = 0; i < cout; ++i) b[i] = bias[i];
        upload(l->d_b, b.data(), b.size() * 4);
        if (n->dt == DT_F16 && cout == 64 && (cin == 192 || l == &n->conv_hr))   // a dense block's conv5; conv_hr of the tail
            upload_packed(l->d_wwino, weight, [&](const float* w, uint16_t* dst) { return pack_conv3x3_wino_weights(dt, w, cout, cin, l->chunks, dst); });
        if (l == &n->conv_last)
            upload_packed(l->d_wlast, weight, [&](const float* w, uint16_t* dst) { return pack_conv_last_pointwise(dt, w, dst); });
        if (l == &n->conv_up1 || l == &n->conv_up2)
            upload_packed(l->d_wphase, weight, [&](const float* w, uint16_t* dst) { return pack_conv_up2x_phase_weights(dt, w, dst); });
        l->set = true;
    });
}

int fw_rrdbnet_finalize(fw_rrdbnet* n) {
    if (!n) return fail(FW_ERR_INVALID, "fw_rrdbnet_finalize: NULL");
    std::lock_guard<std::mutex> lk(n->mu);
    const ConvLayer* singles[] = {&n->conv_first, &n->conv_body, &n->conv_up1, &n->conv_up2, &n->conv_hr, &n->conv_last};
    const char* names[] = {"conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"};
    for (int i = 0; i < 6; ++i)
        if (!singles[i]->set) return fail(FW_ERR_INVALID, std::string("fw_rrdbnet_finalize: missing ") + names[i]);
    for (size_t i = 0; i < n->body.size(); ++i)
        if (!n->body[i].set)
            return fail(FW_ERR_INVALID, "fw_rrdbnet_finalize: missing body." + std::to_string(i / 15) + ".rdb" +
                                            std::to_string((i / 5) % 3 + 1) + ".conv" + std::to_string(i % 5 + 1));
    return FW_OK;
}

size_t fw_rrdbnet_workspace_bytes(const fw_rrdbnet* n, int H, int W) {
    if (!n || H < 1 || W < 1) return 0;
    return make_plan(n, H, W).total;
}

double fw_rrdbnet_flops(const fw_rrdbnet* n, int H, int W) {
    if (!n || H < 1 || W < 1) return 0.0;
    int Ht, Wt;
    trunk_size(n, H, W, &Ht, &Wt);
    const double px = (double)Ht * Wt;
    const double in_ch = n->scale == 2 ? 12 : 3;
    double mac = 9.0 * in_ch * 64;                                             // conv_first
    mac += n->num_block * 3.0 * 9.0 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64);  // RRDB trunk
    mac += 9.0 * 64 * 64;                                                      // conv_body
    mac += 9.0 * 64 * 64 * 4;                                                  // conv_up1 at 2x
    mac += 9.0 * 64 * 64 * 16 * 2;                                             // conv_up2, conv_hr at 4x
    mac += 9.0 * 64 * 3 * 16;                                                  // conv_last
    return 2.0 * mac * px;
}

static int upscale_any(fw_rrdbnet* n, const void* in_bgr, int in_loc, int bits, int H, int W, void* out_bgr, int out_loc,
                       float* out_rgb_f32, void* stream, const char* who) {
    const std::string w(who);
    if (!n || !in_bgr) return fail(FW_ERR_INVALID, w + ": NULL argument");
    if (!out_bgr && !out_rgb_f32) return fail(FW_ERR_INVALID, w + ": no output requested");
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(FW_ERR_INVALID, w + ": bad frame size");
    if (n->scale == 2 && (H < 2 || W < 2)) return fail(FW_ERR_INVALID, w + ": x2 needs >= 2x2 input");
    if ((in_loc != FW_HOST && in_loc != FW_DEVICE) || (out_loc != FW_HOST && out_loc != FW_DEVICE))
        return fail(FW_ERR_INVALID, w + ": bad buffer location");
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    return guarded([&] {
        EngineCall call(n, stream);
        hipStream_t st = call.st;
        const Plan pl = make_plan(n, H, W);
        reserve_workspace(n, pl.total);
        char* ws = (char*)n->ws.p;
        const size_t in_bytes = (size_t)H * W * 3 * (bits / 8);
        const size_t out_bytes = in_bytes * n->scale * n->scale;
        const void* d_in = in_bgr;
        if (in_loc == FW_HOST) {
            void* stage = ws + pl.in_u8;
            FW_HIP_CHECK(hipMemcpyAsync(stage, in_bgr, in_bytes, hipMemcpyHostToDevice, st));
            d_in = stage;
        }
        void* d_out = out_bgr;
        if (out_bgr && out_loc == FW_HOST) d_out = ws + pl.out_u8;
        // (the engine's first forward always runs uncaptured: one-time initialisations inside the launchers must not land in a
        // capture)
        const bool graphed = n->warmed && !n->profile &&
                             (n->graph_mode == 1 || (n->graph_mode == 2 && (long)H * W <= n->graph_max_px));
        n->warmed = true;
        if (!graphed) {
            forward(n, d_in, bits, H, W, d_out, out_rgb_f32, st);
        } else {
            const GraphCache::Key key = {(uint64_t)H, (uint64_t)W, (uint64_t)bits, (uint64_t)d_in, (uint64_t)d_out, (uint64_t)out_rgb_f32};
            n->graphs.launch(key, st, [&](hipStream_t cs) { forward(n, d_in, bits, H, W, d_out, out_rgb_f32, cs); });
        }
        if (out_bgr && out_loc == FW_HOST) {
            FW_HIP_CHECK(hipMemcpyAsync(out_bgr, d_out, out_bytes, hipMemcpyDeviceToHost, st));
            FW_HIP_CHECK(hipStreamSynchronize(st));
        }
    });
}

int fw_rrdbnet_upscale_u8(fw_rrdbnet* n, const uint8_t* in_bgr, int in_loc, int H, int W, uint8_t* out_bgr,
                          int out_loc, float* out_rgb_f32, void* stream) {
    return upscale_any(n, in_bgr, in_loc, 8, H, W, out_bgr, out_loc, out_rgb_f32, stream, "fw_rrdbnet_upscale_u8");
}

int fw_rrdbnet_upscale_u16(fw_rrdbnet* n, const uint16_t* in_bgr, int in_loc, int H, int W, uint16_t* out_bgr,
                           int out_loc, float* out_rgb_f32, void* stream) {
    return upscale_any(n, in_bgr, in_loc, 16, H, W, out_bgr, out_loc, out_rgb_f32, stream, "fw_rrdbnet_upscale_u16");
}

// ---- RRDBs of the trunk on their own, for tests and tools: the launches a forward makes for them, on a caller's fp32 trunk ----
int fw_rrdbnet_run_rrdbs(fw_rrdbnet* n, int first_block, int count, const float* trunk_in_f32, int Ht, int Wt, float* trunk_out_f32,
                         void* growth_out, void* stream) {
    if (!n || !trunk_in_f32 || !trunk_out_f32) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_rrdbs: NULL argument");
    const int fs = n->scale == 2 ? 2 : 1;   // frame pixels per trunk pixel and side (the x2 model's trunk is half its frame)
    if (Ht < 1 || Wt < 1 || Ht > 16384 / fs || Wt > 16384 / fs) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_rrdbs: bad trunk size");
    if (first_block < 0 || count < 1 || first_block >= n->num_block || count > n->num_block - first_block)
        return fail(FW_ERR_INVALID, "fw_rrdbnet_run_rrdbs: blocks " + std::to_string(first_block) + " .. " + std::to_string((long)first_block + count - 1) +
                                        " are not all inside a net of " + std::to_string(n->num_block));
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    return guarded([&] {
        EngineCall call(n, stream);
        hipStream_t st = call.st;
        // the workspace of the forward whose trunk has Ht x Wt pixels
        const Plan pl = make_plan(n, fs * Ht, fs * Wt);
        reserve_workspace(n, pl.total);
        const Trunk T = make_trunk(n, pl, Ht, Wt);
        // what a forward holds on entering first_block: three RDBs per RRDB, each moving on by one buffer
        int cur = 3 * first_block % T.ncat;
        float* Rin = first_block == 0 ? T.F : T.R;
        launch_trunk_from_f32(n->dt, trunk_in_f32, Ht, Wt, T.PL, T.cat[cur], n->split_trunk ? plane(T.cat[cur], 6, T.PL) : nullptr,
                              n->split_trunk ? nullptr : Rin, st);
        int last = cur;
        for (int b = first_block; b < first_block + count; ++b) {
            run_rrdb(n, T, b, b == 0 ? T.F : T.R, cur, st);
            last = (cur + T.ncat - 1) % T.ncat;   // rdb3 ran in the buffer in front of the one it wrote to
        }
        launch_trunk_to_f32(n->dt, T.cat[cur], n->split_trunk ? plane(T.cat[cur], 6, T.PL) : nullptr, n->split_trunk ? nullptr : T.R, Ht, Wt, T.PL,
                            trunk_out_f32, st);
        if (growth_out)   // x1 .. x4 of the last RDB: planes 2-5 of its concat buffer, contiguous
            FW_HIP_CHECK(hipMemcpyAsync(growth_out, plane(T.cat[last], 2, T.PL), (size_t)4 * T.PL * 2, hipMemcpyDeviceToDevice, st));
    });
}

int fw_rrdbnet_block_paths(fw_rrdbnet* n, int* flags) {
    if (!n || !flags) return fail(FW_ERR_INVALID, "fw_rrdbnet_block_paths: NULL argument");
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    std::lock_guard<std::mutex> lk(n->mu);
    const ConvLayer* c5 = &n->body[4];   // conv5 of body.0.rdb1; every dense block has the same form
    // pair_fused, c5_planes and c5_on_wino are what run_rrdb consults
    *flags = (pair_fused(n, 0) ? FW_RRDB_PATH_PAIR12 : 0) | (pair_fused(n, 2) ? FW_RRDB_PATH_PAIR34 : 0) | (n->split_trunk ? FW_RRDB_PATH_SPLIT_TRUNK : 0) |
             (n->split_trunk && n->rrdb_lo ? FW_RRDB_PATH_RRDB_LO : 0) |
             (n->split_trunk && c5_on_wino(n, c5_planes(n, 0), c5[0]) ? FW_RRDB_PATH_C5_WINO_RDB12 : 0) |
             (n->split_trunk && c5_on_wino(n, c5_planes(n, 2), c5[10]) ? FW_RRDB_PATH_C5_WINO_RDB3 : 0);
    return FW_OK;
}

// ---- the two ends of a forward on their own, for tests and tools: the launches a forward makes in front of RRDB 0 and behind the last ----
int fw_rrdbnet_run_head(fw_rrdbnet* n, const void* in_bgr, int bits, int H, int W, float* trunk_out_f32, float* feat_out_f32, void* stream) {
    if (!n || !in_bgr || !trunk_out_f32 || !feat_out_f32) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_head: NULL argument");
    if (bits != 8 && bits != 16) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_head: 8- or 16-bit samples expected");
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_head: bad frame size");
    if (n->scale == 2 && (H < 2 || W < 2)) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_head: x2 needs >= 2x2 input");
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    return guarded([&] {
        EngineCall call(n, stream);
        hipStream_t st = call.st;
        int Ht, Wt;
        trunk_size(n, H, W, &Ht, &Wt);
        const Plan pl = make_plan(n, H, W);
        reserve_workspace(n, pl.total);
        const Trunk T = make_trunk(n, pl, Ht, Wt);
        run_head(n, T, make_ends(n, pl), in_bgr, bits, H, W, st);
        // what RRDB 0 reads: the planes of concat buffer 0, or the fp32 trunk F; and F itself, which conv_body adds later
        launch_trunk_to_f32(n->dt, T.cat[0], n->split_trunk ? plane(T.cat[0], 6, T.PL) : nullptr, n->split_trunk ? nullptr : T.F, Ht, Wt, T.PL,
                            trunk_out_f32, st);
        launch_trunk_to_f32(n->dt, nullptr, nullptr, T.F, Ht, Wt, T.PL, feat_out_f32, st);
    });
}

int fw_rrdbnet_run_tail(fw_rrdbnet* n, const float* feat_f32, const float* trunk_f32, int Ht, int Wt, int img_H, int img_W, int bits, void* out_bgr,
                        float* out_rgb_f32, void* stream) {
    if (!n || !feat_f32) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: NULL argument");
    if (!out_bgr && !out_rgb_f32) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: no output requested");
    if (bits != 8 && bits != 16) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: 8- or 16-bit samples expected");
    const int fs = n->scale == 2 ? 2 : 1;   // frame pixels per trunk pixel and side
    if (Ht < 1 || Wt < 1 || Ht > 16384 / fs || Wt > 16384 / fs) return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: bad trunk size");
    // the image of a frame whose trunk has Ht x Wt pixels: scale x the frame, and the x2 model's frame may be one short of 2 x its trunk
    const int H = img_H / n->scale, W = img_W / n->scale;
    int Hc = 0, Wc = 0;
    if (img_H >= n->scale && img_W >= n->scale && (n->scale != 2 || (H >= 2 && W >= 2))) trunk_size(n, H, W, &Hc, &Wc);
    if (img_H < 1 || img_W < 1 || img_H % n->scale || img_W % n->scale || Hc != Ht || Wc != Wt)
        return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: bad image size: " + std::to_string(img_H) + " x " + std::to_string(img_W) +
                                        " is not the output of a frame whose trunk has " + std::to_string(Ht) + " x " + std::to_string(Wt) + " pixels");
    // run_rrdbs works in the workspace of the frame that fills its trunk: only that frame's tail finds the trunk where it was left
    if (!trunk_f32 && (img_H != 4 * Ht || img_W != 4 * Wt))
        return fail(FW_ERR_INVALID, "fw_rrdbnet_run_tail: the trunk left by run_rrdbs serves the uncropped image alone (bad image size)");
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    return guarded([&] {
        EngineCall call(n, stream);
        hipStream_t st = call.st;
        const Plan pl = make_plan(n, H, W);
        reserve_workspace(n, pl.total);
        const Trunk T = make_trunk(n, pl, Ht, Wt);
        // the buffer a forward holds behind its last RRDB: three RDBs per RRDB, each moving on by one buffer
        const int cur = 3 * n->num_block % T.ncat;
        // (trunk_f32 == NULL: the buffer as fw_rrdbnet_run_rrdbs through the last block left it - the typed planes themselves, where the
        // fp32 sum of a hi + lo pair cannot say which pair it was when it lies half-way between two numbers of the operand type)
        if (trunk_f32)
            launch_trunk_from_f32(n->dt, trunk_f32, Ht, Wt, T.PL, T.cat[cur], n->split_trunk ? plane(T.cat[cur], 6, T.PL) : nullptr,
                                  n->split_trunk ? nullptr : T.R, st);
        launch_trunk_from_f32(n->dt, feat_f32, Ht, Wt, T.PL, nullptr, nullptr, T.F, st);   // conv_first's fp32 output alone
        run_tail(n, T, make_ends(n, pl), cur, bits, img_H, img_W, out_bgr, out_rgb_f32, st);
    });
}

int fw_rrdbnet_tail_paths(fw_rrdbnet* n, int Ht, int Wt, int* flags) {
    if (!n || !flags) return fail(FW_ERR_INVALID, "fw_rrdbnet_tail_paths: NULL argument");
    const int fs = n->scale == 2 ? 2 : 1;
    if (Ht < 1 || Wt < 1 || Ht > 16384 / fs || Wt > 16384 / fs) return fail(FW_ERR_INVALID, "fw_rrdbnet_tail_paths: bad trunk size");
    int rc = fw_rrdbnet_finalize(n);
    if (rc != FW_OK) return rc;
    std::lock_guard<std::mutex> lk(n->mu);
    // up_on_phase, tail_fused and hr_on_wino are what run_tail consults
    *flags = (up_on_phase(n, n->conv_up1) && up_on_phase(n, n->conv_up2) ? FW_RRDB_TAIL_UP_PHASE : 0) | (tail_fused(n, Ht, Wt) ? FW_RRDB_TAIL_FUSED : 0) |
             (hr_on_wino(n) ? FW_RRDB_TAIL_HR_WINO : 0);
    return FW_OK;
}

int fw_rrdbnet_profile_enable(fw_rrdbnet* n, int on) {
    if (!n) return fail(FW_ERR_INVALID, "fw_rrdbnet_profile_enable: NULL");
    std::lock_guard<std::mutex> lk(n->mu);
    n->profile = on != 0;
    n->ev_used = 0;
    n->prof_flops = 0;
    return FW_OK;
}

int fw_rrdbnet_profile_read(fw_rrdbnet* n, int* launches, double* total_ms, double* total_flops) {
    if (!n) return fail(FW_ERR_INVALID, "fw_rrdbnet_profile_read: NULL");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(n->mu);
        DevGuard dg(n->device);
        double ms = 0;
        if (n->ev_used) FW_HIP_CHECK(hipEventSynchronize(n->ev_pool[n->ev_used - 1]));
        for (size_t i = 0; i + 1 < n->ev_used; i += 2) {
            float t = 0;
            FW_HIP_CHECK(hipEventElapsedTime(&t, n->ev_pool[i], n->ev_pool[i + 1]));
            ms += t;
        }
        if (launches) *launches = (int)(n->ev_used / 2);
        if (total_ms) *total_ms = ms;
        if (total_flops) *total_flops = n->prof_flops;
        n->ev_used = 0;
        n->prof_flops = 0;
    });
}

int fw_rrdbnet_destroy(fw_rrdbnet* n) { return destroy_engine(n); }

}  // extern "C"
