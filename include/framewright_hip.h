/*
 * framewright_hip.h — C-ABI of libframewright_hip.so, the MI355X (gfx950 / CDNA4) drop-in for the
 * conv-net hot path of FrameWright (Real-ESRGAN upscale, NAFNet temporal denoise, RIFE interpolation).
 *
 * The reference (/root/reference, pure Python) has no native boundary of its own: the arithmetic is
 * delegated to third-party torch modules / external binaries.  Each entry point below therefore names the
 * reference call it replaces (file:line relative to the reference tree), and INTEGRATION.md shows the
 * ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, 1 = invalid argument, 2 = GPU out of memory
 *     (message contains "memory", so restorer.py:1746's tile-downshift retry still triggers),
 *     3 = HIP runtime error, 4 = internal error.  fw_last_error() returns the message for the calling thread.
 *   - plain pointers and sizes only; buffers are caller-owned.  `loc` arguments say where a buffer lives:
 *     FW_HOST (pageable or pinned host memory) or FW_DEVICE (hipMalloc'd / torch.cuda memory on the
 *     handle's device).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous on
 *     that stream when every buffer is FW_DEVICE; calls with FW_HOST buffers return after the copy back.
 *   - one handle per GPU; calls on one handle are serialised by an internal mutex, so the reference's
 *     ThreadPoolExecutor callers (restorer.py:1894) may share a handle.  A handle owns ONE workspace: when two
 *     FW_DEVICE calls on it are enqueued on different streams, the second stream waits (hipStreamWaitEvent) for an
 *     event the first call recorded behind its last kernel, so the device work of a handle never overlaps whatever
 *     the streams; callers that WANT two forwards in flight create one handle per stream.
 *   - images are H x W x 3 uint8 in BGR order (cv2 convention, plugins/base.py:186-250).
 */
#ifndef FRAMEWRIGHT_HIP_H
#define FRAMEWRIGHT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_OK 0
#define FW_ERR_INVALID 1
#define FW_ERR_OOM 2
#define FW_ERR_HIP 3
#define FW_ERR_INTERNAL 4

#define FW_HOST 0
#define FW_DEVICE 1

/* operand (MFMA input / activation storage) type; accumulation is always fp32 */
#define FW_DTYPE_BF16 0
#define FW_DTYPE_F16 1

typedef struct fw_rrdbnet fw_rrdbnet;
typedef struct fw_nafnet fw_nafnet;

/* -------------------------------------------------------------------------------------------------
 * Library
 * ------------------------------------------------------------------------------------------------- */

/* Message of the last failing call on this thread ("" if none).  Never NULL. */
const char* fw_last_error(void);

/* ABI version of this header: 4.  Bumped whenever an existing entry point changes (1 -> 2, 2 -> 3 and 3 -> 4 were additive: a
 * binder of version 1, 2 or 3 keeps working against this library).  Additive entries no longer bump the version: the flicker
 * reduction entries (fw_bgr_to_lab_u8 ... fw_gamma_lab_tables) were added at version 4, so a binder that needs them looks the
 * symbols up instead of comparing versions. */
int fw_abi_version(void);

/* Number of visible HIP devices (0 when there is no GPU; never fails). */
int fw_device_count(void);

/* -------------------------------------------------------------------------------------------------
 * Real-ESRGAN: RRDBNet generator
 * replaces  basicsr RRDBNet construction + RealESRGANer(...) in get_upsampler()
 *           (processors/pytorch_realesrgan.py:85-173) and upsampler.enhance() (:223,:227;
 *           processors/enhancement/super_resolution.py:524).
 * ------------------------------------------------------------------------------------------------- */

/* Create an RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block, num_grow_ch=32, scale) on
 * `device_id`.  scale in {2,4} (pytorch_realesrgan.py:103-129: x4plus nb=23, anime_6B nb=6, x2plus nb=23). */
int fw_rrdbnet_create(int device_id, int num_block, int scale, int dtype, fw_rrdbnet** out);

/* Upload one convolution.  `key` is the BasicSR state-dict prefix ("conv_first", "body.7.rdb2.conv4",
 * "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"); weight is torch layout
 * [cout][cin][3][3] fp32 (host memory), bias [cout] fp32.  Weights are converted to the operand type
 * (round to nearest even) and packed into MFMA fragments. */
int fw_rrdbnet_set_conv(fw_rrdbnet* net, const char* key, const float* weight, const float* bias, int cout,
                        int cin);

/* Verify that every convolution of the architecture has been uploaded. */
int fw_rrdbnet_finalize(fw_rrdbnet* net);

/* One frame: uint8 BGR H x W x 3 -> uint8 BGR (scale*H) x (scale*W) x 3.
 * Equivalent to RealESRGANer.enhance(img, outscale=scale) for a 3-channel uint8 image with tile=0,
 * pre_pad=0: BGR->RGB, /255, (x2 model: reflect mod-pad to even + pixel_unshuffle(2)), RRDBNet forward,
 * clamp(0,1), *255, round-half-even, RGB->BGR.  If out_rgb_f32 is non-NULL (device memory,
 * (scale*H) x (scale*W) x 3 floats, RGB order) the un-clamped network output is stored there as well
 * (used by the parity tests to measure max-abs before quantisation).  out_bgr may be NULL then. */
int fw_rrdbnet_upscale_u8(fw_rrdbnet* net, const uint8_t* in_bgr, int in_loc, int height, int width,
                          uint8_t* out_bgr, int out_loc, float* out_rgb_f32, void* stream);

/* The same for a 16-bit frame (uint16 BGR, range 65535): RealESRGANer.enhance takes this branch when the image maximum
 * exceeds 256 (cv2.imread(IMREAD_UNCHANGED) of a 16-bit PNG, reference pytorch_realesrgan.py:200-227): /65535 on the way in,
 * clamp(0,1) * 65535, round-half-even, uint16 on the way out. */
int fw_rrdbnet_upscale_u16(fw_rrdbnet* net, const uint16_t* in_bgr, int in_loc, int height, int width,
                           uint16_t* out_bgr, int out_loc, float* out_rgb_f32, void* stream);

/* Bytes of device workspace the net needs for an H x W input (0 on invalid arguments). */
size_t fw_rrdbnet_workspace_bytes(const fw_rrdbnet* net, int height, int width);

/* Algorithmic FLOPs (2 x MAC, un-padded channel counts) of one forward on an H x W input. */
double fw_rrdbnet_flops(const fw_rrdbnet* net, int height, int width);

/* Per-launch timing: when enabled, every conv launch of subsequent upscale calls is bracketed by HIP events on
 * the launch stream.  fw_rrdbnet_profile_read synchronises the stream and returns the number of conv
 * launches timed since the last read, their summed duration (ms) and summed algorithmic FLOPs. */
int fw_rrdbnet_profile_enable(fw_rrdbnet* net, int on);
int fw_rrdbnet_profile_read(fw_rrdbnet* net, int* launches, double* total_ms, double* total_flops);

/* RRDBs of the trunk on their own, on the caller's device buffers (tests, tools): the same launches, workspace, mutex and stream
 * ordering as fw_rrdbnet_upscale_u8 makes for those blocks, dispatched by the handle's own switches (FW_RRDB_* read at create,
 * FW_PAIR_SLIDE per launch).
 * run_rrdbs: RRDBs first_block .. first_block + count - 1 on a trunk of height x width pixels (the trunk's resolution; the model's
 *   scale plays no part), starting with the concat buffer (3 * first_block mod the buffers in rotation) and the residual source a
 *   forward holds on entering first_block.  trunk_in_f32: device fp32 [height][width][64], laid into the engine's representation -
 *   split trunk: typed hi = T(x) in planes 0-1 and typed lo = T(x - float(hi)) in planes 6-7; fp32 trunk: the typed planes and the
 *   fp32 buffer in the accumulator-native layout.  trunk_out_f32: device fp32 [height][width][64], the last RRDB's output
 *   (float(hi) + float(lo), or the fp32 trunk).  growth_out (optional, device, operand-typed [4][height][width][32]): x1 .. x4 of the
 *   last dense block run, planes 2-5 of its concat buffer.  FW_ERR_INVALID: a block range outside the net, a handle that is not
 *   finalised, a non-positive size.
 * block_paths: which kernel forms the RRDBs of this handle dispatch to, as FW_RRDB_PATH_* bits. */
#define FW_RRDB_PATH_PAIR12 1         /* conv1 + conv2 in one launch */
#define FW_RRDB_PATH_PAIR34 2         /* conv3 + conv4 in one launch */
#define FW_RRDB_PATH_SPLIT_TRUNK 4    /* the trunk as typed hi + lo planes, residual adds on the matrix cores */
#define FW_RRDB_PATH_RRDB_LO 8        /* lo planes behind rdb3 only: rdb1 / rdb2 hand on the typed planes alone */
#define FW_RRDB_PATH_C5_WINO_RDB12 16 /* conv5 of rdb1 / rdb2 as row-wise Winograd F(2, 3) */
#define FW_RRDB_PATH_C5_WINO_RDB3 32  /* conv5 of rdb3 in its residual-plane Winograd form */
int fw_rrdbnet_run_rrdbs(fw_rrdbnet* net, int first_block, int count, const float* trunk_in_f32, int height, int width,
                         float* trunk_out_f32, void* growth_out, void* stream);
int fw_rrdbnet_block_paths(fw_rrdbnet* net, int* flags);

/* The two ends of a forward on their own, on the caller's device buffers (tests, tools): the same launches, workspace, mutex and
 * stream ordering as fw_rrdbnet_upscale_u8 / _u16 makes in front of RRDB 0 and behind the last RRDB.  run_head, run_rrdbs over
 * every block and run_tail together are the forward.
 * run_head: frame -> NHWC (bits 8: uint8 BGR / 255; bits 16: uint16 BGR / 65535; the x2 model's reflect mod-pad and pixel-unshuffle)
 *   and conv_first on a device frame of height x width pixels.  trunk_out_f32: device fp32 [Ht][Wt][64] at the trunk's resolution
 *   (the frame's; the x2 model's: ceil(height / 2) x ceil(width / 2)), what RRDB 0 reads - float(hi) + float(lo) of the typed planes,
 *   or the fp32 trunk.  feat_out_f32: the same shape, conv_first's fp32 output as conv_body adds it later.
 * run_tail: conv_body + feat, the two up-convs, conv_hr and conv_last from a trunk of trunk_height x trunk_width pixels.  trunk_f32:
 *   device fp32 [trunk_height][trunk_width][64], laid into the concat buffer a forward holds behind its last RRDB (3 * num_block mod
 *   the buffers in rotation) as run_rrdbs lays in - or NULL: that buffer is read as it stands, which after a run_rrdbs through the
 *   last block on a trunk of the same size (same handle, nothing in between; the uncropped image only, whose frame's workspace
 *   run_rrdbs works in) is the trunk itself, typed pair for typed pair: the fp32
 *   sum of hi + lo does not say which pair it was where it lies half-way between two numbers of the operand type, and conv_body
 *   reads hi alone.  feat_f32: the same shape, laid into conv_first's fp32 buffer.  img_height x
 *   img_width: the image, scale x a frame whose trunk has that size (the x2 model crops its mod-pad: 4 * trunk - 2 or 4 * trunk per
 *   side).  out_bgr: device, uint8 (bits 8) or uint16 (bits 16) BGR [img_height][img_width][3]; out_rgb_f32: device fp32 RGB of the
 *   same shape, the un-clamped network output; either may be NULL, not both.
 * tail_paths: which kernel forms the tail dispatches to on a trunk of that size, as FW_RRDB_TAIL_* bits.
 * FW_ERR_INVALID: NULL arguments, a handle that is not finalised, bits other than 8 or 16, a size outside a forward's range, an x2
 *   frame under 2 x 2, an image that is not the output of a frame with that trunk. */
#define FW_RRDB_TAIL_UP_PHASE 1   /* conv_up1 / conv_up2 as four 2x2 phase convolutions on the source grid */
#define FW_RRDB_TAIL_FUSED 2      /* conv_hr + conv_last in one launch (depends on the size when FW_RRDB_HR_LAST is unset) */
#define FW_RRDB_TAIL_HR_WINO 4    /* conv_hr as row-wise Winograd F(2, 3) */
int fw_rrdbnet_run_head(fw_rrdbnet* net, const void* in_bgr, int bits, int height, int width, float* trunk_out_f32,
                        float* feat_out_f32, void* stream);
int fw_rrdbnet_run_tail(fw_rrdbnet* net, const float* feat_f32, const float* trunk_f32, int trunk_height, int trunk_width,
                        int img_height, int img_width, int bits, void* out_bgr, float* out_rgb_f32, void* stream);
int fw_rrdbnet_tail_paths(fw_rrdbnet* net, int trunk_height, int trunk_width, int* flags);

/* Release device memory.  NULL is allowed. */
int fw_rrdbnet_destroy(fw_rrdbnet* net);

/* -------------------------------------------------------------------------------------------------
 * Operator-level entry points (used by the parity tests; the model calls above use the same kernels).
 * All pointers are device memory on `device_id`'s current context; tensors are NHWC.
 * ------------------------------------------------------------------------------------------------- */

/* Pack a torch-layout conv weight [cout][cin][3][3] (host fp32) into MFMA fragments (host uint16 buffer).
 * Returns the number of uint16 elements (call with dst = NULL to size the buffer).  cout is padded to
 * 32*cout_tiles, cin to 32*cin_chunks. */
size_t fw_pack_conv3x3(int dtype, const float* weight, int cout, int cin, int cout_tiles, int cin_chunks,
                       uint16_t* dst);

/* y = act(conv3x3(x) + bias) written to channels [out_coff, out_coff + 32*cout_tiles) of an NHWC operand-typed
 * buffer.  x: operand-typed; pixel (y,x) of 32-channel chunk c starts at element
 * c*in_plane_stride + (y*W + x)*in_cstride.  in_plane_stride = 0 (or 32) is plain interleaved NHWC with in_cstride
 * channels per pixel; in_plane_stride = H*W*in_cstride with in_cstride = 32 is the chunk-planar layout the RRDB
 * trunk uses (every chunk read is a contiguous stream of whole cache lines).  The first 32*cin_chunks channels are
 * contracted.  The two 32-channel halves of a 64-channel output are out_plane_stride elements apart (0 = 32).
 * upsample2x = 1: x is (H/2 x W/2) and is nearest-neighbour upsampled on the fly (conv_up1/conv_up2 of
 * aesrgan_face.py:258-266).  res1/res2 (fp32 NHWC, 32*cout_tiles channels, may be NULL):
 *   res1 == NULL:  y = act(acc + bias)
 *   res1 != NULL:  y = (acc + bias) * s1 + res1; if res2: y = y * s2 + res2     (aesrgan_face.py:189,204)
 * out / out_f32 may each be NULL. */
int fw_conv3x3_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int height,
                    int width, const void* packed_weight, const float* bias, int cout_tiles, int act_lrelu,
                    int upsample2x, const float* res1, float s1, const float* res2, float s2, void* out,
                    int out_cstride, long out_plane_stride, int out_coff, float* out_f32, void* stream);

/* Same, with the extras the IFNet blocks need: chan_scale (fp32 [32*cout_tiles] or NULL) multiplies (acc + bias) per
 * output channel before the residual add, post_act = 1 applies LeakyReLU(0.2) AFTER the residual add
 * (ResConv: lrelu(conv(x) * beta + x)), and f32_cstride / f32_coff place res1 / res2 / out_f32 in a
 * channel slice of a wider fp32 NHWC buffer (0 / 0 = a dense 32*cout_tiles-channel buffer). */
int fw_conv3x3_nhwc_ex(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int height,
                       int width, const void* packed_weight, const float* bias, int cout_tiles, int act_lrelu,
                       int upsample2x, const float* res1, float s1, const float* res2, float s2, const float* chan_scale,
                       int post_act, int f32_cstride, int f32_coff, void* out, int out_cstride, long out_plane_stride,
                       int out_coff, float* out_f32, void* stream);

/* act_lrelu == 2 in fw_conv3x3_nhwc_ex (res1 == NULL): PReLU, y = max(t, 0) + chan_scale[n] * min(t, 0) with t = acc + bias —
 * the activation of SRVGGNetCompact (realesr-animevideov3, realesr-general-x4v3). */

/* uint8 BGR H x W x 3 -> operand-typed [H][W][out_cstride] RGB/255 in channels 0..2, zeros above (out_cstride >= 32).
 * replaces  img.astype(float32)/255 + BGR->RGB + HWC->CHW of RealESRGANer.pre_process (third-party; call site
 *           processors/pytorch_realesrgan.py:223). */
int fw_u8_to_nhwc(int dtype, const uint8_t* in_bgr, int height, int width, void* out, int out_cstride, void* stream);

/* SRVGGNetCompact tail: out = PixelShuffle(scale)(conv) + nearest-upsample(input), conv = fp32 [H][W][conv_cstride] with
 * channel c*scale^2 + i*scale + j; RGB float [scale*H][scale*W][3] and/or clamp -> x255 -> rint -> uint8 BGR.
 * replaces  the tail of the SRVGGNetCompact forward (third-party `realesrgan.archs.srvgg_arch`; the reference declares
 *           these checkpoints at processors/pytorch_realesrgan.py:119-128). */
int fw_pixel_shuffle_add_u8(const float* conv, int conv_cstride, const uint8_t* in_bgr, int height, int width, int scale,
                            uint8_t* out_bgr, float* out_rgb_f32, void* stream);

/* Two chained growth convolutions of a residual dense block in one kernel (aesrgan_face.py:184-187):
 *   x_a = lrelu(conv_a(x[0 : 32*in_chunks]) + bias_a)            (32 channels) -> out_a
 *   x_b = lrelu(conv_b(cat(x[0 : 32*in_chunks], x_a)) + bias_b)  (32 channels) -> out_b
 * packed_weight_a = fw_pack_conv3x3(cout 32, cin 32*in_chunks, 1, in_chunks), packed_weight_b likewise with
 * in_chunks + 1 (its last chunk multiplies x_a).  out_a / out_b: operand-typed, out_cstride elements per pixel.
 * The shared input chunks are fetched from HBM once for both convolutions and x_a feeds conv_b from LDS. */
int fw_conv3x3_pair_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int in_chunks, int height,
                         int width, const void* packed_weight_a, const float* bias_a, const void* packed_weight_b,
                         const float* bias_b, void* out_a, void* out_b, int out_cstride, void* stream);

/* lrelu(conv3x3(nearest_x2(x)) + bias), 64 -> 64 channels (conv_up1 / conv_up2, aesrgan_face.py:258-266) evaluated on the SOURCE
 * grid as four 2x2 phase convolutions with summed weights: output pixel (2y + a, 2x + b) folds its three tap rows / columns onto two
 * source rows / columns, 4 instead of 9 MFMA taps.  fw_pack_conv_up2x_phase packs a torch-layout weight [64][64][3][3] (host fp32;
 * sums in fp64, rounded to the operand type once; returns the number of uint16, dst = NULL to size the buffer).
 * x: operand-typed source image height x width, 64 channels as two 32-channel chunks in_plane_stride elements apart (0 = 32:
 * interleaved NHWC with in_cstride channels per pixel); out: operand-typed [2*height][2*width][out_cstride], its two 32-channel
 * halves out_plane_stride elements apart (0 = 32). */
size_t fw_pack_conv_up2x_phase(int dtype, const float* weight, uint16_t* dst);
int fw_conv_up2x_phase_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int height, int width,
                            const void* packed_weight, const float* bias, int act_lrelu, void* out, int out_cstride,
                            long out_plane_stride, void* stream);

/* conv5 of a residual dense block on the split trunk (64 output channels; the trunk is held as operand-typed hi planes plus lo planes
 * that keep the rounding error of the hi values):
 *   y = s1 * (conv3x3(x) + bias + in_id_scale * x[0:64] + sum_{c < n_id} id_scale[c] * plane_c);  y = lrelu(y, 0.2) if post_act
 *   out = T(y), out_lo = T(y - T(y)) (out_lo may be NULL: hi only)
 * x, the padding and strides as in fw_conv3x3_nhwc; residual plane c (32 channels) is read at byte offset chunk_off[c] from x with
 * pixel stride in_cstride and feeds output channels [32 (c & 1), 32 (c & 1) + 32).  in_id_scale and id_scale[c] must be exactly
 * representable in the operand type.  The two 32-channel halves of out / out_lo are out_plane_stride elements apart (0 = 32).
 * winograd = 0: the direct kernel, packed_weight = fw_pack_conv3x3(cout 64, cin, 2, cin_chunks).
 * winograd = 1: the row-wise Winograd F(2, 3) kernel (f16 only; no post_act), packed_weight = fw_pack_conv3x3_wino(...).
 * fw_pack_conv3x3_wino packs a torch-layout weight [cout][cin][3][3] (host fp32, cout <= 64, cin <= 32*cin_chunks) into the
 * Winograd kernel's fragments: per tap row (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2), summed in fp32 and rounded to f16
 * once.  f16 only (any other dtype returns 0); returns the number of uint16, dst = NULL to size the buffer.
 * fw_conv3x3_wino_nhwc: act(conv3x3(x) + bias) (act_lrelu 0 or 1), 64 output channels, with the Winograd kernel (conv_hr's form). */
size_t fw_pack_conv3x3_wino(int dtype, const float* weight, int cout, int cin, int cin_chunks, uint16_t* dst);
int fw_conv3x3_split_nhwc(int dtype, int winograd, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int height,
                          int width, const void* packed_weight, const float* bias, float s1, float in_id_scale, int n_id,
                          const long* chunk_off, const float* id_scale, int post_act, void* out, void* out_lo, int out_cstride,
                          long out_plane_stride, int out_coff, void* stream);
int fw_conv3x3_wino_nhwc(int dtype, const void* x, int in_cstride, long in_plane_stride, int cin_chunks, int height, int width,
                         const void* packed_weight, const float* bias, int act_lrelu, void* out, int out_cstride,
                         long out_plane_stride, int out_coff, void* stream);
/* The tail of the RRDBNet, conv_last(lrelu(conv_hr(x), 0.2)): 64 -> 64 -> 3 channels at the output resolution, written as an image
 * (out_u8: uint8 BGR = clamp -> x255 -> rint; out_u16: uint16 BGR, x65535; out_rgb_f32: float RGB, un-clamped; any of them may be
 * NULL, not all), cropped to img_height x img_width <= height x width.  x, the padding and the strides as in fw_conv3x3_nhwc.
 *   fused = 0: the two launches, conv_hr into scratch_u3 (two 32-channel planes [height][width][32] of the operand type), conv_last
 *              out of it; packed_w_hr = fw_pack_conv3x3(cout 64, cin 64, 2, 2), packed_w_last = fw_pack_conv3x3(cout 3, cin 64, 1, 2).
 *   fused = 1: one launch that keeps the 64-channel map on the chip (scratch_u3 and packed_w_last are not used);
 *              packed_w_last_pw = fw_pack_conv_last_pointwise(...).
 * bias_hr: 64 floats; bias_last: 32 floats (3 used, the rest zero).  The two forms round the 64-channel map to the operand type at
 * the same point and differ only in the fp32 summation order of conv_last.
 * fw_pack_conv_last_pointwise packs conv_last's torch-layout weight [3][64][3][3] (host fp32) into the fused form's six matrix
 * fragments; returns the number of uint16, dst = NULL to size the buffer. */
size_t fw_pack_conv_last_pointwise(int dtype, const float* weight, uint16_t* dst);
int fw_conv3x3_hr_last_nhwc(int dtype, int fused, const void* x, int in_cstride, long in_plane_stride, int height, int width,
                            const void* packed_w_hr, const float* bias_hr, const void* packed_w_last, const void* packed_w_last_pw,
                            const float* bias_last, void* scratch_u3, int img_height, int img_width, uint8_t* out_u8,
                            uint16_t* out_u16, float* out_rgb_f32, void* stream);
/* Self-check of the Winograd launchers' argument checks (host only, no device call, nothing launched): for each of the fields
 * the Winograd kernels do not implement (post_act, chan_scale, res1, res2, out_f32, n_groups > 1, act in the split form, in_id_scale /
 * id_scale not exact in f16; out_f32, n_groups, chan_scale, post_act, res1, PReLU and out_lo in the STORE form), one otherwise valid
 * problem with that field set is checked and its status (FW_ERR_INVALID when rejected, FW_OK when not) written to codes[i], i < n.
 * Returns the number of cases, or -1 when one of the unmodified valid problems is rejected (message in fw_last_error). */
int fw_conv3x3_wino_check_fields(int* codes, int n);

/* -------------------------------------------------------------------------------------------------
 * TAP temporal denoise: NAFNet
 * replaces  basicsr NAFNet construction + load in TAPDenoiser._load_nafnet (processors/tap_denoise.py:335-364),
 *           _preprocess_frame / self._model(tensor) / _postprocess_frame (:373-415, :431-434, :455-459).
 * ------------------------------------------------------------------------------------------------- */

/* NAFNet(img_channel=3, width, middle_blk_num, enc_blk_nums[num_levels], dec_blk_nums[num_levels]); the reference
 * passes width=64, middle=12, enc=[2,2,4,8], dec=[2,2,2,2] (tap_denoise.py:340-346).  width in {32, 64}. */
int fw_nafnet_create(int device_id, int width, int middle_blk_num, const int* enc_blk_nums, const int* dec_blk_nums,
                     int num_levels, int dtype, fw_nafnet** out);

/* Upload one state-dict tensor by its key (host fp32, torch layout, `numel` elements): intro.weight/bias,
 * ending.weight/bias, downs.{l}.weight/bias, ups.{i}.0.weight, {encoders.{l}.{j} | middle_blks.{j} |
 * decoders.{i}.{j}}.{norm1,norm2}.{weight,bias} / conv{1..5}.{weight,bias} / sca.1.{weight,bias} / beta / gamma. */
int fw_nafnet_set_tensor(fw_nafnet* net, const char* key, const float* data, size_t numel);
int fw_nafnet_finalize(fw_nafnet* net);

/* One frame (or tile): uint8 BGR H x W x 3 -> uint8 BGR H x W x 3.  BGR->RGB, /255, zero pad to a multiple of
 * 2^num_levels, NAFNet forward (+ input residual), crop, np.clip(x*255, 0, 255).astype(uint8) — truncation, as
 * tap_denoise.py:412 — RGB->BGR.  out_rgb_f32 (optional, device, H x W x 3 RGB) receives the un-quantised output. */
int fw_nafnet_denoise_u8(fw_nafnet* net, const uint8_t* in_bgr, int in_loc, int height, int width, uint8_t* out_bgr,
                         int out_loc, float* out_rgb_f32, void* stream);
double fw_nafnet_flops(const fw_nafnet* net, int height, int width);
int fw_nafnet_destroy(fw_nafnet* net);

/* Single steps of a forward on the caller's buffers (tests, tools): the same launches, workspace, mutex and stream ordering as
 * fw_nafnet_denoise_u8, dispatched by the handle's own switches (FW_NAF_* read at create).
 * run_block: `key` names a block like fw_nafnet_set_tensor does ("encoders.1.0.", "middle_blks.3.", "decoders.2.1."); stream_f32
 * is a device fp32 [height][width][c] buffer, updated in place; sca_out (optional, device float[c]) receives the block's SCA
 * scale.  FW_ERR_INVALID: unknown key, unfinalizable handle, non-positive size.
 * block_paths: which fused kernels that block dispatches to, as FW_NAF_PATH_* bits.
 * run_resample: up = 0: the 2x2 stride-2 conv of `level`, src fp32 [height][width][c] -> dst fp32 [height/2][width/2][2c] (even
 * sides); up = 1: the step INTO `level` (ups[num_levels - 1 - level]): src fp32 [height][width][2c'] of level + 1, 1x1 conv,
 * PixelShuffle(2), added in place to the skip buffer dst fp32 [2 height][2 width][c'], c' = width << level. */
#define FW_NAF_PATH_FRONT 1    /* norm1 + conv1 + depthwise + gate in one kernel (c = 64, 128) */
#define FW_NAF_PATH_TAIL128 2  /* conv3 .. conv5 in one kernel, c = 128 */
#define FW_NAF_PATH_TAIL64 4   /* conv3 .. conv5 in one kernel, c = 64 */
#define FW_NAF_PATH_GEMM 8     /* 1x1 convs on the pipelined GEMM kernel (c >= 256) */
#define FW_NAF_PATH_FUSE_LN 16 /* at least one LayerNorm2d of the block runs inside the staging of the conv that follows it (c = 64, a fused kernel off) */
int fw_nafnet_run_block(fw_nafnet* net, const char* key, float* stream_f32, int height, int width, float* sca_out, void* stream);
int fw_nafnet_block_paths(fw_nafnet* net, const char* key, int* flags);
int fw_nafnet_run_resample(fw_nafnet* net, int level, int up, const float* src_f32, int height, int width, float* dst_f32, void* stream);
/* NAFNet's pre-processing: uint8 BGR H x W x 3 -> typed [padded_height][padded_width][32], RGB / 255 in channels 0..2, zeros in
 * channels 3..31 and outside H x W (tap_denoise.py:373-397 + NAFNet.check_image_size). */
int fw_u8_to_nhwc_padded(int dtype, const uint8_t* in_bgr, int height, int width, int padded_height, int padded_width, void* out,
                         void* stream);

/* -------------------------------------------------------------------------------------------------
 * TAP driver arithmetic on uint8 frames (all pointers device memory; bit-exact restatements)
 * ------------------------------------------------------------------------------------------------- */

/* dst[th][tw][3] = src[y0:y0+th, x0:x0+tw]               (frame[y1:y2, x1:x2], tap_denoise.py:452) */
int fw_u8_crop(const uint8_t* src, int height, int width, int y0, int x0, int th, int tw, uint8_t* dst, void* stream);

/* output[y0:.., x0:..] += tile * tile_weight ; weight[...] += tile_weight, with the linear ramps of
 * tap_denoise.py:461-486 on the tile edges that are interior to the frame (np.linspace(0, 1, overlap)). */
int fw_tile_blend_accumulate(float* acc, float* wsum, int height, int width, const uint8_t* tile, int y0, int x0, int th,
                             int tw, int overlap, void* stream);

/* out = (output / max(weight, 1e-8)).astype(uint8)        (tap_denoise.py:484-486) */
int fw_tile_blend_finish(const float* acc, const float* wsum, int height, int width, uint8_t* out, void* stream);

/* result = sum_k float32(frame_k) * float32(w_k) accumulated in float32, .astype(uint8)   (tap_denoise.py:526-534).
 * `frames` is a HOST array of `count` (<= 16) DEVICE pointers; weights are the normalised host weights. */
int fw_temporal_average_u8(const uint8_t* const* frames, const float* weights, int count, size_t nbytes, uint8_t* out,
                           void* stream);

/* out = (original * (1 - s) + denoised * s).astype(uint8)  (tap_denoise.py:614-618); s is a double like the
 * reference's Python float: (1 - s) is formed in double, then both factors are rounded once to float32. */
int fw_strength_blend_u8(const uint8_t* original, const uint8_t* denoised, double strength, size_t nbytes, uint8_t* out,
                         void* stream);

/* preserve_grain (tap_denoise.py:621-632; motion-adaptive variant :1015-1023 with its own factor):
 *   grain = cv2.subtract(gray(original), cv2.GaussianBlur(gray(original), (0, 0), 3))
 *   out   = cv2.add(denoised, (GRAY2BGR(grain) * factor).astype(np.uint8))
 * on uint8 BGR H x W x 3 device buffers; `scratch` = height*width uint16 of device memory.  OpenCV's 8-bit fixed-point
 * arithmetic (BGR2GRAY 14-bit weights; 19-tap bit-exact Gaussian, BORDER_REFLECT_101; saturating subtract / add). */
int fw_grain_addback_u8(const uint8_t* original, const uint8_t* denoised, int height, int width, double factor,
                        uint16_t* scratch, uint8_t* out, void* stream);

/* cv2.resize(output, (int(w*outscale), int(h*outscale)), interpolation=cv2.INTER_LANCZOS4) on an 8-bit H x W x C image
 * (C <= 4; device pointers): the last step of realesrgan.RealESRGANer.enhance when outscale != netscale — reference call
 * site src/framewright/processors/pytorch_realesrgan.py:223 (`upsampler.enhance(img, outscale=config.scale_factor)`,
 * scale_factor 2 with a x4 model).  OpenCV's fixed-point arithmetic (8x8 taps, 11-bit coefficients, clamped borders);
 * synchronises `stream` before it returns. */
int fw_resize_lanczos4_u8(const uint8_t* src, int src_h, int src_w, int channels, uint8_t* dst, int dst_h, int dst_w,
                          void* stream);
/* The same on 16-bit images: RealESRGANer.enhance with outscale != netscale on a 16-bit frame (cv2.resize of a ushort image runs
 * OpenCV's float path: float weights, eight products summed left to right per pass, saturate_cast<ushort>(cvRound)). */
int fw_resize_lanczos4_u16(const uint16_t* src, int src_h, int src_w, int channels, uint16_t* dst, int dst_h, int dst_w,
                           void* stream);

/* -------------------------------------------------------------------------------------------------
 * The host arithmetic of AESRGANFaceRestorer around its network
 * replaces  `cv2.resize(enhanced_face, (target_w, target_h))` and the feathered float32 blend of `_paste_face_back`,
 *           processors/aesrgan_face.py:543-584 (the network itself: fw_aesrgan_*).  Device pointers.
 * fw_resize_linear_u8: cv2.resize with its default INTER_LINEAR on 8-bit images - OpenCV's fixed-point bilinear (11-bit coefficients,
 * clamped borders), its 2 x 2 "area fast" average for an exact 2:1 decimation (the default upscale_factor), a copy at equal size;
 * synchronises `stream` when it had to build tables.
 * fw_face_paste_u8: frame[y1:y2, x1:x2] = orig * (1 - mask * s) + enhanced * mask * s in float32 with the reference's feather mask
 * (min(w, h) // 8 rows / columns scaled by i / feather), truncating cast; `enhanced` is (y2 - y1) x (x2 - x1) x 3; in place. */
int fw_resize_linear_u8(const uint8_t* src, int src_h, int src_w, int channels, uint8_t* dst, int dst_h, int dst_w, void* stream);
int fw_face_paste_u8(uint8_t* frame, int height, int width, int x1, int y1, int x2, int y2, const uint8_t* enhanced, double strength,
                     void* stream);

/* -------------------------------------------------------------------------------------------------
 * Restormer building blocks (the reference's DEFAULT TAP model)
 * replaces  `Restormer(dim=48, num_blocks=[4,6,6,8], num_refinement_blocks=4, heads=[1,2,4,8],
 *           ffn_expansion_factor=2.66, bias=False, LayerNorm_type='WithBias')` + `self._model(tensor)`
 *           (processors/tap_denoise.py:299-333, 458); architecture per SURVEY.md §A.4; host sequencing
 *           framewright_amd/restormer.py.  Device pointers; the residual stream is fp32 NHWC with a padded channel stride.
 * ------------------------------------------------------------------------------------------------- */

/* LayerNorm over the first `channels` of each pixel, (x - mean) / sqrt(var + eps) * weight + bias (bias may be NULL),
 * fp32 [pixels][x_stride] -> operand-typed [pixels][out_stride]; output channels [channels, zero_to) are zeroed. */
int fw_layernorm_nhwc(int dtype, const float* x, long x_stride, long pixels, int channels, const float* weight,
                      const float* bias, float eps, void* out, long out_stride, int zero_to, void* stream);

/* 1x1 convolution as an MFMA GEMM.  fw_pack_pointwise packs weight [cout][k] (fp32, host; k % 32 == 0) into fragments
 * (returns the uint16 count, dst may be NULL to query).  a: operand-typed or fp32 [pixels][a_stride]; outputs: typed
 * and/or fp32, 32*cout_tiles channels; with res_f32: out_f32 = res_f32 + (acc + bias) * chan_scale (same stride). */
size_t fw_pack_pointwise(int dtype, const float* weight, int cout, int k, void* dst);
int fw_pointwise_nhwc(int dtype, const void* a, int a_is_f32, long a_stride, long pixels, int k, const void* packed_weight,
                      const float* bias, int cout_tiles, void* out_typed, long out_stride, float* out_f32, long f32_stride,
                      const float* res_f32, const float* chan_scale, void* stream);

/* Depthwise 3x3, zero padding, no bias, weight fp32 [channels][9].  mode 0: plain; mode 1: the GDFN gate,
 * out[c] = gelu(dw(x)[c]) * dw(x)[channels/2 + c] for c < channels/2 (exact erf GELU). */
int fw_dwconv3x3_nhwc(int dtype, const void* x, long x_stride, int height, int width, int channels, const float* weight,
                      int mode, void* out, long out_stride, void* stream);

/* MDTA "transposed" attention.  qkv: operand-typed [pixels][stride], q at channel 0, k at k_off, v at v_off, heads*ch
 * channels each (ch = 48 or 96).  fw_attn_matrix: attn[head][c1][c2] = softmax_c2(normalize(q)_c1 . normalize(k)_c2 *
 * temperature[head]) with the dot products over all pixels (deterministic two-level reduction; workspace of
 * fw_attn_workspace_floats floats).  fw_attn_apply: out[p][head*ch + c1] = sum_c2 attn[head][c1][c2] * v[p][head*ch + c2]. */
size_t fw_attn_workspace_floats(int heads, int ch);
int fw_attn_matrix(int dtype, const void* qkv, long stride, long pixels, int k_off, int heads, int ch,
                   const float* temperature, float* workspace, float* attn, void* stream);
/* fw_attn_matrix on the matrix cores (what the engine runs): q and k are first rewritten pixel-major into `qk_scratch`
 * (fw_attn_qk_scratch_elems(pixels, heads, ch) operand-typed elements of device memory), then G = q^T k is an MFMA
 * contraction over the pixel axis; same partial-sum workspace, same deterministic reduction, same result up to fp32
 * summation order. */
size_t fw_attn_qk_scratch_elems(long pixels, int heads, int ch);
int fw_attn_matrix_mfma(int dtype, const void* qkv, long stride, long pixels, int k_off, int heads, int ch,
                        const float* temperature, float* workspace, void* qk_scratch, float* attn, void* stream);
int fw_attn_apply(int dtype, const void* qkv, long stride, long pixels, int v_off, int heads, int ch, const float* attn,
                  void* out, long out_stride, int zero_to, void* stream);
/* The attention matrices as one block-diagonal [k_pad x k_pad] weight in fw_pack_pointwise's fragment order (device buffer of
 * fw_pack_pointwise(dtype, NULL, k_pad, k_pad, NULL) uint16), so that attn @ v runs through fw_pointwise_nhwc on the matrix
 * cores — what the engine uses; fw_attn_apply is the plain form of the same product. */
int fw_attn_pack(int dtype, const float* attn, int heads, int ch, int k_pad, void* packed, void* stream);
/* project_out folded into the attention (restormer.py / reference Attention.forward: project_out(attn @ v)): packed =
 * (proj_weight [dim][dim] fp32) x blockdiag(attn) in fw_pack_pointwise's layout with cout_tiles 32-row tiles, so that
 * project_out(attn @ v) + x is one fw_pointwise_nhwc over v with the residual epilogue. */
int fw_attn_proj_pack(int dtype, const float* attn, const float* proj_weight, int heads, int ch, int k_pad, int cout_tiles, void* packed,
                      void* stream);

/* AESRGAN's AttentionBlock (reference src/framewright/processors/aesrgan_face.py:142-168, the in-tree net behind
 * AESRGANFaceRestorer): attention = softmax(q^T k) over ALL pixels, out = gamma * (v @ attention^T) + x.
 * fw_attn_softmax_rows: p[i][j] = softmax_j(sum_{c<d} q[i][c] k[j][c]) as an operand-typed [pixels][p_stride] matrix, columns
 * [pixels, p_stride) zeroed (p_stride = pixels padded to 32).  fw_pack_pointwise_transposed: fw_pack_pointwise's fragments
 * for the weight W[co][kk] = src[kk][co] from a typed device matrix (W = v^T), so that out = x + gamma * (p @ v) is
 * fw_pointwise_nhwc(a = p, k = p_stride, res_f32 = x, chan_scale = gamma). */
int fw_attn_softmax_rows(int dtype, const void* q, long q_stride, const void* k, long k_stride, long pixels, int d, void* p,
                         long p_stride, void* stream);
int fw_pack_pointwise_transposed(int dtype, const void* src, long src_stride, long k_valid, int cout, int k_pad, void* packed,
                                 void* stream);

/* torch.nn.PixelShuffle(2) (unshuffle = 0) / PixelUnshuffle(2) (unshuffle = 1) on fp32 NHWC; low_h x low_w is the
 * low-resolution size, `channels` the channel count at HIGH resolution; dst channels start at dst_coff. */
int fw_pixel_shuffle2_f32(const float* src, long src_stride, int low_h, int low_w, int channels, float* dst,
                          long dst_stride, int dst_coff, int unshuffle, void* stream);
/* dst[p][dst_coff + c] = src[p][c], c < channels (torch.cat along channels). */
int fw_copy_channels_f32(const float* src, long src_stride, long pixels, int channels, float* dst, long dst_stride,
                         int dst_coff, void* stream);
/* fp32 [pixels][channels] (channels % 32 == 0) -> operand-typed chunk-planar [channels/32][pixels][32]. */
int fw_f32_to_planar(int dtype, const float* x, long pixels, int channels, void* out, void* stream);
/* out = clip((rgb + input/255) * 255, 0, 255).astype(uint8), RGB -> BGR (tap_denoise.py:399-415: truncation); rgb is fp32
 * [H][padded_w][rgb_cstride] with R,G,B in channels 0..2. */
int fw_tap_post_u8(const uint8_t* in_bgr, const float* rgb, int height, int width, int padded_width, int rgb_cstride,
                   uint8_t* out_bgr, float* out_rgb_f32, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Classical motion-compensated temporal denoise (device pointers)
 * replaces  OpticalFlowEstimator.warp_frame (processors/temporal_denoise.py:440-477) and the accumulation of
 *           TemporalDenoiser._denoise_with_flow / _denoise_simple (:1521-1605).  The dense flow (cv2 Farneback / DIS) is
 *           estimated on the host and is not part of this path.
 * ------------------------------------------------------------------------------------------------- */

/* accumulated[p] += aligned[p] * w[p]; weight_sum[p] += w[p]  (float64, like the reference), with
 *   aligned = flow ? cv2.remap(frame, x +/- flow_x, y +/- flow_y, INTER_LINEAR, BORDER_REFLECT_101) : frame
 *   w       = weight_scale * (weight_map ? weight_map[p] : 1), halved where magnitude[p] > motion_threshold.
 * flow_x / flow_y / weight_map / magnitude: fp32 [H][W] or NULL; inverse != 0 subtracts the flow. */
int fw_flow_accumulate_u8(const uint8_t* frame_bgr, const float* flow_x, const float* flow_y, const float* weight_map,
                          double weight_scale, const float* magnitude, float motion_threshold, int inverse, int height,
                          int width, double* accumulated, double* weight_sum, void* stream);
/* out = (accumulated / max(weight_sum, 1e-6)).astype(uint8) */
int fw_flow_accumulate_finish_u8(const double* accumulated, const double* weight_sum, int height, int width,
                                 uint8_t* out_bgr, void* stream);

/* -------------------------------------------------------------------------------------------------
 * RIFE frame interpolation: IFNet v4.6 building blocks (device pointers, fp32 NHWC small-channel tensors)
 * replaces  the arithmetic inside the external binary the reference shells out to,
 *           `rife-ncnn-vulkan -m rife-v4.6` (processors/interpolation.py:628-650); architecture per SURVEY.md §A.5.
 *           The convolutions of the IFBlocks run through fw_conv3x3_nhwc_ex; the host sequencing is
 *           framewright_amd/rife.py (IFNetEngine).
 * ------------------------------------------------------------------------------------------------- */

/* uint8 BGR H x W x 3 -> fp32 RGB/255 [padded_h][padded_w][3], zero outside H x W. */
int fw_u8_to_rgb_f32(const uint8_t* in_bgr, int height, int width, int padded_height, int padded_width, float* out,
                     void* stream);

/* dst[y][x][dst_coff + c] = mul * F.interpolate(src, scale_factor, "bilinear", align_corners=False)[c][y][x]. */
int fw_resize_bilinear_f32(const float* src, int src_h, int src_w, int channels, float* dst, int dst_h, int dst_w,
                           int dst_cstride, int dst_coff, float scale_factor, float mul, void* stream);

/* x = cat(warp(img0, flow[:2]), warp(img1, flow[2:4]), timestep, mask) (8 ch) — or cat(img0, img1, timestep) (7 ch) when
 * flow == mask == NULL.  warp = grid_sample(bilinear, border, align_corners=True) with the flow in pixels. */
int fw_ifnet_build_x(const float* img0, const float* img1, const float* flow, const float* mask, int height, int width,
                     float timestep, float* x, void* stream);

/* pixel_unshuffle(2) + cast: src [h][w][src_cstride] (fp32 if src_is_f32, else operand-typed; first `channels` used) ->
 * dst operand-typed [h/2][w/2][dst_channels], channel c*4 + dy*2 + dx, zero above 4*channels.  Front end of the
 * stride-2 convolutions, which run as 3x3 convolutions on the unshuffled tensor. */
int fw_unshuffle2_cast(int dtype, const void* src, int src_is_f32, int height, int width, int channels, int src_cstride,
                       void* dst, int dst_channels, void* stream);

/* An IFBlock's whole input in one kernel, as the engine runs it: fw_ifnet_build_x, F.interpolate(x, 1/scale),
 * F.interpolate(flow, 1/scale) / scale, cat, pixel_unshuffle(2) and the cast of fw_unshuffle2_cast ->
 * dst operand-typed [height/scale/2][width/scale/2][dst_channels], channel c*4 + dy*2 + dx over the 7 channels (flow == mask == NULL)
 * or the 12 channels (8 of x, 4 of flow) of the block's input, zero above.  height and width multiples of 2*scale; dst_channels a
 * multiple of 8, at least 28 / 48 and at most 64; flow and dst 16-byte aligned. */
int fw_ifnet_stage_input(int dtype, const float* img0, const float* img1, const float* flow, const float* mask, int height, int width,
                         float timestep, int scale, void* dst, int dst_channels, void* stream);

/* [h][w][>=96] with channel ((c6*4 + qy*2 + qx)*4 + py*2 + px) -> [4h][4w][6]: ConvTranspose2d(4,2,1) evaluated as a
 * 3x3 conv with 4 output parities, followed by PixelShuffle(2). */
int fw_depth_to_space4_f32(const float* src, int height, int width, int src_cstride, float* dst, void* stream);

/* flow (+)= bilinear_up(tmp)[:4] * scale ; mask (+)= bilinear_up(tmp)[4]   (first != 0: assign). */
int fw_ifnet_accumulate(const float* tmp, int tmp_h, int tmp_w, int height, int width, float scale, float* flow, float* mask,
                        int first, void* stream);

/* fw_ifnet_accumulate reading the lastconv output in place, without the depth-to-space copy: tmp[Y][X][c6] =
 * t96[Y >> 2][X >> 2][pos*6 + c6] with pos = ((Y&1)*2 + (X&1))*4 + ((Y>>1)&1)*2 + ((X>>1)&1), t96 [feat_h][feat_w][src_cstride]
 * (the row order the engine gives lastconv's weights).  src_cstride even and >= 96, t96 8-byte and flow 16-byte aligned. */
int fw_ifnet_accumulate_d2s(const float* t96, int feat_h, int feat_w, int src_cstride, int height, int width, float scale, float* flow,
                            float* mask, int first, void* stream);

/* merged = warp(img0, flow[:2]) * sigmoid(mask) + warp(img1, flow[2:4]) * (1 - sigmoid(mask)), cropped to H x W;
 * out_bgr = round_half_even(clamp(merged, 0, 1) * 255) (BGR), out_rgb_f32 = merged (RGB); either may be NULL. */
int fw_ifnet_blend(const float* img0, const float* img1, const float* flow, const float* mask, int padded_height,
                   int padded_width, int height, int width, uint8_t* out_bgr, float* out_rgb_f32, void* stream);

/* Motion-blur reduction of the interpolator (reference interpolation.py:403-455: PIL ImageFilter.UnsharpMask(radius, percent,
 * threshold)) on a uint8 H x W x C device image, bit-exact with Pillow's libImaging (BoxBlur.c / UnsharpMask.c):
 *   blur = `passes` extended-box passes along x, then along y, every pass rounded to 8 bits:
 *          (ww * sum_{|k| <= box_radius} in[i+k] + fw_weight * (in[i-box_radius-1] + in[i+box_radius+1]) + 2^23) >> 24,
 *          edge-replicated (the host derives box_radius / ww / fw_weight from the Gaussian radius exactly as Pillow does);
 *   out  = |in - blur| > threshold ? clip8(in + (in - blur) * percent / 100) : in       (C integer division).
 * scratch_a / scratch_b: two H*W*C-byte device buffers.  `out` may alias `src`. */
int fw_unsharp_mask_u8(const uint8_t* src, int height, int width, int channels, int box_radius, unsigned ww, unsigned fw_weight,
                       int passes, int percent, int threshold, uint8_t* scratch_a, uint8_t* scratch_b, uint8_t* out, void* stream);

/* ---- AESRGAN (RRDB trunk + self-attention blocks) as one engine (csrc/aesrgan.hip) -------------------------------------------------
 * The reference's in-tree network of AESRGANFaceRestorer (processors/aesrgan_face.py:205-269, AttentionBlock :142-168): create,
 * hand over the tensors (BasicSR's names for the trunk / tail: conv_first, body.{i}.rdb{1,2,3}.conv{1..5}, conv_body, conv_up1
 * [, conv_up2], conv_hr, conv_last with .weight / .bias; attn.{i}.query|key|value.weight / .bias and attn.{i}.gamma for the block
 * behind RRDB i), finalize, then fw_aesrgan_forward_rgb on fp32 RGB crops in [0, 1] on the device: what AESRGAN.forward returns for
 * a 1 x 3 x H x W input (NHWC, un-clamped).  The attention matrix is pixels x pixels: crops of up to 512 x 512. */
typedef struct fw_aesrgan fw_aesrgan;
int fw_aesrgan_create(int device_id, int num_block, int scale, int num_attention, int dtype, fw_aesrgan** out);
int fw_aesrgan_set_tensor(fw_aesrgan* net, const char* key, const float* data, size_t numel);
int fw_aesrgan_finalize(fw_aesrgan* net);
int fw_aesrgan_forward_rgb(fw_aesrgan* net, const float* x_rgb, int height, int width, float* out_rgb, void* stream);
size_t fw_aesrgan_workspace_bytes(fw_aesrgan* net, int height, int width);
int fw_aesrgan_destroy(fw_aesrgan* net);

/* ---- SRVGGNetCompact as one engine (csrc/srvgg.hip) ---------------------------------------------------------------------------
 * The network of the Real-ESRGAN checkpoints realesr-animevideov3 (num_conv 16) / realesr-general-x4v3 (num_conv 32), which the
 * reference lists in its model table (processors/pytorch_realesrgan.py:119-128): create, hand over the tensors of the published
 * state dict (body.{2i}.weight [cout][cin][3][3], body.{2i}.bias, body.{2i+1}.weight = PReLU slopes [64]), finalize, then any number
 * of fw_srvgg_upscale_u8 calls (uint8 BGR H x W x 3 in, uint8 BGR sH x sW x 3 and / or RGB float out; FW_HOST or FW_DEVICE buffers).
 * One handle per GPU; calls on a handle are serialised by an internal mutex. */
typedef struct fw_srvgg fw_srvgg;
int fw_srvgg_create(int device_id, int num_feat, int num_conv, int upscale, int dtype, fw_srvgg** out);
int fw_srvgg_set_tensor(fw_srvgg* net, const char* key, const float* data, size_t numel);
int fw_srvgg_finalize(fw_srvgg* net);
int fw_srvgg_upscale_u8(fw_srvgg* net, const uint8_t* in_bgr, int in_loc, int height, int width, uint8_t* out_bgr, int out_loc,
                        float* out_rgb_f32, void* stream);
/* 16-bit frames (RealESRGANer.enhance: max_range 65535): uint16 BGR in, / 65535; uint16 BGR out, x 65535, round. */
int fw_srvgg_upscale_u16(fw_srvgg* net, const uint16_t* in_bgr, int in_loc, int height, int width, uint16_t* out_bgr, int out_loc,
                         float* out_rgb_f32, void* stream);
size_t fw_srvgg_workspace_bytes(const fw_srvgg* net, int height, int width);
double fw_srvgg_flops(const fw_srvgg* net, int height, int width);
int fw_srvgg_destroy(fw_srvgg* net);

/* ---- IFNet v4.6 (RIFE x2 interpolation) as one engine ------------------------------------------------------------------------
 * Replaces the reference's `rife-ncnn-vulkan` subprocess (reference src/framewright/processors/interpolation.py:628-650; model
 * directory `rife-v4.6`, :106-124).  Same life cycle as fw_rrdbnet / fw_nafnet: create, set every tensor of the Practical-RIFE
 * IFNet_HDv3 state dict (fp32, PyTorch layouts; keys `block{0..3}.conv0.{0,1}.0.{weight,bias}`,
 * `block{i}.convblock.{0..7}.conv.{weight,bias}`, `block{i}.convblock.{j}.beta`, `block{i}.lastconv.0.{weight,bias}`),
 * finalize (weight transforms + MFMA fragment packing on the host, upload), then any number of fw_ifnet_interp_u8 calls.
 * One handle per GPU; calls on a handle are serialised by an internal mutex.  FW_IFNET_GRAPH=1 in the environment replays a
 * captured hipGraph when a call repeats (frame size, timestep, buffer addresses). */
typedef struct fw_ifnet fw_ifnet;
int fw_ifnet_create(int device_id, int dtype, fw_ifnet** out);
int fw_ifnet_set_tensor(fw_ifnet* net, const char* key, const float* data, size_t numel);
int fw_ifnet_finalize(fw_ifnet* net);
/* frame0 / frame1: uint8 BGR H x W x 3 (both FW_HOST or both FW_DEVICE); timestep in (0, 1) (0.5 = the mid frame of a x2 pass);
 * out_bgr = round_half_even(clamp(merged, 0, 1) * 255) BGR and/or out_rgb_f32 = merged RGB float (device), either may be NULL.
 * Asynchronous on `stream` for device buffers; host outputs are complete on return. */
int fw_ifnet_interp_u8(fw_ifnet* net, const uint8_t* frame0, const uint8_t* frame1, int in_loc, int height, int width,
                       float timestep, uint8_t* out_bgr, int out_loc, float* out_rgb_f32, void* stream);
/* Flow [Hp][Wp][4] (pixels) and mask [Hp][Wp] (before the sigmoid) of the handle's last forward, Hp / Wp = height / width rounded up to
 * a multiple of 32, copied to device buffers on `stream` (either may be NULL).  FW_ERR_INVALID unless the last forward had this size. */
int fw_ifnet_last_flow(fw_ifnet* net, int height, int width, float* flow_out, float* mask_out, void* stream);
size_t fw_ifnet_workspace_bytes(const fw_ifnet* net, int height, int width);
double fw_ifnet_flops(const fw_ifnet* net, int height, int width);
int fw_ifnet_destroy(fw_ifnet* net);

/* ---- Restormer (the reference's default TAP model) as one engine ---------------------------------------------------------------
 * Replaces `basicsr.archs.restormer_arch.Restormer(inp_channels=3, out_channels=3, dim=48, num_blocks=[4,6,6,8],
 * num_refinement_blocks=4, heads=[1,2,4,8], ffn_expansion_factor=2.66, bias=False, LayerNorm_type='WithBias')` as constructed
 * and called at reference src/framewright/processors/tap_denoise.py:299-333 and :458, together with the pre / post-processing of
 * :373-415 (BGR uint8 in, `np.clip(x * 255, 0, 255).astype(uint8)` out - truncation).  Same life cycle as fw_nafnet: create,
 * set every tensor of the state dict (fp32, PyTorch layouts and key names), finalize, denoise.  One handle per GPU, calls
 * serialised by an internal mutex; the workspace is one arena sized by a dry run of the launch sequence. */
typedef struct fw_restormer fw_restormer;
int fw_restormer_create(int device_id, int dim, const int* num_blocks /* [4] */, int num_refinement_blocks,
                        const int* heads /* [4] */, double ffn_expansion_factor, int dtype, fw_restormer** out);
int fw_restormer_set_tensor(fw_restormer* net, const char* key, const float* data, size_t numel);
int fw_restormer_finalize(fw_restormer* net);
/* in_bgr / out_bgr: uint8 BGR H x W x 3, H and W multiples of 8; out_rgb_f32 (device, optional): the un-quantised RGB output. */
int fw_restormer_denoise_u8(fw_restormer* net, const uint8_t* in_bgr, int in_loc, int height, int width, uint8_t* out_bgr,
                            int out_loc, float* out_rgb_f32, void* stream);
size_t fw_restormer_workspace_bytes(fw_restormer* net, int height, int width);   /* 0 before finalize */
/* Single steps of a forward on the caller's device buffers, launched exactly as a forward launches them (tests, tools).
 * run_block: one transformer block, `key` as fw_restormer_set_tensor names blocks ("encoder_level1.0.", "latent.0.",
 *   "decoder_level1.0."), in place on the fp32 stream [height][width][pad32(c)] (lanes c .. pad32(c) - 1 hold zeros and keep them);
 *   attn_out (optional, device fp32 [heads][c / heads][c / heads]) receives the softmaxed attention matrix.
 * block_paths: which kernels that block dispatches to, as FW_REST_PATH_* bits.
 * run_step: what lies between two stages, on a source of height x width pixels.  "down1_2" / "down2_3" / "down3_4": conv3x3 +
 *   PixelUnshuffle, src [h][w][pad32(c)] -> dst [h/2][w/2][pad32(2c)] (even sides); "up4_3" / "up3_2" / "up2_1": conv3x3,
 *   PixelShuffle, the copy of skip [2h][2w][pad32(c/2)] behind it and, for the first two, the reduce_chan 1x1:
 *   src [h][w][pad32(c)] -> dst [2h][2w][pad32(c/2)] ("up2_1": [2h][2w][pad32(c)], the concatenation itself); "output": the last
 *   conv3x3 alone, src [h][w][96] -> dst [h][w][64] with the RGB residual in lanes 0..2 (fw_tap_post_u8 follows it).  Lanes of dst
 *   behind the real channels are written as zeros. */
#define FW_REST_PATH_FRONT_QKV 1   /* norm1 + qkv + qkv_dwconv in one kernel (c = 48, 96) */
#define FW_REST_PATH_FRONT_FFN 2   /* norm2 + project_in + dwconv + GELU gate in one kernel (c = 48, 96) */
#define FW_REST_PATH_QK_DIRECT 4   /* the qkv front writes q / k in the Gram kernel's operand layout */
#define FW_REST_PATH_MERGE_PROJ 8  /* project_out folded into the attention matrix: one residual GEMM */
#define FW_REST_PATH_GEMM16 16     /* qkv / project_in on the pipelined GEMM kernel (c = 192, 384) */
int fw_restormer_run_block(fw_restormer* net, const char* key, float* stream_f32, int height, int width, float* attn_out, void* stream);
int fw_restormer_block_paths(fw_restormer* net, const char* key, int* flags);
int fw_restormer_run_step(fw_restormer* net, const char* step, const float* src_f32, const float* skip_f32, int height, int width,
                          float* dst_f32, void* stream);
int fw_restormer_destroy(fw_restormer* net);

/* `TemporalDenoiser._preserve_edges` (reference src/framewright/processors/temporal_denoise.py:1636-1667): the Canny edges of
 * `original` (cv2.Canny(gray, t, 3t) on cv2.cvtColor(BGR2GRAY)), dilated 3x3 and blurred (GaussianBlur((5, 5), 0) of edges / 255)
 * into a float mask, blend `original` over `denoised`: out = (original * mask + denoised * (1 - mask)).astype(uint8).  uint8 BGR
 * H x W x 3 device buffers; `scratch`: fw_preserve_edges_scratch_bytes(height, width) bytes of device memory.  OpenCV's 8-bit
 * algorithms, restated (oracle/temporal_ref.py).  The hysteresis iterates to its fixed point: the call synchronises `stream`. */
size_t fw_preserve_edges_scratch_bytes(int height, int width);
int fw_preserve_edges_u8(const uint8_t* original, const uint8_t* denoised, int height, int width, double low_threshold,
                         double high_threshold, void* scratch, uint8_t* out, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Dense optical flow for the classical temporal denoise (csrc/optical_flow.hip): Farneback's algorithm as
 * cv2.calcOpticalFlowFarneback runs it (reference temporal_denoise.py:294-305: pyr_scale 0.5, levels 3, winsize 15, iterations 3,
 * poly_n 5, poly_sigma 1.1, flags 0), restated from OpenCV's published source (tests/farneback_ref.py is the contract; cv2 parity
 * unpinned).  Device pointers, caller-owned scratch, explicit stream; nothing is allocated and nothing synchronises.
 *   prev / next : uint8 H x W (channels 1, gray) or H x W x 3 (channels 3, BGR -> gray with cv2's 14-bit weights)
 *   flow_x / flow_y : fp32 [H][W], the displacement from `prev` to `next`
 *   scratch : fw_farneback_scratch_bytes(height, width, levels) bytes
 * Refused with FW_ERR_INVALID and a message, never ignored: poly_n != 5, flags != 0 (OPTFLOW_USE_INITIAL_FLOW,
 * OPTFLOW_FARNEBACK_GAUSSIAN), even or > 31 winsize, pyr_scale outside (0, 1), a pyramid level below scale 1/8 (its smoothing kernel
 * would exceed 19 taps), channels other than 1 or 3. */
size_t fw_farneback_scratch_bytes(int height, int width, int levels);
int fw_farneback_flow_u8(const uint8_t* prev, const uint8_t* next, int channels, int height, int width, double pyr_scale, int levels,
                         int winsize, int iterations, int poly_n, double poly_sigma, int flags, void* scratch, float* flow_x,
                         float* flow_y, void* stream);
/* magnitude = sqrt(flow_x^2 + flow_y^2) (numpy's float32 rounding; may be NULL) and the local variance of `_compute_flow_confidence`
 * (temporal_denoise.py:406-431): 5 x 5 box means (BORDER_REFLECT_101) of the components and of their squared deviations, summed. */
int fw_flow_stats_f32(const float* flow_x, const float* flow_y, int height, int width, float* magnitude, float* variance, void* stream);
/* confidence = 1 - clip(variance / (*variance_p95 + 1e-6), 0, 1) (temporal_denoise.py:435-436) and, with weight_map != NULL,
 * weight_map = confidence * (magnitude > *motion_threshold ? 0.5 : 1): the per-pixel weight of `_denoise_with_flow` (:1560-1564) for
 * fw_flow_accumulate_u8(weight_map, magnitude = NULL).  Both scalars are read from DEVICE memory, so the caller never waits for an
 * order statistic.  confidence or weight_map may be NULL (not both). */
int fw_flow_confidence_f32(const float* variance, const float* variance_p95, const float* magnitude, const float* motion_threshold,
                           int height, int width, float* confidence, float* weight_map, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Non-local-means spatial denoise for the classical temporal denoise (csrc/nlmeans.hip): the reference's `_apply_spatial_denoise`
 * (temporal_denoise.py:1611-1634), cv2.fastNlMeansDenoisingColored(frame, None, h, h, 7, 21) with h = int(3 + strength * 7).
 * OpenCV's 8-bit algorithm restated (tests/nlmeans_ref.py is the contract, held bit for bit; cv2 parity unpinned).  Device
 * pointers, caller-owned scratch, explicit stream; both device entries only launch kernels and never wait for the device, except
 * that the first call with a given (device, h, channels, windows) uploads its weight table (one allocation, one blocking copy; the
 * colour tables likewise, once per device).
 *   fw_nlmeans_u8 : the core on a uint8 H x W x channels plane (channels 1, 2 or 3, pixels interleaved; the weights use
 *     h^2 * channels and the patch distances sum over the channels).  src != dst.  `scratch` is not touched (may be NULL): the
 *     whole neighbourhood is kept on chip.
 *   fw_nlmeans_colored_u8 : 8-bit linear BGR -> Lab (COLOR_LBGR2Lab: no gamma, D65), the core on L with h and on the interleaved
 *     ab plane with h_color, Lab -> BGR.  scratch : fw_nlmeans_scratch_bytes(height, width, search_window) bytes.
 * Refused with FW_ERR_INVALID and a message, nothing launched: channels outside 1 .. 3, h <= 0, a template window other than 3, 5
 * or 7, a search window that is not odd or outside 3 .. 41 (even sizes are REJECTED, where cv2 would force them odd), a side of
 * 1 px (reflect-101 needs 2), NULL pointers, and an h so large that its weight table does not fit the kernel's LDS next to the
 * tile (several thousand non-zero entries; h = 10 has 528 to 1584).
 * fw_nlmeans_scratch_bytes returns 0 on invalid arguments. */
size_t fw_nlmeans_scratch_bytes(int height, int width, int search_window);
int fw_nlmeans_u8(const uint8_t* src, int channels, int height, int width, double h, int template_window, int search_window,
                  void* scratch, uint8_t* dst, void* stream);
int fw_nlmeans_colored_u8(const uint8_t* src_bgr, int height, int width, double h, double h_color, int template_window,
                          int search_window, void* scratch, uint8_t* dst_bgr, void* stream);
/* HOST functions (no GPU needed).  The fixed-point weight table the core's launcher uploads: t[i] = round(mult * exp(-(i m) /
 * (h h channels))), mult = INT32_MAX / (search^2 * 255), m = 2^shift / template^2, zero below 0.001 mult - written truncated behind
 * its last non-zero entry; returns that length (out = NULL: the length only), 0 on invalid arguments (any odd windows are accepted
 * here) or when `capacity` is too small. */
int fw_nlmeans_weight_table(double h, int channels, int template_window, int search_window, int32_t* out, int capacity);
/* The integer tables of the two colour transforms, built once in float64, for comparison with the contract's: which = 0 the
 * 65281-entry f(t) table of the forward transform (16 fractional bits), 1 its 3 x 3 matrix over (B, G, R) (20 bits), 2 the four
 * 256-entry tables of the inverse (fy, Y, a / 500, b / 200), 3 its 3 x 3 matrix (rows B, G, R) and the three constants of the
 * piecewise cube.  Same return convention as fw_nlmeans_weight_table. */
int fw_nlmeans_lab_tables(int which, int32_t* out, int capacity);

/* -------------------------------------------------------------------------------------------------
 * Clip analysis and the temporal-consistency pass of the classical temporal denoise (csrc/temporal_chain.hip).  Device pointers,
 * explicit stream; the three entries only enqueue work and never wait for the device.  tests/temporal_chain_ref.py is the contract
 * (held exactly); cv2 parity unpinned.
 *   fw_frame_stats_u8 : for each of `count` contiguous uint8 BGR H x W x 3 frames, hist[f][256] = the histogram of gray =
 *     (1868 B + 9617 G + 4899 R + 8192) >> 14 (cv2.cvtColor BGR2GRAY) and lap_sums[f] = {sum lap, sum lap^2} as exact integers,
 *     lap = cv2.Laplacian(gray, CV_64F) with ksize 1 (taps [[0,1,0],[1,-4,1],[0,1,0]], BORDER_REFLECT_101): what the reference's
 *     `analyze` (temporal_denoise.py:1110-1300) and `_estimate_noise_reduction` (:1734-1788) need of a frame.  Both outputs are
 *     zeroed on `stream` by the call.  count <= 65535.
 *   fw_flow_accumulate_affine_u8 : fw_flow_accumulate_u8's remap and accumulate with the per-pixel float64 weight
 *     w = w_const + w_conf * (double)confidence[p] (product rounded, then the sum), the neighbour step of
 *     `TemporalConsistencyFilter._apply_flow_guided_filter` (:975-1005).  confidence = NULL: the scalar weight w_const;
 *     flow_x = flow_y = NULL: the frame as it is.
 *   fw_add_weighted_u8 : cv2.addWeighted(a, alpha, b, beta, 0) on uint8 (:1016-1020, :1055-1059): alpha and beta rounded once to
 *     float32, t = fl32(fl32(a * alpha) + fl32(b * beta)), rounded half to even, saturated to 0 .. 255.  `out` may alias `a` or `b`.
 *     (fw_strength_blend_u8 truncates: it is numpy's astype, not this.) */
int fw_frame_stats_u8(const uint8_t* frames_bgr, int count, int height, int width, uint32_t* hist /* [count][256] */,
                      int64_t* lap_sums /* [count][2] */, void* stream);
int fw_flow_accumulate_affine_u8(const uint8_t* frame_bgr, const float* flow_x, const float* flow_y, const float* confidence,
                                 double w_const, double w_conf, int inverse, int height, int width, double* accumulated,
                                 double* weight_sum, void* stream);
int fw_add_weighted_u8(const uint8_t* a, double alpha, const uint8_t* b, double beta, size_t nbytes, uint8_t* out, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Flicker reduction of the classical temporal denoise (csrc/flicker.hip): the reference's Python path,
 * `FlickerReducer._apply_python_deflicker` (temporal_denoise.py:764-836), brightness normalisation in 8-bit gamma Lab
 * (cv2.COLOR_BGR2LAB / COLOR_LAB2BGR).  The ffmpeg `deflicker` filter, the reference's first choice, is not built.  The sRGB and CIE
 * Lab formulas restated in fixed point (tests/flicker_ref.py is the contract, held bit for bit; cv2 parity unpinned).  Device
 * pointers, explicit stream; the four device entries only enqueue work and never wait for the device, except that the first call on
 * a device uploads the tables (an allocation and a blocking copy).
 *   fw_bgr_to_lab_u8 / fw_lab_to_bgr_u8 : the two transforms on n_pixels interleaved 3-byte pixels (sRGB decode, D65, L * 255 / 100,
 *     a + 128, b + 128).  dst may alias src.
 *   fw_lab_l_sums_u8 : l_sums[f] = the sum of L over frame f of `count` contiguous uint8 BGR H x W x 3 frames, an exact integer
 *     (64 bits: an 8K frame exceeds 2^32).  The output is zeroed on `stream` by the call.
 *   fw_deflicker_lab_u8 : per frame f, BGR -> Lab, L = l_luts[f][L], Lab -> BGR in one pass: one read and one write of the frames,
 *     no Lab plane in memory.  l_luts is count x 256 bytes of DEVICE memory.  dst_bgr may alias frames_bgr.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, count outside 1 .. 65535, non-positive sizes, more
 * than 2^30 pixels per frame. */
int fw_bgr_to_lab_u8(const uint8_t* src_bgr, int64_t n_pixels, uint8_t* dst_lab, void* stream);
int fw_lab_to_bgr_u8(const uint8_t* src_lab, int64_t n_pixels, uint8_t* dst_bgr, void* stream);
int fw_lab_l_sums_u8(const uint8_t* frames_bgr, int count, int height, int width, int64_t* l_sums /* [count] */, void* stream);
int fw_deflicker_lab_u8(const uint8_t* frames_bgr, int count, int height, int width, const uint8_t* l_luts /* [count][256] */,
                        uint8_t* dst_bgr, void* stream);
/* HOST function (no GPU needed).  The tables the gamma transforms add to fw_nlmeans_lab_tables', built once in float64, for
 * comparison with the contract's: which = 0 the 256-entry sRGB decode to the 0 .. 65280 scale, 1 the 65281-entry sRGB encode of
 * that scale to 0 .. 255, 2 the same map as 255 thresholds (the first index whose entry exceeds k), which is what the kernels
 * search.  Same return convention as fw_nlmeans_weight_table. */
int fw_gamma_lab_tables(int which, int32_t* out, int capacity);

/* -------------------------------------------------------------------------------------------------
 * Scene-cut detection of the frame interpolator (csrc/scene_cuts.hip): the two tests of the reference's
 * `FrameInterpolator.detect_scene_change` (interpolation.py:267-366) on uint8 H x W x 3 frames in DEVICE memory (any channel order:
 * both tests are symmetric in it).  Explicit stream; the entries only enqueue work and never wait for the device.
 * tests/scene_cut_ref.py is the contract; skimage parity unpinned.
 *   fw_scene_ssim_u8 : ssim[p] = skimage.metrics.structural_similarity (defaults, data_range 255: 7 x 7 uniform window, sample
 *     covariance, K1 0.01, K2 0.03, 3 pixels cropped before the mean) of gray = (c0 + c1 + c2) / 3 of the frames at
 *     frames_a + p * frame_stride_bytes and frames_b + p * frame_stride_bytes, p < pairs, in one launch.  A contiguous clip of n frames
 *     is the n - 1 pairs (clip, clip + H W 3) with stride H W 3; two unrelated frames are pairs = 1 (the stride is not read).  Frames
 *     need no alignment.  The window sums and central moments are exact integers; each map value is seven correctly rounded float64
 *     operations; the sum runs in a fixed order without floating-point atomics, so ssim[p] is the same bits in every run, alone or
 *     in a batch, contiguous or not, within (N + 8) 2^-53 of the contract's exactly rounded sum, N = (H - 6)(W - 6).
 *     `workspace`: fw_scene_ssim_workspace_bytes(pairs, H, W) bytes of device memory, written by the call (no need to clear it).
 *   fw_scene_ssim_workspace_bytes : that size; 0 for arguments fw_scene_ssim_u8 refuses.
 *   fw_hist64x3_u8 : hist[f][c][b] = the number of bytes of channel c of frame f with value >> 2 == b, for `count` contiguous
 *     frames (np.histogram(bins=64, range=(0, 256)) on uint8).  The output is zeroed on `stream` by the call.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, pairs / count outside 1 .. 65535, height or width
 * below 7 (SSIM: the window exceeds the image, the caller falls back to the histograms) or below 1 (histograms), more than 2^30
 * pixels per frame, a negative stride, a zero stride with more than one pair. */
size_t fw_scene_ssim_workspace_bytes(int pairs, int height, int width);
int fw_scene_ssim_u8(const uint8_t* frames_a, const uint8_t* frames_b, int64_t frame_stride_bytes, int pairs, int height, int width,
                     double* ssim /* [pairs] */, void* workspace, void* stream);
int fw_hist64x3_u8(const uint8_t* frames, int count, int height, int width, uint32_t* hist /* [count][3][64] */, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Frame deduplication (csrc/dedup_hash.hip): the two frame hashes of the reference's `FrameDeduplicator`
 * (processors/deduplication.py:106-164) on uint8 BGR H x W x 3 frames in DEVICE memory.  Both are Pillow thumbnails - `convert('L')`
 * is L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, `resize(..., LANCZOS)` a horizontal then a vertical pass of integer taps with
 * 22 fractional bits, each pass rounding to uint8, a pass left out when its size does not change - so the results are Pillow's bytes.
 * tests/dedup_ref.py is the contract, held byte for byte against Pillow itself on the CPU; the dHash bit order is restated from
 * imagehash's definition (imagehash parity unpinned).  Explicit stream; the device entries only enqueue work and never wait for the
 * device, except that the first call for a pair of sizes on a device uploads its tap table (an allocation and a blocking copy).
 *   fw_pil_lanczos_taps : HOST function (no GPU needed).  The table of one pass in_size -> out_size: for output index i the window
 *     starts at xmin[i] and has count[i] taps, taps[i * ksize + k], zero behind the window.  Returns ksize (all three pointers NULL:
 *     ksize only); 0 for sizes outside 1 .. 65536, a NULL among the pointers, or capacity < out_size * ksize.
 *   fw_pil_thumb_u8 : thumbs[f] (out_h x out_w bytes) of the n frames at frames_bgr + f * frame_stride_bytes, in one call.
 *     gray_first = 1: convert('L').resize((out_w, out_h), LANCZOS), the dHash thumbnail; gray_first = 0: resize, then convert('L'),
 *     the pixel-hash thumbnail.  Frames need no alignment; a contiguous clip has stride H W 3, one frame is n = 1 (the stride is not
 *     read).  No atomics and no floating point on the device: a thumbnail is the same bytes in every run, alone or in a batch.
 *     `workspace`: fw_pil_thumb_workspace_bytes(...) bytes of device memory, written by the call (no need to clear it).
 *   fw_pil_thumb_workspace_bytes : that size; 0 for arguments fw_pil_thumb_u8 refuses.
 *   fw_dhash_pack_u8 : bits[f] = the hash_size^2 comparisons px[r][c + 1] > px[r][c] of thumbnail f ((hash_size + 1) wide, hash_size
 *     high), row-major, as one big-endian integer in ceil(hash_size^2 / 8) bytes (the first bit most significant, zero bits in front).
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, n outside 1 .. 65535, non-positive sizes, height or
 * width above 16384, out_w or out_h above 65, a negative stride, a zero stride with more than one frame, hash_size outside 2 .. 64. */
int fw_pil_lanczos_taps(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* taps, int capacity);
size_t fw_pil_thumb_workspace_bytes(int n, int height, int width, int out_w, int out_h, int gray_first);
int fw_pil_thumb_u8(const uint8_t* frames_bgr, int64_t frame_stride_bytes, int n, int height, int width, int out_w, int out_h,
                    int gray_first, uint8_t* thumbs /* [n][out_h][out_w] */, void* workspace, void* stream);
int fw_dhash_pack_u8(const uint8_t* thumbs, int n, int hash_size, uint8_t* bits, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Colour grade (csrc/color_lut.hip): the reference's `LUTManager.apply_to_image_fast` (integration/lut.py; core/restorer.py step 7c,
 * the seasonal grade) on three-channel frames of H x W pixels without row padding in DEVICE memory.  Per sample v (maxv = 255 or
 * 65535), every operation rounded on its own: in float32 x = v / maxv (IEEE division), s = x * (size - 1), lo = floor(s),
 * hi = min(lo + 1, size - 1); then in float64, as NumPy promotes the reference's own lines, f = s - lo; eight corners of the float32
 * table; four lerps along r, two along g, one along b, each a * (1 - f) + b * f as two products and a sum; clip to [0, 1], * maxv,
 * truncate.  The results are the reference's bytes;
 * tests/color_lut_ref.py is the contract, held byte for byte against the reference's own function on the CPU.  A LUT's domain is
 * not applied (`apply_to_image_fast` ignores it).  Explicit stream; the calls only enqueue one launch and never wait or allocate.
 *   fw_lut3d_apply_u8 : dst[f] = grade(src[f]) for the n frames at src + f * src_stride_bytes -> dst + f * dst_stride_bytes.
 *     lut_f32: size^3 x 3 floats in device memory, order [r][g][b][rgb]; tables up to 17^3 are held in LDS, larger ones read through
 *     L2.  bgr != 0: byte 0 of a pixel is blue (OpenCV order), else red.  Frames need no alignment; a contiguous clip has stride
 *     H W 3, one frame is n = 1 (the strides are not read).  dst == src with equal strides grades in place; any other overlap of
 *     source and destination is undefined.  Nothing outside the n frames is read or written.  No atomics: a frame's result is the
 *     same bytes in every run, alone or in a batch, wherever it lies.
 *   fw_lut3d_apply_u16 : the same for 16-bit samples (strides still in bytes; pointers and strides even).
 *   fw_table3_apply_u8 : dst sample = tables[c][src sample] for stored channel c = 0, 1, 2 - a 1D LUT on 8-bit frames, its three
 *     256-byte tables (device memory) built by the host (color_grade.py).
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, n outside 1 .. 65535, height or width outside
 * 1 .. 16384, size outside 2 .. 65, a negative stride, a zero stride with more than one frame, odd 16-bit addresses or strides. */
int fw_lut3d_apply_u8(const uint8_t* src, int64_t src_stride_bytes, int n, int height, int width, const float* lut_f32, int size, int bgr,
                      uint8_t* dst, int64_t dst_stride_bytes, void* stream);
int fw_lut3d_apply_u16(const uint16_t* src, int64_t src_stride_bytes, int n, int height, int width, const float* lut_f32, int size, int bgr,
                       uint16_t* dst, int64_t dst_stride_bytes, void* stream);
int fw_table3_apply_u8(const uint8_t* src, int64_t src_stride_bytes, int n, int height, int width, const uint8_t* tables /* [3][256] */,
                       uint8_t* dst, int64_t dst_stride_bytes, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Deinterlacing and interlace analysis (csrc/deinterlace.hip): the frame path of the reference's `Deinterlacer`
 * (processors/format/interlace.py) on uint8 frames in DEVICE memory, gray (H x W) or BGR (H x W x 3), without row padding.  Every
 * output is an integer function of the input bytes; tests/deinterlace_ref.py is the contract, held byte for byte against the
 * reference's own functions on the CPU.  Explicit stream; the calls enqueue and never wait or allocate.
 *   fw_deinterlace_u8 : one frame of `rows` rows of `row_bytes` = W * C bytes.  parity 1 (top field first) rebuilds odd rows, 0 even
 *     rows; every other row is copied.
 *       FW_DEINTERLACE_YADIF  1 <= y <= rows-2: dst[y] = (cur[y-1] + cur[y+1]) >> 1; prev and next are not read (may be NULL)
 *       FW_DEINTERLACE_BWDIF  2 <= y <= rows-3: num = 3 * (9 * (cur[y-1] + cur[y+1]) - (cur[y-2] + cur[y+2])) + 4 * (prev[y] + next[y]),
 *                             dst[y] = clamp(num, 0, 255 * 64) >> 6; at the ends of a clip prev or next is cur itself
 *       FW_DEINTERLACE_BOB    dst = cv2.resize(cur[parity::2], (W, rows)) with the 8-bit INTER_LINEAR arithmetic of
 *                             fw_resize_linear_u8, the field read in place; prev and next are not read
 *     Frames may start at any byte; 16-byte accesses are used when every pointer and row_bytes are multiples of 16, 4-byte ones
 *     when row_bytes is a multiple of 4 and all pointers agree modulo 4.  Nothing outside the frames is read or written.
 *   fw_deinterlace_batch_u8 : n frames; `frames` is a HOST table of n x 4 device pointers {cur, prev, next, dst}; one launch per
 *     32 frames.
 *   fw_interlace_stats_u8 : `frames` is a HOST table of n device pointers; stats (device, int64 [n][4]) = {n_comb, s_field, s_odd,
 *     s_even} of each frame's gray image g (channels 3: (1868 B + 9617 G + 4899 R + 8192) >> 14; channels 1: the bytes), R = height / 2:
 *     n_comb = #{r < R : sum_x |g[2r+1] - g[2r]| > 30 * width}, s_field = sum_{r < R} |g[2r+1] - g[2r]|,
 *     s_odd = sum_{r < R-1} |g[2r+3] - g[2r+1]|, s_even = sum_{r < R-1} |g[2r+2] - g[2r]|.  Exact integers, equal in every run.
 *   fw_frame_absdiff_sum_u8 : sums (device, int64 [n]) = sum |g(a[i]) - g(b[i])| over the frame; a and b are HOST tables.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers or tables, n < 1, rows / height / width outside
 * 1 .. 16384, row_bytes outside 1 .. 65536, an unknown mode, a parity other than 0 or 1, BOB with rows < 2, channels other than 1
 * or 3, a dst that overlaps cur (or, for BWDIF, prev or next) of any frame of the call: rebuilt rows are read as neighbours. */
#define FW_DEINTERLACE_YADIF 0
#define FW_DEINTERLACE_BWDIF 1
#define FW_DEINTERLACE_BOB 2
int fw_deinterlace_u8(const uint8_t* cur, const uint8_t* prev, const uint8_t* next, uint8_t* dst, int rows, int64_t row_bytes, int mode,
                      int parity, void* stream);
int fw_deinterlace_batch_u8(const void* const* frames /* host [n][4] */, int n, int rows, int64_t row_bytes, int mode, int parity,
                            void* stream);
int fw_interlace_stats_u8(const void* const* frames /* host [n] */, int n, int height, int width, int channels,
                          int64_t* stats /* device [n][4] */, void* stream);
int fw_frame_absdiff_sum_u8(const void* const* a /* host [n] */, const void* const* b /* host [n] */, int n, int height, int width,
                            int channels, int64_t* sums /* device [n] */, void* stream);

/* -------------------------------------------------------------------------------------------------
 * VHS artifact repair and analysis (csrc/vhs.hip): the frame path of the reference's `VHSProcessor` (processors/format/vhs.py) on
 * uint8 frames in DEVICE memory, gray (H x W) or BGR (H x W x 3), without row padding.  tests/vhs_ref.py is the contract, held byte
 * for byte against the reference's own functions on the CPU.  The device forms exact integer statistics and rewrites frames; the
 * decisions between the two are the caller's (vhs.py: the reference's NumPy steps on a few values per frame).  Explicit stream; the
 * calls enqueue and never wait or allocate.  Gray g is the bytes (channels 1) or (1868 B + 9617 G + 4899 R + 8192) >> 14.  A blend
 * fa * a + fb * b is float32: two rounded products, a rounded sum, never an FMA; the cast to uint8 truncates.  `frames`, `src`, `dst`,
 * `sources`, `results` are HOST tables of device pointers; tables of rows, boxes and samples are in DEVICE memory, and the kernels skip
 * every entry of them that does not lie inside a frame, so nothing outside a frame is read or written whatever they hold.
 *   fw_vhs_gray_stats_u8 : any of (NULL = not wanted) row_sums int64 [n][H] = sum_x |g[y][x+1] - g[y][x]|; bottom uint8 [n][30][W] = the
 *     last 30 rows of g; runs int32 [run_capacity][4] = {frame, x, y, length} of every maximal run of g > 250 or of g < 5 in a row with
 *     length >= min_length, in no particular order, and *run_count = how many there are (also when that is more than the capacity:
 *     the caller then calls again with a larger list).  One launch per 32 frames.
 *   fw_vhs_blend_rows_u8 : for each of m table rows {frame, y, y1, y2} / {fa, fb}: dst[frame][y] = fa * ((src[y1] + src[y2]) / 2) + fb *
 *     src[y] byte by byte.  Other rows of dst are not written (the caller copies the frame first).  n <= 32.
 *   fw_vhs_rainbow_u8 : BGR; r = 0.5 c + 0.125 (the four diagonal neighbours) inside, r = c on the border rows and columns, formed as
 *     an integer sum of eighths (exact), then dst = clamp(fa * r + fb * c, 0, 255) for EVERY byte, the borders included.  n <= 32.
 *   fw_vhs_box_gray_sums_u8 : tasks int32 [m][5] = {frame, x, y, w, h}; sums[e] = sum of g over the box, -1 for an entry not inside a
 *     frame.  n <= 64.
 *   fw_vhs_dropout_repair_u8 : boxes int32 [m][8] = {mode, result frame, source frame, x, y, w, h, 0}, rewritten in place in
 *     results[.]: mode 0 res = float32(s) * src + float32(1 - s) * res over the box; mode 1 (needs x > 0 and x + w < W), per column xi:
 *     t = (xi - x + 1) / (w + 1), res = s * ((1 - t) * res[x - 1] + t * res[x + w]) + double(float32(1 - s) * float32(res)) in float64.
 *     The boxes of one call that share a result frame must be disjoint, the two flank columns of a mode 1 box included (the caller
 *     splits a frame's list into such groups and calls once per group, in order).  n_sources <= 64, n_results <= 32.
 *   fw_vhs_edge_counts_u8 : BGR; counts int32 [n][H] = #{x < W - 1 : |Y[x+1] - Y[x]| > 30} with Y = float32(0.299 R + 0.587 G + 0.114 B),
 *     the sum in float64 from left to right.
 *   fw_vhs_chroma_samples_u8 : samples int32 [m][3] = {frame, row, k}: x = the k-th such edge of the row; offsets int32 [m][2] = for R and
 *     for B |x0 + argmax - x| of the channel's |step| over [x0, x1) = [max(0, x - 5), min(W - 2, x + 5)), first maximum, -1 when the
 *     window is empty or the maximum is not above 20, -2 when the entry names no edge.  n <= 64, m <= 6400.
 *   fw_vhs_chroma_shift_u8 : BGR; dst.R[x] = src.R[x - shift] for x >= shift, dst.B[x] = src.B[x + shift] for x < W - shift, every other
 *     byte copied; shifts is a HOST table of n values in 0 .. 2.  n <= 32.
 *   fw_vhs_column_sums_u8 : BGR; sums int64 [W - 1] = sum_y | |R - B|[y][x+1] - |R - B|[y][x] |.
 *   fw_vhs_jitter_shifts_u8 : shifts int32 [(H + 2) / 5]: for rows y = 1, 6, 11 ... the first maximum over j of the exact int32
 *     correlation sum_n g[y][n + j - W / 2] * g[y - 1][n], less W / 2 (numpy.correlate(..., "same") on integers).
 *   fw_vhs_saturation_f64 : BGR; saturation float64 [H][W] = max > 0 ? (max - min) / (max + 1e-6) : 0.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers or tables, frame counts outside the limits above, height
 * or width outside 1 .. 16384, channels other than 1 or 3, table lengths outside 1 .. 2^24, nothing asked of fw_vhs_gray_stats_u8,
 * bottom rows of a frame of fewer than 30 rows, a strength outside (0, 1], a shift outside 0 .. 2, fewer than two columns (column
 * sums) or three rows (jitter), a dst or result that overlaps a source frame of the call or another dst of the call. */
int fw_vhs_gray_stats_u8(const void* const* frames /* host [n] */, int n, int height, int width, int channels, int min_length,
                         int64_t* row_sums, uint8_t* bottom, int32_t* runs, int run_capacity, int32_t* run_count, void* stream);
int fw_vhs_blend_rows_u8(const void* const* src /* host [n] */, void* const* dst /* host [n] */, int n, int rows, int64_t row_bytes,
                         const int32_t* spec_rows /* device [m][4] */, const float* spec_factors /* device [m][2] */, int m, void* stream);
int fw_vhs_rainbow_u8(const void* const* src /* host [n] */, void* const* dst /* host [n] */, int n, int height, int width, float fa, float fb,
                      void* stream);
int fw_vhs_box_gray_sums_u8(const void* const* frames /* host [n] */, int n, int height, int width, int channels,
                            const int32_t* tasks /* device [m][5] */, int m, int64_t* sums /* device [m] */, void* stream);
int fw_vhs_dropout_repair_u8(const void* const* sources /* host */, int n_sources, void* const* results /* host */, int n_results, int height,
                             int width, int channels, const int32_t* boxes /* device [m][8] */, int m, double strength, void* stream);
int fw_vhs_edge_counts_u8(const void* const* frames /* host [n] */, int n, int height, int width, int32_t* counts /* device [n][H] */,
                          void* stream);
int fw_vhs_chroma_samples_u8(const void* const* frames /* host [n] */, int n, int height, int width, const int32_t* samples /* device [m][3] */,
                             int m, int32_t* offsets /* device [m][2] */, void* stream);
int fw_vhs_chroma_shift_u8(const void* const* src /* host [n] */, void* const* dst /* host [n] */, const int32_t* shifts /* host [n] */, int n,
                           int height, int width, void* stream);
int fw_vhs_column_sums_u8(const uint8_t* frame, int height, int width, int64_t* sums /* device [W - 1] */, void* stream);
int fw_vhs_jitter_shifts_u8(const uint8_t* frame, int height, int width, int channels, int32_t* shifts, void* stream);
int fw_vhs_saturation_f64(const uint8_t* frame, int height, int width, double* saturation /* device [H][W] */, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Letterbox / pillarbox statistics, crop and aspect conversion (csrc/aspect.hip): the frame path of the reference's `AspectHandler`
 * (processors/format/aspect.py) on uint8 frames in DEVICE memory, gray (H x W) or BGR (H x W x 3), without row padding.
 * tests/aspect_ref.py is the contract, held byte for byte against the reference's own methods on the CPU.  Integers only.  Explicit
 * stream; the calls enqueue and never wait or allocate.  `frames`, `src`, `dst`, `background`, `strips` are HOST tables of device
 * pointers; 1 .. 32 frames a call.  Gray g is the bytes (channels 1) or (1868 B + 9617 G + 4899 R + 8192) >> 14.
 *   fw_aspect_bar_sums_u8 : row_sums uint32 [n][H] = sum_x g[y][x], column_sums uint32 [n][W] = sum_y g[y][x], exact (aspect.py:636-680,
 *     `_detect_horizontal_bars` / `_detect_vertical_bars`: np.mean(line) > threshold is sum > threshold * length; the walk over the
 *     sums is the caller's).  The sums are zeroed on the stream first and accumulated with integer atomics: the same in every run.
 *   fw_aspect_crop_u8 : dst[i] = src[i][y : y + crop_height, x : x + crop_width] contiguous (aspect.py:458-470 `crop_letterbox`,
 *     :708-728 `_crop_to_ratio`); flip 1 reverses the columns of the result, flip 2 its rows (cv2.flip of a strip, :851 - :885).
 *   fw_aspect_pad_u8 : every byte of dst[i] (out_height x out_width): src[i] at (x_offset, y_offset) (aspect.py:730-781
 *     `_pad_to_ratio`), outside it mode 0 the three bytes of `color` (HOST, taken in B, G, R order as given; gray: color[0]); mode 2
 *     the byte of background[i], a frame of the output size (:811-834 `_apply_blur_fill`); mode 1 the mirror fill (:836-892
 *     `_apply_mirror_fill`): beside the source, over its span only, a bar no wider than the source is the source's edge strip reversed;
 *     a wider bar takes the bytes of strips[4 i + k] (k = 0 left, 1 right, 2 top, 3 bottom; contiguous, of the bar's size; the caller
 *     makes it from the whole source with fw_aspect_crop_u8 reversed and fw_resize_linear_u8); the corners take `color`.
 *   fw_aspect_gauss99_u8 : cv2.GaussianBlur(src, (99, 99), 0) on uint8 (:822) in fixed point: weights is a HOST table of 99 values in 8
 *     fractional bits that sum to 256 (getGaussianKernel(99, 0), sigma 15.2, quantised by the caller); rows: scratch uint16 [H][W][C] =
 *     sum src * w; columns: dst = (sum scratch * w + 2^15) >> 16; BORDER_REFLECT_101, reflected as often as it takes, index 0 for a
 *     side of one pixel.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers or tables, n outside 1 .. 32, height or width (of the
 * frame or of the output) outside 1 .. 16384, channels other than 1 or 3, a crop that is empty or not inside the frame, a flip or a
 * mode out of range, a source that does not lie inside the output, a missing strip of a bar wider than the source, weights that do
 * not sum to 256, a dst (or scratch) that overlaps anything the call reads or another dst of the call. */
int fw_aspect_bar_sums_u8(const void* const* frames /* host [n] */, int n, int height, int width, int channels,
                          uint32_t* row_sums /* device [n][H] */, uint32_t* column_sums /* device [n][W] */, void* stream);
int fw_aspect_crop_u8(const void* const* src /* host [n] */, void* const* dst /* host [n] */, int n, int height, int width, int channels,
                      int x, int y, int crop_width, int crop_height, int flip, void* stream);
int fw_aspect_pad_u8(const void* const* src /* host [n] */, void* const* dst /* host [n] */, int n, int height, int width, int channels,
                     int out_height, int out_width, int x_offset, int y_offset, int mode, const uint8_t* color /* host [3] */,
                     const void* const* background /* host [n], mode 2 */, const void* const* strips /* host [n][4], mode 1 */, void* stream);
int fw_aspect_gauss99_u8(const uint8_t* src, int height, int width, int channels, const uint16_t* weights /* host [99] */,
                         uint16_t* scratch /* device [H][W][C] */, uint8_t* dst, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Frame quality statistics (csrc/quality.hip): the integers every measure of the reference's `FrameQualityScorer.score_frame`
 * (processors/frame_quality_scorer.py:148-427) is a function of, for n uint8 H x W x 3 BGR frames in DEVICE memory (a HOST table of n
 * device pointers; 1 .. 32 frames a call, 2 .. 16384 pixels a side, both sides even: the reference's row-pair subtraction raises on an
 * odd side).  One pass over each frame; the scores are the caller's (quality.py).  tests/quality_ref.frame_statistics is the contract;
 * cv2 parity unpinned.  Gray g = (1868 B + 9617 G + 4899 R + 8192) >> 14; L is L of the 8-bit gamma Lab of fw_bgr_to_lab_u8; every
 * stencil reads BORDER_REFLECT_101.
 *   sums [n][12] int64: 0 sum lap, 1 sum lap^2 (lap = the 3 x 3 cross Laplacian of g), 2 sum d, 3 sum d^2 (d = |g - blur|, blur the
 *     1 4 6 4 1 taps in both directions, (sum + 128) >> 8), 4 sum |g[y-1][x-1] - g[y-1][x+1] - g[y+1][x-1] + g[y+1][x+1]|, 5 and 6 the
 *     number of pixels whose |Sobel x of L| (ksize 3) is above 30 / above 5 and at most 30, 7 sum |g[2k][x] - g[2k+1][x]|, 8 sum
 *     |g[y][2k] - g[y][2k+1]|, 9 sum v and 10 sum v^2 over all 3 H W bytes, 11 zero.
 *   histograms [n][512] uint32: 256 bins of g, then 256 bins of all bytes.
 *   block_sums [n][R + C] uint32, R = len(range(8, H - 8, 8)), C = len(range(8, W - 8, 8)): sum_x |g[i][x] - g[i-1][x]| for each such
 *     row i, then sum_y |g[y][j] - g[y][j-1]| for each such column j.  May be any non-NULL pointer when R + C = 0.
 *   thumbnails [n][1024] uint8: cv2.resize(g, (32, 32)) as fw_resize_linear_u8 computes it (a copy at 32 x 32, the 2 x 2 mean at 64 x 64).
 * scratch: fw_quality_scratch_bytes(n, height, width) bytes of DEVICE memory, 8-byte aligned, where the workgroups leave their partial
 * sums and histograms for a second small launch to add; 0 from that function means a bad argument.  sums is 8-byte aligned too.
 * Everything is an integer (plain stores, and integer atomics for the block sums, which are zeroed on the stream first): the same in
 * every run.  The entry only enqueues work and never waits for the device (the Lab tables are made on a device's first call).
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, n outside 1 .. 32, a side outside 1 .. 16384 or odd, a
 * misaligned scratch or sums, an output or the scratch that overlaps a frame of the call, an output that overlaps the scratch. */
size_t fw_quality_scratch_bytes(int n, int height, int width);
int fw_quality_stats_u8(const void* const* frames /* host [n] */, int n, int height, int width, void* scratch, int64_t* sums /* device [n][12] */,
                        uint32_t* histograms /* device [n][512] */, uint32_t* block_sums /* device [n][R + C] */,
                        uint8_t* thumbnails /* device [n][1024] */, void* stream);

/* -------------------------------------------------------------------------------------------------
 * SDR to HDR conversion of final frames (csrc/hdr.hip): the frame path of the reference's `HDRConverter.convert_frame`
 * (processors/hdr_conversion.py:573-882) on uint8 / uint16 H x W x 3 BGR frames in DEVICE memory, 8 .. 16384 pixels a side, to
 * uint16 BGR.  tests/hdr_ref.py is the contract, byte for byte where a quantising step is on and the curve is rational (cv2's CLAHE,
 * addWeighted, Lab and HSV as that file restates them; cv2 parity unpinned); hdr.py derives everything below from an HDRConfig.
 *   fw_hdr_params: every constant already rounded to float32 by the caller, as numpy rounds a Python float that meets a float32
 *     array.  matrix: rows R, G, B over (R, G, B), applied as round(m0 r), fma(m1, g, .), fma(m2, b, .).  lum_weights over (B, G, R).
 *     curve 0 REINHARD k = {(peak / 100)^2}; 1 ACES {peak / 100, a, b, c, d, e}; 2 HABLE {peak / 100, A, C B, D E, B, D F, E / F,
 *     1 / hable(peak / 100)}; 3 MOBIUS {peak / 100, transition, 1 - transition, -slope}.  clip_code: the first code whose normalised
 *     value exceeds 0.98.  transfer 0 PQ k = {peak / 10000, m1, m2, c1, c2, c3}; 1 HLG {1 / 12, a, b, c} (read only when neither
 *     local_contrast nor saturation is set).  hue_scale: 6 / 180.
 *   gamma: DEVICE float32 [256] (uint8 input) or [65536] (uint16): power(code / maxv, 2.2) as numpy evaluates it.
 *   tail: DEVICE uint16 [2][256]: the transfer function and the 16-bit quantisation of byte / 255 and of float32(byte / 255 * 0.95);
 *     hsv_div: DEVICE int32 [512]: round((255 << 12) / i), then round((180 << 12) / (6 i)), entry 0 of each 0.
 *   fw_hdr_convert: n frames (HOST tables of n device pointers, 1 .. 32) -> dst (uint16, n x H W 3).  With local_contrast: a pass
 *     that accumulates the 8 x 8 x 256 CLAHE tile histograms (integer atomics), a small launch that makes the 64 byte LUTs, and the
 *     pass that writes; scratch is fw_hdr_scratch_bytes(n) bytes of DEVICE memory, 4-byte aligned (else it may be NULL).  With
 *     saturation only: one pass through the tail table.  With neither: one pass, the transfer function per pixel in float32 (powf,
 *     logf: within the error bound of DESIGN K20 of a float64 evaluation, not bit-pinned).
 *   fw_hdr_tonemap_f32: steps 1 - 3 of one frame as float32 H W 3 (recover != 0: times the highlight gain where the flag is set);
 *     fw_hdr_quantise_u8: trunc(. * 255) of that plane; fw_hdr_clahe_u8: cv2.createCLAHE(2.0, (8, 8)).apply on a uint8 H x W plane;
 *     fw_hdr_saturation_u8: BGR -> HSV, s = trunc(clip(s * boost, 0, 255)), HSV -> BGR on n_pixels interleaved pixels;
 *     fw_hdr_transfer_f32: the transfer function and trunc(clip(. * 65535, 0, 65535)) of `count` float32 values.
 * The entries only enqueue work (the Lab tables are made on a device's first call).  Refused with FW_ERR_INVALID and a message,
 * nothing launched: NULL pointers, n outside 1 .. 32, a side outside 8 .. 16384, sample_bytes other than 1 or 2, a curve or a
 * transfer out of range, misaligned 16-bit or float buffers, a dst that overlaps a frame or another dst of the call. */
typedef struct fw_hdr_params {
    float matrix[9];
    float lum_weights[3];
    float curve_k[8];
    float transfer_k[8];
    float lum_floor;          /* 0.0001 */
    float recover_gain;       /* 0.95 */
    float saturation_boost;
    float hue_scale;
    int32_t use_matrix, curve, transfer, local_contrast, saturation, recover, clip_code;
} fw_hdr_params;
size_t fw_hdr_scratch_bytes(int n);
int fw_hdr_convert(const void* const* frames /* host [n] */, void* const* dst /* host [n] */, int n, int height, int width, int sample_bytes,
                   const fw_hdr_params* params, const float* gamma, const uint16_t* tail, const int32_t* hsv_div, void* scratch, void* stream);
int fw_hdr_tonemap_f32(const void* frame, int height, int width, int sample_bytes, const fw_hdr_params* params, const float* gamma,
                       int recover, float* dst, void* stream);
int fw_hdr_quantise_u8(const void* frame, int height, int width, int sample_bytes, const fw_hdr_params* params, const float* gamma,
                       uint8_t* dst, void* stream);
int fw_hdr_clahe_u8(const uint8_t* plane, int height, int width, void* scratch, uint8_t* dst, void* stream);
int fw_hdr_saturation_u8(const uint8_t* bgr, int64_t n_pixels, const int32_t* hsv_div, float boost, float hue_scale, uint8_t* dst, void* stream);
int fw_hdr_transfer_f32(const float* plane, int64_t count, const fw_hdr_params* params, uint16_t* dst, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Compression-artifact removal, the classical path (csrc/qp_artifacts.hip, DESIGN K21): the frame path of the reference's
 * processors/qp_artifact_removal.py with backend 'opencv' on uint8 BGR H x W x 3 DEVICE frames; tests/qp_artifact_ref.py is the
 * contract, byte for byte.  Tables are DEVICE float32 arrays that the host builds in float64:
 *   color [768]: exp(k^2 * -0.5 / sigma_color^2); space [(2r+1)^2], r = max(d / 2, 1): exp((i^2 + j^2) * -0.5 / sigma_space^2), row-major
 *   (entries outside the circular support are not read); gauss15: HOST float32 [15], cv2.getGaussianKernel(15, 0);
 *   noise_table [65536]: standard-normal quantiles at (k + 0.5) / 65536 times 1 + 2 strength.
 *   fw_bilateral_u8c3: cv2.bilateralFilter(frame, d, ...), d 2 .. 15, REFLECT_101, L1 colour distance, float32 sums in the stated order.
 *   fw_gaussian5_u8: cv2.GaussianBlur(frame, (5, 5), 0) as exact fixed point, ([1 4 6 4 1] x [1 4 6 4 1] + 128) >> 8.
 *   fw_qp_artifacts_u8: type_mask bit 0 blocking (bilateral with d, then the float64 blend with the 5 x 5 Gaussian on the rows and
 *     columns next to a multiple of block_size: 4, 8, 16 or 32), bit 1 ringing (Canny 50 / 150, 5 x 5 maximum minus the edges, float32
 *     5-tap Gaussian, float64 blend with the 5 x 5 Gaussian), bit 2 banding (gray, Laplacian, 1 - clip(|.| / 30), 15-tap float32 Gaussian,
 *     out = trunc(clip(frame + noise * mask * strength, 0, 255)) in float64), applied in that order.  The dither is `noise`
 *     (float32 H x W x 3) where it is not NULL, else noise_table[mix64(noise_key + pixel * 3 + channel) >> 48] with the splitmix64
 *     finaliser; noise_key is the host-mixed (seed, frame index).  Tables of steps that the mask leaves out may be NULL.  scratch:
 *     fw_qp_artifacts_scratch_bytes(height, width) bytes, 256-byte aligned.  With ringing the call synchronises `stream` (the
 *     hysteresis reads its round flags on the host); otherwise it only enqueues.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, a side outside 1 .. 16384, channels other than 3,
 * d outside 2 .. 15, a block size other than 4, 8, 16, 32, a type mask outside 0 .. 7, a strength outside (0, 1], an `out` that
 * overlaps `frame`. */
size_t fw_qp_artifacts_scratch_bytes(int height, int width);
int fw_bilateral_u8c3(const uint8_t* frame, uint8_t* out, int height, int width, int channels, int d, const float* color, const float* space,
                      void* stream);
int fw_gaussian5_u8(const uint8_t* frame, uint8_t* out, int height, int width, int channels, void* stream);
int fw_qp_artifacts_u8(const uint8_t* frame, uint8_t* out, int height, int width, int channels, int d, const float* color, const float* space,
                       const float* gauss15, double strength, int block_size, int type_mask, const float* noise, const float* noise_table,
                       uint64_t noise_key, void* scratch, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Missing-frame generation (csrc/frame_generation.hip, DESIGN K22): the frame methods of the reference's
 * processors/frame_generation.py on uint8 BGR H x W x 3 DEVICE frames; tests/frame_generation_ref.py is the contract, byte for
 * byte.  Device pointers, caller-owned scratch, explicit stream; nothing is allocated and nothing synchronises.
 *   fw_framegen_warp_blend_u8: one frame of `_generate_optical_flow` behind its two Farneback flows (float32 H x W planes, cv2's
 *     convention): map = grid + flow * t in float32 (product, then sum), the other frame with 1 - t; both sampled with the 1 / 32
 *     pixel INTER_LINEAR arithmetic and BORDER_REFLECT at any distance; out = addWeighted(warped_before, 1 - t, warped_after, t).
 *   fw_framegen_grain_std_u8: *std_out = the population standard deviation of gray - GaussianBlur(gray, (0, 0), 2) in float32 (17
 *     taps, REFLECT_101, rows then columns, acc += p[k] * c[k] left to right), reduced in float64 through per-workgroup partials in a
 *     fixed order (no atomics: the same bits on every run) and rounded once.  gauss17: HOST float32 [17].  scratch:
 *     fw_framegen_grain_scratch_bytes(height, width) bytes, 8-byte aligned.  Sides of 16 pixels or more.
 *   fw_framegen_finish_u8: the grain (ref_std, cur_std: DEVICE float32 scalars, both NULL: no grain step), where *cur_std > 0 and
 *     *ref_std > *cur_std: trunc(clip(float32(v) + z * float64(*ref_std - *cur_std), 0, 255)) with one z a pixel for its three
 *     channels, z = draws[pixel] (DEVICE float64 H x W) where draws is not NULL, else quantiles[mix64(noise_key + pixel) >> 48]
 *     (DEVICE float64 [65536], standard-normal quantiles at (k + 0.5) / 65536); then addWeighted(before, 1 - alpha_before, v,
 *     alpha_before) where before is not NULL, then the same against after.  out may be generated itself.
 *   fw_framegen_extrapolate_u8: one frame of `_extrapolate_frames`: trunc(clip(float32(reference) + noise, 0, 255)); noise (float32
 *     H x W x 3) where it is not NULL, else noise_table[mix64(noise_key + pixel * 3 + channel) >> 48] (float32 [65536]: 2 x the
 *     quantiles).
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, a side outside 1 .. 16384 (16 .. 16384 for the
 * statistic), t outside (0, 1), a non-finite alpha of a blend that is due, misaligned float buffers, an out that overlaps a source
 * frame (other than fw_framegen_finish_u8's out == generated).  fw_framegen_grain_scratch_bytes returns 0 on invalid arguments. */
int fw_framegen_warp_blend_u8(const uint8_t* before, const uint8_t* after, const float* fwd_x, const float* fwd_y, const float* bwd_x,
                              const float* bwd_y, int height, int width, double t, uint8_t* out, void* stream);
size_t fw_framegen_grain_scratch_bytes(int height, int width);
int fw_framegen_grain_std_u8(const uint8_t* frame, int height, int width, const float* gauss17, void* scratch, float* std_out, void* stream);
int fw_framegen_finish_u8(const uint8_t* generated, uint8_t* out, int height, int width, const float* ref_std, const float* cur_std,
                          const double* draws, const double* quantiles, uint64_t noise_key, const uint8_t* before, double alpha_before,
                          const uint8_t* after, double alpha_after, void* stream);
int fw_framegen_extrapolate_u8(const uint8_t* reference, uint8_t* out, int height, int width, const float* noise, const float* noise_table,
                               uint64_t noise_key, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Cross-frame temporal consistency (csrc/temporal_consistency.hip, DESIGN K23): the classical path of the reference's
 * processors/cross_attention_temporal.py on uint8 BGR H x W x 3 DEVICE frames; tests/temporal_consistency_ref.py is the contract,
 * byte for byte.  Device pointers, explicit stream; nothing is allocated and nothing synchronises.
 *   fw_tcons_gray_hist_u8: hist[256] (DEVICE uint32) = the counts of cvtColor(BGR2GRAY) of one frame, what cv2.calcHist counts in
 *     `_detect_scene_change`; the cell is cleared and filled by integer adds, the same bits on every run.
 *   fw_tcons_apply_u8: `_detect_flicker(prev, cur, next)` and the blend of `_apply_optical_flow_consistency` in one launch: the
 *     binary mask min(dp, dn) * (1 - nb) > flicker_threshold of the gray absolute differences over 255, GaussianBlur((5, 5), 0) with
 *     BORDER_REFLECT_101 as the integer k = 256 x mask, and out = trunc(cur * (1 - m3) + ((prev + next) / 2) * m3), m3 =
 *     (k / 256) * blend_strength, every step one float32 operation.  flicker_threshold and blend_strength are the reference's Python
 *     floats rounded to float32.  out, mask_out (float32 H x W, k / 256) and area_out (one uint64: cleared, then the sum of k over the
 *     frame; the reference's np.mean(mask) is area / (256 H W)) may each be NULL, not all three.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL frames, a side outside 3 .. 16384 (1 .. 16384 for the
 * histogram), a non-finite threshold, a strength outside [0, 1], misaligned mask_out / area_out / hist, an out that overlaps a frame. */
int fw_tcons_gray_hist_u8(const uint8_t* frame, int height, int width, uint32_t* hist, void* stream);
int fw_tcons_apply_u8(const uint8_t* prev, const uint8_t* cur, const uint8_t* next, int height, int width, float flicker_threshold,
                      float blend_strength, uint8_t* out, float* mask_out, uint64_t* area_out, void* stream);

/* -------------------------------------------------------------------------------------------------
 * Perceptual tuning of final frames (csrc/perceptual.hip, DESIGN K24): the frame path of the reference's
 * processors/perceptual_tuning.py (`PerceptualTuner.apply_to_frame`) on uint8 BGR H x W x 3 DEVICE frames; tests/perceptual_ref.py is
 * the contract, byte for byte.  Device pointers, explicit stream; nothing synchronises (the Lab tables are made on a device's first
 * call with detail recovery).  Every weight is the reference's Python double rounded to float32 by the caller.
 *   fw_ptune_unsharp_u8: addWeighted(src, w_src, GaussianBlur(src, (0, 0), 3), w_blur, 0) in one launch: 19 taps in 8-bit fixed point,
 *     rows into 16 bits, columns into 32, (v + 2^15) >> 16, BORDER_REFLECT_101 as often as it takes.
 *   fw_ptune_gauss19_table: HOST function (no GPU needed): the 19 integer taps of that blur (sum 256) into out19.
 *   fw_ptune_clahe_u8: cv2.createCLAHE(clip, (8, 8)).apply on a uint8 H x W plane; limit = max(int(clip * tile area / 256), 1), the
 *     caller's, computed in double.  fw_ptune_detail_u8: BGR -> Lab, that CLAHE in place of L, Lab -> BGR.
 *   fw_ptune_grain_u8: g = gray(original); addWeighted(result, 1.0, max(g - GaussianBlur(g, (5, 5), 0), 0) on all channels, amount, 0).
 *   fw_ptune_apply_u8: the steps that params switches on, in the reference's order: fastNlMeansDenoisingColored(h, h, 7, 21) where
 *     denoise_h > 0 (a launch of fw_nlmeans_colored_u8), then sharpen, colour (fw_hdr_saturation_u8's pixel step; hsv_div is its
 *     DEVICE table), detail and grain (of src, the original).  Without detail: one launch behind the denoise (nothing on: a copy).  With
 *     it: one pass that stores the sharpened and coloured bytes, the tile histograms of their L, the 64 maps, one pass that writes.
 *   scratch: DEVICE memory, 4-byte aligned.  fw_ptune_scratch_bytes(height, width, params) is what fw_ptune_apply_u8 needs with those
 *     params: 0 without denoise and detail (scratch may be NULL), 81920 bytes (the histograms and the maps) with detail alone or with
 *     grain, one frame more where sharpen or colour run in front of detail, and two frames and the non-local means' own planes with
 *     denoise.  params = NULL: the 81920 bytes of fw_ptune_clahe_u8 and fw_ptune_detail_u8.  0 on bad sizes.
 * Refused with FW_ERR_INVALID and a message, nothing launched: NULL pointers, a side outside 3 .. 16384 (8 .. 16384 with detail
 * recovery or CLAHE), weights that are not finite, a limit below 1, a dst that overlaps src (or result / original): every output
 * reads a neighbourhood. */
typedef struct fw_ptune_params {
    int32_t denoise_h;          /* 0: no denoise */
    int32_t sharpen, colour, detail, grain;
    int32_t clahe_limit;
    float w_src, w_blur;        /* sharpen */
    float boost, hue_scale;     /* colour: hue_scale = float32(6 / 180) */
    float grain_amount;
    const int32_t* hsv_div;     /* colour: DEVICE [512], as fw_hdr_saturation_u8 takes it */
} fw_ptune_params;
size_t fw_ptune_scratch_bytes(int height, int width, const fw_ptune_params* params);
int fw_ptune_gauss19_table(int32_t* out19);
int fw_ptune_unsharp_u8(const uint8_t* src, uint8_t* dst, int height, int width, float w_src, float w_blur, void* stream);
int fw_ptune_clahe_u8(const uint8_t* plane, uint8_t* dst, int height, int width, int limit, void* scratch, void* stream);
int fw_ptune_detail_u8(const uint8_t* src, uint8_t* dst, int height, int width, int limit, void* scratch, void* stream);
int fw_ptune_grain_u8(const uint8_t* result, const uint8_t* original, uint8_t* dst, int height, int width, float amount, void* stream);
int fw_ptune_apply_u8(const uint8_t* src, uint8_t* dst, int height, int width, const fw_ptune_params* params, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRAMEWRIGHT_HIP_H */
