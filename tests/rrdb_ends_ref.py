"""TEST INFRASTRUCTURE ONLY (never imported by the product): the two ends of the RRDBNet - what csrc/rrdbnet.hip runs in front of the
first RRDB (run_head) and behind the last one (run_tail) - in plain numpy float64, with per-element bounds.
tests/test_rrdb_ends_ref_host.py pins every restatement to torch in float64 and shows that each planted defect leaves its bound;
tests/test_rrdb_tail_ops_gpu.py (fw_conv3x3_hr_last_nhwc, both forms) and tests/test_rrdb_ends_gpu.py (fw_rrdbnet_run_head /
run_tail) hold the kernels to it.

Head.  csrc/frame_ops.hip (u8_to_nhwc_kernel): sample * fp32(1 / top), top = 255 or 65535, rounded to the operand type T, BGR -> RGB.
The contract is typed(fp32(v) / fp32(top)); for every one of the 256 and 65536 levels and both operand types the two give the same
bits (checked exhaustively in the host test), so ``frame_to_nhwc`` is the contract.  The x2 model reads pixel_unshuffle(2) of the frame
reflect-padded on the right and bottom to even size: channel c * 4 + dy * 2 + dx = colour c of pixel (2 y + dy, 2 x + dx), zeros from
channel 12 up.  conv_first contracts ONE 32-channel chunk.

Tail, op level (fw_conv3x3_hr_last_nhwc).  h = T(lrelu(conv_hr(x) + b)), LeakyReLU's slope the fp32 constant 0.2f; the float plane is
conv_last of the typed h, h outside the image ZERO; the images are rint(clamp(plane, 0, 1) * top) in BGR, cropped to img_H x img_W with
row stride img_W.

Tail, engine level (run_tail).  Rounding points, read from csrc/rrdbnet.hip; every sum stays float64 (the model holds the roundings
of a path, not its summation order):

  every path     weights typed (pack_conv3x3_weights), biases fp32
                 conv_body contracts planes 0-1 of the concat buffer behind the last RRDB: hi = T(trunk).  The lo planes 6-7 of the
                 split trunk and the fp32 trunk buffer are NOT read: the split and the fp32 trunk share one model here
                 body = T(fp32(conv_body(hi) * 1 + F)) with F conv_first's fp32 output, stored typed (EPI_RESIDUAL, f32_native res1)
                 U1 = T(lrelu(conv_up1(nearest2(body)))), U2 = T(lrelu(conv_up2(nearest2(U1)))), h = T(lrelu(conv_hr(U2))): typed stores
                 (h: the fused form hands the same typed bits on in registers - csrc/conv3x3_hr_last.hip's header)
                 the float plane: fp32(conv_last(h))
  phase up-conv  (FW_RRDB_UP_PHASE, default)  the four 2x2 phase kernels are sums of the fp32 taps rounded to T ONCE
                 (conv_pair_ref.up2x_phase, which is called, not restated); the gathering form multiplies by the typed taps
  Winograd hr    (FW_RRDB_HR_WINO=1 with FW_RRDB_C5_WINO=1, f16)  U = f16 of the fp32-transformed fp32 weights, V = B^T d in f16
                 arithmetic: oracle/winograd_ref.winograd_emulation (called, not restated)

Bounds (u = 2^-24, gamma(k) = k u / (1 - k u), helpers of tests/ifnet_glue_ref.py), counted from the kernels, none fitted to what a
kernel returns.  The convention is conv_epilogue_ref's: accumulators start at the bias, one fp32 rounding of the running sum per
v_mfma_f32_16x16x32 (one per tap and 32-channel chunk), products of typed operands exact; A = |bias| + sum |w| |x|.

* conv_first's fp32 output: 9 taps x 1 chunk: gamma(9 * 1 + 1) A_t (the + 1 as in every conv bound of the suite).
* the unfused h: 9 x 2 MFMAs, + 1 for LeakyReLU's product (Lipschitz 1: a t on the other side of zero costs no more than its
  error): typed_allowance(h_ref, gamma(9 * 2 + 1) A_h, T).
* the unfused float plane against float64 conv_last of the scratch's own bits: 9 x 2 MFMAs + 1: gamma(9 * 2 + 1) S.
* the fused float plane against the same sum (csrc/conv3x3_hr_last.hip, epilogue): z[dy][dx] is two chained MFMAs from a zero
  accumulator (2 roundings), r_dy = (z0 + z1) + z2 (2), out = ((b + r_0) + r_1) + r_2 (3): FUSED_ROUNDINGS = 7 on the longest path,
  and one more: gamma(7 + 1) S.  That is 16 times under the 2^-17 S = 128 u S which tests/test_tail_fused_gpu.py allows between the
  two forms (whose own difference may reach gamma(19) + gamma(8)).
* the images: bit for bit rint(clip(plane, 0, 1) * top) in float32 from the kernel's OWN float plane - the kernels emit both from the
  same registers -, and inside ``u8_window`` / ``u16_window`` of the float64 reference.

Measured on an MI355X: DESIGN.md (What pins the RRDBNet's two ends).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import conv_pair_ref as CP
import rrdb_block_ref as RB
from conv_epilogue_ref import conv3x3, rnd, to_bytes, u16_window                                         # noqa: F401  (re-exported)
from ifnet_glue_ref import U8_WINDOW_SHARE, from_bits, gamma, to_bits, typed_allowance, u8_window        # noqa: F401  (re-exported)
from oracle import winograd_ref as WR
from restormer_block_ref import round_to

S = RB.S                                    # lrelu4's slope as the kernels hold it: fp32(0.2)
FUSED_ROUNDINGS = 7                         # module docstring
NUM_BLOCK = RB.NUM_BLOCK
LAST_GAIN = 8.0                             # on conv_last.weight: the float plane then spans about [-0.5, 1.6] and meets both clamps

HEAD_DEFECTS = ("dydx_swapped", "zero_pad", "bgr_kept", "div255_on_u16")
TAIL_DEFECTS = ("feat_dropped", "feat_scaled", "body_rotation_off", "lrelu_on_body", "lrelu_missing_up1")
IMAGE_DEFECTS = ("h_outside_lrelu_bias", "crop_stride_W", "truncate", "top255_on_u16")

# phase: the up-convs as four 2x2 phase convolutions; wino: conv_hr in the Winograd form.  (Split or fp32 trunk, fused or unfused
# tail: no rounding point differs - module docstring.)
TailPath = namedtuple("TailPath", "phase wino")


# ---- head --------------------------------------------------------------------------------------------------------------------------
def frame_to_nhwc(frame_bgr: np.ndarray, dtype: str, scale: int, defect: str | None = None) -> np.ndarray:
    """uint8 / uint16 BGR (H, W, 3) -> the exact typed values conv_first reads, float64 (Ht, Wt, 32)."""
    assert defect is None or defect in HEAD_DEFECTS
    assert frame_bgr.dtype in (np.uint8, np.uint16) and frame_bgr.ndim == 3 and frame_bgr.shape[2] == 3
    top = 255.0 if (frame_bgr.dtype == np.uint8 or defect == "div255_on_u16") else 65535.0
    f = frame_bgr.astype(np.float32) / np.float32(top)
    v = from_bits(to_bits(f, dtype), dtype).reshape(f.shape)
    rgb = v if defect == "bgr_kept" else v[:, :, ::-1]
    H, W, _ = rgb.shape
    if scale != 2:
        out = np.zeros((H, W, 32))
        out[:, :, :3] = rgb
        return out
    assert H >= 2 and W >= 2
    Ht, Wt = (H + 1) // 2, (W + 1) // 2
    pad = np.zeros((2 * Ht, 2 * Wt, 3))
    pad[:H, :W] = rgb
    if defect != "zero_pad":                                      # torch 'reflect' on the right / bottom edge: n -> n - 2
        if W & 1:
            pad[:H, W] = rgb[:, W - 2]
        if H & 1:
            pad[H] = pad[H - 2]
    out = np.zeros((Ht, Wt, 32))
    for c in range(3):
        for dy in range(2):
            for dx in range(2):
                ch = c * 4 + (dx * 2 + dy if defect == "dydx_swapped" else dy * 2 + dx)
                out[:, :, ch] = pad[dy::2, dx::2, c]
    return out


def conv_first(x32: np.ndarray, sd, dtype: str):
    """conv_first in float64 on the exact typed values: (t, A_t), (Ht, Wt, 64)."""
    w = rnd(sd["conv_first.weight"], dtype)
    return conv3x3(x32[:, :, :w.shape[1]], w, sd["conv_first.bias"])


def bound_first(A_t):
    return gamma(9 * 1 + 1) * A_t


def head_trunk(feat_f32: np.ndarray, dtype: str, split: bool) -> np.ndarray:
    """What RRDB 0 reads, from conv_first's own fp32 output: f32(T(F)) + f32(T(F - f32(T(F)))) on the split trunk (the sum of an f16 /
    bf16 pair one below the other is exact in fp32), F itself on the fp32 trunk.  Bit for bit."""
    F = np.asarray(feat_f32, np.float32)
    if not split:
        return F
    hi, lo = RB._hi_lo(F.astype(np.float64), dtype)
    return (hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float32)


# ---- tail, op level ------------------------------------------------------------------------------------------------------------------
def lrelu(t, slope: float = S):
    return np.maximum(t, slope * t)


def conv_hr(x, w_typed, b, slope: float = S):
    """h = lrelu(conv_hr(x) + b) in float64 and A_h: x (H, W, 64) and w exact typed values."""
    t, A = conv3x3(x, w_typed, b)
    return lrelu(t, slope), A


def allow_h(h_ref, A_h, dtype: str):
    return typed_allowance(h_ref, gamma(9 * 2 + 1) * A_h, dtype)


def conv_last(h, w_typed, b, defect: str | None = None, b_hr=None):
    """The float RGB plane (H, W, 3) of a given typed h (H, W, 64) in float64 and S = |b| + sum |W| |h|.  h outside the image is zero -
    the defect puts lrelu(conv_hr's bias) there, as a kernel that computes h on a halo would unless it zeroes it."""
    assert defect in (None, "h_outside_lrelu_bias")
    if defect is None:
        return conv3x3(h, w_typed, b)
    H, W, _ = h.shape
    wide = np.zeros((H + 2, W + 2, 64)) + lrelu(np.asarray(b_hr, np.float64))
    wide[1:-1, 1:-1] = h
    v, A = conv3x3(wide, w_typed, b)
    return v[1:-1, 1:-1], A[1:-1, 1:-1]


def bound_plane(Sm, fused: bool):
    return gamma(FUSED_ROUNDINGS + 1 if fused else 9 * 2 + 1) * Sm


def to_image(val, top: int, defect: str | None = None) -> np.ndarray:
    """rint(clip(val, 0, 1) * top) in BGR, int64, in float64 arithmetic."""
    assert defect in (None, "truncate", "top255_on_u16")
    return to_bytes(val, 255 if defect == "top255_on_u16" else top, "truncate" if defect == "truncate" else None)


def to_image_f32(plane_f32: np.ndarray, top: int) -> np.ndarray:
    """The same in float32 from a kernel's own float plane, as the kernels compute it: rintf(fminf(fmaxf(c, 0), 1) * top), BGR."""
    p = np.asarray(plane_f32, np.float32)
    v = np.minimum(np.maximum(p, np.float32(0)), np.float32(1)) * np.float32(top)
    assert v.dtype == np.float32
    return np.rint(v).astype(np.int64)[:, :, ::-1]


def crop(full: np.ndarray, img_H: int, img_W: int, defect: str | None = None) -> np.ndarray:
    """What a buffer of img_H * img_W * 3 elements holds: the top-left img_H x img_W of `full` (H, W, 3) with row stride img_W - the
    defect stores with row stride W (and drops what falls behind the buffer)."""
    assert defect in (None, "crop_stride_W")
    if defect is None:
        return np.ascontiguousarray(full[:img_H, :img_W]).reshape(-1)
    W = full.shape[1]
    buf = np.zeros(img_H * img_W * 3, full.dtype)
    for y in range(img_H):
        row = full[y, :img_W].reshape(-1)
        at = y * W * 3
        n = max(0, min(row.size, buf.size - at))
        buf[at:at + n] = row[:n]
    return buf


# ---- tail, engine level ----------------------------------------------------------------------------------------------------------------
def nearest2(x):
    return np.repeat(np.repeat(x, 2, 0), 2, 1)


def _w(sd, key):
    return np.asarray(sd[key + ".weight"], np.float32), np.asarray(sd[key + ".bias"], np.float32)


def tail_exact(feat, trunk, sd, defect: str | None = None, other=None, slope: float = 0.2):
    """conv_last(lrelu(conv_hr(lrelu(conv_up2(nearest2(lrelu(conv_up1(nearest2(conv_body(trunk) + feat))))))))) in plain float64:
    the RGB plane (4 Ht, 4 Wt, 3).  ``other``: what the concat buffer one rotation off holds (defect "body_rotation_off")."""
    assert defect is None or defect in TAIL_DEFECTS
    feat, trunk = np.asarray(feat, np.float64), np.asarray(trunk, np.float64)
    src = np.asarray(other, np.float64) if defect == "body_rotation_off" else trunk
    body = conv3x3(src, *_w(sd, "conv_body"))[0]
    if defect == "lrelu_on_body":
        body = lrelu(body, slope)
    body = body + (0.0 if defect == "feat_dropped" else (0.2 if defect == "feat_scaled" else 1.0) * feat)
    u1 = conv3x3(nearest2(body), *_w(sd, "conv_up1"))[0]
    if defect != "lrelu_missing_up1":
        u1 = lrelu(u1, slope)
    u2 = lrelu(conv3x3(nearest2(u1), *_w(sd, "conv_up2"))[0], slope)
    h = lrelu(conv3x3(u2, *_w(sd, "conv_hr"))[0], slope)
    return conv3x3(h, *_w(sd, "conv_last"))[0]


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def tail_rounded(feat, trunk, sd, rt: str, path: TailPath, defect: str | None = None, other=None):
    """The same chain at the rounding points of `path` (module docstring), from the engine's lay-in of the fp32 trunk and feat."""
    assert defect is None or defect in TAIL_DEFECTS
    assert not path.wino or rt == "f16"
    F = _f32(feat)
    lay = RB.lay_in(other if defect == "body_rotation_off" else trunk, rt, RB.Path("lo_rrdb", False, False))
    w, b = _w(sd, "conv_body")
    body = conv3x3(lay.hi, rnd(w, rt), b)[0]                       # planes 0-1 alone: lay.lo is not contracted
    if defect == "lrelu_on_body":
        body = lrelu(body)
    body = round_to(_f32(body + (0.0 if defect == "feat_dropped" else (S if defect == "feat_scaled" else 1.0) * F)), rt)

    def up(x, key, act=True):
        w, b = _w(sd, key)
        if path.phase and act:
            return round_to(CP.up2x_phase(x, w, b, rt)[0], rt)
        t = conv3x3(nearest2(x), rnd(w, rt), b)[0]                 # the gathering form (and the defect without LeakyReLU, on either path)
        return round_to(lrelu(t) if act else t, rt)

    u1 = up(body, "conv_up1", act=defect != "lrelu_missing_up1")
    u2 = up(u1, "conv_up2")
    w, b = _w(sd, "conv_hr")
    if path.wino:
        h = WR.winograd_emulation(u2.astype(np.float16), w, b, act=1)[0]
    else:
        h = lrelu(conv3x3(u2, rnd(w, rt), b)[0])
    h = round_to(h, rt)
    w, b = _w(sd, "conv_last")
    return _f32(conv3x3(h, rnd(w, rt), b)[0])


bounds = RB.bounds            # the 2 q yardstick: (max error, q, 2 q + 1e-6 max |exact|, mean error, its limit)


# ---- seeded inputs shared by the host and the GPU tests ----------------------------------------------------------------------------------
# op level (H, W): one pixel, a few; the fused kernel's 16 x 30 edges; the unfused 16 x 32 edges; several tiles both ways
OP_SHAPES = [(1, 1), (2, 3), (15, 29), (16, 30), (17, 31), (16, 32), (17, 33), (33, 61), (33, 65)]
OP_WIDE_ROWS = 83                                                 # at wide_width(), f16 only


def wide_width(ncu: int = 256) -> int:
    """tests/test_tail_fused_gpu._column_straddling_width() on a device of `ncu` compute units (1900 on the MI355X's 256): the width
    at which 83 rows give the fused kernel 1.5 tiles per workgroup."""
    return 30 * max(1, ncu // 4) - 20


OP_CROPS = [((33, 65), (32, 63)), ((33, 65), (31, 64)), ((17, 33), (16, 32)), ((17, 31), (16, 30))]


def tail_op_inputs(H: int, W: int, dtype: str, seed: int = 1234):
    """x as tests/test_tail_fused_gpu.Tail draws it, conv_last.weight times LAST_GAIN.  Returns the uint16 bits of x (H, W, 64), its
    exact typed values, and the fp32 w_hr, b_hr, w_last, b_last."""
    from framewright_amd.synth import synthetic_rrdbnet_state
    sd = synthetic_rrdbnet_state(1, 4, seed)
    rng = np.random.default_rng(seed * 7919 + H * 31 + W)
    xb = to_bits(rng.uniform(-1, 1, (H, W, 64)).astype(np.float32), dtype).reshape(H, W, 64)
    w_last = (np.asarray(sd["conv_last.weight"], np.float32) * np.float32(LAST_GAIN)).astype(np.float32)
    return (xb, from_bits(xb, dtype).reshape(H, W, 64), np.ascontiguousarray(sd["conv_hr.weight"], np.float32), sd["conv_hr.bias"].astype(np.float32),
            w_last, sd["conv_last.bias"].astype(np.float32))


def ends_state(scale: int):
    """rrdb_block_ref.lively_state's trunk with conv_last unshrunk by LAST_GAIN (and, for the x2 model, a 12-channel conv_first)."""
    from framewright_amd.synth import synthetic_rrdbnet_state
    sd = RB.lively_state()
    if scale == 2:
        sd["conv_first.weight"], sd["conv_first.bias"] = (synthetic_rrdbnet_state(1, 2, seed=2024)[k] for k in ("conv_first.weight", "conv_first.bias"))
    sd["conv_last.weight"] = (sd["conv_last.weight"] * np.float32(LAST_GAIN)).astype(np.float32)
    return sd


HEAD_FRAMES = {4: [(1, 1), (2, 3), (16, 32), (17, 33), (33, 65)], 2: [(2, 2), (3, 5), (32, 64), (33, 65), (34, 66)]}


def head_frame(H: int, W: int, bits: int) -> np.ndarray:
    """BGR (H, W, 3): where the frame has room, every one of the 256 levels in every channel (8-bit) / samples that use all 16 bits,
    in three different orders; otherwise seeded samples."""
    rng = np.random.default_rng([H, W, bits])
    n = H * W
    if bits == 8:
        f = rng.integers(0, 256, (n, 3))
        if n >= 256:
            for c in range(3):
                f[rng.permutation(n)[:256], c] = np.arange(256)
        return f.astype(np.uint8).reshape(H, W, 3)
    f = rng.integers(0, 65536, (n, 3))
    if n >= 32:
        for c in range(3):                                         # every bit seen set and clear: 0, 65535, and the single bits
            f[rng.permutation(n)[:18], c] = [0, 65535] + [1 << k for k in range(16)]
    return f.astype(np.uint16).reshape(H, W, 3)


# engine-level tail: trunk (Ht, Wt) -> the images (img_H, img_W) of the frames that have that trunk
TAIL_TRUNKS = {4: [((1, 1), (4, 4)), ((2, 3), (8, 12)), ((4, 8), (16, 32)), ((5, 9), (20, 36)), ((9, 17), (36, 68))],
               2: [((9, 17), (34, 66)), ((9, 17), (36, 66)), ((9, 17), (34, 68))]}                # frames 17x33, 18x33, 17x34


def tail_inputs(Ht: int, Wt: int):
    """(feat, trunk, other): lively trunks with different seeds, doubled - exact in every format, so each value keeps its place between
    two numbers of the operand type - because at twice the size the float plane meets both clamps (asserted on the host) and at the
    plain size only the upper one; `other` stands for the concat buffer one rotation off."""
    return tuple((np.float32(2.0) * RB.lively_trunk(Ht, Wt, seed)).astype(np.float32) for seed in (7001, 7002, 7003))
