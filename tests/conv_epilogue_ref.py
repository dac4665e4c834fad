"""TEST INFRASTRUCTURE ONLY (never imported by the product): float64 restatements of what fw_conv3x3_nhwc_ex adds to the plain
conv (csrc/conv3x3_mfma.hip: PReLU, chan_scale in front of the residual add, post_act, the fp32 channel slice) and of SRVGGNetCompact's
two ends (csrc/frame_ops.hip: fw_u8_to_nhwc, fw_pixel_shuffle_add_u8), each with a per-element bound, in plain numpy.
tests/test_conv_epilogue_ref_host.py pins them to torch in float64 (F.conv2d, F.prelu, F.leaky_relu(conv * beta + x), F.pixel_shuffle +
F.interpolate(nearest)) and shows that each listed defect leaves its bound; tests/test_conv_epilogue_gpu.py and
tests/test_srvgg_ops_gpu.py hold the kernels to them.

Bounds (u = 2^-24, gamma(k) = k u / (1 - k u), helpers of tests/ifnet_glue_ref.py), none fitted to what a kernel returns:

* the conv: the accumulators start at the bias and chain one v_mfma_f32_16x16x32 per tap and 32-channel chunk: 9 * cin_chunks MFMAs,
  one fp32 rounding of the running sum each, products of typed operands exact (the convention of oracle/winograd_ref.py).
  A_t = sum |w x| + |bias|.
* PReLU (act == 2): y = t > 0 ? t : slope[n] * t, one product more.  The activation is Lipschitz with constant max(1, |slope|), so
  a t on the other side of zero than the reference's costs no more than that times its error: gamma(9 c + 1) * max(1, |slope|) * A_t.
* residual (res1 != NULL): ``* chan_scale`` 1, ``* s1 + res1`` 2, ``* s2 + res2`` 2, post_act's ``0.2 * o`` 1 (LeakyReLU is Lipschitz
  with constant 1): gamma(9 c + 6) * A with A = (A_t |chan_scale| |s1| + |res1|) |s2| + |res2|; the count is the longest path and is
  used for the shorter ones as well.
  Measured on the MI355X, max |err| / (2^-24 A) (the tests print it per case):
    - PReLU, 9 / 18 MFMAs + 1:        f16 3.87 / 2.62, bf16 3.61 / 2.94
    - residual, 9 / 18 MFMAs + 6:     f16 3.27 / 2.30, bf16 2.69 / 3.45
* typed output: the RNE cast of the kernel's own fp32 output (asserted bit for bit, as tests/test_conv3x3_gpu.py does).
* fw_u8_to_nhwc multiplies by the fp32 constant 1 / 255 where the contract divides; both are within one fp32 rounding of v / 255,
  which is never closer than 2^-19 relative to a rounding point of either operand type (255 has no power of two as a multiple), so
  the typed results agree bit for bit: ``u8_to_nhwc`` is typed(fp32(v) / fp32(255)) and the host test checks the other form against it.
* fw_pixel_shuffle_add_u8: conv + px / 255: the division and the sum, gamma(2) * (|conv| + px / 255).  The bytes: ``u8_window``
  (its 65535 analogue: ``u16_window``); the share of elements inside the window is asserted <= ``U8_WINDOW_SHARE`` on the host for
  every input set the GPU test uses.
"""
from __future__ import annotations

import numpy as np

from ifnet_glue_ref import U, U8_WINDOW_SHARE, from_bits, gamma, to_bits, typed_allowance, u8_window   # noqa: F401  (re-exported)

DEFECTS_PRELU = ("slope_n16",)
DEFECTS_RES = ("gamma_n4", "post_act_first", "coff_ignored")
DEFECTS_TAIL = ("sub_transposed", "bgr_kept", "truncate")


def rnd(x, dtype: str) -> np.ndarray:
    x = np.asarray(x, np.float32)
    return from_bits(to_bits(x, dtype), dtype).reshape(x.shape)


def conv3x3(x, w, bias):
    """x (H, W, Cin), w (Cout, Cin, 3, 3): exact typed values; bias fp32.  Zero padding.  Returns t = conv + bias and A_t, (H, W, Cout)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    H, W, _ = x.shape
    xp = np.zeros((H + 2, W + 2, x.shape[2]))
    xp[1:-1, 1:-1] = x
    b = np.asarray(bias, np.float64)
    t, A = np.zeros((H, W, w.shape[0])) + b, np.zeros((H, W, w.shape[0])) + np.abs(b)
    for dy in range(3):
        for dx in range(3):
            win = xp[dy:dy + H, dx:dx + W]
            t += win @ w[:, :, dy, dx].T
            A += np.abs(win) @ np.abs(w[:, :, dy, dx].T)
    return t, A


def prelu(t, A, slopes, cin_chunks: int, defect: str | None = None):
    s = np.asarray(slopes, np.float64)
    if defect == "slope_n16":
        s = np.roll(s, -16)
    return np.where(t > 0, t, s * t), gamma(9 * cin_chunks + 1) * np.maximum(1.0, np.abs(s)) * A


def residual(t, A, cin_chunks: int, chan_scale, s1: float, res1, s2: float = 1.0, res2=None, post_act: int = 0, defect: str | None = None):
    """y = (t * chan_scale) * s1 + res1 [; y * s2 + res2] [; lrelu(y, 0.2)].  res1 / res2 (H, W, 64) fp32: the slice the kernel reads
    (the defect "coff_ignored" is the caller's: it passes channels [0, 64) of the wide buffer)."""
    cs = np.asarray(chan_scale, np.float64)
    if defect == "gamma_n4":
        cs = np.roll(cs, -4)
    s1, s2 = float(np.float32(s1)), float(np.float32(s2))
    y, mag = t * cs * s1, A * np.abs(cs) * abs(s1)
    if defect == "post_act_first" and post_act:
        y = np.maximum(y, 0.2 * y)
    y, mag = y + res1.astype(np.float64), mag + np.abs(res1.astype(np.float64))
    if res2 is not None:
        y, mag = y * s2 + res2.astype(np.float64), mag * abs(s2) + np.abs(res2.astype(np.float64))
    if post_act and defect != "post_act_first":
        y = np.maximum(y, 0.2 * y)
    return y, gamma(9 * cin_chunks + 6) * mag


# ---- SRVGG's two ends ------------------------------------------------------------------------------------------------------------
def u8_to_nhwc(img_bgr: np.ndarray, dtype: str, cstride: int, reciprocal: bool = False, defect: str | None = None) -> np.ndarray:
    """uint8 BGR (H, W, 3) -> uint16 bits (H, W, cstride): typed(fp32(v) / fp32(255)) RGB in channels 0..2, zeros above."""
    H, W, _ = img_bgr.shape
    v = img_bgr.astype(np.float32)
    f = v * (np.float32(1.0) / np.float32(255.0)) if reciprocal else v / np.float32(255.0)
    out = np.zeros((H, W, cstride), np.uint16)
    out[:, :, :3] = to_bits(f if defect == "bgr_kept" else f[:, :, ::-1], dtype)
    return out


def shuffle_tail(conv: np.ndarray, img_bgr: np.ndarray, s: int, defect: str | None = None):
    """PixelShuffle(s)(conv) + nearest-upsample(img / 255): conv fp32 (H, W, >= 3 s^2) with channel c s^2 + i s + j, img uint8 BGR.
    Returns RGB (s H, s W, 3) float64 and its bound."""
    H, W, _ = img_bgr.shape
    c = conv[:, :, :3 * s * s].astype(np.float64).reshape(H, W, 3, s, s)                 # [y][x][c][i][j]
    if defect == "sub_transposed":
        c = c.transpose(0, 1, 2, 4, 3)
    ps = c.transpose(0, 3, 1, 4, 2).reshape(H * s, W * s, 3)                             # [y][i][x][j][c]
    px = img_bgr.astype(np.float64) / 255.0
    base = np.repeat(np.repeat(px if defect == "bgr_kept" else px[:, :, ::-1], s, 0), s, 1)
    return ps + base, gamma(2) * (np.abs(ps) + base)


def to_bytes(val, top: int = 255, defect: str | None = None) -> np.ndarray:
    """rint(clamp(val, 0, 1) * top), in BGR order."""
    v = np.clip(val, 0.0, 1.0) * top
    return (np.floor(v) if defect == "truncate" else np.rint(v)).astype(np.int64)[:, :, ::-1]


def u16_window(val, bound):
    """u8_window's 65535 analogue: the smallest and largest uint16 the bound admits, and the share of elements where they differ."""
    c = np.clip(val, 0.0, 1.0)
    w = 65535.0 * (bound + U * c)
    lo, hi = np.rint(np.clip(65535.0 * c - w, 0, 65535)), np.rint(np.clip(65535.0 * c + w, 0, 65535))
    return lo.astype(np.int64), hi.astype(np.int64), float(np.mean(lo != hi))


# ---- seeded inputs shared by the host and the GPU tests --------------------------------------------------------------------------
CONV_SHAPES = [(1, 1), (5, 3), (16, 32), (17, 33), (33, 65)]


def channel_vector(n: int, seed: int) -> np.ndarray:
    """n distinct per-channel factors (PReLU slopes, beta): negative, zero and above 1 among them."""
    v = np.linspace(-0.75, 1.5, n)
    v[np.abs(v).argmin()] = 0.0
    return np.random.default_rng(seed).permutation(v).astype(np.float32)


def conv_inputs(H: int, W: int, cin_chunks: int, cout_tiles: int, dtype: str):
    """Typed x (H, W, 32 chunks) - with one chunk only three channels are live, as SRVGG's body.0 sees its frame -, weights and an
    fp32 bias whose outputs straddle zero.  Returns the uint16 x, the fp32 weights (Cout, Cin, 3, 3) as the packer takes them, the
    bias, and the exact typed values of x and w."""
    rng = np.random.default_rng([H, W, cin_chunks, cout_tiles])
    cin = 3 if cin_chunks == 1 else 32 * cin_chunks
    x = np.zeros((H, W, 32 * cin_chunks))
    x[:, :, :cin] = rng.standard_normal((H, W, cin)) * np.exp(rng.standard_normal((H, W, 1)))
    w = (rng.standard_normal((32 * cout_tiles, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = (0.3 * rng.standard_normal(32 * cout_tiles)).astype(np.float32)
    xb = to_bits(x, dtype).reshape(x.shape)
    return xb, w, b, from_bits(xb, dtype).reshape(x.shape)[:, :, :cin], rnd(w, dtype)


def residual_buffers(H: int, W: int, cstride: int = 160):
    """The wide fp32 buffers res1 / res2 live in (H, W, cstride), every channel live, so that a wrong channel offset reads other values."""
    rng = np.random.default_rng([H, W, cstride])
    return rng.standard_normal((H, W, cstride)).astype(np.float32), rng.standard_normal((H, W, cstride)).astype(np.float32)


def levels_image() -> np.ndarray:
    """uint8 BGR (16, 16, 3) with all 256 levels in every channel, in three different orders."""
    a = np.arange(256)
    return np.stack([a, a[::-1], (a * 7) % 256], -1).astype(np.uint8).reshape(16, 16, 3)


TAIL_SHAPES = [(1, 1), (7, 5), (20, 33)]


def tail_inputs(H: int, W: int, s: int, cstride: int):
    """conv fp32 (H, W, cstride) such that the sum with the frame covers [-0.1, 1.1] (both clamps), and a uint8 BGR frame."""
    rng = np.random.default_rng([H, W, s, cstride])
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    conv = rng.uniform(-0.6, 0.6, (H, W, cstride)).astype(np.float32)
    return conv, img
