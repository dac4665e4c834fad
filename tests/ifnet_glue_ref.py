"""TEST INFRASTRUCTURE ONLY (never imported by the product): float64 restatements of the IFNet glue kernels of csrc/ifnet_ops.hip,
each with a per-element error bound, in plain vectorised numpy.  tests/test_ifnet_glue_ref_host.py pins these restatements to torch
in float64 (F.interpolate, F.grid_sample through oracle.ifnet_ref.warp, F.pixel_unshuffle, F.pixel_shuffle of conv_transpose2d,
torch.sigmoid); tests/test_ifnet_glue_gpu.py holds the kernels to them.  The arithmetic is IFNet_HDv3 v4.6 as restated in
oracle/ifnet_ref.py: **parity vs upstream (rife-ncnn-vulkan) stays unpinned** - nothing here or there pins a number of the upstream
binary.

Every function takes the kernel's own fp32 / uint8 inputs and evaluates in float64.  ``pts = (ys, xs)`` restricts the evaluation to
those output pixels (flat integer arrays; default: the whole output, row-major), so that a 4K frame can be checked on a sample of
rows and its borders.  Results are ``(N, C)`` arrays over the points.

Bounds.  u = 2^-24 is the unit roundoff of fp32 and gamma(k) = k u / (1 - k u) the usual bound of k chained roundings.  None of the
terms is fitted to what a kernel returns:

* arithmetic: ``gamma(k) * sum |tap * weight|`` with k the number of fp32 roundings on the longest path of the expression, counted
  from the kernel source without credit for operations that happen to be exact (a contracted multiply-add only removes roundings):
    - bilinear blend ``(p00 (1 - wx) + p01 wx) (1 - wy) + (p10 (1 - wx) + p11 wx) wy``: 1 - wx, product, sum, 1 - wy, product,
      sum: k = 6 (``K_BILIN``); resize_bilinear's ``* mul`` makes 7, as does the ``* fmul`` of stage_input's flow channels;
    - accumulate: the blend (6), ``* scale`` exact for the engine's power-of-two scales (asserted), the sum with the old value: 7;
    - u8_to_rgb: one division, correctly rounded: 1;
    - blend: m = 1 / (1 + expf(-mask)) carries expf's relative error times e / (1 + e), the sum and the division (2 roundings);
      v = a m + b (1 - m): the two warps' own bounds, |a| m and |b| m times m's relative error, 1 - m (1), product and sum (2);
    - stage_input: its X taps carry the warp bound, the resize 6 (7) more, then the cast.
  An absolute ``TINY`` = 8 * 2^-126 covers products that fall below the smallest normal fp32 (denormal or flushed).
* position (the warps): the kernel rounds the sample coordinate ``x + f`` to fp32 once: at most half an fp32 ulp of it per axis
  (after the border clamp: coordinates clamped on both sides do not move; none where the exact sum is an fp32 number).  The float64 bilinear surface moves by at most
  dx Sx + dy Sy + dx dy M: Sx = |p01 - p00| (1 - wy) + |p11 - p10| wy and Sy likewise are the local slopes, M = |p00 - p01 - p10 + p11|;
  where the half ulp reaches a neighbouring cell, that cell's larger edge difference and M enter the maxima.  The resizes carry no
  such term: for power-of-two scale factors ``(d + 0.5) / sf - 0.5`` is exact in fp32, which ``bilin_taps`` asserts.
* expf: the HIP math API's accuracy table is not part of the installed ROCm documentation, so the device expf was measured once on
  an MI355X against float64 over [-20, 20], the range of -mask here: see ``EXPF_ULP_MEASURED``; the bound uses twice that.
* typed outputs (f16 / bf16): the kernel's value is the RNE rounding of an fp32 value within the fp32 bound of the reference, so it
  lies within that bound plus half an ulp of the output type at |ref| + bound - one of the two neighbours where the bound
  straddles a rounding point (``typed_allowance``).
* uint8 output: ``rint(clamp(v) * 255)`` with one more rounding for the product.  With w = 255 (bound + u |v|) the result is
  rint(255 ref) exactly wherever 255 ref is farther than w from a half-integer, and one of the two neighbours inside that window
  (``u8_window``).  The share of elements inside the window is a property of the reference alone and must stay <= 0.5 %.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TINY = 8 * 2.0 ** -126
K_BILIN = 6
EXPF_ULP_MEASURED = 0.84    # max |expf(x) - exp(x)| / ulp(exp(x)) over 2^22 evenly spaced fp32 x of [-20, 20], one-kernel program on an MI355X: 0.8348 at x = 18.606
EXPF_REL = 2 * EXPF_ULP_MEASURED * 2.0 ** -23     # x2 margin; an ulp is at most 2^-23 relative
U8_WINDOW_SHARE = 0.005


def gamma(k: int) -> float:
    return k * U / (1 - k * U)


def _grid(H, W, pts):
    if pts is None:
        yy, xx = np.mgrid[0:H, 0:W]
        return yy.ravel(), xx.ravel()
    return np.asarray(pts[0]).ravel().astype(np.int64), np.asarray(pts[1]).ravel().astype(np.int64)


# ---- casts -----------------------------------------------------------------------------------------------------------------------
def to_bits(x, dtype: str) -> np.ndarray:
    """RNE rounding of fp32 values to f16 / bf16, as uint16 bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).view(np.uint16)
    b = x.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)          # finite inputs only


def from_bits(bits, dtype: str) -> np.ndarray:
    bits = np.ascontiguousarray(bits, np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def typed_ulp(x, dtype: str) -> np.ndarray:
    """Spacing of the output type at |x| (float64)."""
    mant, emin = (10, -14) if dtype == "f16" else (7, -126)
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)                               # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(x == 0, emin, np.maximum(e - 1, emin)) - mant)


def typed_allowance(ref, bound, dtype: str) -> np.ndarray:
    return bound + 0.5 * typed_ulp(np.abs(ref) + bound, dtype)


# ---- u8_to_rgb -------------------------------------------------------------------------------------------------------------------
def u8_to_rgb(img_bgr: np.ndarray, Hp: int, Wp: int):
    """uint8 BGR (H, W, 3) -> RGB / 255 on (Hp, Wp, 3), zero outside.  k = 1 (the division)."""
    H, W, _ = img_bgr.shape
    out = np.zeros((Hp, Wp, 3))
    out[:H, :W] = img_bgr[:, :, ::-1].astype(np.float64) / 255.0
    return out, gamma(1) * out


# ---- bilinear resize (align_corners=False) ---------------------------------------------------------------------------------------
def bilin_taps(d: np.ndarray, scale_factor: float, n: int):
    """torch's align_corners=False source index for output indices d: i0, i1, w1 - the same in fp32 as in float64, asserted."""
    inv = np.float32(1.0) / np.float32(scale_factor)
    s32 = np.maximum((d.astype(np.float32) + np.float32(0.5)) * inv - np.float32(0.5), np.float32(0))
    s = np.maximum((d.astype(np.float64) + 0.5) * (1.0 / float(scale_factor)) - 0.5, 0.0)
    assert np.array_equal(s32.astype(np.float64), s), "resize coordinates are not exact in fp32: a power-of-two scale factor is assumed"
    a = np.minimum(np.floor(s).astype(np.int64), n - 1)
    return a, np.minimum(a + 1, n - 1), s - a


def _blend4(fetch, ys0, ys1, wy, xs0, xs1, wx):
    """sum of the four taps: value, propagated input error, magnitude sum (|v| + e weighted)."""
    val = err = mag = 0.0
    for yy, a in ((ys0, 1.0 - wy), (ys1, wy)):
        for xx, b in ((xs0, 1.0 - wx), (xs1, wx)):
            v, e = fetch(yy, xx)
            w = (a * b)[:, None]
            val = val + w * v
            err = err + w * e
            mag = mag + w * (np.abs(v) + e)
    return val, err, mag


def resize_bilinear(src: np.ndarray, scale_factor: float, mul: float = 1.0, pts=None):
    """mul * F.interpolate(src, scale_factor, bilinear, align_corners=False) of src (Hs, Ws, C) fp32.  k = 7."""
    Hs, Ws, _ = src.shape
    Hd, Wd = int(Hs * scale_factor), int(Ws * scale_factor)
    ys, xs = _grid(Hd, Wd, pts)
    y0, y1, wy = bilin_taps(ys, scale_factor, Hs)
    x0, x1, wx = bilin_taps(xs, scale_factor, Ws)
    s64 = src.astype(np.float64)
    val, _, mag = _blend4(lambda yy, xx: (s64[yy, xx], 0.0), y0, y1, wy, x0, x1, wx)
    m = float(np.float32(mul))
    return val * m, gamma(K_BILIN + 1) * mag * abs(m) + TINY


# ---- backward warp (grid_sample bilinear / border / align_corners=True, flow in pixels) ------------------------------------------
def _coord(base, f, n):
    """Clamped float64 sample coordinate, its cell and weight, how far the kernel's fp32 coordinate can sit from it, and the cells
    that displacement reaches."""
    s = base.astype(np.float64) + f.astype(np.float64)
    half = 0.5 * np.spacing(np.abs(s).astype(np.float32)).astype(np.float64)
    half = np.where(s.astype(np.float32).astype(np.float64) == s, 0.0, half)     # the sum is an fp32 number: nothing to round
    sc = np.clip(s, 0.0, n - 1.0)
    lo, hi = np.clip(s - half, 0.0, n - 1.0), np.clip(s + half, 0.0, n - 1.0)
    d = np.maximum(sc - lo, hi - sc)
    top = max(n - 2, 0)
    cell = lambda v: np.clip(np.floor(v).astype(np.int64), 0, top)
    c0 = cell(sc)
    return sc, c0, sc - c0, d, (cell(lo), c0, cell(hi))


def warp(img: np.ndarray, fx: np.ndarray, fy: np.ndarray, ys: np.ndarray, xs: np.ndarray):
    """img (H, W, 3) fp32 sampled at (xs + fx, ys + fy) for the given points (fx, fy fp32 per point).  Returns (value, bound), (N, 3).
    k = 6 plus the position term."""
    H, W, _ = img.shape
    P = img.astype(np.float64)
    _, x0, wx, dx, xcells = _coord(xs, fx, W)
    _, y0, wy, dy, ycells = _coord(ys, fy, H)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    p00, p01, p10, p11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
    wxc, wyc = wx[:, None], wy[:, None]
    val = (p00 * (1 - wxc) + p01 * wxc) * (1 - wyc) + (p10 * (1 - wxc) + p11 * wxc) * wyc
    mag = (np.abs(p00) * (1 - wxc) + np.abs(p01) * wxc) * (1 - wyc) + (np.abs(p10) * (1 - wxc) + np.abs(p11) * wxc) * wyc
    Sx = np.abs(p01 - p00) * (1 - wyc) + np.abs(p11 - p10) * wyc
    Sy = np.abs(p10 - p00) * (1 - wxc) + np.abs(p11 - p01) * wxc
    M = np.abs(p00 - p01 - p10 + p11)
    for cy in ycells:
        for cx in xcells:
            other = (cy != y0) | (cx != x0)
            if not other.any():
                continue
            k = np.flatnonzero(other)
            yy, xx = cy[k], cx[k]
            yb, xb = np.minimum(yy + 1, H - 1), np.minimum(xx + 1, W - 1)
            a, b, c, d = P[yy, xx], P[yy, xb], P[yb, xx], P[yb, xb]
            Sx[k] = np.maximum(Sx[k], np.maximum(np.abs(b - a), np.abs(d - c)))
            Sy[k] = np.maximum(Sy[k], np.maximum(np.abs(c - a), np.abs(d - b)))
            M[k] = np.maximum(M[k], np.abs(a - b - c + d))
    pos = dx[:, None] * Sx + dy[:, None] * Sy + (dx * dy)[:, None] * M
    return val, gamma(K_BILIN) * mag + pos + TINY


def build_x(i0, i1, flow, mask, timestep: float, pts=None):
    """X = cat(warp(i0, flow[:2]), warp(i1, flow[2:4]), timestep, mask) (8 channels), or cat(i0, i1, timestep) (7) without flow.
    i0, i1 (H, W, 3), flow (H, W, 4), mask (H, W) fp32.  The copied channels are exact (bound 0)."""
    H, W, _ = i0.shape
    ys, xs = _grid(H, W, pts)
    t = float(np.float32(timestep))
    n = ys.size
    if flow is None:
        val = np.concatenate([i0[ys, xs].astype(np.float64), i1[ys, xs].astype(np.float64), np.full((n, 1), t)], 1)
        return val, np.zeros_like(val)
    f = flow[ys, xs]
    a, ea = warp(i0, f[:, 0], f[:, 1], ys, xs)
    b, eb = warp(i1, f[:, 2], f[:, 3], ys, xs)
    val = np.concatenate([a, b, np.full((n, 1), t), mask[ys, xs].astype(np.float64)[:, None]], 1)
    return val, np.concatenate([ea, eb, np.zeros((n, 2))], 1)


# ---- pixel (un)shuffle -----------------------------------------------------------------------------------------------------------
def unshuffle2(src: np.ndarray, C: int, cpad: int) -> np.ndarray:
    """src (h, w, >= C) -> (h / 2, w / 2, cpad): channel c * 4 + dy * 2 + dx, zero behind 4 C.  Values unchanged (the caller casts)."""
    h, w = src.shape[:2]
    out = np.zeros((h // 2, w // 2, cpad), src.dtype)
    v = src[:, :, :C].reshape(h // 2, 2, w // 2, 2, C).transpose(0, 2, 4, 1, 3)      # [y][x][c][dy][dx]
    out[:, :, :4 * C] = v.reshape(h // 2, w // 2, 4 * C)
    return out


def depth_to_space4(src: np.ndarray) -> np.ndarray:
    """src (h, w, >= 96), channel ((c6 * 4 + qy * 2 + qx) * 4 + py * 2 + px) -> (4 h, 4 w, 6) at (4 y + 2 py + qy, 4 x + 2 px + qx)."""
    h, w = src.shape[:2]
    v = src[:, :, :96].reshape(h, w, 6, 2, 2, 2, 2)                                   # [y][x][c6][qy][qx][py][px]
    return v.transpose(0, 5, 3, 1, 6, 4, 2).reshape(4 * h, 4 * w, 6)                   # [y][py][qy][x][px][qx][c6]


def tmp_to_t96(tmp: np.ndarray, cs: int = 96, fill: float = 0.0) -> np.ndarray:
    """The layout ifnet_accumulate_d2s_kernel reads: t96[Y >> 2][X >> 2][pos * 6 + c6] = tmp[Y][X][c6],
    pos = ((Y & 1) * 2 + (X & 1)) * 4 + ((Y >> 1) & 1) * 2 + ((X >> 1) & 1).  tmp (4 hf, 4 wf, 6)."""
    Hs, Ws, _ = tmp.shape
    out = np.full((Hs // 4, Ws // 4, cs), fill, tmp.dtype)
    Y, X = np.mgrid[0:Hs, 0:Ws]
    pos = ((Y & 1) * 2 + (X & 1)) * 4 + ((Y >> 1) & 1) * 2 + ((X >> 1) & 1)
    for c6 in range(6):
        out[Y >> 2, X >> 2, pos * 6 + c6] = tmp[:, :, c6]
    return out


def d2s_rows_to_t96(src: np.ndarray) -> np.ndarray:
    """The engine's row permutation of lastconv (fw_ifnet_finalize): row c6 * 16 + p of depth_to_space4's layout -> p * 6 + c6."""
    out = np.empty_like(src[:, :, :96])
    n = np.arange(96)
    out[:, :, (n % 16) * 6 + n // 16] = src[:, :, n]
    return out


# ---- accumulate ------------------------------------------------------------------------------------------------------------------
def accumulate(tmp, H: int, W: int, scale: float, flow, mask, first: bool, pts=None):
    """flow (+)= bilinear_up(tmp, scale)[:4] * scale, mask (+)= bilinear_up(tmp, scale)[4]; tmp (hs, ws, 6), flow (H, W, 4), mask (H, W)
    fp32 (ignored when first).  Returns (flow, flow bound (N, 4), mask, mask bound (N,)).  k = 7."""
    assert np.frexp(float(scale))[0] == 0.5, "* scale is exact for powers of two only"
    hs, ws, _ = tmp.shape
    ys, xs = _grid(H, W, pts)
    y0, y1, wy = bilin_taps(ys, scale, hs)
    x0, x1, wx = bilin_taps(xs, scale, ws)
    t64 = tmp.astype(np.float64)
    val, _, mag = _blend4(lambda yy, xx: (t64[yy, xx, :5], 0.0), y0, y1, wy, x0, x1, wx)
    of = np.zeros((ys.size, 4)) if first else flow[ys, xs].astype(np.float64)
    om = np.zeros(ys.size) if first else mask[ys, xs].astype(np.float64)
    g = gamma(K_BILIN + 1)
    return (of + val[:, :4] * scale, g * (np.abs(of) + mag[:, :4] * scale) + TINY,
            om + val[:, 4], g * (np.abs(om) + mag[:, 4]) + TINY)


# ---- an IFBlock's input ----------------------------------------------------------------------------------------------------------
def stage_input(i0, i1, flow, mask, timestep: float, s: int, cpad: int, pts=None):
    """What ifnet_ref.ifblock feeds conv0, pixel-unshuffled: cat(F.interpolate(X, 1 / s), F.interpolate(flow, 1 / s) / s) with X =
    build_x(...), on the (H / s / 2, W / s / 2) map with channel c * 4 + dy * 2 + dx, zeros behind 4 * 7 (first block: flow is None) or
    4 * 12.  Returns the value BEFORE the cast and its fp32 bound, (N, cpad); compare with ``typed_allowance``."""
    H, W, _ = i0.shape
    hs, ws = H // s, W // s
    cin = 7 if flow is None else 12
    yo, xo = _grid(hs // 2, ws // 2, pts)
    n = yo.size
    val, bnd = np.zeros((n, cpad)), np.zeros((n, cpad))
    f64 = None if flow is None else flow.astype(np.float64)
    fmul = float(np.float32(1.0) / np.float32(s))

    def fetch(yy, xx):
        v, e = build_x(i0, i1, flow, mask, timestep, (yy, xx))
        if flow is not None:
            v = np.concatenate([v, f64[yy, xx]], 1)
            e = np.concatenate([e, np.zeros((yy.size, 4))], 1)
        return v, e

    for sub in range(4):
        ys, xs = 2 * yo + (sub >> 1), 2 * xo + (sub & 1)
        y0, y1, wy = bilin_taps(ys, 1.0 / s, H)
        x0, x1, wx = bilin_taps(xs, 1.0 / s, W)
        v, e, mag = _blend4(fetch, y0, y1, wy, x0, x1, wx)
        b = e + gamma(K_BILIN) * mag
        if flow is not None:
            v[:, 8:] *= fmul
            b[:, 8:] = (e[:, 8:] + gamma(K_BILIN + 1) * mag[:, 8:]) * fmul
        val[:, sub:4 * cin:4] = v
        bnd[:, sub:4 * cin:4] = b + TINY
    return val, bnd


# ---- blend -----------------------------------------------------------------------------------------------------------------------
def sigmoid(mask):
    """1 / (1 + exp(-mask)) and the relative bound of the kernel's m = 1 / (1 + expf(-mask))."""
    e = np.exp(-mask.astype(np.float64))
    return 1.0 / (1.0 + e), (EXPF_REL * e / (1.0 + e) + gamma(2)) * (1 + 2.0 ** -20)     # the factor: second-order terms


def blend(i0, i1, flow, mask, H: int, W: int, pts=None):
    """warp(i0, flow[:2]) sigmoid(mask) + warp(i1, flow[2:4]) (1 - sigmoid(mask)) on the padded (Hp, Wp) inputs, for pixels of the
    H x W crop: un-clamped RGB (N, 3) and its bound."""
    ys, xs = _grid(H, W, pts)
    f = flow[ys, xs]
    a, ea = warp(i0, f[:, 0], f[:, 1], ys, xs)
    b, eb = warp(i1, f[:, 2], f[:, 3], ys, xs)
    m, rm = sigmoid(mask[ys, xs])
    m, rm = m[:, None], rm[:, None]
    em = m * rm                                    # |m_kernel - m|; 1 - m_kernel is off by that plus its own rounding
    e1 = em + U * (1 - m)
    val = a * m + b * (1 - m)
    A, B = np.abs(a) + ea, np.abs(b) + eb
    bound = ea * m + eb * (1 - m) + A * em + B * e1 + gamma(2) * (A * (m + em) + B * (1 - m + e1)) + TINY
    return val, bound


def u8_window(val, bound):
    """uint8 of rint(clamp(val, 0, 1) * 255): the smallest and largest value the bound admits (equal outside the window around a
    half-integer) and the share of elements for which they differ."""
    c = np.clip(val, 0.0, 1.0)
    w = 255.0 * (bound + U * c)
    lo, hi = np.rint(np.clip(255.0 * c - w, 0, 255)), np.rint(np.clip(255.0 * c + w, 0, 255))
    return lo.astype(np.int64), hi.astype(np.int64), float(np.mean(lo != hi))


# ---- seeded inputs shared by the host and the GPU tests --------------------------------------------------------------------------
IMAGE_KINDS = ("noise", "step")
FLOW_KINDS = ("smooth", "integer", "zero", "rand6", "huge", "edge")


def make_images(kind: str, H: int, W: int, rng):
    """Two fp32 images (H, W, 3) in [0, 1]: uniform noise, or a step edge along both axes (the largest slope a warp can meet)."""
    if kind == "noise":
        return rng.random((H, W, 3), np.float32), rng.random((H, W, 3), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    q = ((x >= W // 2) ^ (y >= H // 2)).astype(np.float32)[:, :, None]
    lvl = np.array([0.05, 0.11, 0.15], np.float32)       # levels whose 255-fold is not near a half-integer (the uint8 window)
    return lvl + np.float32(0.8) * q, np.float32(0.97) - lvl - np.float32(0.8) * q


def make_flow(kind: str, H: int, W: int, rng):
    """fp32 flow (H, W, 4): smooth sub-pixel, exact integers, zero, +-6 px noise, +-1e4 (both clamps), or landing exactly on the last
    column / row (first pair) and on column / row 0 or half a pixel inside the border (second pair)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "smooth":
        f = 0.45 * np.stack([np.sin(x / 7 + y / 11), np.cos(x / 5 - y / 9), np.sin(x / 13 + 1), np.cos(y / 6 + 2)], -1)
    elif kind == "integer":
        f = rng.integers(-3, 4, (H, W, 4)).astype(np.float64)
    elif kind == "zero":
        f = np.zeros((H, W, 4))
    elif kind == "rand6":
        f = rng.uniform(-6, 6, (H, W, 4))
    elif kind == "huge":
        f = rng.choice([-1e4, 1e4], (H, W, 4)) + rng.uniform(-1, 1, (H, W, 4))
    elif kind == "edge":
        half = rng.integers(0, 2, (H, W)) * 0.5
        f = np.stack([(W - 1) - x, (H - 1) - y, -x + half * (W > 1), (H - 1) - y - half * (H > 1)], -1)
    else:
        raise ValueError(kind)
    return f.astype(np.float32)


def make_mask(H: int, W: int, rng):
    """fp32 mask (H, W): moderate values, with one pixel in eight at +-20 where the sigmoid saturates."""
    m = rng.normal(0, 3, (H, W))
    sat = rng.random((H, W)) < 0.125
    return np.where(sat, rng.choice([-20.0, 20.0], (H, W)), np.clip(m, -20, 20)).astype(np.float32)


def sample_points(H: int, W: int, rng, rows: int = 24):
    """The points a large frame is checked at: a seeded sample of whole rows, the two outermost rows and columns on every side."""
    if H * W <= 1 << 18:
        return None
    ry = np.unique(np.concatenate([rng.integers(0, H, rows), [0, 1, H - 2, H - 1]]))
    yy, xx = np.meshgrid(ry, np.arange(W), indexing="ij")
    cx = np.array([0, 1, W - 2, W - 1])
    y2, x2 = np.meshgrid(np.arange(H), cx, indexing="ij")
    return np.concatenate([yy.ravel(), y2.ravel()]), np.concatenate([xx.ravel(), x2.ravel()])


def blend_cases(H: int, W: int):
    """(image kind, flow kind) pairs of the blend test at a frame size: every pair on small frames, the two hardest at 1080p."""
    if H * W > 1 << 18:
        return [("step", "rand6"), ("noise", "edge")]
    return [(i, f) for i in IMAGE_KINDS for f in FLOW_KINDS]


def blend_inputs(H: int, W: int, img_kind: str, flow_kind: str):
    """Padded (multiple of 32) images, flow and mask of a blend case, and the points of the H x W crop it is checked at."""
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    rng = np.random.default_rng([H, W, IMAGE_KINDS.index(img_kind), FLOW_KINDS.index(flow_kind)])
    i0, i1 = make_images(img_kind, Hp, Wp, rng)
    return i0, i1, make_flow(flow_kind, Hp, Wp, rng), make_mask(Hp, Wp, rng), sample_points(H, W, rng)
