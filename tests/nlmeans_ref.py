"""TEST INFRASTRUCTURE ONLY (imported by tests/ and nothing on the product path).

numpy restatement of the spatial step of the reference's classical temporal denoise, `_apply_spatial_denoise`
(src/framewright/processors/temporal_denoise.py:1611-1634): cv2.fastNlMeansDenoisingColored(frame, None, h, h, 7, 21) with
h = int(3 + strength * 7).  OpenCV is not installed where this is built and its source could not be consulted, so what follows is
OpenCV's 8-bit non-local-means algorithm AS RECALLED and bit-parity with cv2 is UNPINNED.  This file is the contract the device
kernels (csrc/nlmeans.hip) are held to, bit for bit: every step after the construction of the tables is integer arithmetic.

  * `nlmeans(plane, h, template, search)`: the core on a uint8 H x W x C plane (C = 1, 2, 3, pixels interleaved), running box sums;
    `nlmeans_literal` is the same definition as four nested loops with no running sums - a test holds the two equal.
  * `weight_table(h, channels, template, search)`: the fixed-point weights, built in float64.
  * `bgr_to_lab` / `lab_to_bgr`: 8-bit linear-BGR <-> Lab (COLOR_LBGR2Lab / COLOR_Lab2LBGR: no gamma, D65, L * 255 / 100,
    a + 128, b + 128) as integer arithmetic over tables built once in float64 (`lab_tables`); `bgr_to_lab_textbook` /
    `lab_to_bgr_textbook` evaluate the formulas in float64 - the integer forms stay within 1 LSB of those, rounded.
  * `nlmeans_colored(bgr, h, h_color, template, search)`: Lab split, the core on L (C = 1) and on ab (C = 2), merge, inverse.
"""
import math

import numpy as np

INT32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ the core
def windows(template: int, search: int):
    """(th, sh, template, search) with both windows forced odd, as cv2 does (2 * half + 1)."""
    th, sh = int(template) // 2, int(search) // 2
    return th, sh, 2 * th + 1, 2 * sh + 1


def table_constants(template: int, search: int):
    """(mult, shift, m): the fixed-point weight of distance 0, the shift that turns a patch distance into a table index
    (smallest p with 2^p >= template^2) and m = 2^shift / template^2, the distance one index step stands for."""
    _, _, t, s = windows(template, search)
    mult = min(INT32_MAX // (s * s * 255), INT32_MAX)
    shift = 0
    while (1 << shift) < t * t:
        shift += 1
    return mult, shift, float(1 << shift) / float(t * t)


def weight_table(h: float, channels: int, template: int = 7, search: int = 21) -> np.ndarray:
    """int32 [n], n = int(65025 C / m + 1): t[i] = round_half_even(mult * exp(-(i m) / (h h C))), 0 where that is below
    0.001 mult.  float64 throughout; math.exp is the C library's exp.  The weights fall monotonically, so everything behind the
    first zeroed entry is zero."""
    mult, _, m = table_constants(template, search)
    n = int(65025.0 * channels / m + 1)
    t = np.zeros(n, np.int32)
    den = float(h) * float(h) * float(channels)
    for i in range(n):
        v = float(np.rint(mult * math.exp(-(i * m) / den)))
        if v < 0.001 * mult:
            break
        t[i] = int(v)
    return t


def table_length(t: np.ndarray) -> int:
    """Length of the table truncated behind its last non-zero entry."""
    nz = np.flatnonzero(t)
    return int(nz[-1]) + 1 if nz.size else 0


def _extend(plane: np.ndarray, border: int) -> np.ndarray:
    if plane.dtype != np.uint8 or plane.ndim != 3 or plane.shape[2] not in (1, 2, 3):
        raise ValueError("nlmeans expects a uint8 H x W x C plane, C = 1, 2 or 3")
    if plane.shape[0] < 2 or plane.shape[1] < 2:
        raise ValueError("nlmeans: a side of 1 px cannot be extended by reflection")
    return np.pad(plane.astype(np.int64), ((border, border), (border, border), (0, 0)), mode="reflect")   # reflect-101, repeated


def nlmeans(plane: np.ndarray, h: float, template: int = 7, search: int = 21, return_counts: bool = False):
    """The core.  For each of the search^2 offsets: squared differences summed over the channels, 7 x 7 box sums of those (running
    sums), one table look-up, C multiply-adds.  With return_counts also the number of non-zero-weight offsets per pixel."""
    th, sh, t, s = windows(template, search)
    H, W, C = plane.shape
    ext = _extend(plane, th + sh)
    tab = weight_table(h, C, t, s).astype(np.int64)
    _, shift, _ = table_constants(t, s)
    est = np.zeros((H, W, C), np.int64)
    wsum = np.zeros((H, W), np.int64)
    counts = np.zeros((H, W), np.int64)
    b = th + sh
    own = ext[sh:sh + H + 2 * th, sh:sh + W + 2 * th]                  # the pixels and their template halo
    for oy in range(-sh, sh + 1):
        for ox in range(-sh, sh + 1):
            other = ext[sh + oy:sh + oy + H + 2 * th, sh + ox:sh + ox + W + 2 * th]
            d2 = ((own - other) ** 2).sum(axis=2)
            ii = np.zeros((d2.shape[0] + 1, d2.shape[1] + 1), np.int64)
            ii[1:, 1:] = d2.cumsum(0).cumsum(1)
            dist = ii[t:, t:] - ii[:-t, t:] - ii[t:, :-t] + ii[:-t, :-t]
            assert dist.max() <= INT32_MAX
            wgt = tab[dist >> shift]
            est += wgt[:, :, None] * ext[b + oy:b + oy + H, b + ox:b + ox + W]
            wsum += wgt
            counts += wgt > 0
    assert est.max() < 2 ** 32 and wsum.min() > 0
    out = ((est + (wsum // 2)[:, :, None]) // wsum[:, :, None]).astype(np.uint8)
    return (out, counts) if return_counts else out


def nlmeans_literal(plane: np.ndarray, h: float, template: int = 7, search: int = 21) -> np.ndarray:
    """The definition, slowly: per pixel, per offset, the patch distance summed term by term."""
    th, sh, t, s = windows(template, search)
    H, W, C = plane.shape
    b = th + sh
    ext = _extend(plane, b)
    tab = weight_table(h, C, t, s)
    _, shift, _ = table_constants(t, s)
    out = np.zeros((H, W, C), np.uint8)
    for y in range(H):
        for x in range(W):
            cy, cx = y + b, x + b
            patch = ext[cy - th:cy + th + 1, cx - th:cx + th + 1]
            est, wsum = [0] * C, 0
            for oy in range(-sh, sh + 1):
                for ox in range(-sh, sh + 1):
                    dist = 0
                    other = ext[cy + oy - th:cy + oy + th + 1, cx + ox - th:cx + ox + th + 1]
                    for v, u in zip(patch.reshape(-1).tolist(), other.reshape(-1).tolist()):
                        dist += (v - u) * (v - u)
                    wgt = int(tab[dist >> shift])
                    wsum += wgt
                    for c in range(C):
                        est[c] += wgt * int(ext[cy + oy, cx + ox, c])
            for c in range(C):
                out[y, x, c] = (est[c] + wsum // 2) // wsum
    return out


# ------------------------------------------------------------------------------------------------ linear BGR <-> Lab, 8 bit
XN, ZN = 0.950456, 1.088754                                             # D65 white point
RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
XYZ2RGB = np.array([[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
T0 = 0.008856                                                           # below it f(t) is the straight line 7.787 t + 16 / 116
F_THRESH = 7.787 * T0 + 16.0 / 116.0
L_THRESH = T0 * 903.3

CBRT_STEPS = 256                    # forward table: 256 steps per 8-bit level of the (normalised) X, Y, Z
CBRT_N = 255 * CBRT_STEPS + 1
COEF_BITS = 20                      # forward matrix rows, each summing to exactly 2^20 (white -> the last table entry)
F_BITS = 16                         # f(t), fy, a / 500, b / 200 and the inverse's X, Y, Z carry 16 fractional bits
INV_COEF_BITS = 14                  # inverse matrix x 255 x white point


def _lab_f(t):
    t = np.asarray(t, np.float64)
    return np.where(t > T0, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def lab_tables():
    """Every table and constant of the integer transforms, built in float64 and rounded half to even:
      cbrt     int32 [65281]  round(2^16 f(i / 65280))
      fwd_coef int32 [3][3]   rows X / Xn, Y, Z / Zn over (B, G, R), 2^20 scale, the largest entry adjusted so a row sums to 2^20
      fy, yl   int32 [256]    round(2^16 fy(L8)), round(2^16 Y(L8))
      ax, bz   int32 [256]    round(2^16 (a8 - 128) / 500), round(2^16 (b8 - 128) / 200)
      inv_coef int32 [3][3]   rows B, G, R over (X, Y, Z): round(2^14 255 M^-1 diag(Xn, 1, Zn))
      inv_const int32 [3]     round(2^16 F_THRESH), round(2^16 16 / 116), round(2^16 / 7.787)"""
    i = np.arange(CBRT_N, dtype=np.float64)
    cbrt = np.rint((1 << F_BITS) * _lab_f(i / float(CBRT_N - 1))).astype(np.int32)
    rows = RGB2XYZ / np.array([[XN], [1.0], [ZN]])
    rows = rows / rows.sum(axis=1, keepdims=True)
    fwd = np.rint(rows[:, ::-1] * (1 << COEF_BITS)).astype(np.int64)          # (B, G, R) order
    for r in range(3):
        fwd[r, int(np.argmax(fwd[r]))] += (1 << COEF_BITS) - fwd[r].sum()
    l8 = np.arange(256, dtype=np.float64)
    L = l8 * 100.0 / 255.0
    y_low = L / 903.3
    fy = np.where(L <= L_THRESH, 7.787 * y_low + 16.0 / 116.0, (L + 16.0) / 116.0)
    yl = np.where(L <= L_THRESH, y_low, fy * fy * fy)
    ab = np.arange(256, dtype=np.float64) - 128.0
    inv = XYZ2RGB[::-1] * np.array([[XN, 1.0, ZN]]) * 255.0 * (1 << INV_COEF_BITS)     # rows B, G, R
    return {
        "cbrt": cbrt,
        "fwd_coef": fwd.astype(np.int32),
        "fy": np.rint(fy * (1 << F_BITS)).astype(np.int32),
        "yl": np.rint(yl * (1 << F_BITS)).astype(np.int32),
        "ax": np.rint(ab / 500.0 * (1 << F_BITS)).astype(np.int32),
        "bz": np.rint(ab / 200.0 * (1 << F_BITS)).astype(np.int32),
        "inv_coef": np.rint(inv).astype(np.int32),
        "inv_const": np.array([np.rint(F_THRESH * (1 << F_BITS)), np.rint(16.0 / 116.0 * (1 << F_BITS)),
                               np.rint((1 << F_BITS) / 7.787)]).astype(np.int32),
    }


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = lab_tables()
    return _TABLES


L_SCALE_BITS = 6
L_SCALE = int(np.rint(116.0 * 2.55 * (1 << L_SCALE_BITS)))          # 18931
L_OFFSET = int(np.rint(16.0 * 2.55 * (1 << (F_BITS + L_SCALE_BITS))))


def bgr_to_lab(bgr: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] linear BGR -> uint8 [..., 3] Lab, integers only."""
    t = _tables()
    v = bgr.astype(np.int64)
    c = t["fwd_coef"].astype(np.int64)
    half = 1 << (COEF_BITS - 8 - 1)
    idx = [(c[r, 0] * v[..., 0] + c[r, 1] * v[..., 1] + c[r, 2] * v[..., 2] + half) >> (COEF_BITS - 8) for r in range(3)]
    fx, fy, fz = (t["cbrt"][i].astype(np.int64) for i in idx)
    sh = F_BITS + L_SCALE_BITS
    L = (L_SCALE * fy - L_OFFSET + (1 << (sh - 1))) >> sh
    a = (500 * (fx - fy) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS
    b = (200 * (fy - fz) + (128 << F_BITS) + (1 << (F_BITS - 1))) >> F_BITS
    return np.clip(np.stack([L, a, b], axis=-1), 0, 255).astype(np.uint8)


def _inv_g(t, consts):
    thr, c16, kinv = (int(x) for x in consts)
    cube = (t * t * t + (1 << (2 * F_BITS - 1))) >> (2 * F_BITS)
    line = ((t - c16) * kinv + (1 << (F_BITS - 1))) >> F_BITS
    return np.where(t > thr, cube, line)


def lab_to_bgr(lab: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] Lab -> uint8 [..., 3] linear BGR, integers only (int64 products)."""
    t = _tables()
    fy = t["fy"].astype(np.int64)[lab[..., 0]]
    Y = t["yl"].astype(np.int64)[lab[..., 0]]
    X = _inv_g(fy + t["ax"].astype(np.int64)[lab[..., 1]], t["inv_const"])
    Z = _inv_g(fy - t["bz"].astype(np.int64)[lab[..., 2]], t["inv_const"])
    k = t["inv_coef"].astype(np.int64)
    sh = F_BITS + INV_COEF_BITS
    out = [(k[r, 0] * X + k[r, 1] * Y + k[r, 2] * Z + (1 << (sh - 1))) >> sh for r in range(3)]
    return np.clip(np.stack(out, axis=-1), 0, 255).astype(np.uint8)


def bgr_to_lab_textbook(bgr: np.ndarray) -> np.ndarray:
    """The formulas in float64, rounded and saturated."""
    v = bgr.astype(np.float64) / 255.0
    B, G, R = v[..., 0], v[..., 1], v[..., 2]
    X = (RGB2XYZ[0, 0] * R + RGB2XYZ[0, 1] * G + RGB2XYZ[0, 2] * B) / XN
    Y = RGB2XYZ[1, 0] * R + RGB2XYZ[1, 1] * G + RGB2XYZ[1, 2] * B
    Z = (RGB2XYZ[2, 0] * R + RGB2XYZ[2, 1] * G + RGB2XYZ[2, 2] * B) / ZN
    fx, fy, fz = _lab_f(X), _lab_f(Y), _lab_f(Z)
    L = np.where(Y > T0, 116.0 * fy - 16.0, 903.3 * Y)
    lab = np.stack([L * 255.0 / 100.0, 500.0 * (fx - fy) + 128.0, 200.0 * (fy - fz) + 128.0], axis=-1)
    return np.clip(np.rint(lab), 0, 255).astype(np.uint8)


def lab_to_bgr_textbook(lab: np.ndarray) -> np.ndarray:
    v = lab.astype(np.float64)
    L, a, b = v[..., 0] * 100.0 / 255.0, v[..., 1] - 128.0, v[..., 2] - 128.0
    y_low = L / 903.3
    fy = np.where(L <= L_THRESH, 7.787 * y_low + 16.0 / 116.0, (L + 16.0) / 116.0)
    Y = np.where(L <= L_THRESH, y_low, fy ** 3)
    g = lambda f: np.where(f <= F_THRESH, (f - 16.0 / 116.0) / 7.787, f ** 3)
    X, Z = g(fy + a / 500.0) * XN, g(fy - b / 200.0) * ZN
    rgb = [XYZ2RGB[r, 0] * X + XYZ2RGB[r, 1] * Y + XYZ2RGB[r, 2] * Z for r in range(3)]
    return np.clip(np.rint(np.clip(np.stack(rgb[::-1], axis=-1), 0.0, 1.0) * 255.0), 0, 255).astype(np.uint8)


def nlmeans_colored(bgr: np.ndarray, h: float, h_color: float, template: int = 7, search: int = 21) -> np.ndarray:
    lab = bgr_to_lab(bgr)
    L = nlmeans(np.ascontiguousarray(lab[:, :, :1]), h, template, search)
    ab = nlmeans(np.ascontiguousarray(lab[:, :, 1:]), h_color, template, search)
    return lab_to_bgr(np.concatenate([L, ab], axis=2))


def h_for_strength(strength: float) -> int:
    """temporal_denoise.py:1627."""
    return int(3 + strength * 7)


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def noisy_pattern(height: int, width: int, channels: int, sigma: float, seed: int) -> np.ndarray:
    """A smooth pattern with a step edge plus seeded Gaussian noise, uint8 H x W x C."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    planes = []
    for c in range(channels):
        p = 120.0 + 40.0 * np.sin(xx / (9.0 + 2 * c) + 0.7 * c) * np.cos(yy / (7.0 + c)) + 0.4 * ((xx - yy) % 97.0)
        p += np.where(xx + 0.5 * yy > 0.6 * (width + 0.5 * height) - 5 * c, 45.0, 0.0)
        planes.append(p + rng.normal(0.0, sigma, p.shape))
    return np.clip(np.rint(np.stack(planes, axis=2)), 0, 255).astype(np.uint8)


def core_cases():
    """[(name, plane, h, template, search, exempt)]: what tests/test_nlmeans_gpu.py runs through fw_nlmeans_u8.  `exempt` marks the
    one deliberately degenerate case (sigma 25 at h = 5: the centre is the only offset with weight) that the liveliness condition
    of tests/test_nlmeans_ref_host.py does not apply to."""
    out = []
    for c in (1, 2, 3):
        for h in (5, 6, 10):
            out.append((f"s4_48x64_c{c}_h{h}", noisy_pattern(48, 64, c, 4.0, 10 * c + h), h, 7, 21, False))
    out.append(("s4_37x53_c1_h6", noisy_pattern(37, 53, 1, 4.0, 101), 6, 7, 21, False))
    out.append(("s4_37x53_c2_h5", noisy_pattern(37, 53, 2, 4.0, 102), 5, 7, 21, False))
    out.append(("s4_96x128_c2_h6", noisy_pattern(96, 128, 2, 4.0, 103), 6, 7, 21, False))
    out.append(("s4_96x128_c3_h10", noisy_pattern(96, 128, 3, 4.0, 104), 10, 7, 21, False))
    out.append(("s10_48x64_c1_h10", noisy_pattern(48, 64, 1, 10.0, 105), 10, 7, 21, False))
    out.append(("s4_9x70_c1_h6_short_side", noisy_pattern(9, 70, 1, 4.0, 106), 6, 7, 21, False))
    out.append(("s4_70x5_c2_h6_short_side", noisy_pattern(70, 5, 2, 4.0, 107), 6, 7, 21, False))
    out.append(("s4_64x1920_c1_h6_strip", noisy_pattern(64, 1920, 1, 4.0, 108), 6, 7, 21, False))
    out.append(("s4_48x64_c1_h6_w3_7", noisy_pattern(48, 64, 1, 4.0, 109), 6, 3, 7, False))
    out.append(("s4_37x53_c3_h10_w3_7", noisy_pattern(37, 53, 3, 4.0, 110), 10, 3, 7, False))
    out.append(("s4_48x64_c2_h6_w5_11", noisy_pattern(48, 64, 2, 4.0, 111), 6, 5, 11, False))
    out.append(("s25_48x64_c1_h5_degenerate", noisy_pattern(48, 64, 1, 25.0, 112), 5, 7, 21, True))
    return out


def colored_cases():
    """[(name, bgr frame, h, h_color)] for fw_nlmeans_colored_u8: frames of framewright_amd.synth.synthetic_frames."""
    from framewright_amd.synth import synthetic_frames
    a = synthetic_frames(2, 54, 70, seed=21)
    b = synthetic_frames(1, 40, 96, seed=22)
    return [("synthetic_54x70_h6_h6", np.ascontiguousarray(a[0]), 6, 6),
            ("synthetic_54x70_h10_h6", np.ascontiguousarray(a[1]), 10, 6),
            ("synthetic_40x96_h5_h10", np.ascontiguousarray(b[0]), 5, 10)]


def liveliness(plane: np.ndarray, h: float, template: int = 7, search: int = 21):
    """(fraction of pixels the restatement changes, mean number of non-zero-weight offsets per pixel)."""
    out, counts = nlmeans(plane, h, template, search, return_counts=True)
    return float((out != plane).any(axis=2).mean()), float(counts.mean())
