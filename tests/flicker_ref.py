"""TEST INFRASTRUCTURE ONLY (imported by tests/ and nothing on the product path).

numpy restatement of the reference's Python flicker reduction, `FlickerReducer._apply_python_deflicker`
(src/framewright/processors/temporal_denoise.py:764-836), and of `FlickerReducer.reduce_flicker`'s result dict (:626-700) on that
path.  The reference's first choice, the external ffmpeg `deflicker` filter, is not restated.  OpenCV is not installed where this
is built and its source could not be consulted, so the two colour transforms are the sRGB / CIE Lab formulas in fixed point and
bit-parity with cv2.COLOR_BGR2LAB / COLOR_LAB2BGR is UNPINNED.  This file is the contract the device kernels (csrc/flicker.hip) are
held to, bit for bit: every step after the construction of the tables is integer arithmetic.

  * `bgr_to_lab_gamma` / `lab_to_bgr_gamma`: 8-bit sRGB BGR <-> Lab (D65, L * 255 / 100, a + 128, b + 128), integers over the
    tables of tests/nlmeans_ref.py plus `gamma_tables()`: a 256-entry sRGB decode to the 0 .. 65280 scale in front of the 2^20-row
    matrix (the rows sum to 2^20, so white still lands on the last f(t) entry), and behind the inverse matrix - kept at 16 bits,
    clamped - an sRGB encode table indexed by the 0 .. 65280 value (`encode_thresholds()` is the same map as 255 thresholds).
  * `bgr_to_lab_gamma_textbook` / `lab_to_bgr_gamma_textbook`: the formulas in float64, rounded; the integer forms stay within
    1 LSB of them.
  * `target_brightness`, `l_lut`, `python_deflicker`, `reduce_flicker`: the fallback itself.

A quirk of the reference, kept: the target is the median of mean GRAY levels (cv2.cvtColor BGR2GRAY) of the sampled frames, while
the value of each frame it is compared with is the mean of that frame's Lab L plane.  The two quantities differ (L is a
perceptual lightness, and gray of a mid-gray frame is not its L), so even a clip without flicker is shifted.
"""
import numpy as np

import nlmeans_ref as nr

LIN_MAX = 255 * 256                  # 65280: the scale of a decoded (linear) channel, and the last index of the f(t) table
LIN_SHIFT = nr.F_BITS + nr.INV_COEF_BITS - 8      # the inverse matrix carries x 255: 8 bits less of descale leave x 255 x 256


def _srgb_decode(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def _srgb_encode(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055)


def gamma_tables():
    """decode int32 [256]   round(65280 srgb_decode(v / 255)), half to even
       encode int32 [65281] round(255 srgb_encode(i / 65280)) - monotone, 0 .. 255"""
    dec = np.rint(LIN_MAX * _srgb_decode(np.arange(256, dtype=np.float64) / 255.0)).astype(np.int32)
    enc = np.rint(255.0 * _srgb_encode(np.arange(LIN_MAX + 1, dtype=np.float64) / float(LIN_MAX))).astype(np.int32)
    return {"decode": dec, "encode": enc}


_GAMMA = None


def _gamma():
    global _GAMMA
    if _GAMMA is None:
        _GAMMA = gamma_tables()
    return _GAMMA


def encode_thresholds() -> np.ndarray:
    """int32 [255]: thr[k] = the first index whose encode entry exceeds k.  encode[i] = the number of thresholds <= i."""
    enc = _gamma()["encode"]
    assert (np.diff(enc) >= 0).all() and enc[0] == 0 and enc[-1] == 255
    return np.searchsorted(enc, np.arange(1, 256), side="left").astype(np.int32)


def bgr_to_lab_gamma(bgr: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] sRGB BGR -> uint8 [..., 3] Lab, integers only."""
    t = nr._tables()
    v = _gamma()["decode"].astype(np.int64)[bgr]
    c = t["fwd_coef"].astype(np.int64)
    half = 1 << (nr.COEF_BITS - 1)
    idx = [(c[r, 0] * v[..., 0] + c[r, 1] * v[..., 1] + c[r, 2] * v[..., 2] + half) >> nr.COEF_BITS for r in range(3)]
    fx, fy, fz = (t["cbrt"][i].astype(np.int64) for i in idx)
    sh = nr.F_BITS + nr.L_SCALE_BITS
    L = (nr.L_SCALE * fy - nr.L_OFFSET + (1 << (sh - 1))) >> sh
    a = (500 * (fx - fy) + (128 << nr.F_BITS) + (1 << (nr.F_BITS - 1))) >> nr.F_BITS
    b = (200 * (fy - fz) + (128 << nr.F_BITS) + (1 << (nr.F_BITS - 1))) >> nr.F_BITS
    return np.clip(np.stack([L, a, b], axis=-1), 0, 255).astype(np.uint8)


def lab_to_bgr_gamma(lab: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] Lab -> uint8 [..., 3] sRGB BGR, integers only (int64 products)."""
    t = nr._tables()
    fy = t["fy"].astype(np.int64)[lab[..., 0]]
    Y = t["yl"].astype(np.int64)[lab[..., 0]]
    X = nr._inv_g(fy + t["ax"].astype(np.int64)[lab[..., 1]], t["inv_const"])
    Z = nr._inv_g(fy - t["bz"].astype(np.int64)[lab[..., 2]], t["inv_const"])
    k = t["inv_coef"].astype(np.int64)
    lin = [np.clip((k[r, 0] * X + k[r, 1] * Y + k[r, 2] * Z + (1 << (LIN_SHIFT - 1))) >> LIN_SHIFT, 0, LIN_MAX) for r in range(3)]
    return _gamma()["encode"][np.stack(lin, axis=-1)].astype(np.uint8)


def bgr_to_lab_gamma_textbook(bgr: np.ndarray) -> np.ndarray:
    """The formulas in float64, rounded and saturated."""
    v = _srgb_decode(bgr.astype(np.float64) / 255.0)
    B, G, R = v[..., 0], v[..., 1], v[..., 2]
    M = nr.RGB2XYZ
    X = (M[0, 0] * R + M[0, 1] * G + M[0, 2] * B) / nr.XN
    Y = M[1, 0] * R + M[1, 1] * G + M[1, 2] * B
    Z = (M[2, 0] * R + M[2, 1] * G + M[2, 2] * B) / nr.ZN
    fx, fy, fz = nr._lab_f(X), nr._lab_f(Y), nr._lab_f(Z)
    L = np.where(Y > nr.T0, 116.0 * fy - 16.0, 903.3 * Y)
    lab = np.stack([L * 255.0 / 100.0, 500.0 * (fx - fy) + 128.0, 200.0 * (fy - fz) + 128.0], axis=-1)
    return np.clip(np.rint(lab), 0, 255).astype(np.uint8)


def lab_to_bgr_gamma_textbook(lab: np.ndarray) -> np.ndarray:
    v = lab.astype(np.float64)
    L, a, b = v[..., 0] * 100.0 / 255.0, v[..., 1] - 128.0, v[..., 2] - 128.0
    y_low = L / 903.3
    fy = np.where(L <= nr.L_THRESH, 7.787 * y_low + 16.0 / 116.0, (L + 16.0) / 116.0)
    Y = np.where(L <= nr.L_THRESH, y_low, fy ** 3)
    g = lambda f: np.where(f <= nr.F_THRESH, (f - 16.0 / 116.0) / 7.787, f ** 3)
    X, Z = g(fy + a / 500.0) * nr.XN, g(fy - b / 200.0) * nr.ZN
    M = nr.XYZ2RGB
    rgb = [M[r, 0] * X + M[r, 1] * Y + M[r, 2] * Z for r in range(3)]
    lin = np.clip(np.stack(rgb[::-1], axis=-1), 0.0, 1.0)
    return np.clip(np.rint(_srgb_encode(lin) * 255.0), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the fallback
def gray(bgr: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(BGR2GRAY) on uint8: the 14-bit form of the clip analysis and the Farneback front end."""
    v = bgr.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def target_brightness(frames) -> float:
    """:806-814.  np.median of np.mean(gray) of frames[::10][:50]; the mean is the exact integer sum over N."""
    values = [int(gray(f).astype(np.int64).sum()) / (f.shape[0] * f.shape[1]) for f in list(frames)[::10][:50]]
    return np.median(values)


def l_lut(l_sum: int, n_pixels: int, target) -> np.ndarray:
    """:825-832 as the 256-byte map of a frame's L plane.  float64: `np.clip` of a float64 scalar is an np.float64, and under
    NumPy >= 2 a float32 array plus an np.float64 scalar is float64; astype(uint8) truncates."""
    adj = np.clip(target - int(l_sum) / int(n_pixels), -20, 20)
    return np.clip(np.arange(256, dtype=np.float64) + adj * 0.5, 0, 255).astype(np.uint8)


def python_deflicker(frames):
    """`_apply_python_deflicker` on a clip of uint8 BGR frames -> the list of deflickered frames."""
    frames = list(frames)
    target = target_brightness(frames)
    out = []
    for f in frames:
        lab = bgr_to_lab_gamma(f)
        lut = l_lut(int(lab[..., 0].astype(np.int64).sum()), f.shape[0] * f.shape[1], target)
        lab[..., 0] = lut[lab[..., 0]]
        out.append(lab_to_bgr_gamma(lab))
    return out


def resolve_mode(mode: str, detected_severity) -> str:
    """:660-668.  ADAPTIVE with a detected severity becomes light / medium / aggressive at 0.1 / 0.3."""
    if mode == "adaptive" and detected_severity is not None:
        return "light" if detected_severity < 0.1 else "medium" if detected_severity < 0.3 else "aggressive"
    return mode


def reduce_flicker(frames, mode: str = "adaptive", detected_severity=None):
    """`FlickerReducer.reduce_flicker` where ffmpeg's filter is unavailable -> (frames, result dict).  The mode changes no pixel
    on this path: it only chose the parameters of the ffmpeg filter."""
    frames = list(frames)
    if not frames:
        return [], {"frames_processed": 0, "mode_used": None}
    out = python_deflicker(frames)
    return out, {"success": True, "frames_processed": len(frames), "method": "python_brightness_normalization",
                 "mode_used": resolve_mode(mode, detected_severity)}


# ------------------------------------------------------------------------------------------------ the cases of the tests
def lattice() -> np.ndarray:
    """Every 5th level plus 255 per channel and the 256 grays, uint8 [N, 3].  0, 5, .. already ends on 255, which makes 52 levels;
    level 1 - the darkest step of the decode table, where it is coarsest - is added for the 53^3 colours the transforms are held on."""
    lv = np.array(sorted(set(range(0, 256, 5)) | {1, 255}), np.uint8)
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(-1, 3)
    grays = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    return np.ascontiguousarray(np.concatenate([grid, grays]))


# per-frame gains of `flicker_clip`: frames 0, 10 and 20 (what [::10] samples) are bright, the others flicker around a darker
# level, and a few are dark enough for the +-20 clamp
GAINS = (1.00, 0.62, 0.95, 0.55, 0.88, 0.30, 0.92, 0.58, 0.97, 0.50, 1.00, 0.66, 0.90, 0.35, 0.85, 0.60, 0.94, 0.52, 0.99, 0.25,
         1.00, 0.64, 0.91)


def flicker_clip(count: int = 23, height: int = 40, width: int = 56, seed: int = 5):
    """A synthetic scene under per-frame gains: `count` uint8 BGR frames."""
    from framewright_amd.synth import synthetic_frames
    base = synthetic_frames(1, height, width, seed=seed)[0].astype(np.float64)
    return [np.clip(np.rint(base * GAINS[i % len(GAINS)]), 0, 255).astype(np.uint8) for i in range(count)]
