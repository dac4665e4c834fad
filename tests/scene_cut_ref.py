"""The contract of csrc/scene_cuts.hip: the scene-cut tests of `FrameInterpolator` (the reference's interpolation.py:267-366)
restated so that a device can hold them exactly.

SSIM of the mean-gray images (`policy.ssim_gray_u8`, skimage's structural_similarity with its defaults on uint8):
  * gray = (c0 + c1 + c2) // 3, which is `np.mean(img, axis=2).astype(np.uint8)` for all 766 sums (any channel order);
  * skimage crops (7 - 1) // 2 = 3 pixels from the SSIM map before the mean, so every 7 x 7 window that counts lies inside the
    image: N = (H - 6)(W - 6) values, the one at (i, j) over pixels [i, i + 7) x [j, j + 7), no border rule;
  * the five window sums Sx, Sy, Sxx, Syy, Sxy are integers (< 2^22), and so are the central moments
        mxx = 49 Sxx - Sx^2,  myy = 49 Syy - Sy^2,  mxy = 49 Sxy - Sx Sy   (|m| < 2^28, mxy signed):
    ux = Sx / 49, vx = cov_norm (uxx - ux^2) = mxx / (49 * 48), vxy = mxy / (49 * 48);
  * with numerator and denominator of skimage's S multiplied by 49^2 * (49 * 48),
        S = ((2 Sx Sy + K1) (2 mxy + K2)) / ((Sx^2 + Sy^2 + K1) (mxx + myy + K2)),   K1 = 2401 C1,  K2 = 2352 C2,
    where the four integers are exact.  Float64 enters here, in this order: c = 0.01 * 255.0, C1 = c * c, K1 = C1 * 2401.0 (and
    0.03, 2352.0 for K2); a1 = float(2 Sx Sy) + K1, a2 = float(2 mxy) + K2, b1 = float(Sx^2 + Sy^2) + K1,
    b2 = float(mxx + myy) + K2; S = (a1 * a2) / (b1 * b2): seven correctly rounded operations, |S| <= 1;
  * the result is math.fsum(S) / N: the exactly rounded sum, then one division.

Histogram fallback: hist[c][b] = how many bytes of channel c have value >> 2 == b, which is np.histogram(bins=64, range=(0, 256))
on uint8; the decision is `policy.scene_change_by_histogram`'s own float expression on those counts.
"""
import math

import numpy as np

WIN = 7
_c1 = 0.01 * 255.0
_c2 = 0.03 * 255.0
K1 = (_c1 * _c1) * 2401.0
K2 = (_c2 * _c2) * 2352.0


def mean_gray(img: np.ndarray) -> np.ndarray:
    """H x W x 3 uint8 -> H x W uint8, (c0 + c1 + c2) // 3."""
    return (img.astype(np.int64).sum(axis=2) // 3).astype(np.uint8)


def _window_sums(a: np.ndarray) -> np.ndarray:
    """int64 H x W -> (H - 6) x (W - 6): sums over [i, i + 7) x [j, j + 7), exact."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(axis=0).cumsum(axis=1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_map_gray(g1: np.ndarray, g2: np.ndarray) -> np.ndarray:
    """The (H - 6) x (W - 6) float64 map S of two H x W uint8 images, in the operation order of the module docstring."""
    if g1.shape != g2.shape or g1.ndim != 2 or min(g1.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    x, y = g1.astype(np.int64), g2.astype(np.int64)
    sx, sy, sxx, syy, sxy = (_window_sums(t) for t in (x, y, x * x, y * y, x * y))
    mxx, myy, mxy = 49 * sxx - sx * sx, 49 * syy - sy * sy, 49 * sxy - sx * sy
    a1 = (2 * sx * sy).astype(np.float64) + K1
    a2 = (2 * mxy).astype(np.float64) + K2
    b1 = (sx * sx + sy * sy).astype(np.float64) + K1
    b2 = (mxx + myy).astype(np.float64) + K2
    return (a1 * a2) / (b1 * b2)


def ssim_gray(g1: np.ndarray, g2: np.ndarray) -> float:
    s = ssim_map_gray(g1, g2)
    return math.fsum(s.ravel().tolist()) / s.size


def ssim_frames(a: np.ndarray, b: np.ndarray) -> float:
    """SSIM of the mean-gray images of two H x W x 3 uint8 frames."""
    return ssim_gray(mean_gray(a), mean_gray(b))


def hist64x3(img: np.ndarray) -> np.ndarray:
    """H x W x 3 uint8 -> int64 [3][64], hist[c][b] = #(img[:, :, c] >> 2 == b)."""
    return np.stack([np.bincount((img[:, :, c] >> 2).ravel(), minlength=64) for c in range(3)]).astype(np.int64)


def histogram_decision(h1: np.ndarray, h2: np.ndarray, scene_threshold: float = 0.3) -> bool:
    """`policy.scene_change_by_histogram` from the counts on: the two [3][64] tables concatenated channel by channel."""
    h1, h2 = np.asarray(h1).reshape(-1), np.asarray(h2).reshape(-1)
    h1 = h1.astype(float) / h1.sum()
    h2 = h2.astype(float) / h2.sum()
    return bool(np.minimum(h1, h2).sum() < (1.0 - scene_threshold))


def scene_change(a: np.ndarray, b: np.ndarray, scene_threshold: float = 0.3, use_ssim: bool = True) -> bool:
    """The control flow of `policy.scene_change`: the SSIM test, the histogram test when the SSIM cannot be formed."""
    if use_ssim and a.shape == b.shape and min(a.shape[:2]) >= WIN:
        return bool(ssim_frames(a, b) < (1.0 - scene_threshold))
    return histogram_decision(hist64x3(a), hist64x3(b), scene_threshold)


def detect_clip(frames, scene_threshold: float = 0.3):
    """Boundary indices i + 1 of the pairs (i, i + 1) that are cuts."""
    return [i + 1 for i in range(len(frames) - 1) if scene_change(frames[i], frames[i + 1], scene_threshold)]


# ---- the input kinds both test files use (H x W x 3 uint8 pairs) -------------------------------------------------------------
PAIR_KINDS = ["random", "noise3", "const255", "const0", "white_black", "complement", "gradient_shift"]


def make_pair(kind: str, h: int, w: int, seed: int = 0):
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    rnd = lambda: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "random":
        return rnd(), rnd()
    if kind == "noise3":                    # a frame against itself +- 3
        a = rnd()
        return a, np.clip(a.astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    if kind == "const255":                  # the window sums at their maximum; exactly 1.0
        a = np.full((h, w, 3), 255, np.uint8)
        return a, a.copy()
    if kind == "const0":
        a = np.zeros((h, w, 3), np.uint8)
        return a, a.copy()
    if kind == "white_black":
        return np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    if kind == "complement":                # negative covariance everywhere
        a = rnd()
        return a, 255 - a
    if kind == "gradient_shift":            # a gradient against its one-pixel shift
        ramp = (np.arange(w + 1)[None, :] * 5 + np.arange(h)[:, None] * 3) % 256
        g = np.repeat(ramp[:, :, None], 3, axis=2).astype(np.uint8)
        return np.ascontiguousarray(g[:, :w]), np.ascontiguousarray(g[:, 1:])
    raise ValueError(kind)
