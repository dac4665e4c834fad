"""TEST INFRASTRUCTURE ONLY (imported by tests/ and tools/gen_qp_artifact_golden.py, nothing on the product path).

numpy restatement of the classical frame path of the reference's `processors/qp_artifact_removal.py` (`backend == 'opencv'`):
`_remove_blocking_opencv`, `_remove_ringing_opencv`, `_remove_banding_opencv` and `_process_frame`.  It is the contract of
csrc/qp_artifacts.hip.  cv2 is not installed where this project is built, so every cv2 call is restated here from
its published algorithm and its bytes stay unpinned; what tests/golden/qp_artifact_reference.* pins is the reference's own glue
(dtype promotion, association of the products, order of the steps, strength, truncation), with these functions in cv2's place.

Canny, the 3 x 3 dilate, the float32 5-tap Gaussian and BGR2GRAY are oracle/temporal_ref.py's, by import.

Order of the float32 sums, stated once:
  * bilateral: one partial sum per window row, its taps added left to right from 0; the row sums are then added top to bottom
    onto 0.  The same for each of the four accumulators (b*w, g*w, r*w, w).  The centre tap is a tap like any other.
  * 15-tap Gaussian: acc = 0; acc += p[k] * c[k] for k = 0 .. 14 (left to right, then top to bottom), rows first, columns second.
"""
from __future__ import annotations

from statistics import NormalDist

import numpy as np

from oracle.temporal_ref import bgr2gray_u8, canny_u8, dilate3x3_u8, gaussian5_f32

f32, f64 = np.float32, np.float64
BLOCKING, RINGING, BANDING = "blocking", "ringing", "banding"
DEFAULT_QP = 28


def reflect101(p: np.ndarray, n: int) -> np.ndarray:
    """BORDER_REFLECT_101 of any index, reflected as often as it takes; a side of one pixel is that pixel."""
    p = np.asarray(p, dtype=np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - p - 2, p))


def pad101(a: np.ndarray, r: int) -> np.ndarray:
    """`a` with `r` reflected rows and columns on every side (axes 0 and 1)."""
    h, w = a.shape[:2]
    return a[reflect101(np.arange(-r, h + r), h)][:, reflect101(np.arange(-r, w + r), w)]


# ---- cv2.bilateralFilter on uint8 BGR ----------------------------------------------------------------------------------------------
def bilateral_radius(d: int) -> int:
    return max(int(d) // 2, 1)


def bilateral_tables(d: int, sigma_color: float, sigma_space: float):
    """(colour float32 [768], space float32 [2r+1][2r+1] with 0 outside the circular support), computed in float64."""
    r = bilateral_radius(d)
    k = np.arange(768, dtype=f64)
    color = np.exp(k * k * (-0.5 / (f64(sigma_color) * f64(sigma_color)))).astype(f32)
    i = np.arange(-r, r + 1, dtype=f64)
    rr = i[:, None] ** 2 + i[None, :] ** 2
    space = np.where(rr <= r * r, np.exp(rr * (-0.5 / (f64(sigma_space) * f64(sigma_space)))), 0.0).astype(f32)
    return color, space


def bilateral_u8c3(frame: np.ndarray, d: int, sigma_color: float, sigma_space: float) -> np.ndarray:
    r = bilateral_radius(d)
    color, space = bilateral_tables(d, sigma_color, sigma_space)
    h, w = frame.shape[:2]
    p = pad101(frame, r).astype(np.int32)
    c = frame.astype(np.int32)
    acc = np.zeros((h, w, 4), f32)                               # b*w, g*w, r*w, w
    for dy in range(-r, r + 1):
        row = np.zeros((h, w, 4), f32)
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx > r * r:
                continue
            q = p[r + dy:r + dy + h, r + dx:r + dx + w]
            wgt = f32(space[dy + r, dx + r]) * color[np.abs(q - c).sum(axis=2)]
            row[:, :, :3] += q.astype(f32) * wgt[:, :, None]
            row[:, :, 3] += wgt
        acc += row
    return np.rint(acc[:, :, :3] / acc[:, :, 3:4]).astype(np.uint8)


# ---- cv2.GaussianBlur(uint8, (5, 5), 0): exact fixed point -------------------------------------------------------------------------
def gaussian5_u8(frame: np.ndarray) -> np.ndarray:
    k = (1, 4, 6, 4, 1)
    h, w = frame.shape[:2]
    p = pad101(frame, 2).astype(np.int64)
    rows = sum(k[j] * p[:, j:j + w] for j in range(5))
    return ((sum(k[i] * rows[i:i + h] for i in range(5)) + 128) >> 8).astype(np.uint8)


# ---- the three removers ------------------------------------------------------------------------------------------------------------
def boundary_mask(h: int, w: int, block_size: int) -> np.ndarray:
    mask = np.zeros((h, w), f32)
    for y in range(0, h, block_size):
        mask[max(0, y - 1):min(h, y + 2), :] = 1.0
    for x in range(0, w, block_size):
        mask[:, max(0, x - 1):min(w, x + 2)] = 1.0
    return mask


def blocking_params(strength):
    """(d, sigma_color, sigma_space) of `_remove_blocking_opencv`."""
    return int(5 + strength * 10), 30 + strength * 70, 30 + strength * 70


def boundary_blend(result: np.ndarray, smooth: np.ndarray, mask: np.ndarray, strength) -> np.ndarray:
    """The reference's blend, its association and its promotions: float32 mask, float64 strength."""
    m = mask[:, :, None]
    strength = f64(strength)
    return (result * (1 - m * strength * 0.5) + smooth * m * strength * 0.5).astype(np.uint8)


def remove_blocking(frame: np.ndarray, strength, block_size: int = 8) -> np.ndarray:
    d, sc, ss = blocking_params(f64(strength))
    result = bilateral_u8c3(frame, d, sc, ss)
    if block_size > 0:
        h, w = frame.shape[:2]
        result = boundary_blend(result, gaussian5_u8(frame), boundary_mask(h, w, block_size), strength)
    return result


def ring_region(frame: np.ndarray):
    """(ring, edges): dilate(edges, 3 x 3, iterations 2) - edges, saturating."""
    edges = canny_u8(bgr2gray_u8(frame), 50, 150)
    dil = dilate3x3_u8(dilate3x3_u8(edges))
    return (dil.astype(np.int16) - edges).clip(0, 255).astype(np.uint8), edges


def remove_ringing(frame: np.ndarray, strength) -> np.ndarray:
    ring, _ = ring_region(frame)
    smoothed = gaussian5_u8(frame)
    ring_mask = gaussian5_f32((ring > 0).astype(f32))
    ring_mask = ring_mask[:, :, None] * f64(strength)
    return (frame * (1 - ring_mask) + smoothed * ring_mask).astype(np.uint8)


def gaussian15_coeffs() -> np.ndarray:
    """cv2.getGaussianKernel(15, 0) as float32: sigma 0.3 * ((15 - 1) * 0.5 - 1) + 0.8 = 2.6, float64, normalised, cast."""
    sigma = 0.3 * ((15 - 1) * 0.5 - 1) + 0.8
    x = np.arange(15, dtype=f64) - 7.0
    c = np.exp(-0.5 / (sigma * sigma) * x * x)
    return (c * (1.0 / c.sum())).astype(f32)


def gaussian15_f32(plane: np.ndarray) -> np.ndarray:
    c = gaussian15_coeffs()
    h, w = plane.shape
    p = pad101(plane.astype(f32), 7)
    rows = np.zeros((h + 14, w), f32)
    for k in range(15):
        rows += p[:, k:k + w] * c[k]
    out = np.zeros((h, w), f32)
    for k in range(15):
        out += rows[k:k + h] * c[k]
    return out


def laplacian3_f32(gray: np.ndarray) -> np.ndarray:
    """cv2.Laplacian(float32, CV_32F), ksize 1: [0 1 0; 1 -4 1; 0 1 0], REFLECT_101 (integers: exact in any order)."""
    h, w = gray.shape
    p = pad101(gray.astype(f32), 1)
    return (p[0:h, 1:1 + w] + p[2:2 + h, 1:1 + w] + p[1:1 + h, 0:w] + p[1:1 + h, 2:2 + w] - f32(4) * p[1:1 + h, 1:1 + w]).astype(f32)


def banding_mask(frame: np.ndarray) -> np.ndarray:
    gray = bgr2gray_u8(frame).astype(f32)
    variance = np.abs(laplacian3_f32(gray))
    mask = 1.0 - np.clip(variance / 30.0, 0, 1)
    assert mask.dtype == f32
    return gaussian15_f32(mask)


def remove_banding(frame: np.ndarray, strength, noise: np.ndarray) -> np.ndarray:
    """``noise``: the float32 H x W x 3 plane the reference draws with np.random.normal(0, 1 + strength * 2, shape)."""
    noise = np.asarray(noise)
    assert noise.dtype == f32 and noise.shape == frame.shape
    mask = banding_mask(frame)[:, :, None]
    result = frame.astype(f32) + noise * mask * f64(strength)
    return np.clip(result, 0, 255).astype(np.uint8)


# ---- the counter-based dither noise ------------------------------------------------------------------------------------------------
# 64-bit state from (seed, frame index), mixed; plus the element index pixel * 3 + channel, mixed again; the top 16 bits index a
# table of standard-normal quantiles at (k + 0.5) / 65536.  Integer arithmetic modulo 2^64 throughout (the splitmix64 finaliser).
# The table ends at +-4.32 sigma: the tails beyond are not drawn.
_MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def frame_key(seed: int, frame_index: int) -> int:
    """The mixed 64-bit key of one frame (a Python int; the device receives it as one uint64 argument)."""
    x = ((int(seed) & _MASK) * GOLDEN + (int(frame_index) & _MASK)) & _MASK
    return int(mix64(np.array([x], dtype=np.uint64))[0])


def noise_indices(seed: int, frame_index: int, count: int) -> np.ndarray:
    """The 16-bit table index of elements 0 .. count - 1 (element = pixel * 3 + channel)."""
    with np.errstate(over="ignore"):
        e = np.arange(count, dtype=np.uint64)
        return (mix64(np.uint64(frame_key(seed, frame_index)) + e) >> np.uint64(48)).astype(np.int64)


_QUANTILES = None


def normal_quantiles() -> np.ndarray:
    """float64 [65536]: the standard-normal quantile at (k + 0.5) / 65536."""
    global _QUANTILES
    if _QUANTILES is None:
        nd = NormalDist()
        _QUANTILES = np.array([nd.inv_cdf((k + 0.5) / 65536.0) for k in range(65536)], dtype=f64)
    return _QUANTILES


def noise_table(strength) -> np.ndarray:
    """float32 [65536]: the quantiles times the reference's standard deviation 1 + strength * 2."""
    return (normal_quantiles() * (1 + f64(strength) * 2)).astype(f32)


def counter_noise(shape, strength, seed: int, frame_index: int) -> np.ndarray:
    h, w, c = shape
    return noise_table(strength)[noise_indices(seed, frame_index, h * w * c)].reshape(h, w, c)


# ---- `_process_frame` --------------------------------------------------------------------------------------------------------------
def strength_for_qp(qp: int, strength_multiplier: float = 1.0):
    base = np.clip((qp - 15) / 35.0, 0.1, 1.0)
    return base * strength_multiplier


def type_names(artifact_types) -> list:
    names = [getattr(t, "value", t) for t in artifact_types]
    return [BLOCKING, RINGING, BANDING] if "all" in names else names


def process_frame(frame: np.ndarray, qp: int, config, noise) -> np.ndarray:
    """``config``: anything with `strength_multiplier`, `artifact_types` and `block_size`.  ``noise``: a float32 H x W x 3 plane, or
    (seed, frame index) for the counter generator; read only when banding is among the types."""
    strength = strength_for_qp(qp, config.strength_multiplier)
    types = type_names(config.artifact_types)
    result = frame.copy()
    if BLOCKING in types:
        result = remove_blocking(result, strength, config.block_size)
    if RINGING in types:
        result = remove_ringing(result, strength)
    if BANDING in types:
        if isinstance(noise, tuple):
            noise = counter_noise(frame.shape, strength, *noise)
        result = remove_banding(result, strength, noise)
    return result


# ---- test content --------------------------------------------------------------------------------------------------------------------
def content_frame(h: int, w: int, seed: int = 0) -> np.ndarray:
    """A deterministic uint8 BGR frame with what the three removers look for: a smooth ramp (banding), hard 8 x 8 blocks (blocking), a
    bright rectangle (strong edges, ringing) and a little grain.  Integer arithmetic and `noise_indices` only: no random generator."""
    y, x = np.mgrid[0:h, 0:w]
    ramp = x * 150 // max(w - 1, 1) + y * 50 // max(h - 1, 1)
    blocks = (x // 8 * 37 + y // 8 * 61 + seed * 13) % 48
    grain = (noise_indices(seed, 1 << 20, h * w * 3) >> 13).reshape(h, w, 3)                  # 0 .. 7
    f = ramp[:, :, None] + blocks[:, :, None] // 2 + grain - 4 + np.array([0, 9, 18])
    f[h // 4:max(h // 2, h // 4 + 1), w // 3:max(2 * w // 3, w // 3 + 1)] += 95
    return np.clip(f, 0, 255).astype(np.uint8)
