"""TEST INFRASTRUCTURE ONLY (imported by tests/ and tools/gen_frame_generation_golden.py, nothing on the product path).

numpy restatement of the frame methods of the reference's `processors/frame_generation.py` (`MissingFrameGenerator`):
`detect_gaps`, `_generate_interpolated`, `_generate_optical_flow`, `_extrapolate_frames`, `_match_film_grain`, `_blend_edges`, and of the
driver that `generate_missing` evidently intends.  It is the contract of csrc/frame_generation.hip.  cv2 is not
installed where this project is built, so every cv2 call is restated from its published algorithm and its bytes stay unpinned:
  remap INTER_LINEAR  oracle/temporal_ref.py's fixed-point arithmetic, here with BORDER_REFLECT (`...cba|abc...`)
  addWeighted         tests/temporal_chain_ref.add_weighted
  Farneback           tests/farneback_ref.farneback (float32), poly_sigma 1.2; a test may hand in the flows of the device instead
  BGR2GRAY            oracle/temporal_ref.bgr2gray_u8
  GaussianBlur((0, 0), 2) on float32: ksize = cvRound(2 * 8 + 1) | 1 = 17, tests/farneback_ref.gaussian_taps(17, 2) (float64,
                      normalised, stored as float32), BORDER_REFLECT_101, rows then columns, acc = 0; acc += p[k] * c[k], k = 0 .. 16
What tests/golden/frame_generation_reference.* pins is the reference's own glue around them.

Randomness.  The reference draws from numpy's global generator.  Here a draw is an explicit plane or tests/qp_artifact_ref.py's
counter generator, keyed by (seed, 2 * generated frame number + tag): tag 0 the grain plane (one standard-normal float64 per pixel,
the same for the three channels), tag 1 the extrapolation noise (one float32 N(0, 2) per element pixel * 3 + channel).

The driver.  `generate_missing` calls `_blend_edges(generated, before or after, after)`, which raises on arrays; `fill_gap` passes
`before` where it exists and otherwise `after`, which is what the expression means for anything but an array.
"""
from __future__ import annotations

import re

import numpy as np

import farneback_ref as fr
from oracle import temporal_ref as oref
from qp_artifact_ref import noise_indices, normal_quantiles
from temporal_chain_ref import add_weighted

f32, f64 = np.float32, np.float64
TAG_GRAIN, TAG_EXTRAPOLATE = 0, 1
FARNEBACK = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
INTERPOLATE, OPTICAL_FLOW = "interpolate", "optical_flow"      # the reference's backends (SVD resolves to the first)


# ---- cv2.remap(INTER_LINEAR, BORDER_REFLECT) -----------------------------------------------------------------------------------------
def reflect(p: np.ndarray, n: int) -> np.ndarray:
    """BORDER_REFLECT (`...cba|abc...`) of any index, reflected as often as it takes."""
    p = np.asarray(p, dtype=np.int64).copy()
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p - 1, np.where(p >= n, 2 * n - 1 - p, p))


def remap_linear_reflect(frame, map_x, map_y):
    """oracle/temporal_ref.py's remap with `reflect` in the place of its border function: the arithmetic is that file's, unrestated."""
    saved = oref._reflect101
    oref._reflect101 = reflect
    try:
        return oref.remap_linear_reflect101(frame, map_x, map_y)
    finally:
        oref._reflect101 = saved


# ---- the generators ------------------------------------------------------------------------------------------------------------------
def generate_interpolated(before, after, num_frames: int) -> list:
    return [add_weighted(before, 1 - (i + 1) / (num_frames + 1), after, (i + 1) / (num_frames + 1)) for i in range(num_frames)]


def farneback_flow(a, b):
    """(flow_x, flow_y) float32 of cv2.calcOpticalFlowFarneback(gray(a), gray(b), None, 0.5, 3, 15, 3, 5, 1.2, 0)."""
    fx, fy = fr.farneback(oref.bgr2gray_u8(a), oref.bgr2gray_u8(b), f32, **FARNEBACK)
    return fx.astype(f32), fy.astype(f32)


def warp_blend(before, after, fwd, bwd, t):
    """One frame of `_generate_optical_flow`: fwd / bwd = (flow_x, flow_y) float32; t a Python float in (0, 1)."""
    h, w = before.shape[:2]
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    x, y = x.astype(f32), y.astype(f32)
    tx, ty = fwd[0] * t, fwd[1] * t                              # float32 array * Python float: rounded to float32
    assert tx.dtype == f32
    warped_before = remap_linear_reflect(before, x + tx, y + ty)
    bx, by = bwd[0] * (1 - t), bwd[1] * (1 - t)
    warped_after = remap_linear_reflect(after, x + bx, y + by)
    return add_weighted(warped_before, 1 - t, warped_after, t)


def generate_optical_flow(before, after, num_frames: int, flow=None) -> list:
    """``flow(a, b) -> (flow_x, flow_y)`` float32 replaces `farneback_flow` (a test hands in the device's flows)."""
    flow = flow or farneback_flow
    fwd, bwd = flow(before, after), flow(after, before)
    return [warp_blend(before, after, fwd, bwd, (i + 1) / (num_frames + 1)) for i in range(num_frames)]


def noise_index(number: int, tag: int) -> int:
    return 2 * int(number) + tag


def extrapolation_table() -> np.ndarray:
    """float32 [65536]: np.random.normal(0, 2, .).astype(float32) of the quantiles."""
    return (0.0 + 2.0 * normal_quantiles()).astype(f32)


def extrapolation_noise(shape, seed: int, number: int) -> np.ndarray:
    h, w, c = shape
    return extrapolation_table()[noise_indices(seed, noise_index(number, TAG_EXTRAPOLATE), h * w * c)].reshape(h, w, c)


def extrapolate_frame(reference, noise) -> np.ndarray:
    """One frame of `_extrapolate_frames`; ``noise``: the float32 plane of the reference's np.random.normal(0, 2, shape).astype."""
    assert noise.dtype == f32 and noise.shape == reference.shape
    frame = reference.astype(f32) + noise
    return np.clip(frame, 0, 255).astype(np.uint8)


# ---- `_match_film_grain` -------------------------------------------------------------------------------------------------------------
def gaussian17_coeffs() -> np.ndarray:
    return fr.gaussian_taps(17, 2.0)


def gaussian17_f32(plane: np.ndarray) -> np.ndarray:
    c = gaussian17_coeffs()
    h, w = plane.shape
    idx_y, idx_x = oref._reflect101(np.arange(-8, h + 8), h), oref._reflect101(np.arange(-8, w + 8), w)
    p = plane.astype(f32)[idx_y][:, idx_x]
    rows = np.zeros((h + 16, w), f32)
    for k in range(17):
        rows += p[:, k:k + w] * c[k]
    out = np.zeros((h, w), f32)
    for k in range(17):
        out += rows[k:k + h] * c[k]
    return out


def grain_plane(frame) -> np.ndarray:
    gray = oref.bgr2gray_u8(frame).astype(f32)
    return gray - gaussian17_f32(gray)


def grain_std64(frame) -> float:
    """The population standard deviation of the grain in float64 (np.std's two passes on the float64 copy)."""
    return float(np.std(grain_plane(frame).astype(f64)))


def grain_std(frame) -> np.float32:
    """The statistic as the contract has it: float64, rounded once to float32."""
    return f32(grain_std64(frame))


def grain_std_reference(frame) -> np.float32:
    """The reference's own np.std on the float32 grain (a float32 pairwise sum; not the contract, bounded against it)."""
    return np.std(grain_plane(frame))


def grain_draws(h: int, w: int, seed: int, number: int) -> np.ndarray:
    """float64 H x W standard-normal draws of the grain plane of generated frame ``number``."""
    return normal_quantiles()[noise_indices(seed, noise_index(number, TAG_GRAIN), h * w)].reshape(h, w)


def add_grain(generated, ref_std, cur_std, draws) -> np.ndarray:
    """`_match_film_grain` behind its two statistics (float32 scalars); ``draws``: float64 H x W standard-normal values, so the
    reference's np.random.normal(0, ref - cur, shape) is draws * float64(ref - cur)."""
    ref_std, cur_std = f32(ref_std), f32(cur_std)
    if cur_std > 0 and ref_std > cur_std:
        additional = 0.0 + f64(ref_std - cur_std) * draws
        grain_3ch = np.stack([additional] * 3, axis=-1)
        result = generated.astype(f32) + grain_3ch
        assert result.dtype == f64
        return np.clip(result, 0, 255).astype(np.uint8)
    return generated


def match_film_grain(generated, reference, draws, ref_std=None) -> np.ndarray:
    return add_grain(generated, grain_std(reference) if ref_std is None else ref_std, grain_std(generated), draws)


# ---- `_blend_edges` ------------------------------------------------------------------------------------------------------------------
def edge_blends(index: int, count: int, blend_edges: int, has_after: bool):
    """(alpha against `before` or None, alpha against `after` or None) of generated frame ``index`` of ``count``."""
    if blend_edges <= 0 or count == 0:
        return None, None
    n = min(blend_edges, count)
    j = count - 1 - index
    return ((index + 1) / (n + 1) if index < n else None), ((j + 1) / (n + 1) if has_after and j < n else None)


def blend_edges(generated: list, before, after, blend_edges_n: int) -> list:
    out = []
    for i, g in enumerate(generated):
        ab, aa = edge_blends(i, len(generated), blend_edges_n, after is not None)
        if ab is not None:
            g = add_weighted(before, 1 - ab, g, ab)
        if aa is not None:
            g = add_weighted(after, 1 - aa, g, aa)
        out.append(g)
    return out


def finish(generated, ref_std, cur_std, draws, before, alpha_before, after, alpha_after) -> np.ndarray:
    """What fw_framegen_finish_u8 does to one frame: the grain (ref_std None: off), then the two blends (alpha None: not due)."""
    g = generated if ref_std is None else add_grain(generated, ref_std, cur_std, draws)
    if alpha_before is not None:
        g = add_weighted(before, 1 - alpha_before, g, alpha_before)
    if alpha_after is not None:
        g = add_weighted(after, 1 - alpha_after, g, alpha_after)
    return g


# ---- `detect_gaps` -------------------------------------------------------------------------------------------------------------------
def parse_frame_number(filename: str):
    for pattern in (r"frame[_-]?(\d+)", r"^(\d+)\.", r"_(\d+)\."):
        m = re.search(pattern, filename, re.IGNORECASE)
        if m:
            return int(m.group(1))
    return None


def gaps_from_numbers(frame_numbers, expected_count=None, max_gap_frames: int = 10) -> list:
    """[(start_frame, end_frame, gap_size, has_after)]: the rule of `detect_gaps` on the parsed numbers."""
    nums = sorted(frame_numbers)
    gaps = []
    for cur, nxt in zip(nums, nums[1:]):
        if nxt - cur > 1 and nxt - cur - 1 <= max_gap_frames:
            gaps.append((cur, nxt, nxt - cur - 1, True))
    if expected_count and nums and nums[-1] < expected_count - 1 and expected_count - 1 - nums[-1] <= max_gap_frames:
        gaps.append((nums[-1], expected_count - 1, expected_count - 1 - nums[-1], False))
    return gaps


def detect_gaps(names, expected_count=None, max_gap_frames: int = 10) -> list:
    """``names``: the file names of a directory; `*.png` first, `*.jpg` only where there is no png."""
    names = sorted(names)
    files = [n for n in names if n.endswith(".png")] or [n for n in names if n.endswith(".jpg")]
    nums = [parse_frame_number(n) for n in files]
    return gaps_from_numbers([n for n in nums if n is not None], expected_count, max_gap_frames)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def fill_gap(before, after, start_frame: int, gap_size: int, backend: str = INTERPOLATE, match_grain: bool = True, blend_edges_n: int = 3,
             seed: int = 0, flow=None) -> list:
    """The generated frames start_frame + 1 .. start_frame + gap_size of one gap; ``before`` or ``after`` may be None (not both)."""
    numbers = [start_frame + 1 + i for i in range(gap_size)]
    if before is not None and after is not None:
        generated = generate_optical_flow(before, after, gap_size, flow) if backend == OPTICAL_FLOW else \
            generate_interpolated(before, after, gap_size)
    else:
        # backward extrapolation reverses the list of its draws: keyed by frame number, the order of the draws does not matter
        source = before if before is not None else after
        generated = [extrapolate_frame(source, extrapolation_noise(source.shape, seed, n)) for n in numbers]
    reference = before if before is not None else after
    if match_grain:
        ref_std = grain_std(reference)                         # once a gap
        h, w = reference.shape[:2]
        generated = [match_film_grain(g, reference, grain_draws(h, w, seed, n), ref_std) for g, n in zip(generated, numbers)]
    return blend_edges(generated, reference, after, blend_edges_n)


def fill(frames, frame_numbers, expected_count=None, backend: str = INTERPOLATE, max_gap_frames: int = 10, match_grain: bool = True,
         blend_edges_n: int = 3, seed: int = 0, flow=None):
    """(frames, frame_numbers) with every fillable gap filled; the numbers must rise strictly."""
    frames, nums = list(frames), [int(n) for n in frame_numbers]
    assert len(frames) == len(nums) and all(a < b for a, b in zip(nums, nums[1:]))
    at = {n: f for n, f in zip(nums, frames)}
    for start, end, size, has_after in gaps_from_numbers(nums, expected_count, max_gap_frames):
        made = fill_gap(at[start], at[end] if has_after else None, start, size, backend, match_grain, blend_edges_n, seed, flow)
        at.update({start + 1 + i: g for i, g in enumerate(made)})
    order = sorted(at)
    return [at[n] for n in order], order


# ---- the tolerance of the one float64 reduction --------------------------------------------------------------------------------------
U64, U32 = 2.0 ** -53, 2.0 ** -24


def std_epsilon(grain: np.ndarray) -> float:
    """The relative distance within which the device's float64 deviation and this file's may differ: both sum N exact
    terms in some order.  var = S2 / N - (S1 / N)^2 with |dS2| <= (N - 1) u S2, |dS1| <= (N - 1) u sum|x| <= (N - 1) u N sqrt(m2),
    m2 = S2 / N, and |mean| <= sqrt(m2), gives |d var| <= (3 N + 8) u m2 with the last roundings; a deviation is half of that relative
    to the variance, plus the root's rounding; twice, for the two sides."""
    g = grain.astype(f64)
    n, m2, var = g.size, float(np.mean(g * g)), float(np.var(g))
    return 2 * (0.5 * (3 * n + 8) * U64 * (m2 / var) + U64) if var > 0 else float("inf")


def clear_of_rounding_boundary(value64: float, eps_rel: float) -> bool:
    """True where no float64 within eps_rel of ``value64`` rounds to another float32 than it does."""
    lo, hi = value64 * (1 - eps_rel), value64 * (1 + eps_rel)
    return f32(lo) == f32(hi) == f32(value64)


def std_f32_ulp_bound(n: int) -> int:
    """float32 ulps between np.std of a float32 array of n elements and the float64 value rounded once.  numpy: mean by pairwise
    sums (blocks of 128 in 8 accumulators: 16 additions deep, then log2(n / 128) levels), x - mean (1 rounding; the error of the mean
    enters in second order, counted as 1), the square (1), the pairwise sum again (K), the division (1), then the root, which halves
    the relative error and rounds once; the contract's own rounding is half an ulp.  A relative error of 2^-24 is at most 1 ulp."""
    k = 16 + max(int(np.ceil(np.log2(max(n, 128) / 128))), 0)
    return int(np.ceil(0.5 * (1 + 1 + 1 + k + 1) + 1 + 0.5))


def ulps_apart(a, b) -> int:
    a, b = f32(a), f32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


# ---- test content --------------------------------------------------------------------------------------------------------------------
def grainy_frame(h: int, w: int, seed: int, grain: int = 6, shift: int = 0) -> np.ndarray:
    """A deterministic uint8 BGR frame: a smooth two-way ramp and a bright block, moved ``shift`` pixels to the right, under integer
    grain of amplitude ``grain`` (`noise_indices` only: no random generator)."""
    y, x = np.mgrid[0:h, 0:w]
    x = x - shift
    base = 40 + x * 120 // max(w - 1, 1) + y * 60 // max(h - 1, 1)
    base = base + 50 * ((x > w // 3) & (x < 2 * w // 3) & (y > h // 4) & (y < 3 * h // 4))
    g = (noise_indices(seed, 1 << 21, h * w * 3) % (2 * grain + 1)).reshape(h, w, 3) - grain if grain else 0
    return np.clip(base[:, :, None] + np.array([0, 7, 14]) + g, 0, 255).astype(np.uint8)
