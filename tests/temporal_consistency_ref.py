"""NumPy restatement of the classical path of the reference's `processors/cross_attention_temporal.py`
(`CrossAttentionTemporalProcessor`, :347-429 and :508-651): the contract of csrc/temporal_consistency.hip and of
`framewright_amd.temporal_consistency`, byte for byte.

cv2 is absent where this is built and stays unpinned, as everywhere in this project: `cvtColor(BGR2GRAY)` is
`farneback_ref.bgr2gray_u8`, `GaussianBlur` is `farneback_ref.gaussian_blur`, `calcHist` is `quality_ref.calc_hist`, `absdiff` is
`quality_ref.absdiff`, and `compareHist(HISTCMP_CORREL)` is `compare_hist_correl` below.  tools/gen_temporal_consistency_golden.py
runs the reference's own methods on these stand-ins and asserts that the functions here return the same arrays.

The frame functions are the reference's own operations in its order.  Every float step is one float32 operation, rounded once:
x / 255, 1 - nb, min(dp, dn) * (1 - nb), mask * float32(blend_strength), 1 - m3, cur * (1 - m3), blend * m3, their sum.  Python floats
are weak scalars, so the threshold and the strength enter as float32.

The integer form (`binary_mask`, `blur_k`, `area_numerator`) is what the device computes: the blurred mask of a 0 / 1 plane under the
table 1/16, 4/16, 6/16, 4/16, 1/16 is k / 256 with an integer k in 0 .. 256, and every product and sum of the float32 blur is exact (the
partial sums are multiples of 1 / 256 below 2), so the blur is independent of its summation order.

The area decision.  The reference decides `np.mean(mask) > 0.01`: a float32 pairwise sum, one division by the pixel count, and a
comparison with float32(0.01).  For a frame of up to 2^16 pixels every partial sum is a multiple of 1 / 256 of at most 2^16, which
float32 holds exactly, so the sum is S / 256 exactly and `area_decision` - float32(S / 256) / float32(n) > float32(0.01) - IS the
reference's decision.  For a larger frame the pairwise sum rounds: an element passes through at most `pairwise_depth(n)` additions
(15 within one of the eight accumulators of a 128-element block, 3 to join them, one per halving above), each with a relative error of
at most 2^-24 of a partial sum that is no larger than the total, so the reference's sum is within depth * 2^-24 (1 + 2^-20) of S / 256
relatively; its division and the two roundings of `area_decision` add three more.  `area_guard(n)` is that distance, relative to
float32(0.01): outside it both decisions are the exact one; every golden and test case stays outside it.
"""
from __future__ import annotations

import numpy as np

import farneback_ref as fr
from quality_ref import absdiff, calc_hist

OPTICAL_FLOW, CROSS_ATTENTION, HYBRID = "optical_flow", "cross_attention", "hybrid"
AREA_THRESHOLD = 0.01                                   # `flicker_area > 0.01`
DBL_EPSILON = float(np.finfo(np.float64).eps)


# ---- `_detect_scene_change` ----------------------------------------------------------------------------------------------------------
def gray_hist(frame: np.ndarray) -> np.ndarray:
    """The 256 integer counts of calcHist on the gray frame (what fw_tcons_gray_hist_u8 returns)."""
    return np.bincount(fr.bgr2gray_u8(frame).reshape(-1), minlength=256).astype(np.int64)


def normalized_hist(counts: np.ndarray) -> np.ndarray:
    """calcHist's float32 (256, 1) array over its own float32 sum."""
    hist = np.asarray(counts).astype(np.float32).reshape(256, 1)
    return hist / hist.sum()


def compare_hist_correl(h1: np.ndarray, h2: np.ndarray) -> float:
    """cv2.compareHist(HISTCMP_CORREL): the five sums over the bins in double, in bin order."""
    a, b = np.asarray(h1, np.float64).reshape(-1), np.asarray(h2, np.float64).reshape(-1)
    n = float(a.size)
    s1, s2, s11, s12, s22 = (float(np.cumsum(v)[-1]) for v in (a, b, a * a, a * b, b * b))
    num = s12 - s1 * s2 / n
    den2 = (s11 - s1 * s1 / n) * (s22 - s2 * s2 / n)
    return num / float(np.sqrt(den2)) if abs(den2) > DBL_EPSILON else 1.0


def hist_correlation(counts1: np.ndarray, counts2: np.ndarray) -> float:
    return compare_hist_correl(normalized_hist(counts1), normalized_hist(counts2))


def scene_correlation(f1: np.ndarray, f2: np.ndarray) -> float:
    """`_detect_scene_change` up to its comparison, as the reference writes it."""
    hist1, hist2 = calc_hist(fr.bgr2gray_u8(f1)), calc_hist(fr.bgr2gray_u8(f2))
    hist1 = hist1 / hist1.sum()
    hist2 = hist2 / hist2.sum()
    return compare_hist_correl(hist1, hist2)


def detect_scene_change(f1: np.ndarray, f2: np.ndarray, scene_change_threshold: float = 0.3) -> bool:
    return bool(scene_correlation(f1, f2) < scene_change_threshold)


def scene_changes(frames, scene_change_threshold: float = 0.3) -> list:
    """`apply_consistency`'s list: every i in 1 .. n - 1 whose pair (i - 1, i) is a cut; a pair with a None frame is skipped."""
    return [i for i in range(1, len(frames)) if frames[i] is not None and frames[i - 1] is not None and
            detect_scene_change(frames[i - 1], frames[i], scene_change_threshold)]


# ---- `_detect_flicker` ---------------------------------------------------------------------------------------------------------------
def flicker_score(prev: np.ndarray, cur: np.ndarray, nxt: np.ndarray) -> np.ndarray:
    gray_dp = fr.bgr2gray_u8(absdiff(cur, prev)).astype(np.float32) / 255
    gray_dn = fr.bgr2gray_u8(absdiff(cur, nxt)).astype(np.float32) / 255
    gray_nb = fr.bgr2gray_u8(absdiff(prev, nxt)).astype(np.float32) / 255
    return np.minimum(gray_dp, gray_dn) * (1 - gray_nb)


def detect_flicker(prev: np.ndarray, cur: np.ndarray, nxt: np.ndarray, flicker_threshold: float = 0.02) -> np.ndarray:
    mask = (flicker_score(prev, cur, nxt) > flicker_threshold).astype(np.float32)
    return fr.gaussian_blur(mask, 5, 0, np.float32)


# ---- the integer form ----------------------------------------------------------------------------------------------------------------
def binary_mask(prev: np.ndarray, cur: np.ndarray, nxt: np.ndarray, flicker_threshold: float = 0.02) -> np.ndarray:
    return (flicker_score(prev, cur, nxt) > np.float32(flicker_threshold)).astype(np.uint8)


def blur_k(binary: np.ndarray) -> np.ndarray:
    """256 x GaussianBlur(binary, (5, 5), 0) with BORDER_REFLECT_101, in integers: rows, then columns, taps 1 4 6 4 1."""
    taps = (1, 4, 6, 4, 1)
    h, w = binary.shape
    p = np.pad(binary.astype(np.int64), ((0, 0), (2, 2)), mode="reflect")
    rows = sum(t * p[:, i:i + w] for i, t in enumerate(taps))
    p = np.pad(rows, ((2, 2), (0, 0)), mode="reflect")
    return sum(t * p[i:i + h] for i, t in enumerate(taps))


def mask_from_k(k: np.ndarray) -> np.ndarray:
    return (k.astype(np.float32) / np.float32(256))


def area_numerator(k: np.ndarray) -> int:
    """S = sum k: the reference's np.mean(mask) is S / (256 n)."""
    return int(k.sum())


def area_value(s: int, n: int) -> np.float32:
    return np.float32(s / 256.0) / np.float32(n)


def area_decision(s: int, n: int) -> bool:
    """`np.mean(mask) > 0.01` from the integer S, as the installed NumPy evaluates it for n <= 2^16 (the module docstring)."""
    return bool(area_value(s, n) > np.float32(AREA_THRESHOLD))


def reference_area_decision(mask: np.ndarray) -> bool:
    """The reference's own expression."""
    return bool(np.mean(mask) > 0.01)


def pairwise_depth(n: int) -> int:
    """An upper bound of the additions an element of a float32 np.sum over n elements passes through."""
    return 18 + max(0, int(np.ceil(np.log2(max(n, 1) / 128.0))))


def area_guard(n: int) -> float:
    """The relative distance from float32(0.01) outside which `area_decision` and the reference's decision are both the exact one;
    0 for n <= 2^16, where they are the same expression."""
    return 0.0 if n <= (1 << 16) else (pairwise_depth(n) + 3) * 2.0 ** -24 * (1 + 2.0 ** -20)


def area_distance(s: int, n: int) -> float:
    """|exact area / float32(0.01) - 1|."""
    return abs((s / 256.0 / n) / float(np.float32(AREA_THRESHOLD)) - 1.0)


# ---- `_apply_optical_flow_consistency`, `_apply_hybrid_consistency` ------------------------------------------------------------------
def neighbours(n: int, i: int) -> tuple:
    return max(0, i - 1), min(n - 1, i + 1)


def blend_frame(prev: np.ndarray, cur: np.ndarray, nxt: np.ndarray, mask: np.ndarray, blend_strength: float) -> np.ndarray:
    blend = (prev.astype(np.float32) + nxt.astype(np.float32)) / 2
    mask_3ch = mask[:, :, np.newaxis] * blend_strength
    result = cur.astype(np.float32) * (1 - mask_3ch) + blend * mask_3ch
    return result.astype(np.uint8)


def apply_optical_flow(frames, i: int, flicker_threshold: float = 0.02, blend_strength: float = 0.8) -> np.ndarray:
    center = frames[i]
    if len(frames) < 3:
        return center
    p, n = neighbours(len(frames), i)
    mask = detect_flicker(frames[p], center, frames[n], flicker_threshold)
    return blend_frame(frames[p], center, frames[n], mask, blend_strength)


def add_weighted(a: np.ndarray, alpha: float, b: np.ndarray, beta: float) -> np.ndarray:
    """cv2.addWeighted(a, alpha, b, beta, 0) as fw_add_weighted_u8 defines it (tests/temporal_chain_ref.add_weighted)."""
    from temporal_chain_ref import add_weighted as aw
    return aw(a, alpha, b, beta)


def apply_hybrid(frames, i: int, flicker_threshold: float = 0.02, blend_strength: float = 0.8, attention_fn=None, called=None) -> np.ndarray:
    """`_apply_hybrid_consistency`; ``attention_fn(frames, i) -> frame`` stands where the network stands (None: the backend
    'optical_flow'), followed by the addWeighted of `_apply_cross_attention_consistency`.  ``called``: a list that collects i."""
    p, n = neighbours(len(frames), i)
    k = blur_k(binary_mask(frames[p], frames[i], frames[n], flicker_threshold))
    if attention_fn is not None and area_decision(area_numerator(k), k.size):
        if called is not None:
            called.append(i)
        output = attention_fn(frames, i)
        if blend_strength < 1.0:
            output = add_weighted(frames[i], 1 - blend_strength, output, blend_strength)
        return output
    return apply_optical_flow(frames, i, flicker_threshold, blend_strength)


# ---- `apply_consistency` on a clip in memory -----------------------------------------------------------------------------------------
def in_cut_window(i: int, cuts, attention_window: int) -> bool:
    return any(abs(i - sc) <= attention_window // 2 for sc in cuts)


def apply_clip(frames, method: str = HYBRID, attention_window: int = 7, flicker_threshold: float = 0.02, blend_strength: float = 0.8,
               scene_change_threshold: float = 0.3, attention_fn=None, called=None, cuts=None) -> tuple:
    """(output frames, cuts): a frame inside a cut's window is the input array itself."""
    cuts = scene_changes(frames, scene_change_threshold) if cuts is None else list(cuts)
    out = [frames[i] if in_cut_window(i, cuts, attention_window) else
           apply_frame(frames, i, method, flicker_threshold, blend_strength, attention_fn, called) for i in range(len(frames))]
    return out, cuts


def apply_frame(frames, i: int, method: str = HYBRID, flicker_threshold: float = 0.02, blend_strength: float = 0.8, attention_fn=None,
                called=None) -> np.ndarray:
    """The configured method on frame i, as `apply_consistency` dispatches it outside a cut's window."""
    if method == OPTICAL_FLOW:
        return apply_optical_flow(frames, i, flicker_threshold, blend_strength)
    return apply_hybrid(frames, i, flicker_threshold, blend_strength, attention_fn, called)


def stream_hold_back(attention_window: int) -> int:
    """Frames a stream is behind its input: frame i needs the cuts up to i + window // 2 and its next neighbour."""
    return attention_window // 2 + 1


def stream_clip(frames, method: str = HYBRID, attention_window: int = 7, flicker_threshold: float = 0.02, blend_strength: float = 0.8,
                scene_change_threshold: float = 0.3, attention_fn=None, called=None) -> list:
    """The streaming order on a clip in memory: frame i leaves when frame i + `stream_hold_back` has arrived (and not before three
    frames have, or the clip has ended: a clip of fewer than three frames passes through), from what has arrived by then."""
    lag = stream_hold_back(attention_window)
    n, out, cuts, done = len(frames), [], [], 0
    for j in range(n + 1):                                        # j == n: the end of the clip
        if 1 <= j < n and detect_scene_change(frames[j - 1], frames[j], scene_change_threshold):
            cuts.append(j)
        end = j == n
        while done < n and (end or (j - done >= lag and j >= 2)):
            seen = frames[:n if end else j + 1]
            # before the end at least three frames have arrived, `done` is not the last of them and the cuts up to done + window // 2
            # are known: the clamped neighbours and the `len(frames) < 3` rule read the same from `seen` as from the clip
            assert end or (len(seen) >= 3 and done + 1 < len(seen) and done + attention_window // 2 <= j)
            out.append(frames[done] if in_cut_window(done, cuts, attention_window) else
                       apply_frame(seen, done, method, flicker_threshold, blend_strength, attention_fn, called))
            done += 1
    return out


# ---- test inputs ---------------------------------------------------------------------------------------------------------------------
def flicker_triple(h: int, w: int, seed: int, blobs: bool = True) -> tuple:
    """(prev, cur, next): prev and next differ by at most 3 codes; cur is their neighbourhood perturbed on blobs of 7 x 7 or more
    against every border and in every corner, and on isolated pixels, so the stage has something to do."""
    rng = np.random.default_rng(seed)
    prev = rng.integers(30, 200, (h, w, 3), dtype=np.int64)
    nxt = np.clip(prev + rng.integers(-3, 4, (h, w, 3)), 0, 255)
    cur = np.clip(prev + rng.integers(-2, 3, (h, w, 3)), 0, 255)
    hit = np.zeros((h, w), bool)
    if blobs and h >= 7 and w >= 7:
        s = 7
        for y in sorted({0, (h - s) // 2, h - s}):
            for x in sorted({0, (w - s) // 2, w - s}):
                hit[y:y + s, x:x + s] = True
    iso = rng.random((h, w)) < 0.08
    hit |= iso
    delta = rng.integers(25, 60, (h, w, 3)) * rng.choice([-1, 1], (h, w, 1))
    cur = np.where(hit[:, :, None], np.clip(cur + delta, 0, 255), cur)
    return prev.astype(np.uint8), cur.astype(np.uint8), nxt.astype(np.uint8)


def flicker_clip(n: int, h: int, w: int, seed: int, cut_at=()) -> list:
    """n frames: a ramp scene with one code of noise whose odd frames flicker on blobs and isolated pixels; at every index of
    ``cut_at`` the scene changes (another brightness range, so the gray histograms stop correlating)."""
    rng = np.random.default_rng(seed)
    frames, scene = [], 0
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    ramp = (yy * 60) // h + (xx * 60) // w + 3 * cc
    for i in range(n):
        if i in cut_at:
            scene += 1
        base = ramp + (150 if scene % 2 else 20)
        f = np.clip(base + rng.integers(-1, 2, (h, w, 3)), 0, 255)
        if i % 2:
            hit = rng.random((h, w)) < 0.06
            if h >= 9 and w >= 9:
                y, x = int(rng.integers(0, h - 7)), int(rng.integers(0, w - 7))
                hit[y:y + 7, x:x + 7] = True
                hit[:7, :7] = True
            f = np.where(hit[:, :, None], np.clip(f + 45, 0, 255), f)
        frames.append(f.astype(np.uint8))
    return frames


def sweep_triple() -> tuple:
    """Every (prev, cur, next) triple of equal-channel greys from {0 .. 47} u {48, 56, .. 248} u {255}: 75^3 pixels as 5625 x 75."""
    levels = np.array(list(range(48)) + list(range(48, 249, 8)) + [255], np.uint8)
    assert levels.size == 75
    a, b, c = np.meshgrid(levels, levels, levels, indexing="ij")
    shape = (75 * 75, 75)
    return tuple(np.repeat(v.reshape(shape)[:, :, None], 3, axis=2).copy() for v in (a, b, c))
