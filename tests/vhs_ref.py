"""The contract of csrc/vhs.hip and framewright_amd/vhs.py: a NumPy restatement of the frame path of the reference's `VHSProcessor`
(processors/format/vhs.py) with every type spelled out.  tools/gen_vhs_golden.py holds it against the reference's own functions
(byte for byte for frames, field for field for the analysis); tests/test_vhs_ref_host.py holds it against what that run recorded.
Frames are uint8 arrays H x W (gray) or H x W x 3 (BGR); gray is the project's 14-bit form (tests/deinterlace_ref.gray).

Number formats (NumPy 2: a Python float times a float32 array stays float32, times a uint8 array it is float64):
  blends      tracking, head switching, rainbow, temporal dropout: float32(fa) * a + float32(fb) * b, fb = float32(1 - fa) with the
              difference formed in double; two rounded products, one rounded sum, truncating cast
  spatial     dropout fallback: ((1 - t) * left + t * right) in float64, s * that in float64, plus float32(1 - s) * float32(result)
              widened; truncating cast
  chroma      Y = 0.299 R + 0.587 G + 0.114 B in float64, left to right, then float32
  statistics  sums of |differences| are exact integers; a float32 mean is float32(sum) / float32(count)
A method that changes nothing returns the list or the frame it was given.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F32 = np.float32


@dataclass
class Config:
    tracking: float = 0.5
    head_switching: float = 0.7
    chroma_bleed: float = 0.5
    rainbow_removal: float = 0.5
    dropout_repair: float = 0.6
    head_switch_height: int = 16
    dropout_min_length: int = 5
    temporal_radius: int = 3


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(frames: Sequence[np.ndarray]) -> str:
    """One sha256 over the bytes of a list of frames, in order."""
    h = hashlib.sha256()
    for a in frames:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def gray(frame: np.ndarray) -> np.ndarray:
    if frame.ndim == 2:
        return frame
    v = frame.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + (1 << 13)) >> 14).astype(np.uint8)


def blend_f32(fa: float, a: np.ndarray, fb: float, b: np.ndarray) -> np.ndarray:
    """float32(fa) * a + float32(fb) * b on float32 arrays, as a float32 array."""
    return F32(fa) * a.astype(F32) + F32(fb) * b.astype(F32)


# ---- detection -----------------------------------------------------------------------------------------------------------------------
def head_switching_from_bottom(bottom: np.ndarray, height: int) -> Tuple[bool, Optional[int], float, np.ndarray]:
    """``bottom``: the last 30 gray rows.  The reference's own NumPy expression (np.var squares and rounds in float32)."""
    row_variances = np.var(np.diff(bottom.astype(F32), axis=1), axis=1)
    threshold = np.mean(row_variances) * 2.5
    noisy = np.where(row_variances > threshold)[0]
    if len(noisy) > 2:
        return True, height - 30 + int(np.min(noisy)), min(1.0, len(noisy) / 15.0), row_variances
    return False, None, 0.0, row_variances


def detect_head_switching(g: np.ndarray):
    return head_switching_from_bottom(g[g.shape[0] - 30:, :], g.shape[0])[:3]


def row_diff_sums(g: np.ndarray) -> np.ndarray:
    """int64 [H]: sum over x of |g[y, x+1] - g[y, x]|."""
    v = g.astype(np.int64)
    return np.abs(v[:, 1:] - v[:, :-1]).sum(axis=1)


def tracking_from_sums(sums: np.ndarray, height: int, width: int):
    """The reference's steps on the H float32 row means float32(sum) / float32(W - 1)."""
    row_activity = sums.astype(F32) / F32(width - 1)
    smoothed = np.convolve(row_activity, np.ones(5) / 5, mode="same")
    local_deviation = np.abs(row_activity - smoothed)
    threshold = np.std(local_deviation) * 2.5
    lines = [int(y) for y in np.where(local_deviation > threshold)[0].tolist() if y < height - 30]
    if lines:
        return True, min(1.0, len(lines) / 20.0), lines, local_deviation, threshold
    return False, 0.0, [], local_deviation, threshold


def detect_tracking(g: np.ndarray):
    return tracking_from_sums(row_diff_sums(g), g.shape[0], g.shape[1])[:3]


def dropout_runs(g: np.ndarray, min_length: int) -> List[Tuple[int, int, int, int]]:
    """Runs (x, y, length, 1) of gray > 250 or gray < 5 of at least ``min_length`` pixels, sorted by (y, x)."""
    h, w = g.shape
    runs = []
    for mask in (g > 250, g < 5):
        m = np.zeros((h, w + 2), dtype=np.int8)
        m[:, 1:-1] = mask
        d = np.diff(m, axis=1)
        ys, xs = np.where(d == 1)
        ye, xe = np.where(d == -1)                                    # row-major: the k-th end belongs to the k-th start
        for y, x0, x1 in zip(ys.tolist(), xs.tolist(), xe.tolist()):
            if x1 - x0 >= min_length:
                runs.append((x0, y, x1 - x0, 1))
    return sorted(runs, key=lambda r: (r[1], r[0]))


def merge_dropouts(runs: Sequence[Tuple[int, int, int, int]]) -> List[Tuple[int, int, int, int]]:
    """The reference's greedy rule on runs sorted by (y, x): bounding boxes, which may overlap each other."""
    if not runs:
        return []
    merged = []
    cx, cy, cw, ch = runs[0]
    for x, y, w, h in runs[1:]:
        if y <= cy + ch + 1 and x < cx + cw and x + w > cx:
            nx = min(cx, x)
            cw = max(cx + cw, x + w) - nx
            ch = y + h - cy
            cx = nx
        else:
            merged.append((cx, cy, cw, ch))
            cx, cy, cw, ch = x, y, w, h
    merged.append((cx, cy, cw, ch))
    return merged


def detect_dropouts(g: np.ndarray, min_length: int):
    merged = merge_dropouts(dropout_runs(g, min_length))
    return len(merged) > 0, len(merged), merged


def luma_edge_mask(frame: np.ndarray) -> np.ndarray:
    y = 0.299 * frame[:, :, 2] + 0.587 * frame[:, :, 1] + 0.114 * frame[:, :, 0]          # float64, left to right
    return np.abs(np.diff(y.astype(F32), axis=1)) > 30


def chroma_sample_offsets(frame: np.ndarray, y: int, x: int) -> Tuple[int, int]:
    """(offset of R, offset of B) for an edge at (y, x); -1 where the channel's largest step in the window is not above 20."""
    w = frame.shape[1]
    x0, x1 = max(0, x - 5), min(w - 2, x + 5)
    out = []
    for c in (2, 0):
        row = frame[y, :, c].astype(np.int64)
        local = np.abs(row[1:] - row[:-1])[x0:x1]
        out.append(abs(x0 + int(np.argmax(local)) - x) if len(local) > 0 and local.max() > 20 else -1)
    return out[0], out[1]


def detect_chroma_bleed(frame: np.ndarray, rng=None) -> Tuple[bool, float, Dict]:
    """``rng``: what `choice` is drawn from; None is NumPy's global generator, as in the reference."""
    stats: Dict = {"n_edges": 0, "mean_offset": None}
    mask = luma_edge_mask(frame)
    n = int(mask.sum())
    stats["n_edges"] = n
    if n < 10:
        return False, 0.0, stats
    ys, xs = np.where(mask)
    idx = (rng if rng is not None else np.random).choice(n, min(100, n), replace=False)
    offsets = []
    for i in idx:
        r, b = chroma_sample_offsets(frame, int(ys[i]), int(xs[i]))
        offsets += [o for o in (r, b) if o >= 0]
    if offsets:
        mean_offset = np.mean(offsets)
        stats["mean_offset"] = float(mean_offset)
        if mean_offset > 1.5:
            return True, min(1.0, mean_offset / 5.0), stats
    return False, 0.0, stats


def saturation_map(frame: np.ndarray) -> np.ndarray:
    mx = frame.max(axis=2)
    mn = frame.min(axis=2)
    return np.where(mx > 0, (mx - mn) / (mx + 1e-6), 0)               # uint8 difference (max >= min), float64 quotient


def rainbow_stats(frame: np.ndarray) -> Tuple[float, float]:
    magnitude = np.abs(np.fft.fft2(saturation_map(frame)))
    h, w = magnitude.shape
    return float(np.max(magnitude[h // 4:h // 2, w // 4:w // 2])), float(np.mean(magnitude))


def detect_rainbow(frame: np.ndarray) -> bool:
    diag_max, mean_mag = rainbow_stats(frame)
    return bool(diag_max > mean_mag * 5)


def dot_crawl_column_sums(frame: np.ndarray) -> np.ndarray:
    """int64 [W - 1]: sum over y of | |R - B|[y, x+1] - |R - B|[y, x] |."""
    c = np.abs(frame[:, :, 2].astype(np.int64) - frame[:, :, 0].astype(np.int64))
    return np.abs(c[:, 1:] - c[:, :-1]).sum(axis=0)


def dot_crawl_from_sums(sums: np.ndarray, height: int):
    row_means = sums.astype(F32) / F32(height)
    if len(row_means) < 10:
        return False, None, None
    magnitude = np.abs(np.fft.fft(row_means)[1:len(row_means) // 2])
    if len(magnitude) == 0:
        return False, None, None
    peak, mean = np.max(magnitude), np.mean(magnitude)
    return bool(peak > mean * 8), float(peak), float(mean)


def detect_dot_crawl(frame: np.ndarray) -> bool:
    return dot_crawl_from_sums(dot_crawl_column_sums(frame), frame.shape[0])[0]


def jitter_shifts(g: np.ndarray) -> np.ndarray:
    """The first maximum of the exact integer correlation c[j] = sum_n cur[n + j - W // 2] * prev[n], less W // 2, for rows
    1, 6, 11 ... H - 2.  The reference correlates float32 rows: equal while every partial sum is below 2^24 (W <= 258)."""
    w = g.shape[1]
    v = g.astype(np.int64)
    return np.array([int(np.argmax(np.correlate(v[y], v[y - 1], mode="same"))) - w // 2 for y in range(1, g.shape[0] - 1, 5)])


def jitter_from_shifts(shifts: np.ndarray) -> Tuple[bool, float]:
    var = np.var(shifts)
    if var > 2.0:
        return True, min(1.0, var / 10.0)
    return False, 0.0


@dataclass
class Analysis:
    head_switching_detected: bool = False
    head_switching_position: Optional[int] = None
    head_switching_severity: float = 0.0
    tracking_errors: bool = False
    tracking_severity: float = 0.0
    tracking_line_positions: List[int] = field(default_factory=list)
    dropout_detected: bool = False
    dropout_count: int = 0
    dropout_positions: List[Tuple[int, int, int, int]] = field(default_factory=list)
    chroma_bleed: bool = False
    chroma_bleed_severity: float = 0.0
    rainbow_effect: bool = False
    dot_crawl: bool = False
    jitter_detected: bool = False
    jitter_severity: float = 0.0
    overall_degradation: float = 0.0
    detected_quality: str = "unknown"
    artifact_types: List[str] = field(default_factory=list)


def degradation(a) -> float:
    score = 0.0
    if a.head_switching_detected:
        score += 0.15 * a.head_switching_severity
    if a.tracking_errors:
        score += 0.25 * a.tracking_severity
    if a.dropout_detected:
        score += 0.20 * min(1.0, a.dropout_count / 50.0)
    if a.chroma_bleed:
        score += 0.15 * a.chroma_bleed_severity
    if a.jitter_detected:
        score += 0.10 * a.jitter_severity
    if a.rainbow_effect:
        score += 0.08
    if a.dot_crawl:
        score += 0.07
    return min(1.0, score)


def quality(overall: float, width: int) -> str:
    return "ep" if overall > 0.6 else "lp" if overall > 0.3 else "sp" if width >= 720 else "unknown"


def analyze(frame: np.ndarray, cfg: Optional[Config] = None, rng=None) -> Analysis:
    cfg = cfg or Config()
    a = Analysis()
    g = gray(frame)
    h, w = g.shape
    a.head_switching_detected, a.head_switching_position, a.head_switching_severity = detect_head_switching(g)
    a.artifact_types += ["head_switching"] * a.head_switching_detected
    a.tracking_errors, a.tracking_severity, a.tracking_line_positions = detect_tracking(g)
    a.artifact_types += ["tracking_error"] * len(a.tracking_line_positions)
    a.dropout_detected, a.dropout_count, a.dropout_positions = detect_dropouts(g, cfg.dropout_min_length)
    a.artifact_types += ["dropout"] * a.dropout_count
    if frame.ndim == 3:
        a.chroma_bleed, a.chroma_bleed_severity, _ = detect_chroma_bleed(frame, rng)
        a.artifact_types += ["chroma_bleed"] * a.chroma_bleed
        a.rainbow_effect = detect_rainbow(frame)
        a.artifact_types += ["rainbow"] * a.rainbow_effect
        a.dot_crawl = detect_dot_crawl(frame)
        a.artifact_types += ["dot_crawl"] * a.dot_crawl
    a.jitter_detected, a.jitter_severity = jitter_from_shifts(jitter_shifts(g))
    a.artifact_types += ["jitter"] * a.jitter_detected
    a.overall_degradation = degradation(a)
    a.detected_quality = quality(a.overall_degradation, w)
    return a


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def head_switching_rows(position: int, height: int, strength: float, bh: int) -> List[Tuple[int, int, float, float]]:
    """(y, source row, fa, fb) of every row the step rewrites; the factors are formed in double."""
    rows = []
    if position > bh:
        for y in range(position, min(height, position + bh)):
            fa = strength * (1.0 - (y - position) / bh)
            rows.append((y, position - bh + (y - position) % bh, fa, 1 - fa))
    return rows


def remove_head_switching_frame(frame: np.ndarray, strength: float, cfg: Config) -> np.ndarray:
    detected, position, _ = detect_head_switching(gray(frame))
    if not detected:
        return frame
    out = frame.copy()
    for y, sy, fa, fb in head_switching_rows(position, frame.shape[0], strength, cfg.head_switch_height):
        out[y] = blend_f32(fa, frame[sy], fb, frame[y]).astype(np.uint8)
    return out


def fix_tracking_frame(frame: np.ndarray, strength: float, cfg: Config) -> np.ndarray:
    _, _, lines = detect_tracking(gray(frame))
    if not lines:
        return frame
    out = frame.copy()
    for y in lines:
        if 0 < y < frame.shape[0] - 1:
            mid = (frame[y - 1].astype(F32) + frame[y + 1].astype(F32)) / 2
            out[y] = blend_f32(strength, mid, 1 - strength, frame[y]).astype(np.uint8)
    return out


def box_gray_sum(frame: np.ndarray, box) -> int:
    x, y, w, h = box
    return int(gray(frame[y:y + h, x:x + w]).astype(np.int64).sum())


def fix_dropout_frame(frame: np.ndarray, prev: Sequence[np.ndarray], nxt: Sequence[np.ndarray], strength: float, cfg: Config,
                      log: Optional[list] = None) -> np.ndarray:
    """``log`` receives (box, 'temporal' with the index into prev + nxt | 'spatial' | 'none') per box."""
    detected, _, boxes = detect_dropouts(gray(frame), cfg.dropout_min_length)
    if not detected:
        return frame
    out = frame.copy()
    width = frame.shape[1]
    fb = F32(1 - strength)
    for box in boxes:
        x, y, w, h = box
        xe, ye = x + w, y + h                                         # merged boxes lie inside the frame
        n = w * h
        src = next((k for k, adj in enumerate(list(prev) + list(nxt)) if 10 * n < box_gray_sum(adj, box) < 245 * n), None)
        if src is not None:
            clean = (list(prev) + list(nxt))[src][y:ye, x:xe]
            out[y:ye, x:xe] = blend_f32(strength, clean, 1 - strength, out[y:ye, x:xe]).astype(np.uint8)
            if log is not None:
                log.append((box, "temporal", src))
            continue
        if x > 0 and xe < width:
            left, right = out[y:ye, x - 1].astype(np.float64), out[y:ye, xe].astype(np.float64)
            for xi in range(x, xe):
                t = (xi - x + 1) / (w + 1)
                interpolated = (1 - t) * left + t * right
                out[y:ye, xi] = (strength * interpolated + (fb * out[y:ye, xi].astype(F32)).astype(np.float64)).astype(np.uint8)
            if log is not None:
                log.append((box, "spatial", None))
        elif log is not None:
            log.append((box, "none", None))
    return out


def reduce_chroma_bleed_frame(frame: np.ndarray, strength: float, cfg: Config, rng=None) -> np.ndarray:
    if frame.ndim != 3:
        return frame
    detected, severity, _ = detect_chroma_bleed(frame, rng)
    if not detected:
        return frame
    out = frame.copy()
    shift = int(severity * 2 * strength)
    if shift > 0:
        out[:, shift:, 2] = frame[:, :-shift, 2]
        out[:, :-shift, 0] = frame[:, shift:, 0]
    return out


def rainbow_frame(frame: np.ndarray, strength: float, copy_borders: bool = False) -> np.ndarray:
    """``copy_borders`` is the wrong variant that leaves the border pixels as they are (the fixtures reject it at strength 0.7)."""
    if frame.ndim != 3:
        return frame
    v = frame.astype(np.int64)
    s8 = 8 * v
    s8[1:-1, 1:-1] = 4 * v[1:-1, 1:-1] + v[:-2, :-2] + v[:-2, 2:] + v[2:, :-2] + v[2:, 2:]
    result = s8.astype(F32) / F32(8)                                  # exact: multiples of 1/8 below 2^10
    out = np.clip(blend_f32(strength, result, 1 - strength, frame), 0, 255).astype(np.uint8)
    if copy_borders:
        out[0], out[-1], out[:, 0], out[:, -1] = frame[0], frame[-1], frame[:, 0], frame[:, -1]
    return out


def _each(frames, strength, fn):
    if not frames or strength <= 0:
        return frames
    return [fn(i, f) for i, f in enumerate(frames)]


def remove_head_switching(frames, cfg: Config, strength: Optional[float] = None):
    s = cfg.head_switching if strength is None else strength
    return _each(frames, s, lambda i, f: remove_head_switching_frame(f, s, cfg))


def fix_tracking_errors(frames, cfg: Config, strength: Optional[float] = None):
    s = cfg.tracking if strength is None else strength
    return _each(frames, s, lambda i, f: fix_tracking_frame(f, s, cfg))


def fix_dropout(frames, cfg: Config, strength: Optional[float] = None, log: Optional[list] = None):
    s = cfg.dropout_repair if strength is None else strength
    r = cfg.temporal_radius
    return _each(frames, s, lambda i, f: fix_dropout_frame(f, frames[max(0, i - r):i], frames[i + 1:min(len(frames), i + 1 + r)], s, cfg, log))


def reduce_chroma_bleed(frames, cfg: Config, strength: Optional[float] = None, rng=None):
    s = cfg.chroma_bleed if strength is None else strength
    return _each(frames, s, lambda i, f: reduce_chroma_bleed_frame(f, s, cfg, rng))


def remove_rainbow_artifacts(frames, cfg: Config, strength: Optional[float] = None):
    s = cfg.rainbow_removal if strength is None else strength
    return _each(frames, s, lambda i, f: rainbow_frame(f, s))


def process(frames, cfg: Optional[Config] = None, rng=None):
    cfg = cfg or Config()
    if not frames:
        return frames
    if cfg.head_switching > 0:
        frames = remove_head_switching(frames, cfg)
    if cfg.tracking > 0:
        frames = fix_tracking_errors(frames, cfg)
    if cfg.dropout_repair > 0:
        frames = fix_dropout(frames, cfg)
    if cfg.chroma_bleed > 0:
        frames = reduce_chroma_bleed(frames, cfg, rng=rng)
    if cfg.rainbow_removal > 0:
        frames = remove_rainbow_artifacts(frames, cfg)
    return frames


# ---- clips ---------------------------------------------------------------------------------------------------------------------------
SIZES = ((32, 8), (37, 33), (48, 64), (64, 258))
STRENGTHS = (0.5, 0.7, 1.0)
# float32(s) * v + float32(1 - s) * v truncates to v - 1 for 76 byte values at s = 0.9 (3, 6, 7, 9 ...), for none at 0.5, 0.7 or 1.0:
# the rainbow step blends border pixels with themselves, so 0.9 is where a kernel that copies the borders shows
RAINBOW_STRENGTHS = STRENGTHS + (0.9,)
N_FRAMES = 5


def _base(h: int, w: int, i: int, rng) -> np.ndarray:
    """A smooth BGR frame between 60 and 190 with noise of +-2: no luma edge, no extreme value."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 120 + 35 * np.sin(x / 9.0 + 0.3 * i) + 25 * np.cos(y / 6.0 + 0.2 * i)
    f = np.stack([v + 8, v, v - 8], axis=2) + rng.integers(-2, 3, size=(h, w, 3))
    return np.clip(f, 0, 255).astype(np.uint8)


def _run(f: np.ndarray, y: int, x0: int, x1: int, value: int) -> None:
    if 0 <= y < f.shape[0] and 0 <= x0 < x1 <= f.shape[1]:
        f[y, x0:x1] = value


def clip_mix(h: int, w: int, noisy_from: int) -> List[np.ndarray]:
    """Head-switching noise in the bottom 30 rows from row ``noisy_from`` of that region, tracking rows, dropouts."""
    rng = np.random.default_rng(1000 * h + w + noisy_from)
    frames = [_base(h, w, i, rng) for i in range(N_FRAMES)]
    wide = w >= 33
    for i, f in enumerate(frames):
        for r in range(noisy_from, min(30, noisy_from + 4)):
            f[h - 30 + r] = rng.integers(30, 221, size=(w, 1))
        for y in (1, h - 31, h - 9):
            if 0 < y < h:
                f[y] = np.where((np.arange(w) % 2 == 0)[:, None], 70, 170)
        # dropouts: groups at least three rows apart (the merge joins runs up to two rows apart), clear of the planted rows
        top = h - 22
        if wide:
            if i <= 2:
                _run(f, top, 10, 21, 255)                             # frames 0..2: the clean neighbour is frame 3, a next frame
            if i >= 3:
                _run(f, top, 23, 31, 252)                             # frames 3, 4: the clean neighbour is frame 0, a previous frame
            if i == 2:
                _run(f, top + 3, 8, 14, 255), _run(f, top + 3, 18, 24, 254), _run(f, top + 4, 11, 21, 255)   # overlapping boxes, temporal
            _run(f, top + 7, 5, 10, 0), _run(f, top + 7, 11, 20, 0), _run(f, top + 8, 7, 20, 0)              # overlapping boxes, spatial
            _run(f, top + 11, 0, 7, 255)                              # touches x = 0: no repair
            _run(f, top + 11, w - 6, w, 0)                            # touches x = W: no repair
            _run(f, top + 11, 10, 15, 255), _run(f, top + 11, 18, 22, 255)  # exactly min length (spatial), and one shorter
        else:
            if i == 2:
                _run(f, top, 1, 6, 255)                               # W = 8: min length in frame 2 only (temporal)
            _run(f, top + 3, 2, 7, 0)                                 # every frame: spatial
            _run(f, top + 6, 0, 5, 255)                               # touches x = 0
            _run(f, top + 9, 3, 7, 0)                                 # one shorter than min length
    return frames


def clip_chroma(h: int, w: int, displacement: int, rows: Optional[int] = None) -> List[np.ndarray]:
    """A luma step (G) at the middle column with the R and B steps ``displacement`` columns before it, on ``rows`` rows."""
    rng = np.random.default_rng(2000 * h + w + displacement)
    frames = []
    x0 = max(displacement + 1, w // 2)
    for i in range(N_FRAMES):
        f = np.full((h, w, 3), 60, dtype=np.uint8) + rng.integers(0, 3, size=(h, w, 3)).astype(np.uint8)
        n = h if rows is None else rows
        f[:n, x0 + 1:, 1] += 120
        f[:n, x0 + 1 - displacement:, 2] += 60
        f[:n, x0 + 1 - displacement:, 0] += 60
        f[:, :, 0] += np.uint8(i)                                     # frames differ
        frames.append(f)
    return frames


def clip_grating(h: int, w: int) -> List[np.ndarray]:
    """A diagonal saturation grating at (3H/8, 3W/8) cycles: inside the region `_detect_rainbow` looks at."""
    ky, kx = (3 * h) // 8, (3 * w) // 8
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for i in range(N_FRAMES):
        sat = 0.5 + 0.4 * np.cos(2 * np.pi * (ky * y / h + kx * x / w) + 0.5 * i)
        lo = np.rint(200 * (1 - sat)).astype(np.uint8)
        frames.append(np.stack([lo, lo, np.full((h, w), 200, dtype=np.uint8)], axis=2))
    return frames


def clip_dot_crawl(h: int, w: int) -> List[np.ndarray]:
    """|R - B| steps every fourth column."""
    rng = np.random.default_rng(3000 * h + w)
    frames = []
    for i in range(N_FRAMES):
        f = np.full((h, w, 3), 100, dtype=np.uint8) + rng.integers(0, 2, size=(h, w, 3)).astype(np.uint8)
        f[:, (np.arange(w) + i) % 8 < 4, 2] += 25
        frames.append(f)
    return frames


def clip_jitter(h: int, w: int) -> List[np.ndarray]:
    """White rows between 20 and 235, moved by 3 columns and back every five rows."""
    rng = np.random.default_rng(4000 * h + w)
    frames = []
    for i in range(N_FRAMES):
        row = rng.integers(20, 236, size=w).astype(np.uint8)
        g = np.stack([np.roll(row, 3 if y >= 1 and ((y - 1) // 5) % 2 == 0 else 0) for y in range(h)])
        frames.append(np.stack([g, g, g], axis=2))
    return frames


def clip_plain(h: int, w: int) -> List[np.ndarray]:
    rng = np.random.default_rng(5000 * h + w)
    return [_base(h, w, i, rng) for i in range(N_FRAMES)]


def clips() -> Dict[str, List[np.ndarray]]:
    """name -> list of 5 BGR frames; "<name>/gray" is the same list as gray frames."""
    out: Dict[str, List[np.ndarray]] = {}
    for h, w in SIZES:
        s = f"{h}x{w}"
        out[f"mix_low/{s}"] = clip_mix(h, w, 4)                      # position = H - 26
        if (h, w) in ((37, 33), (48, 64)):
            out[f"mix_high/{s}"] = clip_mix(h, w, 22)                 # position = H - 8: the band is cut off at the last row
        out[f"plain/{s}"] = clip_plain(h, w)
        out[f"jitter/{s}"] = clip_jitter(h, w)
        out[f"grating/{s}"] = clip_grating(h, w)
        out[f"dot_crawl/{s}"] = clip_dot_crawl(h, w)
        if w >= 33:
            out[f"chroma5/{s}"] = clip_chroma(h, w, 5)
            out[f"chroma2/{s}"] = clip_chroma(h, w, 2)
            out[f"few_edges/{s}"] = clip_chroma(h, w, 5, rows=7)
    for name in [n for n in out if n.split("/")[0] in ("mix_low", "mix_high", "jitter")]:
        out[name + "/gray"] = [gray(f) for f in out[name]]
    return out


METHODS = {"head_switching": remove_head_switching, "tracking": fix_tracking_errors, "dropout": fix_dropout,
           "chroma_bleed": reduce_chroma_bleed, "rainbow": remove_rainbow_artifacts}
ANALYSIS_FRAME = 2


def recorded_cases(name: str) -> List[Tuple[str, float]]:
    """(method, strength) pairs recorded for a clip, besides `process` with the default configuration and the analysis of frame 2.
    Every call that reaches the chroma detector is made right after np.random.seed(seed_of(name, method, strength))."""
    kind = name.split("/")[0]
    is_gray = name.endswith("/gray")
    cases = []
    if kind in ("mix_low", "mix_high"):
        cases += [(m, s) for m in ("head_switching", "tracking", "dropout") for s in STRENGTHS]
    if kind in ("mix_low", "plain"):
        cases += [("rainbow", s) for s in RAINBOW_STRENGTHS]
    if kind == "grating":
        cases += [("rainbow", 0.5)]
    if kind in ("chroma5", "chroma2", "few_edges"):
        cases += [("chroma_bleed", 1.0), ("chroma_bleed", 0.5)]
    if kind in ("mix_low", "plain") or is_gray:
        cases += [("chroma_bleed", 0.5)]
    if kind == "jitter":
        cases += [("tracking", 0.5), ("dropout", 0.6)]
    return cases


def seed_of(name: str, method: str, strength: float) -> int:
    return int(hashlib.sha256(f"{name}|{method}|{strength}".encode()).hexdigest()[:7], 16)


def case_key(name: str, method: str, strength: float) -> str:
    return f"{name}|{method}|{strength}"


def stats_record(frame: np.ndarray, cfg: Optional[Config] = None) -> Dict:
    """What each threshold of the analysis sees on a frame, formed as the reference forms it (its locals; not returned by it)."""
    g = gray(frame)
    h, w = g.shape
    _, _, _, variances = head_switching_from_bottom(g[h - 30:], h)
    _, _, _, dev, thr = tracking_from_sums(row_diff_sums(g), h, w)
    rec = {"variance_mean": float(np.mean(variances)), "variance_max": float(np.max(variances)),
           "tracking_threshold": float(thr), "tracking_max_deviation": float(dev.max()),
           "jitter_shifts": [int(v) for v in jitter_shifts(g)]}
    if frame.ndim == 3:
        rec["n_edges"] = int(luma_edge_mask(frame).sum())
        rec["rainbow_diag_max"], rec["rainbow_mean_mag"] = rainbow_stats(frame)
        _, rec["dot_crawl_peak"], rec["dot_crawl_mean"] = dot_crawl_from_sums(dot_crawl_column_sums(frame), h)
    return rec
