"""The contract of csrc/quality.hip and framewright_amd/quality.py: a NumPy restatement of the frame path of the reference's
`FrameQualityScorer` (processors/frame_quality_scorer.py): `score_frame` with its seven measures and the duplicate state they carry
between frames, the report loop of `analyze_video` over a list of frames, `_generate_recommendations`, and the value types.
tools/gen_quality_golden.py holds it against the reference's own methods, field for field; tests/test_quality_ref_host.py holds it
against what that run recorded.  Frames are uint8 arrays H x W x 3 (BGR).

What the cv2 calls mean here (cv2 is absent, so its own bytes are unpinned, as everywhere in this project):
  cvtColor(BGR2GRAY)             the project's 14-bit gray (csrc/stage_common.h, tests/aspect_ref.gray)
  cvtColor(BGR2LAB)              tests/flicker_ref.bgr_to_lab_gamma; only L is read
  Laplacian(gray, CV_64F)        the 3 x 3 cross [0 1 0; 1 -4 1; 0 1 0], BORDER_REFLECT_101
  GaussianBlur(gray, (5, 5), 0)  the taps 1 4 6 4 1 in both directions, (sum + 128) >> 8, BORDER_REFLECT_101
  Sobel(., CV_64F, 1, 1, 3)      the outer product of [-1 0 1] with itself, BORDER_REFLECT_101
  Sobel(., CV_64F, 1, 0, 3)      [1 2 1]^T x [-1 0 1], BORDER_REFLECT_101
  calcHist                       a float32 [256, 1] array of counts
  resize(gray, (32, 32))         oracle/face_ref.resize_linear_u8
  absdiff                        |a - b| on uint8

`frame_statistics(frame)` gives the integers every score is a function of; the device forms exactly these (one pass over the frame)
and the host epilogue of quality.py turns them into the scores.  `score_from_statistics` is that epilogue's arithmetic, so the
statement "the scores are a function of the integers" is itself held by the generator and the host test.

The float bound (DESIGN K19).  The reference takes np.var of the Laplacian and np.std of the noise plane and of the frame's bytes:
pairwise float64 sums over N values.  From the integer sums the variance is the exact rational (N S2 - S1^2) / N^2, rounded once.
`var_bound` / `std_bound` bound the difference between the two.
"""
from __future__ import annotations

import hashlib
import json
import math
import sys
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
if str(ROOT / "tests") not in sys.path:
    sys.path.insert(0, str(ROOT / "tests"))
from oracle.face_ref import resize_linear_u8  # noqa: E402
import flicker_ref  # noqa: E402

U = 2.0 ** -53                                       # the unit roundoff of float64


# ---- value types ------------------------------------------------------------------------------------------------------------------------
class QualityIssue(Enum):
    BLUR = "blur"
    NOISE = "noise"
    OVEREXPOSED = "overexposed"
    UNDEREXPOSED = "underexposed"
    BLOCKING = "blocking"
    BANDING = "banding"
    INTERLACING = "interlacing"
    DUPLICATE = "duplicate"
    BLACK_FRAME = "black_frame"
    CORRUPTED = "corrupted"


@dataclass
class FrameScore:
    frame_number: int
    timestamp: float
    overall_score: float
    sharpness_score: float
    noise_score: float
    exposure_score: float
    artifact_score: float
    issues: List[QualityIssue] = field(default_factory=list)
    issue_details: Dict[str, float] = field(default_factory=dict)

    @property
    def has_issues(self) -> bool:
        return len(self.issues) > 0

    @property
    def is_problematic(self) -> bool:
        critical = {QualityIssue.CORRUPTED, QualityIssue.BLACK_FRAME}
        return self.overall_score < 50 or any(i in critical for i in self.issues)


@dataclass
class QualityReport:
    video_path: str
    total_frames: int
    analyzed_frames: int
    average_score: float
    min_score: float
    max_score: float
    problem_frames: List[FrameScore]
    issue_counts: Dict[str, int]
    score_distribution: Dict[str, int]
    recommendations: List[str]

    def get_worst_frames(self, n: int = 10) -> List[FrameScore]:
        return sorted(self.problem_frames, key=lambda f: f.overall_score)[:n]

    def get_frames_with_issue(self, issue: QualityIssue) -> List[FrameScore]:
        return [f for f in self.problem_frames if issue in f.issues]

    def to_dict(self) -> Dict:
        return {
            "video_path": self.video_path, "total_frames": self.total_frames, "analyzed_frames": self.analyzed_frames,
            "average_score": self.average_score, "min_score": self.min_score, "max_score": self.max_score,
            "problem_frame_count": len(self.problem_frames),
            "problem_frames": [{"frame": f.frame_number, "timestamp": f.timestamp, "score": f.overall_score,
                                "issues": [i.value for i in f.issues]} for f in self.problem_frames],
            "issue_counts": self.issue_counts, "score_distribution": self.score_distribution, "recommendations": self.recommendations}

    def save(self, path) -> None:
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2)


DISTRIBUTION = (("excellent (90-100)", 90), ("good (70-89)", 70), ("fair (50-69)", 50), ("poor (30-49)", 30), ("bad (0-29)", None))


# ---- what the cv2 calls mean ------------------------------------------------------------------------------------------------------------
def gray(frame: np.ndarray) -> np.ndarray:
    v = frame.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def lab_l(frame: np.ndarray) -> np.ndarray:
    return flicker_ref.bgr_to_lab_gamma(frame)[..., 0]


def _pad(plane: np.ndarray, r: int) -> np.ndarray:
    return np.pad(plane.astype(np.int64), r, mode="reflect")          # BORDER_REFLECT_101, reflected as often as it takes


def laplacian(g: np.ndarray) -> np.ndarray:
    p = _pad(g, 1)
    return (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * p[1:-1, 1:-1]).astype(np.float64)


def gaussian_blur5(g: np.ndarray) -> np.ndarray:
    h, w = g.shape
    p = _pad(g, 2)
    k = (1, 4, 6, 4, 1)
    rows = sum(k[i] * p[:, i:i + w] for i in range(5))
    both = sum(k[i] * rows[i:i + h] for i in range(5))
    return ((both + 128) >> 8).astype(np.uint8)


def sobel_xy(g: np.ndarray) -> np.ndarray:
    p = _pad(g, 1)
    return (p[:-2, :-2] - p[:-2, 2:] - p[2:, :-2] + p[2:, 2:]).astype(np.float64)


def sobel_x(g: np.ndarray) -> np.ndarray:
    p = _pad(g, 1)
    d = p[:, 2:] - p[:, :-2]
    return (d[:-2] + 2 * d[1:-1] + d[2:]).astype(np.float64)


def calc_hist(g: np.ndarray) -> np.ndarray:
    return np.bincount(g.reshape(-1), minlength=256).astype(np.float32).reshape(256, 1)


def thumbnail(g: np.ndarray) -> np.ndarray:
    return resize_linear_u8(g, 32, 32)


def absdiff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)


# ---- the float bound --------------------------------------------------------------------------------------------------------------------
def sum_depth(n: int) -> int:
    """An upper bound of the number of float64 additions any term of numpy's pairwise sum of n values passes through: blocks of at most
    128 values are added into 8 accumulators (16 additions) that are combined in 3 more, and the blocks in a binary tree."""
    return 19 + max(0, math.ceil(math.log2(max(n, 1))) - 6)


def var_bound(n: int, variance: float, mean: float = 0.0) -> float:
    """|np.var(x) - fl((n S2 - S1^2) / n^2)| for n integers x of that variance and mean (DESIGN K19).  np.var forms m = fl(S1 / n)
    (S1 is exact), d = fl(x - m), q = fl(d d), a pairwise sum and one division: sum (x - m)^2 = n var + n (m - mean)^2 exactly, with
    |m - mean| <= u |mean|, and every term carries at most 2 + 1 + depth + 1 roundings; the rational carries one."""
    k = sum_depth(n) + 5
    return (k * U / (1 - k * U)) * (variance + (U * mean) ** 2) + U * variance


def std_bound(n: int, std: float, mean: float = 0.0) -> float:
    """The same for np.std: the square root halves the relative error of the variance and rounds once on either side."""
    if std == 0.0:
        return math.sqrt(var_bound(n, 0.0, mean))
    return (var_bound(n, std * std, mean) / (2 * std * std) + 3 * U) * std * (1 + 1e-9)


def exact_variance(n: int, s1: int, s2: int) -> float:
    """fl((n s2 - s1^2) / n^2): Python's integer division rounds the exact quotient once."""
    return (n * s2 - s1 * s1) / (n * n)


def exact_std(n: int, s1: int, s2: int) -> float:
    """The square root of that rational, from an integer square root with 128 fractional bits, rounded once."""
    num = n * s2 - s1 * s1
    return math.isqrt((num << 256) // (n * n)) / (1 << 128)


# ---- the integers -----------------------------------------------------------------------------------------------------------------------
def block_lines(length: int) -> range:
    return range(8, length - 8, 8)


def frame_statistics(frame: np.ndarray) -> Dict[str, object]:
    """The integers every score is a function of.  ValueError for a frame with an odd side, as the reference's row-pair subtraction
    raises one."""
    h, w = frame.shape[:2]
    if h % 2 or w % 2:
        raise ValueError(f"operands could not be broadcast together: a frame with an odd side ({w} x {h})")
    g = gray(frame)
    gi = g.astype(np.int64)
    lap = laplacian(g).astype(np.int64)
    d = absdiff(g, gaussian_blur5(g)).astype(np.int64)
    grad = np.abs(sobel_x(lab_l(frame)).astype(np.int64))
    v = frame.astype(np.int64).reshape(-1)
    return {
        "lap_sum": int(lap.sum()), "lap_sq_sum": int((lap * lap).sum()),
        "noise_sum": int(d.sum()), "noise_sq_sum": int((d * d).sum()),
        "gray_hist": np.bincount(g.reshape(-1), minlength=256).astype(np.int64),
        "block_rows": np.array([int(np.abs(gi[i] - gi[i - 1]).sum()) for i in block_lines(h)], dtype=np.int64),
        "block_cols": np.array([int(np.abs(gi[:, j] - gi[:, j - 1]).sum()) for j in block_lines(w)], dtype=np.int64),
        "edge_sum": int(np.abs(sobel_xy(g).astype(np.int64)).sum()),
        "strong": int((grad > 30).sum()), "weak": int(((grad > 5) & (grad <= 30)).sum()),
        "row_pair_sum": int(np.abs(gi[::2] - gi[1::2]).sum()), "col_pair_sum": int(np.abs(gi[:, ::2] - gi[:, 1::2]).sum()),
        "byte_sum": int(v.sum()), "byte_sq_sum": int((v * v).sum()),
        "byte_hist": np.bincount(frame.reshape(-1), minlength=256).astype(np.int64),
        "thumbnail": thumbnail(g).reshape(-1),
        "height": int(h), "width": int(w),
    }


SCALARS = ("lap_sum", "lap_sq_sum", "noise_sum", "noise_sq_sum", "edge_sum", "strong", "weak", "row_pair_sum", "col_pair_sum", "byte_sum",
           "byte_sq_sum")
ARRAYS = ("gray_hist", "byte_hist", "block_rows", "block_cols", "thumbnail")


def statistics_digest(s: Dict[str, object]) -> str:
    h = hashlib.sha256()
    h.update(",".join(str(int(s[k])) for k in SCALARS).encode())
    for k in ARRAYS:
        h.update(np.ascontiguousarray(np.asarray(s[k]).astype(np.int64)).tobytes())
    return h.hexdigest()


def statistics_equal(a: Dict[str, object], b: Dict[str, object]) -> bool:
    return all(int(a[k]) == int(b[k]) for k in SCALARS) and \
        all(np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)) for k in ARRAYS)


# ---- the scorer -------------------------------------------------------------------------------------------------------------------------
class FrameQualityScorer:
    BLUR_THRESHOLD = 100
    NOISE_THRESHOLD = 15
    OVEREXPOSED_THRESHOLD = 250
    UNDEREXPOSED_THRESHOLD = 20
    BLACK_FRAME_THRESHOLD = 5
    DUPLICATE_THRESHOLD = 0.99

    def __init__(self, sample_rate: int = 1, problem_threshold: float = 60.0, progress_callback: Optional[Callable[[int, int], None]] = None):
        self.sample_rate = max(1, sample_rate)
        self.problem_threshold = problem_threshold
        self.progress_callback = progress_callback
        self._prev_frame_hash = None

    # the seven measures, each on what the reference hands it
    def _calculate_sharpness(self, g):
        variance = laplacian(g).var()
        return min(100, (variance / 500) * 100), variance < self.BLUR_THRESHOLD

    def _calculate_noise(self, g):
        noise_level = np.std(absdiff(g, gaussian_blur5(g)))
        return max(0, 100 - (noise_level / 30) * 100), noise_level > self.NOISE_THRESHOLD

    def _calculate_exposure(self, g):
        mean_brightness = np.mean(g)
        if mean_brightness < self.BLACK_FRAME_THRESHOLD:
            return 0, False, True
        over, under = mean_brightness > self.OVEREXPOSED_THRESHOLD, mean_brightness < self.UNDEREXPOSED_THRESHOLD
        score = 100 * (1 - abs(mean_brightness - 128) / 128)
        hist = calc_hist(g)
        if np.sum(hist[:5]) / g.size > 0.05 or np.sum(hist[251:]) / g.size > 0.05:
            score *= 0.8
        return max(0, score), over, under

    def _detect_blocking(self, g):
        h, w = g.shape
        block_diff, count = 0, 0
        for i in block_lines(h):
            block_diff += np.mean(np.abs(g[i, :].astype(float) - g[i - 1, :].astype(float)))
            count += 1
        for j in block_lines(w):
            block_diff += np.mean(np.abs(g[:, j].astype(float) - g[:, j - 1].astype(float)))
            count += 1
        if count > 0:
            block_diff /= count
        overall_edges = np.mean(np.abs(sobel_xy(g)))
        ratio = block_diff / overall_edges if overall_edges > 0 else 0
        return (max(0, 100 - (ratio - 1) * 50) if ratio > 1 else 100), ratio > 1.5

    def _detect_banding(self, frame):
        grad = np.abs(sobel_x(lab_l(frame)))
        strong, weak = np.sum(grad > 30), np.sum((grad > 5) & (grad <= 30))
        ratio = strong / weak if weak > 0 else 0
        return (max(0, 100 - (ratio - 1) * 25) if ratio > 1 else 100), ratio > 2

    def _detect_interlacing(self, g):
        mean_diff = np.mean(np.abs(g[::2, :].astype(float) - g[1::2, :].astype(float)))
        mean_col_diff = np.mean(np.abs(g[:, ::2].astype(float) - g[:, 1::2].astype(float)))
        ratio = mean_diff / mean_col_diff if mean_col_diff > 0 else 0
        return (max(0, 100 - (ratio - 1) * 30) if ratio > 1 else 100), (ratio > 1.5 and mean_diff > 10)

    def _check_duplicate(self, g):
        frame_hash = thumbnail(g).flatten()
        is_dup = False
        if self._prev_frame_hash is not None:
            with np.errstate(invalid="ignore", divide="ignore"):      # a constant thumbnail: nan, which is not above the threshold
                is_dup = np.corrcoef(frame_hash, self._prev_frame_hash)[0, 1] > self.DUPLICATE_THRESHOLD
        self._prev_frame_hash = frame_hash
        return is_dup

    def _check_corrupted(self, frame):
        if frame is None or frame.size == 0:
            return True
        return bool(np.std(frame) < 1 or len(np.unique(frame)) < 10)

    def score_frame(self, frame: np.ndarray, frame_number: int, fps: float) -> FrameScore:
        timestamp = frame_number / fps if fps > 0 else 0
        if self._check_corrupted(frame):
            return FrameScore(frame_number, timestamp, 0, 0, 0, 0, 0, issues=[QualityIssue.CORRUPTED])
        g = gray(frame)
        sharpness, blurry = self._calculate_sharpness(g)
        noise, noisy = self._calculate_noise(g)
        exposure, over, under = self._calculate_exposure(g)
        blocking, has_blocking = self._detect_blocking(g)
        banding, has_banding = self._detect_banding(frame)
        interlace, has_interlacing = self._detect_interlacing(g)
        duplicate = self._check_duplicate(g)
        return assemble_score(self, frame_number, timestamp, sharpness, blurry, noise, noisy, exposure, over, under,
                              bool(under and np.mean(g) < self.BLACK_FRAME_THRESHOLD), blocking, has_blocking, banding, has_banding,
                              interlace, has_interlacing, duplicate)

    def analyze_frames(self, frames, fps: float, total_frames: Optional[int] = None, start_frame: int = 0, end_frame: Optional[int] = None,
                       video_path: str = "") -> QualityReport:
        """`analyze_video` with the list ``frames`` in the place of the decoder: frame k of the video is frames[k]."""
        total_frames = len(frames) if total_frames is None else int(total_frames)
        if end_frame is None:
            end_frame = total_frames
        self._prev_frame_hash = None
        collector = ReportCollector(self, video_path, total_frames)
        frame_num = start_frame
        while frame_num < end_frame:
            if not 0 <= frame_num < len(frames):
                break
            if (frame_num - start_frame) % self.sample_rate == 0:
                collector.add(self.score_frame(frames[frame_num], frame_num, fps))
                if self.progress_callback:
                    self.progress_callback(frame_num, end_frame)
            frame_num += 1
        return collector.report()

    def _generate_recommendations(self, scores, issue_counts, problem_frames):
        return recommendations(scores, issue_counts)


def assemble_score(k, frame_number, timestamp, sharpness, blurry, noise, noisy, exposure, over, under, black, blocking, has_blocking,
                   banding, has_banding, interlace, has_interlacing, duplicate) -> FrameScore:
    """The tail of `score_frame`: the issue list in the reference's order and the two weighted means."""
    issues, details = [], {}
    if blurry:
        issues.append(QualityIssue.BLUR)
        details["blur_variance"] = sharpness
    if noisy:
        issues.append(QualityIssue.NOISE)
        details["noise_level"] = 100 - noise
    if over:
        issues.append(QualityIssue.OVEREXPOSED)
    if under:
        issues.append(QualityIssue.UNDEREXPOSED)
        if black:
            issues.append(QualityIssue.BLACK_FRAME)
    for flag, issue in ((has_blocking, QualityIssue.BLOCKING), (has_banding, QualityIssue.BANDING),
                        (has_interlacing, QualityIssue.INTERLACING), (duplicate, QualityIssue.DUPLICATE)):
        if flag:
            issues.append(issue)
    artifact = (blocking + banding + interlace) / 3
    overall = sharpness * 0.3 + noise * 0.25 + exposure * 0.25 + artifact * 0.2
    return FrameScore(frame_number, timestamp, overall, sharpness, noise, exposure, artifact, issues, details)


class ReportCollector:
    """The bookkeeping of `analyze_video` around its calls of `score_frame`."""

    def __init__(self, scorer, video_path: str, total_frames: int):
        self.scorer, self.video_path, self.total_frames = scorer, video_path, total_frames
        self.all_scores, self.problem_frames = [], []
        self.issue_counts = {issue.value: 0 for issue in QualityIssue}

    def add(self, score: FrameScore) -> None:
        self.all_scores.append(score.overall_score)
        for issue in score.issues:
            self.issue_counts[issue.value] += 1
        if score.overall_score < self.scorer.problem_threshold or score.has_issues:
            self.problem_frames.append(score)

    def report(self) -> QualityReport:
        dist = {name: 0 for name, _ in DISTRIBUTION}
        for s in self.all_scores:
            dist[next(name for name, low in DISTRIBUTION if low is None or s >= low)] += 1
        scores = self.all_scores
        return QualityReport(video_path=str(self.video_path), total_frames=self.total_frames, analyzed_frames=len(scores),
                             average_score=np.mean(scores) if scores else 0, min_score=min(scores) if scores else 0,
                             max_score=max(scores) if scores else 0, problem_frames=self.problem_frames, issue_counts=self.issue_counts,
                             score_distribution=dist, recommendations=recommendations(scores, self.issue_counts))


RECOMMENDATIONS = {
    "none": "Unable to analyze video",
    "good": "Video quality is good - light processing recommended",
    "moderate": "Video has moderate quality issues - standard processing recommended",
    "poor": "Video has significant quality issues - aggressive processing recommended",
    "blur": "Significant blur detected - consider sharpening or AI upscaling",
    "noise": "High noise levels - recommend denoising (temporal if available)",
    "blocking": "Compression artifacts detected - consider deblocking filter",
    "interlacing": "Interlacing detected - apply deinterlacing (YADIF or QTGMC)",
    "banding": "Color banding present - consider debanding or bit depth increase",
    "duplicate": "Many duplicate frames - video may be telecined or have frame rate issues",
    "black_frame": "Found {n} black frames - may need manual review",
}


def recommendations(scores, issue_counts) -> List[str]:
    """`_generate_recommendations`; the sentences are the reference's public output, which a caller may match on."""
    t = RECOMMENDATIONS
    if not scores:
        return [t["none"]]
    avg = np.mean(scores)
    out = [t["good"] if avg >= 80 else t["moderate"] if avg >= 50 else t["poor"]]
    total = sum(issue_counts.values())
    for key, share in (("blur", 0.1), ("noise", 0.1), ("blocking", 0.1), ("interlacing", 0.05), ("banding", 0.1)):
        if issue_counts.get(key, 0) > total * share:
            out.append(t[key])
    if issue_counts.get("duplicate", 0) > len(scores) * 0.1:
        out.append(t["duplicate"])
    if issue_counts.get("black_frame", 0) > 0:
        out.append(t["black_frame"].format(n=issue_counts["black_frame"]))
    return out


# ---- the scores as a function of the integers -------------------------------------------------------------------------------------------
def measures_from_statistics(k, s: Dict[str, object]) -> Dict[str, object]:
    """Every quantity of `score_frame` short of the duplicate test, from `frame_statistics` alone, with the thresholds of ``k``.
    Wherever the reference's float operations act on exact integers these are the same operations in the same order; the variance
    and the two standard deviations are exact rationals rounded once.  This is the arithmetic of quality.py's host epilogue."""
    h, w = int(s["height"]), int(s["width"])
    n = h * w
    f64 = np.float64
    m = {"byte_std": exact_std(3 * n, int(s["byte_sum"]), int(s["byte_sq_sum"])), "unique": int(np.count_nonzero(s["byte_hist"]))}
    m["corrupted"] = bool(m["byte_std"] < 1 or m["unique"] < 10)
    m["variance"] = f64(exact_variance(n, int(s["lap_sum"]), int(s["lap_sq_sum"])))
    m["sharpness"], m["blurry"] = min(100, (m["variance"] / 500) * 100), bool(m["variance"] < k.BLUR_THRESHOLD)
    m["noise_level"] = f64(exact_std(n, int(s["noise_sum"]), int(s["noise_sq_sum"])))
    m["noise"], m["noisy"] = max(0, 100 - (m["noise_level"] / 30) * 100), bool(m["noise_level"] > k.NOISE_THRESHOLD)
    hist = np.asarray(s["gray_hist"]).astype(np.float32).reshape(256, 1)
    mean = f64(int((np.asarray(s["gray_hist"]).astype(np.int64) * np.arange(256)).sum())) / f64(n)
    m["mean"] = mean
    m["black"] = bool(mean < k.BLACK_FRAME_THRESHOLD)
    if m["black"]:
        m["exposure"], m["over"], m["under"], m["clipped"] = 0, False, True, None
    else:
        m["over"], m["under"] = bool(mean > k.OVEREXPOSED_THRESHOLD), bool(mean < k.UNDEREXPOSED_THRESHOLD)
        score = 100 * (1 - abs(mean - 128) / 128)
        m["clip_dark"], m["clip_bright"] = np.sum(hist[:5]) / n, np.sum(hist[251:]) / n
        m["clipped"] = bool(m["clip_dark"] > 0.05 or m["clip_bright"] > 0.05)
        if m["clipped"]:
            score *= 0.8
        m["exposure"] = max(0, score)
    block_diff, count = 0, 0
    for r in np.asarray(s["block_rows"]).astype(np.int64):
        block_diff += f64(int(r)) / f64(w)
        count += 1
    for c in np.asarray(s["block_cols"]).astype(np.int64):
        block_diff += f64(int(c)) / f64(h)
        count += 1
    if count > 0:
        block_diff /= count
    edges = f64(int(s["edge_sum"])) / f64(n)
    m["blocking_ratio"] = block_diff / edges if edges > 0 else 0
    m["blocking"] = max(0, 100 - (m["blocking_ratio"] - 1) * 50) if m["blocking_ratio"] > 1 else 100
    m["has_blocking"] = bool(m["blocking_ratio"] > 1.5)
    strong, weak = int(s["strong"]), int(s["weak"])
    m["banding_ratio"] = f64(strong) / f64(weak) if weak > 0 else 0
    m["banding"] = max(0, 100 - (m["banding_ratio"] - 1) * 25) if m["banding_ratio"] > 1 else 100
    m["has_banding"] = bool(m["banding_ratio"] > 2)
    half = f64(n // 2)
    m["mean_diff"], m["mean_col_diff"] = f64(int(s["row_pair_sum"])) / half, f64(int(s["col_pair_sum"])) / half
    m["interlace_ratio"] = m["mean_diff"] / m["mean_col_diff"] if m["mean_col_diff"] > 0 else 0
    m["interlace"] = max(0, 100 - (m["interlace_ratio"] - 1) * 30) if m["interlace_ratio"] > 1 else 100
    m["has_interlacing"] = bool(m["interlace_ratio"] > 1.5 and m["mean_diff"] > 10)
    return m


def thumbnails_duplicate(k, thumb: np.ndarray, prev: Optional[np.ndarray]) -> bool:
    if prev is None:
        return False
    with np.errstate(invalid="ignore", divide="ignore"):
        return bool(np.corrcoef(thumb, prev)[0, 1] > k.DUPLICATE_THRESHOLD)


def score_from_statistics(k, s: Dict[str, object], prev_thumb, frame_number: int, fps: float):
    """(FrameScore, the thumbnail the next frame is compared with) from the integers; ``prev_thumb`` is the duplicate state."""
    timestamp = frame_number / fps if fps > 0 else 0
    m = measures_from_statistics(k, s)
    if m["corrupted"]:
        return FrameScore(frame_number, timestamp, 0, 0, 0, 0, 0, issues=[QualityIssue.CORRUPTED]), prev_thumb
    thumb = np.asarray(s["thumbnail"]).astype(np.uint8).reshape(-1)
    dup = thumbnails_duplicate(k, thumb, prev_thumb)
    score = assemble_score(k, frame_number, timestamp, m["sharpness"], m["blurry"], m["noise"], m["noisy"], m["exposure"], m["over"],
                           m["under"], m["under"] and m["black"], m["blocking"], m["has_blocking"], m["banding"], m["has_banding"],
                           m["interlace"], m["has_interlacing"], dup)
    return score, thumb


# ---- comparing a score with a recorded one ----------------------------------------------------------------------------------------------
def score_record(s: FrameScore) -> Dict[str, object]:
    return {"frame_number": int(s.frame_number), "timestamp": repr(float(s.timestamp)), "overall_score": repr(float(s.overall_score)),
            "sharpness_score": repr(float(s.sharpness_score)), "noise_score": repr(float(s.noise_score)),
            "exposure_score": repr(float(s.exposure_score)), "artifact_score": repr(float(s.artifact_score)),
            "issues": [i.value for i in s.issues], "issue_details": {k: repr(float(v)) for k, v in s.issue_details.items()}}


def report_record(r: QualityReport) -> Dict[str, object]:
    return {"video_path": r.video_path, "total_frames": int(r.total_frames), "analyzed_frames": int(r.analyzed_frames),
            "average_score": repr(float(r.average_score)), "min_score": repr(float(r.min_score)), "max_score": repr(float(r.max_score)),
            "problem_frames": [int(f.frame_number) for f in r.problem_frames], "issue_counts": dict(r.issue_counts),
            "score_distribution": dict(r.score_distribution), "recommendations": list(r.recommendations)}


def score_tolerances(rec: Dict[str, object], n_pixels: int) -> Dict[str, float]:
    """How far the three float-bound quantities may move a recorded score (section 5 of the issue, DESIGN K19): the sharpness score is
    variance / 5 (the same relative bound), the noise score 100 - level / 0.3, the overall score 0.3 and 0.25 of them; each chain adds
    a few roundings of values of at most 100 in magnitude, or of the level's 850 before the clamp."""
    sharp, noise = float(rec["sharpness_score"]), float(rec["noise_score"])
    t_sharp = var_bound(n_pixels, sharp) + 4 * U * 100
    level = (100 - noise) * 0.3 if noise > 0 else 255.0
    t_noise = std_bound(n_pixels, level) * (100 / 30) + 4 * U * 850
    return {"sharpness_score": t_sharp, "noise_score": t_noise, "overall_score": 0.3 * t_sharp + 0.25 * t_noise + 8 * U * 100,
            "blur_variance": t_sharp, "noise_level": t_noise + 2 * U * 100}


def assert_score_matches(got: FrameScore, rec: Dict[str, object], n_pixels: int, exact: bool = False) -> None:
    """Every field equal to the record; the sharpness and noise scores and what is formed from them within `score_tolerances`
    (``exact``: those too are equal - the same numpy operations on the same values)."""
    mine = score_record(got)
    tol = score_tolerances(rec, n_pixels)
    for key in ("frame_number", "timestamp", "exposure_score", "artifact_score", "issues"):
        assert mine[key] == rec[key], (key, mine[key], rec[key])
    for key in ("overall_score", "sharpness_score", "noise_score"):
        if exact:
            assert mine[key] == rec[key], (key, mine[key], rec[key])
        assert abs(float(mine[key]) - float(rec[key])) <= tol[key], (key, mine[key], rec[key], tol[key])
    assert sorted(mine["issue_details"]) == sorted(rec["issue_details"])
    for key, value in rec["issue_details"].items():
        if exact:
            assert mine["issue_details"][key] == value, key
        assert abs(float(mine["issue_details"][key]) - float(value)) <= tol[key], (key, mine["issue_details"][key], value)


def assert_report_matches(got: QualityReport, rec: Dict[str, object], n_pixels: int, exact: bool = False) -> None:
    mine = report_record(got)
    for key in ("video_path", "total_frames", "analyzed_frames", "problem_frames", "issue_counts", "score_distribution", "recommendations"):
        assert mine[key] == rec[key], (key, mine[key], rec[key])
    # an overall score moves by at most the largest tolerance of a frame: sharpness 100 and noise level 255 bound every frame's
    tol = score_tolerances({"sharpness_score": "100.0", "noise_score": "0.0"}, max(n_pixels, 1))["overall_score"] + 8 * U * 100
    for key in ("average_score", "min_score", "max_score"):
        if exact:
            assert mine[key] == rec[key], (key, mine[key], rec[key])
        assert abs(float(mine[key]) - float(rec[key])) <= tol, (key, mine[key], rec[key])


# ---- fixtures: seeded, generated, never stored ------------------------------------------------------------------------------------------
def _bgr(plane: np.ndarray, rng=None, chroma: float = 0.0) -> np.ndarray:
    out = np.repeat(plane[:, :, None], 3, axis=2).astype(np.float64)
    if rng is not None and chroma:
        out += rng.normal(0.0, chroma, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _scene(rng, h: int, w: int, texture: float = 9.0, level: float = 128.0) -> np.ndarray:
    """A smooth scene with fine texture: sharp, clean, mid exposure."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = level + 45 * np.sin(x / 6.3 + rng.uniform(0, 6)) * np.cos(y / 4.9 + rng.uniform(0, 6)) + 25 * np.sin((x + y) / 11.0)
    return _bgr(base + rng.normal(0.0, texture, (h, w)), rng, 2.0)


def _blocks(rng, h: int, w: int, amplitude: float, texture: float) -> np.ndarray:
    """8 x 8 blocks of random offsets over fine texture."""
    offs = np.kron(rng.uniform(-amplitude, amplitude, ((h + 7) // 8, (w + 7) // 8)), np.ones((8, 8)))[:h, :w]
    return _bgr(128 + offs + rng.normal(0.0, texture, (h, w)))


def _bands(rng, h: int, w: int, step: int, width: int, ramp: float) -> np.ndarray:
    """Vertical bands `width` columns wide that differ by `step`, on a horizontal ramp of `ramp` per column plus a little noise."""
    x = np.arange(w)
    row = 40 + (x // width) * step + x * ramp
    return _bgr(np.tile(row, (h, 1)) + rng.normal(0.0, 0.6, (h, w)))


def _combed(rng, h: int, w: int, shift: int) -> np.ndarray:
    a = _scene(rng, h, w + shift, texture=2.0)
    out = a[:, :w].copy()
    out[1::2] = a[1::2, shift:shift + w]
    return out


def clips() -> Dict[str, Dict[str, object]]:
    """name -> {frames, fps, and the scorer's and the loop's arguments}.  What each is for is asserted by the generator (`reached`)."""
    rng = np.random.default_rng(20240519)
    H, W = 48, 64
    out: Dict[str, Dict[str, object]] = {}

    def clip(name, frames, fps=25.0, **kw):
        out[name] = {"frames": [np.ascontiguousarray(f) for f in frames], "fps": fps, **kw}

    scene = _scene(rng, H, W)
    smooth = _bgr(np.tile(np.linspace(60, 200, W), (H, 1)) + rng.normal(0, 0.7, (H, W)))
    noisy = _bgr(rng.uniform(0, 255, (H, W)), rng, 20.0)
    over = rng.choice(np.arange(244, 256), size=(H, W, 3), p=np.array([1, 1, 1, 1, 1, 1, 2, 4, 8, 20, 30, 30]) / 100.0).astype(np.uint8)
    under = rng.integers(6, 19, (H, W, 3)).astype(np.uint8)
    black = rng.choice(np.arange(0, 12), size=(H, W, 3), p=np.array([30, 25, 15, 10, 6, 4, 3, 2, 2, 1, 1, 1]) / 100.0).astype(np.uint8)
    clip("issues/48x64", [scene, smooth, noisy, over, under, black, _blocks(rng, H, W, 90, 1.0), _bands(rng, H, W, 14, 8, 0.0),
                          _combed(rng, H, W, 9)])
    # duplicates: the same frame, a near copy below 0.99, the corrupted frames that leave the state alone, a constant thumbnail
    near = np.clip(scene.astype(np.int64) + rng.integers(-60, 61, scene.shape), 0, 255).astype(np.uint8)
    flat = np.full((H, W, 3), 77, np.uint8)
    two = np.zeros((H, W, 3), np.uint8)
    two[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 1] = 255
    clip("duplicates/48x64", [scene, scene.copy(), flat, scene, two, near, scene, _scene(rng, H, W)], fps=30.0)
    hidden = np.full((48, 96, 3), 128, np.uint8)                      # 96 -> 32 columns reads column 3 d + 1 alone: 0 mod 3 is never read
    hidden[:, 0::3] = rng.integers(40, 216, (48, 32, 3))
    clip("constant_thumbnail/48x96", [hidden, hidden.copy(), _scene(rng, 48, 96)])
    # the ratios on both sides of 1 and of their flags
    clip("blocking/48x64", [_blocks(rng, H, W, a, 6.0) for a in (0.0, 5.0, 14.0, 40.0)])
    clip("banding/48x64", [_bands(rng, H, W, 9, 8, r) for r in (2.2, 1.6, 1.2, 0.0)])
    clip("clipping/48x64", [np.where(np.arange(W)[None, :, None] < 8, 0, _scene(rng, H, W)).astype(np.uint8),
                            np.where(np.arange(W)[None, :, None] < 8, 255, _scene(rng, H, W)).astype(np.uint8), _scene(rng, H, W)])
    # the block boundaries: none at all, none in the rows, exactly one row
    clip("no_boundaries/16x16", [_scene(rng, 16, 16), _blocks(rng, 16, 16, 60, 2.0)])
    clip("one_boundary_row/18x26", [_scene(rng, 18, 26), _blocks(rng, 18, 26, 60, 2.0)])
    clip("rows_only/16x40", [_scene(rng, 16, 40)])
    clip("tiny/2x2", [np.array([[[0, 10, 200], [30, 40, 50]], [[60, 70, 80], [90, 100, 110]]], np.uint8)])
    clip("thumbnail_copy/32x32", [_scene(rng, 32, 32), _scene(rng, 32, 32)])
    clip("thumbnail_halved/64x64", [_scene(rng, 64, 64), _scene(rng, 64, 64)])
    clip("poor/48x64", [flat, black, two, _bgr(rng.uniform(0, 255, (H, W)), rng, 20.0)])
    clip("noisy/48x64", [_bgr(rng.uniform(0, 255, (H, W)), rng, 20.0) for _ in range(3)])
    # the loop
    long = [_scene(rng, 32, 48, level=90 + 8 * i) for i in range(7)]
    long[3], long[5] = long[1].copy(), black[:32, :48].copy()
    clip("sampled/32x48", long, fps=24.0, sample_rate=2, start_frame=1)
    clip("window/32x48", long, fps=24.0, sample_rate=3, start_frame=2, end_frame=6, problem_threshold=75.0, total_frames=40)
    clip("no_fps/32x48", long[:2], fps=0.0)
    clip("empty", [], fps=25.0)
    clip("odd_height/33x48", [_scene(rng, 33, 48)], raises="ValueError")
    clip("odd_width/32x47", [_scene(rng, 32, 47)], raises="ValueError")
    return out


def scorer_arguments(c: Dict[str, object]) -> Dict[str, object]:
    return {k: c[k] for k in ("sample_rate", "problem_threshold") if k in c}


def loop_arguments(c: Dict[str, object]) -> Dict[str, object]:
    return {k: c[k] for k in ("total_frames", "start_frame", "end_frame") if k in c}


def reached(js: Dict[str, object]) -> None:
    """The cases the clips exist for, read off the recorded data."""
    c = js["clips"]
    scores = [s for rec in c.values() for s in rec.get("scores", [])]
    for issue in QualityIssue:
        assert any(issue.value in s["issues"] for s in scores) and any(issue.value not in s["issues"] for s in scores), issue
    black = [s for s in scores if "black_frame" in s["issues"]]
    assert black and all(s["exposure_score"] == "0.0" and "underexposed" in s["issues"] for s in black)
    dup = [s["issues"] for s in c["duplicates/48x64"]["scores"]]
    assert dup[2] == ["corrupted"] and dup[4] == ["corrupted"]
    assert [("duplicate" in d) for d in dup] == [False, True, False, True, False, False, False, False]   # [3]: the state skipped [2]
    hidden = c["constant_thumbnail/48x96"]
    assert hidden["statistics_sha256"][0] == hidden["statistics_sha256"][1] and "duplicate" not in hidden["scores"][1]["issues"]
    assert [s["frame_number"] for s in c["sampled/32x48"]["scores"]] == [1, 3, 5] and "duplicate" in c["sampled/32x48"]["scores"][1]["issues"]
    assert [s["frame_number"] for s in c["window/32x48"]["scores"]] == [2, 5] and c["window/32x48"]["report"]["total_frames"] == 40
    assert c["no_fps/32x48"]["scores"][1]["timestamp"] == "0.0"
    assert c["empty"]["report"]["analyzed_frames"] == 0 and c["empty"]["report"]["recommendations"] == [RECOMMENDATIONS["none"]]
    assert c["odd_height/33x48"]["raises"] == c["odd_width/32x47"]["raises"] == "ValueError"
    assert len(block_lines(16)) == 0 and list(block_lines(18)) == [8]
    told = {r for rec in c.values() if "report" in rec for r in rec["report"]["recommendations"]}
    assert all(RECOMMENDATIONS[k] in told for k in ("good", "moderate", "poor", "blur", "noise", "blocking", "interlacing", "banding", "duplicate")), told
