"""Frame quality scoring on frames that are already on the GPU (csrc/quality.hip): per-frame scores and the clip report.

The device form of the reference's `processors/frame_quality_scorer.py` (`FrameQualityScorer` behind `score-frames`): the names,
fields, thresholds, issue order, report and recommendation sentences are the reference's, so a maintainer can bind it
(INTEGRATION.md).  Frames are uint8 CUDA tensors H x W x 3 (BGR) with even sides of 2 .. 16384 pixels.  One pass over a frame's bytes
(`fw_quality_stats_u8`) leaves a few kilobytes of integers on the device - the sums, histograms, block-boundary sums and the 32 x 32
thumbnail that tests/quality_ref.frame_statistics states - and the host epilogue below turns them into the scores in float64.

Wherever the reference's float operations act on exact integers (the mean, both clipping fractions in float32, the running
`block_diff` of per-row means, the ratios) the epilogue runs the same operations in the same order and the fields are equal to the
reference's.  Its np.var of the Laplacian and np.std of the noise plane and of the frame's bytes are pairwise float64 sums over N
values; here they are the exact rational (N S2 - S1^2) / N^2 and its square root, rounded once, which differ from the reference's by
rounding only (DESIGN K19 derives the bound; the sharpness, noise and overall scores carry it).

Deliberately different: gray H x W frames are refused (the reference's Lab conversion needs BGR), and a frame with an odd side is
refused with a ValueError up front, also where the reference would have returned CORRUPTED before its row-pair subtraction raised.
Not built: `analyze_video` from a file (cv2.VideoCapture) - `analyze_frames` is its loop over frames on the device.
"""
from __future__ import annotations

import ctypes as C
import json
import math
from dataclasses import dataclass, field
from enum import Enum
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, contiguous, fetch, upload

BATCH = 32                                       # frames of one launch (the kernel argument table)
MAX_SIDE = 16384
SUMS = 12                                        # int64 a frame (11 used)
THUMB = 32 * 32
_BOUNDS = ((2, MAX_SIDE, 2, MAX_SIDE, "quality: frames of 2 .. 16384 pixels a side expected"),)
_SUM_NAMES = ("lap_sum", "lap_sq_sum", "noise_sum", "noise_sq_sum", "edge_sum", "strong", "weak", "row_pair_sum", "col_pair_sum", "byte_sum",
              "byte_sq_sum")


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


_DISTRIBUTION = (("excellent (90-100)", 90), ("good (70-89)", 70), ("fair (50-69)", 50), ("poor (30-49)", 30), ("bad (0-29)", None))
# the reference's sentences: its public output, which a caller may match on
_SENTENCES = {
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


def block_lines(length: int) -> int:
    """len(range(8, length - 8, 8)): the block-boundary rows or columns of a side."""
    return len(range(8, length - 8, 8))


def generate_recommendations(scores: Sequence[float], issue_counts: Dict[str, int]) -> List[str]:
    """`_generate_recommendations`."""
    if not scores:
        return [_SENTENCES["none"]]
    avg = np.mean(scores)
    out = [_SENTENCES["good"] if avg >= 80 else _SENTENCES["moderate"] if avg >= 50 else _SENTENCES["poor"]]
    total = sum(issue_counts.values())
    for key, share in (("blur", 0.1), ("noise", 0.1), ("blocking", 0.1), ("interlacing", 0.05), ("banding", 0.1)):
        if issue_counts.get(key, 0) > total * share:
            out.append(_SENTENCES[key])
    if issue_counts.get("duplicate", 0) > len(scores) * 0.1:
        out.append(_SENTENCES["duplicate"])
    if issue_counts.get("black_frame", 0) > 0:
        out.append(_SENTENCES["black_frame"].format(n=issue_counts["black_frame"]))
    return out


def _exact_variance(n: int, s1: int, s2: int) -> float:
    """fl((n s2 - s1^2) / n^2): Python's integer division rounds the exact quotient once."""
    return (n * s2 - s1 * s1) / (n * n)


def _exact_std(n: int, s1: int, s2: int) -> float:
    """The square root of that rational, from an integer square root with 128 fractional bits, rounded once."""
    return math.isqrt(((n * s2 - s1 * s1) << 256) // (n * n)) / (1 << 128)


class _Report:
    """The bookkeeping of `analyze_video` around its calls of `score_frame`."""

    def __init__(self, problem_threshold: float):
        self.problem_threshold = problem_threshold
        self.scores: List[float] = []
        self.problem_frames: List[FrameScore] = []
        self.issue_counts = {issue.value: 0 for issue in QualityIssue}

    def add(self, score: FrameScore) -> None:
        self.scores.append(score.overall_score)
        for issue in score.issues:
            self.issue_counts[issue.value] += 1
        if score.overall_score < self.problem_threshold or score.has_issues:
            self.problem_frames.append(score)

    def report(self, video_path: str, total_frames: int) -> QualityReport:
        dist = {name: 0 for name, _ in _DISTRIBUTION}
        for s in self.scores:
            dist[next(name for name, low in _DISTRIBUTION if low is None or s >= low)] += 1
        s = self.scores
        return QualityReport(video_path=str(video_path), total_frames=total_frames, analyzed_frames=len(s),
                             average_score=np.mean(s) if s else 0, min_score=min(s) if s else 0, max_score=max(s) if s else 0,
                             problem_frames=self.problem_frames, issue_counts=self.issue_counts, score_distribution=dist,
                             recommendations=generate_recommendations(s, self.issue_counts))


class DeviceFrameQualityScorer(Stage):
    """The reference's `FrameQualityScorer` on uint8 CUDA frames of one GPU.  Work is queued on torch's current stream of the frames'
    device; `score_frame` waits once for its frame's integers, `analyze_frames` once per batch of 32 sampled frames, `stream` once at
    the end of the stream."""

    BLUR_THRESHOLD = 100
    NOISE_THRESHOLD = 15
    OVEREXPOSED_THRESHOLD = 250
    UNDEREXPOSED_THRESHOLD = 20
    BLACK_FRAME_THRESHOLD = 5
    DUPLICATE_THRESHOLD = 0.99

    def __init__(self, sample_rate: int = 1, problem_threshold: float = 60.0, progress_callback: Optional[Callable[[int, int], None]] = None,
                 gpu_id: int = 0):
        self.sample_rate = max(1, sample_rate)
        self.problem_threshold = problem_threshold
        self.progress_callback = progress_callback
        self.gpu_id = int(gpu_id)
        super().__init__(self.gpu_id)
        self._wrong_device = f"quality: frames on cuda:{self.gpu_id}, the scorer's device, expected"
        self._prev_frame_hash = None

    def reset(self) -> None:
        """Forgets the thumbnail the next frame would be compared with."""
        self._prev_frame_hash = None

    # ---- checks and layout ---------------------------------------------------------------------------------------------------------
    def _check_frames(self, frames: Sequence) -> tuple:
        if len(frames) == 0:
            raise ValueError("quality: at least one frame expected")
        h, w, c = check_frame_list(frames, "quality: frames H x W x 3 (BGR) of one shape expected", _BOUNDS, self._dev,
                                   "quality: uint8 tensors expected", self._wrong_device)
        if c != 3:
            raise ValueError("quality: BGR frames H x W x 3 expected (the Lab measure has no gray form)")
        if h % 2 or w % 2:
            raise ValueError(f"quality: frames with an even number of rows and columns expected, got {w} x {h}")
        return h, w

    @staticmethod
    def statistics_bytes(n: int, h: int, w: int) -> int:
        """Bytes of the statistics of n frames: [n][12] int64, [n][512] uint32, [n][R + C] uint32, [n][1024] uint8."""
        return n * (8 * SUMS + 4 * 512 + 4 * (block_lines(h) + block_lines(w)) + THUMB)

    def _views(self, buf, n: int, h: int, w: int) -> Dict[str, object]:
        import torch
        lines = block_lines(h) + block_lines(w)
        a, b, c = 8 * SUMS * n, 8 * SUMS * n + 2048 * n, 8 * SUMS * n + 2048 * n + 4 * lines * n
        return {"sums": buf[:a].view(torch.int64).view(n, SUMS), "histograms": buf[a:b].view(torch.int32).view(n, 512),
                "block_sums": buf[b:c].view(torch.int32).view(n, lines), "thumbnails": buf[c:c + THUMB * n].view(n, THUMB)}

    def _partial_bytes(self, n: int, h: int, w: int) -> int:
        """Bytes of the scratch the launches of n frames need for their workgroups' partials (a launch takes at most 32 frames, and
        the launches of a call follow each other on one stream, so they share it)."""
        sizes = {min(n, BATCH), n % BATCH or BATCH}
        return max(int(self._lib.fw_quality_scratch_bytes(k, h, w)) for k in sizes)

    def _launch(self, frames: Sequence, buf, h: int, w: int, partials=None) -> Dict[str, object]:
        """Queues the statistics of the (checked, contiguous) frames into ``buf`` and returns its views.  ``partials``: the scratch of
        the launches; None: ``buf`` begins with it (the stage's own scratch holds both)."""
        n, dev = len(frames), frames[0].device
        if partials is None:
            cut = self._partial_bytes(n, h, w)
            partials, buf = buf[:cut], buf[cut:]
        v = self._views(buf, n, h, w)
        lines = block_lines(h) + block_lines(w)
        st = _lib.stream_ptr(dev)
        for b in range(0, n, BATCH):
            part = frames[b:b + BATCH]
            _lib.check(self._lib.fw_quality_stats_u8(
                _lib.ptr_table(part), len(part), h, w, C.c_void_p(partials.data_ptr()), C.c_void_p(v["sums"].data_ptr() + 8 * SUMS * b),
                C.c_void_p(v["histograms"].data_ptr() + 2048 * b), C.c_void_p(v["block_sums"].data_ptr() + 4 * lines * b if lines else buf.data_ptr()),
                C.c_void_p(v["thumbnails"].data_ptr() + THUMB * b), st))
        return v

    # ---- device entries ------------------------------------------------------------------------------------------------------------
    @_lib.on_tensor_device
    def statistics_device(self, frames: Sequence, out=None) -> Dict[str, object]:
        """The integers of every frame, still on the device: {"sums": int64 n x 12, "histograms": int32 n x 512 (gray, then bytes; read
        as uint32), "block_sums": int32 n x (R + C), "thumbnails": uint8 n x 1024}, views of one new buffer or of ``out`` (a contiguous
        uint8 tensor of at least `statistics_bytes` on the frames' device whose address is a multiple of 8)."""
        import torch
        h, w = self._check_frames(frames)
        frames = contiguous(frames)
        need = self.statistics_bytes(len(frames), h, w)
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=frames[0].device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != frames[0].device or not out.is_contiguous() or \
                out.numel() < need or out.data_ptr() % 8:
            raise ValueError(f"quality: out must be a contiguous uint8 tensor of at least {need} bytes on the frames' device, 8-byte aligned")
        return self._launch(frames, out, h, w, self.scratch(self._partial_bytes(len(frames), h, w), frames[0].device))

    def _fetch_statistics(self, views: Dict[str, object], dev, h: int, w: int) -> List[Dict[str, object]]:
        """One wait; a dict per frame in the terms of tests/quality_ref.frame_statistics."""
        sums, hists, blocks, thumbs = fetch(dev, views["sums"], views["histograms"], views["block_sums"], views["thumbnails"])
        hists, blocks = hists.view(np.uint32).astype(np.int64), blocks.view(np.uint32).astype(np.int64)
        rows = block_lines(h)
        out = []
        for i in range(sums.shape[0]):
            s: Dict[str, object] = {name: int(sums[i, k]) for k, name in enumerate(_SUM_NAMES)}
            s.update(gray_hist=hists[i, :256], byte_hist=hists[i, 256:], block_rows=blocks[i, :rows], block_cols=blocks[i, rows:],
                     thumbnail=thumbs[i].copy(), height=h, width=w)
            out.append(s)
        return out

    @_lib.on_tensor_device
    def frame_statistics(self, frames: Sequence) -> List[Dict[str, object]]:
        """`statistics_device`, fetched: a dict of Python integers and NumPy arrays per frame."""
        h, w = self._check_frames(frames)
        frames = contiguous(frames)
        buf = self.scratch(self._partial_bytes(len(frames), h, w) + self.statistics_bytes(len(frames), h, w), frames[0].device)
        return self._fetch_statistics(self._launch(frames, buf, h, w), frames[0].device, h, w)

    # ---- the host epilogue ---------------------------------------------------------------------------------------------------------
    def _score(self, s: Dict[str, object], frame_number: int, fps: float) -> FrameScore:
        """`score_frame` behind its image operations: the reference's float operations, in its order, on the exact integers."""
        f64 = np.float64
        timestamp = frame_number / fps if fps > 0 else 0
        h, w = s["height"], s["width"]
        n = h * w
        # _check_corrupted: np.std of all bytes below 1, or fewer than 10 distinct byte values; the duplicate state is left alone
        if _exact_std(3 * n, s["byte_sum"], s["byte_sq_sum"]) < 1 or int(np.count_nonzero(s["byte_hist"])) < 10:
            return FrameScore(frame_number, timestamp, 0, 0, 0, 0, 0, issues=[QualityIssue.CORRUPTED])
        issues: List[QualityIssue] = []
        details: Dict[str, float] = {}
        # _calculate_sharpness
        variance = f64(_exact_variance(n, s["lap_sum"], s["lap_sq_sum"]))
        sharpness = min(100, (variance / 500) * 100)
        if variance < self.BLUR_THRESHOLD:
            issues.append(QualityIssue.BLUR)
            details["blur_variance"] = sharpness
        # _calculate_noise
        noise_level = f64(_exact_std(n, s["noise_sum"], s["noise_sq_sum"]))
        noise = max(0, 100 - (noise_level / 30) * 100)
        if noise_level > self.NOISE_THRESHOLD:
            issues.append(QualityIssue.NOISE)
            details["noise_level"] = 100 - noise
        # _calculate_exposure: np.mean of uint8 is the exact sum over N; calcHist is float32 counts, summed and divided in float32
        mean = f64(int((s["gray_hist"] * np.arange(256)).sum())) / f64(n)
        if mean < self.BLACK_FRAME_THRESHOLD:
            exposure = 0
            issues += [QualityIssue.UNDEREXPOSED, QualityIssue.BLACK_FRAME]
        else:
            exposure = 100 * (1 - abs(mean - 128) / 128)
            hist = s["gray_hist"].astype(np.float32).reshape(256, 1)
            if np.sum(hist[:5]) / n > 0.05 or np.sum(hist[251:]) / n > 0.05:
                exposure *= 0.8
            exposure = max(0, exposure)
            if mean > self.OVEREXPOSED_THRESHOLD:
                issues.append(QualityIssue.OVEREXPOSED)
            if mean < self.UNDEREXPOSED_THRESHOLD:
                issues.append(QualityIssue.UNDEREXPOSED)
        # _detect_blocking: the running sum of per-line means, rows first, as the reference adds them
        block_diff, count = 0, 0
        for r in s["block_rows"]:
            block_diff += f64(int(r)) / f64(w)
            count += 1
        for c in s["block_cols"]:
            block_diff += f64(int(c)) / f64(h)
            count += 1
        if count > 0:
            block_diff /= count
        edges = f64(s["edge_sum"]) / f64(n)
        ratio = block_diff / edges if edges > 0 else 0
        blocking = max(0, 100 - (ratio - 1) * 50) if ratio > 1 else 100
        if ratio > 1.5:
            issues.append(QualityIssue.BLOCKING)
        # _detect_banding
        ratio = f64(s["strong"]) / f64(s["weak"]) if s["weak"] > 0 else 0
        banding = max(0, 100 - (ratio - 1) * 25) if ratio > 1 else 100
        if ratio > 2:
            issues.append(QualityIssue.BANDING)
        # _detect_interlacing
        mean_diff, mean_col_diff = f64(s["row_pair_sum"]) / f64(n // 2), f64(s["col_pair_sum"]) / f64(n // 2)
        ratio = mean_diff / mean_col_diff if mean_col_diff > 0 else 0
        interlace = max(0, 100 - (ratio - 1) * 30) if ratio > 1 else 100
        if ratio > 1.5 and mean_diff > 10:
            issues.append(QualityIssue.INTERLACING)
        # _check_duplicate
        thumb = s["thumbnail"]
        if self._prev_frame_hash is not None:
            with np.errstate(invalid="ignore", divide="ignore"):      # a constant thumbnail: nan, which is not above the threshold
                if np.corrcoef(thumb, self._prev_frame_hash)[0, 1] > self.DUPLICATE_THRESHOLD:
                    issues.append(QualityIssue.DUPLICATE)
        self._prev_frame_hash = thumb
        artifact = (blocking + banding + interlace) / 3
        overall = sharpness * 0.3 + noise * 0.25 + exposure * 0.25 + artifact * 0.2
        return FrameScore(frame_number, timestamp, overall, sharpness, noise, exposure, artifact, issues, details)

    # ---- the reference's methods -----------------------------------------------------------------------------------------------------
    def score_frame(self, frame, frame_number: int, fps: float) -> FrameScore:
        """Scores one device frame; stateful for duplicates, as the reference is."""
        return self._score(self.frame_statistics([frame])[0], frame_number, fps)

    def analyze_frames(self, frames: Sequence, fps: float, total_frames: Optional[int] = None, start_frame: int = 0,
                       end_frame: Optional[int] = None, video_path: str = "") -> QualityReport:
        """`analyze_video` with ``frames`` (frame k of the video is frames[k]) in the place of the decoder: resets the duplicate state,
        scores every `sample_rate`-th frame from ``start_frame`` up to ``end_frame`` or the end of the list, in batches with one fetch
        of the statistics each."""
        frames = list(frames)
        total_frames = len(frames) if total_frames is None else int(total_frames)
        if end_frame is None:
            end_frame = total_frames
        self.reset()
        picked = [k for k in range(start_frame, min(end_frame, len(frames))) if (k - start_frame) % self.sample_rate == 0] \
            if 0 <= start_frame else []
        collector = _Report(self.problem_threshold)
        for b in range(0, len(picked), BATCH):
            part = picked[b:b + BATCH]
            for k, s in zip(part, self.frame_statistics([frames[k] for k in part])):
                collector.add(self._score(s, k, fps))
                if self.progress_callback:
                    self.progress_callback(k, end_frame)
        return collector.report(video_path, total_frames)

    def stream(self, frames: Iterable, fps: float, on_report: Callable[[QualityReport], None], video_path: str = "") -> Iterator:
        """Yields the frames of an iterator as they are, each scored as it passes: the statistics of every `sample_rate`-th frame are
        queued into a few kilobytes of their own and no frame is kept.  When the iterator ends, one fetch and the host epilogue build
        the report `analyze_frames` gives for the whole clip, and ``on_report`` receives it; a stream that is abandoned reports nothing."""
        import torch
        self.reset()
        pending, shape, count = [], None, 0
        for k, f in enumerate(frames):
            count = k + 1
            if k % self.sample_rate == 0:
                with torch.cuda.device(f.device):
                    h, w = self._check_frames([f])
                    g = contiguous([f])
                    if shape not in (None, (h, w)):
                        raise ValueError("quality: frames H x W x 3 (BGR) of one shape expected")
                    shape = (h, w)
                    buf = torch.empty(self.statistics_bytes(1, h, w), dtype=torch.uint8, device=f.device)
                    pending.append((k, self._launch(g, buf, h, w, self.scratch(self._partial_bytes(1, h, w), f.device))))
            yield f
        collector = _Report(self.problem_threshold)
        if pending:
            dev = pending[0][1]["sums"].device
            with torch.cuda.device(dev):
                merged = {key: torch.cat([v[key] for _, v in pending]) for key in ("sums", "histograms", "block_sums", "thumbnails")}
                for (k, _), s in zip(pending, self._fetch_statistics(merged, dev, *shape)):
                    collector.add(self._score(s, k, fps))
                    if self.progress_callback:
                        self.progress_callback(k, count)
        on_report(collector.report(video_path, count))

    # ---- numpy in ------------------------------------------------------------------------------------------------------------------
    def score_frame_host(self, frame: np.ndarray, frame_number: int, fps: float) -> FrameScore:
        with self.host() as dev:
            return self.score_frame(upload(frame, dev), frame_number, fps)

    def analyze_frames_host(self, frames: Sequence[np.ndarray], fps: float, **kwargs) -> QualityReport:
        """`analyze_frames` on NumPy frames: only the sampled frames of the window are uploaded."""
        with self.host() as dev:
            start, rate = int(kwargs.get("start_frame", 0)), self.sample_rate
            return self.analyze_frames([upload(f, dev) if k >= start and (k - start) % rate == 0 else None for k, f in enumerate(frames)],
                                       fps, **kwargs)
