"""VHS artifact repair and analysis on frames that are already on the GPU (csrc/vhs.hip), behind the deinterlacer and in front of every
other stage.

The device form of the reference's `processors/format/vhs.py` (`VHSProcessor` on lists of frames): the names, fields, defaults and
decisions are the reference's, so a maintainer can bind it.  Frames are uint8 CUDA tensors H x W x 3 (BGR) or H x W
with H >= 32.  The five frame methods and `process` are byte-equal to the reference's own functions through tests/vhs_ref.py.  Each
step runs over the whole list before the next one starts, as in the reference: the device forms the statistics of all frames of a
step (exact integers, or the 30 gray rows a float32 variance is taken over), the host waits once, takes the decisions with the
reference's NumPy steps and queues the rewrite (DESIGN K17).  A method that changes nothing returns the list or the tensor it got.

Not built: `processors/vhs_restoration.py` (ffmpeg throughout) and the ffmpeg check of `VHSProcessor.__init__`.  `dot_crawl_removal`,
`jitter_correction` and `color_phase_correction` are fields of the configuration that nothing reads, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._stage import ANY, Stage, check_frame_list, check_no_overlap, contiguous, upload

logger = logging.getLogger(__name__)

BATCH = 32                                       # frames of one launch that writes frames (the kernel argument table)
TABLE = 64                                       # frames a dropout batch and its temporal neighbours may span
BOTTOM_ROWS = 30
MAX_SIDE = 16384
DEFAULT_RUN_CAPACITY = 8192
_BOUNDS = ((32, ANY, 0, ANY, "vhs: frames of at least 32 rows expected (below 31 the reference's bottom region wraps round)"),
           (0, MAX_SIDE, 2, MAX_SIDE, "vhs: frames of 2 .. 16384 columns and at most 16384 rows expected"))


class VHSQuality(Enum):
    SP = "sp"
    LP = "lp"
    EP = "ep"
    UNKNOWN = "unknown"

    @property
    def horizontal_resolution(self) -> int:
        return {VHSQuality.SP: 240, VHSQuality.LP: 220, VHSQuality.EP: 200, VHSQuality.UNKNOWN: 240}.get(self, 240)


class ArtifactType(Enum):
    HEAD_SWITCHING = "head_switching"
    TRACKING_ERROR = "tracking_error"
    DROPOUT = "dropout"
    CHROMA_BLEED = "chroma_bleed"
    RAINBOW = "rainbow"
    DOT_CRAWL = "dot_crawl"
    JITTER = "jitter"
    COLOR_PHASE = "color_phase"


@dataclass
class VHSConfig:
    """The reference's fields, defaults and validation.  `dot_crawl_removal`, `jitter_correction` and `color_phase_correction` are
    carried and never read, as in the reference."""
    tracking: float = 0.5
    head_switching: float = 0.7
    chroma_bleed: float = 0.5
    rainbow_removal: float = 0.5
    dropout_repair: float = 0.6
    dot_crawl_removal: float = 0.5
    jitter_correction: float = 0.5
    color_phase_correction: float = 0.0
    head_switch_height: int = 16
    dropout_min_length: int = 5
    temporal_radius: int = 3
    preserve_authentic: bool = True
    quality_mode: VHSQuality = VHSQuality.UNKNOWN

    def __post_init__(self):
        for attr in ["tracking", "head_switching", "chroma_bleed", "rainbow_removal", "dropout_repair", "dot_crawl_removal",
                     "jitter_correction"]:
            val = getattr(self, attr)
            if not 0.0 <= val <= 1.0:
                raise ValueError(f"{attr} must be between 0.0 and 1.0")


@dataclass
class VHSArtifactInfo:
    artifact_type: ArtifactType
    severity: float = 0.0
    location: Optional[Tuple[int, int, int, int]] = None             # x, y, w, h
    confidence: float = 0.0


@dataclass
class VHSAnalysis:
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
    detected_quality: VHSQuality = VHSQuality.UNKNOWN
    all_artifacts: List[VHSArtifactInfo] = field(default_factory=list)

    def summary(self) -> str:
        issues = []
        if self.head_switching_detected:
            issues.append(f"Head switching ({self.head_switching_severity*100:.0f}%)")
        if self.tracking_errors:
            issues.append(f"Tracking errors ({self.tracking_severity*100:.0f}%)")
        if self.dropout_detected:
            issues.append(f"{self.dropout_count} dropouts")
        if self.chroma_bleed:
            issues.append(f"Chroma bleed ({self.chroma_bleed_severity*100:.0f}%)")
        if self.rainbow_effect:
            issues.append("Rainbow effect")
        if self.dot_crawl:
            issues.append("Dot crawl")
        if self.jitter_detected:
            issues.append(f"Jitter ({self.jitter_severity*100:.0f}%)")
        issue_str = ", ".join(issues) if issues else "No significant issues"
        return (f"VHS Quality: {self.detected_quality.value.upper()}\n"
                f"Overall degradation: {self.overall_degradation*100:.0f}%\n"
                f"Issues: {issue_str}")


# ---- the reference's host logic on a few values per frame ---------------------------------------------------------------------------
def _head_switching_decision(bottom: np.ndarray, height: int) -> Tuple[bool, Optional[int], float]:
    """``bottom``: the last 30 gray rows (uint8).  The reference's expression itself: np.var squares and rounds in float32."""
    row_variances = np.var(np.diff(bottom.astype(np.float32), axis=1), axis=1)
    threshold = np.mean(row_variances) * 2.5
    noisy_rows = np.where(row_variances > threshold)[0]
    if len(noisy_rows) > 2:
        return True, height - BOTTOM_ROWS + int(np.min(noisy_rows)), min(1.0, len(noisy_rows) / 15.0)
    return False, None, 0.0


def _tracking_decision(row_sums: np.ndarray, height: int, width: int) -> Tuple[bool, float, List[int]]:
    """``row_sums``: exact int64 sums of |diff gray| per row; float32(sum) / float32(W - 1) is the reference's float32 row mean."""
    row_activity = row_sums.astype(np.float32) / np.float32(width - 1)
    smoothed = np.convolve(row_activity, np.ones(5) / 5, mode="same")
    local_deviation = np.abs(row_activity - smoothed)
    threshold = np.std(local_deviation) * 2.5
    lines = [int(y) for y in np.where(local_deviation > threshold)[0].tolist() if y < height - BOTTOM_ROWS]
    if len(lines) > 0:
        return True, min(1.0, len(lines) / 20.0), lines
    return False, 0.0, []


def _merge_dropouts(dropouts: Sequence[Tuple[int, int, int, int]]) -> List[Tuple[int, int, int, int]]:
    """The reference's greedy merge of runs (x, y, w, h) into bounding boxes; sequential by nature, so it stays on the host."""
    if not dropouts:
        return []
    ordered = sorted(dropouts, key=lambda d: (d[1], d[0]))
    merged = []
    cur = list(ordered[0])
    for d in ordered[1:]:
        if d[1] <= cur[1] + cur[3] + 1 and d[0] < cur[0] + cur[2] and d[0] + d[2] > cur[0]:
            new_x = min(cur[0], d[0])
            cur = [new_x, cur[1], max(cur[0] + cur[2], d[0] + d[2]) - new_x, d[1] + d[3] - cur[1]]
        else:
            merged.append(tuple(cur))
            cur = list(d)
    merged.append(tuple(cur))
    return merged


def _dot_crawl_decision(column_sums: np.ndarray, height: int) -> bool:
    row_means = column_sums.astype(np.float32) / np.float32(height)
    if len(row_means) < 10:
        return False
    fft = np.fft.fft(row_means)
    magnitude = np.abs(fft[1:len(fft) // 2])
    if len(magnitude) == 0:
        return False
    return bool(np.max(magnitude) > np.mean(magnitude) * 8)


def _jitter_decision(shifts: np.ndarray) -> Tuple[bool, float]:
    shift_variance = np.var(shifts)
    if shift_variance > 2.0:
        return True, min(1.0, shift_variance / 10.0)
    return False, 0.0


def _calculate_degradation(a: VHSAnalysis) -> float:
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


def _estimate_quality(a: VHSAnalysis, width: int) -> VHSQuality:
    if a.overall_degradation > 0.6:
        return VHSQuality.EP
    if a.overall_degradation > 0.3:
        return VHSQuality.LP
    if width >= 720:
        return VHSQuality.SP
    return VHSQuality.UNKNOWN


def _repair_groups(ops: Sequence[tuple]) -> List[List[tuple]]:
    """Splits a frame's repairs (mode, source, x, y, w, h), which the reference applies one after the other, into consecutive groups
    whose boxes - with the two flank columns a spatial repair reads - are pairwise disjoint: a group is one launch."""
    groups: List[List[tuple]] = []
    rects: List[tuple] = []
    for op in ops:
        mode, _, x, y, w, h = op
        rect = (x - 1, y, x + w + 1, y + h) if mode == 1 else (x, y, x + w, y + h)
        if groups and all(rect[2] <= r[0] or r[2] <= rect[0] or rect[3] <= r[1] or r[3] <= rect[1] for r in rects):
            groups[-1].append(op)
            rects.append(rect)
        else:
            groups.append([op])
            rects = [rect]
    return groups


class DeviceVHSProcessor(Stage):
    """The reference's `VHSProcessor` on uint8 CUDA frames of one GPU.  Work is queued on torch's current stream of the frames' device.
    ``rng``: what the chroma detector's `choice` is drawn from - None is NumPy's global generator, which the reference uses, so a
    seeded run consumes it exactly as the reference does; a `np.random.RandomState` keeps the draws to the caller."""

    def __init__(self, config: Optional[VHSConfig] = None, device_id: int = 0, rng=None):
        self.config = config or VHSConfig()
        self.device_id = int(device_id)
        self.rng = rng
        super().__init__(self.device_id)
        self._wrong_device = f"vhs: frames on cuda:{self.device_id}, the processor's device, expected"

    # ---- checks --------------------------------------------------------------------------------------------------------------------
    def _check_frames(self, frames: Sequence) -> tuple:
        return check_frame_list(frames, "vhs: frames H x W x 3 (BGR) or H x W of one shape expected", _BOUNDS, self._dev,
                                "vhs: uint8 tensors expected", self._wrong_device)

    # ---- device entries: queue, and (where they return NumPy arrays) wait once -------------------------------------------------------
    @_lib.on_tensor_device
    def gray_stats_device(self, frames: Sequence, sums: bool = False, bottom: bool = False, runs: bool = False,
                          run_capacity: Optional[int] = None) -> dict:
        """{"row_sums": int64 n x H, "bottom": uint8 n x 30 x W, "runs": int32 k x 4 (frame, x, y, length) in no particular order} of
        what was asked for, as NumPy arrays.  The run list has a capacity; the entry reports the true count, and on overflow the list
        is allocated again with that count and the statistics run again."""
        import torch
        frames = contiguous(frames)
        h, w, c = self._check_frames(frames)
        n, dev = len(frames), frames[0].device
        t_sums = torch.empty((n, h), dtype=torch.int64, device=dev) if sums else None
        t_bottom = torch.empty((n, BOTTOM_ROWS, w), dtype=torch.uint8, device=dev) if bottom else None
        cap = int(run_capacity or DEFAULT_RUN_CAPACITY)
        out: dict = {}
        while True:
            t_runs = torch.empty((1 + 4 * cap,), dtype=torch.int32, device=dev) if runs else None      # [0] is the counter
            _lib.check(self._lib.fw_vhs_gray_stats_u8(
                _lib.ptr_table(frames), n, h, w, c, int(self.config.dropout_min_length),
                _lib.ptr(t_sums) if sums else None, _lib.ptr(t_bottom) if bottom else None,
                C.c_void_p(t_runs.data_ptr() + 4) if runs else None, cap, _lib.ptr(t_runs) if runs else None,
                _lib.stream_ptr(dev)))
            if not runs:
                break
            fetched = t_runs.cpu().numpy()                            # the wait of this batch
            count = int(fetched[0])
            if count <= cap:
                out["runs"] = fetched[1:1 + 4 * count].reshape(count, 4)
                break
            cap = count                                               # overflow: the entry returned the true count
        if sums:
            out["row_sums"] = t_sums.cpu().numpy()
        if bottom:
            out["bottom"] = t_bottom.cpu().numpy()
        return out

    @_lib.on_tensor_device
    def blend_rows_device(self, srcs: Sequence, dsts: Sequence, spec_rows: np.ndarray, spec_factors: np.ndarray) -> None:
        """dsts[f][y] = fa * ((srcs[f][y1] + srcs[f][y2]) / 2) + fb * srcs[f][y] for every table row (f, y, y1, y2), (fa, fb)."""
        h, w, c = self._check_frames(list(srcs) + list(dsts))
        check_no_overlap(dsts, srcs, "vhs")
        dev = srcs[0].device
        rows = upload(np.asarray(spec_rows, dtype=np.int32).reshape(-1, 4), dev)
        fac = upload(np.asarray(spec_factors, dtype=np.float32).reshape(-1, 2), dev)
        _lib.check(self._lib.fw_vhs_blend_rows_u8(_lib.ptr_table(srcs), _lib.ptr_table(dsts), len(srcs), h, w * c, _lib.ptr(rows),
                                                  _lib.ptr(fac), int(rows.shape[0]), _lib.stream_ptr(dev)))

    @_lib.on_tensor_device
    def rainbow_device(self, frames: Sequence, strength: float, outs: Optional[Sequence] = None) -> List:
        """The rainbow stencil and blend of BGR frames into new tensors (or ``outs``, which must not overlap any source)."""
        frames = contiguous(frames)
        h, w, c = self._check_frames(frames)
        if c != 3:
            raise ValueError("vhs: BGR frames expected")
        if outs is None:
            outs = _lib.empty_like_many(frames)
        else:
            outs = list(outs)
            if len(outs) != len(frames) or any(not o.is_contiguous() for o in outs):
                raise ValueError("vhs: one contiguous destination per frame expected")
            self._check_frames(frames + outs)
        check_no_overlap(outs, frames, "vhs")
        fa, fb = float(np.float32(strength)), float(np.float32(1 - strength))
        st = _lib.stream_ptr(frames[0].device)
        for b in range(0, len(frames), BATCH):
            src, dst = frames[b:b + BATCH], outs[b:b + BATCH]
            _lib.check(self._lib.fw_vhs_rainbow_u8(_lib.ptr_table(src), _lib.ptr_table(dst), len(src), h, w, fa, fb, st))
        return list(outs)

    @_lib.on_tensor_device
    def box_sums_device(self, frames: Sequence, tasks: np.ndarray) -> np.ndarray:
        """int64 sums of gray over boxes (frame, x, y, w, h) of at most 64 frames."""
        import torch
        h, w, c = self._check_frames(frames)
        dev = frames[0].device
        t = upload(np.asarray(tasks, dtype=np.int32).reshape(-1, 5), dev)
        sums = torch.empty((int(t.shape[0]),), dtype=torch.int64, device=dev)
        _lib.check(self._lib.fw_vhs_box_gray_sums_u8(_lib.ptr_table(frames), len(frames), h, w, c, _lib.ptr(t), int(t.shape[0]),
                                                     _lib.ptr(sums), _lib.stream_ptr(dev)))
        return sums.cpu().numpy()

    @_lib.on_tensor_device
    def repair_device(self, sources: Sequence, results: Sequence, boxes: np.ndarray, strength: float) -> None:
        """Boxes (mode, result, source, x, y, w, h, 0) rewritten in place in ``results``; disjoint within a result frame."""
        h, w, c = self._check_frames(list(sources) + list(results))
        check_no_overlap(results, sources, "vhs")
        dev = results[0].device
        t = upload(np.asarray(boxes, dtype=np.int32).reshape(-1, 8), dev)
        _lib.check(self._lib.fw_vhs_dropout_repair_u8(_lib.ptr_table(sources), len(sources), _lib.ptr_table(results), len(results), h, w, c,
                                                      _lib.ptr(t), int(t.shape[0]), float(strength), _lib.stream_ptr(dev)))

    @_lib.on_tensor_device
    def edge_counts_device(self, frames: Sequence) -> np.ndarray:
        import torch
        h, w, c = self._check_frames(frames)
        counts = torch.empty((len(frames), h), dtype=torch.int32, device=frames[0].device)
        _lib.check(self._lib.fw_vhs_edge_counts_u8(_lib.ptr_table(frames), len(frames), h, w, _lib.ptr(counts),
                                                   _lib.stream_ptr(frames[0].device)))
        return counts.cpu().numpy()

    @_lib.on_tensor_device
    def chroma_samples_device(self, frames: Sequence, samples: np.ndarray) -> np.ndarray:
        import torch
        h, w, c = self._check_frames(frames)
        dev = frames[0].device
        t = upload(np.asarray(samples, dtype=np.int32).reshape(-1, 3), dev)
        out = torch.empty((int(t.shape[0]), 2), dtype=torch.int32, device=dev)
        _lib.check(self._lib.fw_vhs_chroma_samples_u8(_lib.ptr_table(frames), len(frames), h, w, _lib.ptr(t), int(t.shape[0]),
                                                      _lib.ptr(out), _lib.stream_ptr(dev)))
        return out.cpu().numpy()

    @_lib.on_tensor_device
    def chroma_shift_device(self, frames: Sequence, shifts: Sequence[int]) -> List:
        h, w, c = self._check_frames(frames)
        outs = _lib.empty_like_many(frames)
        check_no_overlap(outs, frames, "vhs")
        table = (C.c_int32 * len(frames))(*[int(s) for s in shifts])
        _lib.check(self._lib.fw_vhs_chroma_shift_u8(_lib.ptr_table(frames), _lib.ptr_table(outs), table, len(frames), h, w, _lib.stream_ptr(frames[0].device)))
        return outs

    @_lib.on_tensor_device
    def analysis_device(self, frame) -> dict:
        """{"column_sums": int64 W - 1, "jitter_shifts": int32, "rainbow": (diag_max, mean_mag)} of a frame; the first and the last for
        BGR frames only.  The saturation map is the kernel's; its transform is torch.fft.fft2 on the device, and the two magnitudes
        come back as float64."""
        import torch
        h, w, c = self._check_frames([frame])
        dev, st = frame.device, _lib.stream_ptr(frame.device)
        out: dict = {}
        shifts = torch.empty(((h + 2) // 5,), dtype=torch.int32, device=dev)
        _lib.check(self._lib.fw_vhs_jitter_shifts_u8(_lib.ptr(frame), h, w, c, _lib.ptr(shifts), st))
        if c == 3:
            sums = torch.empty((w - 1,), dtype=torch.int64, device=dev)
            _lib.check(self._lib.fw_vhs_column_sums_u8(_lib.ptr(frame), h, w, _lib.ptr(sums), st))
            sat = torch.empty((h, w), dtype=torch.float64, device=dev)
            _lib.check(self._lib.fw_vhs_saturation_f64(_lib.ptr(frame), h, w, _lib.ptr(sat), st))
            magnitude = torch.abs(torch.fft.fft2(sat))
            pair = torch.stack([magnitude[h // 4:h // 2, w // 4:w // 2].max(), magnitude.mean()]).cpu().numpy()
            out["rainbow"] = (float(pair[0]), float(pair[1]))
            out["column_sums"] = sums.cpu().numpy()
        out["jitter_shifts"] = shifts.cpu().numpy()
        return out

    # ---- the reference's methods ---------------------------------------------------------------------------------------------------------
    def _strength(self, strength: Optional[float], name: str) -> float:
        return strength if strength is not None else getattr(self.config, name)

    @staticmethod
    def _progress(cb, n: int) -> None:
        if cb:
            for i in range(n):
                cb((i + 1) / n)

    def _blend_step(self, frames: List, decide) -> List:
        """A step that rewrites rows: ``decide(i)`` gives None (the frame is returned as it is) or the rows (y, y1, y2, fa, fb) of
        frame i to rewrite in a copy of it.  One launch per 32 frames."""
        result = list(frames)
        for b in range(0, len(frames), BATCH):
            srcs, dsts, rows, factors = [], [], [], []
            for i in range(b, min(len(frames), b + BATCH)):
                spec = decide(i)
                if spec is None:
                    continue
                src = frames[i] if frames[i].is_contiguous() else frames[i].contiguous()
                result[i] = src.clone()
                if spec:
                    k = len(srcs)
                    srcs.append(src), dsts.append(result[i])
                    rows += [(k, y, y1, y2) for y, y1, y2, _, _ in spec]
                    factors += [(np.float32(fa), np.float32(fb)) for _, _, _, fa, fb in spec]
            if rows:
                self.blend_rows_device(srcs, dsts, np.array(rows, dtype=np.int32), np.array(factors, dtype=np.float32))
        return result

    def remove_head_switching(self, frames: List, strength: Optional[float] = None, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        strength = self._strength(strength, "head_switching")
        if strength <= 0:
            return frames
        h, w, _ = self._check_frames(frames)
        bottoms = np.concatenate([self.gray_stats_device(frames[b:b + BATCH], bottom=True)["bottom"] for b in range(0, len(frames), BATCH)])
        bh = self.config.head_switch_height

        def decide(i):
            detected, position, _ = _head_switching_decision(bottoms[i], h)
            if not detected:
                return None
            spec = []
            if position > bh:
                for y in range(position, min(h, position + bh)):
                    fa = strength * (1.0 - (y - position) / bh)
                    sy = position - bh + (y - position) % bh
                    if 0 <= sy < h:
                        spec.append((y, sy, sy, fa, 1 - fa))
            return spec

        result = self._blend_step(frames, decide)
        self._progress(progress_callback, len(frames))
        return result

    def fix_tracking_errors(self, frames: List, strength: Optional[float] = None, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        strength = self._strength(strength, "tracking")
        if strength <= 0:
            return frames
        h, w, _ = self._check_frames(frames)
        sums = np.concatenate([self.gray_stats_device(frames[b:b + BATCH], sums=True)["row_sums"] for b in range(0, len(frames), BATCH)])

        def decide(i):
            lines = _tracking_decision(sums[i], h, w)[2]
            if not lines:
                return None
            return [(y, y - 1, y + 1, strength, 1 - strength) for y in lines if 0 < y < h - 1]

        result = self._blend_step(frames, decide)
        self._progress(progress_callback, len(frames))
        return result

    def _dropout_boxes(self, frames: Sequence, run_capacity: Optional[int]) -> List[List[tuple]]:
        runs = self.gray_stats_device(frames, runs=True, run_capacity=run_capacity)["runs"]
        per_frame: List[List[tuple]] = [[] for _ in frames]
        for f, x, y, length in runs.tolist():
            per_frame[f].append((x, y, length, 1))
        return [_merge_dropouts(r) for r in per_frame]

    def _fix_dropout_core(self, frames: List, start: int, stop: int, strength: float, run_capacity: Optional[int] = None) -> List:
        """`fix_dropout` for frames[start:stop] with the temporal neighbours taken from ``frames``."""
        r = int(self.config.temporal_radius)
        if 2 * r + 1 > TABLE:
            raise ValueError(f"vhs: a temporal_radius of at most {(TABLE - 1) // 2} is supported")
        n = len(frames)
        step = max(1, min(BATCH, TABLE - 2 * r))
        result = []
        for b0 in range(start, stop, step):
            b1 = min(stop, b0 + step)
            lo, hi = max(0, b0 - r), min(n, b1 + r)
            window = contiguous(frames[lo:hi])
            boxes = self._dropout_boxes(window[b0 - lo:b1 - lo], run_capacity)
            tasks, owners = [], []
            for i in range(b0, b1):
                cands = list(range(max(0, i - r), i)) + list(range(i + 1, min(n, i + 1 + r)))        # oldest previous frame first
                for k, (x, y, w, h) in enumerate(boxes[i - b0]):
                    for cnd in cands:
                        tasks.append((cnd - lo, x, y, w, h))
                        owners.append((i, k))
            sums = self.box_sums_device(window, np.array(tasks, dtype=np.int32)) if tasks else np.zeros((0,), dtype=np.int64)
            clean: dict = {}
            for (i, k), task, s in zip(owners, tasks, sums.tolist()):
                npx = task[3] * task[4]
                if (i, k) not in clean and 10 * npx < s < 245 * npx:  # the mean of the box strictly between 10 and 245, in integers
                    clean[(i, k)] = task[0]
            outs, levels = [], []
            for i in range(b0, b1):
                if not boxes[i - b0]:
                    outs.append(frames[i])
                    continue
                outs.append(window[i - lo].clone())
                ops = []
                for k, (x, y, w, h) in enumerate(boxes[i - b0]):
                    if (i, k) in clean:
                        ops.append((0, clean[(i, k)], x, y, w, h))
                    elif x > 0 and x + w < int(frames[i].shape[1]):
                        ops.append((1, 0, x, y, w, h))
                for level, group in enumerate(_repair_groups(ops)):
                    while len(levels) <= level:
                        levels.append([])
                    levels[level] += [(mode, i - b0, src, x, y, w, h, 0) for mode, src, x, y, w, h in group]
            for level in levels:                                      # one launch per group level, all frames of the batch together
                used = sorted({e[1] for e in level})
                slot = {f: j for j, f in enumerate(used)}
                table = np.array([(m, slot[f], s, x, y, w, h, 0) for m, f, s, x, y, w, h, _ in level], dtype=np.int32)
                self.repair_device(window, [outs[f] for f in used], table, strength)
            result += outs
        return result

    def fix_dropout(self, frames: List, strength: Optional[float] = None, progress_callback: Optional[Callable[[float], None]] = None,
                    _run_capacity: Optional[int] = None) -> List:
        if not frames:
            return frames
        strength = self._strength(strength, "dropout_repair")
        if strength <= 0:
            return frames
        self._check_frames(frames)
        result = self._fix_dropout_core(list(frames), 0, len(frames), strength, _run_capacity)
        self._progress(progress_callback, len(frames))
        return result

    def _detect_chroma_bleed_batch(self, frames: Sequence) -> List[Tuple[bool, float]]:
        """`_detect_chroma_bleed` of up to 32 BGR frames: one wait for the edge counts, the draws in frame order, one wait for the
        samples."""
        rng = self.rng if self.rng is not None else np.random
        counts = self.edge_counts_device(frames).astype(np.int64)
        samples, spans = [], []
        for i in range(len(frames)):
            n_edges = int(counts[i].sum())
            if n_edges < 10:
                spans.append(None)
                continue
            idx = np.asarray(rng.choice(n_edges, min(100, n_edges), replace=False), dtype=np.int64)
            cum = np.cumsum(counts[i])
            rows = np.searchsorted(cum, idx, side="right")           # np.where(edge_mask) lists the edges row by row
            ks = idx - (cum[rows] - counts[i][rows])
            spans.append((len(samples), len(idx)))
            samples += [(i, int(y), int(k)) for y, k in zip(rows, ks)]
        offsets = self.chroma_samples_device(frames, np.array(samples, dtype=np.int32)) if samples else None
        out = []
        for span in spans:
            if span is None:
                out.append((False, 0.0))
                continue
            got = offsets[span[0]:span[0] + span[1]].reshape(-1)
            if (got < -1).any():
                raise _lib.FramewrightHipError(_lib.FW_ERR_INTERNAL, "vhs: a chroma sample named no edge (edge counts and samples disagree)")
            valid = [int(o) for o in got if o >= 0]
            if valid:
                mean_offset = np.mean(valid)
                if mean_offset > 1.5:
                    out.append((True, min(1.0, mean_offset / 5.0)))
                    continue
            out.append((False, 0.0))
        return out

    def reduce_chroma_bleed(self, frames: List, strength: Optional[float] = None, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        strength = self._strength(strength, "chroma_bleed")
        if strength <= 0:
            return frames
        _, _, c = self._check_frames(frames)
        result = list(frames)
        if c == 3:
            for b in range(0, len(frames), BATCH):
                batch = contiguous(frames[b:b + BATCH])
                found = self._detect_chroma_bleed_batch(batch)
                move, shifts = [], []
                for i, (detected, severity) in enumerate(found):
                    if not detected:
                        continue
                    shift = int(severity * 2 * strength)
                    if shift > 0:
                        move.append(i), shifts.append(shift)
                    else:
                        result[b + i] = batch[i].clone()             # the reference returns a copy here
                if move:
                    for i, o in zip(move, self.chroma_shift_device([batch[i] for i in move], shifts)):
                        result[b + i] = o
        self._progress(progress_callback, len(frames))
        return result

    def remove_rainbow_artifacts(self, frames: List, strength: Optional[float] = None, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        strength = self._strength(strength, "rainbow_removal")
        if strength <= 0:
            return frames
        _, _, c = self._check_frames(frames)
        result = self.rainbow_device(frames, strength) if c == 3 else list(frames)
        self._progress(progress_callback, len(frames))
        return result

    def process(self, frames: List, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        total_steps = 5
        current_step = 0

        def step_callback(progress: float):
            if progress_callback:
                progress_callback((current_step + progress) / total_steps)

        if self.config.head_switching > 0:
            frames = self.remove_head_switching(frames, progress_callback=step_callback)
        current_step += 1
        if self.config.tracking > 0:
            frames = self.fix_tracking_errors(frames, progress_callback=step_callback)
        current_step += 1
        if self.config.dropout_repair > 0:
            frames = self.fix_dropout(frames, progress_callback=step_callback)
        current_step += 1
        if self.config.chroma_bleed > 0:
            frames = self.reduce_chroma_bleed(frames, progress_callback=step_callback)
        current_step += 1
        if self.config.rainbow_removal > 0:
            frames = self.remove_rainbow_artifacts(frames, progress_callback=step_callback)
        current_step += 1
        if progress_callback:
            progress_callback(1.0)
        return frames

    def stream(self, frames: Iterable, block: int = 8) -> Iterator:
        """`process` over an iterator, ``block`` frames at a time: the same bytes as the whole-list call.  Steps 1, 2, 4 and 5 are per
        frame; the dropout repair keeps `temporal_radius` frames of its input on both sides.  The chroma detector draws in frame order,
        as the whole-list call does."""
        if block < 1:
            raise ValueError("block must be >= 1")
        cfg = self.config
        r = int(cfg.temporal_radius) if cfg.dropout_repair > 0 else 0
        held: List = []                                               # the dropout step's input from frame `base` on
        base = done = n_in = 0
        it = iter(frames)
        eof = False
        while not eof:
            chunk = []
            while len(chunk) < block:
                f = next(it, None)
                if f is None:
                    eof = True
                    break
                chunk.append(f)
            if chunk:
                self._check_frames(([held[-1]] if held else []) + chunk)
                if cfg.head_switching > 0:
                    chunk = self.remove_head_switching(chunk)
                if cfg.tracking > 0:
                    chunk = self.fix_tracking_errors(chunk)
                held += chunk
                n_in += len(chunk)
            ready = n_in if eof else max(done, n_in - r)
            if ready > done:
                outs = self._fix_dropout_core(held, done - base, ready - base, cfg.dropout_repair) if cfg.dropout_repair > 0 else held[done - base:ready - base]
                if cfg.chroma_bleed > 0:
                    outs = self.reduce_chroma_bleed(outs)
                if cfg.rainbow_removal > 0:
                    outs = self.remove_rainbow_artifacts(outs)
                yield from outs
                done = ready
                keep = max(base, done - r)
                held, base = held[keep - base:], keep

    def detect_vhs_artifacts(self, frame: Any, _run_capacity: Optional[int] = None) -> VHSAnalysis:
        analysis = VHSAnalysis()
        if frame is None:
            return analysis
        height, width, c = self._check_frames([frame])
        frame = frame if frame.is_contiguous() else frame.contiguous()
        stats = self.gray_stats_device([frame], sums=True, bottom=True, runs=True, run_capacity=_run_capacity)
        extra = self.analysis_device(frame)

        hs_detected, hs_position, hs_severity = _head_switching_decision(stats["bottom"][0], height)
        analysis.head_switching_detected, analysis.head_switching_position, analysis.head_switching_severity = hs_detected, hs_position, hs_severity
        if hs_detected:
            analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.HEAD_SWITCHING, hs_severity, (0, hs_position or 0, width, self.config.head_switch_height), 0.9))

        tr_detected, tr_severity, tr_positions = _tracking_decision(stats["row_sums"][0], height, width)
        analysis.tracking_errors, analysis.tracking_severity, analysis.tracking_line_positions = tr_detected, tr_severity, tr_positions
        for pos in tr_positions:
            analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.TRACKING_ERROR, tr_severity, (0, pos, width, 1), 0.8))

        merged = _merge_dropouts([(x, y, length, 1) for _, x, y, length in stats["runs"].tolist()])
        analysis.dropout_detected, analysis.dropout_count, analysis.dropout_positions = len(merged) > 0, len(merged), merged
        for pos in merged:
            analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.DROPOUT, 0.8, pos, 0.85))

        if c == 3:
            cb_detected, cb_severity = self._detect_chroma_bleed_batch([frame])[0]
            analysis.chroma_bleed, analysis.chroma_bleed_severity = cb_detected, cb_severity
            if cb_detected:
                analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.CHROMA_BLEED, cb_severity, confidence=0.7))
            diag_max, mean_mag = extra["rainbow"]
            analysis.rainbow_effect = bool(diag_max > mean_mag * 5)
            if analysis.rainbow_effect:
                analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.RAINBOW, 0.6, confidence=0.6))
            analysis.dot_crawl = _dot_crawl_decision(extra["column_sums"], height)
            if analysis.dot_crawl:
                analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.DOT_CRAWL, 0.5, confidence=0.6))

        jt_detected, jt_severity = _jitter_decision(extra["jitter_shifts"])
        analysis.jitter_detected, analysis.jitter_severity = jt_detected, jt_severity
        if jt_detected:
            analysis.all_artifacts.append(VHSArtifactInfo(ArtifactType.JITTER, jt_severity, confidence=0.75))
        analysis.overall_degradation = _calculate_degradation(analysis)
        analysis.detected_quality = _estimate_quality(analysis, width)
        return analysis


def create_vhs_processor(tracking: float = 0.5, head_switching: float = 0.7, chroma_bleed: float = 0.5, dropout_repair: float = 0.6,
                         preserve_authentic: bool = True, device_id: int = 0) -> DeviceVHSProcessor:
    return DeviceVHSProcessor(VHSConfig(tracking=tracking, head_switching=head_switching, chroma_bleed=chroma_bleed,
                                        dropout_repair=dropout_repair, preserve_authentic=preserve_authentic), device_id=device_id)
