"""Deinterlacing and interlace analysis on frames that are already on the GPU (csrc/deinterlace.hip), in front of every other stage.

The device form of the reference's `processors/format/interlace.py` (`Deinterlacer` on lists of frames): the names, fields,
defaults and decisions are the reference's, so a maintainer can bind it.  Frames are uint8 CUDA tensors H x W x 3
(BGR) or H x W.  The frame methods are byte-equal to the reference's own functions through tests/deinterlace_ref.py; the analysis
forms its means on the host in float64 from the device's exact integer sums, where the reference forms float32 means (DESIGN K16).

Not built: `process_video` (ffmpeg) and `processors/interlace_handler.py` (ffmpeg throughout).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np

from . import _lib
from ._stage import ANY, Stage, check_frame_list, check_no_overlap, check_out, contiguous

logger = logging.getLogger(__name__)

FW_DEINTERLACE_YADIF, FW_DEINTERLACE_BWDIF, FW_DEINTERLACE_BOB = 0, 1, 2
_BOUNDS = ((1, ANY, 1, ANY, "empty frames"),)


class DeinterlaceMethod(Enum):
    BOB = "bob"
    WEAVE = "weave"
    YADIF = "yadif"
    BWDIF = "bwdif"
    NEURAL = "neural"
    NNEDI = "nnedi"

    @property
    def doubles_framerate(self) -> bool:
        return self in [DeinterlaceMethod.BOB]

    @property
    def requires_neural(self) -> bool:
        return self in [DeinterlaceMethod.NEURAL, DeinterlaceMethod.NNEDI]


class FieldOrder(Enum):
    TFF = "tff"
    BFF = "bff"
    AUTO = "auto"
    UNKNOWN = "unknown"

    @property
    def ffmpeg_value(self) -> str:
        return {"tff": "0", "bff": "1"}.get(self.value, "-1")


class TelecinePattern(Enum):
    PATTERN_3_2 = "3:2"
    PATTERN_2_3 = "2:3"
    PATTERN_2_2 = "2:2"
    PATTERN_EURO = "euro"
    NONE = "none"


@dataclass
class InterlaceConfig:
    """The reference's fields and defaults.  ``ffmpeg_backend`` is accepted and ignored: nothing here goes through ffmpeg."""
    method: DeinterlaceMethod = DeinterlaceMethod.YADIF
    field_order: FieldOrder = FieldOrder.AUTO
    telecine: bool = True
    detection_threshold: float = 0.3
    comb_threshold: float = 0.15
    sample_count: int = 50
    preserve_framerate: bool = False
    neural_model: Optional[Path] = None
    ffmpeg_backend: bool = True

    def __post_init__(self):
        if not 0.0 <= self.detection_threshold <= 1.0:
            raise ValueError("detection_threshold must be between 0.0 and 1.0")
        if not 0.0 <= self.comb_threshold <= 1.0:
            raise ValueError("comb_threshold must be between 0.0 and 1.0")


@dataclass
class InterlaceAnalysis:
    is_interlaced: bool = False
    field_order: FieldOrder = FieldOrder.UNKNOWN
    confidence: float = 0.0
    combing_percentage: float = 0.0
    telecine_pattern: TelecinePattern = TelecinePattern.NONE
    recommended_method: DeinterlaceMethod = DeinterlaceMethod.YADIF
    progressive_percentage: float = 0.0
    tff_percentage: float = 0.0
    bff_percentage: float = 0.0
    details: Dict[str, Any] = field(default_factory=dict)

    def summary(self) -> str:
        if not self.is_interlaced:
            return "Progressive video (no deinterlacing needed)"
        pattern_str = ""
        if self.telecine_pattern != TelecinePattern.NONE:
            pattern_str = f" with {self.telecine_pattern.value} telecine"
        return (f"Interlaced ({self.field_order.value.upper()}{pattern_str})\n"
                f"Combing in {self.combing_percentage:.1f}% of frames\n"
                f"Confidence: {self.confidence*100:.0f}%\n"
                f"Recommended: {self.recommended_method.value.upper()}")


class DeviceDeinterlacer(Stage):
    """The reference's `Deinterlacer` on uint8 CUDA frames of one GPU.  Work is queued on torch's current stream of the frames'
    device; the analysis entries synchronise once per batch of statistics."""

    def __init__(self, config: Optional[InterlaceConfig] = None, device_id: int = 0):
        self.config = config or InterlaceConfig()
        self.device_id = int(device_id)
        super().__init__(self.device_id)

    # ---- device entries ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_frames(frames) -> tuple:
        return check_frame_list(frames, "uint8 CUDA tensors H x W x 3 (BGR) or H x W of one shape on one device expected", _BOUNDS)

    @staticmethod
    def _check_out(out, numel: int, dev) -> None:
        import torch
        check_out(out, f"a contiguous int64 tensor of {numel} elements on {dev} expected", torch.int64, dev, numel=numel)

    @_lib.on_tensor_device
    def interpolate_device(self, frames: Sequence, mode: int, parity: int, prev=None, nxt=None, batched: bool = True,
                           outs: Optional[Sequence] = None) -> List:
        """The line interpolation of a list: new tensors.  ``prev`` / ``nxt`` stand in front of and behind the list for BWDIF (a
        stream's neighbours); without them the first and last frames are their own neighbours.  BOB returns the ``parity`` field of
        every frame at full height.  ``batched=False`` makes one call per frame (the single C entry).  ``outs`` are the
        destinations to use (contiguous, of the frames' shape) instead of new tensors; they must not overlap any source.
        ``prev`` and ``nxt`` are held to the frames' dtype, shape and device and read through a contiguous copy where they are
        views, as the frames are."""
        frames = list(frames)
        if not frames:
            return []
        h, w, c = self._check_frames(frames + [t for t in (prev, nxt) if t is not None])
        frames = contiguous(frames)
        prev = prev if prev is None or prev.is_contiguous() else prev.contiguous()
        nxt = nxt if nxt is None or nxt.is_contiguous() else nxt.contiguous()
        if mode == FW_DEINTERLACE_BOB and h < 2:
            raise ValueError("BOB needs frames of at least 2 rows")
        n = len(frames)
        if outs is None:
            outs = _lib.empty_like_many(frames)
        else:
            outs = list(outs)
            if len(outs) != n or any(not o.is_contiguous() for o in outs):
                raise ValueError("one contiguous destination per frame expected")
            self._check_frames(frames + outs)
        prevs = [frames[i - 1] if i > 0 else (prev if prev is not None else frames[i]) for i in range(n)]
        nexts = [frames[i + 1] if i < n - 1 else (nxt if nxt is not None else frames[i]) for i in range(n)]
        check_no_overlap(outs, frames + [t for t in (prev, nxt) if t is not None], "deinterlace")
        st = _lib.stream_ptr(frames[0].device)
        if batched:
            table = _lib.ptr_table([t for task in zip(frames, prevs, nexts, outs) for t in task])   # n x {cur, prev, next, dst}
            _lib.check(self._lib.fw_deinterlace_batch_u8(table, n, h, w * c, mode, parity, st))
        else:
            for i in range(n):
                _lib.check(self._lib.fw_deinterlace_u8(_lib.ptr(frames[i]), _lib.ptr(prevs[i]),
                                                       _lib.ptr(nexts[i]), _lib.ptr(outs[i]), h, w * c, mode,
                                                       parity, st))
        return outs

    @_lib.on_tensor_device
    def stats_device(self, frames: Sequence, out=None):
        """int64 CUDA tensor n x 4: {n_comb, s_field, s_odd, s_even} of every frame (one launch per 32 frames).  ``out``: a
        contiguous int64 CUDA tensor of 4 n elements to write instead of a new one."""
        import torch
        frames = list(frames)
        h, w, c = self._check_frames(frames)
        frames = contiguous(frames)
        if out is None:
            out = torch.empty((len(frames), 4), dtype=torch.int64, device=frames[0].device)
        self._check_out(out, 4 * len(frames), frames[0].device)
        _lib.check(self._lib.fw_interlace_stats_u8(_lib.ptr_table(frames), len(frames), h, w, c, _lib.ptr(out), _lib.stream_ptr(frames[0].device)))
        return out

    @_lib.on_tensor_device
    def pair_sums_device(self, a: Sequence, b: Sequence, out=None):
        """int64 CUDA tensor n: sum |gray(a[i]) - gray(b[i])|.  ``out``: a contiguous int64 CUDA tensor of n elements to write."""
        import torch
        a, b = list(a), list(b)
        if len(a) != len(b):
            raise ValueError("as many frames in a as in b expected")
        h, w, c = self._check_frames(a + b)
        a, b = contiguous(a), contiguous(b)
        if out is None:
            out = torch.empty((len(a),), dtype=torch.int64, device=a[0].device)
        self._check_out(out, len(a), a[0].device)
        _lib.check(self._lib.fw_frame_absdiff_sum_u8(_lib.ptr_table(a), _lib.ptr_table(b), len(a), h, w, c, _lib.ptr(out), _lib.stream_ptr(a[0].device)))
        return out

    def _frame_differences(self, frames: Sequence, pairs: Sequence[tuple]) -> List[float]:
        if not pairs:
            return []
        sums = self.pair_sums_device([frames[i] for i, _ in pairs], [frames[j] for _, j in pairs]).cpu().numpy()   # one synchronisation
        npix = int(frames[0].shape[0]) * int(frames[0].shape[1])
        return [int(s) / npix for s in sums]

    # ---- the reference's host logic ------------------------------------------------------------------------------------------------
    def analyze(self, frames: Sequence, progress_callback: Optional[Callable[[float], None]] = None) -> InterlaceAnalysis:
        analysis = InterlaceAnalysis()
        if not frames:
            return analysis
        h, w = int(frames[0].shape[0]), int(frames[0].shape[1])
        if h < 4:
            raise ValueError("analyze needs frames of at least 4 rows (there is no pair of rows of one field below that)")
        n = len(frames)
        sample_indices = np.linspace(0, n - 1, min(self.config.sample_count, n), dtype=int)
        sampled = [frames[int(i)] for i in sample_indices]
        pairs = [(int(i), min(int(i) + 1, n - 1)) for i in sample_indices if i < n - 1]
        import torch
        self._check_frames(sampled)
        ns, npairs = len(sampled), len(pairs)
        both = torch.empty((4 * ns + npairs,), dtype=torch.int64, device=sampled[0].device)      # one buffer, one fetch
        self.stats_device(sampled, out=both[:4 * ns])
        if pairs:
            self.pair_sums_device([frames[i] for i, _ in pairs], [frames[j] for _, j in pairs], out=both[4 * ns:])
        fetched = both.cpu().numpy()                                  # the one synchronisation of this batch
        st = fetched[:4 * ns].reshape(ns, 4)
        frame_diffs = [int(v) / (h * w) for v in fetched[4 * ns:]]
        r = h // 2
        combing_scores = []
        scores = {"tff": 0, "bff": 0, "prog": 0}
        for k in range(len(sampled)):
            n_comb, s_field, s_odd, s_even = (int(v) for v in st[k])
            combing_scores.append(np.int64(n_comb) / r)
            diff = s_field / (r * w)
            odd_gradient, even_gradient = s_odd / ((r - 1) * w), s_even / ((r - 1) * w)
            if diff < 5:
                hint = "prog"
            elif odd_gradient > even_gradient * 1.1:
                hint = "tff"
            elif even_gradient > odd_gradient * 1.1:
                hint = "bff"
            else:
                hint = "prog"                                        # 'unknown' is counted with the progressive votes
            scores[hint] += 1
            if progress_callback:
                progress_callback((k + 1) / len(sampled))
        avg_combing = np.mean(combing_scores) if combing_scores else 0
        analysis.combing_percentage = avg_combing * 100
        total = sum(scores.values())
        if total > 0:
            analysis.tff_percentage = scores["tff"] / total * 100
            analysis.bff_percentage = scores["bff"] / total * 100
            analysis.progressive_percentage = scores["prog"] / total * 100
        interlaced_percentage = analysis.tff_percentage + analysis.bff_percentage
        analysis.is_interlaced = bool(interlaced_percentage > 30 or analysis.combing_percentage > self.config.detection_threshold * 100)
        if analysis.tff_percentage > analysis.bff_percentage + 10:
            analysis.field_order = FieldOrder.TFF
        elif analysis.bff_percentage > analysis.tff_percentage + 10:
            analysis.field_order = FieldOrder.BFF
        else:
            analysis.field_order = FieldOrder.UNKNOWN
        analysis.confidence = min(1.0, abs(interlaced_percentage - 50) / 50)
        if frame_diffs:
            analysis.telecine_pattern = self._detect_telecine_pattern(frame_diffs)
            analysis.details["telecine"] = {"pattern": analysis.telecine_pattern.value, "diff_variance": float(np.var(frame_diffs))}
        analysis.recommended_method = self._recommend_method(analysis)
        return analysis

    def detect_interlacing(self, frames: Sequence, progress_callback=None) -> bool:
        return self.analyze(frames, progress_callback).is_interlaced

    def detect_field_order(self, frames: Sequence, progress_callback=None) -> FieldOrder:
        return self.analyze(frames, progress_callback).field_order

    def resolve_field_order(self, frames: Sequence) -> FieldOrder:
        """The configured order; AUTO is taken from the first 20 frames, UNKNOWN becoming TFF."""
        order = self.config.field_order
        if order == FieldOrder.AUTO:
            order = self.detect_field_order(list(frames[:min(20, len(frames))]))
            if order == FieldOrder.UNKNOWN:
                order = FieldOrder.TFF
        return order

    def _kernel_mode(self, method: Optional[DeinterlaceMethod]) -> Optional[int]:
        """The kernel mode of a method, None for WEAVE (frames pass through)."""
        method = method or self.config.method
        if method == DeinterlaceMethod.BOB:
            return FW_DEINTERLACE_BOB
        if method == DeinterlaceMethod.WEAVE:
            return None
        if method == DeinterlaceMethod.BWDIF:
            return FW_DEINTERLACE_BWDIF
        if method in (DeinterlaceMethod.NEURAL, DeinterlaceMethod.NNEDI):
            logger.warning(f"{method.value.upper()} deinterlacing not implemented, falling back to BWDIF")
            return FW_DEINTERLACE_BWDIF
        return FW_DEINTERLACE_YADIF                                   # YADIF and anything unknown

    def _apply(self, frames: List, mode: Optional[int], order: FieldOrder, prev=None, nxt=None) -> List:
        if mode is None:
            return frames
        parity = 1 if order == FieldOrder.TFF else 0                  # the reference's `is_tff`: everything else is BFF
        if mode == FW_DEINTERLACE_BOB:
            even, odd = self.interpolate_device(frames, mode, 0), self.interpolate_device(frames, mode, 1)
            first, second = (even, odd) if parity == 1 else (odd, even)
            return [t for pair in zip(first, second) for t in pair]
        return self.interpolate_device(frames, mode, parity, prev, nxt)

    def deinterlace(self, frames: Sequence, method: Optional[DeinterlaceMethod] = None, progress_callback=None) -> List:
        if not frames:
            return frames
        frames = list(frames) if not isinstance(frames, list) else frames
        mode = self._kernel_mode(method)
        out = self._apply(frames, mode, self.resolve_field_order(frames))
        if progress_callback:
            progress_callback(1.0)
        return out

    def stream(self, frames: Iterable, method: Optional[DeinterlaceMethod] = None, block: int = 8) -> Iterator:
        """`deinterlace` over an iterator, ``block`` frames at a time with one frame of lookahead for BWDIF: the same frames as the
        whole-list call.  AUTO is refused: a stream has no "first 20 frames"."""
        if self.config.field_order == FieldOrder.AUTO:
            raise ValueError("FieldOrder.AUTO needs the clip's first 20 frames: give a stream an explicit field order")
        mode = self._kernel_mode(method)
        order = self.config.field_order
        need = 1 if mode == FW_DEINTERLACE_BWDIF else 0
        buf: List = []
        prev = None
        it = iter(frames)
        eof = False
        while not eof:
            while len(buf) < block + need:
                f = next(it, None)
                if f is None:
                    eof = True
                    break
                self._check_frames([f] if not buf and prev is None else [buf[-1] if buf else prev, f])
                # contiguous once: a block's neighbours are these tensors too (WEAVE passes the caller's frames through)
                buf.append(f if mode is None or f.is_contiguous() else f.contiguous())
            n_out = len(buf) if eof else block
            if n_out == 0:
                return
            head = buf[:n_out]
            nxt = buf[n_out] if n_out < len(buf) else None
            yield from self._apply(head, mode, order, prev if need else None, nxt if need else None)
            prev, buf = head[-1], buf[n_out:]

    def detect_telecine(self, frames: Sequence, progress_callback=None) -> TelecinePattern:
        if not frames or len(frames) < 10:
            return TelecinePattern.NONE
        m = min(60, len(frames) - 1)
        diffs = self._frame_differences(frames, [(i, i + 1) for i in range(m)])
        if progress_callback:
            progress_callback(1.0)
        return self._detect_telecine_pattern(diffs)

    def inverse_telecine(self, frames: Sequence, pattern: Optional[TelecinePattern] = None, progress_callback=None) -> List:
        if not frames:
            return frames
        if pattern is None:
            pattern = self.detect_telecine(frames[:min(60, len(frames))])
        if pattern == TelecinePattern.NONE:
            return frames
        diffs = self._frame_differences(frames, [(i, i + 1) for i in range(len(frames) - 1)])
        if not diffs:
            return frames
        duplicate_mask = np.array(diffs) < np.mean(diffs) * 0.3
        result = [frames[0]] + [frames[i] for i in range(1, len(frames)) if not duplicate_mask[i - 1]]
        if progress_callback:
            progress_callback(1.0)
        logger.info(f"IVTC: Reduced {len(frames)} frames to {len(result)} frames")
        return result

    @staticmethod
    def _detect_telecine_pattern(diffs: Sequence[float]) -> TelecinePattern:
        if len(diffs) < 10:
            return TelecinePattern.NONE
        diffs_array = np.array(diffs)
        is_duplicate = diffs_array < np.mean(diffs_array) * 0.3
        duplicate_ratio = np.sum(is_duplicate) / len(is_duplicate)
        if 0.35 < duplicate_ratio < 0.45:
            for offset in range(5):
                pattern_matches = total_checks = 0
                for i in range(offset, len(is_duplicate) - 5, 5):
                    if i + 2 < len(is_duplicate):
                        total_checks += 1
                        if is_duplicate[i] or is_duplicate[i + 2]:
                            pattern_matches += 1
                if total_checks > 0 and pattern_matches / total_checks > 0.6:
                    return TelecinePattern.PATTERN_3_2
        if 0.45 < duplicate_ratio < 0.55:
            return TelecinePattern.PATTERN_2_2
        return TelecinePattern.NONE

    @staticmethod
    def _recommend_method(analysis: InterlaceAnalysis) -> DeinterlaceMethod:
        if not analysis.is_interlaced:
            return DeinterlaceMethod.WEAVE
        if analysis.telecine_pattern != TelecinePattern.NONE:
            return DeinterlaceMethod.YADIF
        if analysis.combing_percentage > 50:
            return DeinterlaceMethod.BWDIF
        return DeinterlaceMethod.YADIF


def create_deinterlacer(method: str = "yadif", field_order: str = "auto", telecine_detection: bool = True, device_id: int = 0) -> DeviceDeinterlacer:
    try:
        deint_method = DeinterlaceMethod(method.lower())
    except ValueError:
        deint_method = DeinterlaceMethod.YADIF
    try:
        order = FieldOrder(field_order.lower())
    except ValueError:
        order = FieldOrder.AUTO
    return DeviceDeinterlacer(InterlaceConfig(method=deint_method, field_order=order, telecine=telecine_detection), device_id=device_id)
