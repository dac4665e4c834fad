"""Cross-frame temporal consistency on the device (kernel set K23, csrc/temporal_consistency.hip).

The reference's `processors/cross_attention_temporal.py` (`CrossAttentionTemporalProcessor`) de-flickers the final frames behind the
interpolation and in front of the colour grade (step 7b): it lists the scene cuts of the clip (gray histogram correlation below
`scene_change_threshold`), passes every frame within `attention_window // 2` of a cut through unchanged, and on every other frame
detects flicker - the frame differs from both neighbours, which agree with each other - and blends the mean of the neighbours in
under the blurred flicker mask.  `DeviceTemporalConsistencyProcessor` runs `_detect_scene_change`, `_detect_flicker`,
`_apply_optical_flow_consistency`, `_apply_hybrid_consistency` and `apply_consistency` on uint8 BGR frames that are already on the GPU;
tests/temporal_consistency_ref.py is the contract, byte for byte.

Not built: the cross-attention network (`CrossFrameAttention`).  The reference ships no weights for it - it runs a randomly
initialised net when the `.pth` is absent - and global attention over 7 x 32400 tokens at 1080p is beyond any frame budget.  It is a
hook: ``attention_fn(frames, i) -> frame``, a callable the caller injects, handed the list of uint8 CUDA frames and the index of the
centre in it, returning a uint8 CUDA frame of the same shape.  From `apply_device` the list is the clip; from `stream` it is the
frames that are held, which reach from `attention_window // 2` behind the centre to at least as far in front of it (less where the
clip ends).  `CROSS_ATTENTION` without a hook is refused; `HYBRID` without one is the classical path on every frame, as the reference's
HYBRID is without torch, and takes no host wait.  `HYBRID` with a hook reads the flicker area of each frame - one wait a frame - and
calls the hook where it is above 0.01; the hook's frame is blended with the centre by `fw_add_weighted_u8` when `blend_strength < 1`.

The reference's restorer (`restorer.py:2405-2485`) cannot run its step 7b: it passes `window_size=` to `CrossAttentionConfig`, calls
`processor.process_frame` and builds `TemporalConsistencyResult(processed_frames=, method_used=)`, none of which exist.  What binds
to this stage is `apply_consistency` / `apply_device`, with the restorer's default strength 0.5.
"""
from __future__ import annotations

import logging
import shutil
import time
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Callable, Iterable, Iterator, List, Optional

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, check_no_overlap, contiguous, fetch, upload
from .qp_artifacts import MAX_SIDE, _read_image, _write_image

logger = logging.getLogger(__name__)

AREA_THRESHOLD = 0.01
DBL_EPSILON = float(np.finfo(np.float64).eps)


class TemporalMethod(Enum):
    OPTICAL_FLOW = "optical_flow"
    CROSS_ATTENTION = "cross_attention"
    HYBRID = "hybrid"


@dataclass
class CrossAttentionConfig:
    """The reference's fields, defaults and validation; ``method`` also takes its string form.  ``attention_heads``, ``embed_dim``,
    ``preserve_edges`` and ``half_precision`` play no part in the classical path (they do not in the reference either)."""
    method: TemporalMethod = TemporalMethod.HYBRID
    attention_window: int = 7
    attention_heads: int = 8
    embed_dim: int = 256
    flicker_threshold: float = 0.02
    blend_strength: float = 0.8
    preserve_edges: bool = True
    scene_change_threshold: float = 0.3
    gpu_id: int = 0
    half_precision: bool = True

    def __post_init__(self) -> None:
        if isinstance(self.method, str):
            self.method = TemporalMethod(self.method)
        if self.attention_window < 1:
            raise ValueError(f"attention_window must be >= 1, got {self.attention_window}")
        if not 0.0 <= self.blend_strength <= 1.0:
            raise ValueError(f"blend_strength must be 0-1, got {self.blend_strength}")


@dataclass
class TemporalConsistencyResult:
    """The reference's fields, and ``flicker_areas``: np.mean of the flicker mask of every frame `apply_consistency` processed outside
    a cut's window, in frame order."""
    frames_processed: int = 0
    frames_failed: int = 0
    flicker_regions_fixed: int = 0
    scene_changes_detected: List[int] = field(default_factory=list)
    output_dir: Optional[Path] = None
    processing_time_seconds: float = 0.0
    peak_vram_mb: int = 0
    flicker_areas: List[float] = field(default_factory=list)


def hist_correlation(counts1: np.ndarray, counts2: np.ndarray) -> float:
    """cv2.compareHist(HISTCMP_CORREL) of two 256-bin count vectors, each as calcHist's float32 array over its own float32 sum: the
    five sums over the bins in double, in bin order."""
    h1, h2 = (np.asarray(c).astype(np.float32).reshape(256, 1) for c in (counts1, counts2))
    a, b = (h1 / h1.sum()).astype(np.float64).reshape(-1), (h2 / h2.sum()).astype(np.float64).reshape(-1)
    s1, s2, s11, s12, s22 = (float(np.cumsum(v)[-1]) for v in (a, b, a * a, a * b, b * b))
    num = s12 - s1 * s2 / 256.0
    den2 = (s11 - s1 * s1 / 256.0) * (s22 - s2 * s2 / 256.0)
    return num / float(np.sqrt(den2)) if abs(den2) > DBL_EPSILON else 1.0


def area_value(area_sum: int, pixels: int) -> np.float32:
    """np.mean of the float32 mask from the integer sum of k = 256 x mask: exactly the reference's value for a frame of up to 2^16
    pixels, within a few float32 roundings of it beyond (tests/temporal_consistency_ref.py derives the distance)."""
    return np.float32(int(area_sum) / 256.0) / np.float32(pixels)


def in_cut_window(i: int, cuts, attention_window: int) -> bool:
    return any(abs(i - sc) <= attention_window // 2 for sc in cuts)


class DeviceTemporalConsistencyProcessor(Stage):
    """The reference's `CrossAttentionTemporalProcessor` on uint8 BGR CUDA frames of one GPU.  Work is queued on torch's current
    stream of the frames' device.  The host waits where it must read a decision: once a clip for the histograms of the cut list,
    and once a frame for the flicker area when a hook is set."""

    def __init__(self, config: Optional[CrossAttentionConfig] = None, attention_fn: Optional[Callable] = None, gpu_id: Optional[int] = None):
        self.config = config or CrossAttentionConfig()
        if self.config.method == TemporalMethod.CROSS_ATTENTION and attention_fn is None:
            raise ValueError("temporal_consistency: the cross-attention network is not built; CROSS_ATTENTION needs an attention_fn(frames, i) -> "
                             "frame, or use OPTICAL_FLOW / HYBRID")
        self.attention_fn = attention_fn
        self.gpu_id = int(self.config.gpu_id if gpu_id is None else gpu_id)
        super().__init__(self.gpu_id, needs_gpu=False)
        self._backend = "cross_attention" if attention_fn is not None and self.config.method != TemporalMethod.OPTICAL_FLOW else "optical_flow"
        self._threshold = float(np.float32(self.config.flicker_threshold))          # Python floats are weak scalars next to float32 arrays
        self._strength = float(np.float32(self.config.blend_strength))
        self._closed = False
        self._wrong = "temporal_consistency: uint8 CUDA tensors H x W x 3 (BGR) of one shape expected"

    def is_available(self) -> bool:
        return not self._closed

    def clear_cache(self) -> None:
        self._scratch = None

    def close(self) -> None:
        """Releases the scratch; frame calls that arrive afterwards raise."""
        self._closed = True
        self.clear_cache()

    # ---- checks ------------------------------------------------------------------------------------------------------------------
    def _check(self, frames, min_side: int = 3) -> tuple:
        if self._closed:
            raise ValueError("temporal_consistency: the processor is closed")
        dev = self.gpu_device()
        small = "temporal_consistency: frames of 3 .. 16384 pixels a side expected (the 5 x 5 blur reflects two pixels)"
        h, w, _ = check_frame_list(frames, self._wrong, [(min_side, MAX_SIDE, min_side, MAX_SIDE, small)], dev=dev,
                                   wrong_device=f"temporal_consistency: frames on cuda:{self.gpu_id}, the processor's device, expected")
        if frames[0].dim() != 3:
            raise ValueError(self._wrong)
        return h, w, dev

    # ---- scene cuts --------------------------------------------------------------------------------------------------------------
    def _hist_launch(self, frame, cell) -> None:
        h, w = int(frame.shape[0]), int(frame.shape[1])
        _lib.check(self._lib.fw_tcons_gray_hist_u8(_lib.ptr(frame), h, w, _lib.ptr(cell), _lib.stream_ptr(frame.device)))

    @_lib.on_tensor_device
    def gray_hists_device(self, frames):
        """The 256 gray counts of every frame as one int32 CUDA tensor n x 256: one launch a frame, no wait."""
        import torch
        frames = list(frames)
        _, _, dev = self._check(frames, min_side=1)
        hists = torch.empty((len(frames), 256), dtype=torch.int32, device=dev)
        for f, cell in zip(contiguous(frames), hists.unbind(0)):
            self._hist_launch(f, cell)
        return hists

    def _is_cut(self, counts1, counts2) -> bool:
        return bool(hist_correlation(counts1, counts2) < self.config.scene_change_threshold)

    def detect_scene_change_device(self, f1, f2) -> bool:
        """`_detect_scene_change`: True where the correlation of the two gray histograms is below `scene_change_threshold`."""
        counts = fetch(f1.device, self.gray_hists_device([f1, f2]))
        return self._is_cut(counts[0], counts[1])

    def scene_changes_device(self, frames) -> List[int]:
        """`apply_consistency`'s cut list: every i in 1 .. n - 1 whose pair (i - 1, i) is a cut.  One histogram launch a frame, not a
        pair, and the counts of the whole clip are fetched in one wait."""
        frames = list(frames)
        if len(frames) < 2:
            return []
        counts = fetch(frames[0].device, self.gray_hists_device(frames))
        return [i for i in range(1, len(frames)) if self._is_cut(counts[i - 1], counts[i])]

    # ---- frames ------------------------------------------------------------------------------------------------------------------
    def _launch(self, prev, cur, nxt, out=None, mask=None, area=None) -> None:
        h, w = int(cur.shape[0]), int(cur.shape[1])
        _lib.check(self._lib.fw_tcons_apply_u8(_lib.ptr(prev), _lib.ptr(cur), _lib.ptr(nxt), h, w, self._threshold, self._strength,
                                               _lib.ptr(out), _lib.ptr(mask), _lib.ptr(area), _lib.stream_ptr(cur.device)))

    @_lib.on_tensor_device
    def detect_flicker_device(self, prev, cur, nxt, out=None):
        """`_detect_flicker`: the blurred flicker mask as a float32 CUDA tensor H x W (``out``: where to write it)."""
        import torch
        h, w, dev = self._check([prev, cur, nxt])
        prev, cur, nxt = contiguous([prev, cur, nxt])
        mask = torch.empty((h, w), dtype=torch.float32, device=dev) if out is None else out
        self._launch(prev, cur, nxt, mask=mask)
        return mask

    def flicker_area_device(self, prev, cur, nxt) -> float:
        """np.mean of `_detect_flicker`'s mask, from the integer area numerator (one wait)."""
        import torch
        h, w, dev = self._check([prev, cur, nxt])
        prev, cur, nxt = contiguous([prev, cur, nxt])
        cell = torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            self._launch(prev, cur, nxt, area=cell)
        return float(area_value(int(fetch(dev, cell)[0]), h * w))

    def _frame(self, frames, i: int, out, area_cell=None, areas: Optional[list] = None, short: Optional[bool] = None):
        """The configured method on frame ``i`` of ``frames`` (checked, contiguous) into ``out``; returns the output tensor, which is
        ``frames[i]`` itself where the reference returns its centre frame.  ``area_cell``: a device int64 cell for the area numerator,
        read when a hook is set or ``areas`` collects the areas.  ``short``: the clip has fewer than three frames (None: ``frames`` is
        the clip)."""
        n = len(frames)
        short = n < 3 if short is None else short
        cur, prev, nxt = frames[i], frames[max(0, i - 1)], frames[min(n - 1, i + 1)]
        h, w, dev = int(cur.shape[0]), int(cur.shape[1]), cur.device
        hooked = self._backend == "cross_attention"
        classical = not short and not (hooked and self.config.method == TemporalMethod.CROSS_ATTENTION)
        need_area = (hooked and self.config.method == TemporalMethod.HYBRID) or (areas is not None and self.config.method != TemporalMethod.CROSS_ATTENTION)
        if classical or need_area:
            self._launch(prev, cur, nxt, out=out if classical else None, area=area_cell if need_area else None)
        area = None
        if need_area:
            area = area_value(int(fetch(dev, area_cell)[0]), h * w)
            if areas is not None:
                areas.append(float(area))
        if hooked and (self.config.method == TemporalMethod.CROSS_ATTENTION or area > np.float32(AREA_THRESHOLD)):
            result = self.attention_fn(frames, i)
            self._check([cur, result])
            if self.config.blend_strength < 1.0:
                s = self.config.blend_strength
                check_no_overlap([out], [cur, result], "temporal_consistency")
                _lib.check(self._lib.fw_add_weighted_u8(_lib.ptr(cur), 1 - s, _lib.ptr(result.contiguous()), s, h * w * 3, _lib.ptr(out),
                                                        _lib.stream_ptr(dev)))
                return out
            return result
        return out if classical else cur

    @_lib.on_tensor_device
    def apply_frame_device(self, frames, i: int, out=None):
        """The configured method on frame ``i`` of the clip ``frames``, as `apply_consistency` dispatches it outside a cut's window
        (`_apply_optical_flow_consistency` / `_apply_hybrid_consistency` / the hook).  Returns a new tensor (``out`` where given), or
        ``frames[i]`` itself for a clip of fewer than three frames, which the reference returns unchanged."""
        import torch
        frames = list(frames)
        h, w, dev = self._check(frames)
        if not 0 <= int(i) < len(frames):
            raise ValueError("temporal_consistency: a frame index inside the clip expected")
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        else:
            self._check([frames[0], out])
            if not out.is_contiguous():
                raise ValueError("temporal_consistency: a contiguous destination expected")
        check_no_overlap([out], frames, "temporal_consistency")
        return self._frame(contiguous(frames), int(i), out, self._area_cell(dev))

    def _area_cell(self, dev):
        import torch
        return torch.empty(1, dtype=torch.int64, device=dev) if self._backend == "cross_attention" else None

    @_lib.on_tensor_device
    def apply_device(self, frames, scene_changes: Optional[Iterable[int]] = None) -> list:
        """`apply_consistency` on a clip in memory: uint8 H x W x 3 BGR CUDA tensors of one shape -> the output frames.  A frame
        inside a cut's window (|i - cut| <= attention_window // 2) is the input tensor itself, and so is every frame of a clip of
        fewer than three frames; every processed frame of a call is a view of one allocation.  ``scene_changes``: the cut list, where
        the caller has it; None: `scene_changes_device`, the call's one wait."""
        import torch
        frames = list(frames)
        if not frames:
            return []
        h, w, dev = self._check(frames)
        frames = contiguous(frames)
        cuts = self.scene_changes_device(frames) if scene_changes is None else [int(c) for c in scene_changes]
        todo = [i for i in range(len(frames)) if not in_cut_window(i, cuts, self.config.attention_window)]
        buf = torch.empty((len(todo), h, w, 3), dtype=torch.uint8, device=dev)           # one allocation for a call
        cell = self._area_cell(dev)
        out = list(frames)
        for slot, i in zip(buf.unbind(0), todo):
            out[i] = self._frame(frames, i, slot, cell)
        return out

    def apply(self, frames) -> List[np.ndarray]:
        """Host in, host out: uint8 H x W x 3 arrays -> the output arrays."""
        frames = [np.ascontiguousarray(f) for f in frames]
        for a in frames:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("temporal_consistency: uint8 arrays H x W x 3 (BGR) expected")
        if not frames:
            return []
        with self.host() as dev:
            outs = self.apply_device([upload(a, dev) for a in frames])
            got = fetch(dev, *outs)
            return [got] if len(outs) == 1 else list(got)

    def stream(self, frames: Iterable) -> Iterator:
        """Frames in clip order -> the output frames in order, `attention_window // 2 + 1` frames behind the input: frame i needs the
        cuts up to i + attention_window // 2 and its next neighbour, and nothing leaves before three frames have arrived or the clip
        has ended (a clip of fewer than three frames passes through).  The frames equal `apply_device` on the whole clip.  Each
        arriving frame costs one histogram launch and one wait for its 256 counts; the stage holds the frames from
        max(attention_window // 2, 1) behind the next output to the newest."""
        import torch
        window = self.config.attention_window
        lag, keep = window // 2 + 1, max(window // 2, 1)
        held, first = [], 0                          # the frames first .. first + len(held) - 1 of the clip
        cuts, counts_prev, done, j = [], None, 0, -1

        def emit(short: bool):
            """Output frame `done` from the held frames, which hold its neighbours; ``short``: the clip has ended below three frames."""
            nonlocal done, held, first
            at = done - first
            if in_cut_window(done, cuts, window):
                result = held[at]
            else:
                with torch.cuda.device(held[at].device):
                    result = self._frame(held, at, torch.empty_like(held[at]), self._area_cell(held[at].device), short=short)
            done += 1
            drop = max(0, done - keep - first)
            held, first = held[drop:], first + drop
            return result

        for frame in frames:
            j += 1
            self._check([frame])
            frame = frame.contiguous()
            if held and frame.shape != held[-1].shape:
                raise ValueError(self._wrong)
            counts = fetch(frame.device, self.gray_hists_device([frame]))[0]
            if counts_prev is not None and self._is_cut(counts_prev, counts):
                cuts.append(j)
            counts_prev = counts
            held.append(frame)
            while j - done >= lag and j >= 2:
                yield emit(False)
        n = j + 1
        while done < n:
            yield emit(n < 3)

    # ---- the reference's directory driver ----------------------------------------------------------------------------------------
    def apply_consistency(self, input_dir, output_dir, progress_callback: Optional[Callable[[float], None]] = None,
                          read_image: Optional[Callable] = None, write_image: Optional[Callable] = None) -> TemporalConsistencyResult:
        """`CrossAttentionTemporalProcessor.apply_consistency`: every `*.png` of ``input_dir`` (else every `*.jpg`) is read, the cuts
        are listed over the readable neighbours, and every frame is written to ``output_dir`` under its name - unchanged inside a
        cut's window, else through the configured method.  An unreadable frame counts as failed; a frame whose processing or
        writing raises (a neighbour that is unreadable, for one) counts as failed and its file is copied.  ``read_image(path) ->
        array or None`` and ``write_image(path, array)`` replace cv2's imread and imwrite."""
        result = TemporalConsistencyResult()
        start_time = time.time()
        if not self.is_available():
            logger.error("Temporal consistency not available")
            return result
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        result.output_dir = output_dir
        input_dir = Path(input_dir)
        frame_files = sorted(input_dir.glob("*.png"))
        if not frame_files:
            frame_files = sorted(input_dir.glob("*.jpg"))
        if not frame_files:
            logger.warning(f"No frames found in {input_dir}")
            return result
        total_frames = len(frame_files)
        window = self.config.attention_window
        logger.info(f"Temporal consistency ({self.config.method.value}): {total_frames} frames, window={window}")
        read_image, write_image = read_image or _read_image, write_image or _write_image
        import torch
        with self.host() as dev:
            images = [read_image(f) for f in frame_files]
            frames = [None if a is None else upload(a, dev) for a in images]
            hists = torch.zeros((total_frames, 256), dtype=torch.int32, device=dev)
            for f, cell in zip(frames, hists.unbind(0)):
                if f is not None:
                    self._check([f], min_side=1)
                    self._hist_launch(f, cell)
            counts = fetch(dev, hists)                               # one wait for the clip
            for i in range(1, total_frames):
                if frames[i] is not None and frames[i - 1] is not None and self._is_cut(counts[i - 1], counts[i]):
                    result.scene_changes_detected.append(i)
            logger.info(f"Detected {len(result.scene_changes_detected)} scene changes")
            cell = torch.empty(1, dtype=torch.int64, device=dev)
            for i, frame_file in enumerate(frame_files):
                try:
                    if frames[i] is None:
                        logger.warning(f"Skipping invalid frame: {frame_file}")
                        result.frames_failed += 1
                        continue
                    if in_cut_window(i, result.scene_changes_detected, window):
                        processed = images[i]
                    else:
                        n = total_frames
                        if any(frames[k] is None for k in (max(0, i - 1), min(n - 1, i + 1))):
                            raise ValueError(f"temporal_consistency: a neighbour of {frame_file.name} is unreadable")
                        self._check([frames[k] for k in (max(0, i - 1), i, min(n - 1, i + 1))])
                        out = torch.empty_like(frames[i])
                        processed = fetch(dev, self._frame(frames, i, out, cell, result.flicker_areas))
                    write_image(output_dir / frame_file.name, processed)
                    result.frames_processed += 1
                except Exception as e:  # noqa: BLE001 - the reference logs, counts the frame as failed, copies it and goes on
                    logger.error(f"Failed to process {frame_file}: {e}")
                    result.frames_failed += 1
                    try:
                        shutil.copy2(frame_file, output_dir / frame_file.name)
                    except Exception:  # noqa: BLE001
                        pass
                if progress_callback:
                    progress_callback((i + 1) / total_frames)
        result.processing_time_seconds = time.time() - start_time
        logger.info(f"Temporal consistency complete: {result.frames_processed}/{total_frames} frames, time: {result.processing_time_seconds:.1f}s")
        return result


def create_temporal_processor(method: str = "hybrid", window: int = 7, blend_strength: float = 0.8, gpu_id: int = 0,
                              attention_fn: Optional[Callable] = None) -> DeviceTemporalConsistencyProcessor:
    config = CrossAttentionConfig(method=TemporalMethod(method), attention_window=window, blend_strength=blend_strength, gpu_id=gpu_id)
    return DeviceTemporalConsistencyProcessor(config, attention_fn)
