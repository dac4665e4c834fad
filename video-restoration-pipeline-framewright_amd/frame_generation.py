"""Missing-frame generation on the device (kernel set K22, csrc/frame_generation.hip).

The reference's `processors/frame_generation.py` (`MissingFrameGenerator`) finds holes in the frame numbering of damaged footage and
fills them between frame extraction and the upscale (step 5f): by blending the two boundary frames, or by warping both along Farneback
flow and blending; it then matches film grain and cross-fades into the boundaries.  `DeviceMissingFrameGenerator` runs its frame methods
- `_generate_interpolated`, `_generate_optical_flow`, `_extrapolate_frames`, `_match_film_grain`, `_blend_edges` - and `detect_gaps` on
uint8 BGR frames that are already on the GPU; tests/frame_generation_ref.py is the contract, byte for byte.

The driver.  The reference's `generate_missing` calls `_blend_edges(generated, before or after, after)`, which raises for every gap
with a `before` frame (an array has no truth value), so its own driver fills no ordinary gap.  This driver passes `before` where it
exists and otherwise `after`.  `FrameGenerationConfig` also takes the string "optical_flow", which the reference's restorer passes and
its own enum refuses, as `OPTICAL_FLOW_WARP`.  `fill` / `fill_device` are what the restorer's `fill_gap` call has no counterpart for.

Randomness.  The reference draws from numpy's global generator.  Here the noise is the counter-based generator of `qp_artifacts`
(`frame_key`, the 65536 standard-normal quantiles), keyed by (seed, 2 * generated frame number + tag): tag 0 the grain plane, tag 1
the extrapolation noise.  `config.seed=None` means seed 0.

Not built: `GenerationModel.SVD` (Stable Video Diffusion); it resolves to the `interpolate` backend with the reference's warning, as
the reference does without diffusers.  Frames of less than 16 pixels a side cannot have their grain matched (the 17-tap blur).
"""
from __future__ import annotations

import ctypes as C
import logging
import re
import shutil
import time
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Callable, Iterable, Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, contiguous, fetch, upload
from .qp_artifacts import MAX_SIDE, _read_image, _write_image, frame_key, normal_quantiles

logger = logging.getLogger(__name__)

TAG_GRAIN, TAG_EXTRAPOLATE = 0, 1
FARNEBACK = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)


class GenerationModel(Enum):
    SVD = "svd"
    INTERPOLATE_BLEND = "interpolate_blend"
    OPTICAL_FLOW_WARP = "optical_flow_warp"


@dataclass
class FrameGenerationConfig:
    """The reference's fields, defaults and validation.  ``model`` also takes "optical_flow" for `OPTICAL_FLOW_WARP`.
    ``motion_extrapolation``, ``temporal_consistency`` and ``half_precision`` play no part in the frame path (they do not in the
    reference either)."""
    model: GenerationModel = GenerationModel.INTERPOLATE_BLEND
    max_gap_frames: int = 10
    match_grain: bool = True
    blend_edges: int = 3
    motion_extrapolation: bool = True
    temporal_consistency: bool = True
    seed: Optional[int] = None
    gpu_id: int = 0
    half_precision: bool = True

    def __post_init__(self) -> None:
        if isinstance(self.model, str):
            self.model = GenerationModel("optical_flow_warp" if self.model == "optical_flow" else self.model)
        if self.max_gap_frames < 1:
            raise ValueError(f"max_gap_frames must be >= 1, got {self.max_gap_frames}")
        if self.blend_edges < 0:
            raise ValueError(f"blend_edges must be >= 0, got {self.blend_edges}")


@dataclass
class GapInfo:
    start_frame: int                       # last valid frame before the gap
    end_frame: int                         # first valid frame after it (an end gap: the last expected frame)
    gap_size: int
    before_path: Optional[Path] = None
    after_path: Optional[Path] = None


@dataclass
class FrameGenerationResult:
    frames_generated: int = 0
    frames_failed: int = 0
    gaps_processed: int = 0
    output_dir: Optional[Path] = None
    processing_time_seconds: float = 0.0
    peak_vram_mb: int = 0


def gaussian17_coeffs() -> np.ndarray:
    """cv2.getGaussianKernel(17, 2) as float32: 17 = cvRound(2 * 8 + 1) | 1, GaussianBlur's size for sigma 2 on a float image;
    float64, summed in tap order, normalised, cast."""
    x = np.arange(17, dtype=np.float64) - 8.0
    k = np.exp(-0.5 / (2.0 * 2.0) * x * x)
    total = 0.0
    for v in k:
        total += float(v)
    return (k / total).astype(np.float32)


def noise_key(seed: int, number: int, tag: int) -> int:
    return frame_key(seed, 2 * int(number) + tag)


def parse_frame_number(filename: str) -> Optional[int]:
    """frame_00001.png, 00001.png, frame00001.png, shot_00001.png: the reference's three patterns, in its order."""
    for pattern in (r"frame[_-]?(\d+)", r"^(\d+)\.", r"_(\d+)\."):
        match = re.search(pattern, filename, re.IGNORECASE)
        if match:
            return int(match.group(1))
    return None


def edge_blends(index: int, count: int, blend_edges: int, has_after: bool) -> Tuple[Optional[float], Optional[float]]:
    """`_blend_edges` for generated frame ``index`` of ``count``: (alpha against `before`, alpha against `after`), None where no
    blend is due."""
    if blend_edges <= 0 or count == 0:
        return None, None
    n = min(blend_edges, count)
    j = count - 1 - index
    return ((index + 1) / (n + 1) if index < n else None), ((j + 1) / (n + 1) if has_after and j < n else None)


class DeviceMissingFrameGenerator(Stage):
    """The reference's `MissingFrameGenerator` on uint8 BGR CUDA frames of one GPU.  Work is queued on torch's current stream of the
    frames' device and the host never waits: the grain decision reads its two deviations on the device."""

    def __init__(self, config: Optional[FrameGenerationConfig] = None, gpu_id: Optional[int] = None):
        self.config = config or FrameGenerationConfig()
        self.gpu_id = int(self.config.gpu_id if gpu_id is None else gpu_id)
        super().__init__(self.gpu_id, needs_gpu=False)       # detect_gaps and the gap rule need no GPU
        self._backend = self._detect_backend()
        self._gauss17 = gaussian17_coeffs()
        self._tables = {}                                    # str(device) -> (quantiles float64, extrapolation table float32)
        self._flow = None
        self._closed = False
        self._wrong = "frame_generation: uint8 CUDA tensors H x W x 3 (BGR) of one shape expected"

    def _detect_backend(self) -> str:
        if self.config.model == GenerationModel.SVD:
            logger.warning("SVD not available, falling back to interpolation")
            return "interpolate"
        return "optical_flow" if self.config.model == GenerationModel.OPTICAL_FLOW_WARP else "interpolate"

    def is_available(self) -> bool:
        return not self._closed

    def clear_cache(self) -> None:
        self._tables, self._scratch, self._flow = {}, None, None

    def close(self) -> None:
        """Releases the tables, the flow estimator and the scratch; frame calls that arrive afterwards raise."""
        self._closed = True
        self.clear_cache()

    # ---- gaps --------------------------------------------------------------------------------------------------------------------
    def _gaps(self, frame_numbers, expected_count, path_by_number=None) -> List[GapInfo]:
        frame_numbers = sorted(frame_numbers)
        paths = path_by_number or {}
        gaps = []
        for current, next_num in zip(frame_numbers, frame_numbers[1:]):
            if next_num - current > 1:
                gap_size = next_num - current - 1
                if gap_size <= self.config.max_gap_frames:
                    gaps.append(GapInfo(current, next_num, gap_size, paths.get(current), paths.get(next_num)))
                else:
                    logger.warning(f"Gap too large to fill: frames {current}-{next_num} ({gap_size} missing, max {self.config.max_gap_frames})")
        if expected_count and frame_numbers:
            last_frame = frame_numbers[-1]
            if last_frame < expected_count - 1:
                gap_size = expected_count - 1 - last_frame
                if gap_size <= self.config.max_gap_frames:
                    gaps.append(GapInfo(last_frame, expected_count - 1, gap_size, paths.get(last_frame), None))
        return gaps

    def gaps_from_numbers(self, frame_numbers, expected_count: Optional[int] = None) -> List[GapInfo]:
        """The rule of `detect_gaps` on a list of frame numbers (frames that are already in memory: no paths)."""
        return self._gaps([int(n) for n in frame_numbers], expected_count)

    def detect_gaps(self, frames_dir, expected_count: Optional[int] = None) -> List[GapInfo]:
        """`MissingFrameGenerator.detect_gaps`: every `*.png` of ``frames_dir`` (else every `*.jpg`), numbered by its name; a gap of
        up to `max_gap_frames` frames is reported, a larger one only logged; ``expected_count`` adds the gap behind the last frame."""
        frames_dir = Path(frames_dir)
        frame_files = sorted(frames_dir.glob("*.png"))
        if not frame_files:
            frame_files = sorted(frames_dir.glob("*.jpg"))
        if not frame_files:
            logger.warning(f"No frames found in {frames_dir}")
            return []
        path_by_number = {}
        for f in frame_files:
            num = parse_frame_number(f.name)
            if num is not None:
                path_by_number[num] = f
        if not path_by_number:
            logger.warning("Could not parse frame numbers")
            return []
        gaps = self._gaps(list(path_by_number), expected_count, path_by_number)
        logger.info(f"Detected {len(gaps)} gaps in frame sequence")
        return gaps

    # ---- frames ------------------------------------------------------------------------------------------------------------------
    def _seed(self, seed: Optional[int]) -> int:
        seed = self.config.seed if seed is None else seed
        return 0 if seed is None else int(seed)

    def _tables_for(self, dev):
        key = str(dev)
        if key not in self._tables:
            q = normal_quantiles()
            self._tables[key] = (upload(q, dev), upload((0.0 + 2.0 * q).astype(np.float32), dev))
        return self._tables[key]

    def _flow_estimator(self):
        if self._flow is None:
            from .temporal_denoise import DeviceFlowEstimator
            self._flow = DeviceFlowEstimator(gpu_id=self.gpu_id, convention="cv2", **FARNEBACK)
        return self._flow

    def _check(self, frames) -> tuple:
        if self._closed:
            raise ValueError("frame_generation: the generator is closed")
        dev = self.gpu_device()
        h, w, _ = check_frame_list(frames, self._wrong, [(1, MAX_SIDE, 1, MAX_SIDE, "frame_generation: frames of 1 .. 16384 pixels a side expected")],
                                   dev=dev, wrong_device=f"frame_generation: frames on cuda:{self.gpu_id}, the generator's device, expected")
        if frames[0].dim() != 3:
            raise ValueError(self._wrong)
        if self.config.match_grain and min(h, w) < 16:
            raise ValueError("frame_generation: match_grain needs frames of 16 pixels a side or more (the 17-tap blur)")
        return h, w, dev

    def grain_std_device(self, frame, out=None):
        """The statistic of `_match_film_grain` of one frame as a float32 CUDA tensor of one element (``out``: where to write it)."""
        import torch
        h, w, dev = int(frame.shape[0]), int(frame.shape[1]), frame.device
        out = torch.empty(1, dtype=torch.float32, device=dev) if out is None else out
        scratch = self.scratch(int(self._lib.fw_framegen_grain_scratch_bytes(h, w)), dev)
        _lib.check(self._lib.fw_framegen_grain_std_u8(_lib.ptr(frame), h, w, self._gauss17.ctypes.data_as(C.c_void_p), _lib.ptr(scratch),
                                                      _lib.ptr(out), _lib.stream_ptr(dev)))
        return out

    def _fill_gap(self, before, after, start: int, slots: list, stds, seed: int) -> None:
        """Writes the generated frames start + 1 .. start + len(slots) of one gap into ``slots``; ``stds``: len(slots) + 1 floats."""
        size = len(slots)
        reference = before if before is not None else after
        h, w, dev = int(reference.shape[0]), int(reference.shape[1]), reference.device
        st, p, lib = _lib.stream_ptr(dev), _lib.ptr, self._lib
        quantiles, extra_table = self._tables_for(dev)
        if before is not None and after is not None:
            if self._backend == "optical_flow":
                est = self._flow_estimator()
                (fx, fy), (bx, by) = est.flow_device(before, after), est.flow_device(after, before)
                for i, o in enumerate(slots):
                    _lib.check(lib.fw_framegen_warp_blend_u8(p(before), p(after), p(fx), p(fy), p(bx), p(by), h, w, (i + 1) / (size + 1), p(o), st))
            else:
                for i, o in enumerate(slots):
                    alpha = (i + 1) / (size + 1)
                    _lib.check(lib.fw_add_weighted_u8(p(before), 1 - alpha, p(after), alpha, h * w * 3, p(o), st))
        else:
            for i, o in enumerate(slots):
                _lib.check(lib.fw_framegen_extrapolate_u8(p(reference), p(o), h, w, None, p(extra_table),
                                                          noise_key(seed, start + 1 + i, TAG_EXTRAPOLATE), st))
        grain = self.config.match_grain
        if grain:
            self.grain_std_device(reference, stds[0:1])           # once a gap
        for i, o in enumerate(slots):
            alpha_b, alpha_a = edge_blends(i, size, self.config.blend_edges, after is not None)
            if not grain and alpha_b is None and alpha_a is None:
                continue
            if grain:
                self.grain_std_device(o, stds[1 + i:2 + i])
            _lib.check(lib.fw_framegen_finish_u8(p(o), p(o), h, w, p(stds[0:1]) if grain else None, p(stds[1 + i:2 + i]) if grain else None, None,
                                                 p(quantiles) if grain else None, noise_key(seed, start + 1 + i, TAG_GRAIN),
                                                 p(reference) if alpha_b is not None else None, alpha_b or 0.0,
                                                 p(after) if alpha_a is not None else None, alpha_a or 0.0, st))

    @_lib.on_tensor_device
    def fill_device(self, frames, frame_numbers, expected_count: Optional[int] = None, seed: Optional[int] = None) -> Tuple[list, List[int]]:
        """uint8 H x W x 3 BGR CUDA tensors of one shape and their strictly rising frame numbers -> (frames, frame_numbers) with every
        gap of up to `max_gap_frames` frames filled, and with ``expected_count`` the gap behind the last frame.  The input tensors are
        in the result as they are; all generated frames of a call are views of one allocation."""
        import torch
        frames, numbers = list(frames), [int(n) for n in frame_numbers]
        if len(frames) != len(numbers) or any(a >= b for a, b in zip(numbers, numbers[1:])):
            raise ValueError("frame_generation: one strictly rising frame number per frame expected")
        if not frames:
            return [], []
        h, w, dev = self._check(frames)
        gaps = self._gaps(numbers, expected_count)
        total = sum(g.gap_size for g in gaps)
        if not total:
            return frames, numbers
        frames = contiguous(frames)
        at = dict(zip(numbers, frames))
        buf = torch.empty((total, h, w, 3), dtype=torch.uint8, device=dev)           # one allocation for a call
        stds = torch.empty(total + len(gaps), dtype=torch.float32, device=dev)
        seed, done = self._seed(seed), 0
        for k, g in enumerate(gaps):
            slots = list(buf[done:done + g.gap_size].unbind(0))
            end_gap = g.end_frame not in at
            self._fill_gap(at[g.start_frame], None if end_gap else at[g.end_frame], g.start_frame, slots, stds[done + k:done + k + g.gap_size + 1], seed)
            at.update({g.start_frame + 1 + i: s for i, s in enumerate(slots)})
            done += g.gap_size
        order = sorted(at)
        return [at[n] for n in order], order

    def fill(self, frames, frame_numbers, expected_count: Optional[int] = None, seed: Optional[int] = None) -> Tuple[List[np.ndarray], List[int]]:
        """Host in, host out: uint8 H x W x 3 arrays and their numbers -> (arrays, numbers) with the gaps filled."""
        frames = [np.ascontiguousarray(f) for f in frames]
        for a in frames:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("frame_generation: uint8 arrays H x W x 3 (BGR) expected")
        if not frames:
            return [], []
        with self.host() as dev:
            outs, numbers = self.fill_device([upload(a, dev) for a in frames], frame_numbers, expected_count, seed)
            got = fetch(dev, *outs)
            return ([got] if len(outs) == 1 else list(got)), numbers

    def stream(self, pairs: Iterable, expected_count: Optional[int] = None, seed: Optional[int] = None) -> Iterator:
        """(number, frame) pairs in rising order -> (number, frame) pairs with the gaps filled, one frame held back: the frames equal
        `fill_device` on the whole clip.  The generated frames of one gap are views of one allocation."""
        prev = None
        for number, frame in pairs:
            number = int(number)
            if prev is not None:
                if number <= prev[0]:
                    raise ValueError("frame_generation: one strictly rising frame number per frame expected")
                frames, numbers = self.fill_device([prev[1], frame], [prev[0], number], None, seed)
                yield from zip(numbers[:-1], frames[:-1])
            prev = (number, frame)
        if prev is not None:
            frames, numbers = self.fill_device([prev[1]], [prev[0]], expected_count, seed)
            yield from zip(numbers, frames)

    # ---- the reference's directory driver ----------------------------------------------------------------------------------------
    def generate_missing(self, input_dir, output_dir, gaps: List[GapInfo], progress_callback: Optional[Callable[[float], None]] = None,
                         read_image: Optional[Callable] = None, write_image: Optional[Callable] = None) -> FrameGenerationResult:
        """`MissingFrameGenerator.generate_missing`: every `*.png` and `*.jpg` of ``input_dir`` is copied to ``output_dir``, then the
        frames of every gap are generated from its boundary images and written as `frame_{n:08d}.png`.  A gap without a readable
        boundary counts as failed, and so does one whose generation or writing raises.  ``read_image(path) -> array or None`` and
        ``write_image(path, array)`` replace cv2's imread and imwrite."""
        result = FrameGenerationResult()
        start_time = time.time()
        if not self.is_available():
            logger.error("Frame generation not available")
            return result
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        result.output_dir = output_dir
        input_dir = Path(input_dir)
        read_image, write_image = read_image or _read_image, write_image or _write_image
        for pattern in ("*.png", "*.jpg"):
            for frame_file in input_dir.glob(pattern):
                shutil.copy2(frame_file, output_dir / frame_file.name)
        if not gaps:
            logger.info("No gaps to fill")
            return result
        total_work = sum(gap.gap_size for gap in gaps)
        work_done = 0
        logger.info(f"Generating {total_work} frames to fill {len(gaps)} gaps")
        seed = self._seed(None)
        for gap in gaps:
            try:
                before = read_image(gap.before_path) if gap.before_path and Path(gap.before_path).exists() else None
                after = read_image(gap.after_path) if gap.after_path and Path(gap.after_path).exists() else None
                if before is None and after is None:
                    logger.warning(f"No boundary frames for gap at {gap.start_frame}")
                    result.frames_failed += gap.gap_size
                    continue
                import torch
                with self.host() as dev:
                    b, a = (None if f is None else upload(f, dev) for f in (before, after))
                    self._check([f for f in (b, a) if f is not None])
                    ref = b if b is not None else a
                    slots = list(torch.empty((gap.gap_size,) + tuple(ref.shape), dtype=torch.uint8, device=dev).unbind(0))
                    stds = torch.empty(gap.gap_size + 1, dtype=torch.float32, device=dev)
                    self._fill_gap(b, a, gap.start_frame, slots, stds, seed)
                    generated = fetch(dev, *slots)
                    generated = [generated] if len(slots) == 1 else generated
                for i, frame in enumerate(generated):
                    write_image(output_dir / f"frame_{gap.start_frame + i + 1:08d}.png", frame)
                    result.frames_generated += 1
                result.gaps_processed += 1
            except Exception as e:  # noqa: BLE001 - the reference logs, counts the gap as failed and goes on
                logger.error(f"Failed to fill gap at {gap.start_frame}: {e}")
                result.frames_failed += gap.gap_size
            work_done += gap.gap_size
            if progress_callback:
                progress_callback(work_done / total_work)
        result.processing_time_seconds = time.time() - start_time
        logger.info(f"Frame generation complete: {result.frames_generated} generated, {result.gaps_processed}/{len(gaps)} gaps filled, "
                    f"time: {result.processing_time_seconds:.1f}s")
        return result


def create_frame_generator(model: str = "interpolate_blend", max_gap: int = 10, match_grain: bool = True,
                           gpu_id: int = 0) -> DeviceMissingFrameGenerator:
    config = FrameGenerationConfig(model=model, max_gap_frames=max_gap, match_grain=match_grain, gpu_id=gpu_id)
    return DeviceMissingFrameGenerator(config)
