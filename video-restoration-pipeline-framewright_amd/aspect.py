"""Letterbox / pillarbox detection, bar cropping and aspect conversion on frames that are already on the GPU (csrc/aspect.hip): the crop
in front of the chain (behind the deinterlacer and the VHS processor), the conversion behind the colour grade.

The device form of the reference's `processors/format/aspect.py` (`AspectHandler` on lists of frames): the names, fields, defaults and
decisions are the reference's, so a maintainer can bind it.  Frames are uint8 CUDA tensors H x W x 3 (BGR) or H x W of
1 .. 16384 pixels a side.  `analyze_frame`, `analyze`, `detect_aspect`, `detect_letterbox`, `crop_letterbox`, `convert_aspect`,
`add_pillarbox` and `add_letterbox` are byte-equal and field-equal to the reference's own methods through tests/aspect_ref.py.  The
device forms the gray row and column sums of the frames of a call (exact integers), the host waits once and walks them with the
reference's steps, and the device crops, pads or resizes (DESIGN K18).  Where the reference returns the frame or the list it was given
- no bars, a frame already at the target ratio - so does this.

Deliberately different: a crop or a conversion that leaves no row or no column is refused with a ValueError (the reference returns
empty arrays or fails inside cv2).  Not built: `process_video` and `_detect_ffmpeg_crop` (ffmpeg command lines) and the ffmpeg check of
`AspectHandler.__init__`.  `sample_count` apart, `edge_tolerance`, `preserve_center` and `target_ratio` are fields that no frame method
reads, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from enum import Enum
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, contiguous, fetch, upload

logger = logging.getLogger(__name__)

BATCH = 32                                       # frames of one launch (the kernel argument table)
MAX_SIDE = 16384
ANALYSIS_FRAMES = 20                             # `crop_letterbox` analyses frames[:20]
GAUSS_TAPS = 99
_BOUNDS = ((1, MAX_SIDE, 1, MAX_SIDE, "aspect: frames of 1 .. 16384 pixels a side expected"),)


class StandardAspectRatio(Enum):
    RATIO_4_3 = "4:3"
    RATIO_16_9 = "16:9"
    RATIO_1_85_1 = "1.85:1"
    RATIO_2_35_1 = "2.35:1"
    RATIO_2_39_1 = "2.39:1"
    RATIO_21_9 = "21:9"
    RATIO_1_1 = "1:1"
    RATIO_9_16 = "9:16"
    RATIO_IMAX = "1.43:1"
    RATIO_70MM = "2.20:1"

    @property
    def decimal(self) -> float:
        return {"4:3": 4 / 3, "16:9": 16 / 9, "1.85:1": 1.85, "2.35:1": 2.35, "2.39:1": 2.39, "21:9": 21 / 9, "1:1": 1.0, "9:16": 9 / 16,
                "1.43:1": 1.43, "2.20:1": 2.20}.get(self.value, 16 / 9)

    @classmethod
    def from_decimal(cls, ratio: float, tolerance: float = 0.05) -> Optional["StandardAspectRatio"]:
        for ar in cls:                                                # the first in declaration order, as in the reference
            if abs(ar.decimal - ratio) < tolerance:
                return ar
        return None

    @classmethod
    def from_string(cls, ratio_str: str) -> Optional["StandardAspectRatio"]:
        normalized = ratio_str.lower().strip()
        for ar in cls:
            if ar.value.lower() == normalized:
                return ar
        try:
            return cls.from_decimal(float(normalized.replace(":", "/").split("/")[0]))
        except Exception:  # noqa: BLE001 - the reference catches everything here
            return None


class ConversionMethod(Enum):
    CROP = "crop"
    PAD = "pad"
    SCALE = "scale"
    FIT = "fit"
    STRETCH = "stretch"


class FillMode(Enum):
    BLACK = "black"
    BLUR = "blur"
    MIRROR = "mirror"
    COLOR = "color"


@dataclass
class AspectConfig:
    """The reference's fields, defaults and validation.  `fill_color` is written into BGR frames in the order given."""
    target_ratio: Optional[str] = None
    method: ConversionMethod = ConversionMethod.FIT
    fill_mode: FillMode = FillMode.BLACK
    fill_color: Tuple[int, int, int] = (0, 0, 0)
    black_threshold: int = 16
    min_bar_size: int = 4
    sample_count: int = 20
    edge_tolerance: int = 2
    preserve_center: bool = True
    align_to: int = 2

    def __post_init__(self):
        if not 0 <= self.black_threshold <= 255:
            raise ValueError("black_threshold must be between 0 and 255")
        if self.min_bar_size < 0:
            raise ValueError("min_bar_size must be non-negative")


@dataclass
class CropRegion:
    x: int = 0
    y: int = 0
    width: int = 0
    height: int = 0

    def as_tuple(self) -> Tuple[int, int, int, int]:
        return (self.x, self.y, self.width, self.height)

    def as_ffmpeg_filter(self) -> str:
        return f"crop={self.width}:{self.height}:{self.x}:{self.y}"


@dataclass
class AspectAnalysis:
    frame_width: int = 0
    frame_height: int = 0
    detected_ratio: float = 0.0
    detected_standard: Optional[StandardAspectRatio] = None
    has_letterbox: bool = False
    has_pillarbox: bool = False
    top_bar: int = 0
    bottom_bar: int = 0
    left_bar: int = 0
    right_bar: int = 0
    content_x: int = 0
    content_y: int = 0
    content_width: int = 0
    content_height: int = 0
    content_ratio: float = 0.0
    is_variable: bool = False
    confidence: float = 0.0

    @property
    def crop_region(self) -> CropRegion:
        return CropRegion(x=self.content_x, y=self.content_y, width=self.content_width, height=self.content_height)

    @property
    def bar_percentage(self) -> float:
        if self.frame_width == 0 or self.frame_height == 0:
            return 0.0
        total = self.frame_width * self.frame_height
        content = self.content_width * self.content_height
        return (1 - content / total) * 100 if total > 0 else 0.0

    def summary(self) -> str:
        if not self.has_letterbox and not self.has_pillarbox:
            ratio_name = self.detected_standard.value if self.detected_standard else f"{self.detected_ratio:.2f}:1"
            return f"Full frame content at {ratio_name}"
        bar_info = []
        if self.has_letterbox:
            bar_info.append(f"Letterbox: top={self.top_bar}px, bottom={self.bottom_bar}px")
        if self.has_pillarbox:
            bar_info.append(f"Pillarbox: left={self.left_bar}px, right={self.right_bar}px")
        content_ratio_name = StandardAspectRatio.from_decimal(self.content_ratio)
        ratio_str = content_ratio_name.value if content_ratio_name else f"{self.content_ratio:.2f}:1"
        return (f"Frame: {self.frame_width}x{self.frame_height}\n"
                f"Content: {self.content_width}x{self.content_height} ({ratio_str})\n"
                f"{'; '.join(bar_info)}\n"
                f"Black bars: {self.bar_percentage:.1f}% of frame")


# ---- the reference's host logic on a few hundred sums per frame ---------------------------------------------------------------------
def _bars_from_sums(sums: np.ndarray, other_length: int, threshold: int) -> Tuple[int, int]:
    """(leading, trailing) bar of one direction: np.mean(line) > threshold is sum > threshold * length for exact integer sums.  The
    search covers the outer thirds only; a bar that does not end there is 0, as in the reference."""
    n = int(sums.shape[0])
    content = sums.astype(np.int64) > int(threshold) * int(other_length)
    head = np.flatnonzero(content[:n // 3])
    lead = int(head[0]) if head.size else 0
    tail = np.flatnonzero(content[2 * n // 3 + 1:])
    trail = n - 1 - (2 * n // 3 + 1 + int(tail[-1])) if tail.size else 0
    return lead, trail


def _frame_analysis(rows: np.ndarray, cols: np.ndarray, config: AspectConfig) -> AspectAnalysis:
    height, width = int(rows.shape[0]), int(cols.shape[0])
    a = AspectAnalysis()
    a.frame_width, a.frame_height = width, height
    a.detected_ratio = width / height if height > 0 else 1.0
    a.top_bar, a.bottom_bar = _bars_from_sums(rows, width, config.black_threshold)
    a.has_letterbox = (a.top_bar + a.bottom_bar) >= config.min_bar_size
    a.left_bar, a.right_bar = _bars_from_sums(cols, height, config.black_threshold)
    a.has_pillarbox = (a.left_bar + a.right_bar) >= config.min_bar_size
    a.content_x, a.content_y = a.left_bar, a.top_bar
    a.content_width = width - a.left_bar - a.right_bar
    a.content_height = height - a.top_bar - a.bottom_bar
    a.content_ratio = a.content_width / a.content_height if a.content_height > 0 else a.detected_ratio
    a.detected_standard = StandardAspectRatio.from_decimal(a.content_ratio)
    a.confidence = 1.0
    if a.has_letterbox or a.has_pillarbox:
        if a.has_letterbox and abs(a.top_bar - a.bottom_bar) > 5:
            a.confidence -= 0.1
        if a.has_pillarbox and abs(a.left_bar - a.right_bar) > 5:
            a.confidence -= 0.1
    return a


def _aggregate(analyses: Sequence[AspectAnalysis], config: AspectConfig) -> AspectAnalysis:
    """`analyze` behind its per-frame analyses: each bar is int() of the float64 np.median over the samples (x.5 goes down), the
    variability and the confidence come from np.std of the top and bottom bars in float64, and each bar below `min_bar_size` is
    zeroed on its own."""
    r = AspectAnalysis()
    first = analyses[0]
    r.frame_width, r.frame_height, r.detected_ratio = first.frame_width, first.frame_height, first.detected_ratio
    spread = {}
    for name in ("top_bar", "bottom_bar", "left_bar", "right_bar"):
        values = [getattr(a, name) for a in analyses]
        spread[name] = np.std(values)
        bar = int(np.median(values))
        setattr(r, name, bar if bar >= config.min_bar_size else 0)
    top_std, bottom_std = spread["top_bar"], spread["bottom_bar"]
    r.is_variable = bool(top_std > 5 or bottom_std > 5)
    r.has_letterbox, r.has_pillarbox = (r.top_bar + r.bottom_bar) > 0, (r.left_bar + r.right_bar) > 0
    r.content_x, r.content_y = r.left_bar, r.top_bar
    r.content_width = r.frame_width - r.left_bar - r.right_bar
    r.content_height = r.frame_height - r.top_bar - r.bottom_bar
    if r.content_height > 0:
        r.content_ratio = r.content_width / r.content_height
    r.detected_standard = StandardAspectRatio.from_decimal(r.content_ratio)
    r.confidence = float(1.0 - min(1.0, (top_std + bottom_std) / 20))
    return r


def gauss99_table() -> np.ndarray:
    """uint16 [99], sum 256: getGaussianKernel(99, 0) in 8 fractional bits, built on the host in float64 (DESIGN K18): sigma = 0.3 *
    ((99 - 1) * 0.5 - 1) + 0.8, w = exp(-0.5 / sigma^2 * x^2) normalised; quantised from both ends towards the centre with the
    rounding error carried to the next tap, the centre tap taking what is left of 256."""
    n = GAUSS_TAPS
    sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    w = np.exp((-0.5 / (sigma * sigma)) * x * x)
    w = w * (1.0 / float(np.sum(w)))
    q = np.zeros(n, dtype=np.int64)
    err, total = 0.0, 0
    for i in range(n // 2):
        adj = float(w[i]) * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        q[i] = q[n - 1 - i] = v
        total += v
    q[n // 2] = 256 - 2 * total
    return q.astype(np.uint16)


def _parse_target(target: Union[str, StandardAspectRatio, float]) -> float:
    if isinstance(target, StandardAspectRatio):
        return target.decimal
    if isinstance(target, str):
        std = StandardAspectRatio.from_string(target)
        return std.decimal if std else 16 / 9
    return float(target)


class DeviceAspectHandler(Stage):
    """The reference's `AspectHandler` on uint8 CUDA frames of one GPU.  Work is queued on torch's current stream of the frames' device;
    an analysis waits once for its sums, and every resize (SCALE, FIT, STRETCH, the blur fill, a mirror bar wider than the frame)
    waits for its tables, as `fw_resize_lanczos4_u8` and `fw_resize_linear_u8` do."""

    def __init__(self, config: Optional[AspectConfig] = None, device_id: int = 0):
        self.config = config or AspectConfig()
        self.device_id = int(device_id)
        super().__init__(self.device_id)
        self._wrong_device = f"aspect: frames on cuda:{self.device_id}, the handler's device, expected"
        self._gauss = gauss99_table()

    # ---- checks --------------------------------------------------------------------------------------------------------------------
    def _check_frames(self, frames: Sequence) -> tuple:
        return check_frame_list(frames, "aspect: frames H x W x 3 (BGR) or H x W of one shape expected", _BOUNDS, self._dev,
                                "aspect: uint8 tensors expected", self._wrong_device)

    @staticmethod
    def _check_size(h: int, w: int, what: str) -> None:
        if h < 1 or w < 1:
            raise ValueError(f"aspect: {what} leaves no rows or no columns ({w} x {h})")
        if h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError(f"aspect: {what} gives {w} x {h}, beyond 16384 pixels a side")

    def _new(self, like, n: int, h: int, w: int) -> List:
        """n new contiguous frames h x w with the channels of ``like``: one allocation cut into views."""
        import torch
        shape = (n, h, w, 3) if like.dim() == 3 else (n, h, w)
        return list(torch.empty(shape, dtype=torch.uint8, device=like.device).unbind(0))

    # ---- device entries ------------------------------------------------------------------------------------------------------------
    @_lib.on_tensor_device
    def bar_sums_device(self, frames: Sequence) -> Tuple[np.ndarray, np.ndarray]:
        """(row sums uint32 n x H, column sums uint32 n x W) of the gray image of every frame, as NumPy arrays: one wait."""
        import torch
        frames = contiguous(frames)
        h, w, c = self._check_frames(frames)
        n, dev = len(frames), frames[0].device
        sums = torch.empty((n, h + w), dtype=torch.int32, device=dev)        # rows of all frames, then columns of all frames
        rows, cols = sums.view(-1)[:n * h], sums.view(-1)[n * h:]
        st = _lib.stream_ptr(dev)
        for b in range(0, n, BATCH):
            part = frames[b:b + BATCH]
            _lib.check(self._lib.fw_aspect_bar_sums_u8(_lib.ptr_table(part), len(part), h, w, c, C.c_void_p(rows.data_ptr() + 4 * b * h),
                                                       C.c_void_p(cols.data_ptr() + 4 * b * w), st))
        got = fetch(dev, sums).view(np.uint32).reshape(-1)
        return got[:n * h].reshape(n, h), got[n * h:].reshape(n, w)

    @_lib.on_tensor_device
    def crop_device(self, frames: Sequence, x: int, y: int, width: int, height: int, flip: int = 0) -> List:
        """frames[i][y : y + height, x : x + width] as new contiguous tensors; ``flip`` 1 reverses their columns, 2 their rows."""
        frames = contiguous(frames)
        h, w, c = self._check_frames(frames)
        self._check_size(height, width, "the crop")
        if x < 0 or y < 0 or x + width > w or y + height > h:
            raise ValueError(f"aspect: the crop {width} x {height} at ({x}, {y}) does not lie inside the {w} x {h} frame")
        outs = self._new(frames[0], len(frames), height, width)
        st = _lib.stream_ptr(frames[0].device)
        for b in range(0, len(frames), BATCH):
            src, dst = frames[b:b + BATCH], outs[b:b + BATCH]
            _lib.check(self._lib.fw_aspect_crop_u8(_lib.ptr_table(src), _lib.ptr_table(dst), len(src), h, w, c, int(x), int(y), int(width),
                                                   int(height), int(flip), st))
        return outs

    @_lib.on_tensor_device
    def pad_device(self, frames: Sequence, out_height: int, out_width: int, x_offset: int, y_offset: int, fill_mode: FillMode,
                   color: Sequence[int] = (0, 0, 0)) -> List:
        """New frames out_height x out_width with frames[i] at (x_offset, y_offset) and the rest filled as ``fill_mode`` says."""
        frames = contiguous(frames)
        h, w, c = self._check_frames(frames)
        self._check_size(out_height, out_width, "the padded frame")
        if x_offset < 0 or y_offset < 0 or x_offset + w > out_width or y_offset + h > out_height:
            raise ValueError("aspect: the frame does not lie inside the padded frame")
        st = _lib.stream_ptr(frames[0].device)
        bars = (x_offset, out_width - x_offset - w, y_offset, out_height - y_offset - h)
        if max(bars) == 0:                                            # nothing is missing: the reference's copy
            return self.crop_device(frames, 0, 0, w, h)
        outs = self._new(frames[0], len(frames), out_height, out_width)
        col = (C.c_uint8 * 3)(*[int(v) & 255 for v in (tuple(color) + (0, 0, 0))[:3]])
        backs = strips = None                                         # read by the queued launch; the allocator keeps them until it ran
        if fill_mode == FillMode.BLUR:
            mode, backs = 2, []
            for f in frames:
                back = self._new(f, 1, out_height, out_width)[0]
                self._resize(self._lib.fw_resize_linear_u8, self.gauss99_device(f), back)
                backs.append(back)
        elif fill_mode == FillMode.MIRROR:
            mode = 1
            sizes = ((h, bars[0]), (h, bars[1]), (bars[2], w), (bars[3], w))
            wide = [k for k in range(4) if bars[k] > (w if k < 2 else h)]
            if wide:                                                  # the whole frame reversed and stretched to the bar
                flipped = {1: self.crop_device(frames, 0, 0, w, h, flip=1) if any(k < 2 for k in wide) else None,
                           2: self.crop_device(frames, 0, 0, w, h, flip=2) if any(k >= 2 for k in wide) else None}
                strips = []
                for i, f in enumerate(frames):
                    row = [None] * 4
                    for k in wide:
                        row[k] = self._new(f, 1, sizes[k][0], sizes[k][1])[0]
                        self._resize(self._lib.fw_resize_linear_u8, flipped[1 if k < 2 else 2][i], row[k])
                    strips.append(row)
        else:
            mode = 0
        for b in range(0, len(frames), BATCH):
            src, dst = frames[b:b + BATCH], outs[b:b + BATCH]
            table = None
            if strips is not None:
                table = (C.c_void_p * (4 * len(src)))(*[t.data_ptr() if t is not None else None for row in strips[b:b + BATCH] for t in row])
            _lib.check(self._lib.fw_aspect_pad_u8(_lib.ptr_table(src), _lib.ptr_table(dst), len(src), h, w, c, int(out_height), int(out_width),
                                                  int(x_offset), int(y_offset), mode, col,
                                                  _lib.ptr_table(backs[b:b + BATCH]) if backs is not None else None, table, st))
        return outs

    @_lib.on_tensor_device
    def gauss99_device(self, frame):
        """cv2.GaussianBlur(frame, (99, 99), 0) in OpenCV's fixed point, as a new tensor."""
        import torch
        frame = frame if frame.is_contiguous() else frame.contiguous()
        h, w, c = self._check_frames([frame])
        out = torch.empty_like(frame)
        tmp = self.scratch(2 * h * w * c + 16, frame.device)
        base = (tmp.data_ptr() + 15) & ~15
        table = (C.c_uint16 * GAUSS_TAPS)(*[int(v) for v in self._gauss])
        _lib.check(self._lib.fw_aspect_gauss99_u8(_lib.ptr(frame), h, w, c, table, C.c_void_p(base), _lib.ptr(out), _lib.stream_ptr(frame.device)))
        return out

    def _resize(self, fn, src, dst) -> None:
        c = 3 if src.dim() == 3 else 1
        _lib.check(fn(_lib.ptr(src), int(src.shape[0]), int(src.shape[1]), c, _lib.ptr(dst), int(dst.shape[0]), int(dst.shape[1]),
                      _lib.stream_ptr(src.device)))

    @_lib.on_tensor_device
    def resize_lanczos4_device(self, frames: Sequence, out_width: int, out_height: int) -> List:
        """cv2.resize(frame, (out_width, out_height), interpolation=cv2.INTER_LANCZOS4) of every frame, as new tensors."""
        frames = contiguous(frames)
        self._check_frames(frames)
        self._check_size(out_height, out_width, "the resize")
        outs = self._new(frames[0], len(frames), out_height, out_width)
        for f, o in zip(frames, outs):
            self._resize(self._lib.fw_resize_lanczos4_u8, f, o)
        return outs

    # ---- the reference's methods -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _progress(cb, n: int) -> None:
        if cb:
            for i in range(n):
                cb((i + 1) / n)

    def _analyze_frames(self, frames: Sequence) -> List[AspectAnalysis]:
        rows, cols = self.bar_sums_device(frames)
        return [_frame_analysis(rows[i], cols[i], self.config) for i in range(len(frames))]

    def analyze_frame(self, frame) -> AspectAnalysis:
        if frame is None:
            return AspectAnalysis()
        return self._analyze_frames([frame])[0]

    def detect_aspect(self, frame) -> float:
        if frame is None:
            return 16 / 9
        analysis = self.analyze_frame(frame)
        return analysis.content_ratio if analysis.content_ratio > 0 else analysis.detected_ratio

    def detect_letterbox(self, frame) -> bool:
        if frame is None:
            return False
        return self.analyze_frame(frame).has_letterbox

    def analyze(self, frames: Sequence, progress_callback: Optional[Callable[[float], None]] = None) -> AspectAnalysis:
        if not frames:
            return AspectAnalysis()
        sample_indices = np.linspace(0, len(frames) - 1, min(self.config.sample_count, len(frames)), dtype=int)
        analyses = self._analyze_frames([frames[int(i)] for i in sample_indices])
        self._progress(progress_callback, len(sample_indices))
        return _aggregate(analyses, self.config)

    def _crop_box(self, analysis: AspectAnalysis) -> Tuple[int, int, int, int]:
        crop = analysis.crop_region
        align = self.config.align_to
        x, y, w, h = crop.x, crop.y, (crop.width // align) * align, (crop.height // align) * align
        if w < 1 or h < 1:
            raise ValueError(f"aspect: the crop {crop.width} x {crop.height} aligned to {align} leaves no rows or no columns")
        return x, y, w, h

    def crop_letterbox(self, frames: List, analysis: Optional[AspectAnalysis] = None,
                       progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        self._check_frames(frames)
        if analysis is None:
            analysis = self.analyze(frames[:min(ANALYSIS_FRAMES, len(frames))])
        if not analysis.has_letterbox and not analysis.has_pillarbox:
            return frames
        result = self.crop_device(frames, *self._crop_box(analysis))
        self._progress(progress_callback, len(frames))
        return result

    def stream(self, frames: Iterable, block: int = 8) -> Iterator:
        """`crop_letterbox` over an iterator: the first min(20, n) frames are held back for the analysis, then the frames are cropped
        ``block`` at a time as they arrive.  The same tensors as the whole-list call (the input tensors themselves without bars)."""
        if block < 1:
            raise ValueError("block must be >= 1")
        it = iter(frames)
        head: List = []
        for f in it:
            head.append(f)
            if len(head) == ANALYSIS_FRAMES:
                break
        if not head:
            return
        self._check_frames(head)
        analysis = self.analyze(head)
        if not analysis.has_letterbox and not analysis.has_pillarbox:
            box = None
        else:
            box = self._crop_box(analysis)
        shape = head[0].shape
        chunk = head
        while chunk:
            for b in range(0, len(chunk), block):
                part = chunk[b:b + block]
                if any(f.shape != shape for f in part):
                    raise ValueError("aspect: frames H x W x 3 (BGR) or H x W of one shape expected")
                yield from (part if box is None else self.crop_device(part, *box))
            chunk = []
            for f in it:
                chunk.append(f)
                if len(chunk) == block:
                    break

    def convert_aspect(self, frames: List, target: Union[str, StandardAspectRatio, float], method: Optional[ConversionMethod] = None,
                       progress_callback: Optional[Callable[[float], None]] = None) -> List:
        if not frames:
            return frames
        target_ratio = _parse_target(target)
        method = method or self.config.method
        if not isinstance(method, ConversionMethod):
            raise ValueError(f"aspect: unknown conversion method {method!r}")
        if not isinstance(self.config.fill_mode, FillMode):
            raise ValueError(f"aspect: unknown fill mode {self.config.fill_mode!r}")
        height, width, _ = self._check_frames(frames)                 # one shape: one decision for the list
        if abs(width / height - target_ratio) < 0.01:
            result = list(frames)                                     # already correct: the tensors themselves
        else:
            result = self._convert(list(frames), height, width, target_ratio, method)
        self._progress(progress_callback, len(frames))
        return result

    def _convert(self, frames: List, height: int, width: int, ratio: float, method: ConversionMethod) -> List:
        current = width / height
        if method == ConversionMethod.CROP:
            if current > ratio:
                new_width = int(height * ratio)
                return self.crop_device(frames, (width - new_width) // 2, 0, new_width, height)
            new_height = int(width / ratio)
            return self.crop_device(frames, 0, (height - new_height) // 2, width, new_height)
        if method == ConversionMethod.PAD:
            return self._pad_to_ratio(frames, height, width, ratio)
        if method in (ConversionMethod.SCALE, ConversionMethod.STRETCH):
            return self.resize_lanczos4_device(frames, int(height * ratio), height)
        if current > ratio:                                           # FIT: scale, then pad again (a copy when nothing is missing)
            new_width, new_height = int(height * ratio), height
        else:
            new_width, new_height = width, int(width / ratio)
        return self._pad_to_ratio(self.resize_lanczos4_device(frames, new_width, new_height), new_height, new_width, ratio)

    def _pad_to_ratio(self, frames: List, height: int, width: int, ratio: float) -> List:
        cfg = self.config
        if width / height < ratio:
            out_h, out_w = height, int(height * ratio)
            x_off, y_off = (out_w - width) // 2, 0
        else:
            out_h, out_w = int(width / ratio), width
            x_off, y_off = 0, (out_h - height) // 2
        if out_h < height or out_w < width:
            raise ValueError(f"aspect: padding {width} x {height} to ratio {ratio} gives a smaller frame ({out_w} x {out_h})")
        color = tuple(cfg.fill_color) if cfg.fill_mode == FillMode.COLOR else (0, 0, 0)
        return self.pad_device(frames, out_h, out_w, x_off, y_off, cfg.fill_mode, color)

    def add_pillarbox(self, frames: List, target, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        return self.convert_aspect(frames, target, method=ConversionMethod.PAD, progress_callback=progress_callback)

    def add_letterbox(self, frames: List, target, progress_callback: Optional[Callable[[float], None]] = None) -> List:
        return self.convert_aspect(frames, target, method=ConversionMethod.PAD, progress_callback=progress_callback)

    # ---- numpy in, numpy out -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _fetch_list(dev, tensors: Sequence) -> List[np.ndarray]:
        got = fetch(dev, *tensors)
        return [got] if len(tensors) == 1 else list(got)

    def analyze_host(self, frames: Sequence[np.ndarray]) -> AspectAnalysis:
        with self.host() as dev:
            return self.analyze([upload(f, dev) for f in frames])

    def crop_letterbox_host(self, frames: List[np.ndarray], analysis: Optional[AspectAnalysis] = None) -> List[np.ndarray]:
        """The input list itself when there are no bars, as the reference returns it."""
        if not frames:
            return frames
        with self.host() as dev:
            devs = [upload(f, dev) for f in frames]
            outs = self.crop_letterbox(devs, analysis)
            return frames if outs is devs else self._fetch_list(dev, outs)

    def convert_aspect_host(self, frames: List[np.ndarray], target, method: Optional[ConversionMethod] = None) -> List[np.ndarray]:
        """A frame already at the target ratio comes back as the input array."""
        if not frames:
            return frames
        with self.host() as dev:
            devs = [upload(f, dev) for f in frames]
            outs = self.convert_aspect(devs, target, method)
            return [f if o is d else g for f, o, d, g in zip(frames, outs, devs, self._fetch_list(dev, outs))]


def create_aspect_handler(target_ratio: Optional[str] = None, method: str = "fit", fill_mode: str = "black",
                          device_id: int = 0) -> DeviceAspectHandler:
    try:
        conv_method = ConversionMethod(method.lower())
    except ValueError:
        conv_method = ConversionMethod.FIT
    try:
        fill = FillMode(fill_mode.lower())
    except ValueError:
        fill = FillMode.BLACK
    return DeviceAspectHandler(AspectConfig(target_ratio=target_ratio, method=conv_method, fill_mode=fill), device_id=device_id)
