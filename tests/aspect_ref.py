"""The contract of csrc/aspect.hip and framewright_amd/aspect.py: a NumPy restatement of the frame path of the reference's
`AspectHandler` (processors/format/aspect.py) with every type spelled out.  tools/gen_aspect_golden.py holds it against the reference's
own methods (byte for byte for frames, field for field for the analysis); tests/test_aspect_ref_host.py holds it against what that run
recorded.  Frames are uint8 arrays H x W (gray) or H x W x 3 (BGR).  Not restated: `process_video` and `_detect_ffmpeg_crop`, which
only build and run ffmpeg command lines.

What the cv2 calls mean here (cv2 is absent, so its own bytes are unpinned, as everywhere in this project):
  cvtColor(BGR2GRAY)           the project's 14-bit gray (tests/vhs_ref.gray)
  resize(..., INTER_LANCZOS4)  oracle/lanczos_ref.resize_lanczos4_u8
  resize(...)                  oracle/face_ref.resize_linear_u8 (the same size: a copy; an exact halving: the 2 x 2 mean)
  flip                         a reversed view
  GaussianBlur(src, (99, 99), 0) on uint8: OpenCV's fixed-point path as this project reads it, `gaussian_blur_99` below

Integers where the reference has float means: np.mean(line) > threshold for uint8 values and an integer threshold is
sum > threshold * length - the float64 quotient of an exact integer sum below 2^53 by a length below 2^40 cannot round across an
integer - so the bar search runs on integer row and column sums of the gray image.
"""
from __future__ import annotations

import hashlib
import sys
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle.face_ref import resize_linear_u8  # noqa: E402
from oracle.lanczos_ref import resize_lanczos4_u8  # noqa: E402


# ---- value types ------------------------------------------------------------------------------------------------------------------------
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
        return _DECIMALS.get(self.value, 16 / 9)

    @classmethod
    def from_decimal(cls, ratio: float, tolerance: float = 0.05) -> Optional["StandardAspectRatio"]:
        """The first member, in declaration order, closer than ``tolerance``: 2.35 is found before 2.39 and 21:9."""
        for ar in cls:
            if abs(ar.decimal - ratio) < tolerance:
                return ar
        return None

    @classmethod
    def from_string(cls, ratio_str: str) -> Optional["StandardAspectRatio"]:
        """A member's own spelling, else the number in front of the first ':' or '/' through `from_decimal` ("2.0:1" names nothing)."""
        text = ratio_str.lower().strip()
        for ar in cls:
            if ar.value.lower() == text:
                return ar
        try:
            return cls.from_decimal(float(text.replace(":", "/").split("/")[0]))
        except Exception:  # noqa: BLE001 - the reference catches everything here
            return None


_DECIMALS = {"4:3": 4 / 3, "16:9": 16 / 9, "1.85:1": 1.85, "2.35:1": 2.35, "2.39:1": 2.39, "21:9": 21 / 9, "1:1": 1.0, "9:16": 9 / 16,
             "1.43:1": 1.43, "2.20:1": 2.20}


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
        return (1 - (self.content_width * self.content_height) / (self.frame_width * self.frame_height)) * 100

    def summary(self) -> str:
        if not self.has_letterbox and not self.has_pillarbox:
            name = self.detected_standard.value if self.detected_standard else f"{self.detected_ratio:.2f}:1"
            return f"Full frame content at {name}"
        bars = []
        if self.has_letterbox:
            bars.append(f"Letterbox: top={self.top_bar}px, bottom={self.bottom_bar}px")
        if self.has_pillarbox:
            bars.append(f"Pillarbox: left={self.left_bar}px, right={self.right_bar}px")
        std = StandardAspectRatio.from_decimal(self.content_ratio)
        ratio = std.value if std else f"{self.content_ratio:.2f}:1"
        return (f"Frame: {self.frame_width}x{self.frame_height}\n"
                f"Content: {self.content_width}x{self.content_height} ({ratio})\n"
                f"{'; '.join(bars)}\n"
                f"Black bars: {self.bar_percentage:.1f}% of frame")


ANALYSIS_FIELDS = ("frame_width", "frame_height", "detected_ratio", "has_letterbox", "has_pillarbox", "top_bar", "bottom_bar", "left_bar",
                   "right_bar", "content_x", "content_y", "content_width", "content_height", "content_ratio", "is_variable", "confidence")


def analysis_record(a: AspectAnalysis) -> dict:
    """The fields of an analysis (of either implementation) as plain JSON values, with what its three derived members say."""
    rec = {}
    for k in ANALYSIS_FIELDS:
        v = getattr(a, k)
        rec[k] = bool(v) if isinstance(v, (bool, np.bool_)) else (int(v) if isinstance(v, (int, np.integer)) else float(v))
    rec["detected_standard"] = a.detected_standard.value if a.detected_standard else None
    rec["crop_region"] = [int(v) for v in a.crop_region.as_tuple()]
    rec["bar_percentage"] = float(a.bar_percentage)
    rec["summary"] = a.summary()
    return rec


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def gray(frame: np.ndarray) -> np.ndarray:
    if frame.ndim == 2:
        return frame
    v = frame.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + (1 << 13)) >> 14).astype(np.uint8)


def bar_sums(frame: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(row sums [H], column sums [W]) of the gray image, exact, as uint32 (at most 255 * 16384)."""
    g = gray(frame).astype(np.int64)
    return g.sum(axis=1).astype(np.uint32), g.sum(axis=0).astype(np.uint32)


def bars_from_sums(sums: np.ndarray, other_length: int, threshold: int) -> Tuple[int, int]:
    """(leading bar, trailing bar) of one direction from its line sums; each line is ``other_length`` pixels long.  The leading bar
    is the first line of the first third that is content, the trailing bar the distance of the last content line of the last third
    from the end; a bar that does not end inside its third counts as 0, and so does a frame without content."""
    n = len(sums)
    limit = int(threshold) * int(other_length)
    lead = 0
    for i in range(n // 3):
        if int(sums[i]) > limit:
            lead = i
            break
    trail = 0
    for i in range(n - 1, 2 * n // 3, -1):
        if int(sums[i]) > limit:
            trail = n - 1 - i
            break
    return lead, trail


GAUSS_TAPS = 99


def gauss99_table() -> np.ndarray:
    """int64 [99], sum 256: the weights of getGaussianKernel(99, 0) in 8 fractional bits.  sigma = 0.3 * ((99 - 1) * 0.5 - 1) + 0.8 =
    15.2; w[i] = exp(-0.5 / sigma^2 * x^2) at x = i - 49 in float64, times 1 / sum.  Quantised from both ends towards the centre with
    the rounding error carried along: v = rint(w[i] * 256 + err), err = w[i] * 256 + err - v, the same v for tap i and tap 98 - i;
    the centre tap takes what is left of 256."""
    n = GAUSS_TAPS
    sigma = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    scale2x = -0.5 / (sigma * sigma)
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    w = np.exp(scale2x * x * x)
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
    return q


def reflect101(p: np.ndarray, length: int) -> np.ndarray:
    """BORDER_REFLECT_101 for any index, reflected as often as it takes; a side of one pixel is that pixel."""
    p = np.asarray(p, dtype=np.int64).copy()
    if length == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= length)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= length, 2 * length - p - 2, p))


def gaussian_blur_99(img: np.ndarray) -> np.ndarray:
    """Rows first: h = sum src * k (at most 255 * 256, 16 bits), then columns: v = sum h * k (32 bits), out = (v + 2^15) >> 16."""
    k = gauss99_table()
    squeeze = img.ndim == 2
    src = (img[:, :, None] if squeeze else img).astype(np.int64)
    hs, ws, _ = src.shape
    taps = np.arange(GAUSS_TAPS) - GAUSS_TAPS // 2
    hor = np.zeros_like(src)
    xs = np.arange(ws)
    for t, kt in zip(taps.tolist(), k.tolist()):
        if kt:
            hor += src[:, reflect101(xs + t, ws), :] * kt
    ver = np.zeros_like(src)
    ys = np.arange(hs)
    for t, kt in zip(taps.tolist(), k.tolist()):
        if kt:
            ver += hor[reflect101(ys + t, hs)] * kt
    out = ((ver + (1 << 15)) >> 16).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


def parse_target(target: Union[str, StandardAspectRatio, float]) -> float:
    if isinstance(target, StandardAspectRatio):
        return target.decimal
    if isinstance(target, str):
        std = StandardAspectRatio.from_string(target)
        return std.decimal if std else 16 / 9
    return float(target)


# ---- the handler ----------------------------------------------------------------------------------------------------------------------------
class AspectHandler:
    def __init__(self, config: Optional[AspectConfig] = None):
        self.config = config or AspectConfig()

    # detection
    def analyze_frame(self, frame: Optional[np.ndarray]) -> AspectAnalysis:
        a = AspectAnalysis()
        if frame is None:
            return a
        height, width = frame.shape[:2]
        a.frame_width, a.frame_height = width, height
        a.detected_ratio = width / height if height > 0 else 1.0
        rows, cols = bar_sums(frame)
        a.top_bar, a.bottom_bar = bars_from_sums(rows, width, self.config.black_threshold)
        a.has_letterbox = (a.top_bar + a.bottom_bar) >= self.config.min_bar_size
        a.left_bar, a.right_bar = bars_from_sums(cols, height, self.config.black_threshold)
        a.has_pillarbox = (a.left_bar + a.right_bar) >= self.config.min_bar_size
        a.content_x, a.content_y = a.left_bar, a.top_bar
        a.content_width = width - a.left_bar - a.right_bar
        a.content_height = height - a.top_bar - a.bottom_bar
        a.content_ratio = a.content_width / a.content_height if a.content_height > 0 else a.detected_ratio
        a.detected_standard = StandardAspectRatio.from_decimal(a.content_ratio)
        a.confidence = 1.0
        if a.has_letterbox and abs(a.top_bar - a.bottom_bar) > 5:
            a.confidence -= 0.1
        if a.has_pillarbox and abs(a.left_bar - a.right_bar) > 5:
            a.confidence -= 0.1
        return a

    def detect_aspect(self, frame: Optional[np.ndarray]) -> float:
        if frame is None:
            return 16 / 9
        a = self.analyze_frame(frame)
        return a.content_ratio if a.content_ratio > 0 else a.detected_ratio

    def detect_letterbox(self, frame: Optional[np.ndarray]) -> bool:
        return False if frame is None else self.analyze_frame(frame).has_letterbox

    def analyze(self, frames: Sequence[np.ndarray], progress_callback=None) -> AspectAnalysis:
        if not frames:
            return AspectAnalysis()
        indices = np.linspace(0, len(frames) - 1, min(self.config.sample_count, len(frames)), dtype=int)
        per_frame = []
        for i, idx in enumerate(indices):
            per_frame.append(self.analyze_frame(frames[idx]))
            if progress_callback:
                progress_callback((i + 1) / len(indices))
        return aggregate(per_frame, self.config.min_bar_size)

    # cropping
    def crop_letterbox(self, frames: List[np.ndarray], analysis: Optional[AspectAnalysis] = None, progress_callback=None) -> List[np.ndarray]:
        if not frames:
            return frames
        if analysis is None:
            analysis = self.analyze(frames[:min(20, len(frames))])
        if not analysis.has_letterbox and not analysis.has_pillarbox:
            return frames
        x, y, w, h = aligned_crop(analysis.crop_region, self.config.align_to)
        out = []
        for i, f in enumerate(frames):
            out.append(f[y:y + h, x:x + w])
            if progress_callback:
                progress_callback((i + 1) / len(frames))
        return out

    # conversion
    def convert_aspect(self, frames: List[np.ndarray], target, method: Optional[ConversionMethod] = None, progress_callback=None) -> List[np.ndarray]:
        if not frames:
            return frames
        ratio = parse_target(target)
        method = method or self.config.method
        out = []
        for i, f in enumerate(frames):
            out.append(self._convert_frame(f, ratio, method))
            if progress_callback:
                progress_callback((i + 1) / len(frames))
        return out

    def add_pillarbox(self, frames, target, progress_callback=None):
        return self.convert_aspect(frames, target, method=ConversionMethod.PAD, progress_callback=progress_callback)

    def add_letterbox(self, frames, target, progress_callback=None):
        return self.convert_aspect(frames, target, method=ConversionMethod.PAD, progress_callback=progress_callback)

    def _convert_frame(self, frame: np.ndarray, ratio: float, method: ConversionMethod) -> np.ndarray:
        height, width = frame.shape[:2]
        if abs(width / height - ratio) < 0.01:
            return frame
        if method == ConversionMethod.CROP:
            return self._crop_to_ratio(frame, ratio)
        if method == ConversionMethod.PAD:
            return self._pad_to_ratio(frame, ratio)
        if method in (ConversionMethod.SCALE, ConversionMethod.STRETCH):
            return resize_lanczos4_u8(frame, int(height * ratio), height)
        if method == ConversionMethod.FIT:
            return self._fit_to_ratio(frame, ratio)
        return frame

    @staticmethod
    def _crop_to_ratio(frame: np.ndarray, ratio: float) -> np.ndarray:
        height, width = frame.shape[:2]
        if width / height > ratio:
            new_width = int(height * ratio)
            x0 = (width - new_width) // 2
            return frame[:, x0:x0 + new_width]
        new_height = int(width / ratio)
        y0 = (height - new_height) // 2
        return frame[y0:y0 + new_height]

    def _pad_to_ratio(self, frame: np.ndarray, ratio: float) -> np.ndarray:
        height, width = frame.shape[:2]
        cfg = self.config
        color = tuple(cfg.fill_color) if cfg.fill_mode == FillMode.COLOR else (0, 0, 0)
        if width / height < ratio:
            out_h, out_w = height, int(height * ratio)
            x_off, y_off = (out_w - width) // 2, 0
        else:
            out_h, out_w = int(width / ratio), width
            x_off, y_off = 0, (out_h - height) // 2
        if frame.ndim == 3:
            result = np.full((out_h, out_w, 3), color, dtype=np.uint8)           # the configured tuple lands in B, G, R unchanged
        else:
            result = np.full((out_h, out_w), color[0], dtype=np.uint8)
        result[y_off:y_off + height, x_off:x_off + width] = frame
        if cfg.fill_mode == FillMode.BLUR:
            back = resize_linear_u8(gaussian_blur_99(frame), out_w, out_h)
            outside = np.ones((out_h, out_w), dtype=bool)
            outside[y_off:y_off + height, x_off:x_off + width] = False
            result[outside] = back[outside]
        elif cfg.fill_mode == FillMode.MIRROR:
            mirror_fill(result, frame, x_off, y_off)
        return result

    def _fit_to_ratio(self, frame: np.ndarray, ratio: float) -> np.ndarray:
        height, width = frame.shape[:2]
        if width / height > ratio:
            scaled = resize_lanczos4_u8(frame, int(height * ratio), height)
        else:
            scaled = resize_lanczos4_u8(frame, width, int(width / ratio))
        return self._pad_to_ratio(scaled, ratio)                                     # pads again: a copy when nothing is missing


def aggregate(per_frame: Sequence[AspectAnalysis], min_bar_size: int) -> AspectAnalysis:
    """`analyze` behind its per-frame analyses: int() of the float64 median of each bar (x.5 goes down), the variability and the
    confidence from np.std of the top and bottom bars in float64, each bar below ``min_bar_size`` zeroed on its own."""
    r = AspectAnalysis()
    first = per_frame[0]
    r.frame_width, r.frame_height, r.detected_ratio = first.frame_width, first.frame_height, first.detected_ratio
    r.top_bar = int(np.median([a.top_bar for a in per_frame]))
    r.bottom_bar = int(np.median([a.bottom_bar for a in per_frame]))
    r.left_bar = int(np.median([a.left_bar for a in per_frame]))
    r.right_bar = int(np.median([a.right_bar for a in per_frame]))
    top_std = np.std([a.top_bar for a in per_frame])
    bottom_std = np.std([a.bottom_bar for a in per_frame])
    r.is_variable = bool(top_std > 5 or bottom_std > 5)
    for name in ("top_bar", "bottom_bar", "left_bar", "right_bar"):
        if getattr(r, name) < min_bar_size:
            setattr(r, name, 0)
    r.has_letterbox = (r.top_bar + r.bottom_bar) > 0
    r.has_pillarbox = (r.left_bar + r.right_bar) > 0
    r.content_x, r.content_y = r.left_bar, r.top_bar
    r.content_width = r.frame_width - r.left_bar - r.right_bar
    r.content_height = r.frame_height - r.top_bar - r.bottom_bar
    if r.content_height > 0:
        r.content_ratio = r.content_width / r.content_height
    r.detected_standard = StandardAspectRatio.from_decimal(r.content_ratio)
    r.confidence = float(1.0 - min(1.0, (top_std + bottom_std) / 20))
    return r


def aligned_crop(crop: CropRegion, align_to: int) -> Tuple[int, int, int, int]:
    """(x, y, w, h) with the width and the height floored to a multiple of ``align_to``; the offset stays."""
    return crop.x, crop.y, (crop.width // align_to) * align_to, (crop.height // align_to) * align_to


def mirror_fill(result: np.ndarray, source: np.ndarray, x_off: int, y_off: int) -> None:
    """The four strips beside the source, each over the source's span only (the corners keep the fill colour): the strip of the source
    next to the bar, at most as wide as the bar, reversed and brought to the bar's size with the linear resize - a pure reversal when
    the bar is no wider than the source, the whole source reversed and stretched when it is."""
    src_h, src_w = source.shape[:2]
    res_h, res_w = result.shape[:2]
    if x_off > 0:
        strip = source[:, :min(x_off, src_w)][:, ::-1]
        result[y_off:y_off + src_h, :x_off] = resize_linear_u8(strip, x_off, src_h)
    right = x_off + src_w
    if right < res_w:
        strip = source[:, max(0, src_w - (res_w - right)):][:, ::-1]
        result[y_off:y_off + src_h, right:] = resize_linear_u8(strip, res_w - right, src_h)
    if y_off > 0:
        strip = source[:min(y_off, src_h)][::-1]
        result[:y_off, x_off:x_off + src_w] = resize_linear_u8(strip, src_w, y_off)
    bottom = y_off + src_h
    if bottom < res_h:
        strip = source[max(0, src_h - (res_h - bottom)):][::-1]
        result[bottom:, x_off:x_off + src_w] = resize_linear_u8(strip, src_w, res_h - bottom)


def create_aspect_handler(target_ratio: Optional[str] = None, method: str = "fit", fill_mode: str = "black") -> AspectHandler:
    try:
        m = ConversionMethod(method.lower())
    except ValueError:
        m = ConversionMethod.FIT
    try:
        fill = FillMode(fill_mode.lower())
    except ValueError:
        fill = FillMode.BLACK
    return AspectHandler(AspectConfig(target_ratio=target_ratio, method=m, fill_mode=fill))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(37, 33), (48, 64), (64, 258), (32, 8), (2, 2)]             # H x W: odd, even, more than 256 columns, narrow, empty thirds
BLUR_WIDE = (37, 120)                                                 # wider than the 99 taps
FILL_COLOR = (200, 30, 90)


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(frames: Sequence[np.ndarray]) -> str:
    """One sha256 over the shapes and the bytes of a list of frames, in order."""
    h = hashlib.sha256()
    for a in frames:
        h.update(repr(tuple(a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _content(rng, h: int, w: int) -> np.ndarray:
    return rng.randint(40, 256, size=(h, w, 3)).astype(np.uint8)


def clip_bars(h: int, w: int, bars: Sequence[Tuple[int, int, int, int]], seed: int) -> List[np.ndarray]:
    """One BGR frame per (top, bottom, left, right): content of 40 .. 255 inside, bars of 0 .. 8 (dark, not constant) outside."""
    rng = np.random.RandomState(seed)
    out = []
    for top, bottom, left, right in bars:
        f = rng.randint(0, 9, size=(h, w, 3)).astype(np.uint8)
        f[top:h - bottom, left:w - right] = _content(rng, h, w)[top:h - bottom, left:w - right]
        out.append(f)
    return out


def clip_threshold(h: int, w: int, seed: int) -> List[np.ndarray]:
    """Row 2 and column 2 sum to exactly threshold * length (16 everywhere: still bar), row 3 and column 3 to one more (content)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        f = np.zeros((h, w, 3), dtype=np.uint8)
        f[4:, 4:] = _content(rng, h, w)[4:, 4:]
        f[2:4, :] = 16
        f[:, 2:4] = 16
        f[3, 5] = 17
        f[6, 3] = 17
        out.append(f)
    return out


def clips() -> Dict[str, List[np.ndarray]]:
    """name -> list of BGR frames; "<name>/gray" is the same list as gray frames."""
    out: Dict[str, List[np.ndarray]] = {}
    for k, (h, w) in enumerate(SIZES):
        s = f"{h}x{w}"
        t, l = h // 3, w // 3
        out[f"letterbox/{s}"] = clip_bars(h, w, [(h // 6, h // 6 + 1, 0, 0)] * 5, 100 + k)
        out[f"pillarbox/{s}"] = clip_bars(h, w, [(0, 0, w // 6 + 1, w // 6)] * 3, 200 + k)
        out[f"edge_found/{s}"] = clip_bars(h, w, [(max(0, t - 1), max(0, t - 8), max(0, l - 1), max(0, l - 8))] * 3, 300 + k)
        out[f"edge_lost/{s}"] = clip_bars(h, w, [(t, t, l, l)] * 3, 400 + k)
        out[f"black/{s}"] = [np.zeros((h, w, 3), dtype=np.uint8) for _ in range(2)]
        out[f"variable/{s}"] = clip_bars(h, w, [(0 if i % 2 == 0 and i < 4 else max(0, t - 1), min(i, max(0, t - 1)), 0, 0) for i in range(5)], 500 + k)
        out[f"median_half/{s}"] = clip_bars(h, w, [(min(a, max(0, t - 1)), min(b, max(0, t - 1)), 0, 0) for a, b in ((4, 6), (4, 7), (5, 6), (5, 7))], 600 + k)
        out[f"small_bar/{s}"] = clip_bars(h, w, [(min(2, max(0, t - 1)), min(1, max(0, t - 1)), min(3, max(0, l - 1)), min(3, max(0, l - 1)))] * 3, 700 + k)
        out[f"plain/{s}"] = clip_bars(h, w, [(0, 0, 0, 0)] * 2, 800 + k)
        if min(h, w) >= 33:
            out[f"threshold/{s}"] = clip_threshold(h, w, 900 + k)
    base = clip_bars(37, 33, [(6, 7, 0, 0)] * 5, 1000)
    out["long/37x33"] = [base[(3 * i) % 5] for i in range(23)]        # more than the 20 frames the crop analyses
    for name in [n for n in out if n.split("/")[0] in ("letterbox", "edge_found", "threshold", "long") and "2x2" not in n]:
        out[name + "/gray"] = [gray(f) for f in out[name]]
    return out


CROP_ALIGNS = (2, 16)


def convert_frames() -> Dict[str, List[np.ndarray]]:
    """name -> two frames of content to convert: every size as BGR, 37x33 as gray too, and 37x120 for the blur."""
    out = {}
    for k, (h, w) in enumerate(SIZES + [BLUR_WIDE]):
        out[f"{h}x{w}"] = [_content(np.random.RandomState(40 + k), h, w), _content(np.random.RandomState(60 + k), h, w)]
    out["37x33/gray"] = [gray(f) for f in out["37x33"]]
    return out


def convert_cases(name: str, frames: Sequence[np.ndarray]) -> List[Tuple[str, str, str, object]]:
    """(key, method, fill mode, target) for a convert fixture.  Targets: 1.5 times wider and narrower than the frame, 3.5 times for the
    mirror fill that stretches, the frame's own ratio, and three spellings.  A case whose arithmetic leaves no row or column (2 x 2,
    32 x 8) is not listed: the reference fails or returns empty arrays there, the device refuses."""
    h, w = frames[0].shape[:2]
    cur = w / h
    cases: List[Tuple[str, str, object]] = []
    for label, ratio in (("wider", cur * 1.5), ("narrower", cur / 1.5)):
        for method in ("crop", "scale", "stretch"):
            cases.append((method, "black", label, ratio))
        for method in ("pad", "fit"):
            for fill in ("black", "color", "mirror", "blur"):
                cases.append((method, fill, label, ratio))
    cases += [("pad", "mirror", "wider3", cur * 3.5), ("pad", "mirror", "narrower3", cur / 3.5),
              ("pad", "color", "wider3", cur * 3.5), ("pad", "blur", "narrower3", cur / 3.5)]
    cases += [(m, "black", "same", cur) for m in ("crop", "pad", "fit")]
    cases += [("pad", "black", "str-4:3", "4:3"), ("fit", "mirror", "str-2.0:1", "2.0:1"), ("crop", "black", "std-2.35", StandardAspectRatio.RATIO_2_35_1)]
    if name == BLUR_WIDE_NAME:
        cases = [c for c in cases if c[1] == "blur"]
    out = []
    for method, fill, label, target in cases:
        ratio = parse_target(target)
        if abs(cur - ratio) >= 0.01 and min(int(h * ratio), int(w / ratio)) < 1:
            continue
        out.append((f"{name}|{method}|{fill}|{label}", method, fill, target))
    return out


BLUR_WIDE_NAME = f"{BLUR_WIDE[0]}x{BLUR_WIDE[1]}"


def handler_for(method: str, fill: str, cls=AspectHandler, config_cls=AspectConfig, method_enum=ConversionMethod, fill_enum=FillMode):
    """The handler of a convert case, of this module or (with the four classes given) of another implementation."""
    return cls(config_cls(method=method_enum(method), fill_mode=fill_enum(fill), fill_color=FILL_COLOR))
