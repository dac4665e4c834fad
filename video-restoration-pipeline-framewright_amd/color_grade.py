"""Colour grade on the device (kernel set K15, csrc/color_lut.hip).

Step 7c of the reference's restore loop (src/framewright/restorer.py `_apply_seasonal_grade`) builds a 33^3 LUT with
`LUTManager.create_seasonal_lut` and runs `LUTManager.apply_to_image_fast` (src/framewright/integration/lut.py) over every PNG that
goes to reassembly: eight fancy-indexed gathers and seven lerps of an H x W x 3 float32 array per frame, on one host core.

`DeviceColorGrader` uploads the float32 table once and grades uint8 / uint16 frames that are already on the GPU in one elementwise
pass (`fw_lut3d_apply_u8` / `_u16`); the bytes are the reference's (tests/color_lut_ref.py is the contract).  The LUT builders and
the `.cube` reader and writer below are restated from what the reference computes, in its operation order, in float64; a 1D LUT on
8-bit frames becomes three byte tables, the reference's scalar path evaluated for the 256 values of each channel
(`fw_table3_apply_u8`).  As in `apply_to_image_fast`, a 3D LUT's domain is not applied.
"""
from __future__ import annotations

import ctypes as C
import logging
import re
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._stage import Stage, check_stack, fetch, upload

logger = logging.getLogger(__name__)

MIN_SIZE, MAX_SIZE = 2, 65          # what fw_lut3d_apply_* accepts


class LUTType(Enum):
    LUT_1D = "1d"
    LUT_3D = "3d"


@dataclass
class LUT:
    """A look-up table: ``data_3d`` is a float64 array size x size x size x 3 indexed [r][g][b], ``data_1d`` one of n x 3."""
    name: str = "Untitled"
    lut_type: LUTType = LUTType.LUT_3D
    size: int = 33
    domain_min: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    domain_max: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    data_1d: Optional[np.ndarray] = None
    data_3d: Optional[np.ndarray] = None
    title: str = ""
    comments: List[str] = field(default_factory=list)

    def table_f32(self) -> np.ndarray:
        """The float32 table `apply_to_image_fast` indexes: every entry rounded once from float64."""
        if self.lut_type != LUTType.LUT_3D or self.data_3d is None:
            raise ValueError("table_f32: a 3D LUT with data expected")
        return np.ascontiguousarray(np.asarray(self.data_3d, np.float64).astype(np.float32))

    def apply_to_rgb_array(self, rgb: np.ndarray) -> np.ndarray:
        """The reference's `LUT.apply_to_rgb` on an N x 3 float64 array: clamp to the domain, normalise, interpolate (float64)."""
        rgb = np.asarray(rgb, np.float64)
        dmin, dmax = np.asarray(self.domain_min, np.float64), np.asarray(self.domain_max, np.float64)
        v = np.maximum(dmin, np.minimum(dmax, rgb))
        if self.lut_type == LUTType.LUT_1D and self.data_1d is not None and len(self.data_1d):
            norm = (v - dmin) / (dmax - dmin)
            data = np.asarray(self.data_1d, np.float64)
            n = len(data)
            idx = norm * (n - 1)
            lo = idx.astype(np.int64)
            hi = np.minimum(lo + 1, n - 1)
            frac = idx - lo
            ch = np.arange(3)
            return (1 - frac) * data[lo, ch] + frac * data[hi, ch]
        if self.lut_type == LUTType.LUT_3D and self.data_3d is not None:
            norm = (v - dmin) / (dmax - dmin)
            data = np.asarray(self.data_3d, np.float64)
            s = self.size
            idx = norm * (s - 1)
            lo = idx.astype(np.int64)
            hi = np.minimum(lo + 1, s - 1)
            fr = idx - lo
            r0, g0, b0, r1, g1, b1 = lo[:, 0], lo[:, 1], lo[:, 2], hi[:, 0], hi[:, 1], hi[:, 2]
            rf, gf, bf = fr[:, 0:1], fr[:, 1:2], fr[:, 2:3]
            c00 = data[r0, g0, b0] * (1 - rf) + data[r1, g0, b0] * rf
            c01 = data[r0, g0, b1] * (1 - rf) + data[r1, g0, b1] * rf
            c10 = data[r0, g1, b0] * (1 - rf) + data[r1, g1, b0] * rf
            c11 = data[r0, g1, b1] * (1 - rf) + data[r1, g1, b1] * rf
            c0 = c00 * (1 - gf) + c10 * gf
            c1 = c01 * (1 - gf) + c11 * gf
            return c0 * (1 - bf) + c1 * bf
        return v


# ---- builders (LUTManager.create_*, restated) ---------------------------------------------------------------------------------------
def _axis(size: int) -> List[float]:
    return [i / (size - 1) for i in range(size)]


def _grid(r: Sequence[float], g: Sequence[float], b: Sequence[float]) -> np.ndarray:
    """table[ri][gi][bi] = (r[ri], g[gi], b[bi])"""
    size = len(r)
    t = np.empty((size, size, size, 3), np.float64)
    t[..., 0] = np.asarray(r, np.float64)[:, None, None]
    t[..., 1] = np.asarray(g, np.float64)[None, :, None]
    t[..., 2] = np.asarray(b, np.float64)[None, None, :]
    return t


def _check_size(size: int) -> int:
    size = int(size)
    if size < 2:
        raise ValueError("a LUT has at least two entries a side")
    return size


def create_identity_lut(size: int = 33, lut_type: LUTType = LUTType.LUT_3D) -> LUT:
    size = _check_size(size)
    ax = _axis(size)
    lut = LUT(name="Identity", lut_type=lut_type, size=size)
    if lut_type == LUTType.LUT_1D:
        lut.data_1d = np.repeat(np.asarray(ax, np.float64)[:, None], 3, axis=1)
    else:
        lut.data_3d = _grid(ax, ax, ax)
    return lut


def create_contrast_lut(contrast: float = 1.2, size: int = 33) -> LUT:
    """A 1D S-curve: sign(v - 0.5) |v - 0.5| ** (1 / contrast) + 0.5, clamped."""
    lut = create_identity_lut(size, LUTType.LUT_1D)
    lut.name = f"Contrast_{contrast:.1f}"

    def curve(val: float) -> float:
        centered = val - 0.5
        sign = 1 if centered >= 0 else -1
        return max(0, min(1, sign * (abs(centered) ** (1 / contrast)) + 0.5))

    lut.data_1d = np.repeat(np.asarray([curve(v) for v in _axis(lut.size)], np.float64)[:, None], 3, axis=1)
    return lut


FILM_STOCKS = {
    "kodak_vision3": {"r_lift": 0.02, "r_gamma": 1.05, "r_gain": 0.98, "g_lift": 0.01, "g_gamma": 1.0, "g_gain": 1.0,
                      "b_lift": 0.0, "b_gamma": 0.95, "b_gain": 1.02},
    "fuji_eterna": {"r_lift": 0.015, "r_gamma": 1.02, "r_gain": 0.97, "g_lift": 0.02, "g_gamma": 1.0, "g_gain": 0.99,
                    "b_lift": 0.025, "b_gamma": 0.98, "b_gain": 1.01},
    "kodachrome": {"r_lift": 0.03, "r_gamma": 1.1, "r_gain": 1.0, "g_lift": 0.02, "g_gamma": 1.05, "g_gain": 0.98,
                   "b_lift": 0.01, "b_gamma": 0.95, "b_gain": 0.95},
    "ektachrome": {"r_lift": 0.01, "r_gamma": 1.08, "r_gain": 0.99, "g_lift": 0.015, "g_gamma": 1.02, "g_gain": 1.0,
                   "b_lift": 0.02, "b_gamma": 1.0, "b_gain": 1.02},
}

SEASONS = {
    "winter": {"r_lift": -0.02, "r_gamma": 0.97, "r_gain": 0.95, "g_lift": -0.01, "g_gamma": 0.98, "g_gain": 0.96,
               "b_lift": 0.04, "b_gamma": 1.04, "b_gain": 1.02, "saturation": 0.75},
    "spring": {"r_lift": 0.01, "r_gamma": 1.02, "r_gain": 1.00, "g_lift": 0.02, "g_gamma": 1.04, "g_gain": 1.02,
               "b_lift": 0.01, "b_gamma": 1.00, "b_gain": 0.98, "saturation": 0.90},
    "summer": {"r_lift": 0.02, "r_gamma": 1.06, "r_gain": 1.02, "g_lift": 0.02, "g_gamma": 1.04, "g_gain": 1.01,
               "b_lift": -0.01, "b_gamma": 0.96, "b_gain": 0.96, "saturation": 1.15},
    "autumn": {"r_lift": 0.03, "r_gamma": 1.08, "r_gain": 1.02, "g_lift": 0.01, "g_gamma": 1.00, "g_gain": 0.96,
               "b_lift": -0.02, "b_gamma": 0.94, "b_gain": 0.92, "saturation": 1.05},
}


def create_film_emulation_lut(film_stock: str = "kodak_vision3", size: int = 33) -> LUT:
    """Per channel (v * gain + lift) ** (1 / gamma), clamped; an unknown stock is kodak_vision3, as in the reference."""
    lut = create_identity_lut(size, LUTType.LUT_3D)
    lut.name = f"Film_{film_stock}"
    lut.title = f"Film Emulation: {film_stock}"
    p = FILM_STOCKS.get(film_stock, FILM_STOCKS["kodak_vision3"])

    def channel(val: float, lift: float, gamma: float, gain: float) -> float:
        val = val * gain + lift
        val = val ** (1 / gamma)
        return max(0, min(1, val))

    ax = _axis(lut.size)
    lut.data_3d = _grid(*[[channel(v, p[c + "_lift"], p[c + "_gamma"], p[c + "_gain"]) for v in ax] for c in "rgb"])
    return lut


def create_seasonal_lut(season: str = "winter", strength: float = 1.0, size: int = 33) -> LUT:
    """Per channel lift / gamma / gain, then a saturation change about the Rec. 709 luma; the preset is blended toward the
    identity by ``strength``."""
    if season not in SEASONS:
        raise ValueError(f"Unknown season '{season}'. Valid seasons: {list(SEASONS.keys())}")
    lut = create_identity_lut(size, LUTType.LUT_3D)
    lut.name = f"Seasonal_{season}"
    lut.title = f"Seasonal Color Grade: {season} (strength={strength:.1f})"
    p = SEASONS[season]

    def lerp(a: float, b: float, t: float) -> float:
        return a + (b - a) * t

    def grade(val: float, lift: float, gamma: float, gain: float) -> float:
        val = val * gain + lift
        val = max(0.0, min(1.0, val))
        if gamma != 1.0 and val > 0:
            val = val ** (1.0 / gamma)
        return max(0.0, min(1.0, val))

    ax = _axis(lut.size)
    chans = [[grade(v, lerp(0, p[c + "_lift"], strength), lerp(1.0, p[c + "_gamma"], strength), lerp(1.0, p[c + "_gain"], strength))
              for v in ax] for c in "rgb"]
    sat = lerp(1.0, p["saturation"], strength)
    t = _grid(*chans)
    r, g, b = t[..., 0], t[..., 1], t[..., 2]
    luma = 0.2126 * r + 0.7152 * g + 0.0722 * b           # float64 products and sums, left to right: no contraction in numpy
    lut.data_3d = np.clip(np.stack([luma + (r - luma) * sat, luma + (g - luma) * sat, luma + (b - luma) * sat], axis=-1), 0.0, 1.0)
    return lut


def combine_luts(luts: Sequence[LUT], size: int = 33) -> LUT:
    """One 3D LUT that applies ``luts`` in turn to every grid point (each with its own domain and interpolation, in float64)."""
    result = create_identity_lut(size, LUTType.LUT_3D)
    result.name = "Combined"
    result.title = " + ".join(lut.name for lut in luts)
    rgb = result.data_3d.reshape(-1, 3)
    for lut in luts:
        rgb = lut.apply_to_rgb_array(rgb)
    result.data_3d = rgb.reshape(result.size, result.size, result.size, 3)
    return result


# ---- .cube ----------------------------------------------------------------------------------------------------------------------------
def read_cube(path) -> LUT:
    """A `.cube` file (1D or 3D): TITLE, LUT_1D_SIZE, LUT_3D_SIZE, DOMAIN_MIN, DOMAIN_MAX, `#` comments, then the rows - red
    fastest for a 3D table.  Rows that are missing are the identity's, as in the reference's parser."""
    path = Path(path)
    lut = LUT(name=path.stem)
    rows: List[Tuple[float, float, float]] = []
    for line in path.read_text(encoding="utf-8", errors="replace").split("\n"):
        line = line.strip()
        if not line:
            continue
        if line.startswith("#"):
            lut.comments.append(line[1:].strip())
            continue
        if line.startswith("TITLE"):
            m = re.match(r'TITLE\s+"?([^"]+)"?', line)
            if m:
                lut.title = m.group(1)
            continue
        if line.startswith("LUT_1D_SIZE") or line.startswith("LUT_3D_SIZE"):
            m = re.match(r"LUT_[13]D_SIZE\s+(\d+)", line)
            if m:
                lut.lut_type = LUTType.LUT_1D if line.startswith("LUT_1D") else LUTType.LUT_3D
                lut.size = int(m.group(1))
            continue
        if line.startswith("DOMAIN_MIN"):
            lut.domain_min = tuple(float(v) for v in line.split()[1:4])
            continue
        if line.startswith("DOMAIN_MAX"):
            lut.domain_max = tuple(float(v) for v in line.split()[1:4])
            continue
        parts = line.split()
        if len(parts) >= 3:
            try:
                rows.append((float(parts[0]), float(parts[1]), float(parts[2])))
            except ValueError:
                pass
    if lut.lut_type == LUTType.LUT_1D:
        lut.data_1d = np.asarray(rows, np.float64).reshape(-1, 3)
        return lut
    size = _check_size(lut.size)
    data = create_identity_lut(size).data_3d
    flat = np.asarray(rows[:size ** 3], np.float64).reshape(-1, 3)
    # row i belongs to r = i % size, g = (i // size) % size, b = i // size^2
    by_bgr = data.transpose(2, 1, 0, 3).reshape(-1, 3).copy()
    by_bgr[:len(flat)] = flat
    lut.data_3d = np.ascontiguousarray(by_bgr.reshape(size, size, size, 3).transpose(2, 1, 0, 3))
    return lut


def write_cube(lut: LUT, path) -> None:
    """The reference's `.cube` text: title, comments, the domain when it is not [0, 1], the size, ten decimals per value."""
    lines = [f'TITLE "{lut.title or lut.name}"']
    lines += [f"# {c}" for c in lut.comments]
    lines.append("")
    if tuple(lut.domain_min) != (0.0, 0.0, 0.0):
        lines.append("DOMAIN_MIN {} {} {}".format(*lut.domain_min))
    if tuple(lut.domain_max) != (1.0, 1.0, 1.0):
        lines.append("DOMAIN_MAX {} {} {}".format(*lut.domain_max))
    if lut.lut_type == LUTType.LUT_1D:
        rows = np.asarray(lut.data_1d, np.float64).reshape(-1, 3) if lut.data_1d is not None else np.zeros((0, 3))
        lines += [f"LUT_1D_SIZE {len(rows) if len(rows) else lut.size}", ""]
    else:
        rows = np.asarray(lut.data_3d, np.float64).transpose(2, 1, 0, 3).reshape(-1, 3) if lut.data_3d is not None else np.zeros((0, 3))
        lines += [f"LUT_3D_SIZE {lut.size}", ""]
    lines += [f"{r:.10f} {g:.10f} {b:.10f}" for r, g, b in rows.tolist()]
    Path(path).write_text("\n".join(lines), encoding="utf-8")


# ---- what the device is given -----------------------------------------------------------------------------------------------------
def check_finite(lut: LUT) -> None:
    """The reference's result for a table with a NaN or an infinity is undefined (`astype(uint8)` of a NaN): refused."""
    data = lut.data_1d if lut.lut_type == LUTType.LUT_1D else lut.data_3d
    if data is None or not np.asarray(data).size:
        raise ValueError("LUT without data")
    if not np.all(np.isfinite(np.asarray(data, np.float64))):
        raise ValueError("LUT with a non-finite entry")
    if lut.lut_type == LUTType.LUT_1D and not np.all(np.isfinite(np.asarray([lut.domain_min, lut.domain_max], np.float64))):
        raise ValueError("LUT with a non-finite domain")


def byte_tables_1d(lut: LUT, bgr: bool = True) -> np.ndarray:
    """3 x 256 uint8, one table per STORED channel: what the reference's `apply_to_image` (the path `apply_to_image_fast` takes for
    a 1D LUT) makes of every 8-bit value.  Restated with its types: the normalised sample is float32, `apply_to_rgb` clamps it with
    Python's min / max (a sample at or beyond the domain's edge becomes the edge, a Python float, and the rest of that sample's
    arithmetic is float64), `_apply_1d` interpolates, the result is stored as float32, clipped, scaled and truncated."""
    if lut.lut_type != LUTType.LUT_1D:
        raise ValueError("byte_tables_1d: a 1D LUT expected")
    check_finite(lut)
    data = np.asarray(lut.data_1d, np.float64).reshape(-1, 3)
    n = len(data)
    f32 = np.float32
    out = np.empty((3, 256), np.uint8)
    with np.errstate(all="ignore"):
        for c in range(3):                      # LUT channel: 0 = red
            dmin, dmax = float(lut.domain_min[c]), float(lut.domain_max[c])
            for v in range(256):
                x = f32(v) / f32(255.0)
                r = x if x < f32(dmax) else dmax                         # min(dmax, x): numpy compares a float32 scalar with a
                if isinstance(r, float):                                 # Python float in float32
                    r = r if r > dmin else dmin                          # max(dmin, .)
                else:
                    r = r if r > f32(dmin) else dmin
                T = np.float64 if isinstance(r, float) else f32
                norm = (T(r) - T(dmin)) / T(dmax - dmin)
                idx = norm * T(n - 1)
                lo = int(idx)
                hi = min(lo + 1, n - 1)
                frac = idx - T(lo)
                val = f32((T(1) - frac) * T(data[lo][c]) + frac * T(data[hi][c]))
                out[2 - c if bgr else c, v] = np.uint8(min(max(val, f32(0)), f32(1)) * f32(255))
    return out


def _read_png_bgr(path: Path) -> Optional[np.ndarray]:
    """`cv2.imread(path)`: 8-bit BGR whatever the file holds; through Pillow where cv2 is absent (as rife.py reads its frames)."""
    try:
        import cv2
        return cv2.imread(str(path))
    except ImportError:
        from PIL import Image
        try:
            with Image.open(str(path)) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
        except Exception:  # noqa: BLE001 - cv2.imread returns None for what it cannot read
            return None


class DeviceColorGrader(Stage):
    """A LUT held on one GPU and applied to frames there.  3D LUTs of 2 .. 65 entries a side grade uint8 and uint16 frames; a 1D
    LUT grades uint8 frames through three byte tables.  ``bgr`` (default, OpenCV's order) says that channel 0 of a frame is blue."""

    def __init__(self, lut: LUT, device_id: int = 0, bgr: bool = True):
        check_finite(lut)
        self.lut = lut
        self.device_id = int(device_id)
        self.bgr = bool(bgr)
        super().__init__(self.device_id)
        if lut.lut_type == LUTType.LUT_3D:
            table = lut.table_f32()
            self.size = int(table.shape[0])
            if table.shape != (self.size, self.size, self.size, 3) or not MIN_SIZE <= self.size <= MAX_SIZE:
                raise ValueError(f"a 3D LUT of {MIN_SIZE} .. {MAX_SIZE} entries a side expected")
            self._table = upload(table, self._dev)
        else:
            self.size = 0
            self._table = upload(byte_tables_1d(lut, self.bgr), self._dev)

    # ---- one launch ------------------------------------------------------------------------------------------------------------
    def _launch(self, src_ptr: int, src_stride: int, n: int, h: int, w: int, wide: bool, dst_ptr: int, dst_stride: int, dev) -> None:
        st = _lib.stream_ptr(dev)
        if self.size:
            fn = self._lib.fw_lut3d_apply_u16 if wide else self._lib.fw_lut3d_apply_u8
            _lib.check(fn(C.c_void_p(src_ptr), src_stride, n, h, w, _lib.ptr(self._table), self.size, int(self.bgr),
                          C.c_void_p(dst_ptr), dst_stride, st))
        else:
            if wide:
                raise ValueError("a 1D LUT grades 8-bit frames only")
            _lib.check(self._lib.fw_table3_apply_u8(C.c_void_p(src_ptr), src_stride, n, h, w, _lib.ptr(self._table),
                                                    C.c_void_p(dst_ptr), dst_stride, st))

    @staticmethod
    def _check(t, dims: int):
        import torch
        check_stack(t, dims, "uint8 or uint16 (or int16 holding those bits) CUDA tensors [n x] H x W x 3 expected",
                    dtypes=(torch.uint8, torch.uint16, torch.int16))
        return t.dtype != torch.uint8

    def _clip(self, clip, inplace: bool):
        """n x H x W x 3: one launch.  Frames that are contiguous in themselves may lie any stride apart."""
        import torch
        wide = self._check(clip, 4)
        if clip.device != self._dev:
            raise ValueError(f"frames on {clip.device}, the LUT on {self._dev}")
        n, h, w = (int(v) for v in clip.shape[:3])
        if n == 0 or h == 0 or w == 0:
            return clip if inplace else clip.clone()
        item = 2 if wide else 1
        framewise = clip[0].is_contiguous() and (n == 1 or clip.stride(0) >= h * w * 3)
        if not framewise:
            if inplace:
                raise ValueError("in place needs frames that are contiguous in themselves")
            clip = clip.contiguous()
        out = clip if inplace else torch.empty((n, h, w, 3), dtype=clip.dtype, device=clip.device)
        for k in range(0, n, 65535):
            m = min(65535, n - k)
            self._launch(clip[k].data_ptr(), clip.stride(0) * item, m, h, w, wide, out[k].data_ptr(), out.stride(0) * item, clip.device)
        return out

    @_lib.on_tensor_device
    def apply_device(self, frames, inplace: bool = False):
        """A uint8 / uint16 n x H x W x 3 CUDA tensor -> a new tensor of the same shape (one launch); a list of H x W x 3 CUDA
        tensors -> a list of new tensors (one launch each, one allocation for frames of one size).  ``inplace=True`` overwrites the
        frames and returns them.  The work is queued on torch's current stream of the frames' device."""
        import torch
        if isinstance(frames, torch.Tensor):
            return self._clip(frames, inplace)
        frames = list(frames)
        for f in frames:
            self._check(f, 3)
        if inplace:
            if any(not f.is_contiguous() for f in frames):
                raise ValueError("in place needs contiguous frames")
            outs = frames
        else:
            frames = [f.contiguous() for f in frames]
            outs = _lib.empty_like_many(frames)
        for f, o in zip(frames, outs):
            self._launch_pair(f, o)
        return outs

    def _launch_pair(self, f, o) -> None:
        if f.device != self._dev:
            raise ValueError(f"frames on {f.device}, the LUT on {self._dev}")
        h, w = int(f.shape[0]), int(f.shape[1])
        if h and w:
            self._launch(f.data_ptr(), 0, 1, h, w, self._check(f, 3), o.data_ptr(), 0, f.device)

    @_lib.on_tensor_device
    def apply(self, image: np.ndarray) -> np.ndarray:
        """Host in, host out: an H x W x 3 or n x H x W x 3 uint8 / uint16 array."""
        a = np.ascontiguousarray(image)
        if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError("apply expects a uint8 or uint16 array [n x] H x W x 3")
        wide = a.dtype == np.uint16
        t = upload(a.view(np.int16) if wide else a, self._dev)                        # the bytes only
        res = fetch(self._dev, self._clip(t if a.ndim == 4 else t.unsqueeze(0), True)).reshape(a.shape)
        return res.view(np.uint16) if wide else res

    # ---- the reference's step 7c ---------------------------------------------------------------------------------------------------
    @classmethod
    def grade_directory(cls, frames_dir, season: str, strength: float = 0.7, progress: Optional[Callable[[float], None]] = None,
                        device_id: int = 0) -> int:
        """`_apply_seasonal_grade`: every `*.png` of ``frames_dir``, sorted, is read as 8-bit BGR, graded with the seasonal 33^3 LUT
        and written back under its own name.  ``progress`` is called at 0, at every 100th frame and at the last.  An empty
        directory is a warning; a frame that fails is logged and skipped.  Returns the number of frames graded."""
        from .realesrgan import _imwrite
        frames_dir = Path(frames_dir)
        grader = cls(create_seasonal_lut(season=season, strength=strength), device_id=device_id)
        files = sorted(frames_dir.glob("*.png"))
        total = len(files)
        if total == 0:
            logger.warning("No frames found for seasonal grading")
            return 0
        if progress:
            progress(0.0)
        done = 0
        for i, path in enumerate(files):
            try:
                img = _read_png_bgr(path)
                if img is not None:
                    _imwrite(path, grader.apply(img))
                    done += 1
            except Exception as e:  # noqa: BLE001 - the reference logs and goes on
                logger.warning(f"Seasonal grade failed for {path.name}: {e}")
            if progress and ((i + 1) % 100 == 0 or (i + 1) == total):
                progress((i + 1) / total)
        logger.info(f"Seasonal color grade ({season}) applied to {total} frames")
        return done
