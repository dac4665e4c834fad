"""SDR to HDR conversion of final frames on the device (kernel set K20, csrc/hdr.hip).

The reference's `processors/hdr_conversion.py` turns the 8-bit BGR frames the chain produces into 16-bit PQ (HDR10) or HLG frames in
BT.2020: `HDRConverter.convert_frame` is a dozen full-frame float32 numpy passes and four cv2 calls on one host core, on the largest
frames there are (7680 x 4320 behind the x4 upscale).  `DeviceHDRConverter` converts uint8 / uint16 frames that are already on the
GPU in at most two passes and one small launch (`fw_hdr_convert`); tests/hdr_ref.py is the contract.

Every table that a transcendental function goes into is built here, once per config, on the host, with the reference's own numpy
expressions, and uploaded: the gamma table (256 or 65536 float32 entries), the 2 x 256 tail table - the PQ / HLG transfer and the
16-bit quantisation of every byte and of every byte times 0.95 - and the code from which the highlight flag is set.  Every Python
float that the reference lets meet a float32 array is rounded to float32 here, as numpy does, and handed to the kernel.

Not built: `analyze_dynamic_range`, so `HDRConversionResult.max_cll`, `max_fall` and `avg_dynamic_range_stops` stay at their defaults
in `convert_directory` (they need order statistics and a float32 mean); `convert_video`, `is_hdr_source` and the ffmpeg filter strings.
"""
from __future__ import annotations

import ctypes as C
import logging
import shutil
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Callable, Iterable, Iterator, List, Optional

import numpy as np

from . import _lib
from ._stage import Stage, check_stack, fetch, upload

logger = logging.getLogger(__name__)

BATCH = 32                                       # frames of one launch (the kernel argument table)
MIN_SIDE, MAX_SIDE = 8, 16384                    # CLAHE has 8 x 8 tiles
f32 = np.float32


class HDRFormat(Enum):
    HDR10 = "hdr10"
    HDR10_PLUS = "hdr10plus"
    DOLBY_VISION = "dolby_vision"
    HLG = "hlg"


class ToneMapping(Enum):
    REINHARD = "reinhard"
    ACES = "aces"
    HABLE = "hable"
    MOBIUS = "mobius"


class ColorSpace(Enum):
    BT2020 = "bt2020"
    P3 = "p3"
    REC709 = "rec709"


@dataclass
class HDRConfig:
    """The reference's fields, defaults, validation and string coercion.  ``max_content_light_level``, ``max_frame_avg_light_level``
    and ``shadow_detail`` play no part in the frame path (they do not in the reference either)."""
    target_format: HDRFormat = HDRFormat.HDR10
    peak_brightness: int = 1000
    tone_mapping: ToneMapping = ToneMapping.ACES
    color_space: ColorSpace = ColorSpace.BT2020
    enable_local_contrast: bool = True
    max_content_light_level: Optional[int] = None
    max_frame_avg_light_level: Optional[int] = None
    saturation_boost: float = 1.1
    highlight_recovery: bool = True
    shadow_detail: float = 1.0

    def __post_init__(self) -> None:
        if not 400 <= self.peak_brightness <= 10000:
            raise ValueError(f"peak_brightness must be between 400 and 10000 nits, got {self.peak_brightness}")
        if not 0.8 <= self.saturation_boost <= 1.5:
            raise ValueError(f"saturation_boost must be between 0.8 and 1.5, got {self.saturation_boost}")
        if not 0.0 <= self.shadow_detail <= 2.0:
            raise ValueError(f"shadow_detail must be between 0.0 and 2.0, got {self.shadow_detail}")
        if isinstance(self.target_format, str):
            self.target_format = HDRFormat(self.target_format.lower())
        if isinstance(self.tone_mapping, str):
            self.tone_mapping = ToneMapping(self.tone_mapping.lower())
        if isinstance(self.color_space, str):
            self.color_space = ColorSpace(self.color_space.lower())


@dataclass
class HDRConversionResult:
    frames_processed: int = 0
    frames_converted: int = 0
    frames_skipped: int = 0
    failed_frames: int = 0
    output_dir: Optional[Path] = None
    max_cll: int = 0                        # not measured here: see the module docstring
    max_fall: int = 0
    avg_dynamic_range_stops: float = 0.0


class _Params(C.Structure):
    """`fw_hdr_params` of include/framewright_hip.h"""
    _fields_ = [("matrix", C.c_float * 9), ("lum_weights", C.c_float * 3), ("curve_k", C.c_float * 8), ("transfer_k", C.c_float * 8),
                ("lum_floor", C.c_float), ("recover_gain", C.c_float), ("saturation_boost", C.c_float), ("hue_scale", C.c_float),
                ("use_matrix", C.c_int32), ("curve", C.c_int32), ("transfer", C.c_int32), ("local_contrast", C.c_int32),
                ("saturation", C.c_int32), ("recover", C.c_int32), ("clip_code", C.c_int32)]


MATRIX_709_2020 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]], dtype=np.float32)
_CURVES = {ToneMapping.REINHARD: 0, ToneMapping.ACES: 1, ToneMapping.HABLE: 2, ToneMapping.MOBIUS: 3}
_PQ = (HDRFormat.HDR10, HDRFormat.HDR10_PLUS, HDRFormat.DOLBY_VISION)


def saturation_on(config: HDRConfig) -> bool:
    return abs(config.saturation_boost - 1.0) > 0.01


def curve_constants(config: HDRConfig) -> List[float]:
    """The Python floats of `_apply_tone_mapping`, evaluated in float64 as Python evaluates them (the kernel receives them as float32)."""
    peak_scale = config.peak_brightness / 100.0
    if config.tone_mapping == ToneMapping.REINHARD:
        return [peak_scale ** 2]
    if config.tone_mapping == ToneMapping.ACES:
        return [peak_scale, 2.51, 0.03, 2.43, 0.59, 0.14]
    if config.tone_mapping == ToneMapping.HABLE:
        A, B, Cc, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
        white = ((peak_scale * (A * peak_scale + Cc * B) + D * E) / (peak_scale * (A * peak_scale + B) + D * F)) - E / F
        return [peak_scale, A, Cc * B, D * E, B, D * F, E / F, 1.0 / white]
    transition, slope = 0.3, 0.8
    return [peak_scale, transition, 1.0 - transition, -slope]


def transfer_constants(config: HDRConfig) -> List[float]:
    if config.target_format in _PQ:
        return [config.peak_brightness / 10000.0, 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0, 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0,
                2392.0 / 4096.0 * 32.0]
    return [1.0 / 12.0, 0.17883277, 0.28466892, 0.55991073]


def transfer_numpy(x: np.ndarray, config: HDRConfig) -> np.ndarray:
    """`_apply_pq_transfer` / `_apply_hlg_transfer` on a float32 array, with the reference's expressions."""
    if config.target_format in _PQ:
        m1, m2, c1, c2, c3 = transfer_constants(config)[1:]
        L = np.clip(x, 0, 1) * (config.peak_brightness / 10000.0)
        Lm1 = np.power(L, m1)
        return np.clip(np.power((c1 + c2 * Lm1) / (1.0 + c3 * Lm1), m2), 0, 1)
    _, a, b, c = transfer_constants(config)
    E = np.clip(x, 0, 1)
    with np.errstate(all="ignore"):                       # the reference evaluates the log branch for every value and discards
        E_prime = np.where(E <= 1.0 / 12.0, np.sqrt(3.0 * E), a * np.log(12.0 * E - b) + c)
    return np.clip(E_prime, 0, 1)


def host_tables(config: HDRConfig) -> dict:
    """gamma8 / gamma16 (float32), tail (uint16 [2][256]), clip8 / clip16 (the first flagged code), hsv_div (int32 [512])."""
    x8 = np.arange(256).astype(np.uint8).astype(f32) / 255.0
    x16 = np.arange(65536).astype(np.uint16).astype(f32) / 65535.0
    tail = np.clip(transfer_numpy(np.stack([x8, x8 * 0.95]), config) * 65535.0, 0, 65535).astype(np.uint16)

    def first(mask):
        idx = np.flatnonzero(mask)
        return int(idx[0]) if idx.size else int(mask.size)

    div = np.zeros(512, np.int32)
    i = np.arange(1, 256, dtype=np.float64)
    div[1:256] = np.rint((255 << 12) / i)
    div[257:] = np.rint((180 << 12) / (6.0 * i))
    return {"gamma8": np.power(np.clip(x8, 0.0, 1.0), 2.2), "gamma16": np.power(np.clip(x16, 0.0, 1.0), 2.2), "tail": tail,
            "clip8": first(x8 > 0.98), "clip16": first(x16 > 0.98), "hsv_div": div}


def make_params(config: HDRConfig, clip_code: int) -> _Params:
    p = _Params()
    p.matrix[:] = [float(v) for v in MATRIX_709_2020.ravel()]
    p.lum_weights[:] = [float(f32(v)) for v in (0.0722, 0.7152, 0.2126)]
    ck = curve_constants(config)
    p.curve_k[:] = [float(f32(v)) for v in ck] + [0.0] * (8 - len(ck))
    tk = transfer_constants(config)
    p.transfer_k[:] = [float(f32(v)) for v in tk] + [0.0] * (8 - len(tk))
    p.lum_floor, p.recover_gain = float(f32(0.0001)), float(f32(0.95))
    p.saturation_boost, p.hue_scale = float(f32(config.saturation_boost)), float(f32(6 / 180))
    p.use_matrix = int(config.color_space in (ColorSpace.BT2020, ColorSpace.P3))       # P3 takes the BT.2020 matrix, as in the reference
    p.curve, p.transfer = _CURVES[config.tone_mapping], int(config.target_format not in _PQ)
    p.local_contrast, p.saturation = int(bool(config.enable_local_contrast)), int(saturation_on(config))
    p.recover, p.clip_code = int(bool(config.highlight_recovery)), int(clip_code)
    return p


def _read_image(path: Path) -> Optional[np.ndarray]:
    """`cv2.imread(path, IMREAD_UNCHANGED)` where cv2 is present, else 8-bit BGR through Pillow; None for what cannot be read."""
    try:
        import cv2
        return cv2.imread(str(path), cv2.IMREAD_UNCHANGED)
    except ImportError:
        from PIL import Image
        try:
            with Image.open(str(path)) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
        except Exception:  # noqa: BLE001 - cv2.imread returns None for what it cannot read
            return None


def _write_image(path: Path, frame: np.ndarray) -> None:
    import cv2                                           # a 16-bit three-channel PNG: Pillow has no such mode; inject `write` without cv2
    cv2.imwrite(str(path), frame)


class DeviceHDRConverter(Stage):
    """The reference's `HDRConverter` frame path on uint8 / uint16 BGR CUDA frames of one GPU; the results are new uint16 tensors.
    Work is queued on torch's current stream of the frames' device and nothing waits."""

    def __init__(self, config: Optional[HDRConfig] = None, gpu_id: int = 0):
        self.config = config or HDRConfig()
        self.gpu_id = int(gpu_id)
        super().__init__(self.gpu_id)
        t = host_tables(self.config)
        self._clip = {1: t["clip8"], 2: t["clip16"]}
        self._params = {b: make_params(self.config, self._clip[b]) for b in (1, 2)}
        self._gamma = {1: upload(t["gamma8"], self._dev), 2: None}
        self._gamma16_host = t["gamma16"]                              # uploaded with the first 16-bit frame (256 KiB)
        self._tail = upload(t["tail"].view(np.int16), self._dev)
        self._div = upload(t["hsv_div"], self._dev)
        self._wrong = "hdr: uint8 or uint16 CUDA tensors H x W x 3 (BGR) expected"
        self._closed = False

    def is_available(self) -> bool:
        return not self._closed

    def close(self) -> None:
        """Releases the tables and the scratch; calls that arrive afterwards raise."""
        self._closed = True
        self._gamma, self._tail, self._div, self._scratch = {1: None, 2: None}, None, None, None

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def _check(self, f) -> int:
        """-> bytes a sample"""
        import torch
        if self._closed:
            raise ValueError("hdr: the converter is closed")
        check_stack(f, 3, self._wrong, dtypes=(torch.uint8, torch.uint16, torch.int16))
        if f.device != self._dev:
            raise ValueError(f"hdr: frames on cuda:{self.gpu_id}, the converter's device, expected")
        h, w = int(f.shape[0]), int(f.shape[1])
        if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
            raise ValueError("hdr: frames of 8 .. 16384 pixels a side expected")
        return 1 if f.dtype == torch.uint8 else 2

    def _gamma_for(self, b: int):
        if self._gamma[b] is None:
            self._gamma[2] = upload(self._gamma16_host, self._dev)
        return self._gamma[b]

    def _scratch_for(self, n: int):
        if not self.config.enable_local_contrast:
            return None
        return self.scratch(int(self._lib.fw_hdr_scratch_bytes(n)), self._dev)

    # ---- frames ----------------------------------------------------------------------------------------------------------------
    @_lib.on_tensor_device
    def convert_device(self, frames) -> list:
        """A list of uint8 / uint16 H x W x 3 BGR CUDA tensors (one tensor may appear several times) -> a list of new uint16
        tensors, one allocation for frames of one shape; launches of up to 32 frames of one shape and type."""
        import torch
        frames = list(frames)
        if not frames:
            return []
        widths = [self._check(f) for f in frames]
        frames = [f if f.is_contiguous() else f.contiguous() for f in frames]
        same = all(f.shape == frames[0].shape for f in frames)
        if same:
            buf = torch.empty((len(frames),) + tuple(frames[0].shape), dtype=torch.uint16, device=self._dev)
            outs = list(buf.unbind(0))
        else:
            outs = [torch.empty(tuple(f.shape), dtype=torch.uint16, device=self._dev) for f in frames]
        st = _lib.stream_ptr(self._dev)
        k = 0
        while k < len(frames):
            m = k + 1
            while m < len(frames) and m - k < BATCH and frames[m].shape == frames[k].shape and widths[m] == widths[k]:
                m += 1
            b, n = widths[k], m - k
            h, w = int(frames[k].shape[0]), int(frames[k].shape[1])
            _lib.check(self._lib.fw_hdr_convert(_lib.ptr_table(frames[k:m]), _lib.ptr_table(outs[k:m]), n, h, w, b, C.byref(self._params[b]),
                                                _lib.ptr(self._gamma_for(b)), _lib.ptr(self._tail), _lib.ptr(self._div),
                                                _lib.ptr(self._scratch_for(n)), st))
            k = m
        return outs

    def convert_frames(self, frames) -> list:
        return self.convert_device(frames)

    def convert_frame(self, frame):
        return self.convert_device([frame])[0]

    def stream(self, frames: Iterable) -> Iterator:
        """Yields the converted frame of every frame of an iterator, in order; nothing is held back."""
        for f in frames:
            yield self.convert_device([f])[0]

    def convert_numpy(self, frame: np.ndarray) -> np.ndarray:
        """Host in, host out: a uint8 / uint16 H x W x 3 array -> uint16."""
        import torch
        a = np.ascontiguousarray(frame)
        if a.dtype not in (np.uint8, np.uint16) or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("hdr: a uint8 or uint16 array H x W x 3 (BGR) expected")
        with self.host() as dev:
            t = upload(a.view(np.int16) if a.dtype == np.uint16 else a, dev)                  # the bytes only
            return fetch(dev, self.convert_device([t])[0].view(torch.int16)).view(np.uint16)

    # ---- the stages alone (what tests/test_hdr_gpu.py holds to tests/hdr_ref.py) ------------------------------------------------
    @_lib.on_tensor_device
    def tone_mapped_plane(self, frame, recover: bool = False):
        """Steps 1 - 3 as a float32 H x W x 3 tensor; ``recover``: times 0.95 where the highlight flag is set (the float path's input
        of the transfer function)."""
        import torch
        b = self._check(frame)
        frame = frame.contiguous()
        out = torch.empty(tuple(frame.shape), dtype=torch.float32, device=self._dev)
        _lib.check(self._lib.fw_hdr_tonemap_f32(_lib.ptr(frame), int(frame.shape[0]), int(frame.shape[1]), b, C.byref(self._params[b]),
                                                _lib.ptr(self._gamma_for(b)), int(bool(recover)), _lib.ptr(out), _lib.stream_ptr(self._dev)))
        return out

    @_lib.on_tensor_device
    def quantised_plane(self, frame):
        import torch
        b = self._check(frame)
        frame = frame.contiguous()
        out = torch.empty(tuple(frame.shape), dtype=torch.uint8, device=self._dev)
        _lib.check(self._lib.fw_hdr_quantise_u8(_lib.ptr(frame), int(frame.shape[0]), int(frame.shape[1]), b, C.byref(self._params[b]),
                                                _lib.ptr(self._gamma_for(b)), _lib.ptr(out), _lib.stream_ptr(self._dev)))
        return out

    @_lib.on_tensor_device
    def clahe(self, plane):
        """cv2.createCLAHE(2.0, (8, 8)).apply on a uint8 H x W CUDA tensor."""
        import torch
        if self._closed:
            raise ValueError("hdr: the converter is closed")
        if not isinstance(plane, torch.Tensor) or plane.dtype != torch.uint8 or not plane.is_cuda or plane.dim() != 2 or plane.device != self._dev:
            raise ValueError("hdr: a uint8 CUDA tensor H x W on the converter's device expected")
        h, w = int(plane.shape[0]), int(plane.shape[1])
        if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
            raise ValueError("hdr: frames of 8 .. 16384 pixels a side expected")
        plane = plane.contiguous()
        out = torch.empty_like(plane)
        scratch = self.scratch(int(self._lib.fw_hdr_scratch_bytes(1)), self._dev)
        _lib.check(self._lib.fw_hdr_clahe_u8(_lib.ptr(plane), h, w, _lib.ptr(scratch), _lib.ptr(out), _lib.stream_ptr(self._dev)))
        return out

    @_lib.on_tensor_device
    def saturate(self, bgr, boost: Optional[float] = None):
        """`_adjust_saturation` on bytes: a uint8 [...] x 3 CUDA tensor through integer HSV, the boost and float32 HSV -> BGR."""
        import torch
        if self._closed:
            raise ValueError("hdr: the converter is closed")
        if not isinstance(bgr, torch.Tensor) or bgr.dtype != torch.uint8 or not bgr.is_cuda or bgr.shape[-1] != 3 or bgr.device != self._dev \
                or bgr.numel() == 0:
            raise ValueError("hdr: a uint8 CUDA tensor [...] x 3 (BGR) on the converter's device expected")
        bgr = bgr.contiguous()
        out = torch.empty_like(bgr)
        boost = self.config.saturation_boost if boost is None else boost
        _lib.check(self._lib.fw_hdr_saturation_u8(_lib.ptr(bgr), bgr.numel() // 3, _lib.ptr(self._div), float(f32(boost)), float(f32(6 / 180)),
                                                  _lib.ptr(out), _lib.stream_ptr(self._dev)))
        return out

    @_lib.on_tensor_device
    def transfer(self, plane):
        """The config's transfer function and the 16-bit quantisation of a float32 CUDA tensor, evaluated per value in float32."""
        import torch
        if self._closed:
            raise ValueError("hdr: the converter is closed")
        if not isinstance(plane, torch.Tensor) or plane.dtype != torch.float32 or not plane.is_cuda or plane.device != self._dev or plane.numel() == 0:
            raise ValueError("hdr: a float32 CUDA tensor on the converter's device expected")
        plane = plane.contiguous()
        out = torch.empty(tuple(plane.shape), dtype=torch.uint16, device=self._dev)
        _lib.check(self._lib.fw_hdr_transfer_f32(_lib.ptr(plane), plane.numel(), C.byref(self._params[1]), _lib.ptr(out), _lib.stream_ptr(self._dev)))
        return out

    # ---- the reference's directory driver ------------------------------------------------------------------------------------------
    def convert_directory(self, input_dir, output_dir, progress_callback: Optional[Callable[[float], None]] = None,
                          read: Optional[Callable] = None, write: Optional[Callable] = None) -> HDRConversionResult:
        """`HDRConverter.convert_directory`: every `*.png` of ``input_dir`` (else every `*.jpg`), sorted, is read, converted and
        written as `<stem>.png` into ``output_dir``; a frame that cannot be read counts as failed, one whose conversion or writing
        raises is copied as it is and counts as failed and processed.  ``read(path) -> array or None`` and ``write(path, array)``
        replace cv2's imread (IMREAD_UNCHANGED) and imwrite."""
        result = HDRConversionResult(output_dir=output_dir)
        input_dir, output_dir = Path(input_dir), Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        read, write = read or _read_image, write or _write_image
        frames = sorted(input_dir.glob("*.png"))
        if not frames:
            frames = sorted(input_dir.glob("*.jpg"))
        if not frames:
            logger.warning("No frames found in input directory")
            return result
        logger.info(f"Converting {len(frames)} frames to HDR")
        for i, frame_path in enumerate(frames):
            try:
                frame = read(frame_path)
                if frame is None:
                    logger.warning(f"Failed to read frame: {frame_path}")
                    result.failed_frames += 1
                    continue
                write(output_dir / frame_path.with_suffix(".png").name, self.convert_numpy(frame))
                result.frames_converted += 1
                result.frames_processed += 1
            except Exception as e:  # noqa: BLE001 - the reference copies the frame and goes on
                logger.debug(f"Failed to convert {frame_path.name}: {e}")
                shutil.copy(frame_path, output_dir / frame_path.name)
                result.failed_frames += 1
                result.frames_processed += 1
            if progress_callback:
                progress_callback((i + 1) / len(frames))
        logger.info(f"HDR conversion complete: {result.frames_converted} frames")
        return result


def create_hdr_converter(target_format: str = "hdr10", peak_brightness: int = 1000, tone_mapping: str = "aces",
                         enable_local_contrast: bool = True) -> DeviceHDRConverter:
    config = HDRConfig(target_format=HDRFormat(target_format.lower()), peak_brightness=peak_brightness,
                       tone_mapping=ToneMapping(tone_mapping.lower()), enable_local_contrast=enable_local_contrast)
    return DeviceHDRConverter(config)
