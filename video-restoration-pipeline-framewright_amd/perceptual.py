"""Perceptual tuning of final frames on the device (kernel set K24, csrc/perceptual.hip).

The reference's `processors/perceptual_tuning.py` (`PerceptualTuner`) is the user-facing look control, `--perceptual faithful |
balanced | enhanced | 0.0-1.0`: a profile of five strengths - fixed for FAITHFUL and ENHANCED, a Python-double lerp between them for
BALANCED, then the two limits and the grain floor - decides which of five cv2 steps run on a frame and with what constants:
non-local-means denoise, a sigma-3 unsharp mask, a saturation boost in HSV, CLAHE on the Lab L, and the original frame's grain added
back.  `DevicePerceptualTuner` runs `get_profile`, `adjust_settings` and `apply_to_frame` on uint8 BGR frames that are already on the
GPU, behind the temporal-consistency pass and in front of the colour grade; tests/perceptual_ref.py is the contract, byte for byte.

Every threshold of the reference is a strict `>` on a Python double, so the profile is formed here with the same double operations
in the same order; the kernels get the constants already rounded to what cv2 and numpy make of them (float32 weights, an int h, an
int CLAHE limit).  uint16 frames are refused: the reference's cv2 calls are 8-bit only.  The reference's restorer never calls its
tuner; what binds to this stage is `apply_device`.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, check_no_overlap, fetch, upload
from .qp_artifacts import MAX_SIDE, _read_image, _write_image

logger = logging.getLogger(__name__)
f32 = np.float32

FIELDS = ("sharpening", "denoise", "color_enhancement", "detail_recovery", "grain_preservation")
MIN_SIDE, DETAIL_MIN_SIDE = 3, 8


def _unit(v: float) -> float:
    return max(0.0, min(1.0, v))


class PerceptualMode(Enum):
    FAITHFUL = "faithful"
    BALANCED = "balanced"
    ENHANCED = "enhanced"


@dataclass
class PerceptualConfig:
    """The reference's fields and defaults; ``balance`` and the two limits are clamped to [0, 1]."""
    mode: PerceptualMode = PerceptualMode.BALANCED
    balance: float = 0.5
    preserve_grain: bool = True
    preserve_color_cast: bool = False
    sharpening_limit: float = 0.4
    denoise_limit: float = 0.6

    def __post_init__(self) -> None:
        self.balance, self.sharpening_limit, self.denoise_limit = _unit(self.balance), _unit(self.sharpening_limit), _unit(self.denoise_limit)


@dataclass
class PerceptualProfile:
    sharpening: float = 0.0
    denoise: float = 0.0
    color_enhancement: float = 0.0
    detail_recovery: float = 0.0
    grain_preservation: float = 1.0

    def __post_init__(self) -> None:
        for name in FIELDS:
            setattr(self, name, _unit(getattr(self, name)))

    def to_dict(self) -> Dict[str, float]:
        return {name: getattr(self, name) for name in FIELDS}


_FAITHFUL = (0.1, 0.1, 0.0, 0.2, 1.0)         # in the order of FIELDS
_ENHANCED = (0.6, 0.7, 0.5, 0.8, 0.2)


class _Params(C.Structure):
    """`fw_ptune_params` of include/framewright_hip.h"""
    _fields_ = [("denoise_h", C.c_int32), ("sharpen", C.c_int32), ("colour", C.c_int32), ("detail", C.c_int32), ("grain", C.c_int32),
                ("clahe_limit", C.c_int32), ("w_src", C.c_float), ("w_blur", C.c_float), ("boost", C.c_float), ("hue_scale", C.c_float),
                ("grain_amount", C.c_float), ("hsv_div", C.c_void_p)]


@dataclass
class PerceptualPlan:
    """The steps that run on a frame, in order, and their constants as the kernels take them: ``h`` of the non-local means (0:
    off), the two addWeighted weights, the saturation boost and the grain amount as float32 values, the CLAHE clip limit as the
    Python double (`clahe_limit` makes the integer of a frame size)."""
    steps: tuple = ()
    h: int = 0
    w_src: float = 0.0
    w_blur: float = 0.0
    boost: float = 0.0
    clip_limit: float = 0.0
    grain_amount: float = 0.0

    def to_dict(self) -> dict:
        return {"steps": list(self.steps), "h": self.h, "w_src": self.w_src, "w_blur": self.w_blur, "boost": self.boost,
                "clip_limit": self.clip_limit, "grain_amount": self.grain_amount}


def compute_profile(config: PerceptualConfig) -> PerceptualProfile:
    """`PerceptualTuner.get_profile`: a + (b - a) * balance in Python doubles, then the limits and the grain floor."""
    if config.mode == PerceptualMode.FAITHFUL:
        p = PerceptualProfile(*_FAITHFUL)
    elif config.mode == PerceptualMode.ENHANCED:
        p = PerceptualProfile(*_ENHANCED)
    else:
        p = PerceptualProfile(*(a + (b - a) * config.balance for a, b in zip(_FAITHFUL, _ENHANCED)))
    if p.sharpening > config.sharpening_limit:
        p.sharpening = config.sharpening_limit
    if p.denoise > config.denoise_limit:
        p.denoise = config.denoise_limit
    if config.preserve_grain:
        p.grain_preservation = max(p.grain_preservation, 0.7)
    return p


def compute_plan(config: PerceptualConfig, p: PerceptualProfile) -> PerceptualPlan:
    """The conditions and constants of `apply_to_frame`, every one in the reference's double arithmetic before it is rounded."""
    steps, out = [], PerceptualPlan()
    if p.denoise > 0.1 and p.grain_preservation < 0.9:
        h = int(p.denoise * (1 - p.grain_preservation) * 10)
        if h > 0:
            steps.append("denoise")
            out.h = h
    if p.sharpening > 0.1:
        amount = p.sharpening * 1.5
        steps.append("sharpen")
        out.w_src, out.w_blur = float(f32(1 + amount)), float(f32(-amount))
    if p.color_enhancement > 0.1:
        steps.append("colour")
        out.boost = float(f32(1 + p.color_enhancement * 0.3))
    if p.detail_recovery > 0.2:
        steps.append("detail")
        out.clip_limit = 1.0 + p.detail_recovery * 2.0
    if config.preserve_grain and p.grain_preservation > 0.3:
        steps.append("grain")
        out.grain_amount = float(f32(p.grain_preservation * 0.5))
    out.steps = tuple(steps)
    return out


def adjust_settings(config: PerceptualConfig, p: PerceptualProfile, base_settings: Dict[str, Any], content_type: str = "general") -> Dict[str, Any]:
    """`PerceptualTuner.adjust_settings`: the four strengths scaled by 0.5 + the profile's value where the caller gave one, else
    the profile's; the profile's grain preservation; the overrides of the content type ("film", "animation", "documentary",
    "lowlight", "faces"; any other: none), each from the values in front of the overrides; the colour-cast cap."""
    s = dict(base_settings)
    for name in FIELDS[:4]:
        s[name] = s[name] * (0.5 + getattr(p, name)) if name in s else getattr(p, name)
    s["grain_preservation"] = p.grain_preservation
    grain, denoise, sharp = s["grain_preservation"], s["denoise"], s["sharpening"]
    colour, detail = s["color_enhancement"], s["detail_recovery"]
    overrides = {"film": {"grain_preservation": min(grain + 0.2, 1.0), "denoise": max(denoise - 0.1, 0)},
                 "animation": {"grain_preservation": 0.0, "sharpening": min(sharp + 0.1, 1.0), "denoise": min(denoise + 0.2, 1.0)},
                 "documentary": {"grain_preservation": min(grain + 0.1, 1.0), "color_enhancement": max(colour - 0.1, 0)},
                 "lowlight": {"denoise": min(denoise + 0.2, 1.0), "detail_recovery": min(detail + 0.2, 1.0)},
                 "faces": {"denoise": min(denoise + 0.1, 1.0), "detail_recovery": min(detail + 0.15, 1.0),
                           "sharpening": max(sharp - 0.05, 0)}}
    s.update(overrides.get(content_type, {}))
    if config.preserve_color_cast:
        s["preserve_color_cast"] = True
        s["color_enhancement"] = min(s.get("color_enhancement", 0), 0.2)
    return s


def clahe_limit(clip_limit: float, h: int, w: int) -> int:
    """cv2's integer clip limit of one of the 8 x 8 tiles of an h x w plane (padded to multiples of 8 where either side is none)."""
    hp, wp = (h, w) if h % 8 == 0 and w % 8 == 0 else (h + 8 - h % 8, w + 8 - w % 8)
    return max(int(clip_limit * ((hp // 8) * (wp // 8)) / 256), 1)


def hsv_div_table() -> np.ndarray:
    """int32 [512]: round((255 << 12) / i), then round((180 << 12) / (6 i)); entry 0 of each half is 0 (fw_hdr_saturation_u8's)."""
    div = np.zeros(512, np.int32)
    i = np.arange(1, 256, dtype=np.float64)
    div[1:256] = np.rint((255 << 12) / i)
    div[257:] = np.rint((180 << 12) / (6.0 * i))
    return div


class DevicePerceptualTuner(Stage):
    """The reference's `PerceptualTuner` on uint8 BGR CUDA frames H x W x 3 of one GPU; the results are new tensors and the inputs
    are left as they are.  Work is queued on torch's current stream of the stage's device; the host never waits."""

    def __init__(self, config: Optional[PerceptualConfig] = None, gpu_id: int = 0):
        self.config = config or PerceptualConfig()
        self.gpu_id = int(gpu_id)
        super().__init__(self.gpu_id, needs_gpu=False)
        self._div = None
        self._closed = False
        self._wrong = "perceptual: uint8 CUDA tensors H x W x 3 (BGR) expected"
        logger.info(f"DevicePerceptualTuner: mode={self.config.mode.value}, balance={self.config.balance}")

    def close(self) -> None:
        """Releases the scratch and the table; frame calls that arrive afterwards raise."""
        self._closed = True
        self._scratch = self._div = None

    # ---- host logic ------------------------------------------------------------------------------------------------------------
    def get_profile(self) -> PerceptualProfile:
        """The profile of ``config`` as it is now: formed on every call (five double operations), so a caller that changes
        ``tuner.config`` between frames gets the new profile, as with the reference's fresh tuner."""
        return compute_profile(self.config)

    def plan(self) -> PerceptualPlan:
        return compute_plan(self.config, self.get_profile())

    def adjust_settings(self, base_settings: Dict[str, Any], content_type: str = "general") -> Dict[str, Any]:
        """`PerceptualTuner.adjust_settings` under this tuner's profile (pure host logic: `adjust_settings`)."""
        return adjust_settings(self.config, self.get_profile(), base_settings, content_type)

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def _check(self, frames, detail: bool = False) -> tuple:
        import torch
        if self._closed:
            raise ValueError("perceptual: the tuner is closed")
        dev = self.gpu_device()
        for f in frames:
            if isinstance(f, torch.Tensor) and f.dtype in tuple(getattr(torch, n) for n in ("uint16", "int16") if hasattr(torch, n)):
                raise ValueError("perceptual: uint8 frames expected (the reference's cv2 calls are 8-bit only; 16-bit frames are not built)")
            if isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.dim() == 2:
                raise ValueError("perceptual: BGR frames H x W x 3 expected, not gray planes")
        small = "perceptual: frames of 3 .. 16384 pixels a side expected (the 5 x 5 blur reflects two pixels)"
        bounds = [(MIN_SIDE, MAX_SIDE, MIN_SIDE, MAX_SIDE, small)]
        if detail:
            bounds.append((DETAIL_MIN_SIDE, MAX_SIDE, DETAIL_MIN_SIDE, MAX_SIDE,
                           "perceptual: frames of 8 .. 16384 pixels a side expected with detail recovery (8 x 8 CLAHE tiles)"))
        h, w, _ = check_frame_list(frames, self._wrong, bounds, dev=dev,
                                   wrong_device=f"perceptual: frames on cuda:{self.gpu_id}, the tuner's device, expected")
        return h, w, dev

    def _scratch_for(self, h: int, w: int, dev, params: Optional[_Params] = None):
        """What the call needs and no more: 80 KiB for the CLAHE and detail entries (``params`` None) and for a plan with detail
        alone; one frame more behind sharpen or colour; two frames and the non-local means' planes only where the denoise runs."""
        need = int(self._lib.fw_ptune_scratch_bytes(h, w, C.cast(C.pointer(params), C.c_void_p) if params is not None else None))
        return self.scratch(need, dev) if need else None

    def _table(self, dev):
        if self._div is None or self._div.device != dev:
            self._div = upload(hsv_div_table(), dev)
        return self._div

    # ---- the steps alone -------------------------------------------------------------------------------------------------------
    @_lib.on_tensor_device
    def unsharp_device(self, frame, w_src: float, w_blur: float):
        """addWeighted(x, w_src, GaussianBlur(x, (0, 0), 3), w_blur, 0); the weights are rounded to float32."""
        import torch
        h, w, dev = self._check([frame])
        frame = frame.contiguous()
        out = torch.empty_like(frame)
        _lib.check(self._lib.fw_ptune_unsharp_u8(_lib.ptr(frame), _lib.ptr(out), h, w, float(f32(w_src)), float(f32(w_blur)), _lib.stream_ptr(dev)))
        return out

    @_lib.on_tensor_device
    def saturation_device(self, frame, boost: float):
        """The colour step: fw_hdr_saturation_u8 with the boost rounded to float32."""
        import torch
        h, w, dev = self._check([frame])
        frame = frame.contiguous()
        out = torch.empty_like(frame)
        _lib.check(self._lib.fw_hdr_saturation_u8(_lib.ptr(frame), h * w, _lib.ptr(self._table(dev)), float(f32(boost)), float(f32(6 / 180)),
                                                  _lib.ptr(out), _lib.stream_ptr(dev)))
        return out

    @_lib.on_tensor_device
    def clahe_device(self, plane, clip_limit: float):
        """cv2.createCLAHE(clip_limit, (8, 8)).apply on a uint8 H x W CUDA plane."""
        import torch
        if not isinstance(plane, torch.Tensor) or plane.dtype != torch.uint8 or not plane.is_cuda or plane.dim() != 2 or plane.device != self.gpu_device():
            raise ValueError("perceptual: a uint8 CUDA plane H x W on the tuner's device expected")
        h, w, dev = int(plane.shape[0]), int(plane.shape[1]), plane.device
        if not (DETAIL_MIN_SIDE <= h <= MAX_SIDE and DETAIL_MIN_SIDE <= w <= MAX_SIDE):
            raise ValueError("perceptual: planes of 8 .. 16384 pixels a side expected (8 x 8 CLAHE tiles)")
        plane = plane.contiguous()
        out = torch.empty_like(plane)
        _lib.check(self._lib.fw_ptune_clahe_u8(_lib.ptr(plane), _lib.ptr(out), h, w, clahe_limit(clip_limit, h, w),
                                               _lib.ptr(self._scratch_for(h, w, dev)), _lib.stream_ptr(dev)))
        return out

    @_lib.on_tensor_device
    def detail_device(self, frame, clip_limit: float):
        """BGR -> Lab, L replaced by its CLAHE, Lab -> BGR."""
        import torch
        h, w, dev = self._check([frame], detail=True)
        frame = frame.contiguous()
        out = torch.empty_like(frame)
        _lib.check(self._lib.fw_ptune_detail_u8(_lib.ptr(frame), _lib.ptr(out), h, w, clahe_limit(clip_limit, h, w),
                                                _lib.ptr(self._scratch_for(h, w, dev)), _lib.stream_ptr(dev)))
        return out

    @_lib.on_tensor_device
    def grain_device(self, result, original, amount: float):
        """addWeighted(result, 1.0, grain of ``original`` on all three channels, amount, 0)."""
        import torch
        h, w, dev = self._check([result, original])
        result, original = result.contiguous(), original.contiguous()
        out = torch.empty_like(result)
        _lib.check(self._lib.fw_ptune_grain_u8(_lib.ptr(result), _lib.ptr(original), _lib.ptr(out), h, w, float(f32(amount)), _lib.stream_ptr(dev)))
        return out

    def gauss19_table(self) -> np.ndarray:
        """The 19 integer taps the unsharp kernel is compiled with."""
        out = (C.c_int32 * 19)()
        _lib.check(self._lib.fw_ptune_gauss19_table(C.cast(out, C.c_void_p)))
        return np.array(out[:], dtype=np.int64)

    # ---- frames ----------------------------------------------------------------------------------------------------------------
    def _params(self, plan: PerceptualPlan, h: int, w: int, dev) -> _Params:
        p = _Params()
        on = set(plan.steps)
        p.denoise_h = plan.h if "denoise" in on else 0
        p.sharpen, p.colour, p.detail, p.grain = ("sharpen" in on), ("colour" in on), ("detail" in on), ("grain" in on)
        p.clahe_limit = clahe_limit(plan.clip_limit, h, w) if "detail" in on else 0
        p.w_src, p.w_blur, p.boost, p.hue_scale, p.grain_amount = plan.w_src, plan.w_blur, plan.boost, float(f32(6 / 180)), plan.grain_amount
        p.hsv_div = self._table(dev).data_ptr() if "colour" in on else None
        return p

    def _launch(self, frame, out, plan: PerceptualPlan, h: int, w: int, dev) -> None:
        params = self._params(plan, h, w, dev)
        scratch = self._scratch_for(h, w, dev, params)
        _lib.check(self._lib.fw_ptune_apply_u8(_lib.ptr(frame), _lib.ptr(out), h, w, C.cast(C.pointer(params), C.c_void_p), _lib.ptr(scratch),
                                               _lib.stream_ptr(dev)))

    @_lib.on_tensor_device
    def apply_frame_device(self, frame, out=None, plan: Optional[PerceptualPlan] = None):
        """`apply_to_frame` on one uint8 H x W x 3 BGR CUDA tensor -> a new tensor (``out`` where given; it must not overlap the
        frame).  With no step on the result is a copy.  ``plan`` replaces the configuration's own (a measurement without the
        denoise, say)."""
        import torch
        plan = self.plan() if plan is None else plan
        h, w, dev = self._check([frame], detail="detail" in plan.steps)
        if frame.dim() != 3:
            raise ValueError(self._wrong)
        frame = frame.contiguous()
        if out is None:
            out = torch.empty_like(frame)
        else:
            self._check([frame, out])
            if not out.is_contiguous():
                raise ValueError("perceptual: a contiguous destination expected")
            check_no_overlap([out], [frame], "perceptual")
        self._launch(frame, out, plan, h, w, dev)
        return out

    @_lib.on_tensor_device
    def apply_device(self, frames) -> list:
        """A list of uint8 H x W x 3 BGR CUDA tensors of one shape -> new tensors, one allocation a call.  A tensor that is in the
        list several times (a repeated frame) is tuned once and its result is in the output as often."""
        frames = list(frames)
        if not frames:
            return []
        plan = self.plan()
        h, w, dev = self._check(frames, detail="detail" in plan.steps)
        if frames[0].dim() != 3:
            raise ValueError(self._wrong)
        unique = {}
        for f in frames:
            unique.setdefault(id(f), f)
        srcs = [f.contiguous() for f in unique.values()]
        outs = dict(zip(unique, _lib.empty_like_many(srcs)))
        for key, f in zip(unique, srcs):
            self._launch(f, outs[key], plan, h, w, dev)
        return [outs[id(f)] for f in frames]

    def apply(self, frames) -> List[np.ndarray]:
        """Host in, host out: uint8 H x W x 3 arrays -> the tuned arrays."""
        frames = [np.ascontiguousarray(f) for f in frames]
        for a in frames:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("perceptual: uint8 arrays H x W x 3 (BGR) expected (the reference's cv2 calls are 8-bit only)")
        if not frames:
            return []
        with self.host() as dev:
            outs = self.apply_device([upload(a, dev) for a in frames])
            got = fetch(dev, *outs)
            return [got] if len(outs) == 1 else list(got)

    def apply_to_frame(self, frame: np.ndarray) -> np.ndarray:
        """The reference's method name: one host array in, one out."""
        return self.apply([frame])[0]

    def stream(self, frames: Iterable) -> Iterator:
        """Frames in order -> the tuned frames in order; nothing is held back (every step reads one frame)."""
        for f in frames:
            yield self.apply_frame_device(f)

    def apply_directory(self, src, dst, read_fn: Optional[Callable] = None, write_fn: Optional[Callable] = None) -> int:
        """Every `*.png` of ``src`` (else every `*.jpg`), in name order, through `apply_to_frame` into ``dst`` under its name; returns
        the number of frames written.  ``read_fn(path) -> array or None`` and ``write_fn(path, array)`` replace the image reader and
        writer; a file that cannot be read is skipped."""
        src, dst = Path(src), Path(dst)
        dst.mkdir(parents=True, exist_ok=True)
        files = sorted(src.glob("*.png")) or sorted(src.glob("*.jpg"))
        read_fn, write_fn = read_fn or _read_image, write_fn or _write_image
        done = 0
        with self.host() as dev:
            for path in files:
                image = read_fn(path)
                if image is None:
                    logger.warning(f"Skipping invalid frame: {path}")
                    continue
                write_fn(dst / path.name, fetch(dev, self.apply_frame_device(upload(image, dev))))
                done += 1
        return done


def create_perceptual_tuner(mode: str = "balanced", gpu_id: int = 0) -> DevicePerceptualTuner:
    """The reference's factory: the mode by name, balance 0.0 / 0.5 / 1.0 with it."""
    modes = {"faithful": (PerceptualMode.FAITHFUL, 0.0), "balanced": (PerceptualMode.BALANCED, 0.5), "enhanced": (PerceptualMode.ENHANCED, 1.0)}
    if mode.lower() not in modes:
        raise ValueError(f"Unknown mode '{mode}'. Valid modes: {', '.join(modes)}")
    m, balance = modes[mode.lower()]
    return DevicePerceptualTuner(PerceptualConfig(mode=m, balance=balance), gpu_id)


def get_perceptual_profile(balance: float) -> PerceptualProfile:
    """The BALANCED profile at ``balance`` (clamped to [0, 1]) under the default limits; no GPU is touched."""
    return compute_profile(PerceptualConfig(mode=PerceptualMode.BALANCED, balance=_unit(balance)))
