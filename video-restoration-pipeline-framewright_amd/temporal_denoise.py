"""Classical motion-compensated temporal denoise on the device — the accumulate/warp half of the reference's
`processors/temporal_denoise.py`: `OpticalFlowEstimator.warp_frame` (:440-477),
`TemporalDenoiser._denoise_with_flow` (:1521-1580) and `_denoise_simple` (:1582-1605).

The dense optical flow is cv2's (Farneback / DIS) in the reference.  By default it stays a host computation: pass an estimator
(`flow_fn(frame, center) -> FlowField`); without one the flow-compensated method raises like the reference does without
OpenCV ("OpenCV required for optical flow estimation"), and the simple weighted average needs none.

`DeviceFlowEstimator` is the reference's `OpticalFlowEstimator` (:211-477) on the device: Farneback's flow with the reference's
parameters (:294-305), the magnitude (:320) and the confidence map (:406-438), csrc/optical_flow.hip.  Given to
`DeviceTemporalAccumulator(flow_estimator=...)` it makes the flow-compensated denoise run without leaving the device: every frame of
a window is uploaded once, flows, statistics and percentiles are computed there, and the host waits once per output frame.
cv2 is not available where this is built, so parity of the flow with cv2.calcOpticalFlowFarneback is unpinned; the kernels are held
to a float64 numpy restatement of OpenCV's algorithm (tests/farneback_ref.py).

`DeviceSpatialDenoiser` is `_apply_spatial_denoise` (:1611-1634), cv2.fastNlMeansDenoisingColored(frame, None, h, h, 7, 21) with
h = int(3 + strength * 7), on the device (csrc/nlmeans.hip): the step the reference's defaults (noise_strength 0.5 > 0.3) take on
every frame, between the accumulate and the edge-preserve.  Held bit for bit to the integer restatement in tests/nlmeans_ref.py;
cv2 parity unpinned.

`DeviceTemporalDenoiser` is the reference's entry point, `TemporalDenoiser.denoise_frames` (:1302-1424), from the first frame to the
last on the device: `DeviceClipAnalyzer` is phase 1 (`analyze`, :1110-1300: scene cuts, noise level, flicker metrics and the
recommendations, all from fw_frame_stats_u8's per-frame histogram and Laplacian sums), the chain above is phase 3, and
`DeviceTemporalConsistencyFilter` is phase 4 (`TemporalConsistencyFilter`, :839-1061: fw_flow_accumulate_affine_u8,
fw_add_weighted_u8), followed by `_estimate_noise_reduction` (:1734-1788).  tests/temporal_chain_ref.py is the contract of the new
kernels and of the host arithmetic; cv2 parity unpinned.

`DeviceFlickerReducer` is phase 2, the reference's `FlickerReducer` (:480-836) on its Python path, `_apply_python_deflicker`
(:764-836): brightness normalisation in 8-bit gamma Lab (csrc/flicker.hip: fw_lab_l_sums_u8, fw_deflicker_lab_u8), held bit for bit
to tests/flicker_ref.py; cv2 parity unpinned.  It is opt-in: `DeviceTemporalDenoiser(config, device_flicker=True)` deflickers every
input frame on the device as it is uploaded.  Without the flag nothing changes: `denoise_clip(frames, deflicker_fn=...)` stays the
seam for a host function from the list of frames to the list of deflickered frames, and without either no frame is deflickered.
Not built:
  - the external ffmpeg `deflicker` filter, the reference's first choice for phase 2 (it works on swscale's YUV planes; ffmpeg
    is not available where this is built and nothing here can restate it).
  - `AutoTemporalDenoiser`: its default preset asks for DIS flow, which `DeviceFlowEstimator` refuses.
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field
from enum import Enum, auto
from pathlib import Path
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._stage import Stage, check_out, check_stack, fetch, upload


@dataclass
class FlowField:
    """Field-for-field the reference dataclass (temporal_denoise.py:190-207)."""
    flow_x: np.ndarray
    flow_y: np.ndarray
    magnitude: np.ndarray
    confidence: np.ndarray
    frame_idx_from: int = 0
    frame_idx_to: int = 1


def _default_flow_fn(frame: np.ndarray, center: np.ndarray) -> FlowField:
    try:
        import cv2  # noqa: F401
    except ImportError:
        raise RuntimeError("OpenCV required for optical flow estimation")   # temporal_denoise.py:275-276
    raise RuntimeError("pass flow_fn: the dense-flow estimator is a host computation outside the accelerated path")


class OpticalFlowMethod(Enum):
    """The reference's enum (temporal_denoise.py:94-110), value for value."""
    FARNEBACK = "farneback"
    LUCAS_KANADE = "lucas_kanade"
    DIS = "dis"
    RAFT = "raft"
    RIFE = "rife"


# cv2.calcOpticalFlowFarneback's arguments in the reference call (temporal_denoise.py:295-305)
FARNEBACK_PARAMS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.1, flags=0)


def _percentile_index(n: int, q: float):
    """np.percentile(a, q) (method "linear") of n float32 values as (lower index, upper index, weight of the upper one), in the
    operations numpy >= 2 performs for a float32 array: q / 100 and the virtual index (n - 1) q / 100 are float32 there."""
    quant = np.asanyarray(np.true_divide(q, np.float32(100)))
    virtual = np.asanyarray((n - 1) * quant)
    if virtual >= n - 1:
        return n - 1, n - 1, np.float32(0)
    lo = int(np.floor(virtual))
    return lo, lo + 1, np.float32(np.float64(virtual) - lo)


def _percentile_sorted(srt, q: float):
    """np.percentile(., q) of a sorted float32 tensor, as a one-element float32 tensor on the tensor's device (nothing is fetched):
    numpy's `_lerp` in the array's own precision - a + (b - a) t, or b - (b - a) (1 - t) where t >= 0.5."""
    lo, hi, t = _percentile_index(int(srt.numel()), q)
    a, b = srt[lo:lo + 1], srt[hi:hi + 1]
    d = b - a
    if t >= 0.5:
        return b - d * float(np.float32(1) - t)                # a Python scalar keeps the tensor's float32
    return a + d * float(t)


class DeviceFlowEstimator(Stage):
    """`OpticalFlowEstimator` (temporal_denoise.py:211-477) on one GPU: Farneback dense optical flow (fw_farneback_flow_u8), magnitude,
    local-variance confidence (fw_flow_stats_f32, fw_flow_confidence_f32).  RAFT and RIFE run Farneback, as the reference's `else`
    branch does (:311-315); DIS and LUCAS_KANADE are not built and raise NotImplementedError.

    Direction of the field `estimate(frame1, frame2)` returns.  The reference uses the pair the way its docstring shows (:219-220, and
    `_denoise_with_flow` :1553-1554): `flow = estimate(frame, center); aligned = warp_frame(frame, flow)`, and `warp_frame` samples
    `frame` at p + flow(p).  That brings `frame` onto `center` only if flow is the displacement FROM `center` TO `frame`
    (center(p) ~ frame(p + flow(p)), i.e. cv2.calcOpticalFlowFarneback(center, frame)).  The reference passes the images to cv2 the
    other way round, (frame, center), and so moves a translating neighbour away from the centre frame (to 2 d instead of 0): on a
    clip translating 2 px per frame with sigma-10 noise its flow-compensated average measures 23.98 dB against the clean centre
    frame, the plain average 28.56 dB, the noisy frame 28.05 dB.  `convention="align"` (the default) returns the field that
    `warp_frame(frame1, .)` needs - Farneback's flow with (frame2, frame1) as cv2's (prev, next) - and the same clip measures
    35.00 dB; `convention="cv2"` is the reference's call, argument for argument.  `flow_device(prev, next)` and the C-ABI are always
    cv2's convention: prev(p) ~ next(p + flow(p))."""

    def __init__(self, method: OpticalFlowMethod = OpticalFlowMethod.FARNEBACK, gpu_id: int = 0, convention: str = "align",
                 **farneback_params):
        method = OpticalFlowMethod(method)
        if convention not in ("align", "cv2"):
            raise ValueError(f"convention must be 'align' or 'cv2', got {convention!r}")
        self.convention = convention
        if method in (OpticalFlowMethod.DIS, OpticalFlowMethod.LUCAS_KANADE):
            raise NotImplementedError(f"optical flow method {method.name} ({method.value!r}) is not implemented on the device; "
                                      "FARNEBACK is (RAFT and RIFE fall back to it, as in the reference)")
        unknown = set(farneback_params) - set(FARNEBACK_PARAMS)
        if unknown:
            raise TypeError(f"unknown Farneback parameter(s): {sorted(unknown)}")
        self.method, self.gpu_id = method, int(gpu_id)
        self.params = {**FARNEBACK_PARAMS, **farneback_params}
        super().__init__(self.gpu_id)

    @staticmethod
    def _load(frame) -> np.ndarray:
        if isinstance(frame, (str, Path)):
            from PIL import Image                              # BGR, as the reference's cv2.imread (:279-287)
            frame = np.asarray(Image.open(str(frame)).convert("RGB"))[:, :, ::-1]
        frame = np.ascontiguousarray(frame)
        if frame.dtype != np.uint8 or frame.ndim not in (2, 3) or (frame.ndim == 3 and frame.shape[2] != 3):
            raise ValueError("optical flow expects uint8 BGR (H x W x 3) or gray (H x W) frames")
        return frame

    def _scratch_for(self, h: int, w: int, dev):
        return self.scratch(int(self._lib.fw_farneback_scratch_bytes(h, w, int(self.params["levels"]))), dev)

    @_lib.on_tensor_device
    def flow_device(self, t1, t2):
        """(flow_x, flow_y): fp32 H x W device tensors, cv2.calcOpticalFlowFarneback(t1, t2): t1(p) ~ t2(p + flow(p)), whatever
        `convention` is (uint8 device tensors, H x W x 3 BGR or H x W gray)."""
        import torch
        if t1.shape != t2.shape or t1.dtype != torch.uint8 or t2.dtype != torch.uint8 or t1.dim() not in (2, 3) or \
                (t1.dim() == 3 and t1.shape[2] != 3) or not t1.is_cuda or t1.device != t2.device:
            raise ValueError("optical flow expects two uint8 device frames of one size, BGR (H x W x 3) or gray (H x W)")
        t1, t2 = t1.contiguous(), t2.contiguous()
        dev = t1.device
        h, w = int(t1.shape[0]), int(t1.shape[1])
        p = self.params
        scratch = self._scratch_for(h, w, dev)
        fx = torch.empty((h, w), dtype=torch.float32, device=dev)
        fy = torch.empty((h, w), dtype=torch.float32, device=dev)
        st = _lib.stream_ptr(dev)
        _lib.check(self._lib.fw_farneback_flow_u8(_lib.ptr(t1), _lib.ptr(t2), 1 if t1.dim() == 2 else 3, h, w,
                                                  float(p["pyr_scale"]), int(p["levels"]), int(p["winsize"]), int(p["iterations"]),
                                                  int(p["poly_n"]), float(p["poly_sigma"]), int(p["flags"]),
                                                  _lib.ptr(scratch), _lib.ptr(fx), _lib.ptr(fy), st))
        return fx, fy

    @_lib.on_tensor_device
    def maps_device(self, t1, t2, weight_map: bool = False):
        """(flow_x, flow_y, magnitude, confidence[, weight_map]) as fp32 device tensors; nothing is fetched to the host.
        weight_map = confidence, halved where the magnitude exceeds its 90th percentile (`_denoise_with_flow`, :1560-1564).
        The field is the one `estimate(t1, t2)` returns: see `convention` in the class docstring."""
        import torch
        fx, fy = self.flow_device(t2, t1) if self.convention == "align" else self.flow_device(t1, t2)
        dev = fx.device
        h, w = int(fx.shape[0]), int(fx.shape[1])
        mag, var, conf = torch.empty_like(fx), torch.empty_like(fx), torch.empty_like(fx)
        wm = torch.empty_like(fx) if weight_map else None
        st, p = _lib.stream_ptr(dev), _lib.ptr
        _lib.check(self._lib.fw_flow_stats_f32(p(fx), p(fy), h, w, p(mag), p(var), st))
        # the two order statistics are plumbing: a device sort each (torch.quantile refuses inputs of this size), index arithmetic on the host
        p95 = _percentile_sorted(torch.sort(var.reshape(-1)).values, 95)
        thr = _percentile_sorted(torch.sort(mag.reshape(-1)).values, 90) if weight_map else None
        _lib.check(self._lib.fw_flow_confidence_f32(p(var), p(p95), p(mag) if weight_map else None, p(thr), h, w, p(conf), p(wm), st))
        return (fx, fy, mag, conf, wm) if weight_map else (fx, fy, mag, conf)

    def estimate_device(self, t1, t2):
        """The four maps of a `FlowField` (flow_x, flow_y, magnitude, confidence) as device tensors."""
        return self.maps_device(t1, t2)

    def estimate(self, frame1: Union[np.ndarray, str, Path], frame2: Union[np.ndarray, str, Path]) -> FlowField:
        """`OpticalFlowEstimator.estimate` (:261-332): numpy frames or image paths in, a numpy FlowField (fp32 maps) out - the field by
        which `warp_frame(frame1, .)` brings `frame1` onto `frame2` (`convention="cv2"`: the reference's cv2 call, (frame1, frame2))."""
        a, b = self._load(frame1), self._load(frame2)
        with self.host() as dev:
            fx, fy, mag, conf = fetch(dev, *self.maps_device(upload(a, dev), upload(b, dev)))
        return FlowField(flow_x=fx, flow_y=fy, magnitude=mag, confidence=conf, frame_idx_from=0, frame_idx_to=1)

    def warp_frame(self, frame: np.ndarray, flow: FlowField, inverse: bool = False) -> np.ndarray:
        """`OpticalFlowEstimator.warp_frame` (:440-477), the existing remap kernel."""
        return DeviceTemporalAccumulator(gpu_id=self.gpu_id).warp_frame(frame, flow, inverse=inverse)


class DeviceSpatialDenoiser(Stage):
    """`TemporalDenoiser._apply_spatial_denoise` (temporal_denoise.py:1611-1634) on one GPU: non-local means on the Lab planes of a
    BGR frame (fw_nlmeans_colored_u8), and the plain core on a 1-, 2- or 3-channel plane (fw_nlmeans_u8).  The windows are the
    reference's (7, 21); the kernels take a template window of 3, 5 or 7 and an odd search window of 3 .. 41, and even sizes are
    rejected where cv2 would force them odd.  tests/nlmeans_ref.py is the contract (bit-exact); cv2 parity unpinned."""

    def __init__(self, gpu_id: int = 0, template_window: int = 7, search_window: int = 21):
        self.gpu_id, self.template_window, self.search_window = int(gpu_id), int(template_window), int(search_window)
        super().__init__(self.gpu_id)

    @staticmethod
    def h_for_strength(strength: float) -> int:
        """The filter strength of the reference's call (:1627)."""
        return int(3 + strength * 7)

    def _scratch_for(self, h: int, w: int, dev):
        need = int(self._lib.fw_nlmeans_scratch_bytes(h, w, self.search_window))
        if need <= 0:
            raise ValueError(f"non-local means: bad frame size {h} x {w} or search window {self.search_window}")
        return self.scratch(need, dev)

    @_lib.on_tensor_device
    def denoise_device(self, t, h: float, h_color: Optional[float] = None):
        """cv2.fastNlMeansDenoisingColored(t, None, h, h_color, template, search) of a uint8 BGR (H x W x 3) device tensor -> a new
        device tensor; `t` is left untouched, nothing is fetched and nothing waits for the device.  h_color defaults to h, the
        reference's call."""
        import torch
        check_stack(t, 3, "the spatial denoise expects a uint8 BGR (H x W x 3) device frame", test_type=False)
        t = t.contiguous()
        dev = t.device
        hh, ww = int(t.shape[0]), int(t.shape[1])
        scratch = self._scratch_for(hh, ww, dev)
        out = torch.empty_like(t)
        st = _lib.stream_ptr(dev)
        _lib.check(self._lib.fw_nlmeans_colored_u8(_lib.ptr(t), hh, ww, float(h), float(h if h_color is None else h_color),
                                                   self.template_window, self.search_window, _lib.ptr(scratch),
                                                   _lib.ptr(out), st))
        return out

    @_lib.on_tensor_device
    def nlmeans_device(self, plane, h: float):
        """The plain core (cv2.fastNlMeansDenoising's 8-bit algorithm) on a uint8 device plane, H x W or H x W x C with C = 1, 2, 3
        interleaved channels that share one weight per offset -> a new device tensor of the same shape."""
        import torch
        if plane.dtype != torch.uint8 or plane.dim() not in (2, 3) or (plane.dim() == 3 and not 1 <= plane.shape[2] <= 3) or not plane.is_cuda:
            raise ValueError("non-local means expects a uint8 device plane, H x W or H x W x C with C = 1, 2 or 3")
        plane = plane.contiguous()
        dev = plane.device
        out = torch.empty_like(plane)
        st = _lib.stream_ptr(dev)
        _lib.check(self._lib.fw_nlmeans_u8(_lib.ptr(plane), 1 if plane.dim() == 2 else int(plane.shape[2]), int(plane.shape[0]),
                                           int(plane.shape[1]), float(h), self.template_window, self.search_window, None,
                                           _lib.ptr(out), st))
        return out

    def denoise(self, frame: np.ndarray, strength: float) -> np.ndarray:
        """`_apply_spatial_denoise(frame, strength)`: numpy uint8 BGR in and out."""
        frame = np.ascontiguousarray(frame)
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("the spatial denoise expects a uint8 BGR (H x W x 3) frame")
        with self.host() as dev:
            return fetch(dev, self.denoise_device(upload(frame, dev), self.h_for_strength(strength)))


class DeviceTemporalAccumulator(Stage):
    """The float64 accumulate of `_denoise_with_flow` / `_denoise_simple` on one GPU.

    flow_fn: a host estimator, `flow_fn(frame, center) -> FlowField` (e.g. cv2's); its maps are uploaded per neighbour.
    flow_estimator: a `DeviceFlowEstimator`; `denoise_with_flow` and `denoise_sequence` then keep frames, flows, statistics and weights
    on the device and wait for it once per output frame.  Passing both is a ValueError; with neither, the flow-compensated method
    behaves as the reference does without OpenCV."""

    def __init__(self, temporal_weight_decay: float = 0.5, gpu_id: int = 0, flow_fn: Optional[Callable] = None,
                 flow_estimator: Optional[DeviceFlowEstimator] = None):
        if flow_fn is not None and flow_estimator is not None:
            raise ValueError("pass flow_fn (a host estimator) or flow_estimator (a DeviceFlowEstimator), not both")
        super().__init__(gpu_id)
        self.decay, self.gpu_id = float(temporal_weight_decay), int(gpu_id)
        self.flow_fn = flow_fn or _default_flow_fn
        self.flow_estimator = flow_estimator
        self._spatial = None

    def warp_frame(self, frame: np.ndarray, flow: FlowField, inverse: bool = False) -> np.ndarray:
        """`OpticalFlowEstimator.warp_frame`: cv2.remap(frame, grid +/- flow, INTER_LINEAR, BORDER_REFLECT_101)."""
        import torch
        dev = self._dev
        h, w = frame.shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        self._accumulate(upload(frame, dev), flow, 1.0, None, None, inverse, acc, ws)
        return self._finish(acc, ws)

    @_lib.on_tensor_device
    def _accumulate(self, frame_dev, flow: Optional[FlowField], scale: float, wmap, thr, inverse, acc, ws) -> None:
        import torch
        dev = acc.device
        h, w = int(acc.shape[0]), int(acc.shape[1])
        st = _lib.stream_ptr(dev)
        f32 = lambda a: upload(np.asarray(a, dtype=np.float32), dev)
        keep = []
        p = _lib.ptr
        fx = fy = mg = wm = None
        if flow is not None:
            fx, fy = f32(flow.flow_x), f32(flow.flow_y)
            keep += [fx, fy]
        if wmap is not None:
            wm = f32(wmap)
            keep.append(wm)
        if thr is not None:
            mg = f32(flow.magnitude)
            keep.append(mg)
        _lib.check(self._lib.fw_flow_accumulate_u8(p(frame_dev), p(fx), p(fy), p(wm), float(scale), p(mg),
                                                   float(thr) if thr is not None else 0.0, int(bool(inverse)), h, w, p(acc), p(ws), st))
        torch.cuda.current_stream(dev).synchronize()   # the uploaded maps above are temporaries

    @_lib.on_tensor_device
    def _finish(self, acc, ws) -> np.ndarray:
        import torch
        h, w = int(acc.shape[0]), int(acc.shape[1])
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=acc.device)
        st = _lib.stream_ptr(acc.device)
        _lib.check(self._lib.fw_flow_accumulate_finish_u8(_lib.ptr(acc), _lib.ptr(ws), h, w,
                                                          _lib.ptr(out), st))
        torch.cuda.synchronize(acc.device)
        return out.cpu().numpy()

    def denoise_with_flow(self, center_local_idx: int, window: Sequence[np.ndarray]) -> np.ndarray:
        """`_denoise_with_flow` (temporal_denoise.py:1521-1580) for the frames of one window."""
        import torch
        dev = self._dev
        if self.flow_estimator is not None:
            with self.host():
                out = self._window_device(center_local_idx, [upload(f, dev) for f in window])
                torch.cuda.synchronize(dev)
            return out.cpu().numpy()
        center = window[center_local_idx]
        h, w = center.shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        for local_i, frame in enumerate(window):
            distance = abs(local_i - center_local_idx)
            fd = upload(frame, dev)
            if distance == 0:
                self._accumulate(fd, None, 1.0, None, None, False, acc, ws)
                continue
            temporal = math.exp(-distance * self.decay)       # np.exp on a Python float: the same libm value
            try:
                flow = self.flow_fn(frame, center)
                thr = np.percentile(flow.magnitude, 90)       # host: the flow and its statistics are host data
                self._accumulate(fd, flow, temporal, flow.confidence, thr, False, acc, ws)
            except Exception:                                 # "Flow failed, using unaligned" (:1565-1569)
                self._accumulate(fd, None, temporal, None, None, False, acc, ws)
        return self._finish(acc, ws)

    @_lib.on_tensor_device
    def _window_device(self, center_local_idx: int, frames_dev):
        """`_denoise_with_flow` for a window of uint8 BGR device frames -> the uint8 device result.  Only launches: flow, statistics,
        percentiles, weights and the accumulate all read device memory, and nothing here waits for the device."""
        import torch
        center = frames_dev[center_local_idx]
        dev = center.device
        h, w = int(center.shape[0]), int(center.shape[1])
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        st, p = _lib.stream_ptr(dev), _lib.ptr
        for local_i, fd in enumerate(frames_dev):
            distance = abs(local_i - center_local_idx)
            fx = fy = wm = None
            if distance:
                try:
                    fx, fy, _, _, wm = self.flow_estimator.maps_device(fd, center, weight_map=True)
                except Exception:                                 # "Flow failed, using unaligned" (:1565-1569)
                    fx = fy = wm = None
            # the halving above the magnitude's 90th percentile is already in `wm`: a factor 0.5 is exact, so magnitude = NULL here gives
            # the bytes of the host-threshold form
            _lib.check(self._lib.fw_flow_accumulate_u8(p(fd), p(fx), p(fy), p(wm), math.exp(-distance * self.decay) if distance else 1.0,
                                                       None, 0.0, 0, h, w, p(acc), p(ws), st))
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        _lib.check(self._lib.fw_flow_accumulate_finish_u8(p(acc), p(ws), h, w, p(out), st))
        return out

    SPATIAL_THRESHOLD = 0.3     # `if self.config.noise_strength > 0.3` (temporal_denoise.py:1506)

    @staticmethod
    def _check_sequence_args(n: int, temporal_radius: int, noise_strength: Optional[float], scene_changes: Sequence[int]):
        """Validation of `denoise_sequence`'s arguments (no GPU involved) -> (run the spatial step?, set of scene-cut frames)."""
        if temporal_radius < 1:
            raise ValueError(f"temporal_radius must be >= 1, got {temporal_radius}")
        if noise_strength is not None:
            if isinstance(noise_strength, bool) or not isinstance(noise_strength, (int, float, np.integer, np.floating)) or \
                    not math.isfinite(noise_strength) or noise_strength < 0:
                raise ValueError(f"noise_strength must be None or a finite number >= 0, got {noise_strength!r}")
        cuts = set()
        for c in scene_changes:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
                raise ValueError(f"scene_changes must hold frame indices (int), got {c!r}")
            if not 0 <= int(c) < n:
                raise ValueError(f"scene_changes: frame index {int(c)} outside the clip of {n} frames")
            cuts.add(int(c))
        return noise_strength is not None and noise_strength > DeviceTemporalAccumulator.SPATIAL_THRESHOLD, cuts

    def _spatial_denoiser(self) -> "DeviceSpatialDenoiser":
        if self._spatial is None:
            self._spatial = DeviceSpatialDenoiser(gpu_id=self.gpu_id)
        return self._spatial

    def denoise_sequence(self, frames: Sequence[np.ndarray], temporal_radius: int = 3, preserve_edges: bool = False,
                         edge_threshold: int = 30, noise_strength: Optional[float] = None,
                         scene_changes: Sequence[int] = ()) -> Iterator[np.ndarray]:
        """The reference's per-frame chain over a clip (temporal_denoise.py:1480-1514): frame i is denoised from the window
        [i - radius, i + radius] clipped to the clip - a frame listed in `scene_changes` from a window of itself alone (:1483-1489) -
        one result per input frame, in order.  With `noise_strength` given and > 0.3 the spatial denoise (:1506-1507,
        `DeviceSpatialDenoiser`, h = int(3 + 7 noise_strength)) follows the accumulate; `preserve_edges` chains `_preserve_edges`
        (:1636-1667, fw_preserve_edges_u8) behind it, the reference's order.  With a `flow_estimator` the clip is uploaded once, every
        step stays on the device and each output frame costs one wait and one download.  Detecting the scene cuts and flicker
        reduction are not part of it."""
        import torch
        frames = list(frames)
        n = len(frames)
        spatial, cuts = self._check_sequence_args(n, temporal_radius, noise_strength, scene_changes)
        dev = self._dev
        if self.flow_estimator is None:
            for i in range(n):
                lo, hi = (i, i + 1) if i in cuts else (max(0, i - temporal_radius), min(n, i + temporal_radius + 1))
                out = self.denoise_with_flow(i - lo, frames[lo:hi])
                if spatial:
                    out = self._spatial_denoiser().denoise(out, noise_strength)
                yield self.preserve_edges(frames[i], out, edge_threshold) if preserve_edges else out
            return
        with self.host():
            devs = [upload(f, dev) for f in frames]
        for i in range(n):
            lo, hi = (i, i + 1) if i in cuts else (max(0, i - temporal_radius), min(n, i + temporal_radius + 1))
            with self.host():
                out = self._chain_device(i - lo, devs[lo:hi], noise_strength if spatial else None, preserve_edges, edge_threshold)
                torch.cuda.synchronize(dev)
                res = out.cpu().numpy()
            yield res

    @_lib.on_tensor_device
    def _chain_device(self, center_local_idx: int, window_dev, spatial_strength: Optional[float], preserve_edges: bool,
                      edge_threshold: int, simple: bool = False):
        """One frame of the reference's chain (:1499-1511) on a window of uint8 BGR device frames -> the uint8 device result:
        accumulate (`_denoise_simple`'s weights with `simple`), the spatial denoise when `spatial_strength` is given, the edge
        preserve against the window's centre frame.  Only launches, apart from the edge mask's hysteresis (fw_preserve_edges_u8)."""
        center = window_dev[center_local_idx]
        out = self._window_simple_device(window_dev) if simple else self._window_device(center_local_idx, window_dev)
        if spatial_strength is not None:
            out = self._spatial_denoiser().denoise_device(out, DeviceSpatialDenoiser.h_for_strength(spatial_strength))
        return self._preserve_edges_device(center, out, edge_threshold) if preserve_edges else out

    def _preserve_edges_device(self, original, denoised, edge_threshold: int):
        """`_preserve_edges` on two uint8 BGR device frames of one size -> a new device frame; the device is current."""
        import torch
        h, w = int(denoised.shape[0]), int(denoised.shape[1])
        scratch = torch.empty(int(self._lib.fw_preserve_edges_scratch_bytes(h, w)), dtype=torch.uint8, device=denoised.device)
        out = torch.empty_like(denoised)
        _lib.check(self._lib.fw_preserve_edges_u8(_lib.ptr(original), _lib.ptr(denoised), h, w, float(edge_threshold),
                                                  float(edge_threshold * 3), _lib.ptr(scratch), _lib.ptr(out),
                                                  _lib.stream_ptr(denoised.device)))
        return out

    @_lib.on_tensor_device
    def _window_simple_device(self, frames_dev):
        """`_denoise_simple` (:1582-1605) for a window of uint8 BGR device frames: scalar weights exp(-|i - len // 2| decay), the
        reference's centre (the middle of the WINDOW, also where the clip's edge has clipped it)."""
        import torch
        dev = frames_dev[0].device
        h, w = int(frames_dev[0].shape[0]), int(frames_dev[0].shape[1])
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        st = _lib.stream_ptr(dev)
        center_idx = len(frames_dev) // 2
        for i, fd in enumerate(frames_dev):
            _lib.check(self._lib.fw_flow_accumulate_u8(_lib.ptr(fd), None, None, None, math.exp(-abs(i - center_idx) * self.decay),
                                                       None, 0.0, 0, h, w, _lib.ptr(acc), _lib.ptr(ws), st))
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        _lib.check(self._lib.fw_flow_accumulate_finish_u8(_lib.ptr(acc), _lib.ptr(ws), h, w,
                                                          _lib.ptr(out), st))
        return out

    def preserve_edges(self, original: np.ndarray, denoised: np.ndarray, edge_threshold: int = 30) -> np.ndarray:
        """`TemporalDenoiser._preserve_edges` (temporal_denoise.py:1636-1667): the original frame shows through a blurred,
        dilated Canny edge mask (thresholds ``edge_threshold`` and three times that, config default 30, :146).  uint8 BGR frames
        in and out; fw_preserve_edges_u8."""
        import torch
        if original.shape != denoised.shape or original.dtype != np.uint8 or denoised.dtype != np.uint8 or original.ndim != 3 or \
                original.shape[2] != 3:
            raise ValueError("preserve_edges expects two uint8 BGR frames of one size")
        with self.host() as dev:
            out = self._preserve_edges_device(upload(original, dev), upload(denoised, dev), edge_threshold)
            torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    def denoise_simple(self, window: Sequence[np.ndarray]) -> np.ndarray:
        """`_denoise_simple` (temporal_denoise.py:1582-1605).  The reference divides by a scalar weight sum; per-pixel sums
        of the same scalars give the same float64 quotient."""
        import torch
        dev = self._dev
        h, w = window[0].shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        center_idx = len(window) // 2
        for i, frame in enumerate(window):
            self._accumulate(upload(frame, dev), None, math.exp(-abs(i - center_idx) * self.decay), None, None, False, acc, ws)
        return self._finish(acc, ws)


# ---- the reference's entry point: analysis, the chain above, the temporal-consistency pass ------------------------------------------

class DenoiseMethod(Enum):
    """The reference's enum (temporal_denoise.py:59-75), value for value."""
    MULTI_FRAME_AVERAGE = auto()
    OPTICAL_FLOW_WARP = auto()
    NON_LOCAL_MEANS_TEMPORAL = auto()
    BILATERAL_TEMPORAL = auto()
    VBM4D = auto()


class FlickerMode(Enum):
    """The reference's enum (temporal_denoise.py:78-91), value for value."""
    LIGHT = "light"
    MEDIUM = "medium"
    AGGRESSIVE = "aggressive"
    ADAPTIVE = "adaptive"


@dataclass
class TemporalDenoiseConfig:
    """Field for field the reference dataclass and its validation (temporal_denoise.py:113-163)."""
    temporal_radius: int = 3
    noise_strength: float = 0.5
    method: DenoiseMethod = DenoiseMethod.OPTICAL_FLOW_WARP
    enable_optical_flow: bool = True
    optical_flow_method: OpticalFlowMethod = OpticalFlowMethod.FARNEBACK
    enable_flicker_reduction: bool = True
    flicker_mode: FlickerMode = FlickerMode.ADAPTIVE
    preserve_edges: bool = True
    edge_threshold: int = 30
    temporal_weight_decay: float = 0.5
    scene_change_threshold: float = 0.7
    gpu_id: int = 0
    chunk_size: int = 50

    def __post_init__(self) -> None:
        if self.temporal_radius < 1:
            raise ValueError(f"temporal_radius must be >= 1, got {self.temporal_radius}")
        if not 0.0 <= self.noise_strength <= 1.0:
            raise ValueError(f"noise_strength must be 0-1, got {self.noise_strength}")
        if not 0.0 <= self.temporal_weight_decay <= 1.0:
            raise ValueError(f"temporal_weight_decay must be 0-1, got {self.temporal_weight_decay}")
        if not 0.0 <= self.scene_change_threshold <= 1.0:
            raise ValueError(f"scene_change_threshold must be 0-1, got {self.scene_change_threshold}")
        if self.chunk_size < 10:
            raise ValueError(f"chunk_size must be >= 10, got {self.chunk_size}")


@dataclass
class TemporalDenoiseResult:
    """Field for field the reference dataclass (temporal_denoise.py:166-187)."""
    frames_processed: int = 0
    frames_failed: int = 0
    output_dir: Optional[Path] = None
    scene_changes_detected: List[int] = field(default_factory=list)
    avg_noise_reduction: float = 0.0
    flicker_reduction_applied: bool = False
    processing_time_seconds: float = 0.0
    peak_memory_mb: int = 0


# Pure host functions: from the per-frame (histogram, sum lap, sum lap^2) of fw_frame_stats_u8 to every number `analyze` reports.

def brightness_from_hist(hist) -> float:
    """np.mean(gray) (:564) from gray's histogram: sum v hist[v] / N.  Both integers are below 2^53, so the quotient is the one
    numpy forms from its exact float64 sum."""
    h = [int(c) for c in hist]
    return sum(v * c for v, c in enumerate(h)) / sum(h)


def laplacian_variance(n_pixels: int, sum_lap: int, sum_lap_sq: int) -> float:
    """cv2.Laplacian(gray, CV_64F).var() (:1236-1237) from the exact sums: (N S2 - S1^2) / N^2 in integers, rounded once."""
    n, s1, s2 = int(n_pixels), int(sum_lap), int(sum_lap_sq)
    return (n * s2 - s1 * s1) / (n * n)


def hist_correlation(hist1, hist2) -> float:
    """cv2.compareHist(h1, h2, HISTCMP_CORREL) of two float32 histograms: the five sums run in double in bin order, then
    (s12 - s1 s2 / n) / sqrt((s11 - s1^2 / n) (s22 - s2^2 / n)), 1.0 where the denominator's square is within DBL_EPSILON of 0."""
    a, b = np.asarray(hist1, np.float32).reshape(-1).tolist(), np.asarray(hist2, np.float32).reshape(-1).tolist()
    s1 = s2 = s11 = s12 = s22 = 0.0
    for x, y in zip(a, b):
        s12 += x * y
        s1 += x
        s11 += x * x
        s2 += y
        s22 += y * y
    scale = 1.0 / len(a)
    num = s12 - s1 * s2 * scale
    denom2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale)
    return num / math.sqrt(denom2) if abs(denom2) > 2.220446049250313e-16 else 1.0


def scene_changes_from_hists(hists, sample_rate: int, threshold: float) -> List[int]:
    """`_detect_scene_changes` (:1158-1207) to the letter, from the gray histograms of the frames (hists[i] is read only for the
    frames the loop visits; the others may be None): the pairs are (i, min(i + sample_rate, n - 1)), the histograms float32 and
    normalised by sum + 1e-6 (in float32, as cv2.calcHist's output is), and the index recorded is i + sample_rate - which the last
    pair can put at or beyond n."""
    n = len(hists)
    if n < 2:
        return []
    if sample_rate < 1:
        raise ValueError(f"sample_rate must be >= 1, got {sample_rate}")

    def norm(h):
        h = np.asarray(h).astype(np.float32)
        return h / (h.sum() + 1e-6)

    out = []
    for i in range(0, n - 1, sample_rate):
        if hist_correlation(norm(hists[i]), norm(hists[min(i + sample_rate, n - 1)])) < threshold:
            out.append(i + sample_rate)
    return out


def noise_level_from_variances(variances: Sequence[float], sample_rate: int) -> float:
    """`_estimate_noise_level` (:1230-1252) from the Laplacian variance of every frame: every `sample_rate`-th, the first 50 of
    those, the median, / 5000, clipped to [0, 1]."""
    picked = list(variances)[::sample_rate][:50]
    if not picked:
        return 0.0
    return float(np.clip(np.median(picked) / 5000, 0, 1))


def flicker_metrics_from_brightness(brightness: Sequence[float], sample_rate: int = 1, max_samples: int = 200) -> Dict[str, Any]:
    """`FlickerReducer.analyze_flicker` (:538-625) from the mean gray level of every frame of the clip."""
    quiet = {"severity": 0.0, "temporal_variance": 0.0, "frequency": 0.0, "recommended_mode": FlickerMode.LIGHT.value}
    values = list(brightness)
    if len(values) < 3:
        return quiet
    values = values[::sample_rate][:max_samples]
    if len(values) < 3:
        return quiet
    b = np.array(values)
    temporal_variance = np.std(b) / (np.mean(b) + 1e-6)
    diffs = np.abs(np.diff(b))
    mean_diff, max_diff = np.mean(diffs), np.max(diffs)
    fft = np.fft.fft(b - np.mean(b))
    power = np.abs(fft[:len(fft) // 2]) ** 2
    if len(power) > 1:
        dominant_freq_idx = np.argmax(power[1:]) + 1
        dominant_power = power[dominant_freq_idx] / (np.sum(power) + 1e-6)
    else:
        dominant_freq_idx, dominant_power = 0, 0.0
    severity = min(1.0, (temporal_variance * 2 + (mean_diff / 255) * 3 + dominant_power * 0.5))
    recommended = FlickerMode.LIGHT if severity < 0.1 else FlickerMode.MEDIUM if severity < 0.3 else FlickerMode.AGGRESSIVE
    return {"severity": float(severity), "temporal_variance": float(temporal_variance), "frequency": float(dominant_freq_idx),
            "mean_brightness_diff": float(mean_diff), "max_brightness_diff": float(max_diff), "recommended_mode": recommended.value}


def generate_recommendations(analysis: Dict[str, Any], config: TemporalDenoiseConfig) -> Dict[str, Any]:
    """`_generate_recommendations` (:1254-1300)."""
    rec = {"temporal_radius": config.temporal_radius, "noise_strength": config.noise_strength,
           "enable_flicker_reduction": config.enable_flicker_reduction, "flicker_mode": config.flicker_mode.value}
    noise_level = analysis.get("noise_level", 0.0)
    flicker_severity = analysis.get("flicker_metrics", {}).get("severity", 0.0)
    rec["noise_strength"] = 0.3 if noise_level < 0.2 else 0.5 if noise_level < 0.5 else 0.7
    if len(analysis.get("scene_changes", [])) > 10:
        rec["temporal_radius"] = 2
    elif noise_level > 0.5:
        rec["temporal_radius"] = 4
    if flicker_severity > 0.3:
        rec["enable_flicker_reduction"] = True
        rec["flicker_mode"] = analysis.get("flicker_metrics", {}).get("recommended_mode", "medium")
    return rec


def noise_reduction_from_variances(input_variances: Sequence[float], output_variances: Sequence[float]) -> float:
    """The tail of `_estimate_noise_reduction` (:1777-1788): 1 - mean(out) / mean(in), clipped to [0, 1]; 0 without frames or
    where the input has no Laplacian energy."""
    if not len(input_variances) or not len(output_variances):
        return 0.0
    avg_input, avg_output = np.mean(input_variances), np.mean(output_variances)
    if avg_input <= 0:
        return 0.0
    return float(np.clip(1 - (avg_output / avg_input), 0, 1))


def _check_clip(frames) -> List[np.ndarray]:
    """A clip as a list of contiguous uint8 BGR frames of one size (no GPU involved)."""
    frames = [np.ascontiguousarray(f) for f in frames]
    for f in frames:
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape != frames[0].shape:
            raise ValueError("a clip is a sequence of uint8 BGR (H x W x 3) frames of one size")
    return frames


class DeviceClipAnalyzer(Stage):
    """Phase 1 of the reference, `TemporalDenoiser.analyze` (temporal_denoise.py:1110-1300), with the per-frame work on one GPU:
    fw_frame_stats_u8 reads a resident batch of frames once and leaves 256 histogram bins and two integer sums per frame; the
    pure host functions above turn those into the reference's `analysis` dict.  Only the frames the reference samples are uploaded
    (every `sample_rate`-th and the last), at most `config.chunk_size` at a time.

    Gray is always cv2.cvtColor(BGR2GRAY)'s 14-bit form.  The reference's noise estimate reads its frames with IMREAD_GRAYSCALE,
    where the image decoder does the conversion: those need not be the same bytes, so `noise_level` is the reference's only up to
    that difference."""

    def __init__(self, config: Optional[TemporalDenoiseConfig] = None):
        self.config = config or TemporalDenoiseConfig()
        self.gpu_id = int(self.config.gpu_id)
        super().__init__(self.gpu_id)

    @_lib.on_tensor_device
    def stats_device(self, clip_u8) -> Tuple[np.ndarray, np.ndarray]:
        """(hist [count][256] uint32, sums [count][2] int64 = sum lap, sum lap^2) of a uint8 count x H x W x 3 BGR device tensor: one
        launch for the whole batch, one wait, one download of count x 258 words."""
        import torch
        check_stack(clip_u8, 4, "frame statistics expect a uint8 count x H x W x 3 BGR device tensor", min_count=1, test_type=False)
        clip_u8 = clip_u8.contiguous()
        dev = clip_u8.device
        count, h, w = (int(v) for v in clip_u8.shape[:3])
        buf = torch.empty(count * 130, dtype=torch.int64, device=dev)       # count x 256 uint32, then count x 2 int64
        st = _lib.stream_ptr(dev)
        _lib.check(self._lib.fw_frame_stats_u8(_lib.ptr(clip_u8), count, h, w, _lib.ptr(buf),
                                               C.c_void_p(buf.data_ptr() + count * 1024), st))
        host = fetch(dev, buf)
        return host[:count * 128].view(np.uint32).reshape(count, 256).copy(), host[count * 128:].reshape(count, 2).copy()

    def frame_stats(self, frames: Sequence[np.ndarray]):
        """`stats_device` of host frames, uploaded `config.chunk_size` at a time -> (hist, sums) over all of them."""
        frames = _check_clip(frames)
        step = int(self.config.chunk_size)
        hists, sums = [np.zeros((0, 256), np.uint32)], [np.zeros((0, 2), np.int64)]
        for s in range(0, len(frames), step):
            with self.host() as dev:
                hs, ss = self.stats_device(upload(np.stack(frames[s:s + step]), dev))
            hists.append(hs)
            sums.append(ss)
        return np.concatenate(hists), np.concatenate(sums)

    def laplacian_variances(self, frames: Sequence[np.ndarray]) -> List[float]:
        """cv2.Laplacian(gray, CV_64F).var() of every frame."""
        frames = _check_clip(frames)
        if not frames:
            return []
        n_px = frames[0].shape[0] * frames[0].shape[1]
        return [laplacian_variance(n_px, s1, s2) for s1, s2 in self.frame_stats(frames)[1].tolist()]

    def analyze(self, frames: Sequence[np.ndarray], sample_rate: int = 5) -> Dict[str, Any]:
        """The reference's `analysis` dict for a clip of uint8 BGR frames."""
        frames = _check_clip(frames)
        if sample_rate < 1:
            raise ValueError(f"sample_rate must be >= 1, got {sample_rate}")
        if not frames:
            return {"error": "No frames found"}
        n = len(frames)
        analysis = {"total_frames": n, "noise_level": 0.0, "flicker_metrics": {}, "scene_changes": [], "recommended_config": {}}
        picked = sorted(set(range(0, n, sample_rate)) | {n - 1})            # what the three loops of the reference read
        hist, sums = self.frame_stats([frames[i] for i in picked])
        n_px = frames[0].shape[0] * frames[0].shape[1]
        hists: List[Optional[np.ndarray]] = [None] * n
        for k, i in enumerate(picked):
            hists[i] = hist[k]
        sampled = [k for k, i in enumerate(picked) if i % sample_rate == 0]  # frames[::sample_rate]
        if self.config.enable_flicker_reduction:
            # analyze_flicker samples frames[::sample_rate][:200] of a clip of at least three frames
            analysis["flicker_metrics"] = flicker_metrics_from_brightness(
                [brightness_from_hist(hist[k]) for k in sampled] if n >= 3 else [], 1, 200)
        analysis["scene_changes"] = scene_changes_from_hists(hists, sample_rate, self.config.scene_change_threshold)
        analysis["noise_level"] = noise_level_from_variances(
            [laplacian_variance(n_px, int(sums[k][0]), int(sums[k][1])) for k in sampled], 1)
        analysis["recommended_config"] = generate_recommendations(analysis, self.config)
        return analysis


class DeviceFlickerReducer(Stage):
    """`FlickerReducer` (temporal_denoise.py:480-836) on one GPU, on the reference's Python path `_apply_python_deflicker`
    (:764-836); the ffmpeg `deflicker` filter it tries first is not built, so this path is the behaviour, not the fallback.

    target = np.median of the mean gray level of frames[::10][:50] (fw_frame_stats_u8's histograms); per frame, L of 8-bit gamma Lab
    becomes clip(L + clip(target - mean L, -20, 20) * 0.5, 0, 255), truncated, and the frame returns to BGR.  The reference's quirk
    is kept: the target is a GRAY brightness, the frame's own value a mean of L.  For each batch of at most `chunk_size` resident
    frames the host waits once for the L sums (fw_lab_l_sums_u8), builds the 256-byte maps in float64 - what NumPy >= 2 computes for
    `l.astype(np.float32) + np.float64 scalar` - uploads them and launches fw_deflicker_lab_u8.  The mode changes no pixel on this
    path (it only chose ffmpeg parameters); `reduce_flicker` reports it as the reference does."""

    def __init__(self, mode: FlickerMode = FlickerMode.ADAPTIVE, preserve_brightness_changes: bool = True, gpu_id: int = 0,
                 chunk_size: int = 50):
        if chunk_size < 1:
            raise ValueError(f"chunk_size must be >= 1, got {chunk_size}")
        self.mode, self.preserve_brightness_changes = FlickerMode(mode), bool(preserve_brightness_changes)
        self.gpu_id, self.chunk_size = int(gpu_id), int(chunk_size)
        self._detected_severity: Optional[float] = None
        super().__init__(self.gpu_id)
        self._analyzer = DeviceClipAnalyzer(TemporalDenoiseConfig(gpu_id=self.gpu_id, chunk_size=max(10, self.chunk_size)))

    def analyze_flicker(self, frames: Sequence[np.ndarray], sample_rate: int = 1, max_samples: int = 200) -> Dict[str, Any]:
        """`analyze_flicker` (:518-625) of a clip of uint8 BGR frames; only the sampled frames are uploaded.  The severity is
        remembered: it resolves ADAPTIVE in `reduce_flicker`."""
        frames = _check_clip(frames)
        if sample_rate < 1:
            raise ValueError(f"sample_rate must be >= 1, got {sample_rate}")
        picked = frames[::sample_rate][:max_samples] if len(frames) >= 3 else []
        metrics = flicker_metrics_from_brightness([brightness_from_hist(h) for h in self._analyzer.frame_stats(picked)[0]], 1, max_samples)
        self._detected_severity = metrics["severity"]
        return metrics

    def resolved_mode(self) -> FlickerMode:
        """:660-668."""
        if self.mode == FlickerMode.ADAPTIVE and self._detected_severity is not None:
            s = self._detected_severity
            return FlickerMode.LIGHT if s < 0.1 else FlickerMode.MEDIUM if s < 0.3 else FlickerMode.AGGRESSIVE
        return self.mode

    @staticmethod
    def l_luts(l_sums: Sequence[int], n_pixels: int, target) -> np.ndarray:
        """uint8 [count][256]: the map of each frame's L plane (:825-832), float64 throughout, truncated."""
        levels = np.arange(256, dtype=np.float64)
        out = np.empty((len(l_sums), 256), np.uint8)
        for k, s in enumerate(l_sums):
            adjustment = np.clip(target - int(s) / int(n_pixels), -20, 20)
            out[k] = np.clip(levels + adjustment * 0.5, 0, 255).astype(np.uint8)
        return out

    def target_brightness(self, frames: Sequence[np.ndarray]):
        """:806-814 for a clip of numpy frames: only frames[::10][:50] are uploaded."""
        picked = _check_clip(list(frames)[::10][:50])
        return np.median([brightness_from_hist(h) for h in self._analyzer.frame_stats(picked)[0]])

    @_lib.on_tensor_device
    def target_brightness_device(self, devs):
        """The same from resident frames (a list, or a count x H x W x 3 stack)."""
        import torch
        picked = list(devs)[::10][:50]
        return np.median([brightness_from_hist(h) for h in self._analyzer.stats_device(torch.stack(picked))[0]])

    @_lib.on_tensor_device
    def deflicker_batch_device(self, batch, target, out=None):
        """One batch: a uint8 count x H x W x 3 BGR device tensor -> the deflickered batch (`out`, which may be `batch` itself, or a
        new tensor).  One wait (the L sums), one upload of count x 256 bytes, two launches."""
        import torch
        check_stack(batch, 4, "flicker reduction expects a uint8 count x H x W x 3 BGR device tensor", min_count=1, test_type=False)
        batch = batch.contiguous()
        dev = batch.device
        count, h, w = (int(v) for v in batch.shape[:3])
        if out is None:
            out = torch.empty_like(batch)
        else:
            check_out(out, "flicker reduction: `out` must be a contiguous uint8 device tensor of the batch's shape", torch.uint8, dev,
                      shape=batch.shape, test_type=False)
        sums = torch.empty(count, dtype=torch.int64, device=dev)
        st = _lib.stream_ptr(dev)
        _lib.check(self._lib.fw_lab_l_sums_u8(_lib.ptr(batch), count, h, w, _lib.ptr(sums), st))
        luts = upload(self.l_luts(fetch(dev, sums).tolist(), h * w, target), dev)
        _lib.check(self._lib.fw_deflicker_lab_u8(_lib.ptr(batch), count, h, w, _lib.ptr(luts),
                                                 _lib.ptr(out), st))
        # `luts` is freed when this returns; the caching allocator hands the block out again on this stream only, behind the launch
        return out

    @_lib.on_tensor_device
    def reduce_flicker_device(self, devs, target=None):
        """Resident uint8 BGR frames in - a list of H x W x 3 tensors or a count x H x W x 3 stack - resident deflickered frames out, in
        the same form.  `target` defaults to the one these frames give (frames[::10][:50]); a caller that streams a clip through in
        pieces passes the whole clip's."""
        import torch
        stacked = isinstance(devs, torch.Tensor)
        frames = devs if stacked else list(devs)
        if len(frames) == 0:
            return devs if stacked else []
        if target is None:
            target = self.target_brightness_device(frames)
        outs = []
        for s in range(0, len(frames), self.chunk_size):
            part = frames[s:s + self.chunk_size]
            outs.append(self.deflicker_batch_device(part if stacked else torch.stack(part), target))
        if stacked:
            return torch.cat(outs) if len(outs) > 1 else outs[0]
        return [f for o in outs for f in o.unbind(0)]

    def reduce_flicker(self, frames: Sequence[np.ndarray]) -> Tuple[List[np.ndarray], Dict[str, Any]]:
        """The host form of `reduce_flicker` (:626-700): numpy frames in, (numpy frames, the reference's result dict) out.  The clip
        is uploaded `chunk_size` frames at a time; the target comes from the sampled frames only."""
        frames = _check_clip(frames)
        if not frames:
            return [], {"frames_processed": 0, "mode_used": None}
        mode = self.resolved_mode()
        target = self.target_brightness(frames)
        out: List[np.ndarray] = []
        for s in range(0, len(frames), self.chunk_size):
            with self.host() as dev:
                batch = upload(np.stack(frames[s:s + self.chunk_size]), dev)
                out += list(fetch(dev, self.deflicker_batch_device(batch, target, out=batch)))
        return out, {"success": True, "frames_processed": len(out), "method": "python_brightness_normalization", "mode_used": mode.value}


class DeviceTemporalConsistencyFilter(Stage):
    """Phase 4 of the reference, `TemporalConsistencyFilter` (temporal_denoise.py:839-1061), on one GPU.

    Flow-guided form (`use_optical_flow` and more than one frame in the window, :955-1022): every neighbour is remapped onto the
    centre frame by `flow_estimator.maps_device(neighbour, centre)` and accumulated in float64 with the per-pixel weight
    tw (1 - s) + tw s confidence, tw = exp(-0.5 distance) (fw_flow_accumulate_affine_u8); the centre frame has weight 1, a
    neighbour whose flow raises the scalar weight tw, unaligned; the quotient (fw_flow_accumulate_finish_u8) is blended with the
    centre frame by cv2.addWeighted(centre, 1 - s, result, s) (fw_add_weighted_u8).  Simple form (:1024-1061): scalar weights tw,
    blend with s / 2.  Windows always read the INPUT frames: the filter is not recursive."""

    def __init__(self, strength: float = 0.5, temporal_radius: int = 2, use_optical_flow: bool = True,
                 flow_estimator: Optional[DeviceFlowEstimator] = None, gpu_id: int = 0):
        if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not math.isfinite(strength):
            raise ValueError(f"strength must be a finite number, got {strength!r}")
        if isinstance(temporal_radius, bool) or not isinstance(temporal_radius, (int, np.integer)) or temporal_radius < 0:
            raise ValueError(f"temporal_radius must be an int >= 0, got {temporal_radius!r}")
        self.strength, self.temporal_radius, self.use_optical_flow = float(strength), int(temporal_radius), bool(use_optical_flow)
        self.gpu_id = int(gpu_id)
        super().__init__(self.gpu_id)
        self.flow_estimator = flow_estimator or (DeviceFlowEstimator(gpu_id=self.gpu_id) if self.use_optical_flow else None)

    @_lib.on_tensor_device
    def apply_device(self, devs, i: int):
        """The filtered frame i of a clip of uint8 BGR device frames, as a uint8 device tensor.  Only launches."""
        import torch
        n, s = len(devs), self.strength
        if not 0 <= i < n:
            raise ValueError(f"frame index {i} outside the clip of {n} frames")
        lo, hi = max(0, i - self.temporal_radius), min(n, i + self.temporal_radius + 1)
        center = devs[i]
        dev = center.device
        h, w = int(center.shape[0]), int(center.shape[1])
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        st, p = _lib.stream_ptr(dev), _lib.ptr
        guided = self.use_optical_flow and hi - lo > 1
        for j in range(lo, hi):
            tw = float(np.exp(-abs(j - i) * 0.5))
            fx = fy = conf = None
            w_const, w_conf = tw, 0.0                                  # the simple form, and a neighbour whose flow failed
            if guided and j == i:
                w_const = 1.0
            elif guided:
                try:
                    fx, fy, _, conf = self.flow_estimator.maps_device(devs[j], center)
                    w_const, w_conf = tw * (1 - s), tw * s
                except Exception:                                      # "Flow estimation failed" (:993-996)
                    fx = fy = conf = None
            _lib.check(self._lib.fw_flow_accumulate_affine_u8(p(devs[j]), p(fx), p(fy), p(conf), w_const, w_conf, 0, h, w, p(acc), p(ws), st))
        result = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        _lib.check(self._lib.fw_flow_accumulate_finish_u8(p(acc), p(ws), h, w, p(result), st))
        blend = s if guided else s * 0.5
        out = torch.empty_like(result)
        _lib.check(self._lib.fw_add_weighted_u8(p(center), 1 - blend, p(result), blend, h * w * 3, p(out), st))
        return out

    def apply_sequence(self, frames: Sequence[np.ndarray]) -> Iterator[np.ndarray]:
        """`TemporalConsistencyFilter.apply` over a clip of numpy frames: the clip is uploaded once, one wait and one download per
        output frame."""
        import torch
        frames = _check_clip(frames)
        dev = self._dev
        with self.host():
            devs = [upload(f, dev) for f in frames]
        for i in range(len(frames)):
            with self.host():
                out = self.apply_device(devs, i)
                torch.cuda.synchronize(dev)
                res = out.cpu().numpy()
            yield res


class DeviceTemporalDenoiser:
    """`TemporalDenoiser` (temporal_denoise.py:1064-1424) on one GPU: analysis, the accumulate -> non-local means -> edge-preserve
    chain, the temporal-consistency pass and the noise-reduction estimate, with the clip on the device from the upload of a frame to
    the download of its result.  The reference hands PNG directories from phase to phase (lossless: the same bytes).  Flicker
    reduction (phase 2) is opt-in: with `device_flicker=True` and `config.enable_flicker_reduction` every input frame is deflickered on
    the device as it is uploaded (`DeviceFlickerReducer`), with the target of the whole clip's samples; otherwise it is the
    caller's (`deflicker_fn`, see the module docstring) or does not happen."""

    NOISE_REDUCTION_FRAMES = 20     # `_estimate_noise_reduction` reads the first 20 (:1751)

    def __init__(self, config: Optional[TemporalDenoiseConfig] = None, device_flicker: bool = False):
        self.config = config or TemporalDenoiseConfig()
        c = self.config
        self.device_flicker = bool(device_flicker)
        self._flicker_reducer = DeviceFlickerReducer(mode=c.flicker_mode, gpu_id=c.gpu_id, chunk_size=c.chunk_size) \
            if self.device_flicker else None
        self._analyzer = DeviceClipAnalyzer(c)
        self._flow_estimator = DeviceFlowEstimator(method=c.optical_flow_method, gpu_id=c.gpu_id)
        self._accumulator = DeviceTemporalAccumulator(temporal_weight_decay=c.temporal_weight_decay, gpu_id=c.gpu_id,
                                                      flow_estimator=self._flow_estimator)
        self._consistency_filter = DeviceTemporalConsistencyFilter(strength=c.noise_strength, temporal_radius=c.temporal_radius,
                                                                   use_optical_flow=c.enable_optical_flow,
                                                                   flow_estimator=self._flow_estimator, gpu_id=c.gpu_id)
        self._scene_changes: List[int] = []

    def analyze(self, frames: Sequence[np.ndarray], sample_rate: int = 5) -> Dict[str, Any]:
        analysis = self._analyzer.analyze(frames, sample_rate)
        self._scene_changes = analysis.get("scene_changes", [])
        return analysis

    def denoise_clip(self, frames: Sequence[np.ndarray], deflicker_fn: Optional[Callable] = None,
                     progress_callback: Optional[Callable[[float], None]] = None) -> Tuple[List[np.ndarray], TemporalDenoiseResult]:
        """`denoise_frames` on a clip in memory -> (the output frames, the reference's result record).

        Frames stream through the two device phases chunk by chunk: at most chunk_size + 2 radius input frames and as many denoised
        frames are resident, a denoised frame is dropped once the last consistency window that reads it is done, and every frame is
        computed from the same windows whatever `chunk_size` is - the output does not depend on it.  Scene-cut indices at or beyond
        the clip's end (`scene_changes_from_hists`) match no frame in the reference and are dropped here.
        Progress: the reference's fractions at the phase boundaries and per chunk of phase 3; phase 4 runs interleaved with it, so its
        per-frame fractions are not reported.
        With `device_flicker` (and `config.enable_flicker_reduction`) the analysis reads the original frames, the target brightness
        comes from the whole clip's samples before phase 3 starts, and each input frame is deflickered on the device when it is
        uploaded: nothing returns to the host between the phases.  `deflicker_fn` together with `device_flicker` is a ValueError."""
        import torch
        if deflicker_fn is not None and self.device_flicker:
            raise ValueError("pass deflicker_fn (a host hook) or build the denoiser with device_flicker=True, not both")
        start = time.time()
        c = self.config
        tell = progress_callback or (lambda p: None)
        frames = _check_clip(frames)
        result = TemporalDenoiseResult()
        n = len(frames)
        if n == 0:
            return [], result
        tell(0.02)
        analysis = self.analyze(frames)
        result.scene_changes_detected = analysis.get("scene_changes", [])
        tell(0.05)
        current = frames
        if c.enable_flicker_reduction and deflicker_fn is not None:
            current = _check_clip(deflicker_fn(list(frames)))
            if len(current) != n or current[0].shape != frames[0].shape:
                raise ValueError("deflicker_fn must return as many frames, of the same size, as it was given")
            result.flicker_reduction_applied = True
        target = None
        if c.enable_flicker_reduction and self.device_flicker:
            target = self._flicker_reducer.target_brightness(frames)
            result.flicker_reduction_applied = True
        tell(0.25)
        cuts = {i for i in self._scene_changes if i < n}
        r, step = c.temporal_radius, c.chunk_size
        spatial = c.noise_strength if c.noise_strength > DeviceTemporalAccumulator.SPATIAL_THRESHOLD else None
        dev = self._analyzer._dev
        inputs: Dict[int, Any] = {}       # resident input frames
        denoised: Dict[int, Any] = {}     # resident phase-3 results
        outputs: List[np.ndarray] = []
        out_vars: List[float] = []
        n_px = frames[0].shape[0] * frames[0].shape[1]
        for s in range(0, n, step):
            e = min(s + step, n)
            with torch.cuda.device(dev):
                for i in [k for k in inputs if k < s - r]:
                    del inputs[i]
                fresh = [i for i in range(max(0, s - r), min(n, e + r)) if i not in inputs]
                if target is None:
                    for i in fresh:
                        inputs[i] = upload(current[i], dev)
                elif fresh:
                    batch = upload(np.stack([current[i] for i in fresh]), dev)
                    for i, t in zip(fresh, self._flicker_reducer.reduce_flicker_device(batch, target).unbind(0)):
                        inputs[i] = t
                for i in range(s, e):
                    lo, hi = (i, i + 1) if i in cuts else (max(0, i - r), min(n, i + r + 1))
                    window = [inputs[k] for k in range(lo, hi)]
                    denoised[i] = self._accumulator._chain_device(i - lo, window, spatial, c.preserve_edges, c.edge_threshold,
                                                                  simple=not (c.enable_optical_flow and len(window) > 1))
                tell(0.25 + (e / n) * 0.6)
                # phase 4 for every frame whose window is complete
                done = len(outputs)
                ready = n if e == n else max(done, e - r)
                base = max(0, done - r)
                clip = [denoised[k] for k in range(base, e)]
                finished = []
                for i in range(done, ready):
                    finished.append(self._consistency_filter.apply_device(clip, i - base))
                torch.cuda.synchronize(dev)
                head = [t for i, t in zip(range(done, ready), finished) if i < self.NOISE_REDUCTION_FRAMES]
                if head:
                    out_vars += [laplacian_variance(n_px, s1, s2) for s1, s2 in self._analyzer.stats_device(torch.stack(head))[1].tolist()]
                outputs += [t.cpu().numpy() for t in finished]
                for i in [k for k in denoised if k < ready - r]:
                    del denoised[i]
        tell(0.85)
        tell(0.95)
        result.frames_processed = len(outputs)
        result.frames_failed = n - result.frames_processed
        result.avg_noise_reduction = noise_reduction_from_variances(
            self._analyzer.laplacian_variances(frames[:self.NOISE_REDUCTION_FRAMES]), out_vars)
        result.processing_time_seconds = time.time() - start
        tell(1.0)
        return outputs, result

    def denoise_frames(self, input_dir: Union[str, Path], output_dir: Union[str, Path],
                       progress_callback: Optional[Callable[[float], None]] = None) -> TemporalDenoiseResult:
        """The directory form (:1302-1424): `*.png`, else `*.jpg`, sorted; the results are written under the same names."""
        from PIL import Image
        input_dir, output_dir = Path(input_dir), Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        paths = sorted(input_dir.glob("*.png")) or sorted(input_dir.glob("*.jpg"))
        if not paths:
            return TemporalDenoiseResult()
        start = time.time()
        outputs, result = self.denoise_clip([DeviceFlowEstimator._load(p) for p in paths], progress_callback=progress_callback)
        for p, frame in zip(paths, outputs):
            Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(str(output_dir / p.name))
        result.output_dir = output_dir
        result.processing_time_seconds = time.time() - start
        return result


def create_temporal_denoiser(strength: float = 0.5, temporal_radius: int = 3, enable_optical_flow: bool = True,
                             enable_flicker_reduction: bool = True, gpu_id: int = 0, device_flicker: bool = False) -> DeviceTemporalDenoiser:
    """The reference's factory (temporal_denoise.py:1894-1920); `device_flicker` opts into phase 2 on the device."""
    return DeviceTemporalDenoiser(TemporalDenoiseConfig(noise_strength=strength, temporal_radius=temporal_radius,
                                                        enable_optical_flow=enable_optical_flow,
                                                        enable_flicker_reduction=enable_flicker_reduction, gpu_id=gpu_id),
                                  device_flicker=device_flicker)
