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
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from enum import Enum
from pathlib import Path
from typing import Callable, Iterator, List, Optional, Sequence, Union

import numpy as np

from . import _lib


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


class DeviceFlowEstimator:
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
        self._lib = _lib.load()
        _lib.require_gpu()
        self._scratch = None

    def _dev(self):
        import torch
        return torch.device("cuda", self.gpu_id)

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
        import torch
        need = int(self._lib.fw_farneback_scratch_bytes(h, w, int(self.params["levels"])))
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._scratch

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
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(self._lib.fw_farneback_flow_u8(C.c_void_p(t1.data_ptr()), C.c_void_p(t2.data_ptr()), 1 if t1.dim() == 2 else 3, h, w,
                                                  float(p["pyr_scale"]), int(p["levels"]), int(p["winsize"]), int(p["iterations"]),
                                                  int(p["poly_n"]), float(p["poly_sigma"]), int(p["flags"]),
                                                  C.c_void_p(scratch.data_ptr()), C.c_void_p(fx.data_ptr()), C.c_void_p(fy.data_ptr()), st))
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
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
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
        import torch
        dev = self._dev()
        a, b = self._load(frame1), self._load(frame2)
        with torch.cuda.device(dev):
            maps = self.maps_device(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
            torch.cuda.current_stream(dev).synchronize()
            fx, fy, mag, conf = (m.cpu().numpy() for m in maps)
        return FlowField(flow_x=fx, flow_y=fy, magnitude=mag, confidence=conf, frame_idx_from=0, frame_idx_to=1)

    def warp_frame(self, frame: np.ndarray, flow: FlowField, inverse: bool = False) -> np.ndarray:
        """`OpticalFlowEstimator.warp_frame` (:440-477), the existing remap kernel."""
        return DeviceTemporalAccumulator(gpu_id=self.gpu_id).warp_frame(frame, flow, inverse=inverse)


class DeviceSpatialDenoiser:
    """`TemporalDenoiser._apply_spatial_denoise` (temporal_denoise.py:1611-1634) on one GPU: non-local means on the Lab planes of a
    BGR frame (fw_nlmeans_colored_u8), and the plain core on a 1-, 2- or 3-channel plane (fw_nlmeans_u8).  The windows are the
    reference's (7, 21); the kernels take a template window of 3, 5 or 7 and an odd search window of 3 .. 41, and even sizes are
    rejected where cv2 would force them odd.  tests/nlmeans_ref.py is the contract (bit-exact); cv2 parity unpinned."""

    def __init__(self, gpu_id: int = 0, template_window: int = 7, search_window: int = 21):
        self.gpu_id, self.template_window, self.search_window = int(gpu_id), int(template_window), int(search_window)
        self._lib = _lib.load()
        _lib.require_gpu()
        self._scratch = None

    def _dev(self):
        import torch
        return torch.device("cuda", self.gpu_id)

    @staticmethod
    def h_for_strength(strength: float) -> int:
        """The filter strength of the reference's call (:1627)."""
        return int(3 + strength * 7)

    def _scratch_for(self, h: int, w: int, dev):
        import torch
        need = int(self._lib.fw_nlmeans_scratch_bytes(h, w, self.search_window))
        if need <= 0:
            raise ValueError(f"non-local means: bad frame size {h} x {w} or search window {self.search_window}")
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._scratch

    @_lib.on_tensor_device
    def denoise_device(self, t, h: float, h_color: Optional[float] = None):
        """cv2.fastNlMeansDenoisingColored(t, None, h, h_color, template, search) of a uint8 BGR (H x W x 3) device tensor -> a new
        device tensor; `t` is left untouched, nothing is fetched and nothing waits for the device.  h_color defaults to h, the
        reference's call."""
        import torch
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda:
            raise ValueError("the spatial denoise expects a uint8 BGR (H x W x 3) device frame")
        t = t.contiguous()
        dev = t.device
        hh, ww = int(t.shape[0]), int(t.shape[1])
        scratch = self._scratch_for(hh, ww, dev)
        out = torch.empty_like(t)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(self._lib.fw_nlmeans_colored_u8(C.c_void_p(t.data_ptr()), hh, ww, float(h), float(h if h_color is None else h_color),
                                                   self.template_window, self.search_window, C.c_void_p(scratch.data_ptr()),
                                                   C.c_void_p(out.data_ptr()), st))
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
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(self._lib.fw_nlmeans_u8(C.c_void_p(plane.data_ptr()), 1 if plane.dim() == 2 else int(plane.shape[2]), int(plane.shape[0]),
                                           int(plane.shape[1]), float(h), self.template_window, self.search_window, None,
                                           C.c_void_p(out.data_ptr()), st))
        return out

    def denoise(self, frame: np.ndarray, strength: float) -> np.ndarray:
        """`_apply_spatial_denoise(frame, strength)`: numpy uint8 BGR in and out."""
        import torch
        frame = np.ascontiguousarray(frame)
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("the spatial denoise expects a uint8 BGR (H x W x 3) frame")
        dev = self._dev()
        with torch.cuda.device(dev):
            out = self.denoise_device(torch.from_numpy(frame).to(dev), self.h_for_strength(strength))
            torch.cuda.current_stream(dev).synchronize()
            return out.cpu().numpy()


class DeviceTemporalAccumulator:
    """The float64 accumulate of `_denoise_with_flow` / `_denoise_simple` on one GPU.

    flow_fn: a host estimator, `flow_fn(frame, center) -> FlowField` (e.g. cv2's); its maps are uploaded per neighbour.
    flow_estimator: a `DeviceFlowEstimator`; `denoise_with_flow` and `denoise_sequence` then keep frames, flows, statistics and weights
    on the device and wait for it once per output frame.  Passing both is a ValueError; with neither, the flow-compensated method
    behaves as the reference does without OpenCV."""

    def __init__(self, temporal_weight_decay: float = 0.5, gpu_id: int = 0, flow_fn: Optional[Callable] = None,
                 flow_estimator: Optional[DeviceFlowEstimator] = None):
        if flow_fn is not None and flow_estimator is not None:
            raise ValueError("pass flow_fn (a host estimator) or flow_estimator (a DeviceFlowEstimator), not both")
        self._lib = _lib.load()
        _lib.require_gpu()
        self.decay, self.gpu_id = float(temporal_weight_decay), int(gpu_id)
        self.flow_fn = flow_fn or _default_flow_fn
        self.flow_estimator = flow_estimator
        self._spatial = None

    def _dev(self):
        import torch
        return torch.device("cuda", self.gpu_id)

    def warp_frame(self, frame: np.ndarray, flow: FlowField, inverse: bool = False) -> np.ndarray:
        """`OpticalFlowEstimator.warp_frame`: cv2.remap(frame, grid +/- flow, INTER_LINEAR, BORDER_REFLECT_101)."""
        import torch
        dev = self._dev()
        h, w = frame.shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        self._accumulate(torch.from_numpy(np.ascontiguousarray(frame)).to(dev), flow, 1.0, None, None, inverse, acc, ws)
        return self._finish(acc, ws)

    @_lib.on_tensor_device
    def _accumulate(self, frame_dev, flow: Optional[FlowField], scale: float, wmap, thr, inverse, acc, ws) -> None:
        import torch
        dev = acc.device
        h, w = int(acc.shape[0]), int(acc.shape[1])
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        keep = []
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
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
        st = C.c_void_p(torch.cuda.current_stream(acc.device).cuda_stream)
        _lib.check(self._lib.fw_flow_accumulate_finish_u8(C.c_void_p(acc.data_ptr()), C.c_void_p(ws.data_ptr()), h, w,
                                                          C.c_void_p(out.data_ptr()), st))
        torch.cuda.synchronize(acc.device)
        return out.cpu().numpy()

    def denoise_with_flow(self, center_local_idx: int, window: Sequence[np.ndarray]) -> np.ndarray:
        """`_denoise_with_flow` (temporal_denoise.py:1521-1580) for the frames of one window."""
        import torch
        dev = self._dev()
        if self.flow_estimator is not None:
            with torch.cuda.device(dev):
                out = self._window_device(center_local_idx, [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in window])
                torch.cuda.synchronize(dev)
            return out.cpu().numpy()
        center = window[center_local_idx]
        h, w = center.shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        for local_i, frame in enumerate(window):
            distance = abs(local_i - center_local_idx)
            fd = torch.from_numpy(np.ascontiguousarray(frame)).to(dev)
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
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
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
        dev = self._dev()
        if self.flow_estimator is None:
            for i in range(n):
                lo, hi = (i, i + 1) if i in cuts else (max(0, i - temporal_radius), min(n, i + temporal_radius + 1))
                out = self.denoise_with_flow(i - lo, frames[lo:hi])
                if spatial:
                    out = self._spatial_denoiser().denoise(out, noise_strength)
                yield self.preserve_edges(frames[i], out, edge_threshold) if preserve_edges else out
            return
        with torch.cuda.device(dev):
            devs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
        for i in range(n):
            lo, hi = (i, i + 1) if i in cuts else (max(0, i - temporal_radius), min(n, i + temporal_radius + 1))
            with torch.cuda.device(dev):
                out = self._window_device(i - lo, devs[lo:hi])
                if spatial:
                    out = self._spatial_denoiser().denoise_device(out, DeviceSpatialDenoiser.h_for_strength(noise_strength))
                if preserve_edges:
                    h, w = int(out.shape[0]), int(out.shape[1])
                    scratch = torch.empty(int(self._lib.fw_preserve_edges_scratch_bytes(h, w)), dtype=torch.uint8, device=dev)
                    blended = torch.empty_like(out)
                    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _lib.check(self._lib.fw_preserve_edges_u8(C.c_void_p(devs[i].data_ptr()), C.c_void_p(out.data_ptr()), h, w,
                                                              float(edge_threshold), float(edge_threshold * 3),
                                                              C.c_void_p(scratch.data_ptr()), C.c_void_p(blended.data_ptr()), st))
                    out = blended
                torch.cuda.synchronize(dev)
                res = out.cpu().numpy()
            yield res

    def preserve_edges(self, original: np.ndarray, denoised: np.ndarray, edge_threshold: int = 30) -> np.ndarray:
        """`TemporalDenoiser._preserve_edges` (temporal_denoise.py:1636-1667): the original frame shows through a blurred,
        dilated Canny edge mask (thresholds ``edge_threshold`` and three times that, config default 30, :146).  uint8 BGR frames
        in and out; fw_preserve_edges_u8."""
        import torch
        if original.shape != denoised.shape or original.dtype != np.uint8 or denoised.dtype != np.uint8 or original.ndim != 3 or \
                original.shape[2] != 3:
            raise ValueError("preserve_edges expects two uint8 BGR frames of one size")
        dev = self._dev()
        h, w = original.shape[:2]
        with torch.cuda.device(dev):
            o = torch.from_numpy(np.ascontiguousarray(original)).to(dev)
            d = torch.from_numpy(np.ascontiguousarray(denoised)).to(dev)
            scratch = torch.empty(int(self._lib.fw_preserve_edges_scratch_bytes(h, w)), dtype=torch.uint8, device=dev)
            out = torch.empty_like(o)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(self._lib.fw_preserve_edges_u8(C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), h, w, float(edge_threshold),
                                                      float(edge_threshold * 3), C.c_void_p(scratch.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), st))
            torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    def denoise_simple(self, window: Sequence[np.ndarray]) -> np.ndarray:
        """`_denoise_simple` (temporal_denoise.py:1582-1605).  The reference divides by a scalar weight sum; per-pixel sums
        of the same scalars give the same float64 quotient."""
        import torch
        dev = self._dev()
        h, w = window[0].shape[:2]
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        ws = torch.zeros((h, w), dtype=torch.float64, device=dev)
        center_idx = len(window) // 2
        for i, frame in enumerate(window):
            self._accumulate(torch.from_numpy(np.ascontiguousarray(frame)).to(dev), None, math.exp(-abs(i - center_idx) * self.decay),
                             None, None, False, acc, ws)
        return self._finish(acc, ws)
