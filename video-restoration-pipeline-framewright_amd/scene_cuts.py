"""Scene-cut detection on the device for the frame interpolator (kernel set K13, csrc/scene_cuts.hip).

The reference's `FrameInterpolator.detect_scene_change` (src/framewright/processors/interpolation.py:267-366) decides a cut from
the SSIM of the mean-gray images, and from a 3 x 64-bin histogram intersection when the SSIM cannot be formed.  `policy.scene_change`
is that test on the host in float64 NumPy; `DeviceSceneCutDetector` is the same test on uint8 frames that are already on the GPU:
`fw_scene_ssim_u8` leaves one float64 per pair, `fw_hist64x3_u8` 192 counts per frame, and only those are downloaded.  Both tests
are symmetric in the channel order, so BGR tensors give the decisions the host path takes from RGB arrays.
tests/scene_cut_ref.py is the contract of the two kernels.
"""
from __future__ import annotations

from typing import List

import numpy as np

from . import _lib
from ._stage import Stage, check_stack, fetch

SSIM_WINDOW = 7


class DeviceSceneCutDetector(Stage):
    """The scene-cut tests of `policy.scene_change` on one GPU.  Every method takes uint8 CUDA tensors (H x W x 3, or n x H x W x 3
    for a clip), enqueues on torch's current stream of the tensors' device, waits for that stream and returns host values."""

    def __init__(self, gpu_id: int = 0):
        self.gpu_id = int(gpu_id)
        super().__init__(self.gpu_id)

    @staticmethod
    def _check(t, dims: int, what: str):
        check_stack(t, dims, f"{what} expects uint8 CUDA tensors {'n x ' if dims == 4 else ''}H x W x 3")
        return t.contiguous()

    def _ssim(self, a, b, stride: int, pairs: int, h: int, w: int) -> List[float]:
        import torch
        dev = a.device
        out = torch.empty(pairs, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, self._lib.fw_scene_ssim_workspace_bytes(pairs, h, w) // 8), dtype=torch.float64, device=dev)
        _lib.check(self._lib.fw_scene_ssim_u8(_lib.ptr(a), _lib.ptr(b), stride, pairs, h, w, _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr(dev)))
        return fetch(dev, out).tolist()

    @_lib.on_tensor_device
    def ssim_pairs_device(self, frames) -> List[float]:
        """SSIM of the n - 1 consecutive pairs of a uint8 n x H x W x 3 device clip: one launch, one wait, n - 1 floats back.
        Raises FramewrightHipError (FW_ERR_INVALID) when a side is shorter than the 7-pixel window."""
        frames = self._check(frames, 4, "ssim_pairs_device")
        n, h, w = (int(v) for v in frames.shape[:3])
        if n < 2:
            return []
        return self._ssim(frames[0], frames[1], h * w * 3, n - 1, h, w)

    @_lib.on_tensor_device
    def ssim_pair_device(self, a, b) -> float:
        a, b = self._check(a, 3, "ssim_pair_device"), self._check(b, 3, "ssim_pair_device")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError("frame sizes or devices differ")
        return self._ssim(a, b, 0, 1, int(a.shape[0]), int(a.shape[1]))[0]

    @_lib.on_tensor_device
    def histograms_device(self, frames) -> np.ndarray:
        """int64 n x 3 x 64: per frame and channel, np.histogram(bins=64, range=(0, 256)) of its bytes."""
        import torch
        frames = self._check(frames, 4, "histograms_device")
        n, h, w = (int(v) for v in frames.shape[:3])
        if n < 1 or h < 1 or w < 1:
            raise ValueError("histograms_device expects at least one non-empty frame")
        dev = frames.device
        hist = torch.empty((n, 3, 64), dtype=torch.int32, device=dev)
        _lib.check(self._lib.fw_hist64x3_u8(_lib.ptr(frames), n, h, w, _lib.ptr(hist), _lib.stream_ptr(dev)))
        return fetch(dev, hist).view(np.uint32).astype(np.int64)

    @staticmethod
    def histogram_decision(h1: np.ndarray, h2: np.ndarray, scene_threshold: float = 0.3) -> bool:
        """`policy.scene_change_by_histogram`'s own float expression on two 3 x 64 tables of counts."""
        h1, h2 = np.asarray(h1).reshape(-1), np.asarray(h2).reshape(-1)
        h1 = h1.astype(float) / h1.sum()
        h2 = h2.astype(float) / h2.sum()
        return bool(np.minimum(h1, h2).sum() < (1.0 - scene_threshold))

    def scene_change_device(self, a, b, scene_threshold: float = 0.3, use_ssim: bool = True) -> bool:
        """`policy.scene_change(a, b, scene_threshold, use_ssim)` on two device frames: SSIM < 1 - threshold; the histogram test
        when the SSIM cannot be formed (a side shorter than 7, or frames of different sizes) or is not asked for."""
        a, b = self._check(a, 3, "scene_change_device"), self._check(b, 3, "scene_change_device")
        if use_ssim and a.shape == b.shape and min(a.shape[:2]) >= SSIM_WINDOW:
            return bool(self.ssim_pair_device(a, b) < (1.0 - scene_threshold))
        ha, hb = self.histograms_device(a.unsqueeze(0))[0], self.histograms_device(b.unsqueeze(0))[0]
        return self.histogram_decision(ha, hb, scene_threshold)

    def detect_clip_device(self, frames, scene_threshold: float = 0.3) -> List[int]:
        """Boundary indices i + 1 of the pairs (i, i + 1) of a device clip that are cuts."""
        frames = self._check(frames, 4, "detect_clip_device")
        n, h, w = (int(v) for v in frames.shape[:3])
        if n < 2:
            return []
        if min(h, w) >= SSIM_WINDOW:
            flags = [s < (1.0 - scene_threshold) for s in self.ssim_pairs_device(frames)]
        else:
            hs = self.histograms_device(frames)
            flags = [self.histogram_decision(hs[i], hs[i + 1], scene_threshold) for i in range(n - 1)]
        return [i + 1 for i, f in enumerate(flags) if f]
