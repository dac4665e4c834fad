"""What the Python drivers of the eighteen frame stages share (DeviceFlowEstimator, DeviceSpatialDenoiser, DeviceTemporalAccumulator,
DeviceClipAnalyzer, DeviceFlickerReducer, DeviceTemporalConsistencyFilter, DeviceSceneCutDetector, DeviceFrameDeduplicator,
DeviceColorGrader, DeviceDeinterlacer, DeviceVHSProcessor, DeviceAspectHandler, DeviceFrameQualityScorer, DeviceHDRConverter,
DeviceQPArtifactRemover, DeviceMissingFrameGenerator, DeviceTemporalConsistencyProcessor, DevicePerceptualTuner): the owner of a device and a scratch buffer, the frame checks, the overlap
check and the transfers between numpy and the device.  The C++ counterpart is csrc/stage_common.h.  Every check takes the refusing
stage's own message: what a stage says when it refuses is the stage's, that it is said is written here.
"""
from __future__ import annotations

import contextlib

import numpy as np

from . import _lib

ANY = 1 << 62                                       # an upper bound that no frame reaches

# ---- host transfer ------------------------------------------------------------------------------------------------------------------
def upload(array, dev):
    """A numpy array (made contiguous where it is not) as a tensor on ``dev``."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def fetch(dev, *tensors):
    """Waits once, for torch's current stream on ``dev``, and returns the tensors as numpy arrays (one tensor: the array itself)."""
    import torch
    torch.cuda.current_stream(dev).synchronize()
    arrays = [t.cpu().numpy() for t in tensors]
    return arrays[0] if len(arrays) == 1 else arrays


# ---- frame checks -------------------------------------------------------------------------------------------------------------------
def contiguous(frames) -> list:
    """The frames, each as it is where it is contiguous, else a contiguous copy."""
    return [f if f.is_contiguous() else f.contiguous() for f in frames]


def check_frame_list(frames, wrong: str, bounds, dev=None, wrong_dtype: str = None, wrong_device: str = None) -> tuple:
    """A non-empty list of uint8 CUDA frames H x W x 3 or H x W of one shape -> (h, w, channels).  They must all be on ``dev``, or on
    the first frame's device when ``dev`` is None.  ``wrong`` is the stage's refusal of a frame that is none of that; ``wrong_dtype``
    and ``wrong_device`` replace it for a frame that is no uint8 tensor / not on the device, for a stage that tells them apart.
    ``bounds``: the stage's (min rows, max rows, min columns, max columns, message), checked in turn; `ANY` for no upper bound.
    This runs on every call, also for one small frame: each frame's shape is read once, and the bounds are plain integers."""
    import torch
    f0 = frames[0]
    shape0, dev = getattr(f0, "shape", None), (dev if dev is not None else getattr(f0, "device", None))
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8:
            raise ValueError(wrong_dtype or wrong)
        if not f.is_cuda or f.device != dev:
            raise ValueError(wrong_device or wrong)
        shape = f.shape
        if shape != shape0 or (len(shape) != 2 and (len(shape) != 3 or shape[2] != 3)):
            raise ValueError(wrong)
    h, w = shape0[0], shape0[1]
    for min_h, max_h, min_w, max_w, message in bounds:
        if not (min_h <= h <= max_h and min_w <= w <= max_w):
            raise ValueError(message)
    return h, w, (3 if len(shape0) == 3 else 1)


def check_stack(t, dims: int, wrong: str, dtypes=None, min_count: int = 0, test_type: bool = True) -> None:
    """A CUDA tensor of ``dims`` dimensions whose last is 3 - a frame H x W x 3 (3) or a stack n x H x W x 3 (4) - of one of
    ``dtypes`` (uint8 when None) and of at least ``min_count`` entries along its first dimension; else ValueError(``wrong``).
    ``test_type=False`` is for a stage that never tested for a tensor: what is none fails on its first attribute, as it did."""
    import torch
    if (test_type and not isinstance(t, torch.Tensor)) or t.dtype not in (dtypes or (torch.uint8,)) or not t.is_cuda or \
            t.dim() != dims or t.shape[-1] != 3 or t.shape[0] < min_count:
        raise ValueError(wrong)


def check_out(out, wrong: str, dtype, dev, numel: int = None, shape=None, test_type: bool = True) -> None:
    """A caller's destination: a contiguous tensor of ``dtype`` on ``dev`` with ``numel`` elements or of ``shape``."""
    import torch
    if (test_type and not isinstance(out, torch.Tensor)) or out.dtype != dtype or out.device != dev or not out.is_contiguous() or \
            (numel is not None and out.numel() != numel) or (shape is not None and out.shape != shape):
        raise ValueError(wrong)


def storage_range(t):
    """[first byte, last byte + 1) of the storage a uint8 tensor's elements lie in."""
    span = 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride())) if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + span


def check_no_overlap(dsts, srcs, who: str) -> None:
    """Refuses, in the name of stage ``who``, destinations that share bytes with a source (a kernel would read rows it has rebuilt)."""
    marks = sorted([(*storage_range(t), 0) for t in dsts] + [(*storage_range(t), 1) for t in srcs])
    end = [0, 0]                                     # furthest end so far of destinations / of sources
    for lo, hi, kind in marks:
        if hi > lo and lo < end[1 - kind]:
            raise ValueError(f"{who}: a destination overlaps a source frame (rebuilt rows are read as neighbours)")
        end[kind] = max(end[kind], hi)


# ---- the owner ----------------------------------------------------------------------------------------------------------------------
class Stage:
    """Base of the drivers: the loaded library ``_lib``, the device ``_dev`` (a ``torch.device``, what `_lib.owner_device` and
    `_lib.on_tensor_device` read) and one scratch buffer.  A subclass keeps its public name for the index (``gpu_id`` / ``device_id``),
    validates its own arguments before it calls this constructor, and writes its messages and its ``fw_*`` calls."""

    def __init__(self, index: int, needs_gpu: bool = True):
        """``needs_gpu=False`` puts the refusal of a machine without a GPU off to the first `gpu_device()`."""
        import torch
        self._lib = _lib.load()
        self._dev = torch.device("cuda", int(index))
        self._gpu_seen = False
        self._scratch = None
        if needs_gpu:
            self.gpu_device()

    def gpu_device(self):
        """``_dev``, once a GPU is known to be there (`FramewrightHipError` when none is: there is no CPU fallback)."""
        if not self._gpu_seen:
            _lib.require_gpu()
            self._gpu_seen = True
        return self._dev

    def scratch(self, need_bytes: int, dev):
        """The stage's one uint8 scratch tensor, at least ``need_bytes`` on ``dev``: it only grows, and is made anew on another device."""
        import torch
        if self._scratch is None or self._scratch.numel() < need_bytes or self._scratch.device != dev:
            self._scratch = torch.empty(need_bytes, dtype=torch.uint8, device=dev)
        return self._scratch

    @contextlib.contextmanager
    def host(self):
        """The body of a numpy-in / numpy-out method, with the stage's device current:
        ``with self.host() as dev: out = self.x_device(upload(a, dev)); return fetch(dev, out)``."""
        import torch
        with torch.cuda.device(self.gpu_device()):
            yield self._dev
