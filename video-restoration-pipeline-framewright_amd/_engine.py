"""What the Python owners of the six network engines share (RRDBNetEngine, NAFNetEngine, IFNetEngine, RestormerEngine, SRVGGNetEngine,
AESRGANEngine): weight conversion, the owner of one native handle, and the fan-out of independent forwards over side streams.
The C++ counterpart is csrc/engine_common.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Sequence

import numpy as np

from . import _lib
from ._lib import FramewrightHipError


def to_numpy(t) -> np.ndarray:
    """A weight as a numpy array: arrays pass through, torch tensors (any float type, any device) come back as float32."""
    if isinstance(t, np.ndarray):
        return t
    if hasattr(t, "detach"):
        return t.detach().float().cpu().numpy()
    return np.asarray(t)


def unwrap_state(state: Mapping[str, object], keys: Sequence[str]) -> Mapping[str, object]:
    """The state dict inside a checkpoint: the value under the first of the wrapper ``keys`` that is present, else ``state``."""
    for k in keys:
        if k in state:
            return state[k]  # type: ignore[return-value]
    return state


class Engine:
    """Owner of one native engine handle ``_h`` on one GPU.  A subclass names its ``fw_*_create`` / ``fw_*_destroy`` entries, checks
    its structural arguments in ``_configure`` and makes the ctypes call of its forward; everything below is written here once."""

    def __init__(self, create: str, destroy: str, dtype: str, device_id: int, **config):
        """``config``: the subclass's constructor arguments besides ``dtype`` / ``device_id``.  ``_configure(**config)`` validates them
        and returns what ``create`` takes between the device id and the dtype."""
        import torch
        self._lib = _lib.load()
        _lib.require_gpu()
        self._destroy = getattr(self._lib, destroy)
        self._ctor = dict(config, dtype=dtype, device_id=device_id)     # what clone() constructs with
        args = self._configure(**config)
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_lib.DTYPES)}")
        self.dtype, self.device_id = dtype, int(device_id)
        self._dev = torch.device("cuda", self.device_id)
        h = C.c_void_p()
        _lib.check(getattr(self._lib, create)(self.device_id, *args, _lib.DTYPES[dtype], C.byref(h)))
        self._h = h
        self._state = None          # the float32 arrays clone() loads, for the engines that keep them

    def _configure(self, **config) -> tuple:
        return ()

    # ---- weights ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def missing_key(key: str) -> FramewrightHipError:
        return FramewrightHipError(_lib.FW_ERR_INVALID, f"state dict is missing {key}")

    def no_weights(self, who: str = "") -> FramewrightHipError:
        return FramewrightHipError(_lib.FW_ERR_INVALID, f"{type(self).__name__}{who}: no weights loaded")

    def load_tensors(self, shapes, state: Mapping[str, object], set_tensor, finalize) -> dict:
        """Every ``(key, shape)`` of ``shapes`` from ``state`` into the engine as contiguous float32, then ``finalize``.  Returns the
        arrays that went in, by key."""
        kept = {}
        for key, shape in shapes:
            if key not in state:
                raise self.missing_key(key)
            a = np.ascontiguousarray(to_numpy(state[key]), dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise FramewrightHipError(_lib.FW_ERR_INVALID, f"{key}: expected shape {shape}, got {a.shape}")
            _lib.check(set_tensor(self._h, key.encode(), C.c_void_p(a.ctypes.data), a.size))
            kept[key] = a
        _lib.check(finalize(self._h))
        return kept

    # ---- frame checks ----------------------------------------------------------------------------------------------------------------
    def check_frame_u8(self, t, who: str) -> None:
        import torch
        if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
            raise ValueError(f"{who} expects a contiguous uint8 CUDA tensor H x W x 3")
        if t.device != self._dev:
            raise ValueError(f"tensor is on {t.device}, engine on {self._dev}")

    def check_out(self, out, out_rgb_f32, shape) -> None:
        import torch
        for t, dt in ((out, torch.uint8), (out_rgb_f32, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != self._dev):
                raise ValueError("output tensor has the wrong dtype/shape/device")

    @staticmethod
    def check_host_frame_u8(a) -> np.ndarray:
        f = np.ascontiguousarray(a)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("expected an H x W x 3 uint8 BGR frame")
        return f

    # ---- lifetime --------------------------------------------------------------------------------------------------------------------
    def clone(self):
        """A second handle with the same weights and its own workspace, so that two forwards can be in flight on two streams."""
        if self._state is None:
            raise self.no_weights(".clone")
        e = type(self)(**self._ctor)
        e.load_state_dict(self._state)
        return e

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy(h)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class StreamPool:
    """Workers for independent forwards of one engine kind: worker 0 is the engine itself, the others are clones (their own
    workspaces), each with a ``torch.cuda.Stream`` of its own and a copy of ``extras`` (per-worker fields of the caller).  Workers
    are made when first asked for."""

    def __init__(self, engine, device, **extras):
        self.engine, self.device, self.extras, self.workers = engine, device, extras, []

    def take(self, k: int) -> list:
        """The first ``k`` workers."""
        import torch
        while len(self.workers) < k:
            eng = self.engine if not self.workers else self.engine.clone()
            self.workers.append({"engine": eng, "stream": torch.cuda.Stream(device=self.device), **self.extras})
        return self.workers[:k]

    def close(self) -> None:
        """Closes the clones; the engine stays its owner's."""
        for wk in self.workers[1:]:
            wk["engine"].close()
        self.workers = []

    def fan_out(self, items, call, k: int) -> list:
        """``call(worker_engine, item, out)`` for every item (a sequence of tensors), item i on worker i % k under that worker's
        stream, into an output buffer shaped like the item's first tensor.  Asynchronous on the caller's current stream: the workers
        start once it reaches this point, and it waits for all of them."""
        import torch
        items = [tuple(it) for it in items]
        workers = self.take(k)
        main = torch.cuda.current_stream(self.device)
        outs = _lib.empty_like_many([it[0] for it in items])     # one allocation: a hipMalloc per output would serialise the streams
        start = torch.cuda.Event()
        start.record(main)          # the inputs and the output buffers are ready once the caller's stream gets here
        for i, it in enumerate(items):
            wk = workers[i % k]
            if i < k:
                wk["stream"].wait_event(start)
            with torch.cuda.stream(wk["stream"]):
                call(wk["engine"], it, outs[i])
            for t in it + (outs[i],):
                t.record_stream(wk["stream"])
        for wk in workers:
            ev = torch.cuda.Event()
            ev.record(wk["stream"])
            main.wait_event(ev)
        return outs
