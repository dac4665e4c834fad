"""ctypes binding of libframewright_hip.so (C-ABI declared in include/framewright_hip.h).

The library is the product: if it is missing or does not load, every operator raises — there is no eager /
CPU fallback on this path.
"""
from __future__ import annotations

import ctypes as C
import re
import threading
from pathlib import Path
from typing import Optional

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "lib" / "libframewright_hip.so"
HEADER_PATH = PKG_DIR.parent / "include" / "framewright_hip.h"


class FramewrightHipError(RuntimeError):
    """Raised for every failing C-ABI call; ``code`` is the FW_ERR_* status."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class FramewrightOutOfMemory(FramewrightHipError):
    """FW_ERR_OOM — message contains "memory" so reference restorer.py:1746 retries with a smaller tile."""


_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "unsigned": C.c_uint, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
# HOST arrays that the callers hand over as typed ctypes arrays: the header cannot tell them from device pointers of the same type
_HOST_ARRAYS = {("fw_rrdbnet_profile_read", "total_ms"): C.POINTER(C.c_double),
                ("fw_rrdbnet_profile_read", "total_flops"): C.POINTER(C.c_double),
                ("fw_temporal_average_u8", "weights"): C.POINTER(C.c_float),
                ("fw_conv3x3_split_nhwc", "id_scale"): C.POINTER(C.c_float)}


def _read_header(text: str, host_arrays: dict = _HOST_ARRAYS) -> list:
    """``(name, restype, argtypes)`` of every prototype of the header ``text``, in its order.  Scalars map to their ctypes scalar,
    ``const char*`` to ``c_char_p``, ``int*`` / ``long*`` to ``POINTER`` of it, ``T**`` (T not void) to ``POINTER(c_void_p)``, every
    other pointer to ``c_void_p``; ``host_arrays`` types single parameters by (function, parameter name).  Whatever does not fit
    raises: nothing is guessed."""
    def fail(entry, why):
        raise FramewrightHipError(FW_ERR_INTERNAL, f"{HEADER_PATH.name}: {entry}: {why}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\{[^{}]*\}", " ", text)      # the members of typedef struct fw_hdr_params { ... }
    statements = [" ".join(s.split()) for s in text.replace("}", " ").split(";")]
    typedefs = {s.split()[-1] for s in statements if s.startswith("typedef ")}

    def ctype(entry, decl, named):
        toks = decl.replace("*", " * ").split()
        words, stars = [t for t in toks if t not in ("*", "const")], toks.count("*")
        if len(words) != 1 + named or not all(w.isidentifier() for w in words) or toks[-1] != words[-1] and named:
            fail(entry, f"cannot split '{decl.strip()}'")
        base = words[0]
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        known = base in _SCALARS or base in typedefs or base in ("void", "char") or re.fullmatch(r"u?int(8|16|32|64)_t", base)
        if not known or not 1 <= stars <= 2:
            fail(entry, f"unknown type in '{decl.strip()}'")
        if stars == 2:
            return C.c_void_p if base == "void" else C.POINTER(C.c_void_p)
        if base == "char" and "const" in toks:
            return C.c_char_p
        return C.POINTER(_SCALARS[base]) if base in ("int", "long") else C.c_void_p

    out, seen = [], set()
    for s in statements:
        if not s or s.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", s)
        if not m:
            fail(s[:60], "not a prototype")
        ret, name, params = m.groups()
        argtypes = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            t, key = ctype(name, p, True), (name, p.replace("*", " ").split()[-1])
            seen.add(key)
            argtypes.append(host_arrays.get(key, t))
        out.append((name, ctype(name, ret, False), argtypes))
    for fn, param in sorted(host_arrays.keys() - seen):
        fail(fn, f"the host-array table names the parameter '{param}', which the header does not have")
    return out


if not HEADER_PATH.exists():     # code 4 is FW_ERR_INTERNAL, which only the header that is missing names
    raise FramewrightHipError(4, f"{HEADER_PATH} not found: the C-ABI is read from it; there is no second copy")
_HEADER = HEADER_PATH.read_text()
# FW_OK .. FW_ERR_INTERNAL, FW_HOST / FW_DEVICE, FW_DTYPE_*, FW_NAF_PATH_*, FW_REST_PATH_*: the header's `#define FW_<NAME> <integer>` lines
globals().update({n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FW_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*(?:/[/*].*)?$",
                                                       _HEADER, re.M)})
_SIGNATURES = _read_header(_HEADER)
EXPORTS = [name for name, _, _ in _SIGNATURES]      # every symbol include/framewright_hip.h declares, in its order
DTYPES = {"bf16": FW_DTYPE_BF16, "bfloat16": FW_DTYPE_BF16, "f16": FW_DTYPE_F16, "fp16": FW_DTYPE_F16,
          "float16": FW_DTYPE_F16, "half": FW_DTYPE_F16}

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises FramewrightHipError when it is absent — build it with
    ``python __graft_entry__.py build`` (hipcc, gfx950)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            raise FramewrightHipError(FW_ERR_INTERNAL,
                                      f"{LIB_PATH} not found: the HIP extension is not built "
                                      "(run `python __graft_entry__.py build`); there is no CPU fallback")
        # torch bundles its own libamdhip64.so.7; importing it first makes both share ONE HIP runtime, so
        # torch.cuda device pointers and streams can be handed to the library.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is plumbing, the library also works stand-alone
            pass
        try:
            lib = C.CDLL(str(LIB_PATH))
        except OSError as e:
            raise FramewrightHipError(FW_ERR_INTERNAL, f"cannot load {LIB_PATH}: {e}") from e
        for name, restype, argtypes in _SIGNATURES:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def check(status: int) -> None:
    if status == FW_OK:
        return
    msg = load().fw_last_error().decode("utf-8", "replace")
    if status == FW_ERR_OOM:
        raise FramewrightOutOfMemory(status, msg)
    raise FramewrightHipError(status, msg)


def require_gpu() -> int:
    """Number of visible devices; raises when there is none (the product path never runs on the CPU)."""
    n = load().fw_device_count()
    if n <= 0:
        raise FramewrightHipError(FW_ERR_HIP, "no HIP device visible: framewright_amd has no CPU fallback")
    return n


def on_tensor_device(fn):
    """Decorator for device-level entry methods: run the body with the CUDA device of the first tensor argument current, so
    that ``torch.cuda.current_stream()``, scratch allocations and the library's block-level launchers (which launch on the
    current device: zero pages, default streams) all refer to the device that owns the buffers - an engine created with
    ``device_id != 0`` must not depend on the caller's current device."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        import torch
        dev = None
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                dev = a.device
                break
            if isinstance(a, (list, tuple)):
                t = next((x for x in a if isinstance(x, torch.Tensor) and x.is_cuda), None)   # any element: [None, tensor, ...] is a rank's block
                if t is not None:
                    dev = t.device
                    break
        if dev is None and args:
            # no CUDA tensor among the arguments (numpy frames, None placeholders): the owner says where it lives
            dev = owner_device(args[0])
        if dev is None:
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def owner_device(obj):
    """The CUDA device an engine, a stage or a driver lives on, or ``None``: an engine's ``_dev`` / ``device_id``, a driver's
    ``config.gpu_id``, a stage's ``gpu_id``."""
    import torch
    cand = getattr(obj, "_dev", None)
    if cand is None:
        cand = getattr(obj, "device_id", None)
    if cand is None:
        cand = getattr(getattr(obj, "config", None), "gpu_id", None)
    if cand is None:
        cand = getattr(obj, "gpu_id", None)
    if isinstance(cand, torch.device):
        return cand if cand.type == "cuda" else None
    if isinstance(cand, int) and not isinstance(cand, bool) and cand >= 0 and torch.cuda.is_available():
        return torch.device("cuda", cand)
    return None


def ptr(t) -> Optional[C.c_void_p]:
    """The device address of a tensor as a pointer argument of the C-ABI; ``None`` (an optional buffer left out) stays ``None``."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ptr_table(tensors) -> C.Array:
    """A host table of the tensors' device addresses (a ``const void* const*`` argument), in the order given."""
    tensors = list(tensors)
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def stream_ptr(dev) -> C.c_void_p:
    """torch's current stream on ``dev`` as the stream argument of the C-ABI."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def empty_like_many(frames) -> list:
    """Output buffers for a batch of frames: ONE allocation cut into views when the frames agree in shape (the usual clip), else one
    per frame.  A hipMalloc is a device-wide synchronisation: a hundred of them in front of a hundred forwards that are meant to
    overlap on side streams serialise those streams (measured on the `rife` bench line: 1.21 - 1.40 ms per 1080p pair with one
    allocation per mid frame on a cold allocator, 0.83 with the buffers in place - profiles/r03_ab/rife_output_buffers.txt)."""
    import torch
    frames = list(frames)
    if len(frames) > 1 and all(f.shape == frames[0].shape and f.dtype == frames[0].dtype and f.device == frames[0].device for f in frames):
        buf = torch.empty((len(frames),) + tuple(frames[0].shape), dtype=frames[0].dtype, device=frames[0].device)
        return list(buf.unbind(0))
    return [torch.empty_like(f) for f in frames]


def side_streams(env_name: str, default: int) -> int:
    """How many forwards of one engine kind may be in flight on their own streams (with engine clones).  ``env_name`` overrides.
    Measured on MI355X / ROCm 7.2: up to three worker streams beside the caller's overlap as intended; with a fourth the work
    serialises (RIFE) or runs 1.7x slower than one stream (NAFNet) - the process's hardware queues are shared by then - so the
    defaults stay below that, and a process that is one rank of several (RCCL brings streams of its own) runs one at a time."""
    import os
    v = os.environ.get(env_name)
    if v is not None:
        return max(1, int(v))
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return 1
    except Exception:  # noqa: BLE001 - no torch.distributed: a single process
        pass
    return default
