"""TEST INFRASTRUCTURE ONLY: sentinel-filled device buffers with a guard on both sides, for the C-ABI kernel tests (the scheme of
tests/test_conv_split_wino_gpu.py).  ``take()`` downloads the body and asserts that both guards still hold the sentinel; what the body
keeps of the sentinel is the test's to assert (``untouched``)."""
import ctypes as C

import numpy as np
import torch

GUARD = 4096                       # guard elements on both sides
SENT = {"u16": 0x7E5A,             # a NaN pattern of f16 and bf16
        "f32": 0x7FC5A5A5,         # a NaN pattern of fp32
        "u8": 0xA5}
_TORCH = {"u16": torch.int16, "f32": torch.int32, "u8": torch.uint8}
_NP = {"u16": np.uint16, "f32": np.uint32, "u8": np.uint8}

F16, BF16 = "f16", "bf16"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}


def dtype_id(dtype: str) -> int:
    from framewright_amd import _lib
    return _lib.FW_DTYPE_F16 if dtype == "f16" else _lib.FW_DTYPE_BF16


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, byte_offset: int = 0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def dev(a: np.ndarray):
    """A host array on the device, bit for bit (uint16 / uint32 travel as their signed twins)."""
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).cuda()


class Guarded:
    def __init__(self, n: int, kind: str):
        self.n, self.kind = int(n), kind
        sent = SENT[kind]
        if kind != "u8":
            sent = int(np.array([sent], _NP[kind]).view(np.int16 if kind == "u16" else np.int32)[0])
        self.t = torch.full((GUARD + self.n + GUARD,), sent, dtype=_TORCH[kind], device="cuda")
        self.itemsize = self.t.element_size()

    def ptr(self, elem_offset: int = 0):
        return C.c_void_p(self.t.data_ptr() + (GUARD + elem_offset) * self.itemsize)

    def fill(self, a: np.ndarray, elem_offset: int = 0):
        """Write host values (bit patterns) into the body."""
        flat = dev(np.ascontiguousarray(a).reshape(-1).view(_NP[self.kind])).view(_TORCH[self.kind])
        self.t[GUARD + elem_offset:GUARD + elem_offset + flat.numel()] = flat

    def body(self):
        """The body as a device tensor of the raw integer type (a view)."""
        return self.t[GUARD:GUARD + self.n]

    def take(self) -> np.ndarray:
        a = self.t.cpu().numpy().view(_NP[self.kind])
        for name, g in (("front", a[:GUARD]), ("back", a[GUARD + self.n:])):
            bad = np.flatnonzero(g != SENT[self.kind])
            assert bad.size == 0, f"{bad.size} elements of the {name} guard were written, first at {bad[:4]}"
        return a[GUARD:GUARD + self.n].copy()


def untouched(a: np.ndarray, kind: str) -> bool:
    return bool((a == SENT[kind]).all())


def f32(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)
