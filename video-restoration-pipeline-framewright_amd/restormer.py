"""Restormer on MI355X — the reference's DEFAULT TAP model (`TAPModel.RESTORMER`, tap_denoise.py:110, `_load_restormer`
:299-333).  Host sequencing over the C-ABI building blocks of csrc/restormer_ops.hip, the pointwise MFMA GEMM and the 3x3
MFMA conv kernel; architecture per SURVEY.md §A.4 (the class itself is third-party and absent: parity unpinned, oracle
oracle/restormer_ref.py).

Layout: fp32 NHWC residual stream [pixels][pad32(dim)] (dim 48 is carried with stride 64, pad channels stay zero);
LayerNorm writes operand-typed tensors padded to 32 channels for the GEMMs; q / k / v live in one typed buffer at channel
offsets 0 / dp / 2*dp; the GDFN halves x1 / x2 at 0 / hp (hidden 127 -> 128 etc.), with the 1x1 and depthwise weights
re-laid to match on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Sequence, Tuple

import numpy as np

from . import _lib
from ._engine import Engine, unwrap_state

RESTORMER_ARGS = dict(dim=48, num_blocks=(4, 6, 6, 8), num_refinement_blocks=4, heads=(1, 2, 4, 8), ffn_expansion_factor=2.66)


def _pad(n: int, m: int = 32) -> int:
    return (n + m - 1) // m * m


def _stages(dim, num_blocks, num_refinement_blocks, heads):
    """(state-dict prefix, blocks, channel count, heads) in forward order."""
    return [("encoder_level1", num_blocks[0], dim, heads[0]), ("encoder_level2", num_blocks[1], 2 * dim, heads[1]),
            ("encoder_level3", num_blocks[2], 4 * dim, heads[2]), ("latent", num_blocks[3], 8 * dim, heads[3]),
            ("decoder_level3", num_blocks[2], 4 * dim, heads[2]), ("decoder_level2", num_blocks[1], 2 * dim, heads[1]),
            ("decoder_level1", num_blocks[0], 2 * dim, heads[0]), ("refinement", num_refinement_blocks, 2 * dim, heads[0])]


def restormer_tensor_shapes(dim=48, num_blocks=(4, 6, 6, 8), num_refinement_blocks=4, heads=(1, 2, 4, 8),
                            ffn_expansion_factor=2.66) -> List[Tuple[str, Tuple[int, ...]]]:
    out: List[Tuple[str, Tuple[int, ...]]] = [("patch_embed.proj.weight", (dim, 3, 3, 3))]
    for name, n, c, h in _stages(dim, num_blocks, num_refinement_blocks, heads):
        hid = int(c * ffn_expansion_factor)
        for i in range(n):
            p = f"{name}.{i}."
            out += [(p + "norm1.body.weight", (c,)), (p + "norm1.body.bias", (c,)), (p + "attn.temperature", (h, 1, 1)),
                    (p + "attn.qkv.weight", (3 * c, c, 1, 1)), (p + "attn.qkv_dwconv.weight", (3 * c, 1, 3, 3)),
                    (p + "attn.project_out.weight", (c, c, 1, 1)), (p + "norm2.body.weight", (c,)), (p + "norm2.body.bias", (c,)),
                    (p + "ffn.project_in.weight", (2 * hid, c, 1, 1)), (p + "ffn.dwconv.weight", (2 * hid, 1, 3, 3)),
                    (p + "ffn.project_out.weight", (c, hid, 1, 1))]
    out += [("down1_2.body.0.weight", (dim // 2, dim, 3, 3)), ("down2_3.body.0.weight", (dim, 2 * dim, 3, 3)),
            ("down3_4.body.0.weight", (2 * dim, 4 * dim, 3, 3)), ("up4_3.body.0.weight", (16 * dim, 8 * dim, 3, 3)),
            ("reduce_chan_level3.weight", (4 * dim, 8 * dim, 1, 1)), ("up3_2.body.0.weight", (8 * dim, 4 * dim, 3, 3)),
            ("reduce_chan_level2.weight", (2 * dim, 4 * dim, 1, 1)), ("up2_1.body.0.weight", (4 * dim, 2 * dim, 3, 3)),
            ("output.weight", (3, 2 * dim, 3, 3))]
    return out


def synthetic_restormer_state(seed: int = 0, **args):
    """Seeded weights with the published keys/shapes, scaled so that the residual stream stays O(1)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in restormer_tensor_shapes(**args):
        if key.endswith("norm1.body.weight") or key.endswith("norm2.body.weight"):
            sd[key] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif key.endswith(".bias"):
            sd[key] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
        elif key.endswith("temperature"):
            sd[key] = (1.0 + 0.5 * rng.random(shape)).astype(np.float32)
        elif "dwconv" in key:
            sd[key] = (rng.standard_normal(shape) / 3.0).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 0.1 if key == "output.weight" else 0.5 if "project_out" in key else 1.0
            sd[key] = (rng.standard_normal(shape) * gain / np.sqrt(fan_in)).astype(np.float32)
    return sd


class RestormerEngine(Engine):
    """Restormer resident on one GPU: thin owner of an ``fw_restormer*`` (csrc/restormer.hip - weight re-layout, workspace arena
    and the ~800 launches of a forward live behind the C-ABI, one mutex per handle).  ``denoise_device`` mirrors NAFNetEngine
    (uint8 BGR in, uint8 BGR out)."""

    def __init__(self, dim: int = 48, num_blocks: Sequence[int] = (4, 6, 6, 8), num_refinement_blocks: int = 4,
                 heads: Sequence[int] = (1, 2, 4, 8), ffn_expansion_factor: float = 2.66, dtype: str = "f16", device_id: int = 0):
        super().__init__("fw_restormer_create", "fw_restormer_destroy", dtype, device_id, dim=dim, num_blocks=num_blocks,
                         num_refinement_blocks=num_refinement_blocks, heads=heads, ffn_expansion_factor=ffn_expansion_factor)

    def _configure(self, dim, num_blocks, num_refinement_blocks, heads, ffn_expansion_factor):
        if dim != 48:
            raise ValueError("RestormerEngine: dim must be 48 (per-head width 48 / 96 is what the attention kernels take)")
        self.args = dict(dim=int(dim), num_blocks=tuple(num_blocks), num_refinement_blocks=int(num_refinement_blocks),
                         heads=tuple(heads), ffn_expansion_factor=float(ffn_expansion_factor))
        for (_, _, c, h) in _stages(dim, num_blocks, num_refinement_blocks, heads):
            if c % h or c // h not in (48, 96):
                raise ValueError("RestormerEngine: channels per head must be 48 or 96")
        return (int(dim), (C.c_int * 4)(*self.args["num_blocks"]), int(num_refinement_blocks), (C.c_int * 4)(*self.args["heads"]),
                float(ffn_expansion_factor))

    # ---- weights ----------------------------------------------------------------------------------------------------
    def load_state_dict(self, state: Mapping[str, object]) -> None:
        self._state = self.load_tensors(restormer_tensor_shapes(**self.args), unwrap_state(state, ("params", "state_dict")),
                                        self._lib.fw_restormer_set_tensor, self._lib.fw_restormer_finalize)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def denoise_device(self, frame, out=None, out_rgb_f32=None):
        """torch.uint8 CUDA tensor H x W x 3 (H, W multiples of 8, as the network's three PixelUnshuffles require) -> same
        shape; asynchronous on torch's current stream of the engine's device."""
        import torch
        if self._state is None:
            raise self.no_weights()
        self.check_frame_u8(frame, "denoise_device")
        H, Wd = int(frame.shape[0]), int(frame.shape[1])
        if H % 8 or Wd % 8:
            raise ValueError(f"Restormer needs frame sizes divisible by 8, got {Wd}x{H}")
        if out is None and out_rgb_f32 is None:
            out = torch.empty_like(frame)
        _lib.check(self._lib.fw_restormer_denoise_u8(self._h, _lib.ptr(frame), _lib.FW_DEVICE, H, Wd, _lib.ptr(out), _lib.FW_DEVICE,
                                                     _lib.ptr(out_rgb_f32), _lib.stream_ptr(self._dev)))
        return out if out is not None else out_rgb_f32

    def denoise(self, frame_bgr: np.ndarray) -> np.ndarray:
        f = self.check_host_frame_u8(frame_bgr)
        if f.shape[0] % 8 or f.shape[1] % 8:
            raise ValueError(f"Restormer needs frame sizes divisible by 8, got {f.shape[1]}x{f.shape[0]}")
        if self._state is None:
            raise self.no_weights()
        out = np.empty_like(f)
        _lib.check(self._lib.fw_restormer_denoise_u8(self._h, C.c_void_p(f.ctypes.data), _lib.FW_HOST, f.shape[0], f.shape[1],
                                                     C.c_void_p(out.ctypes.data), _lib.FW_HOST, None, None))
        return out

    # ---- single steps of a forward on the caller's buffers (tests, tools) ----
    STEPS = ("down1_2", "down2_3", "down3_4", "up4_3", "up3_2", "up2_1", "output")

    def _block_shape(self, key: str):
        """(channels, heads) of the block ``key`` names ("encoder_level1.0.", "latent.0."), or None."""
        for name, n, c, heads in _stages(self.args["dim"], self.args["num_blocks"], self.args["num_refinement_blocks"], self.args["heads"]):
            if key.startswith(name + ".") and key[len(name) + 1:-1].isdigit() and key.endswith(".") and int(key[len(name) + 1:-1]) < n:
                return c, heads
        return None

    @staticmethod
    def _check_stream(t, what, shape=None):
        import torch
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"{what} expects a contiguous float32 CUDA tensor H x W x channels" + (f" of shape {shape}" if shape else ""))

    @_lib.on_tensor_device
    def run_block(self, stream_f32, key: str, attn_out=None):
        """One transformer block (``key`` as in the state dict: "encoder_level1.0.", "latent.0.") in place on a contiguous float32
        CUDA tensor H x W x pad32(c) whose lanes behind c hold zeros, dispatched as in a forward; ``attn_out`` (float32 CUDA,
        heads x c/heads x c/heads) receives the softmaxed attention matrix."""
        import torch
        self._check_stream(stream_f32, "run_block")
        shape = self._block_shape(key)
        if shape is None or int(stream_f32.shape[2]) != _pad(shape[0]):
            raise ValueError(f"run_block: {key!r} does not name a block of a {int(stream_f32.shape[2])}-lane stream")
        c, heads = shape
        if attn_out is not None and (attn_out.dtype != torch.float32 or not attn_out.is_cuda or not attn_out.is_contiguous() or
                                     attn_out.numel() < c * (c // heads)):
            raise ValueError("attn_out must be a contiguous float32 CUDA tensor heads x c/heads x c/heads")
        _lib.check(self._lib.fw_restormer_run_block(self._h, key.encode(), _lib.ptr(stream_f32), int(stream_f32.shape[0]),
                                                    int(stream_f32.shape[1]), _lib.ptr(attn_out), _lib.stream_ptr(stream_f32.device)))
        return stream_f32

    def block_paths(self, key: str) -> int:
        """FW_REST_PATH_* bits of the kernels that block dispatches to."""
        flags = C.c_int(0)
        _lib.check(self._lib.fw_restormer_block_paths(self._h, key.encode(), C.byref(flags)))
        return flags.value

    def step_shapes(self, step: str, h: int, w: int):
        """(src, skip or None, dst) shapes of ``step`` on a source of h x w pixels."""
        d = self.args["dim"]
        if step not in self.STEPS:
            raise ValueError(f"run_step: unknown step {step!r}")
        i = self.STEPS.index(step)
        if i < 3:
            c = d << i
            return (h, w, _pad(c)), None, (h // 2, w // 2, _pad(2 * c))
        if i < 6:
            c = d << (6 - i)                       # channels of the source: 8d, 4d, 2d
            return (h, w, _pad(c)), (2 * h, 2 * w, _pad(c // 2)), (2 * h, 2 * w, _pad(c // 2 if i < 5 else c))
        return (h, w, _pad(2 * d)), None, (h, w, 64)

    @_lib.on_tensor_device
    def run_step(self, step: str, src_f32, dst_f32, skip_f32=None):
        """What a forward runs between two stages (``STEPS``; shapes: ``step_shapes``) from src into dst, contiguous float32 CUDA
        tensors; the up steps also take the encoder's skip stream."""
        h, w = int(src_f32.shape[0]), int(src_f32.shape[1])
        src, skip, dst = self.step_shapes(step, h, w)
        if skip is None and step != "output" and (h | w) & 1:
            raise ValueError("run_step: a down step needs even sides")
        self._check_stream(src_f32, "run_step", src)
        self._check_stream(dst_f32, "run_step", dst)
        if (skip is None) != (skip_f32 is None):
            raise ValueError(f"run_step: {step} {'needs' if skip else 'takes no'} skip stream")
        if skip is not None:
            self._check_stream(skip_f32, "run_step", skip)
        _lib.check(self._lib.fw_restormer_run_step(self._h, step.encode(), _lib.ptr(src_f32), _lib.ptr(skip_f32), h, w, _lib.ptr(dst_f32),
                                                   _lib.stream_ptr(src_f32.device)))
        return dst_f32

    def close(self) -> None:
        super().close()
        self._state = None
