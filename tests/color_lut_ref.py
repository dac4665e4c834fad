"""The contract of the device colour grade (csrc/color_lut.hip): a NumPy restatement, with every type spelled out, of what the
reference's `LUTManager.apply_to_image_fast` (src/framewright/integration/lut.py) computes for a uint8 / uint16 three-channel frame,
every operation rounded on its own.  The sample is normalised and scaled in float32; the fraction is `scaled - indices_low`, a
float32 array minus an int32 one, which NumPy promotes to FLOAT64, and so every lerp, the clip and the final scale are float64.
tests/test_color_lut_ref_host.py holds it byte for byte against outputs recorded from the reference
itself (tests/golden/color_lut_reference.*, written by tools/gen_color_lut_golden.py); on the GPU machine, where the reference does
not exist, the device is compared with this file.

`apply_lut3d(..., lerp32=True)`, `(..., reciprocal=True)` and `(..., fused=True)` are the wrong variants a hasty kernel, an
optimiser or a compiler would produce: the lerps in float32 (what the code reads like), the division by 255 / 65535 replaced by a
multiplication with (size - 1) / maxv, and every lerp's sum contracted into one FMA (emulated in extended precision: the product
b f keeps 64 bits where an FMA keeps all).  The tests show that the first two are REJECTED on the recorded hard colours, so a
device that took either shortcut fails; the generator records how many colours the third changes.
"""
from __future__ import annotations

import hashlib

import numpy as np

F32 = np.float32


def _lerp(a, b, f, fused):
    if not fused:
        return a * (1 - f) + b * f
    # fma(b, f, a * (1 - f)): the product b f carried wider than float64, one rounding of the sum to float64
    p = (a * (1 - f)).astype(np.longdouble)
    return (b.astype(np.longdouble) * f.astype(np.longdouble) + p).astype(np.float64)


def apply_lut3d(image: np.ndarray, table: np.ndarray, bgr: bool = True, fused: bool = False, reciprocal: bool = False,
                lerp32: bool = False) -> np.ndarray:
    """image: [...] x 3 uint8 or uint16; table: size^3 x 3 float32 indexed [r][g][b].  bgr: channel 0 of a pixel is blue."""
    table = np.asarray(table)
    assert table.dtype == F32 and table.ndim == 4 and image.dtype in (np.uint8, np.uint16) and image.shape[-1] == 3
    size = table.shape[0]
    maxv = F32(255.0 if image.dtype == np.uint8 else 65535.0)
    px = image.reshape(-1, 3)
    if reciprocal:
        scaled = px.astype(F32) * (F32(size - 1) / maxv)
    else:
        scaled = (px.astype(F32) / maxv) * F32(size - 1)
    lo = np.floor(scaled).astype(np.int32)
    hi = np.minimum(lo + 1, size - 1)
    fr = scaled.astype(np.float64) - lo.astype(np.float64)          # float32 - int32 -> float64 in NumPy; exact
    wide = F32 if lerp32 else np.float64
    fr, table = fr.astype(wide), table.astype(wide)
    lo = np.clip(lo, 0, size - 1)
    hi = np.clip(hi, 0, size - 1)
    ri, gi, bi = (2, 1, 0) if bgr else (0, 1, 2)
    r0, g0, b0, r1, g1, b1 = lo[:, ri], lo[:, gi], lo[:, bi], hi[:, ri], hi[:, gi], hi[:, bi]
    rf, gf, bf = fr[:, ri:ri + 1], fr[:, gi:gi + 1], fr[:, bi:bi + 1]
    c00 = _lerp(table[r0, g0, b0], table[r1, g0, b0], rf, fused)
    c01 = _lerp(table[r0, g0, b1], table[r1, g0, b1], rf, fused)
    c10 = _lerp(table[r0, g1, b0], table[r1, g1, b0], rf, fused)
    c11 = _lerp(table[r0, g1, b1], table[r1, g1, b1], rf, fused)
    c0 = _lerp(c00, c10, gf, fused)
    c1 = _lerp(c01, c11, gf, fused)
    res = _lerp(c0, c1, bf, fused)
    if bgr:
        res = res[:, ::-1]
    return (np.clip(res, wide(0), wide(1)) * wide(maxv)).astype(image.dtype).reshape(image.shape)


def apply_table3(image: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """image: [...] x 3 uint8; tables: 3 x 256 uint8, one per stored channel."""
    out = np.empty_like(image)
    for c in range(3):
        out[..., c] = tables[c][image[..., c]]
    return out


# ---- the images both the generator tool and the tests form --------------------------------------------------------------------------
IMAGE_SIZES = [(1, 1), (3, 5), (7, 13), (33, 131), (64, 64), (135, 240)]
TABLE_SIZES = [2, 5, 17, 18, 33, 65]          # 17 | 18: the last table the kernel holds in LDS and the first it does not
CUBE_SIDE = 4096


def test_image(h: int, w: int, dtype, n: int = 1, seed: int = 0) -> np.ndarray:
    """n x h x w x 3 seeded noise with the extremes present: 0 and the maximum reach the last plane of the table (hi == lo)."""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed + (1 if np.dtype(dtype) == np.uint16 else 0))
    top = 255 if np.dtype(dtype) == np.uint8 else 65535
    a = rng.integers(0, top + 1, size=(n, h, w, 3), dtype=np.int64)
    edge = rng.random((n, h, w, 3))
    a[edge < 0.05] = 0
    a[edge > 0.95] = top
    return a.astype(dtype)


test_image.__test__ = False


def full_range_u16() -> np.ndarray:
    """256 x 256 x 3 uint16: every 16-bit value once in every channel, the channels permuted apart."""
    rng = np.random.default_rng(65536)
    return np.stack([rng.permutation(65536) for _ in range(3)], axis=-1).astype(np.uint16).reshape(256, 256, 3)


def cube_rows(y0: int, rows: int) -> np.ndarray:
    """Rows y0 .. y0 + rows of the 4096 x 4096 BGR image that holds every 8-bit colour once: pixel i = 4096 y + x has
    b = i & 255, g = (i >> 8) & 255, r = i >> 16."""
    i = np.arange(y0 * CUBE_SIDE, (y0 + rows) * CUBE_SIDE, dtype=np.int64).reshape(rows, CUBE_SIDE)
    return np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8)


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cube_digest(fn, strip: int = 256) -> str:
    """sha256 of fn(image) over the whole cube image, formed strip by strip (the operation is per pixel)."""
    h = hashlib.sha256()
    for y0 in range(0, CUBE_SIDE, strip):
        h.update(np.ascontiguousarray(fn(cube_rows(y0, strip))).tobytes())
    return h.hexdigest()
