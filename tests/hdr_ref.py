"""TEST INFRASTRUCTURE ONLY (imported by tests/ and tools/ and nothing on the product path).

numpy restatement of the frame path of the reference's SDR to HDR conversion, `HDRConverter.convert_frame`
(src/framewright/processors/hdr_conversion.py): gamma removal, the Rec.709 -> BT.2020 matrix, the luminance tone map, local contrast
(CLAHE on Lab L, blended half and half), the HSV saturation boost, the highlight flag and the PQ / HLG transfer to 16 bits.  This file
is the contract csrc/hdr.hip is held to, byte for byte, and tools/gen_hdr_golden.py holds it against the reference's own code.

The reference's numpy steps are restated operation for operation in float32, each rounded once.  Its four cv2 calls are restated from
the published formulas, because OpenCV is not installed where this is built: `bgr2lab` / `lab2bgr` are tests/flicker_ref.py's
fixed-point gamma Lab, `clahe`, `add_weighted`, `bgr2hsv` (the 8-bit integer form, hue 0 .. 179) and `hsv2bgr` (float32) are below.
cv2's own bytes stay UNPINNED, as everywhere in this project: THIS RESTATEMENT IS THE DEFINITION of those steps.

Two things are pinned by the golden rather than by a formula.  `np.dot(rgb, M.T)` in float32 is the BLAS's order; on the machine the
golden was recorded on it is one rounded product and two fused multiply-adds per output (`to_bt2020`), not three rounded products.
And every table built with a transcendental numpy call (`build_tables`: gamma, the PQ / HLG tail, the clipped-flag thresholds) may
differ in a last bit between SIMD `pow` variants, so `convert_frame` takes recorded tables.

When a quantising step ran (local contrast on, or |saturation_boost - 1| > 0.01; both are defaults) the frame in front of the
transfer function is bytes / 255, optionally times 0.95 where the highlight flag is set, so the transfer and the 16-bit quantisation
are a 2 x 256 table.  With both steps off the transfer runs per pixel in float32 (`transfer_and_quantise` on a float plane).
"""
import numpy as np

import flicker_ref as fr

f32 = np.float32

M_709_2020 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]], dtype=np.float32)
PQ_FORMATS = ("hdr10", "hdr10plus", "dolby_vision")
RATIONAL_CURVES = ("reinhard", "aces", "hable")


def _name(v) -> str:
    return v.value if hasattr(v, "value") else str(v).lower()


def uses_matrix(config) -> bool:
    return _name(config.color_space) in ("bt2020", "p3")           # the reference gives P3 the BT.2020 matrix


def saturation_on(config) -> bool:
    return abs(config.saturation_boost - 1.0) > 0.01


def quantised(config) -> bool:
    return bool(config.enable_local_contrast) or saturation_on(config)


# ---- the transfer functions and the tables ------------------------------------------------------------------------------------------
def pq_transfer(frame: np.ndarray, peak_brightness: int) -> np.ndarray:
    m1 = 2610.0 / 16384.0
    m2 = 2523.0 / 4096.0 * 128.0
    c1 = 3424.0 / 4096.0
    c2 = 2413.0 / 4096.0 * 32.0
    c3 = 2392.0 / 4096.0 * 32.0
    L = np.clip(frame, 0, 1) * (peak_brightness / 10000.0)
    Lm1 = np.power(L, m1)
    pq = np.power((c1 + c2 * Lm1) / (1.0 + c3 * Lm1), m2)
    return np.clip(pq, 0, 1)


def hlg_transfer(frame: np.ndarray) -> np.ndarray:
    a, b, c = 0.17883277, 0.28466892, 0.55991073
    E = np.clip(frame, 0, 1)
    with np.errstate(all="ignore"):                                  # the log branch is evaluated for every E, also where it is negative
        E_prime = np.where(E <= 1.0 / 12.0, np.sqrt(3.0 * E), a * np.log(12.0 * E - b) + c)
    return np.clip(E_prime, 0, 1)


def transfer(frame: np.ndarray, config) -> np.ndarray:
    if _name(config.target_format) in PQ_FORMATS:
        return pq_transfer(frame, config.peak_brightness)
    return hlg_transfer(frame)


def quantise16(x: np.ndarray) -> np.ndarray:
    return np.clip(x * 65535.0, 0, 65535).astype(np.uint16)


def first_true(mask: np.ndarray) -> int:
    """The first code of a monotone flag table (its length when none is set)."""
    idx = np.flatnonzero(mask)
    assert idx.size == 0 or mask[idx[0]:].all()
    return int(idx[0]) if idx.size else int(mask.size)


def build_tables(config) -> dict:
    """Every table that a transcendental numpy call or a float comparison goes into, with the reference's own expressions:
    gamma8 / gamma16 float32 [256] / [65536], tail uint16 [2][256] (row 1: the highlight-reduced value), clip8 / clip16 the first
    code whose normalised value exceeds 0.98."""
    x8 = np.arange(256).astype(np.uint8).astype(f32) / 255.0
    x16 = np.arange(65536).astype(np.uint16).astype(f32) / 65535.0
    return {"gamma8": np.power(np.clip(x8, 0.0, 1.0), 2.2), "gamma16": np.power(np.clip(x16, 0.0, 1.0), 2.2),
            "tail": quantise16(transfer(np.stack([x8, x8 * 0.95]), config)),
            "clip8": first_true(x8 > 0.98), "clip16": first_true(x16 > 0.98)}


# ---- steps 1 - 3: float32 planes --------------------------------------------------------------------------------------------------------
def linearize(frame: np.ndarray, tables: dict) -> np.ndarray:
    """power(clip(frame / maxv, 0, 1), 2.2): a function of the code, so a table."""
    assert frame.dtype in (np.uint8, np.uint16)
    return tables["gamma8" if frame.dtype == np.uint8 else "gamma16"][frame]


def fma32(a, b, c) -> np.ndarray:
    """float32 fma(a, b, c), exactly: the product is exact in float64, the float64 sum is rounded to odd with the error of the
    addition (TwoSum), and a value rounded to odd at 53 bits rounds to 24 bits as the exact value does."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    toward = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    even = (s.view(np.int64) & 1) == 0
    return np.where((err != 0) & even, toward, s).astype(f32)


def to_bt2020(lin: np.ndarray) -> np.ndarray:
    """`np.dot(rgb, M.T)` on the BGR plane: out_i = fma(M[i][2], b, fma(M[i][1], g, round(M[i][0] * r)))."""
    b, g, r = lin[..., 0], lin[..., 1], lin[..., 2]
    rows = [fma32(M_709_2020[i][2], b, fma32(M_709_2020[i][1], g, M_709_2020[i][0] * r)) for i in range(3)]
    return np.stack(rows[::-1], axis=-1)


def luminance(frame: np.ndarray) -> np.ndarray:
    lum = 0.0722 * frame[:, :, 0] + 0.7152 * frame[:, :, 1] + 0.2126 * frame[:, :, 2]
    return np.clip(lum, 0.0001, None)


def _hable(x):
    A, B, C, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F


def curve(lum: np.ndarray, config, exp=np.exp) -> np.ndarray:
    """lum_hdr of the clipped float32 luminance.  Python scalars enter float32 arithmetic as float32, every operation rounds once."""
    peak_scale = config.peak_brightness / 100.0
    tm = _name(config.tone_mapping)
    if tm == "reinhard":
        return lum * (1 + lum / (peak_scale ** 2)) / (1 + lum)
    if tm == "aces":
        a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
        ls = lum * peak_scale
        return np.clip((ls * (a * ls + b)) / (ls * (c * ls + d) + e), 0, 1)
    if tm == "hable":
        return _hable(lum * peak_scale) * (1.0 / _hable(peak_scale))
    transition, slope = 0.3, 0.8
    ls = lum * peak_scale
    linear = ls <= transition
    out = np.zeros_like(ls)
    out[linear] = ls[linear]
    x = ls[~linear]
    out[~linear] = transition + (1.0 - transition) * (1.0 - exp(-slope * (x - transition) / (1.0 - transition)))
    return out


def apply_scale(frame: np.ndarray, lum: np.ndarray, lum_hdr: np.ndarray) -> np.ndarray:
    scale = np.where(lum > 0.0001, lum_hdr / lum, 1.0)
    return np.clip(frame * scale[:, :, np.newaxis], 0, 1)


def tone_map(frame: np.ndarray, config) -> np.ndarray:
    lum = luminance(frame)
    return apply_scale(frame, lum, curve(lum, config))


def quantise8(frame: np.ndarray) -> np.ndarray:
    return (np.clip(frame, 0, 1) * 255).astype(np.uint8)


# ---- cv2, restated -------------------------------------------------------------------------------------------------------------------
bgr2lab = fr.bgr_to_lab_gamma
lab2bgr = fr.lab_to_bgr_gamma


def _sat8(x) -> np.ndarray:
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def clahe_geometry(h: int, w: int, grid=(8, 8)):
    """(padded rows, padded columns, tile rows, tile columns)"""
    gx, gy = grid
    if h % gy == 0 and w % gx == 0:
        hp, wp = h, w
    else:
        hp, wp = h + gy - h % gy, w + gx - w % gx
    return hp, wp, hp // gy, wp // gx


def clahe_luts(l: np.ndarray, clip_limit=2.0, grid=(8, 8)) -> np.ndarray:
    """uint8 [gy][gx][256]: the tile maps."""
    h, w = l.shape
    gx, gy = grid
    hp, wp, th, tw = clahe_geometry(h, w, grid)
    ext = np.pad(l, ((0, hp - h), (0, wp - w)), mode="reflect") if (hp, wp) != (h, w) else l
    area = th * tw
    limit = max(int(clip_limit * area / 256), 1)
    scale = f32(255.0 / area)
    luts = np.empty((gy, gx, 256), np.uint8)
    for ty in range(gy):
        for tx in range(gx):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            excess = int(np.maximum(hist - limit, 0).sum())
            hist = np.minimum(hist, limit) + excess // 256
            residual = excess % 256
            if residual:
                step = max(256 // residual, 1)
                hist[np.arange(0, 256, step)[:residual]] += 1
            luts[ty, tx] = _sat8(np.cumsum(hist).astype(f32) * scale)
    return luts


def clahe_interpolate(l: np.ndarray, luts: np.ndarray, grid=(8, 8)) -> np.ndarray:
    h, w = l.shape
    gx, gy = grid
    _, _, th, tw = clahe_geometry(h, w, grid)

    def axis(n, tile, count):
        f = np.arange(n).astype(f32) * f32(1 / tile) - f32(0.5)
        t1 = np.floor(f)
        return (np.clip(t1, 0, count - 1).astype(np.int64), np.clip(t1 + 1, 0, count - 1).astype(np.int64), (f - t1).astype(f32))

    ty1, ty2, ya = (v[:, None] for v in axis(h, th, gy))
    tx1, tx2, xa = (v[None, :] for v in axis(w, tw, gx))
    one = f32(1)
    v = l.astype(np.int64)
    top = luts[ty1, tx1, v].astype(f32) * (one - xa) + luts[ty1, tx2, v].astype(f32) * xa
    bottom = luts[ty2, tx1, v].astype(f32) * (one - xa) + luts[ty2, tx2, v].astype(f32) * xa
    res = top * (one - ya) + bottom * ya
    assert res.dtype == np.float32
    return _sat8(res)


def clahe(l: np.ndarray, clip_limit=2.0, grid=(8, 8)) -> np.ndarray:
    assert l.dtype == np.uint8 and l.ndim == 2
    return clahe_interpolate(l, clahe_luts(l, clip_limit, grid), grid)


def add_weighted(a: np.ndarray, alpha: float, b: np.ndarray, beta: float, gamma: float = 0) -> np.ndarray:
    assert gamma == 0
    return _sat8(a.astype(f32) * f32(alpha) + b.astype(f32) * f32(beta))


def _div_table(scale: int) -> np.ndarray:
    t = np.zeros(256, np.int64)
    t[1:] = np.rint(scale / np.arange(1, 256, dtype=np.float64)).astype(np.int64)
    return t


SDIV = _div_table(255 << 12)                  # sdiv[i] = round((255 << 12) / i)
HDIV = _div_table((180 << 12) // 6)           # hdiv[i] = round((180 << 12) / (6 i))
HSV_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])     # (b, g, r) picks of tab per sector


def bgr2hsv(bgr: np.ndarray) -> np.ndarray:
    v3 = bgr.astype(np.int64)
    b, g, r = v3[..., 0], v3[..., 1], v3[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + 2048) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv: np.ndarray) -> np.ndarray:
    h = hsv[..., 0].astype(f32) * f32(6 / 180)
    s = hsv[..., 1].astype(f32) / f32(255)
    v = hsv[..., 2].astype(f32) / f32(255)
    sector = np.floor(h)
    f = h - sector
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    pick = HSV_SECTORS[sector.astype(np.int64) % 6]
    return _sat8(np.take_along_axis(tab, pick, axis=-1) * f32(255))


# ---- steps 4 - 6 on bytes ---------------------------------------------------------------------------------------------------------------
def local_contrast_u8(q: np.ndarray) -> np.ndarray:
    lab = bgr2lab(q)
    l = lab[:, :, 0].copy()
    lab[:, :, 0] = add_weighted(l, 0.5, clahe(l), 0.5, 0)
    return lab2bgr(lab)


def adjust_saturation_u8(q: np.ndarray, boost: float) -> np.ndarray:
    hsv = bgr2hsv(q).astype(f32)
    hsv[:, :, 1] = np.clip(hsv[:, :, 1] * boost, 0, 255)
    return hsv2bgr(hsv.astype(np.uint8))


def local_contrast(frame: np.ndarray) -> np.ndarray:
    return local_contrast_u8(quantise8(frame)).astype(f32) / 255.0


def adjust_saturation(frame: np.ndarray, config) -> np.ndarray:
    return adjust_saturation_u8(quantise8(frame), config.saturation_boost).astype(f32) / 255.0


def clipped_mask(frame: np.ndarray, tables: dict) -> np.ndarray:
    """any(frame / maxv > 0.98) over the channels, as a comparison of codes"""
    return (frame >= tables["clip8" if frame.dtype == np.uint8 else "clip16"]).any(axis=2)


def recover_highlights(original: np.ndarray, processed: np.ndarray, tables: dict) -> np.ndarray:
    mask = clipped_mask(original, tables)
    if not mask.any():
        return processed
    return np.where(mask[:, :, np.newaxis], processed * 0.95, processed)


def transfer_and_quantise(frame: np.ndarray, config) -> np.ndarray:
    """The float path: the transfer function per pixel in float32, then 16 bits (truncated)."""
    return quantise16(transfer(frame, config))


# ---- the paths that are not bit-pinned: float64 yardsticks and the derived bounds (DESIGN K20) ------------------------------------------
U = 2.0 ** -24                     # unit roundoff of float32: every rounded operation has a relative error of at most U
POW_ULPS = EXP_ULPS = LOG_ULPS = 2   # relied on for powf / expf / logf (the HIP math API documents 1 ulp each; 1 ulp <= 2 U relative)
PQ_REL = 78.84375 * (5.008 + 0.1 * POW_ULPS) + 2 * POW_ULPS + 1       # relative error of trunc's argument, in units of U
HLG_ABS = 0.17883277 * (2.4 + (2 * LOG_ULPS + 1) * 2.461) + 2          # absolute error of trunc's argument / 65535, in units of U
MOBIUS_ULPS = 25                   # of the tone-mapped plane against the float64 formula on the same float32 luminance


def transfer64(frame: np.ndarray, config) -> np.ndarray:
    """The transfer function times 65535 in float64 on a float32 plane, with the constants the float32 evaluation uses (the Python
    floats rounded to float32): what the float32 result is compared with."""
    x = np.clip(frame.astype(np.float64), 0, 1)
    c = lambda v: float(f32(v))                                                    # noqa: E731
    if _name(config.target_format) in PQ_FORMATS:
        lm = np.power(x * c(config.peak_brightness / 10000.0), c(2610.0 / 16384.0))
        y = np.power((c(3424.0 / 4096.0) + c(2413.0 / 4096.0 * 32.0) * lm) / (1.0 + c(2392.0 / 4096.0 * 32.0) * lm), c(2523.0 / 4096.0 * 128.0))
    else:
        with np.errstate(all="ignore"):
            y = np.where(x <= c(1.0 / 12.0), np.sqrt(3.0 * x), c(0.17883277) * np.log(np.maximum(12.0 * x - c(0.28466892), 1e-300)) + c(0.55991073))
    return np.clip(np.clip(y, 0, 1) * 65535.0, 0, 65535)


def epsilon_codes(v64: np.ndarray, config) -> np.ndarray:
    """The per-sample bound, in output codes, on |float32 evaluation - float64 evaluation| in front of the truncation."""
    if _name(config.target_format) in PQ_FORMATS:
        return v64 * (PQ_REL * U)
    return np.full_like(v64, 65535.0 * HLG_ABS * U)


def float_rule_violations(got: np.ndarray, plane: np.ndarray, config) -> int:
    """The number of samples of ``got`` (uint16) that break the rule of the float path: equal to trunc of the float64 value, or one
    code away from it while that value lies within epsilon of an integer."""
    v = transfer64(plane, config)
    want = np.floor(v)
    diff = np.abs(got.astype(np.float64) - want)
    near = np.abs(v - np.rint(v)) <= epsilon_codes(v, config)
    return int(((diff > 1) | ((diff == 1) & ~near)).sum())


def mobius_plane64(lin: np.ndarray, config) -> np.ndarray:
    """The MOBIUS tone map in float64 on the float32 linear plane and its float32 luminance (constants as float32)."""
    lum = luminance(lin).astype(np.float64)
    c = lambda v: float(f32(v))                                                    # noqa: E731
    x = lum * c(config.peak_brightness / 100.0)
    t, omt, ms = c(0.3), c(1.0 - 0.3), c(-0.8)
    lh = np.where(x <= t, x, t + omt * (1.0 - np.exp(ms * (x - t) / omt)))
    scale = np.where(lum > c(0.0001), lh / lum, 1.0)
    return np.clip(lin.astype(np.float64) * scale[:, :, None], 0, 1)


def ulp_distance(a32: np.ndarray, b64: np.ndarray) -> np.ndarray:
    """|a - b| in units of the float32 spacing at b"""
    return np.abs(a32.astype(np.float64) - b64) / np.spacing(np.maximum(np.abs(b64), 2.0 ** -126).astype(f32)).astype(np.float64)


# ---- test content ---------------------------------------------------------------------------------------------------------------------
def content_frame(h: int, w: int, dtype=np.uint8, seed: int = 0) -> np.ndarray:
    """A frame that reaches every branch at any size from 8 x 8: bands of random samples, a smooth ramp (CLAHE tiles clip), pure
    grays (s == 0 in HSV) and a block at the top of the range (the highlight flag; for uint16 codes on both sides of 64225), and, where
    the frame has room, a run of all 256 codes (uint16: each code's byte repeated, k * 257)."""
    rng = np.random.default_rng(1000 * h + w + seed)
    maxv = 255 if dtype == np.uint8 else 65535
    f = rng.integers(0, maxv + 1, (h, w, 3)).astype(np.int64)
    q = max(h // 4, 1)
    ramp = (np.arange(w)[None, :] * maxv // max(w - 1, 1) + np.arange(q)[:, None] * (maxv // 64)) % (maxv + 1)
    f[q:2 * q] = np.stack([ramp, ramp * 7 // 8, ramp * 3 // 4], axis=-1)
    gray = rng.integers(0, maxv + 1, (q, w)).astype(np.int64)
    gray[0, :min(w, 4)] = (0, maxv, maxv // 2, 1)[:min(w, 4)]
    f[2 * q:3 * q] = gray[..., None]
    edge = 250 if dtype == np.uint8 else 64225
    hot = rng.integers(edge - 3, edge + 3, (q, max(w // 2, 1), 3))
    f[3 * q:4 * q, :hot.shape[1]] = np.minimum(hot, maxv)
    if w * 3 * q >= 256 * 3:
        codes = np.arange(256) * (1 if dtype == np.uint8 else 257)
        flat = f[:q].reshape(-1, 3)
        flat[:256] = codes[:, None] + np.zeros(3, np.int64)
        flat[256:512, 1] = codes[:len(flat[256:512])]
        f[:q] = flat.reshape(q, w, 3)
    return f.astype(dtype)


# ---- the frame ------------------------------------------------------------------------------------------------------------------------
def tone_mapped_plane(frame: np.ndarray, config, tables=None) -> np.ndarray:
    """Steps 1 - 3: float32 H x W x 3."""
    return tone_map(linear_plane(frame, config, tables), config)


def linear_plane(frame: np.ndarray, config, tables=None) -> np.ndarray:
    """Steps 1 and 2."""
    t = tables if tables is not None else build_tables(config)
    lin = linearize(frame, t)
    return to_bt2020(lin) if uses_matrix(config) else lin


def quantised_chain(q: np.ndarray, frame: np.ndarray, config, tables: dict) -> np.ndarray:
    """Everything behind the first quantisation, on the bytes ``q`` of the tone-mapped plane: uint16 H x W x 3."""
    return tail_lookup(chain_bytes(q, config), frame, config, tables)


def chain_bytes(q: np.ndarray, config) -> np.ndarray:
    """Steps 4 and 5 on bytes (between them the reference divides by 255 and requantises: the identity)."""
    if config.enable_local_contrast:
        q = local_contrast_u8(q)
    if saturation_on(config):
        q = adjust_saturation_u8(q, config.saturation_boost)
    return q


def tail_lookup(q: np.ndarray, frame: np.ndarray, config, tables: dict) -> np.ndarray:
    """Steps 6 and 7 and the 16-bit quantisation of bytes / 255: row 1 of the tail table where the highlight flag is set."""
    flag = clipped_mask(frame, tables) if config.highlight_recovery else np.zeros(frame.shape[:2], bool)
    return tables["tail"][flag[:, :, None].astype(np.int64), q]


def convert_frame(frame: np.ndarray, config, tables=None, tone_mapped=None) -> np.ndarray:
    """uint8 / uint16 BGR H x W x 3 -> uint16 BGR.  ``tables``: `build_tables(config)` or the recorded ones.  ``tone_mapped``
    replaces steps 1 - 3 with a given float32 plane (the MOBIUS chain check feeds the device's own plane)."""
    t = tables if tables is not None else build_tables(config)
    hdr = tone_mapped if tone_mapped is not None else tone_mapped_plane(frame, config, t)
    if quantised(config):
        return quantised_chain(quantise8(hdr), frame, config, t)
    if config.highlight_recovery:
        hdr = recover_highlights(frame, hdr, t)
    return transfer_and_quantise(hdr, config)
