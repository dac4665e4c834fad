"""TEST INFRASTRUCTURE ONLY (imported by tests/ and tools/gen_perceptual_golden.py, nothing on the product path).

numpy restatement of the frame path of the reference's `processors/perceptual_tuning.py` (`PerceptualTuner.get_profile`,
`apply_to_frame`, `adjust_settings`).  It is the contract of csrc/perceptual.hip and of `framewright_amd.perceptual`.
cv2 is not installed where this project is built, so every cv2 call is what the older restatements say it is, by import:

    fastNlMeansDenoisingColored(x, None, h, h, 7, 21)   nlmeans_ref.nlmeans_colored
    cvtColor BGR2LAB / LAB2BGR                          flicker_ref.bgr_to_lab_gamma / lab_to_bgr_gamma
    createCLAHE(clip, (8, 8)).apply, addWeighted,
    cvtColor BGR2HSV / HSV2BGR and the saturation step  hdr_ref.clahe / add_weighted / adjust_saturation_u8
    GaussianBlur(gray, (5, 5), 0) on bytes              qp_artifact_ref.gaussian5_u8
    cvtColor BGR2GRAY                                   farneback_ref.bgr2gray_u8

and one piece is new: GaussianBlur(x, (0, 0), 3) on bytes, 19 taps in cv2's 8-bit fixed point, after aspect_ref.gauss99_table's
scheme.  cv2's own bytes stay unpinned; what tests/golden/perceptual_reference.* pins is the reference's own glue - the profile
arithmetic in Python doubles, the strict thresholds, int() of h, the float32 weights, the order of the steps, the grain taken from the
ORIGINAL frame - with these functions in cv2's place.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum

import numpy as np

import flicker_ref as fl
import hdr_ref as hd
from aspect_ref import reflect101
from farneback_ref import bgr2gray_u8
from nlmeans_ref import nlmeans_colored
from qp_artifact_ref import gaussian5_u8

f32 = np.float32
FIELDS = ("sharpening", "denoise", "color_enhancement", "detail_recovery", "grain_preservation")
GAUSS19_TAPS, GAUSS19_SIGMA = 19, 3.0
CONTENT_TYPES = ("general", "film", "animation", "documentary", "lowlight", "faces")


def _unit(v: float) -> float:
    return max(0.0, min(1.0, v))


class PerceptualMode(Enum):
    FAITHFUL = "faithful"
    BALANCED = "balanced"
    ENHANCED = "enhanced"


@dataclass
class PerceptualConfig:
    mode: PerceptualMode = PerceptualMode.BALANCED
    balance: float = 0.5
    preserve_grain: bool = True
    preserve_color_cast: bool = False
    sharpening_limit: float = 0.4
    denoise_limit: float = 0.6

    def __post_init__(self) -> None:
        self.balance, self.sharpening_limit, self.denoise_limit = _unit(self.balance), _unit(self.sharpening_limit), _unit(self.denoise_limit)


@dataclass
class PerceptualProfile:
    sharpening: float = 0.0
    denoise: float = 0.0
    color_enhancement: float = 0.0
    detail_recovery: float = 0.0
    grain_preservation: float = 1.0

    def __post_init__(self) -> None:
        for name in FIELDS:
            setattr(self, name, _unit(getattr(self, name)))

    def to_dict(self) -> dict:
        return {name: getattr(self, name) for name in FIELDS}


FAITHFUL = (0.1, 0.1, 0.0, 0.2, 1.0)          # in the order of FIELDS
ENHANCED = (0.6, 0.7, 0.5, 0.8, 0.2)


def profile(config: PerceptualConfig) -> PerceptualProfile:
    """`get_profile`: Python doubles, the lerp as a + (b - a) * t, then the two limits and the grain floor."""
    if config.mode == PerceptualMode.FAITHFUL:
        p = PerceptualProfile(*FAITHFUL)
    elif config.mode == PerceptualMode.ENHANCED:
        p = PerceptualProfile(*ENHANCED)
    else:
        p = PerceptualProfile(*(a + (b - a) * config.balance for a, b in zip(FAITHFUL, ENHANCED)))
    if p.sharpening > config.sharpening_limit:
        p.sharpening = config.sharpening_limit
    if p.denoise > config.denoise_limit:
        p.denoise = config.denoise_limit
    if config.preserve_grain:
        p.grain_preservation = max(p.grain_preservation, 0.7)
    return p


def plan(config: PerceptualConfig, to_int=int) -> dict:
    """The steps that run, in order, and their constants as the kernels take them: ``h`` (0: no denoise), the two addWeighted
    weights and the grain amount as float32 values, the saturation boost as float32, the CLAHE clip limit as the Python double (the
    integer limit of a frame size is `clahe_limit`).  ``to_int`` is the conversion of h (the reference's is int())."""
    p = profile(config)
    out = {"steps": [], "h": 0, "w_src": 0.0, "w_blur": 0.0, "boost": 0.0, "clip_limit": 0.0, "grain_amount": 0.0}
    if p.denoise > 0.1 and p.grain_preservation < 0.9:
        h = to_int(p.denoise * (1 - p.grain_preservation) * 10)
        if h > 0:
            out["steps"].append("denoise")
            out["h"] = h
    if p.sharpening > 0.1:
        amount = p.sharpening * 1.5
        out["steps"].append("sharpen")
        out["w_src"], out["w_blur"] = float(f32(1 + amount)), float(f32(-amount))
    if p.color_enhancement > 0.1:
        out["steps"].append("colour")
        out["boost"] = float(f32(1 + p.color_enhancement * 0.3))
    if p.detail_recovery > 0.2:
        out["steps"].append("detail")
        out["clip_limit"] = 1.0 + p.detail_recovery * 2.0
    if config.preserve_grain and p.grain_preservation > 0.3:
        out["steps"].append("grain")
        out["grain_amount"] = float(f32(p.grain_preservation * 0.5))
    return out


def clahe_limit(clip_limit: float, h: int, w: int) -> int:
    """The integer clip limit of one 8 x 8 tile of an h x w plane: max(int(clip * area / 256), 1) in double."""
    _, _, th, tw = hd.clahe_geometry(h, w)
    return max(int(clip_limit * (th * tw) / 256), 1)


# ---- GaussianBlur(x, (0, 0), 3) on bytes ---------------------------------------------------------------------------------------------
def gauss19_table(carry: bool = True) -> np.ndarray:
    """int64 [19], sum 256: exp(-x^2 / 18) at x = -9 .. 9 in float64 over its sum, quantised to 8 fractional bits from both ends
    towards the centre with the rounding error carried along (``carry=False``: each tap rounded alone, for the test that shows the
    difference); the centre tap takes what is left of 256."""
    n = GAUSS19_TAPS
    assert n == int(round(GAUSS19_SIGMA * 6 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    w = np.exp(-0.5 / (GAUSS19_SIGMA * GAUSS19_SIGMA) * x * x)
    w = w * (1.0 / float(np.sum(w)))
    q = np.zeros(n, dtype=np.int64)
    err, total = 0.0, 0
    for i in range(n // 2):
        adj = float(w[i]) * 256.0 + (err if carry else 0.0)
        v = int(np.rint(adj))
        err = adj - v
        q[i] = q[n - 1 - i] = v
        total += v
    q[n // 2] = 256 - 2 * total
    return q


def reflect_once(p: np.ndarray, length: int) -> np.ndarray:
    """A single reflection and a clamp: what `reflect101` must NOT be replaced by (a 9-pixel halo on a 9-pixel side reflects twice)."""
    p = np.asarray(p, dtype=np.int64)
    p = np.where(p < 0, -p, p)
    p = np.where(p >= length, 2 * length - 2 - p, p)
    return np.clip(p, 0, length - 1)


def gaussian_blur_sigma3_u8(img: np.ndarray, table: np.ndarray = None, reflect=reflect101) -> np.ndarray:
    """Rows first: h = sum src * k (at most 255 * 256: 16 bits), then columns: v = sum h * k (32 bits), out = (v + 2^15) >> 16."""
    k = gauss19_table() if table is None else table
    squeeze = img.ndim == 2
    src = (img[:, :, None] if squeeze else img).astype(np.int64)
    hs, ws, _ = src.shape
    taps = np.arange(GAUSS19_TAPS) - GAUSS19_TAPS // 2
    hor = np.zeros_like(src)
    for t, kt in zip(taps.tolist(), k.tolist()):
        hor += src[:, reflect(np.arange(ws) + t, ws), :] * kt
    ver = np.zeros_like(src)
    for t, kt in zip(taps.tolist(), k.tolist()):
        ver += hor[reflect(np.arange(hs) + t, hs)] * kt
    out = ((ver + (1 << 15)) >> 16).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


# ---- the steps -----------------------------------------------------------------------------------------------------------------------
def unsharp_u8(x: np.ndarray, w_src: float, w_blur: float) -> np.ndarray:
    return hd.add_weighted(x, w_src, gaussian_blur_sigma3_u8(x), w_blur, 0)


def saturation_u8(x: np.ndarray, boost: float) -> np.ndarray:
    return hd.adjust_saturation_u8(x, f32(boost))


def detail_u8(x: np.ndarray, clip_limit: float) -> np.ndarray:
    """L is REPLACED by its CLAHE (the HDR path blends half and half)."""
    lab = fl.bgr_to_lab_gamma(x)
    lab[:, :, 0] = hd.clahe(np.ascontiguousarray(lab[:, :, 0]), clip_limit)
    return fl.lab_to_bgr_gamma(lab)


def grain_u8(original: np.ndarray) -> np.ndarray:
    """cv2.subtract(gray, GaussianBlur(gray, (5, 5), 0)) of the ORIGINAL frame: saturating, so 0 where the blur exceeds the gray."""
    g = bgr2gray_u8(original)
    return np.maximum(g.astype(np.int64) - gaussian5_u8(g).astype(np.int64), 0).astype(np.uint8)


def grain_tail_u8(result: np.ndarray, original: np.ndarray, amount: float) -> np.ndarray:
    grain = grain_u8(original)
    return hd.add_weighted(result, 1.0, np.repeat(grain[:, :, None], 3, axis=2), amount, 0)


def add_weighted_fused(a: np.ndarray, alpha: float, b: np.ndarray, beta: float) -> np.ndarray:
    """What a contracting compiler makes of addWeighted, for the tests that plant it: fma(a, alpha, fl(b * beta)), two roundings
    where cv2 has three (float64 holds a * alpha exactly).  NOT the contract."""
    p = (b.astype(f32) * f32(beta)).astype(np.float64)
    t = (a.astype(np.float64) * np.float64(f32(alpha)) + p).astype(f32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


# BALANCED at this balance has grain_preservation just below 0.75 and the grain amount float32(0.375) - 2^-24: the amount at which the
# tail as ONE fused multiply-add differs from the definition on 584 of the 65536 (result, grain) pairs.  At the amounts of the round balances
# (0.35, 0.4, 0.5) no pair of bytes differs, so the tests that must catch a contracted tail use this configuration.
FMA_BALANCE = 0.312500149


def grain_tail_fused(result: np.ndarray, original: np.ndarray, amount: float) -> np.ndarray:
    """The tail as one fused multiply-add, fma(grain, amount, result): rounded once where cv2 rounds the product and then the sum
    (float64 holds the product exactly).  NOT the contract."""
    grain = grain_u8(original).astype(np.float64)[:, :, None]
    t = (grain * np.float64(f32(amount)) + result.astype(np.float64)).astype(f32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def fused_tail_pairs(amount: float) -> np.ndarray:
    """int [n][2]: the (result byte, grain byte) pairs on which the fused tail and the definition give different bytes."""
    a, g = np.arange(256, dtype=np.float64)[:, None], np.arange(256, dtype=np.float64)[None, :]
    two = a.astype(f32) * f32(1.0) + g.astype(f32) * f32(amount)
    one = (a + g * np.float64(f32(amount))).astype(f32)
    return np.argwhere(np.rint(two) != np.rint(one))


def tail_sensitive_result(result: np.ndarray, original: np.ndarray, amount: float) -> np.ndarray:
    """``result`` with every pixel whose grain (of ``original``) has a sensitive partner set to that partner on all three channels:
    the frame on which a fused tail shows."""
    partner = np.full(256, -1, np.int64)
    for a, g in fused_tail_pairs(amount)[::-1].tolist():
        partner[g] = a
    want = partner[grain_u8(original)]
    out = result.copy()
    out[want >= 0] = want[want >= 0][:, None].astype(np.uint8)
    return out


def denoise_u8(x: np.ndarray, h: int) -> np.ndarray:
    return nlmeans_colored(x, h, h, 7, 21)


def apply_plan(frame: np.ndarray, pl: dict) -> np.ndarray:
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    x = frame.copy()
    for step in pl["steps"]:
        if step == "denoise":
            x = denoise_u8(x, pl["h"])
        elif step == "sharpen":
            x = unsharp_u8(x, pl["w_src"], pl["w_blur"])
        elif step == "colour":
            x = saturation_u8(x, pl["boost"])
        elif step == "detail":
            x = detail_u8(x, pl["clip_limit"])
        else:
            assert step == "grain"
            x = grain_tail_u8(x, frame, pl["grain_amount"])
    return x


def apply_to_frame(frame: np.ndarray, config: PerceptualConfig) -> np.ndarray:
    """`PerceptualTuner.apply_to_frame`."""
    return apply_plan(frame, plan(config))


# ---- adjust_settings -----------------------------------------------------------------------------------------------------------------
def adjust_settings(config: PerceptualConfig, base_settings: dict, content_type: str = "general") -> dict:
    """`PerceptualTuner.adjust_settings`: the four strengths scaled by 0.5 + profile value where the caller gave one, else the
    profile's; the grain preservation; the content type's overrides, each from the values BEFORE any override; the colour cast."""
    p = profile(config)
    s = dict(base_settings)
    for name in FIELDS[:4]:
        s[name] = s[name] * (0.5 + getattr(p, name)) if name in s else getattr(p, name)
    s["grain_preservation"] = p.grain_preservation
    grain, denoise, sharp = s.get("grain_preservation", 1.0), s.get("denoise", 0), s.get("sharpening", 0)
    colour, detail = s.get("color_enhancement", 0), s.get("detail_recovery", 0)
    table = {"film": {"grain_preservation": min(grain + 0.2, 1.0), "denoise": max(denoise - 0.1, 0)},
             "animation": {"grain_preservation": 0.0, "sharpening": min(sharp + 0.1, 1.0), "denoise": min(denoise + 0.2, 1.0)},
             "documentary": {"grain_preservation": min(grain + 0.1, 1.0), "color_enhancement": max(colour - 0.1, 0)},
             "lowlight": {"denoise": min(denoise + 0.2, 1.0), "detail_recovery": min(detail + 0.2, 1.0)},
             "faces": {"denoise": min(denoise + 0.1, 1.0), "detail_recovery": min(detail + 0.15, 1.0), "sharpening": max(sharp - 0.05, 0)}}
    s.update(table.get(content_type, {}))
    if config.preserve_color_cast:
        s["preserve_color_cast"] = True
        s["color_enhancement"] = min(s.get("color_enhancement", 0), 0.2)
    return s


# ---- test content --------------------------------------------------------------------------------------------------------------------
def content_frame(h: int, w: int, seed: int = 0) -> np.ndarray:
    """hdr_ref.content_frame (random bands, a ramp whose CLAHE tiles clip, pure grays, a block at the top of the range) with
    hard black / white edges over it: next to them the sharpened value leaves [0, 255] on both sides, and the 5 x 5 blur of the
    gray exceeds the gray on the dark side of each."""
    f = hd.content_frame(h, w, np.uint8, seed)
    rng = np.random.default_rng(7000 * h + w + seed)
    cw, ch = max(w // 6, 1), max(h // 3, 1)
    f[:ch, :cw] = 255
    f[:ch, cw:2 * cw] = 0
    f[h - ch:, w - cw:] = rng.integers(236, 256, (ch, cw, 3))
    f[h - ch:, max(w - 2 * cw, 0):w - cw] = rng.integers(0, 20, (ch, w - cw - max(w - 2 * cw, 0), 3))
    return f
