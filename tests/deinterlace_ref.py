"""The contract of csrc/deinterlace.hip and framewright_amd/deinterlace.py: a NumPy restatement of the frame path of the reference's
`Deinterlacer` (processors/format/interlace.py) with every type spelled out.  tools/gen_deinterlace_golden.py holds it against the
reference's own functions (byte for byte for frames, field for field for the analysis); tests/test_deinterlace_ref_host.py holds it
against what that run recorded.  Frames are uint8 arrays H x W (gray) or H x W x 3 (BGR).

Integer forms (each was the reference's float32 expression; every intermediate there is a multiple of 1/64 below 2^10, so float32
holds it exactly and the truncating cast is a floor):
  YADIF  1 <= y <= H-2, y % 2 == parity : out[y] = (cur[y-1] + cur[y+1]) >> 1
  BWDIF  2 <= y <= H-3, y % 2 == parity : num = 3 * (9 * (cur[y-1] + cur[y+1]) - (cur[y-2] + cur[y+2])) + 4 * (prev[y] + next[y]),
         out[y] = clamp(num, 0, 255 * 64) >> 6.  The temporal weights sum to 0.125 (0.25 * 0.25 twice), not 0.25: rebuilt lines
         carry 0.875 of the brightness.  That is the reference.
  BOB    cv2.resize(frame[p::2], (W, H)) -> oracle/face_ref.resize_linear_u8 (cv2 itself is absent: unpinned)
parity 1 = TFF (odd rows rebuilt), 0 = BFF.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oracle.face_ref import resize_linear_u8  # noqa: E402

YADIF, BWDIF, BOB = 0, 1, 2


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def yadif_frame(cur: np.ndarray, parity: int, rounding: bool = False) -> np.ndarray:
    """``rounding`` is the wrong variant ((a + b + 1) >> 1) that the fixtures reject."""
    h = cur.shape[0]
    c = cur.astype(np.int64)
    out = cur.copy()
    for y in range(1, h - 1):
        if y % 2 == parity:
            out[y] = ((c[y - 1] + c[y + 1] + (1 if rounding else 0)) >> 1).astype(np.uint8)
    return out


def bwdif_frame(cur: np.ndarray, prev: np.ndarray, nxt: np.ndarray, parity: int, temporal_quarter: bool = False) -> np.ndarray:
    """``temporal_quarter`` is the wrong variant with temporal weight (prev + next) / 4 (8 * instead of 4 * in 64ths)."""
    h = cur.shape[0]
    c, p, n = cur.astype(np.int64), prev.astype(np.int64), nxt.astype(np.int64)
    out = cur.copy()
    for y in range(2, h - 2):
        if y % 2 == parity:
            num = 3 * (9 * (c[y - 1] + c[y + 1]) - (c[y - 2] + c[y + 2])) + (8 if temporal_quarter else 4) * (p[y] + n[y])
            out[y] = (np.clip(num, 0, 255 * 64) >> 6).astype(np.uint8)
    return out


def bob_field(cur: np.ndarray, field_parity: int) -> np.ndarray:
    h, w = cur.shape[:2]
    if h < 2:
        raise ValueError("BOB needs two rows")
    return resize_linear_u8(cur[field_parity::2], w, h)


def yadif(frames: Sequence[np.ndarray], parity: int, **kw) -> List[np.ndarray]:
    return [yadif_frame(f, parity, **kw) for f in frames]


def bwdif(frames: Sequence[np.ndarray], parity: int, **kw) -> List[np.ndarray]:
    n = len(frames)
    return [bwdif_frame(f, frames[i - 1] if i > 0 else f, frames[i + 1] if i < n - 1 else f, parity, **kw) for i, f in enumerate(frames)]


def bob(frames: Sequence[np.ndarray], parity: int) -> List[np.ndarray]:
    """parity 1 (TFF): even field first."""
    out: List[np.ndarray] = []
    for f in frames:
        even, odd = bob_field(f, 0), bob_field(f, 1)
        out += [even, odd] if parity == 1 else [odd, even]
    return out


# ---- statistics: exact integers ------------------------------------------------------------------------------------------------------
def gray(frame: np.ndarray) -> np.ndarray:
    if frame.ndim == 2:
        return frame
    v = frame.astype(np.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + (1 << 13)) >> 14).astype(np.uint8)


def stats(frame: np.ndarray) -> tuple:
    """(n_comb, s_field, s_odd, s_even) as Python ints."""
    g = gray(frame).astype(np.int64)
    h, w = g.shape
    r = h // 2
    even, odd = g[0:2 * r:2], g[1:2 * r:2]
    rows = np.abs(odd - even).sum(axis=1)
    n_comb = int((rows > 30 * w).sum())
    s_odd = int(np.abs(odd[1:] - odd[:-1]).sum()) if r > 1 else 0
    s_even = int(np.abs(even[1:] - even[:-1]).sum()) if r > 1 else 0
    return n_comb, int(rows.sum()), s_odd, s_even


def pair_sum(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.abs(gray(a).astype(np.int64) - gray(b).astype(np.int64)).sum())


def stats_float32(frame: np.ndarray) -> dict:
    """The same statistics in the number formats the reference forms them in (float32 means of float32 arrays, a float64 mean per
    row for the combing test): what its thresholds are compared with.  The reference keeps these as locals and returns only the
    decision, so the fixtures record THESE values, not the reference's; what ties them to it is the generator's assertion that the
    hint and the combing ratio they lead to equal the reference's own on every fixture frame."""
    g = gray(frame)
    odd, even = g[1::2, :].astype(np.float32), g[::2, :].astype(np.float32)
    m = min(odd.shape[0], even.shape[0])
    odd, even = odd[:m], even[:m]
    row_means = np.mean(np.abs(g[1::2][:m].astype(float) - g[::2][:m].astype(float)), axis=1)
    return {"odd_gradient": np.abs(np.diff(odd, axis=0)).mean(), "even_gradient": np.abs(np.diff(even, axis=0)).mean(),
            "diff": np.abs(odd - even).mean(), "row_means": row_means}


def frame_difference_float32(a: np.ndarray, b: np.ndarray) -> np.float32:
    return np.mean(np.abs(gray(a).astype(np.float32) - gray(b).astype(np.float32)))


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
METHODS = ("bob", "weave", "yadif", "bwdif", "neural", "nnedi")
ORDERS = ("tff", "bff", "auto", "unknown")
PATTERNS = ("3:2", "2:3", "2:2", "euro", "none")


@dataclass
class Analysis:
    is_interlaced: bool = False
    field_order: str = "unknown"
    confidence: float = 0.0
    combing_percentage: float = 0.0
    telecine_pattern: str = "none"
    recommended_method: str = "yadif"
    progressive_percentage: float = 0.0
    tff_percentage: float = 0.0
    bff_percentage: float = 0.0
    details: Dict[str, Any] = field(default_factory=dict)


def comb_ratio(st: tuple, h: int) -> float:
    return float(np.int64(st[0]) / (h // 2))


def order_hint(st: tuple, h: int, w: int) -> str:
    r = h // 2
    diff = st[1] / (r * w)
    odd_gradient, even_gradient = st[2] / ((r - 1) * w), st[3] / ((r - 1) * w)
    if diff < 5:
        return "prog"
    if odd_gradient > even_gradient * 1.1:
        return "tff"
    if even_gradient > odd_gradient * 1.1:
        return "bff"
    return "unknown"


def frame_difference(a: np.ndarray, b: np.ndarray) -> float:
    return pair_sum(a, b) / (a.shape[0] * a.shape[1])


def telecine_pattern(diffs: Sequence[float]) -> str:
    if len(diffs) < 10:
        return "none"
    arr = np.array(diffs)
    is_dup = arr < np.mean(arr) * 0.3
    ratio = np.sum(is_dup) / len(is_dup)
    if 0.35 < ratio < 0.45:
        for offset in range(5):
            matches = checks = 0
            for i in range(offset, len(is_dup) - 5, 5):
                if i + 2 < len(is_dup):
                    checks += 1
                    if is_dup[i] or is_dup[i + 2]:
                        matches += 1
            if checks > 0 and matches / checks > 0.6:
                return "3:2"
    if 0.45 < ratio < 0.55:
        return "2:2"
    return "none"


def recommend(a: Analysis) -> str:
    if not a.is_interlaced:
        return "weave"
    if a.telecine_pattern != "none":
        return "yadif"
    return "bwdif" if a.combing_percentage > 50 else "yadif"


def sample_indices(n: int, sample_count: int) -> np.ndarray:
    return np.linspace(0, n - 1, min(sample_count, n), dtype=int)


def analyze(frames: Sequence[np.ndarray], sample_count: int = 50, detection_threshold: float = 0.3) -> Analysis:
    a = Analysis()
    if not frames:
        return a
    h, w = frames[0].shape[:2]
    if h < 4:
        raise ValueError("analyze needs frames of at least 4 rows")
    combing, votes, diffs = [], {"tff": 0, "bff": 0, "prog": 0}, []
    for idx in sample_indices(len(frames), sample_count):
        st = stats(frames[idx])
        combing.append(comb_ratio(st, h))
        hint = order_hint(st, h, w)
        votes[hint if hint in ("tff", "bff") else "prog"] += 1
        if idx < len(frames) - 1:
            diffs.append(frame_difference(frames[idx], frames[min(idx + 1, len(frames) - 1)]))
    a.combing_percentage = (np.mean(combing) if combing else 0) * 100
    total = sum(votes.values())
    if total > 0:
        a.tff_percentage = votes["tff"] / total * 100
        a.bff_percentage = votes["bff"] / total * 100
        a.progressive_percentage = votes["prog"] / total * 100
    interlaced = a.tff_percentage + a.bff_percentage
    a.is_interlaced = bool(interlaced > 30 or a.combing_percentage > detection_threshold * 100)
    if a.tff_percentage > a.bff_percentage + 10:
        a.field_order = "tff"
    elif a.bff_percentage > a.tff_percentage + 10:
        a.field_order = "bff"
    else:
        a.field_order = "unknown"
    a.confidence = min(1.0, abs(interlaced - 50) / 50)
    if diffs:
        a.telecine_pattern = telecine_pattern(diffs)
        a.details["telecine"] = {"pattern": a.telecine_pattern, "diff_variance": float(np.var(diffs))}
    a.recommended_method = recommend(a)
    return a


def detect_telecine(frames: Sequence[np.ndarray]) -> str:
    if not frames or len(frames) < 10:
        return "none"
    return telecine_pattern([frame_difference(frames[i], frames[i + 1]) for i in range(min(60, len(frames) - 1))])


def inverse_telecine_indices(frames: Sequence[np.ndarray], pattern: Optional[str] = None) -> List[int]:
    """Indices of the frames that stay."""
    n = len(frames)
    if not frames:
        return []
    if pattern is None:
        pattern = detect_telecine(frames[:min(60, n)])
    diffs = [frame_difference(frames[i], frames[i + 1]) for i in range(n - 1)]
    if pattern == "none" or not diffs:
        return list(range(n))
    dup = np.array(diffs) < np.mean(diffs) * 0.3
    return [0] + [i for i in range(1, n) if not dup[i - 1]]


def resolve_order(frames: Sequence[np.ndarray], order: str, sample_count: int = 50, detection_threshold: float = 0.3) -> str:
    if order == "auto":
        order = analyze(frames[:min(20, len(frames))], sample_count, detection_threshold).field_order
        if order == "unknown":
            order = "tff"
    return order


def deinterlace(frames: Sequence[np.ndarray], method: str, order: str) -> List[np.ndarray]:
    """``order`` is already resolved; the reference's `is_tff = field_order == TFF` makes everything else BFF."""
    if not frames:
        return list(frames)
    parity = 1 if order == "tff" else 0
    if method == "bob":
        return bob(frames, parity)
    if method == "weave":
        return list(frames)
    if method in ("bwdif", "neural", "nnedi"):
        return bwdif(frames, parity)
    return yadif(frames, parity)


# ---- fixture clips (shared by the generator and the tests; all under 65 793 pixels) ----------------------------------------------------
def noise_clip(n: int, h: int, w: int, c: int, seed: int) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 1 else (h, w, c)
    out = []
    for _ in range(n):
        f = rng.integers(0, 256, size=shape, dtype=np.uint8)
        f[:, : max(1, w // 4)] = 255                      # saturated columns: the clamp of BWDIF is exercised at both ends
        f[0::2, max(1, w // 4): max(2, w // 2)] = 0
        f[1::2, max(1, w // 4): max(2, w // 2)] = 255
        out.append(f)
    return out


def _smooth(rng, h: int, w: int, c: int, freq: float) -> np.ndarray:
    """A smooth progressive picture: a few sinusoids, so vertical gradients are small and well away from every threshold."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for _ in range(c):
        ph = rng.random(4) * 6.28
        chans.append(128 + 50 * np.sin(freq * y / h * 6.28 + ph[0]) * np.cos(x / w * 6.28 + ph[1]) + 40 * np.sin((x + y) / (w + h) * 12 + ph[2]))
    img = np.stack(chans, axis=-1) if c == 3 else chans[0]
    return np.clip(img, 0, 255).astype(np.uint8)


def combed_clip(n: int, h: int, w: int, c: int, seed: int, newer: str) -> List[np.ndarray]:
    """Two pictures woven: the field named by ``newer`` ('odd' -> votes TFF, 'even' -> BFF) carries the busier picture."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        calm, busy = _smooth(rng, h, w, c, 1.0), _smooth(rng, h, w, c, 9.0 + i % 3)
        busy = np.clip(busy.astype(np.int64) + rng.integers(-60, 61, size=busy.shape), 0, 255).astype(np.uint8)
        f = calm.copy()
        f[(1 if newer == "odd" else 0)::2] = busy[(1 if newer == "odd" else 0)::2]
        out.append(f)
    return out


def progressive_clip(n: int, h: int, w: int, c: int, seed: int) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [_smooth(rng, h, w, c, 1.0) for _ in range(n)]


def cadence_clip(pattern: Sequence[bool], h: int, w: int, c: int, seed: int) -> List[np.ndarray]:
    """pattern[i] True: frame i + 1 repeats frame i but for a speck of noise (a small, non-zero difference)."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 1 else (h, w, c)
    frames = [rng.integers(0, 256, size=shape, dtype=np.uint8)]
    for dup in pattern:
        if dup:
            f = frames[-1].copy()
            f[rng.integers(0, h), rng.integers(0, w)] ^= 1
        else:
            f = rng.integers(0, 256, size=shape, dtype=np.uint8)
        frames.append(f)
    return frames


def analysis_clips() -> Dict[str, List[np.ndarray]]:
    """Every branch of the host logic: combed TFF, combed BFF, progressive, 3:2, 2:2, fewer than ten frames; gray and colour."""
    clips: Dict[str, List[np.ndarray]] = {}
    for c, tag in ((1, "gray"), (3, "bgr")):
        clips[f"tff/{tag}"] = combed_clip(12, 48, 64, c, 1, "odd")
        clips[f"bff/{tag}"] = combed_clip(12, 48, 64, c, 2, "even")
        clips[f"progressive/{tag}"] = progressive_clip(12, 48, 64, c, 3)
        clips[f"cadence32/{tag}"] = cadence_clip(([True, False, True, False, False] * 5)[:24], 24, 32, c, 4)
        clips[f"cadence22/{tag}"] = cadence_clip(([True, False] * 12)[:23], 24, 32, c, 5)
        clips[f"short/{tag}"] = combed_clip(6, 17, 33, c, 6, "odd")
    return clips


FRAME_SHAPES = [(5, 3), (6, 7), (9, 16), (17, 33)]


def frame_clips() -> Dict[str, List[np.ndarray]]:
    return {f"{h}x{w}x{c}": noise_clip(4, h, w, c, 100 * h + w + c) for h, w in FRAME_SHAPES for c in (1, 3)}


def sha256(a: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
