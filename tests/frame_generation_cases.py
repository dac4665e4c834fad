"""TEST INFRASTRUCTURE ONLY.  The inputs that tests/test_frame_generation_gpu.py runs on the device and that
tests/test_frame_generation_ref_host.py checks on the CPU beforehand (the standard-deviation rule of DESIGN.md K22): three frame sizes
with odd sides, sides that are no multiple of the 64 x 16 tile or of a wave, and a width above one workgroup row."""
import numpy as np

import frame_generation_ref as R

SIZES = ((45, 67), (64, 96), (33, 130))
CLIP_NUMBERS, CLIP_EXPECTED = (0, 1, 4, 5, 7), 10          # gaps: 2 and 3 (two frames), 6 (one: shorter than blend_edges), 8 and 9 (the end)
SEED = 3


def pair(h: int, w: int):
    return R.grainy_frame(h, w, h), R.grainy_frame(h, w, w, shift=2)


def clip(h: int = 45, w: int = 67) -> list:
    return [R.grainy_frame(h, w, 40 + n, shift=n) for n in CLIP_NUMBERS]


def flows(h: int, w: int) -> dict:
    """The synthetic flows: name -> (flow_x, flow_y) float32.  `outward` points out of every border, by more than the frame's side."""
    y, x = np.mgrid[0:h, 0:w]
    const = lambda vx, vy: (np.full((h, w), vx, np.float32), np.full((h, w), vy, np.float32))       # noqa: E731
    out_x = np.where(x < w // 2, -(2.5 * w + 0.37), 2.5 * w + 0.37).astype(np.float32)
    out_y = np.where(y < h // 2, -(1.5 * h + 0.61), 1.5 * h + 0.61).astype(np.float32)
    return {"zero": const(0.0, 0.0), "constant": const(3.3, -2.6), "outward": (out_x, out_y)}


def interpolated(h: int = 45, w: int = 67) -> dict:
    """Generated frame number -> (reference frame, the frame in front of the grain step) of the clip with the `interpolate` backend."""
    frames = dict(zip(CLIP_NUMBERS, clip(h, w)))
    made = {}
    for start, end, size, has_after in R.gaps_from_numbers(CLIP_NUMBERS, CLIP_EXPECTED):
        before = frames[start]
        gen = R.generate_interpolated(before, frames[end], size) if has_after else \
            [R.extrapolate_frame(before, R.extrapolation_noise(before.shape, SEED, start + 1 + i)) for i in range(size)]
        made.update({start + 1 + i: (before, g) for i, g in enumerate(gen)})
    return made


def statistic_frames() -> dict:
    """Every frame whose deviation a GPU test compares with the contract's, by name."""
    out = {}
    for h, w in SIZES:
        out[f"before_{h}x{w}"], out[f"after_{h}x{w}"] = pair(h, w)
    out.update({f"clip_{n}": f for n, f in zip(CLIP_NUMBERS, clip())})
    out.update({f"generated_{n}": g for n, (_, g) in interpolated().items()})
    return out


def grain_decisions() -> dict:
    return {f"generated_{n}": pair_ for n, pair_ in interpolated().items()}
