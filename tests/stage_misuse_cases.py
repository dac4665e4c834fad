"""Misuse of the eleven frame-stage drivers (DeviceFlowEstimator, DeviceSpatialDenoiser, DeviceTemporalAccumulator, DeviceClipAnalyzer,
DeviceFlickerReducer, DeviceTemporalConsistencyFilter, DeviceSceneCutDetector, DeviceFrameDeduplicator, DeviceColorGrader,
DeviceDeinterlacer, DeviceVHSProcessor) and what they produce, shared by tools/gen_stage_misuse_golden.py (which records what the
package answers) and tests/test_stage_misuse_gpu.py (which replays them against tests/golden/stage_misuse.json and
tests/golden/stage_outputs.json).  `answer`, `describe` and `digest` are those of engine_misuse_cases.py.

Frames are synth.synthetic_frames(6, 40, 56): 40 x 56 is the smallest size all stages accept together (VHS needs 32 rows, SSIM 7,
non-local means' 21-pixel search window and Farneback's three levels fit).  A misuse case is ``(driver, label, call, literal)``:
``call(ctx)`` makes the one wrong call and its answer is the exception's class name, ``str(e)`` and ``e.code`` where it has one, or a
description of the value returned (`shape_of`).  ``literal`` is ``None`` for a case whose answer is the recording; the cases that carry a
literal answer are the deliberate differences from the recording ("Stage drivers (Python)").  An output case is
``(label, call)``: ``call(ctx)`` returns tensors, arrays or plain values, and `as_frames` turns them into what `digest` hashes.

Every listed call is refused by a Python check, or by an argument check of the library that runs before its first launch.  Not
listed, because the method hands the tensors to a kernel unchecked and a wrong one would be read or written past its end:
  - `DeviceTemporalAccumulator.warp_frame`, `denoise_simple`, `denoise_with_flow` (frames and flow maps of any dtype or size),
    `_window_device`, `_chain_device`;
  - `DeviceTemporalConsistencyFilter.apply_device` (only the index is checked);
  - `DeviceFlickerReducer.reduce_flicker_device` with frames of different sizes (torch.stack's own message);
  - `DeviceVHSProcessor.box_sums_device`, `repair_device`, `blend_rows_device` and `chroma_samples_device` with tables that name rows,
    boxes or frames outside the frames; `chroma_shift_device` allocates its destinations itself, so its overlap refusal cannot be
    reached from outside;
  - a wrong device (a second GPU is not assumed).
"""
from __future__ import annotations

import tempfile
from pathlib import Path

import numpy as np
import torch

from engine_misuse_cases import answer as _answer
from engine_misuse_cases import describe, digest  # noqa: F401 - digest is used through this module by the tool and the test
from framewright_amd import _lib
from framewright_amd import color_grade as CG
from framewright_amd import dedup as DD
from framewright_amd import deinterlace as DI
from framewright_amd import scene_cuts as SC
from framewright_amd import temporal_denoise as TD
from framewright_amd import vhs as VH
from framewright_amd.synth import synthetic_frames

H, W = 40, 56
DRIVERS = ["DeviceFlowEstimator", "DeviceSpatialDenoiser", "DeviceTemporalAccumulator", "DeviceClipAnalyzer", "DeviceFlickerReducer",
           "DeviceTemporalConsistencyFilter", "DeviceSceneCutDetector", "DeviceFrameDeduplicator", "DeviceColorGrader",
           "DeviceDeinterlacer", "DeviceVHSProcessor"]
VHS_OVERLAP = {"raises": "ValueError", "message": "vhs: a destination overlaps a source frame (rebuilt rows are read as neighbours)"}


class Context:
    """What the cases share: the test frames on the host and on the device, and one driver of each kind, made when first asked for."""

    def __init__(self):
        self.frames = synthetic_frames(6, H, W, seed=33)
        self._made = {}

    def dev(self, i=0):
        """Frame ``i`` as a new uint8 H x W x 3 CUDA tensor."""
        return torch.from_numpy(self.frames[i]).cuda()

    def devs(self, n=6):
        return [self.dev(i) for i in range(n)]

    def stack(self, n=6):
        return torch.from_numpy(self.frames[:n]).cuda()

    def gray(self, i=0):
        return self.dev(i)[:, :, 1].contiguous()

    def get(self, name):
        if name not in self._made:
            self._made[name] = MAKE[name]()
        return self._made[name]


MAKE = {
    "DeviceFlowEstimator": lambda: TD.DeviceFlowEstimator(),
    "DeviceSpatialDenoiser": lambda: TD.DeviceSpatialDenoiser(),
    "DeviceTemporalAccumulator": lambda: TD.DeviceTemporalAccumulator(flow_estimator=TD.DeviceFlowEstimator()),
    "DeviceClipAnalyzer": lambda: TD.DeviceClipAnalyzer(),
    "DeviceFlickerReducer": lambda: TD.DeviceFlickerReducer(chunk_size=4),
    "DeviceTemporalConsistencyFilter": lambda: TD.DeviceTemporalConsistencyFilter(),
    "DeviceSceneCutDetector": lambda: SC.DeviceSceneCutDetector(),
    "DeviceFrameDeduplicator": lambda: DD.DeviceFrameDeduplicator(imagehash_available=True),
    "DeviceColorGrader": lambda: CG.DeviceColorGrader(CG.create_seasonal_lut("autumn", 0.7)),
    "DeviceDeinterlacer": lambda: DI.DeviceDeinterlacer(DI.InterlaceConfig(field_order=DI.FieldOrder.TFF)),
    "DeviceVHSProcessor": lambda: VH.DeviceVHSProcessor(rng=np.random.RandomState(5)),
}


def shape_of(v) -> str:
    """`describe`, element by element through lists, tuples and dicts (a list of tensors is its shapes, not its pixels)."""
    if isinstance(v, (list, tuple)):
        return ("[%s]" if isinstance(v, list) else "(%s)") % ", ".join(shape_of(x) for x in v)
    if isinstance(v, dict):
        return "{%s}" % ", ".join(f"{k!r}: {shape_of(x)}" for k, x in v.items())
    return describe(v)


def answer(call, ctx) -> dict:
    return _answer(lambda c: shape_of(call(c)), ctx)


def as_frames(v) -> list:
    """An output case's value as the list `digest` takes: tensors and arrays as they are, everything else (hashes, decisions, float
    lists, analysis records) as the bytes of its repr."""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return [v]
    if isinstance(v, (list, tuple)) and v and all(isinstance(x, (torch.Tensor, np.ndarray)) for x in v):
        return list(v)
    if isinstance(v, TD.FlowField):
        return [v.flow_x, v.flow_y, v.magnitude, v.confidence]
    if isinstance(v, dict) and v and all(isinstance(x, np.ndarray) for x in v.values()):
        return [v[k] for k in sorted(v)]
    return [np.frombuffer(repr(v).encode(), np.uint8)]


def _four(t):
    return torch.cat([t, t[..., :1]], dim=-1).contiguous()


def misuse_cases() -> list:
    out: list = []

    def add(driver, label, call, literal=None):
        out.append((driver, label, call, literal))

    def wrong_frames(driver, label, call, good, other_rank, listed=False):
        """The refusals of one frame argument: ``call(c, x)`` hands ``x`` over, ``good(c)`` is a tensor the method takes and
        ``other_rank(t)`` the same pixels at a rank it does not take; ``listed`` puts the tensor into a list."""
        one = (lambda t: [t]) if listed else (lambda t: t)
        add(driver, f"{label} with a float32 tensor", lambda c: call(c, one(good(c).float())))
        add(driver, f"{label} with a host tensor", lambda c: call(c, one(good(c).cpu())))
        add(driver, f"{label} with another rank", lambda c: call(c, one(other_rank(good(c)))))
        add(driver, f"{label} with 4 channels", lambda c: call(c, one(_four(good(c)))))

    frame = lambda c: c.dev()                        # noqa: E731
    clip = lambda c: c.stack(2)                      # noqa: E731
    first = lambda t: t[0]                           # noqa: E731 - n x H x W x 3 -> H x W x 3
    up = lambda t: t.unsqueeze(0)                    # noqa: E731 - H x W x 3 -> 1 x H x W x 3

    # ---- DeviceFlowEstimator
    n = "DeviceFlowEstimator"
    add(n, 'convention="x"', lambda c: TD.DeviceFlowEstimator(convention="x"))
    add(n, "an unknown Farneback key", lambda c: TD.DeviceFlowEstimator(window=15))
    add(n, "method DIS", lambda c: TD.DeviceFlowEstimator(method="dis"))
    add(n, "method unknown", lambda c: TD.DeviceFlowEstimator(method="x"))
    wrong_frames(n, "flow_device", lambda c, x: c.get("DeviceFlowEstimator").flow_device(x, x), frame, up)
    add(n, "flow_device with frames of two sizes", lambda c: c.get("DeviceFlowEstimator").flow_device(c.dev(), c.dev(1)[:32].contiguous()))
    add(n, "flow_device with a gray and a BGR frame", lambda c: c.get("DeviceFlowEstimator").flow_device(c.gray(), c.dev()))
    add(n, "maps_device with a float32 tensor", lambda c: c.get("DeviceFlowEstimator").maps_device(c.dev().float(), c.dev(1).float()))
    add(n, "estimate with a float array", lambda c: c.get("DeviceFlowEstimator").estimate(c.frames[0].astype(np.float32), c.frames[1]))
    add(n, "estimate with a 4-D array", lambda c: c.get("DeviceFlowEstimator").estimate(c.frames[:2], c.frames[1]))
    add(n, "estimate with 4 channels", lambda c: c.get("DeviceFlowEstimator").estimate(np.concatenate([c.frames[0], c.frames[0][:, :, :1]], 2), c.frames[1]))
    add(n, "estimate with frames of two sizes", lambda c: c.get("DeviceFlowEstimator").estimate(c.frames[0], c.frames[1][:32]))

    # ---- DeviceSpatialDenoiser
    n = "DeviceSpatialDenoiser"
    wrong_frames(n, "denoise_device", lambda c, x: c.get("DeviceSpatialDenoiser").denoise_device(x, 6), frame, lambda t: t[:, :, 0].contiguous())
    wrong_frames(n, "nlmeans_device", lambda c, x: c.get("DeviceSpatialDenoiser").nlmeans_device(x, 6.0), frame, up)
    add(n, "denoise with a float array", lambda c: c.get("DeviceSpatialDenoiser").denoise(c.frames[0].astype(np.float32), 0.5))
    add(n, "denoise with a 2-D array", lambda c: c.get("DeviceSpatialDenoiser").denoise(c.frames[0][:, :, 0], 0.5))
    add(n, "denoise_device with search window 20", lambda c: TD.DeviceSpatialDenoiser(search_window=20).denoise_device(c.dev(), 6))
    add(n, "nlmeans_device with h 0", lambda c: c.get("DeviceSpatialDenoiser").nlmeans_device(c.gray(), 0.0))
    add(n, "nlmeans_device with template window 9", lambda c: TD.DeviceSpatialDenoiser(template_window=9).nlmeans_device(c.gray(), 6.0))

    # ---- DeviceTemporalAccumulator
    n = "DeviceTemporalAccumulator"
    add(n, "flow_fn together with flow_estimator",
        lambda c: TD.DeviceTemporalAccumulator(flow_fn=lambda a, b: None, flow_estimator=c.get("DeviceFlowEstimator")))
    add(n, "denoise_sequence with temporal_radius 0", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, temporal_radius=0)))
    add(n, "denoise_sequence with noise_strength -1", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, noise_strength=-1)))
    add(n, "denoise_sequence with noise_strength nan", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, noise_strength=float("nan"))))
    add(n, "denoise_sequence with noise_strength True", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, noise_strength=True)))
    add(n, "denoise_sequence with a scene change outside the clip", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, scene_changes=[6])))
    add(n, "denoise_sequence with a scene change 1.5", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames, scene_changes=[1.5])))
    add(n, "denoise_sequence of no frames", lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence([])))
    add(n, "preserve_edges with frames of two sizes", lambda c: c.get("DeviceTemporalAccumulator").preserve_edges(c.frames[0], c.frames[1][:32]))
    add(n, "preserve_edges with a float array", lambda c: c.get("DeviceTemporalAccumulator").preserve_edges(c.frames[0], c.frames[1].astype(np.float32)))
    add(n, "preserve_edges with 2-D arrays", lambda c: c.get("DeviceTemporalAccumulator").preserve_edges(c.frames[0][:, :, 0], c.frames[1][:, :, 0]))

    # ---- DeviceClipAnalyzer
    n = "DeviceClipAnalyzer"
    add(n, "chunk_size 0 in the config", lambda c: TD.DeviceClipAnalyzer(TD.TemporalDenoiseConfig(chunk_size=0)))
    wrong_frames(n, "stats_device", lambda c, x: c.get("DeviceClipAnalyzer").stats_device(x), clip, first)
    add(n, "stats_device with no frame", lambda c: c.get("DeviceClipAnalyzer").stats_device(c.stack()[:0]))
    add(n, "frame_stats with a float array", lambda c: c.get("DeviceClipAnalyzer").frame_stats([c.frames[0].astype(np.float32)]))
    add(n, "frame_stats with frames of two sizes", lambda c: c.get("DeviceClipAnalyzer").frame_stats([c.frames[0], c.frames[1][:32]]))
    add(n, "frame_stats with 2-D arrays", lambda c: c.get("DeviceClipAnalyzer").frame_stats([c.frames[0][:, :, 0]]))
    add(n, "frame_stats of no frames", lambda c: c.get("DeviceClipAnalyzer").frame_stats([]))
    add(n, "analyze with sample_rate 0", lambda c: c.get("DeviceClipAnalyzer").analyze(c.frames, sample_rate=0))
    add(n, "analyze of no frames", lambda c: c.get("DeviceClipAnalyzer").analyze([]))
    add(n, "laplacian_variances of no frames", lambda c: c.get("DeviceClipAnalyzer").laplacian_variances([]))

    # ---- DeviceFlickerReducer
    n = "DeviceFlickerReducer"
    add(n, "chunk_size 0", lambda c: TD.DeviceFlickerReducer(chunk_size=0))
    add(n, "mode unknown", lambda c: TD.DeviceFlickerReducer(mode="x"))
    wrong_frames(n, "deflicker_batch_device", lambda c, x: c.get("DeviceFlickerReducer").deflicker_batch_device(x, 128.0), clip, first)
    add(n, "deflicker_batch_device with no frame", lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack()[:0], 128.0))
    add(n, "deflicker_batch_device with a float32 out",
        lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 128.0, out=torch.empty((6, H, W, 3), dtype=torch.float32, device="cuda")))
    add(n, "deflicker_batch_device with an out of 5 frames",
        lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 128.0, out=torch.empty((5, H, W, 3), dtype=torch.uint8, device="cuda")))
    add(n, "deflicker_batch_device with a host out",
        lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 128.0, out=torch.empty((6, H, W, 3), dtype=torch.uint8)))
    add(n, "deflicker_batch_device with a non-contiguous out",
        lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 128.0, out=torch.empty((6, H, 2 * W, 3), dtype=torch.uint8, device="cuda")[:, :, ::2]))
    add(n, "reduce_flicker_device of an empty list", lambda c: c.get("DeviceFlickerReducer").reduce_flicker_device([]))
    add(n, "reduce_flicker_device of an empty stack", lambda c: c.get("DeviceFlickerReducer").reduce_flicker_device(c.stack()[:0]))
    add(n, "reduce_flicker of no frames", lambda c: c.get("DeviceFlickerReducer").reduce_flicker([]))
    add(n, "reduce_flicker with a float array", lambda c: c.get("DeviceFlickerReducer").reduce_flicker([c.frames[0].astype(np.float32)]))
    add(n, "reduce_flicker with frames of two sizes", lambda c: c.get("DeviceFlickerReducer").reduce_flicker([c.frames[0], c.frames[1][:32]]))
    add(n, "analyze_flicker with sample_rate 0", lambda c: c.get("DeviceFlickerReducer").analyze_flicker(c.frames, sample_rate=0))
    add(n, "analyze_flicker of two frames", lambda c: c.get("DeviceFlickerReducer").analyze_flicker(c.frames[:2]))

    # ---- DeviceTemporalConsistencyFilter
    n = "DeviceTemporalConsistencyFilter"
    add(n, 'strength "x"', lambda c: TD.DeviceTemporalConsistencyFilter(strength="x"))
    add(n, "strength nan", lambda c: TD.DeviceTemporalConsistencyFilter(strength=float("nan")))
    add(n, "strength True", lambda c: TD.DeviceTemporalConsistencyFilter(strength=True))
    add(n, "temporal_radius -1", lambda c: TD.DeviceTemporalConsistencyFilter(temporal_radius=-1))
    add(n, "temporal_radius 1.5", lambda c: TD.DeviceTemporalConsistencyFilter(temporal_radius=1.5))
    add(n, "apply_device with index 6 of 6", lambda c: c.get("DeviceTemporalConsistencyFilter").apply_device(c.devs(), 6))
    add(n, "apply_device with index -1", lambda c: c.get("DeviceTemporalConsistencyFilter").apply_device(c.devs(), -1))
    add(n, "apply_device of no frames", lambda c: c.get("DeviceTemporalConsistencyFilter").apply_device([], 0))
    add(n, "apply_sequence with a float array", lambda c: list(c.get("DeviceTemporalConsistencyFilter").apply_sequence([c.frames[0].astype(np.float32)])))
    add(n, "apply_sequence with frames of two sizes", lambda c: list(c.get("DeviceTemporalConsistencyFilter").apply_sequence([c.frames[0], c.frames[1][:32]])))
    add(n, "apply_sequence of no frames", lambda c: list(c.get("DeviceTemporalConsistencyFilter").apply_sequence([])))

    # ---- DeviceSceneCutDetector
    n = "DeviceSceneCutDetector"
    for method in ("ssim_pairs_device", "histograms_device", "detect_clip_device"):
        wrong_frames(n, method, lambda c, x, method=method: getattr(c.get("DeviceSceneCutDetector"), method)(x), clip, first)
    wrong_frames(n, "ssim_pair_device", lambda c, x: c.get("DeviceSceneCutDetector").ssim_pair_device(x, x), frame, up)
    wrong_frames(n, "scene_change_device", lambda c, x: c.get("DeviceSceneCutDetector").scene_change_device(c.dev(), x), frame, up)
    add(n, "ssim_pairs_device with a numpy array", lambda c: c.get("DeviceSceneCutDetector").ssim_pairs_device(c.frames))
    add(n, "ssim_pair_device with frames of two sizes", lambda c: c.get("DeviceSceneCutDetector").ssim_pair_device(c.dev(), c.dev(1)[:32].contiguous()))
    add(n, "ssim_pairs_device of one frame", lambda c: c.get("DeviceSceneCutDetector").ssim_pairs_device(c.stack(1)))
    add(n, "detect_clip_device of one frame", lambda c: c.get("DeviceSceneCutDetector").detect_clip_device(c.stack(1)))
    add(n, "histograms_device of no frame", lambda c: c.get("DeviceSceneCutDetector").histograms_device(c.stack()[:0]))
    add(n, "ssim_pairs_device with a 6-pixel side", lambda c: c.get("DeviceSceneCutDetector").ssim_pairs_device(c.stack()[:, :6].contiguous()))
    add(n, "ssim_pair_device with a 6-pixel side", lambda c: c.get("DeviceSceneCutDetector").ssim_pair_device(c.dev()[:, :6].contiguous(), c.dev(1)[:, :6].contiguous()))

    # ---- DeviceFrameDeduplicator
    n = "DeviceFrameDeduplicator"
    wrong_frames(n, "hashes_device of a stack", lambda c, x: c.get("DeviceFrameDeduplicator").hashes_device(x), clip, first)
    wrong_frames(n, "hashes_device of a list", lambda c, x: c.get("DeviceFrameDeduplicator").hashes_device(x), frame, up, listed=True)
    add(n, "hashes_device of a list with a numpy array", lambda c: c.get("DeviceFrameDeduplicator").hashes_device([c.dev(), c.frames[1]]))
    add(n, "hashes_device of an empty list", lambda c: c.get("DeviceFrameDeduplicator").hashes_device([]))
    add(n, "hashes_device of an empty stack", lambda c: c.get("DeviceFrameDeduplicator").hashes_device(c.stack()[:0]))
    add(n, "analyze_clip_device of an empty list", lambda c: c.get("DeviceFrameDeduplicator").analyze_clip_device([]))
    add(n, "reconstruct_device with one enhanced frame too few",
        lambda c: c.get("DeviceFrameDeduplicator").reconstruct_device([c.dev()], DD.DeduplicationResult(total_frames=3, unique_frames=2, unique_indices=[0, 2],
                                                                                   frame_mapping={0: 0, 1: 0, 2: 2})))
    add(n, "extract_unique_frames without unique frames",
        lambda c: c.get("DeviceFrameDeduplicator").extract_unique_frames(Path("no_such_dir"), Path("no_such_out"), result=DD.DeduplicationResult()))

    def empty_directory(c):
        with tempfile.TemporaryDirectory() as tmp:
            return c.get("DeviceFrameDeduplicator").analyze_frames(Path(tmp))
    add(n, "analyze_frames of an empty directory", empty_directory)

    # ---- DeviceColorGrader
    n = "DeviceColorGrader"
    one_d = lambda: CG.DeviceColorGrader(CG.create_contrast_lut(1.2))      # noqa: E731
    add(n, "a 3D LUT of size 1", lambda c: CG.DeviceColorGrader(CG.LUT(size=1, data_3d=np.zeros((1, 1, 1, 3)))))
    add(n, "a 3D LUT of size 66", lambda c: CG.DeviceColorGrader(CG.LUT(size=66, data_3d=np.zeros((66, 66, 66, 3)))))
    add(n, "a 3D LUT that is no cube", lambda c: CG.DeviceColorGrader(CG.LUT(size=4, data_3d=np.zeros((4, 4, 5, 3)))))
    add(n, "a LUT without data", lambda c: CG.DeviceColorGrader(CG.LUT()))
    add(n, "a LUT with a NaN", lambda c: CG.DeviceColorGrader(CG.LUT(size=2, data_3d=np.full((2, 2, 2, 3), np.nan))))
    wrong_frames(n, "apply_device of a stack", lambda c, x: c.get("DeviceColorGrader").apply_device(x), clip, first)
    wrong_frames(n, "apply_device of a list", lambda c, x: c.get("DeviceColorGrader").apply_device(x), frame, up, listed=True)
    add(n, "apply_device of a list with a numpy array", lambda c: c.get("DeviceColorGrader").apply_device([c.frames[0]]))
    add(n, "a 1D LUT given an int16 stack", lambda c: one_d().apply_device(c.stack().to(torch.int16)))
    add(n, "a 1D LUT given an int16 list", lambda c: one_d().apply_device([c.dev().to(torch.int16)]))
    add(n, "a 1D LUT given a uint16 array", lambda c: one_d().apply(c.frames[0].astype(np.uint16)))
    add(n, "apply_device in place on a stack of views", lambda c: c.get("DeviceColorGrader").apply_device(c.stack()[:, :, ::2], inplace=True))
    add(n, "apply_device in place on a list of views", lambda c: c.get("DeviceColorGrader").apply_device([c.dev()[:, ::2]], inplace=True))
    add(n, "apply with a float array", lambda c: c.get("DeviceColorGrader").apply(c.frames[0].astype(np.float32)))
    add(n, "apply with a 2-D array", lambda c: c.get("DeviceColorGrader").apply(c.frames[0][:, :, 0]))
    add(n, "apply with 4 channels", lambda c: c.get("DeviceColorGrader").apply(np.concatenate([c.frames[0], c.frames[0][:, :, :1]], 2)))
    add(n, "apply_device of an empty stack", lambda c: c.get("DeviceColorGrader").apply_device(c.stack()[:0]))
    add(n, "apply_device of an empty list", lambda c: c.get("DeviceColorGrader").apply_device([]))

    # ---- DeviceDeinterlacer
    n = "DeviceDeinterlacer"
    Y, B, BOB = DI.FW_DEINTERLACE_YADIF, DI.FW_DEINTERLACE_BWDIF, DI.FW_DEINTERLACE_BOB
    add(n, "detection_threshold 2 in the config", lambda c: DI.DeviceDeinterlacer(DI.InterlaceConfig(detection_threshold=2)))
    wrong_frames(n, "interpolate_device", lambda c, x: c.get("DeviceDeinterlacer").interpolate_device(x, Y, 1), frame, up, listed=True)
    wrong_frames(n, "stats_device", lambda c, x: c.get("DeviceDeinterlacer").stats_device(x), frame, up, listed=True)
    add(n, "interpolate_device with a numpy array", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.frames[0]], Y, 1))
    add(n, "interpolate_device with frames of two sizes", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev(), c.dev(1)[:32].contiguous()], Y, 1))
    add(n, "interpolate_device with a gray and a BGR frame", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.gray(), c.dev()], Y, 1))
    add(n, "interpolate_device with frames of no rows", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()[:0]], Y, 1))
    add(n, "interpolate_device with a prev of another size", lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs(2), B, 1, prev=c.dev(2)[:32].contiguous()))
    add(n, "interpolate_device BOB of one row", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()[:1].contiguous()], BOB, 0))
    add(n, "interpolate_device with one destination for two frames", lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs(2), Y, 1, outs=[torch.empty_like(c.dev())]))
    add(n, "interpolate_device with non-contiguous outs",
        lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], Y, 1, outs=[torch.empty((H, 2 * W, 3), dtype=torch.uint8, device="cuda")[:, ::2]]))
    add(n, "interpolate_device with outs of another size",
        lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], Y, 1, outs=[torch.empty((H, W + 1, 3), dtype=torch.uint8, device="cuda")]))
    add(n, "interpolate_device with float32 outs",
        lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], Y, 1, outs=[torch.empty((H, W, 3), dtype=torch.float32, device="cuda")]))
    add(n, "interpolate_device with host outs", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], Y, 1, outs=[torch.empty((H, W, 3), dtype=torch.uint8)]))

    def onto_itself(c):
        fr = c.devs(2)
        return c.get("DeviceDeinterlacer").interpolate_device(fr, Y, 1, outs=fr)
    add(n, "interpolate_device onto its own frames", onto_itself)

    def into_the_next(c):
        buf = torch.zeros((3 * H * W * 3,), dtype=torch.uint8, device="cuda")
        fr = [buf[:H * W * 3].view(H, W, 3), buf[H * W * 3:2 * H * W * 3].view(H, W, 3)]
        return c.get("DeviceDeinterlacer").interpolate_device([fr[0]], B, 1, nxt=fr[1], outs=[buf[H * W * 3 + 100:2 * H * W * 3 + 100].view(H, W, 3)])
    add(n, "interpolate_device into the middle of nxt", into_the_next)
    add(n, "interpolate_device with mode 3", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], 3, 1, batched=False))
    add(n, "interpolate_device with parity 2", lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.dev()], Y, 2, batched=False))
    add(n, "interpolate_device of no frames", lambda c: c.get("DeviceDeinterlacer").interpolate_device([], Y, 1))
    for label, make in (("a float32 out", lambda k: torch.empty((k,), dtype=torch.float32, device="cuda")),
                        ("an out one element short", lambda k: torch.empty((k - 1,), dtype=torch.int64, device="cuda")),
                        ("a host out", lambda k: torch.empty((k,), dtype=torch.int64)),
                        ("a non-contiguous out", lambda k: torch.empty((2 * k,), dtype=torch.int64, device="cuda")[::2])):
        add(n, f"stats_device with {label}", lambda c, make=make: c.get("DeviceDeinterlacer").stats_device(c.devs(2), out=make(8)))
        add(n, f"pair_sums_device with {label}", lambda c, make=make: c.get("DeviceDeinterlacer").pair_sums_device(c.devs(2), c.devs(2), out=make(2)))
    add(n, "pair_sums_device with len(a) != len(b)", lambda c: c.get("DeviceDeinterlacer").pair_sums_device(c.devs(2), c.devs(3)))
    add(n, "pair_sums_device with a float32 tensor in b", lambda c: c.get("DeviceDeinterlacer").pair_sums_device([c.dev()], [c.dev().float()]))
    add(n, "analyze of no frames", lambda c: c.get("DeviceDeinterlacer").analyze([]))
    add(n, "analyze of frames of 3 rows", lambda c: c.get("DeviceDeinterlacer").analyze([c.dev()[:3].contiguous()] * 2))
    add(n, "analyze with a float32 tensor", lambda c: c.get("DeviceDeinterlacer").analyze([c.dev().float()] * 2))
    add(n, "deinterlace of no frames", lambda c: c.get("DeviceDeinterlacer").deinterlace([]))
    add(n, "deinterlace WEAVE", lambda c: c.get("DeviceDeinterlacer").deinterlace(c.devs(2), DI.DeinterlaceMethod.WEAVE))
    add(n, "stream with FieldOrder.AUTO", lambda c: list(DI.DeviceDeinterlacer().stream(iter(c.devs(2)))))
    add(n, "stream with frames of two sizes", lambda c: list(c.get("DeviceDeinterlacer").stream(iter([c.dev(), c.dev(1)[:32].contiguous()]))))
    add(n, "stream of no frames", lambda c: list(c.get("DeviceDeinterlacer").stream(iter([]))))
    add(n, "detect_telecine of 6 frames", lambda c: c.get("DeviceDeinterlacer").detect_telecine(c.devs()))
    add(n, "inverse_telecine of no frames", lambda c: c.get("DeviceDeinterlacer").inverse_telecine([]))

    # ---- DeviceVHSProcessor
    n = "DeviceVHSProcessor"
    add(n, "tracking 2 in the config", lambda c: VH.DeviceVHSProcessor(VH.VHSConfig(tracking=2)))
    for method, call in (("gray_stats_device", lambda c, x: c.get("DeviceVHSProcessor").gray_stats_device(x, sums=True)),
                         ("rainbow_device", lambda c, x: c.get("DeviceVHSProcessor").rainbow_device(x, 0.5)),
                         ("process", lambda c, x: c.get("DeviceVHSProcessor").process(x))):
        wrong_frames(n, method, call, frame, up, listed=True)
        add(n, f"{method} with frames of two sizes", lambda c, call=call: call(c, [c.dev(), c.dev(1)[:32].contiguous()]))
        add(n, f"{method} with frames of 31 rows", lambda c, call=call: call(c, [c.dev()[:31].contiguous()]))
        add(n, f"{method} with frames of one column", lambda c, call=call: call(c, [c.dev()[:, :1].contiguous()]))
    add(n, "process with a numpy array", lambda c: c.get("DeviceVHSProcessor").process([c.frames[0]]))
    add(n, "detect_vhs_artifacts with a float32 tensor", lambda c: c.get("DeviceVHSProcessor").detect_vhs_artifacts(c.dev().float()))
    add(n, "detect_vhs_artifacts of None", lambda c: c.get("DeviceVHSProcessor").detect_vhs_artifacts(None))
    add(n, "rainbow_device with gray frames", lambda c: c.get("DeviceVHSProcessor").rainbow_device([c.gray()], 0.5))
    add(n, "rainbow_device with one destination for two frames", lambda c: c.get("DeviceVHSProcessor").rainbow_device(c.devs(2), 0.5, outs=[torch.empty_like(c.dev())]))
    add(n, "rainbow_device with non-contiguous outs",
        lambda c: c.get("DeviceVHSProcessor").rainbow_device([c.dev()], 0.5, outs=[torch.empty((H, 2 * W, 3), dtype=torch.uint8, device="cuda")[:, ::2]]))
    add(n, "rainbow_device with outs of another size",
        lambda c: c.get("DeviceVHSProcessor").rainbow_device([c.dev()], 0.5, outs=[torch.empty((H, W + 1, 3), dtype=torch.uint8, device="cuda")]))
    add(n, "rainbow_device with host outs", lambda c: c.get("DeviceVHSProcessor").rainbow_device([c.dev()], 0.5, outs=[torch.empty((H, W, 3), dtype=torch.uint8)]))
    add(n, "box_sums_device with a float32 tensor", lambda c: c.get("DeviceVHSProcessor").box_sums_device([c.dev().float()], np.array([(0, 1, 1, 2, 2)], np.int32)))
    add(n, "edge_counts_device with a host tensor", lambda c: c.get("DeviceVHSProcessor").edge_counts_device([c.dev().cpu()]))
    add(n, "chroma_samples_device with 4 channels", lambda c: c.get("DeviceVHSProcessor").chroma_samples_device([_four(c.dev())], np.array([(0, 1, 0)], np.int32)))
    add(n, "chroma_shift_device with frames of 31 rows", lambda c: c.get("DeviceVHSProcessor").chroma_shift_device([c.dev()[:31].contiguous()], [1]))
    add(n, "chroma_shift_device with shift 3", lambda c: c.get("DeviceVHSProcessor").chroma_shift_device([c.dev()], [3]))
    add(n, "blend_rows_device with no rows",
        lambda c: c.get("DeviceVHSProcessor").blend_rows_device([c.dev()], [c.dev(1)], np.zeros((0, 4), np.int32), np.zeros((0, 2), np.float32)))
    add(n, "fix_dropout with temporal_radius 32", lambda c: VH.DeviceVHSProcessor(VH.VHSConfig(temporal_radius=32)).fix_dropout(c.devs(2)))
    add(n, "stream with block 0", lambda c: list(c.get("DeviceVHSProcessor").stream(iter(c.devs(2)), block=0)))
    add(n, "stream with frames of two sizes", lambda c: list(c.get("DeviceVHSProcessor").stream(iter([c.dev(), c.dev(1)[:32].contiguous()]), block=1)))
    add(n, "process of no frames", lambda c: c.get("DeviceVHSProcessor").process([]))
    add(n, "fix_dropout of no frames", lambda c: c.get("DeviceVHSProcessor").fix_dropout([]))
    add(n, "remove_head_switching with strength 0", lambda c: c.get("DeviceVHSProcessor").remove_head_switching(c.devs(2), strength=0))
    # the deliberate difference: the overlap refusal of the VHS entries names vhs, not deinterlace

    def rainbow_onto_itself(c):
        fr = c.devs(2)
        return c.get("DeviceVHSProcessor").rainbow_device(fr, 0.5, outs=fr)

    def blend_onto_itself(c):
        f = c.dev()
        return c.get("DeviceVHSProcessor").blend_rows_device([f], [f], np.array([(0, 5, 4, 6)], np.int32), np.array([(0.5, 0.5)], np.float32))

    def repair_onto_itself(c):
        f = c.dev()
        return c.get("DeviceVHSProcessor").repair_device([f, c.dev(1)], [f], np.array([(0, 0, 1, 4, 4, 3, 2, 0)], np.int32), 0.6)
    add(n, "rainbow_device onto its own frames", rainbow_onto_itself, VHS_OVERLAP)
    add(n, "blend_rows_device onto its own frame", blend_onto_itself, VHS_OVERLAP)
    add(n, "repair_device onto one of its sources", repair_onto_itself, VHS_OVERLAP)
    # the other deliberate difference: `_dev` is an attribute on every driver, so `_lib.owner_device` answers for the six temporal ones
    for name in DRIVERS[:6]:
        add(name, "owner_device", lambda c, name=name: str(_lib.owner_device(c.get(name))), {"returns": repr("'cuda:0'")})
    return out



# ---- what the drivers produce ---------------------------------------------------------------------------------------------------------
def _vhs(seed=5, **config):
    return VH.DeviceVHSProcessor(VH.VHSConfig(**config), rng=np.random.RandomState(seed))


def _blend_rows(c):
    srcs, dsts = c.devs(2), [c.dev(0).clone(), c.dev(1).clone()]
    rows = np.array([(0, 5, 4, 6), (0, 20, 19, 21), (1, 38, 37, 39)], np.int32)
    c.get("DeviceVHSProcessor").blend_rows_device(srcs, dsts, rows, np.array([(0.5, 0.5), (0.25, 0.75), (1.0, 0.0)], np.float32))
    return dsts


def _repair(c):
    sources, results = c.devs(3), [c.dev(1).clone()]
    boxes = np.array([(0, 0, 0, 4, 4, 6, 2, 0), (1, 0, 0, 20, 30, 5, 1, 0)], np.int32)     # a temporal copy from frame 0, a spatial fill
    c.get("DeviceVHSProcessor").repair_device(sources, results, boxes, 0.6)
    return results


def _interlaced(c):
    """The frames woven from two neighbours each, so that the analysis has combing to find."""
    fr = c.devs()
    out = []
    for a, b in zip(fr, fr[1:] + fr[:1]):
        w = a.clone()
        w[1::2] = b[1::2]
        out.append(w)
    return out


def output_cases() -> list:
    out: list = []

    def add(label, call):
        out.append((label, call))

    Y, B, BOB = DI.FW_DEINTERLACE_YADIF, DI.FW_DEINTERLACE_BWDIF, DI.FW_DEINTERLACE_BOB
    n = "DeviceFlowEstimator"
    add(f"{n} flow_device", lambda c: c.get("DeviceFlowEstimator").flow_device(c.dev(0), c.dev(1)))
    add(f"{n} flow_device on gray", lambda c: c.get("DeviceFlowEstimator").flow_device(c.gray(0), c.gray(1)))
    add(f"{n} maps_device with the weight map", lambda c: c.get("DeviceFlowEstimator").maps_device(c.dev(0), c.dev(1), weight_map=True))
    add(f"{n} maps_device, convention cv2", lambda c: TD.DeviceFlowEstimator(convention="cv2").maps_device(c.dev(0), c.dev(1)))
    add(f"{n} estimate", lambda c: c.get("DeviceFlowEstimator").estimate(c.frames[0], c.frames[1]))
    add(f"{n} warp_frame", lambda c: c.get("DeviceFlowEstimator").warp_frame(c.frames[0], c.get("DeviceFlowEstimator").estimate(c.frames[0], c.frames[1])))
    n = "DeviceSpatialDenoiser"
    add(f"{n} denoise_device", lambda c: c.get("DeviceSpatialDenoiser").denoise_device(c.dev(), 6))
    add(f"{n} nlmeans_device on gray", lambda c: c.get("DeviceSpatialDenoiser").nlmeans_device(c.gray(), 6.0))
    add(f"{n} nlmeans_device on two channels", lambda c: c.get("DeviceSpatialDenoiser").nlmeans_device(c.dev()[:, :, :2].contiguous(), 4.0))
    add(f"{n} denoise", lambda c: c.get("DeviceSpatialDenoiser").denoise(c.frames[0], 0.5))
    n = "DeviceTemporalAccumulator"
    add(f"{n} _chain_device", lambda c: c.get("DeviceTemporalAccumulator")._chain_device(1, c.devs(3), 0.5, True, 30))
    add(f"{n} _chain_device simple", lambda c: c.get("DeviceTemporalAccumulator")._chain_device(1, c.devs(3), None, False, 30, simple=True))
    add(f"{n} denoise_with_flow on the device", lambda c: c.get("DeviceTemporalAccumulator").denoise_with_flow(1, list(c.frames[:3])))
    add(f"{n} denoise_with_flow without a flow", lambda c: TD.DeviceTemporalAccumulator().denoise_with_flow(1, list(c.frames[:3])))
    add(f"{n} denoise_simple", lambda c: c.get("DeviceTemporalAccumulator").denoise_simple(list(c.frames[:3])))
    add(f"{n} preserve_edges", lambda c: c.get("DeviceTemporalAccumulator").preserve_edges(c.frames[0], c.frames[1]))
    add(f"{n} denoise_sequence on the device",
        lambda c: list(c.get("DeviceTemporalAccumulator").denoise_sequence(c.frames[:4], temporal_radius=1, preserve_edges=True, noise_strength=0.5, scene_changes=[2])))
    add(f"{n} denoise_sequence on the host path",
        lambda c: list(TD.DeviceTemporalAccumulator().denoise_sequence(c.frames[:3], temporal_radius=1, preserve_edges=True, noise_strength=0.5)))
    n = "DeviceClipAnalyzer"
    add(f"{n} stats_device", lambda c: c.get("DeviceClipAnalyzer").stats_device(c.stack()))
    add(f"{n} frame_stats", lambda c: c.get("DeviceClipAnalyzer").frame_stats(c.frames))
    add(f"{n} analyze", lambda c: c.get("DeviceClipAnalyzer").analyze(c.frames, sample_rate=2))
    add(f"{n} laplacian_variances", lambda c: c.get("DeviceClipAnalyzer").laplacian_variances(c.frames))
    n = "DeviceFlickerReducer"
    add(f"{n} deflicker_batch_device", lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 120.0))
    add(f"{n} deflicker_batch_device into out", lambda c: c.get("DeviceFlickerReducer").deflicker_batch_device(c.stack(), 120.0, out=torch.empty_like(c.stack())))
    add(f"{n} reduce_flicker_device of a list", lambda c: c.get("DeviceFlickerReducer").reduce_flicker_device(c.devs()))
    add(f"{n} reduce_flicker_device of a stack", lambda c: c.get("DeviceFlickerReducer").reduce_flicker_device(c.stack()))
    add(f"{n} target_brightness_device", lambda c: c.get("DeviceFlickerReducer").target_brightness_device(c.devs()))
    add(f"{n} reduce_flicker", lambda c: c.get("DeviceFlickerReducer").reduce_flicker(c.frames)[0])
    add(f"{n} analyze_flicker", lambda c: c.get("DeviceFlickerReducer").analyze_flicker(c.frames))
    n = "DeviceTemporalConsistencyFilter"
    add(f"{n} apply_device", lambda c: c.get("DeviceTemporalConsistencyFilter").apply_device(c.devs(), 2))
    add(f"{n} apply_device at the clip's edge", lambda c: c.get("DeviceTemporalConsistencyFilter").apply_device(c.devs(), 0))
    add(f"{n} apply_device without flow", lambda c: TD.DeviceTemporalConsistencyFilter(use_optical_flow=False).apply_device(c.devs(), 2))
    add(f"{n} apply_sequence", lambda c: list(c.get("DeviceTemporalConsistencyFilter").apply_sequence(c.frames[:4])))
    n = "DeviceSceneCutDetector"
    add(f"{n} ssim_pairs_device", lambda c: c.get("DeviceSceneCutDetector").ssim_pairs_device(c.stack()))
    add(f"{n} ssim_pair_device", lambda c: c.get("DeviceSceneCutDetector").ssim_pair_device(c.dev(0), c.dev(3)))
    add(f"{n} histograms_device", lambda c: c.get("DeviceSceneCutDetector").histograms_device(c.stack()))
    add(f"{n} scene_change_device", lambda c: [c.get("DeviceSceneCutDetector").scene_change_device(c.dev(0), 255 - c.dev(3)),
                                               c.get("DeviceSceneCutDetector").scene_change_device(c.dev(0), c.dev(1), use_ssim=False)])
    add(f"{n} detect_clip_device", lambda c: c.get("DeviceSceneCutDetector").detect_clip_device(torch.cat([c.stack(3), 255 - c.stack(3).flip(1)])))
    n = "DeviceFrameDeduplicator"
    pixel = lambda: DD.DeviceFrameDeduplicator(imagehash_available=False)      # noqa: E731
    add(f"{n} hashes_device of a stack", lambda c: c.get("DeviceFrameDeduplicator").hashes_device(c.stack()))
    add(f"{n} hashes_device of a list", lambda c: c.get("DeviceFrameDeduplicator").hashes_device(c.devs()))
    add(f"{n} hashes_device of a list of two sizes", lambda c: c.get("DeviceFrameDeduplicator").hashes_device([c.dev(0), c.dev(1)[:32].contiguous()]))
    add(f"{n} pixel hashes of a stack", lambda c: pixel().hashes_device(c.stack()))
    add(f"{n} pixel hashes of a list", lambda c: pixel().hashes_device(c.devs()))
    add(f"{n} analyze_clip_device", lambda c: c.get("DeviceFrameDeduplicator").analyze_clip_device([c.dev(i // 2) for i in range(6)]))
    n = "DeviceColorGrader"
    add(f"{n} apply_device of a stack", lambda c: c.get("DeviceColorGrader").apply_device(c.stack()))
    add(f"{n} apply_device of a list", lambda c: c.get("DeviceColorGrader").apply_device(c.devs()))
    add(f"{n} apply_device in place", lambda c: c.get("DeviceColorGrader").apply_device(c.stack(), inplace=True))
    add(f"{n} apply_device of an int16 stack", lambda c: c.get("DeviceColorGrader").apply_device((c.stack().to(torch.int32) * 257 - 32768).to(torch.int16)))
    add(f"{n} apply_device of a list of views", lambda c: c.get("DeviceColorGrader").apply_device([c.dev(0)[:, ::2], c.dev(1)[::2]]))
    add(f"{n} a 1D LUT on a stack", lambda c: CG.DeviceColorGrader(CG.create_contrast_lut(1.2)).apply_device(c.stack()))
    add(f"{n} apply", lambda c: c.get("DeviceColorGrader").apply(c.frames[0]))
    add(f"{n} apply of a uint16 clip", lambda c: c.get("DeviceColorGrader").apply(c.frames[:2].astype(np.uint16) * 257))
    n = "DeviceDeinterlacer"
    add(f"{n} interpolate_device YADIF batched", lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs(), Y, 1, batched=True))
    add(f"{n} interpolate_device YADIF one by one", lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs(), Y, 1, batched=False))
    add(f"{n} interpolate_device BWDIF with neighbours batched", lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs()[1:5], B, 0, prev=c.dev(0), nxt=c.dev(5)))
    add(f"{n} interpolate_device BWDIF with neighbours one by one",
        lambda c: c.get("DeviceDeinterlacer").interpolate_device(c.devs()[1:5], B, 0, prev=c.dev(0), nxt=c.dev(5), batched=False))
    add(f"{n} interpolate_device BOB on gray into outs",
        lambda c: c.get("DeviceDeinterlacer").interpolate_device([c.gray(0), c.gray(1)], BOB, 0, outs=[torch.empty_like(c.gray()), torch.empty_like(c.gray())]))
    add(f"{n} stats_device", lambda c: c.get("DeviceDeinterlacer").stats_device(_interlaced(c)))
    add(f"{n} pair_sums_device", lambda c: c.get("DeviceDeinterlacer").pair_sums_device(c.devs()[:5], c.devs()[1:]))
    add(f"{n} deinterlace BWDIF", lambda c: c.get("DeviceDeinterlacer").deinterlace(_interlaced(c), DI.DeinterlaceMethod.BWDIF))
    add(f"{n} deinterlace BOB", lambda c: c.get("DeviceDeinterlacer").deinterlace(_interlaced(c), DI.DeinterlaceMethod.BOB))
    add(f"{n} stream YADIF", lambda c: list(c.get("DeviceDeinterlacer").stream(iter(_interlaced(c)), block=4)))
    add(f"{n} analyze", lambda c: DI.DeviceDeinterlacer().analyze(_interlaced(c)))
    n = "DeviceVHSProcessor"
    add(f"{n} gray_stats_device", lambda c: {k: (v[np.lexsort(v.T[::-1])] if k == "runs" else v) for k, v in
                                             c.get("DeviceVHSProcessor").gray_stats_device(c.devs(), sums=True, bottom=True, runs=True).items()})
    add(f"{n} blend_rows_device", _blend_rows)
    add(f"{n} rainbow_device", lambda c: c.get("DeviceVHSProcessor").rainbow_device(c.devs(), 0.5))
    add(f"{n} rainbow_device into outs", lambda c: c.get("DeviceVHSProcessor").rainbow_device(c.devs(2), 0.25, outs=[torch.empty_like(c.dev()), torch.empty_like(c.dev())]))
    add(f"{n} box_sums_device", lambda c: c.get("DeviceVHSProcessor").box_sums_device(c.devs(3), np.array([(0, 1, 1, 5, 4), (2, 10, 30, 40, 10)], np.int32)))
    add(f"{n} repair_device", _repair)
    add(f"{n} edge_counts_device", lambda c: c.get("DeviceVHSProcessor").edge_counts_device(c.devs()))
    add(f"{n} chroma_shift_device", lambda c: c.get("DeviceVHSProcessor").chroma_shift_device(c.devs(3), [1, 2, 1]))
    add(f"{n} analysis_device", lambda c: c.get("DeviceVHSProcessor").analysis_device(c.dev()))
    add(f"{n} process", lambda c: _vhs(5).process(c.devs()))
    add(f"{n} process on gray", lambda c: _vhs(5).process([c.gray(i) for i in range(6)]))
    add(f"{n} stream", lambda c: list(_vhs(5).stream(iter(c.devs()), block=2)))
    add(f"{n} detect_vhs_artifacts", lambda c: _vhs(7).detect_vhs_artifacts(c.dev()))
    return out


def record_outputs(ctx) -> dict:
    got = {}
    for label, call in output_cases():
        v = call(ctx)
        torch.cuda.synchronize()
        got[label] = digest(as_frames(v))
    return got
