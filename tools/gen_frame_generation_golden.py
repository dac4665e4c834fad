#!/usr/bin/env python3
"""Writes tests/golden/frame_generation_reference.json and .npz from the reference's own `processors/frame_generation.py`:

    python tools/gen_frame_generation_golden.py /path/to/reference/src/framewright/processors/frame_generation.py

The reference needs cv2 and cv2 is absent here.  A stub module named `cv2` in `sys.modules` maps the calls of this file - `cvtColor`,
`calcOpticalFlowFarneback`, `remap`, `addWeighted`, `GaussianBlur`, `imread`, `imwrite` - to what tests/frame_generation_ref.py says
they mean, so cv2's own bytes stay unpinned, as everywhere in this project, and everything else is the reference's own code running:
the interpolation factors, the float32 products of the flow, the maps, the grain decision and its promotions, the clipping, the
order and the factors of the edge blends, the gap rule and the file names.

The reference draws from `np.random.normal`; for the run it is replaced by the counter generator of tests/qp_artifact_ref.py, keyed
as the restatement keys it.  For every case the tool runs the reference's frame methods in the order its driver runs them, runs
the restatement, and ASSERTS equality; it records digests, inputs and outputs of a few cases, the reference's float32 np.std next
to the contract's value, `detect_gaps` on lists of file names, the value types, and `generate_missing` itself with in-memory images
in cv2.imread's and cv2.imwrite's place: on a gap without a `before` frame, the one path it survives, and on gaps with one, where it
raises.  Data only: nothing of the reference's program text is written.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import logging
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import frame_generation_ref as R  # noqa: E402
from qp_artifact_ref import noise_indices, normal_quantiles  # noqa: E402

H, W = 24, 40
SEED = 5
# (key, model, gap size, has after, blend_edges, match_grain, smooth reference)
CASES = [(f"{m}|gap{g}|blend{b}|grain{int(mg)}", m, g, True, b, mg, False)
         for m in ("interpolate_blend", "optical_flow_warp") for g in (1, 2, 4, 10) for b, mg in ((3, True), (0, True), (1, False))]
CASES += [("interpolate_blend|gap2|blend3|grain1|ref_le_cur", "interpolate_blend", 2, True, 3, True, True),
          ("interpolate_blend|end3|blend3|grain1", "interpolate_blend", 3, False, 3, True, False),
          ("optical_flow_warp|end2|blend1|grain1", "optical_flow_warp", 2, False, 1, True, False),
          ("interpolate_blend|end4|blend0|grain0", "interpolate_blend", 4, False, 0, False, False)]
NPZ_CASES = ("interpolate_blend|gap2|blend3|grain1", "optical_flow_warp|gap1|blend3|grain1", "optical_flow_warp|gap4|blend0|grain1",
             "interpolate_blend|gap2|blend3|grain1|ref_le_cur", "interpolate_blend|end3|blend3|grain1")
NAME_LISTS = {
    "plain": (["frame_00000000.png", "frame_00000001.png", "frame_00000004.png", "frame_00000005.png", "frame_00000017.png"], None),
    "expected": (["frame_00000000.png", "frame_00000002.png"], 6),
    "expected_reached": (["frame_00000000.png", "frame_00000002.png"], 3),
    "end_too_large": (["frame_00000000.png"], 13),
    "patterns": (["Frame-0003.png", "0005.png", "shot_0009.png", "frame12.png", "notes.png"], None),
    "jpg_only": (["frame_001.jpg", "frame_004.jpg"], None),
    "png_wins": (["frame_001.jpg", "frame_009.jpg", "frame_002.png", "frame_004.png"], None),
    "empty": ([], 5),
    "unparsed": (["a.png", "b.png"], 5),
}


class Draws:
    """np.random.normal's stand-in: every call takes the next (seed, generated frame number, tag) of `queue`."""

    def __init__(self):
        self.queue = []

    def __call__(self, loc, scale, size):
        seed, number, tag = self.queue.pop(0)
        count = int(np.prod(size))
        assert len(size) == (2 if tag == R.TAG_GRAIN else 3)
        z = normal_quantiles()[noise_indices(seed, R.noise_index(number, tag), count)].reshape(size)
        return loc + np.float64(scale) * z


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.__version__ = "0.0-restated"
    stub.COLOR_BGR2GRAY, stub.INTER_LINEAR, stub.BORDER_REFLECT = 6, 1, 2

    def cvt(img, code):
        assert code == stub.COLOR_BGR2GRAY
        return R.oref.bgr2gray_u8(img)

    def farneback(prev, nxt, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
        assert flow is None and flags == 0 and prev.ndim == 2
        got = dict(pyr_scale=pyr_scale, levels=levels, winsize=winsize, iterations=iterations, poly_n=poly_n, poly_sigma=poly_sigma)
        assert got == R.FARNEBACK, got
        fx, fy = R.fr.farneback(prev, nxt, np.float32, **got)
        return np.stack([fx, fy], axis=-1).astype(np.float32)

    def remap(img, map_x, map_y, interpolation, borderMode=None):
        assert interpolation == stub.INTER_LINEAR and borderMode == stub.BORDER_REFLECT
        assert map_x.dtype == np.float32 and map_y.dtype == np.float32
        return R.remap_linear_reflect(img, map_x, map_y)

    def add_weighted(a, alpha, b, beta, gamma):
        assert gamma == 0
        return R.add_weighted(a, alpha, b, beta)

    def blur(img, ksize, sigma):
        assert tuple(ksize) == (0, 0) and sigma == 2 and img.dtype == np.float32
        return R.gaussian17_f32(img)

    stub.cvtColor, stub.calcOpticalFlowFarneback, stub.remap, stub.addWeighted, stub.GaussianBlur = cvt, farneback, remap, add_weighted, blur
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_frame_generation", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_frame_generation"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod, stub


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_methods(gen, draws, before, after, start, size, seed):
    """The reference's frame methods in its driver's order, with `before` where `before or after` stands."""
    numbers = [start + 1 + i for i in range(size)]
    if after is not None:
        generated = gen._generate_optical_flow(before, after, size) if gen._backend == "optical_flow" else \
            gen._generate_interpolated(before, after, size)
    else:
        draws.queue = [(seed, n, R.TAG_EXTRAPOLATE) for n in numbers]
        generated = gen._extrapolate_frames(before, size, "forward")
    stds = []
    for i, frame in enumerate(generated):
        draws.queue = [(seed, numbers[i], R.TAG_GRAIN)]
        generated[i] = gen._match_film_grain(frame, before)
        stds.append(len(draws.queue) == 0)                       # a draw was taken: ref > cur > 0
    return gen._blend_edges(generated, before, after), stds


def main() -> None:
    ref, stub = load_reference(sys.argv[1])
    logging.disable(logging.CRITICAL)
    draws = Draws()
    real_normal = np.random.normal
    np.random.normal = draws
    try:
        record(ref, stub, draws)
    finally:
        np.random.normal = real_normal


def record(ref, stub, draws) -> None:
    before, after = R.grainy_frame(H, W, 1), R.grainy_frame(H, W, 2, shift=2)
    smooth = (R.grainy_frame(H, W, 3, grain=0) // 8 + 100).astype(np.uint8)     # faint edges, no grain: its statistic is the smaller one
    npz = {"input|before": before, "input|after": after, "input|smooth": smooth}
    js_cases = {}
    for key, model, size, has_after, blend, grain, use_smooth in CASES:
        config = ref.FrameGenerationConfig(model=ref.GenerationModel(model), blend_edges=blend, match_grain=grain, seed=SEED)
        gen = ref.MissingFrameGenerator(config)
        b, a = (smooth if use_smooth else before), (after if has_after else None)
        keep = b.copy()
        got, drew = run_methods(gen, draws, b, a, 10, size, SEED)
        want = R.fill_gap(b, a, 10, size, gen._backend, grain, blend, SEED)
        assert len(got) == len(want) == size and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want)), key
        assert np.array_equal(b, keep), key
        js_cases[key] = {"model": model, "backend": gen._backend, "gap_size": size, "has_after": has_after, "blend_edges": blend,
                         "match_grain": grain, "before": "smooth" if use_smooth else "before", "seed": SEED, "start_frame": 10,
                         "grain_added": drew if grain else None, "sha256": [sha(g) for g in got]}
        if key in NPZ_CASES:
            npz[f"output|{key}"] = np.stack(got)
    assert any(c["grain_added"] and all(c["grain_added"]) for c in js_cases.values())
    assert js_cases["interpolate_blend|gap2|blend3|grain1|ref_le_cur"]["grain_added"] == [False, False]

    # the statistic: the reference's own float32 np.std of its grain plane next to the contract's float64 value
    stds = {}
    for name, frame in (("before", before), ("after", after), ("smooth", smooth)):
        gray = stub.cvtColor(frame, stub.COLOR_BGR2GRAY).astype(np.float32)
        own = np.std(gray - stub.GaussianBlur(gray, (0, 0), 2))
        assert own.dtype == np.float32 and own == R.grain_std_reference(frame)
        stds[name] = {"reference_f32": float(own), "contract_f64": R.grain_std64(frame), "contract_f32": float(R.grain_std(frame))}

    # the reflect border far outside the frame, through the reference's own map arithmetic: a flow of -3 widths at t = 0.5
    far = np.zeros((H, W, 2), np.float32)
    far[..., 0], far[..., 1] = -6.0 * W + 0.3, 4.0 * H - 0.7
    stub_flow = stub.calcOpticalFlowFarneback
    stub.calcOpticalFlowFarneback = lambda *a: far
    try:
        gen = ref.MissingFrameGenerator(ref.FrameGenerationConfig(model=ref.GenerationModel.OPTICAL_FLOW_WARP))
        got = gen._generate_optical_flow(before, after, 1)[0]
    finally:
        stub.calcOpticalFlowFarneback = stub_flow
    fxy = (far[..., 0], far[..., 1])
    assert np.array_equal(got, R.warp_blend(before, after, fxy, fxy, 0.5))
    npz["output|far_flow"] = got

    # detect_gaps on directories of empty files
    gaps = {}
    for name, (names, expected) in NAME_LISTS.items():
        with tempfile.TemporaryDirectory() as tmp:
            for n in names:
                (Path(tmp) / n).write_bytes(b"")
            for max_gap in (10, 2):
                found = ref.MissingFrameGenerator(ref.FrameGenerationConfig(max_gap_frames=max_gap)).detect_gaps(Path(tmp), expected)
                rows = [[g.start_frame, g.end_frame, g.gap_size, g.after_path is not None] for g in found]
                assert rows == [list(r) for r in R.detect_gaps(names, expected, max_gap)], (name, max_gap)
                assert all((g.before_path.name if g.before_path else None) in names for g in found)
                gaps[f"{name}|max{max_gap}"] = {"names": names, "expected_count": expected, "max_gap_frames": max_gap, "gaps": rows}

    # the value types
    cfg = ref.FrameGenerationConfig()
    defaults = {k: (v.value if isinstance(v, ref.GenerationModel) else v) for k, v in cfg.__dict__.items()}
    rejected = []
    for bad in ({"max_gap_frames": 0}, {"blend_edges": -1}, {"model": "optical_flow"}, {"model": "rife"}):
        try:
            ref.FrameGenerationConfig(**bad)
            raise AssertionError(bad)
        except ValueError as e:
            rejected.append([bad, str(e)])
    enums = {"GenerationModel": {m.name: m.value for m in ref.GenerationModel}}
    backends = {m.value: ref.MissingFrameGenerator(ref.FrameGenerationConfig(model=m))._backend for m in ref.GenerationModel}
    made = ref.create_frame_generator("optical_flow_warp", 4, False, 1).config
    created = {k: (v.value if isinstance(v, ref.GenerationModel) else v) for k, v in made.__dict__.items()}
    result_defaults = dict(ref.FrameGenerationResult().__dict__)
    gap_defaults = {k: v for k, v in ref.GapInfo(1, 3, 1).__dict__.items()}
    try:
        ref.FrameGenerationResult(gaps_detected=1)
        raise AssertionError("gaps_detected")
    except TypeError as e:
        restorer_calls = {"fill_gap": hasattr(ref.MissingFrameGenerator, "fill_gap"), "gaps_detected": str(e)}

    # generate_missing with in-memory images
    driver = {}
    for name, has_before, has_after in (("after_only", False, True), ("both", True, True), ("before_only", True, False)):
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = Path(tmp) / "in", Path(tmp) / "out"
            src.mkdir()
            images = {"frame_00000004.png": before, "frame_00000007.png": after}
            for n in images:
                (src / n).write_bytes(n.encode())
            written, progress, messages = {}, [], []
            stub.imread = lambda p: images[Path(p).name].copy()
            stub.imwrite = lambda p, img: written.__setitem__(Path(p).name, img)
            gen = ref.MissingFrameGenerator(ref.FrameGenerationConfig(seed=SEED))
            gap = ref.GapInfo(4, 7, 2, src / "frame_00000004.png" if has_before else None, src / "frame_00000007.png" if has_after else None)
            numbers = iter([5, 6])
            inner_grain, inner_extra = gen._match_film_grain, gen._extrapolate_frames

            def grain(frame, reference):
                draws.queue = [(SEED, next(numbers), R.TAG_GRAIN)]
                return inner_grain(frame, reference)

            def extrapolate(reference, count, direction="forward"):
                order = [5, 6] if direction == "forward" else [6, 5]     # the backward list is reversed behind the draws
                draws.queue = [(SEED, n, R.TAG_EXTRAPOLATE) for n in order]
                return inner_extra(reference, count, direction)

            gen._match_film_grain, gen._extrapolate_frames = grain, extrapolate
            handler = logging.Handler()
            handler.emit = lambda rec: messages.append(rec.getMessage())
            logging.disable(logging.NOTSET)
            ref.logger.addHandler(handler)
            try:
                res = gen.generate_missing(src, dst, [gap], progress.append)
            finally:
                ref.logger.removeHandler(handler)
                logging.disable(logging.CRITICAL)
            if name == "after_only":
                want = R.fill_gap(None, after, 4, 2, R.INTERPOLATE, True, 3, SEED)
                assert sorted(written) == ["frame_00000005.png", "frame_00000006.png"]
                assert all(np.array_equal(written[f"frame_{5 + i:08d}.png"], w) for i, w in enumerate(want))
                npz["output|driver_after_only"] = np.stack(want)
            driver[name] = {"frames_generated": res.frames_generated, "frames_failed": res.frames_failed, "gaps_processed": res.gaps_processed,
                            "written": sorted(written), "copied": sorted(p.name for p in dst.iterdir()), "progress": progress,
                            "errors": [m for m in messages if m.startswith("Failed")]}
    assert driver["both"]["frames_failed"] == 2 and driver["before_only"]["frames_failed"] == 2 and driver["after_only"]["frames_generated"] == 2

    js = {"numpy": np.__version__, "height": H, "width": W, "defaults": defaults, "rejected": rejected, "enums": enums, "backends": backends,
          "created": created, "result_defaults": result_defaults, "gap_defaults": gap_defaults, "restorer_calls": restorer_calls,
          "gaussian17": [float(v) for v in R.gaussian17_coeffs()], "stds": stds, "detect_gaps": gaps, "driver": driver}
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"), default=str)        # noqa: E731 - one line per case
    head = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js.items())
    body = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js_cases.items())
    (out_dir / "frame_generation_reference.json").write_text(f'{{{head},\n"cases":{{\n{body}\n}}\n}}\n')
    np.savez_compressed(out_dir / "frame_generation_reference.npz", **npz)
    for name in ("frame_generation_reference.json", "frame_generation_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")
    print(len(js_cases), "cases")


if __name__ == "__main__":
    main()
