#!/usr/bin/env python3
"""Writes tests/golden/temporal_consistency_reference.json and .npz from the reference's own `processors/cross_attention_temporal.py`:

    python tools/gen_temporal_consistency_golden.py /path/to/reference/src/framewright/processors/cross_attention_temporal.py

The reference needs cv2 and cv2 is absent here.  A stub module named `cv2` in `sys.modules` maps the calls of this file - `cvtColor`,
`calcHist`, `compareHist`, `absdiff`, `GaussianBlur`, `imread`, `imwrite` - to what tests/temporal_consistency_ref.py says they mean,
so cv2's own bytes stay unpinned, as everywhere in this project, and everything else is the reference's own code running: the
normalisation of the histograms, the float32 score, its threshold, the neighbour rule, the blend and its truncation, the area
decision, the cut list, the window rule, the counting, the naming and the per-frame fallback.

For every case the tool runs the reference's methods and the restatement and ASSERTS equality; it records digests, and inputs and
outputs of a few cases, the value types, and what the restorer's own driver (`restorer.py`, `cross_attention_temporal`) does with
them: it passes `window_size=` to `CrossAttentionConfig`, calls `processor.process_frame` and builds
`TemporalConsistencyResult(processed_frames=, method_used=)`, none of which exist.  Data only: nothing of the reference's program text
is written.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import logging
import re
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import temporal_consistency_ref as R  # noqa: E402

H, W = 24, 40
CLIPS = {"plain9": (9, ()), "cut9": (9, (4,)), "twocuts9": (9, (3, 5)), "three": (3, ()), "two": (2, ()), "one": (1, ())}
FRAME_CASES = [(m, s, t) for m in (R.OPTICAL_FLOW, R.HYBRID) for s in (0.0, 0.5, 0.8, 1.0) for t in (0.02, 0.1)]
DRIVER_CASES = [(clip, m, w) for clip in ("plain9", "cut9", "twocuts9") for m in (R.OPTICAL_FLOW, R.HYBRID) for w in (1, 3, 7)] + \
               [(clip, m, 7) for clip in ("three", "two", "one") for m in (R.OPTICAL_FLOW, R.HYBRID)]
NPZ_FRAME_CASES = ("optical_flow|s0.8|t0.02",)
NPZ_DRIVER_CASES = ("twocuts9|hybrid|w1",)


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.__version__ = "0.0-restated"
    stub.COLOR_BGR2GRAY, stub.HISTCMP_CORREL = 6, 0

    def cvt(img, code):
        assert code == stub.COLOR_BGR2GRAY and img.dtype == np.uint8
        return R.fr.bgr2gray_u8(img)

    def calc_hist(images, channels, mask, hist_size, ranges):
        assert len(images) == 1 and channels == [0] and mask is None and hist_size == [256] and ranges == [0, 256]
        return R.calc_hist(images[0])

    def compare_hist(h1, h2, method):
        assert method == stub.HISTCMP_CORREL and h1.dtype == np.float32 and h2.dtype == np.float32
        return R.compare_hist_correl(h1, h2)

    def blur(img, ksize, sigma):
        assert tuple(ksize) == (5, 5) and sigma == 0 and img.dtype == np.float32
        return R.fr.gaussian_blur(img, 5, 0, np.float32)

    stub.cvtColor, stub.calcHist, stub.compareHist, stub.absdiff, stub.GaussianBlur = cvt, calc_hist, compare_hist, R.absdiff, blur
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_cross_attention_temporal", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_cross_attention_temporal"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod, stub


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def processor(ref, method, window=7, strength=0.8, threshold=0.02):
    proc = ref.CrossAttentionTemporalProcessor(ref.CrossAttentionConfig(method=ref.TemporalMethod(method), attention_window=window,
                                                                        blend_strength=strength, flicker_threshold=threshold))
    proc._backend = "optical_flow"                                # HYBRID with the network out of reach: the classical path
    return proc


def main() -> None:
    ref, stub = load_reference(sys.argv[1])
    logging.disable(logging.CRITICAL)
    clips = {name: R.flicker_clip(n, H, W, 11 + k, cuts) for k, (name, (n, cuts)) in enumerate(CLIPS.items())}
    npz = {f"input|{name}": np.stack(clips[name]) for name in ("twocuts9", "plain9")}

    # the frame methods, frame by frame, on the nine-frame clip and on the short ones
    frame_cases = {}
    for method, strength, threshold in FRAME_CASES:
        key = f"{method}|s{strength:g}|t{threshold:g}"
        proc = processor(ref, method, 7, strength, threshold)
        fn = proc._apply_optical_flow_consistency if method == R.OPTICAL_FLOW else proc._apply_hybrid_consistency
        row = {}
        for name in ("plain9", "three", "two", "one"):
            frames = clips[name]
            keep = [f.copy() for f in frames]
            got = [fn(frames, i) for i in range(len(frames))]
            want = [R.apply_frame(frames, i, method, threshold, strength) for i in range(len(frames))]
            assert all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want)), (key, name)
            assert all(np.array_equal(a, b) for a, b in zip(frames, keep)), (key, name)
            if len(frames) < 3:
                assert all(g is f for g, f in zip(got, frames)), (key, name)
            row[name] = [sha(g) for g in got]
            if name == "plain9" and key in NPZ_FRAME_CASES:
                npz[f"output|frames|{key}"] = np.stack(got)
        frame_cases[key] = {"method": method, "blend_strength": strength, "flicker_threshold": threshold, "sha256": row}
    plain = clips["plain9"]
    assert any(not np.array_equal(R.apply_frame(plain, i), plain[i]) for i in range(9))
    assert all(np.array_equal(R.apply_frame(plain, i, blend_strength=0.0), plain[i]) for i in range(9))

    # the mask, its integer form and the area decision
    masks = {}
    for threshold in (0.02, 0.1):
        proc = processor(ref, R.HYBRID, threshold=threshold)
        rows = []
        for i in range(9):
            p, n = R.neighbours(9, i)
            own = proc._detect_flicker(plain[p], plain[i], plain[n])
            k = R.blur_k(R.binary_mask(plain[p], plain[i], plain[n], threshold))
            assert own.dtype == np.float32 and np.array_equal(own, R.detect_flicker(plain[p], plain[i], plain[n], threshold))
            assert np.array_equal(own.view(np.uint32), R.mask_from_k(k).view(np.uint32))
            s = R.area_numerator(k)
            own_area = np.mean(own)
            assert own_area.dtype == np.float32 and own_area == R.area_value(s, k.size)
            assert bool(own_area > 0.01) == R.area_decision(s, k.size)
            rows.append({"sha256": sha(own), "area_sum": s, "area_f32": float(own_area), "above": bool(own_area > 0.01)})
        masks[f"t{threshold:g}"] = rows
        if threshold == 0.02:
            npz["output|mask_k|t0.02"] = np.stack([R.blur_k(R.binary_mask(plain[R.neighbours(9, i)[0]], plain[i], plain[R.neighbours(9, i)[1]], 0.02))
                                                   for i in range(9)]).astype(np.uint16)      # the reference's mask is k / 256, asserted above
    assert any(r["above"] for r in masks["t0.02"]) and any(not r["above"] for r in masks["t0.02"])

    # the scene test
    scenes = {}
    for name in ("plain9", "cut9", "twocuts9"):
        frames, proc = clips[name], processor(ref, R.HYBRID)
        hist = [R.gray_hist(f) for f in frames]
        corr = [R.scene_correlation(frames[i - 1], frames[i]) for i in range(1, 9)]
        assert corr == [R.hist_correlation(hist[i - 1], hist[i]) for i in range(1, 9)]
        own = [i for i in range(1, 9) if proc._detect_scene_change(frames[i - 1], frames[i])]
        assert own == R.scene_changes(frames) == list(CLIPS[name][1]), (name, own, corr)
        scenes[name] = {"correlation": corr, "cuts": own}
    flat = np.full((H, W, 3), 77, np.uint8)
    assert R.scene_correlation(flat, flat) == 1.0 and not processor(ref, R.HYBRID)._detect_scene_change(flat, flat)
    scenes["flat"] = {"correlation": [1.0], "cuts": []}

    # apply_consistency with in-memory images
    driver = {}
    for clip, method, window in DRIVER_CASES:
        key = f"{clip}|{method}|w{window}"
        driver[key] = run_driver(ref, stub, clips[clip], method, window, None)
        want, cuts = R.apply_clip(clips[clip], method, window)
        assert cuts == driver[key]["scene_changes_detected"] and driver[key]["sha256"] == [sha(w) for w in want], key
        assert driver[key]["frames_processed"] == len(want) and driver[key]["frames_failed"] == 0
        assert [sha(w) for w in R.stream_clip(clips[clip], method, window)] == driver[key]["sha256"], key
        if key in NPZ_DRIVER_CASES:
            npz[f"output|driver|{key}"] = np.stack(want)
    driver["plain9|hybrid|w7|none3"] = run_driver(ref, stub, clips["plain9"], R.HYBRID, 7, 3)
    assert driver["plain9|hybrid|w7|none3"]["frames_failed"] == 3          # the unreadable frame and both its neighbours

    # the value types
    cfg = ref.CrossAttentionConfig()
    plainv = lambda v: v.value if isinstance(v, ref.TemporalMethod) else v        # noqa: E731
    defaults = {k: plainv(v) for k, v in cfg.__dict__.items()}
    rejected = []
    for bad in ({"attention_window": 0}, {"blend_strength": -0.1}, {"blend_strength": 1.5}, {"method": "rife"}):
        try:
            ref.CrossAttentionConfig(**bad)
            raise AssertionError(bad)
        except ValueError as e:
            rejected.append([bad, str(e)])
    accepted = [{"method": "optical_flow"}, {"method": "hybrid"}, {"attention_window": 1}, {"blend_strength": 0.0}, {"blend_strength": 1.0}]
    for good in accepted:
        ref.CrossAttentionConfig(**good)
    enums = {"TemporalMethod": {m.name: m.value for m in ref.TemporalMethod}}
    created = {k: plainv(v) for k, v in ref.create_temporal_processor("optical_flow", 5, 0.25, 1).config.__dict__.items()}
    result_defaults = {k: (None if v is None else v) for k, v in ref.TemporalConsistencyResult().__dict__.items()}

    # the restorer's own driver
    restorer = {}
    for name, call in (("window_size", lambda: ref.CrossAttentionConfig(method=ref.TemporalMethod.HYBRID, window_size=7, blend_strength=0.5)),
                       ("processed_frames", lambda: ref.TemporalConsistencyResult(processed_frames=0)),
                       ("method_used", lambda: ref.TemporalConsistencyResult(method_used="hybrid"))):
        try:
            call()
            raise AssertionError(name)
        except TypeError as e:
            restorer[name] = f"TypeError: {e}"
    restorer["process_frame"] = hasattr(ref.CrossAttentionTemporalProcessor, "process_frame")
    assert restorer["process_frame"] is False
    text_path = Path(sys.argv[1]).resolve().parent.parent / "restorer.py"
    if text_path.exists():
        text = text_path.read_text()
        found = re.search(r"temporal_blend_strength'\s*,\s*([0-9.]+)", text)
        restorer["default_blend_strength"] = float(found.group(1))
        restorer["passes_window_size"] = "window_size=" in text
        restorer["calls_process_frame"] = "processor.process_frame(" in text
        assert restorer["default_blend_strength"] == 0.5 and restorer["passes_window_size"] and restorer["calls_process_frame"]

    js = {"numpy": np.__version__, "height": H, "width": W, "defaults": defaults, "rejected": rejected, "accepted": accepted, "enums": enums,
          "created": created, "result_defaults": result_defaults, "restorer": restorer, "clips": {k: [v[0], list(v[1]), [sha(f) for f in clips[k]]] for k, v in CLIPS.items()},
          "hold_back": {str(w): R.stream_hold_back(w) for w in (1, 3, 7)}, "scenes": scenes, "masks": masks, "driver": driver}
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"), default=str)        # noqa: E731 - one line per case
    head = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js.items())
    body = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in frame_cases.items())
    (out_dir / "temporal_consistency_reference.json").write_text(f'{{{head},\n"cases":{{\n{body}\n}}\n}}\n')
    np.savez_compressed(out_dir / "temporal_consistency_reference.npz", **npz)
    for name in ("temporal_consistency_reference.json", "temporal_consistency_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")
    print(len(frame_cases), "frame cases,", len(driver), "driver cases")


def run_driver(ref, stub, frames, method, window, none_at):
    """The reference's `apply_consistency` on a directory of name-only files, the images handed over in memory."""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in", Path(tmp) / "out"
        src.mkdir()
        names = [f"frame_{i:08d}.png" for i in range(len(frames))]
        images = dict(zip(names, frames))
        for n in names:
            (src / n).write_bytes(n.encode())
        written, progress, messages = {}, [], []
        stub.imread = lambda p: None if none_at is not None and Path(p).name == names[none_at] else images[Path(p).name]
        stub.imwrite = lambda p, img: written.__setitem__(Path(p).name, img)
        proc = processor(ref, method, window)
        handler = logging.Handler()
        handler.emit = lambda rec: messages.append(rec.getMessage())
        logging.disable(logging.NOTSET)
        ref.logger.addHandler(handler)
        try:
            res = proc.apply_consistency(src, dst, progress.append)
        finally:
            ref.logger.removeHandler(handler)
            logging.disable(logging.CRITICAL)
        return {"method": method, "attention_window": window, "frames_processed": res.frames_processed, "frames_failed": res.frames_failed,
                "flicker_regions_fixed": res.flicker_regions_fixed, "scene_changes_detected": list(res.scene_changes_detected),
                "written": "all" if sorted(written) == names else sorted(written),
                "copied": "all" if sorted(p.name for p in dst.iterdir()) == names else sorted(p.name for p in dst.iterdir()), "progress": progress,
                "failed": sum(m.startswith("Failed") for m in messages), "skipped": sum(m.startswith("Skipping") for m in messages),
                "sha256": [sha(written[n]) if n in written else None for n in names]}


if __name__ == "__main__":
    main()
