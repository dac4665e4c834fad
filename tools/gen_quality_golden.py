#!/usr/bin/env python3
"""Writes tests/golden/quality_reference.json from the reference's own `processors/frame_quality_scorer.py`:

    python tools/gen_quality_golden.py /path/to/reference/src/framewright/processors/frame_quality_scorer.py

The reference imports cv2, which is absent here.  A stub module named `cv2` in `sys.modules` maps the calls of its frame path to what
tests/quality_ref.py says they mean (the 14-bit gray, the gamma Lab of tests/flicker_ref, the cross Laplacian, the 1 4 6 4 1 blur, the
two Sobel products, a float32 histogram, oracle/face_ref's linear resize, absdiff on uint8), so cv2's own bytes stay unpinned, as
everywhere in this project, and everything else - the measures, their thresholds, the duplicate state, the loop of `analyze_video`
over a stub `VideoCapture` that hands out the fixture frames, the report and its recommendations - is the reference's own code running.

Recorded for every clip of `quality_ref.clips()`: each analysed frame's `FrameScore` fields (floats by `repr`), issue list and
`issue_details`, the report's fields, and a digest of `frame_statistics` of every frame.  The generator asserts that quality_ref equals
the reference on all of it, that the scores formed from the integers alone stay within the float bound, that every thresholded
quantity lies further from its threshold than that bound, and that the clips reach the cases they exist for.  Data only: nothing of
the reference's program text is written.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import quality_ref as R  # noqa: E402

CLIP: dict = {"frames": [], "fps": 0.0, "total": 0}                   # what the stub VideoCapture plays


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.CV_64F, stub.COLOR_BGR2GRAY, stub.COLOR_BGR2LAB = 6, 6, 44
    stub.CAP_PROP_FPS, stub.CAP_PROP_FRAME_COUNT, stub.CAP_PROP_POS_FRAMES = 5, 7, 1

    def cvt(img, code):
        return R.gray(img) if code == stub.COLOR_BGR2GRAY and img.ndim == 3 else R.flicker_ref.bgr_to_lab_gamma(img)

    def sobel(img, depth, dx, dy, ksize=3):
        assert depth == stub.CV_64F and ksize == 3 and (dx, dy) in ((1, 1), (1, 0))
        return R.sobel_xy(img) if dy else R.sobel_x(img)

    def gaussian_blur(img, ksize, sigma):
        assert tuple(ksize) == (5, 5) and sigma == 0
        return R.gaussian_blur5(img)

    def calc_hist(images, channels, mask, sizes, ranges):
        assert channels == [0] and mask is None and sizes == [256] and ranges == [0, 256]
        return R.calc_hist(images[0])

    def resize(img, size):
        assert tuple(size) == (32, 32)
        return R.thumbnail(img)

    class VideoCapture:
        def __init__(self, path):
            self.pos = 0

        def get(self, prop):
            return CLIP["fps"] if prop == stub.CAP_PROP_FPS else CLIP["total"]

        def set(self, prop, value):
            assert prop == stub.CAP_PROP_POS_FRAMES
            self.pos = int(value)

        def read(self):
            if not 0 <= self.pos < len(CLIP["frames"]):
                return False, None
            self.pos += 1
            return True, CLIP["frames"][self.pos - 1]

        def release(self):
            pass

    stub.cvtColor, stub.Sobel, stub.GaussianBlur, stub.calcHist, stub.resize = cvt, sobel, gaussian_blur, calc_hist, resize
    stub.Laplacian = lambda img, depth: R.laplacian(img)
    stub.absdiff, stub.VideoCapture = R.absdiff, VideoCapture
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_quality", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_quality"] = mod
    spec.loader.exec_module(mod)
    return mod


class Recording:
    """A scorer whose `score_frame` keeps every score it returns."""

    def __init__(self, scorer):
        self.scorer, self.scores, inner = scorer, [], scorer.score_frame

        def keep(frame, frame_number, fps):
            s = inner(frame, frame_number, fps)
            self.scores.append(s)
            return s
        scorer.score_frame = keep


def far(value: float, threshold: float, bound: float, what) -> None:
    assert abs(float(value) - threshold) > bound + 64 * R.U * abs(threshold), (what, value, threshold, bound)


def margins(k, stats: dict, score, what) -> dict:
    """Every thresholded quantity of a frame lies further from its threshold than the float bound; returns the measures."""
    m = R.measures_from_statistics(k, stats)
    n = stats["height"] * stats["width"]
    mean3 = stats["byte_sum"] / (3 * n)
    far(m["byte_std"], 1.0, R.std_bound(3 * n, m["byte_std"], mean3), (what, "std"))
    if m["corrupted"]:
        return m
    far(m["variance"], k.BLUR_THRESHOLD, R.var_bound(n, m["variance"], stats["lap_sum"] / n), (what, "variance"))
    far(m["variance"], 500.0, R.var_bound(n, m["variance"], stats["lap_sum"] / n), (what, "variance cap"))
    far(m["noise_level"], k.NOISE_THRESHOLD, R.std_bound(n, m["noise_level"], stats["noise_sum"] / n), (what, "noise"))
    far(m["noise_level"], 30.0, R.std_bound(n, m["noise_level"], stats["noise_sum"] / n), (what, "noise clamp"))
    for t in (k.BLACK_FRAME_THRESHOLD, k.OVEREXPOSED_THRESHOLD, k.UNDEREXPOSED_THRESHOLD):
        far(m["mean"], t, 0.0, (what, "mean"))
    if not m["black"]:
        far(m["clip_dark"], 0.05, 0.0, (what, "clip"))
        far(m["clip_bright"], 0.05, 0.0, (what, "clip"))
    for name, ts in (("blocking_ratio", (1, 1.5)), ("banding_ratio", (1, 2)), ("interlace_ratio", (1, 1.5))):
        for t in ts:
            far(m[name], t, 0.0, (what, name))
    far(m["mean_diff"], 10, 0.0, (what, "mean_diff"))
    tol = R.score_tolerances(R.score_record(score), n)["overall_score"]
    for t in (k.problem_threshold, 90, 70, 50, 30):
        far(score.overall_score, t, tol, (what, "overall"))
    return m


def main() -> None:
    ref = load_reference(sys.argv[1])
    assert [(i.name, i.value) for i in ref.QualityIssue] == [(i.name, i.value) for i in R.QualityIssue]
    for name in ("BLUR_THRESHOLD", "NOISE_THRESHOLD", "OVEREXPOSED_THRESHOLD", "UNDEREXPOSED_THRESHOLD", "BLACK_FRAME_THRESHOLD",
                 "DUPLICATE_THRESHOLD"):
        assert getattr(ref.FrameQualityScorer, name) == getattr(R.FrameQualityScorer, name)
    js: dict = {"numpy": np.__version__, "clips": {}}
    measures: dict = {}
    for name, c in R.clips().items():
        frames, fps = c["frames"], c["fps"]
        loop = R.loop_arguments(c)
        CLIP.update(frames=frames, fps=fps, total=loop.get("total_frames", len(frames)))
        theirs, mine = Recording(ref.FrameQualityScorer(**R.scorer_arguments(c))), Recording(R.FrameQualityScorer(**R.scorer_arguments(c)))
        window = {k: v for k, v in loop.items() if k != "total_frames"}
        if c.get("raises"):
            for run in (lambda: theirs.scorer.analyze_video(name, **window), lambda: mine.scorer.analyze_frames(frames, fps, video_path=name, **loop)):
                try:
                    run()
                    raise AssertionError(name)
                except ValueError:
                    pass
            js["clips"][name] = {"raises": "ValueError", "shape": list(frames[0].shape)}
            print(name, "ValueError", flush=True)
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            report = theirs.scorer.analyze_video(name, **window)
        my_report = mine.scorer.analyze_frames(frames, fps, video_path=name, **loop)
        rec = {"shape": list(frames[0].shape) if frames else None, "fps": fps, "scores": [R.score_record(s) for s in theirs.scores],
               "report": R.report_record(report), "statistics_sha256": [R.statistics_digest(R.frame_statistics(f)) for f in frames]}
        n = frames[0].shape[0] * frames[0].shape[1] if frames else 0
        assert rec["scores"] == [R.score_record(s) for s in mine.scores], name
        assert rec["report"] == R.report_record(my_report), (name, rec["report"], R.report_record(my_report))
        assert report.to_dict().keys() == my_report.to_dict().keys()
        assert [f.frame_number for f in report.get_worst_frames(3)] == [f.frame_number for f in my_report.get_worst_frames(3)]
        for issue in R.QualityIssue:
            assert [f.frame_number for f in report.get_frames_with_issue(ref.QualityIssue(issue.value))] == \
                [f.frame_number for f in my_report.get_frames_with_issue(issue)]
        # the scores as a function of the integers alone: within the bound of the record, and far from every threshold
        k, prev, collector = mine.scorer, None, R.ReportCollector(mine.scorer, name, my_report.total_frames)
        measures[name] = []
        for s, r in zip(theirs.scores, rec["scores"]):
            stats = R.frame_statistics(frames[s.frame_number])
            got, prev = R.score_from_statistics(k, stats, prev, s.frame_number, fps)
            R.assert_score_matches(got, r, n)
            collector.add(got)
            measures[name].append(margins(k, stats, s, (name, s.frame_number)))
        R.assert_report_matches(collector.report(), rec["report"], n)
        if theirs.scores:
            tol = R.score_tolerances({"sharpness_score": "100.0", "noise_score": "0.0"}, n)["overall_score"]
            far(report.average_score, 80, tol, (name, "average"))
            far(report.average_score, 50, tol, (name, "average"))
        js["clips"][name] = rec
        print(name, [",".join(r["issues"]) or "-" for r in rec["scores"]], rec["report"]["average_score"], flush=True)
    reached(js, measures)
    out = ROOT / "tests" / "golden" / "quality_reference.json"
    dump = lambda v: json.dumps(v, separators=(",", ":"))             # noqa: E731
    out.write_text(f'{{"numpy":{dump(js["numpy"])},\n"clips":{{\n' + ",\n".join(f"{dump(n)}:{dump(v)}" for n, v in js["clips"].items()) + "\n}}\n")
    print(out.name, out.stat().st_size, "bytes")


def reached(js: dict, measures: dict) -> None:
    """The cases the clips exist for, read off the recorded data and the measures (tests/test_quality_ref_host.py asserts the first)."""
    R.reached(js)
    flat = [m for ms in measures.values() for m in ms if not m["corrupted"]]
    assert any(m["byte_std"] < 1 for ms in measures.values() for m in ms)
    assert any(m["corrupted"] and m["byte_std"] >= 1 and m["unique"] < 10 for ms in measures.values() for m in ms)
    assert any(m["clipped"] is True for m in flat) and any(m["clipped"] is False for m in flat) and any(m["black"] for m in flat)
    for name, flag in (("blocking_ratio", 1.5), ("banding_ratio", 2)):
        v = [float(m[name]) for m in flat]
        assert any(x < 1 for x in v) and any(1 < x < flag for x in v) and any(x > flag for x in v), (name, sorted(v))
    v = [float(m["interlace_ratio"]) for m in flat]
    assert any(x < 1 for x in v) and any(x > 1.5 for x in v)


if __name__ == "__main__":
    main()
