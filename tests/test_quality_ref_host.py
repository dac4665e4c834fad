"""tests/quality_ref.py against what tools/gen_quality_golden.py recorded from the reference's own scorer (CPU only).

Every field, issue list, report field and recommendation is equal to the record; the sharpness and noise scores and what is formed
from them (the overall score, `issue_details`, the report's average, minimum and maximum) are held within the float bound that
DESIGN K19 derives (`quality_ref.score_tolerances`), the corrupted test by its margin from the threshold."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import quality_ref as R  # noqa: E402

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "quality_reference.json").read_text())
CLIPS = R.clips()


def pixels(clip) -> int:
    return clip["frames"][0].shape[0] * clip["frames"][0].shape[1] if clip["frames"] else 0


def test_the_record_covers_every_clip_and_reaches_its_cases():
    assert sorted(GOLDEN["clips"]) == sorted(CLIPS)
    R.reached(GOLDEN)


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_restatement_equals_the_record(name):
    clip, rec = CLIPS[name], GOLDEN["clips"][name]
    scorer = R.FrameQualityScorer(**R.scorer_arguments(clip))
    if clip.get("raises"):
        assert rec["raises"] == "ValueError"
        with pytest.raises(ValueError):
            scorer.analyze_frames(clip["frames"], clip["fps"])
        return
    scores, inner = [], scorer.score_frame
    scorer.score_frame = lambda *a: scores.append(inner(*a)) or scores[-1]
    seen = []
    scorer.progress_callback = lambda k, end: seen.append(k)
    report = scorer.analyze_frames(clip["frames"], clip["fps"], video_path=name, **R.loop_arguments(clip))
    assert len(scores) == len(rec["scores"]) and seen == [r["frame_number"] for r in rec["scores"]]
    for got, want in zip(scores, rec["scores"]):
        R.assert_score_matches(got, want, pixels(clip))
    R.assert_report_matches(report, rec["report"], pixels(clip))
    assert report.to_dict()["problem_frame_count"] == len(rec["report"]["problem_frames"])
    assert [f.frame_number for f in report.get_frames_with_issue(R.QualityIssue.DUPLICATE)] == \
        [r["frame_number"] for r in rec["scores"] if "duplicate" in r["issues"]]
    assert [R.statistics_digest(R.frame_statistics(f)) for f in clip["frames"]] == rec["statistics_sha256"]


@pytest.mark.parametrize("name", sorted(n for n, c in CLIPS.items() if not c.get("raises")))
def test_scores_are_a_function_of_the_integers(name):
    clip, rec = CLIPS[name], GOLDEN["clips"][name]
    k, prev = R.FrameQualityScorer(**R.scorer_arguments(clip)), None
    collector = R.ReportCollector(k, name, rec["report"]["total_frames"])
    for want in rec["scores"]:
        got, prev = R.score_from_statistics(k, R.frame_statistics(clip["frames"][want["frame_number"]]), prev, want["frame_number"], clip["fps"])
        R.assert_score_matches(got, want, pixels(clip))
        collector.add(got)
    R.assert_report_matches(collector.report(), rec["report"], pixels(clip))


def test_float_bound_holds_numpy_against_the_exact_rational():
    rng = np.random.default_rng(3)
    for n, scale in ((7, 3), (4096, 1020), (200_000, 255), (1 << 20, 1020)):
        x = rng.integers(-scale if scale > 255 else 0, scale + 1, n).astype(np.int64)
        s1, s2 = int(x.sum()), int((x * x).sum())
        var, std = R.exact_variance(n, s1, s2), R.exact_std(n, s1, s2)
        assert abs(float(np.var(x.astype(np.float64))) - var) <= R.var_bound(n, var, s1 / n)
        assert abs(float(np.std(x.astype(np.float64))) - std) <= R.std_bound(n, std, s1 / n)
    assert R.exact_std(4, 10, 30) == math.sqrt(5) / 2 and R.exact_variance(4, 10, 30) == 1.25
    assert R.var_bound(1 << 28, 1.0) < 64 * R.U                       # a few dozen roundings, not N of them


def test_report_helpers_and_save(tmp_path):
    clip = CLIPS["issues/48x64"]
    report = R.FrameQualityScorer().analyze_frames(clip["frames"], clip["fps"], video_path="clip")
    worst = report.get_worst_frames(2)
    assert len(worst) == 2 and worst[0].overall_score <= worst[1].overall_score == sorted(f.overall_score for f in report.problem_frames)[1]
    report.average_score = float(report.average_score)
    report.save(tmp_path / "r.json")
    assert json.loads((tmp_path / "r.json").read_text())["problem_frame_count"] == len(report.problem_frames)
    assert report.problem_frames[-1].is_problematic in (True, False) and report.problem_frames[0].has_issues
