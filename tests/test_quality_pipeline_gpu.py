"""GPU: the two quality scorers in `DeviceRestorationPipeline` (pipeline.py): the input scorer in front of the deinterlacer, the output
scorer behind the aspect conversion, in `run_device`, `run`, `stream_device` and `run_stream`.  The chain is the smallest with a seam on
either side: a x2 upscaler with synthetic weights and the colour grade, so the outputs differ from the inputs in size and content."""
import numpy as np
import pytest

import quality_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G
from framewright_amd import quality as Q
from framewright_amd import realesrgan as SR
from framewright_amd.pipeline import DeviceRestorationPipeline
from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state

pytestmark = pytest.mark.gpu
FPS = 24.0


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def stages(torch_mod):
    sr = SR.RRDBNetEngine(2, 2, "f16")
    sr.load_state_dict(synthetic_rrdbnet_state(2, 2, seed=5))
    yield {"upscaler": sr, "color_grader": G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, 9))}
    sr.close()


@pytest.fixture(scope="module")
def clip():
    frames = list(synthetic_frames(5, 40, 56, seed=33))
    frames[3] = frames[2].copy()                                     # a duplicate on the way in
    return frames


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def records(report):
    return R.report_record(report), [R.score_record(f) for f in report.problem_frames]


def scorers():
    return {"quality_scorer": Q.DeviceFrameQualityScorer(problem_threshold=101.0), "input_quality_scorer": Q.DeviceFrameQualityScorer(problem_threshold=101.0)}


def test_frames_are_untouched_and_reports_equal_analyze_frames(torch_mod, stages, clip):
    plain = DeviceRestorationPipeline(**stages)
    before = host(plain.run_device(clip))
    assert plain.last_quality_report is None and plain.last_input_quality_report is None
    p = DeviceRestorationPipeline(quality_fps=FPS, **stages, **scorers())
    out = p.run_device(clip)
    assert same(host(out), before) and out[0].shape == (80, 112, 3)
    fresh = Q.DeviceFrameQualityScorer(problem_threshold=101.0)       # every frame is a problem frame: the records hold every score
    want_in = records(fresh.analyze_frames([torch_mod.from_numpy(f).cuda() for f in clip], FPS))
    want_out = records(fresh.analyze_frames(out, FPS))
    assert records(p.last_input_quality_report) == want_in and records(p.last_quality_report) == want_out
    assert p.last_input_quality_report.analyzed_frames == 5 and p.last_quality_report.analyzed_frames == 5
    assert p.last_input_quality_report.issue_counts["duplicate"] == 1
    # the device's scores are the contract's on the same frames
    ref = R.FrameQualityScorer(problem_threshold=101.0).analyze_frames(before, FPS)
    R.assert_report_matches(p.last_quality_report, R.report_record(ref), 80 * 112)
    for got, want in zip(p.last_quality_report.problem_frames, ref.problem_frames):
        R.assert_score_matches(got, R.score_record(want), 80 * 112)
    # run: the numpy form
    assert same(p.run(clip), before) and records(p.last_quality_report) == want_out and records(p.last_input_quality_report) == want_in
    # the streaming forms
    for block in (1, 3):
        assert same(host(p.stream_device(iter(clip), block=block)), before)
        assert records(p.last_quality_report) == want_out and records(p.last_input_quality_report) == want_in

    class Writer:
        def __init__(self):
            self.frames = []

        def write(self, array, ready=None, release=None):
            ready()
            self.frames.append(array.copy())
            release()

    writer = Writer()
    p.last_quality_report = None
    assert p.run_stream(iter(clip), writer, block=2) == 5 and same(writer.frames, before)
    assert records(p.last_quality_report) == want_out and records(p.last_input_quality_report) == want_in


def test_each_scorer_alone_and_as_the_only_stage(torch_mod, stages, clip):
    before = host(DeviceRestorationPipeline(**stages).run_device(clip))
    only_out = DeviceRestorationPipeline(quality_scorer=Q.DeviceFrameQualityScorer(sample_rate=2), quality_fps=FPS, **stages)
    assert same(host(only_out.run_device(clip)), before)
    assert only_out.last_input_quality_report is None and only_out.last_quality_report.analyzed_frames == 3
    streamed = DeviceRestorationPipeline(quality_scorer=Q.DeviceFrameQualityScorer(sample_rate=2), quality_fps=FPS, **stages)
    assert same(host(streamed.stream_device(iter(clip), block=2)), before)
    assert records(streamed.last_quality_report) == records(only_out.last_quality_report)
    alone = DeviceRestorationPipeline(input_quality_scorer=Q.DeviceFrameQualityScorer(problem_threshold=101.0))     # its device is the pipeline's
    assert same(host(alone.run_device(clip)), clip) and alone.last_input_quality_report.total_frames == 5
    assert alone.last_input_quality_report.problem_frames[0].timestamp == 0          # no fps given: the reference's 0
    assert same(host(alone.stream_device(iter(clip))), clip) and alone.last_input_quality_report.analyzed_frames == 5


def test_an_abandoned_generator_reports_nothing(torch_mod, stages, clip):
    p = DeviceRestorationPipeline(quality_fps=FPS, **stages, **scorers())
    p.run_device(clip)
    assert p.last_quality_report is not None
    g = p.stream_device(iter(clip), block=2)
    first = next(g)
    assert first.shape == (80, 112, 3) and p.last_quality_report is None and p.last_input_quality_report is None
    g.close()
    assert p.last_quality_report is None
    g = p.stream_device(iter(clip), block=2)
    n = sum(1 for _ in g)
    assert n == 5 and p.last_quality_report.analyzed_frames == 5 and p.last_input_quality_report.analyzed_frames == 5
