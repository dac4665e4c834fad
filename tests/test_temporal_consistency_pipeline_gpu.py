"""GPU: the temporal-consistency stage in `DeviceRestorationPipeline` (pipeline.py), behind the interpolation and in front of the
colour grade, in `run_device`, `run`, `stream_device` and `run_stream`.  40 x 70 frames of a flickering clip with a cut, one x2 pass of
an interpolator stub that averages its two frames on the device (so the host can say what the stage is handed): the pipeline with the
stage equals the restatement applied to the stage-less output, the grade sees the stage's frames, the streaming forms equal
`run_device`, and without the stage nothing changes."""
import numpy as np
import pytest

import temporal_consistency_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as CG
from framewright_amd import temporal_consistency as TC
from framewright_amd.pipeline import DeviceRestorationPipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def clip():
    return R.flicker_clip(7, 40, 70, 77, (4,))


class Interpolator:
    """The mean of its two frames, rounded down, in the shape of `IFNetEngine`."""
    device_id = 0

    def interpolate_device(self, a, b):
        return (a & b) + ((a ^ b) >> 1)


def mid(a, b):
    return ((a.astype(np.uint16) + b) >> 1).astype(np.uint8)


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


class Writer:
    def __init__(self):
        self.frames = []

    def write(self, array, ready=None, release=None):
        ready()
        self.frames.append(array.copy())
        release()


@pytest.mark.parametrize("method,window", [("optical_flow", 3), ("hybrid", 7)])
def test_the_pipeline_equals_the_restatement_on_the_stage_less_output(torch_mod, clip, method, window):
    stage = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method=method, attention_window=window))
    grader = CG.DeviceColorGrader(CG.create_seasonal_lut("winter"))
    interp = Interpolator()
    before = host(DeviceRestorationPipeline(interpolator=interp).run_device(clip))
    by_hand = [clip[0]]
    for a, b in zip(clip, clip[1:]):
        by_hand += [mid(a, b), b]
    assert len(before) == 13 and same(before, by_hand)
    want, cuts = R.apply_clip(before, method, window)
    # the mean across the cut correlates with neither scene: two cuts closer than the window; and the stage has changed frames
    assert cuts == [7, 8] and sum(not np.array_equal(w, b) for w, b in zip(want, before)) >= 3
    p = DeviceRestorationPipeline(interpolator=interp, temporal_consistency=stage)
    assert stage in p._stages()
    assert same(host(p.run_device(clip)), want) and same(p.run(clip), want)
    for block in (1, 3):
        assert same(host(p.stream_device(iter(clip), block=block)), want)
    writer = Writer()
    assert p.run_stream(iter(clip), writer, block=2) == 13 and same(writer.frames, want)
    # with the grade behind it: the grade is handed the stage's frames
    graded = host(grader.apply_device([torch_mod.from_numpy(w).cuda() for w in want]))
    g = DeviceRestorationPipeline(interpolator=interp, temporal_consistency=stage, color_grader=grader)
    assert same(host(g.run_device(clip)), graded) and same(host(g.stream_device(iter(clip), block=2)), graded)
    assert not same(graded, host(DeviceRestorationPipeline(interpolator=interp, color_grader=grader).run_device(clip)))
    alone = DeviceRestorationPipeline(temporal_consistency=stage)       # its device is the pipeline's
    assert same(host(alone.run_device(clip)), R.apply_clip(clip, method, window)[0])
    g.close()
    assert not stage.is_available()


def test_without_the_stage_nothing_changes(torch_mod, clip):
    interp = Interpolator()
    grader = CG.DeviceColorGrader(CG.create_seasonal_lut("winter"))
    before = host(DeviceRestorationPipeline(interpolator=interp, color_grader=grader).run_device(clip))
    p = DeviceRestorationPipeline(interpolator=interp, color_grader=grader, temporal_consistency=None)
    assert p.temporal_consistency is None
    for got in (host(p.run_device(clip)), p.run(clip), host(p.stream_device(iter(clip), block=2))):
        assert same(got, before)
