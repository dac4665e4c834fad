"""GPU: the perceptual tuner in `DeviceRestorationPipeline` (pipeline.py), behind the temporal-consistency pass and in front of the
colour grade, in `run_device`, `run`, `stream_device` and `run_stream`.  A three-frame 24 x 40 clip: the pipeline with the stage equals
the stages applied by hand in the documented order, the streaming forms equal `run_device`, and without the stage nothing changes."""
import numpy as np
import pytest

import perceptual_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as CG
from framewright_amd import perceptual as PT
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
    return [R.content_frame(24, 40, seed) for seed in (0, 1, 2)]


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


@pytest.mark.parametrize("mode", ["balanced", "enhanced"])
def test_the_pipeline_equals_the_stages_by_hand(torch_mod, clip, mode):
    tuner = PT.create_perceptual_tuner(mode)
    rcfg = R.PerceptualConfig(mode=R.PerceptualMode(mode), balance={"balanced": 0.5, "enhanced": 1.0}[mode])
    want = [R.apply_to_frame(f, rcfg) for f in clip]
    assert all(not np.array_equal(w, f) for w, f in zip(want, clip))
    p = DeviceRestorationPipeline(perceptual_tuner=tuner)
    assert tuner in p._stages()
    assert same(host(p.run_device(clip)), want) and same(p.run(clip), want)
    for block in (1, 2):
        assert same(host(p.stream_device(iter(clip), block=block)), want)
    writer = Writer()
    assert p.run_stream(iter(clip), writer, block=2) == 3 and same(writer.frames, want)
    # the documented order: temporal consistency, the tuner, the colour grade
    stage = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="optical_flow", attention_window=3))
    grader = CG.DeviceColorGrader(CG.create_seasonal_lut("winter"))
    dev = [torch_mod.from_numpy(f).cuda() for f in clip]
    by_hand = host(grader.apply_device(tuner.apply_device(stage.apply_device(dev))))
    full = DeviceRestorationPipeline(temporal_consistency=stage, perceptual_tuner=tuner, color_grader=grader)
    assert same(host(full.run_device(clip)), by_hand) and same(host(full.stream_device(iter(clip), block=2)), by_hand)
    other_order = host(tuner.apply_device(grader.apply_device(stage.apply_device(dev))))
    assert not same(by_hand, other_order)
    full.close()
    with pytest.raises(ValueError, match="the tuner is closed"):
        tuner.apply_device(dev)


def test_without_the_stage_nothing_changes(torch_mod, clip):
    grader = CG.DeviceColorGrader(CG.create_seasonal_lut("winter"))
    before = host(DeviceRestorationPipeline(color_grader=grader).run_device(clip))
    p = DeviceRestorationPipeline(color_grader=grader, perceptual_tuner=None)
    assert p.perceptual_tuner is None
    for got in (host(p.run_device(clip)), p.run(clip), host(p.stream_device(iter(clip), block=2))):
        assert same(got, before)
