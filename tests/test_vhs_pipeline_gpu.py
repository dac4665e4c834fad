"""GPU: the VHS processor behind the deinterlacer and in front of every other stage of `DeviceRestorationPipeline` (pipeline.py)."""
import numpy as np
import pytest

import vhs_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G
from framewright_amd import deinterlace as D
from framewright_amd import vhs as V
from framewright_amd.pipeline import DeviceRestorationPipeline

pytestmark = pytest.mark.gpu
CLIPS = R.clips()


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def grader(torch_mod):
    return G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, 9))


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["mix_low/48x64", "mix_high/37x33", "chroma5/37x33", "mix_low/32x8", "mix_low/37x33/gray"])
@pytest.mark.parametrize("block", [1, 2, 5])
def test_stream_equals_the_list_form(torch_mod, name, block):
    clip = CLIPS[name]
    dev = [torch_mod.from_numpy(f).cuda() for f in clip]
    p = V.DeviceVHSProcessor()
    np.random.seed(11)
    whole = host(p.process(dev))
    np.random.seed(11)
    assert same(whole, R.process(clip, R.Config()))
    np.random.seed(11)
    assert same(host(p.stream(iter(dev), block=block)), whole)


def test_stream_with_a_short_radius_and_long_list(torch_mod):
    base = CLIPS["mix_low/37x33"]
    clip = [base[(3 * i) % 5] for i in range(11)]
    dev = [torch_mod.from_numpy(f).cuda() for f in clip]
    for radius in (0, 1, 3):
        p = V.DeviceVHSProcessor(V.VHSConfig(temporal_radius=radius, rainbow_removal=0.9))
        np.random.seed(3)
        whole = host(p.process(dev))
        np.random.seed(3)
        assert same(whole, R.process(clip, R.Config(temporal_radius=radius, rainbow_removal=0.9)))
        for block in (1, 4):
            np.random.seed(3)
            assert same(host(p.stream(iter(dev), block=block)), whole)


def test_pipeline_equals_processor_then_pipeline(torch_mod, grader):
    clip = CLIPS["mix_low/48x64"]
    vhs = V.DeviceVHSProcessor()
    deint = D.create_deinterlacer("yadif", "tff")
    np.random.seed(21)
    first = vhs.process(deint.deinterlace([torch_mod.from_numpy(f).cuda() for f in clip]))
    want = host(DeviceRestorationPipeline(color_grader=grader).run_device(first))
    p = DeviceRestorationPipeline(color_grader=grader, deinterlacer=deint, vhs_processor=vhs)
    np.random.seed(21)
    assert same(host(p.run_device(clip)), want)
    for block in (1, 2, 5):
        np.random.seed(21)
        assert same(host(p.stream_device(iter(clip), block=block)), want)
    alone = DeviceRestorationPipeline(vhs_processor=vhs)               # the only stage: its device is the pipeline's
    np.random.seed(21)
    whole = host(alone.run_device(clip))
    np.random.seed(21)
    assert same(whole, R.process(clip, R.Config()))
    np.random.seed(21)
    assert same(host(alone.stream_device(iter(clip), block=2)), whole)


def test_none_changes_nothing(torch_mod, grader):
    clip = CLIPS["mix_low/48x64"]
    before = host(DeviceRestorationPipeline(color_grader=grader).run_device(clip))
    p = DeviceRestorationPipeline(color_grader=grader, vhs_processor=None)
    for got in (host(p.run_device(clip)), host(p.stream_device(iter(clip), block=2))):
        assert same(got, before)
