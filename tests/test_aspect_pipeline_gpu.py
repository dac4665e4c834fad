"""GPU: the aspect handler in `DeviceRestorationPipeline` (pipeline.py): the bar crop behind the deinterlacer and the VHS processor and in
front of every other stage, the conversion behind the colour grade."""
import numpy as np
import pytest

import aspect_ref as R
from framewright_amd import _lib
from framewright_amd import aspect as A
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
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def handler(method="pad", fill="mirror"):
    return R.handler_for(method, fill, A.DeviceAspectHandler, A.AspectConfig, A.ConversionMethod, A.FillMode)


@pytest.mark.parametrize("name", ["letterbox/48x64", "long/37x33", "plain/48x64"])
def test_pipeline_equals_crop_then_pipeline_then_convert(torch_mod, grader, name):
    clip = CLIPS[name]
    asp = handler()
    deint = D.create_deinterlacer("yadif", "tff")
    vhs = V.DeviceVHSProcessor()
    np.random.seed(21)
    front = vhs.process(deint.deinterlace([torch_mod.from_numpy(f).cuda() for f in clip]))
    cropped = asp.crop_letterbox(front)
    graded = DeviceRestorationPipeline(color_grader=grader).run_device(cropped)
    want = host(asp.convert_aspect(graded, "16:9"))
    assert want[0].shape[1] == int(want[0].shape[0] * (16 / 9)) or want[0].shape[0] == int(want[0].shape[1] / (16 / 9))
    p = DeviceRestorationPipeline(color_grader=grader, deinterlacer=deint, vhs_processor=vhs, aspect_handler=asp, aspect_target="16:9")
    np.random.seed(21)
    assert same(host(p.run_device(clip)), want)
    for block in (1, 2, 5):
        np.random.seed(21)
        assert same(host(p.stream_device(iter(clip), block=block)), want)
    # the crop alone, the conversion alone
    only_crop = DeviceRestorationPipeline(color_grader=grader, aspect_handler=asp)
    assert same(host(only_crop.run_device(clip)), host(DeviceRestorationPipeline(color_grader=grader).run_device(
        R.AspectHandler().crop_letterbox(clip))))
    only_convert = DeviceRestorationPipeline(color_grader=grader, aspect_handler=asp, aspect_target=2.0, crop_bars=False)
    uncropped = host(DeviceRestorationPipeline(color_grader=grader).run_device(clip))
    assert same(host(only_convert.run_device(clip)), R.handler_for("pad", "mirror").convert_aspect(uncropped, 2.0))
    assert same(host(only_convert.stream_device(iter(clip), block=2)), R.handler_for("pad", "mirror").convert_aspect(uncropped, 2.0))


def test_the_handler_as_the_only_stage(torch_mod):
    clip = CLIPS["edge_found/48x64"]
    asp = handler("fit", "black")
    alone = DeviceRestorationPipeline(aspect_handler=asp, aspect_target="4:3")          # its device is the pipeline's
    ref = R.handler_for("fit", "black")
    want = ref.convert_aspect(ref.crop_letterbox(clip), "4:3")
    assert same(host(alone.run_device(clip)), want)
    assert same(host(alone.stream_device(iter(clip), block=2)), want)
    assert same(alone.run(clip), want)


def test_none_changes_nothing(torch_mod, grader):
    clip = CLIPS["letterbox/48x64"]
    before = host(DeviceRestorationPipeline(color_grader=grader).run_device(clip))
    for p in (DeviceRestorationPipeline(color_grader=grader, aspect_handler=None),
              DeviceRestorationPipeline(color_grader=grader, aspect_handler=None, aspect_target="16:9", crop_bars=True),
              DeviceRestorationPipeline(color_grader=grader, aspect_handler=handler(), crop_bars=False)):
        for got in (host(p.run_device(clip)), host(p.stream_device(iter(clip), block=2))):
            assert same(got, before)
