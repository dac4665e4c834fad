"""GPU: the deinterlacer as the first stage of `DeviceRestorationPipeline` (pipeline.py)."""
import numpy as np
import pytest

import deinterlace_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G
from framewright_amd import deinterlace as D
from framewright_amd.pipeline import DeviceRestorationPipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def clip():
    return R.noise_clip(4, 32, 48, 3, 21)


@pytest.fixture(scope="module")
def grader(torch_mod):
    return G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, 9))


def host(frames):
    return [t.cpu().numpy() for t in frames]


def test_none_changes_nothing(torch_mod, clip, grader):
    before = host(DeviceRestorationPipeline(color_grader=grader).run_device(clip))
    p = DeviceRestorationPipeline(color_grader=grader, deinterlacer=None)
    for got in (host(p.run_device(clip)), host(p.stream_device(iter(clip), block=2))):
        assert len(got) == len(before) and all(np.array_equal(a, b) for a, b in zip(got, before))


@pytest.mark.parametrize("method", ["bwdif", "yadif", "bob"])
def test_stream_equals_run_device_and_the_contract(torch_mod, clip, grader, method):
    d = D.create_deinterlacer(method, "tff")
    alone = DeviceRestorationPipeline(deinterlacer=d)
    whole = host(alone.run_device(clip))
    want = R.deinterlace(clip, method, "tff")
    assert len(whole) == len(want) and all(np.array_equal(a, b) for a, b in zip(whole, want))
    streamed = host(alone.stream_device(iter(clip), block=2))
    assert len(streamed) == len(whole) and all(np.array_equal(a, b) for a, b in zip(streamed, whole))
    both = DeviceRestorationPipeline(color_grader=grader, deinterlacer=d)
    graded = host(both.run_device(clip))
    assert all(np.array_equal(a, b) for a, b in zip(graded, host(grader.apply_device([torch_mod.from_numpy(f).cuda() for f in want]))))
    streamed = host(both.stream_device(iter(clip), block=2))
    assert len(streamed) == len(graded) and all(np.array_equal(a, b) for a, b in zip(streamed, graded))


def test_auto_is_refused_in_the_stream_forms(torch_mod, clip):
    p = DeviceRestorationPipeline(deinterlacer=D.create_deinterlacer("bwdif", "auto"))
    with pytest.raises(ValueError):
        list(p.stream_device(iter(clip), block=2))

    class Writer:
        def write(self, *a, **k):
            raise AssertionError("nothing is written")

    with pytest.raises(ValueError):
        p.run_stream(iter(clip), Writer(), block=2)
    assert len(p.run_device(clip)) == len(clip)                     # the whole-clip form resolves AUTO from the clip
