"""GPU: the HDR converter as the last step of `DeviceRestorationPipeline` (pipeline.py), behind the colour grade, in `run_device`, `run`,
`stream_device` and `run_stream`.  The chain is the smallest with a seam in front of it: a x2 upscaler with synthetic weights and the
colour grade, so the converter sees frames the pipeline made.  Exact equality with converting the pipeline's 8-bit output afterwards."""
import numpy as np
import pytest

import hdr_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G
from framewright_amd import hdr as H
from framewright_amd import realesrgan as SR
from framewright_amd.pipeline import DeviceRestorationPipeline
from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state

pytestmark = pytest.mark.gpu


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
    return list(synthetic_frames(4, 40, 56, seed=35))


def host16(torch, frames):
    torch.cuda.synchronize()
    return [t.view(torch.int16).cpu().numpy().view(np.uint16) for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def test_the_converter_is_the_last_step_in_every_run_form(torch_mod, stages, clip):
    plain = DeviceRestorationPipeline(**stages)
    before = plain.run_device(clip)
    assert all(t.dtype == torch_mod.uint8 for t in before) and before[0].shape == (80, 112, 3)
    conv = H.DeviceHDRConverter(H.HDRConfig(tone_mapping="hable", peak_brightness=600))
    want = host16(torch_mod, conv.convert_device(before))
    assert same(want, [R.convert_frame(t.cpu().numpy(), conv.config) for t in before])
    p = DeviceRestorationPipeline(hdr_converter=conv, **stages)
    out = p.run_device(clip)
    assert all(t.dtype == torch_mod.uint16 for t in out) and same(host16(torch_mod, out), want)
    got = p.run(clip)
    assert same([a.view(np.uint16) if a.dtype != np.uint16 else a for a in got], want)
    for block in (1, 3):
        assert same(host16(torch_mod, list(p.stream_device(iter(clip), block=block))), want)

    class Writer:
        def __init__(self):
            self.frames = []

        def write(self, array, ready=None, release=None):
            ready()
            self.frames.append(array.copy())
            release()

    writer = Writer()
    assert p.run_stream(iter(clip), writer, block=2) == 4
    assert same([a.view(np.uint16) for a in writer.frames], want)
    # without the argument nothing changes: the same 8-bit frames, and no converter in the stage tuple
    again = DeviceRestorationPipeline(**stages)
    assert again.hdr_converter is None and same([t.cpu().numpy() for t in again.run_device(clip)], [t.cpu().numpy() for t in before])


def test_repeated_frames_and_the_converter_as_the_only_stage(torch_mod, clip):
    conv = H.DeviceHDRConverter()
    p = DeviceRestorationPipeline(hdr_converter=conv)                 # its device is the pipeline's
    t = torch_mod.from_numpy(clip[0]).cuda()
    out = p.run_device([t, t, clip[1], t])                            # one tensor several times in the list
    want = [R.convert_frame(f, conv.config) for f in (clip[0], clip[0], clip[1], clip[0])]
    assert same(host16(torch_mod, out), want) and len({o.data_ptr() for o in out}) == 4
    assert same(host16(torch_mod, list(p.stream_device(iter([t, t, clip[1], t])))), want)


def test_close_releases_the_stage(torch_mod, clip):
    conv = H.DeviceHDRConverter()
    p = DeviceRestorationPipeline(hdr_converter=conv)
    assert conv.is_available() and p.run_device(clip[:1])[0].dtype == torch_mod.uint16
    p.close()
    assert not conv.is_available() and conv._tail is None and conv._scratch is None
    with pytest.raises(ValueError, match="hdr: the converter is closed"):
        p.run_device(clip[:1])
