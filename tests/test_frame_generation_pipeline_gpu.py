"""GPU: the missing-frame generator in `DeviceRestorationPipeline` (pipeline.py), behind the denoiser and in front of the upscale, in
`run_device`, `run`, `stream_device` and `run_stream`.  48 x 64 frames, a x2 RRDBNet with synthetic weights behind a denoiser stub
that records what it was handed: the pipeline with a generator equals generator-then-pipeline composed by hand, the streaming forms
equal `run_device`, and without a generator or without frame numbers nothing changes."""
import numpy as np
import pytest

import frame_generation_ref as R
from framewright_amd import _lib
from framewright_amd import frame_generation as FG
from framewright_amd import realesrgan as SR
from framewright_amd.pipeline import DeviceRestorationPipeline
from framewright_amd.synth import synthetic_rrdbnet_state

pytestmark = pytest.mark.gpu
NUMBERS, EXPECTED = (3, 4, 7, 8, 10), 12                       # gaps: 5 and 6, 9, and 11 behind the last frame


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def upscaler(torch_mod):
    sr = SR.RRDBNetEngine(2, 2, "f16")
    sr.load_state_dict(synthetic_rrdbnet_state(2, 2, seed=5))
    yield sr
    sr.close()


@pytest.fixture(scope="module")
def clip():
    return [R.grainy_frame(48, 64, 60 + n, shift=n) for n in NUMBERS]


class Denoiser:
    """255 - frame with a window of one frame, in the shape of `TAPDenoiser`; keeps what it was handed."""

    class config:
        temporal_window = 1

    def __init__(self):
        self.seen = []

    def denoise_only_device(self, frames):
        self.seen += [f.cpu().numpy() for f in frames]
        return [255 - f for f in frames]

    def denoise_clip_device(self, frames, halo_before=None, halo_after=None, denoised=None):
        return list(denoised) if denoised is not None else self.denoise_only_device(list(frames))


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["interpolate_blend", "optical_flow"])
def test_the_pipeline_equals_generator_then_pipeline_by_hand(torch_mod, upscaler, clip, model):
    gen = FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(model=model, seed=8))
    den = Denoiser()
    p = DeviceRestorationPipeline(denoiser=den, upscaler=upscaler, frame_generator=gen, expected_frames=EXPECTED)
    assert gen in p._stages()
    out = host(p.run_device(clip, NUMBERS))
    assert same(den.seen, clip)                                  # the denoiser sees the clip with its holes: the generator is behind it
    # by hand: the denoiser's frames through the generator alone, then through a pipeline that has only the upscaler
    filled, numbers = gen.fill_device([255 - torch_mod.from_numpy(f).cuda() for f in clip], NUMBERS, EXPECTED)
    assert numbers == list(range(3, 12))
    want = host(DeviceRestorationPipeline(upscaler=upscaler).run_device(filled))
    assert len(out) == 9 and out[0].shape == (96, 128, 3) and same(out, want)
    if model == "interpolate_blend":                             # and the generator's frames are the restatement's
        ref = R.fill([255 - f for f in clip], NUMBERS, EXPECTED, seed=8)[0]
        assert same(host(filled), ref)
    assert same(p.run(clip, NUMBERS), want)
    for block in (1, 3):
        assert same(host(p.stream_device(iter(clip), block=block, frame_numbers=iter(NUMBERS))), want)

    class Writer:
        def __init__(self):
            self.frames = []

        def write(self, array, ready=None, release=None):
            ready()
            self.frames.append(array.copy())
            release()

    writer = Writer()
    assert p.run_stream(iter(clip), writer, block=2, frame_numbers=NUMBERS) == 9 and same(writer.frames, want)


def test_without_a_generator_or_without_numbers_nothing_changes(torch_mod, upscaler, clip):
    stages = dict(denoiser=Denoiser(), upscaler=upscaler)
    before = host(DeviceRestorationPipeline(**stages).run_device(clip))
    assert len(before) == 5
    gen = FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(seed=8))
    with_gen = DeviceRestorationPipeline(frame_generator=gen, expected_frames=EXPECTED, **stages)
    without = DeviceRestorationPipeline(frame_generator=None, expected_frames=EXPECTED, **stages)
    for got in (host(with_gen.run_device(clip)), with_gen.run(clip), host(with_gen.stream_device(iter(clip), block=2)),
                host(without.run_device(clip, NUMBERS)), host(without.stream_device(iter(clip), block=2, frame_numbers=NUMBERS))):
        assert same(got, before)
    alone = DeviceRestorationPipeline(frame_generator=gen)       # its device is the pipeline's
    assert len(alone.run_device(clip, NUMBERS)) == 8 and len(alone.run_device(clip)) == 5


def test_close_reaches_the_generator(torch_mod, clip):
    gen = FG.DeviceMissingFrameGenerator()
    p = DeviceRestorationPipeline(frame_generator=gen)
    assert gen.is_available() and len(p.run_device(clip, NUMBERS)) == 8 and gen._scratch is not None
    p.close()
    assert not gen.is_available() and gen._scratch is None and gen._tables == {}
    with pytest.raises(ValueError, match="frame_generation: the generator is closed"):
        p.run_device(clip, NUMBERS)
