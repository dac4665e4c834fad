"""GPU: the artifact remover behind the bar crop and in front of the denoiser of `DeviceRestorationPipeline` (pipeline.py), in
`run_device`, `run`, `stream_device` and `run_stream`.  24 x 40 frames; the crop, the denoiser and the upscaler are stubs that record
what they were handed, so the position of the stage in the chain is what is tested, byte for byte against tests/qp_artifact_ref.py."""
import numpy as np
import pytest

import qp_artifact_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G
from framewright_amd import qp_artifacts as Q
from framewright_amd.pipeline import DeviceRestorationPipeline

pytestmark = pytest.mark.gpu
QP = 34


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def clip():
    return [R.content_frame(28, 40, 20 + i) for i in range(5)]


class Crop:
    """Two rows off the top and the bottom, in the shape of `DeviceAspectHandler.crop_letterbox` / `.stream`."""

    def crop_letterbox(self, frames):
        return [f[2:-2].contiguous() for f in frames]

    def stream(self, frames, block=8):
        for f in frames:
            yield f[2:-2].contiguous()


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


class Upscaler:
    def upscale_device(self, f):
        return f.repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous()


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def cleaned(clip, config, qp=QP):
    return [R.process_frame(f[2:-2], qp, config, (config.seed, i)) for i, f in enumerate(clip)]


def test_the_stage_runs_behind_the_crop_and_in_front_of_the_denoiser(torch_mod, clip):
    rem = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(seed=4))
    den = Denoiser()
    p = DeviceRestorationPipeline(denoiser=den, upscaler=Upscaler(), aspect_handler=Crop(), artifact_remover=rem, artifact_qp=QP)
    assert rem in p._stages()
    want_in = cleaned(clip, rem.config)
    want = [np.repeat(np.repeat(255 - f, 2, axis=0), 2, axis=1) for f in want_in]
    out = host(p.run_device(clip))
    assert same(den.seen, want_in) and same(out, want) and out[0].shape == (48, 80, 3)
    assert same(p.run(clip), want)
    for block in (1, 3):
        den.seen = []
        assert same(host(p.stream_device(iter(clip), block=block)), want) and same(den.seen, want_in)

    class Writer:
        def __init__(self):
            self.frames = []

        def write(self, array, ready=None, release=None):
            ready()
            self.frames.append(array.copy())
            release()

    writer = Writer()
    assert p.run_stream(iter(clip), writer, block=2) == 5 and same(writer.frames, want)


def test_the_qp_falls_back_and_the_remover_alone_names_the_device(torch_mod, clip):
    rem = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(manual_qp=40, artifact_types=[Q.ArtifactType.BLOCKING, Q.ArtifactType.BANDING]))
    alone = DeviceRestorationPipeline(artifact_remover=rem)                       # its device is the pipeline's
    want = [R.process_frame(f, 40, rem.config, (0, i)) for i, f in enumerate(clip)]
    assert same(host(alone.run_device(clip)), want) and same(host(alone.stream_device(iter(clip), block=2)), want)
    t = torch_mod.from_numpy(clip[0]).cuda()
    out = alone.run_device([t, t])                                                # one tensor twice: two dithers, two new tensors
    assert len({o.data_ptr() for o in out} | {t.data_ptr()}) == 3 and np.array_equal(t.cpu().numpy(), clip[0])
    assert same(host(out), [R.process_frame(clip[0], 40, rem.config, (0, i)) for i in range(2)])


def test_without_the_stage_nothing_changes(torch_mod, clip):
    grader = G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, 9))
    stages = dict(denoiser=Denoiser(), upscaler=Upscaler(), aspect_handler=Crop(), color_grader=grader)
    before = host(DeviceRestorationPipeline(**stages).run_device(clip))
    p = DeviceRestorationPipeline(artifact_remover=None, artifact_qp=40, **stages)
    assert p.artifact_remover is None
    for got in (host(p.run_device(clip)), host(p.stream_device(iter(clip), block=2))):
        assert same(got, before)
    want = [np.repeat(np.repeat(255 - f[2:-2], 2, axis=0), 2, axis=1) for f in clip]
    assert same(before, host(grader.apply_device([torch_mod.from_numpy(f).cuda() for f in want])))


def test_close_reaches_the_stage(torch_mod, clip):
    rem = Q.DeviceQPArtifactRemover()
    p = DeviceRestorationPipeline(artifact_remover=rem)
    assert rem.is_available() and p.run_device(clip[:1])[0].shape == (28, 40, 3) and rem._scratch is not None
    p.close()
    assert not rem.is_available() and rem._scratch is None and rem._tables == {}
    with pytest.raises(ValueError, match="qp_artifacts: the remover is closed"):
        p.run_device(clip[:1])
