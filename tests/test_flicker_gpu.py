"""csrc/flicker.hip and the classes built on it (DeviceFlickerReducer, DeviceTemporalDenoiser(device_flicker=True)) against
tests/flicker_ref.py.  Every comparison is an equality with the restatement: the transforms and the L sums are integer arithmetic
over tables built in float64, and the maps of L are built on the host in the restatement's float64."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flicker_ref as fr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402
from framewright_amd.synth import synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _transform(hip_lib, name, pixels, in_place=False, offset=0):
    """fw_bgr_to_lab_u8 / fw_lab_to_bgr_u8 on a uint8 [N, 3] array; `offset` shifts both device buffers off their 4-byte alignment."""
    torch, dev = _torch()
    n = pixels.shape[0]
    src = torch.zeros(offset + 3 * n + 8, dtype=torch.uint8, device=dev)
    src[offset:offset + 3 * n] = torch.from_numpy(np.ascontiguousarray(pixels).reshape(-1)).to(dev)
    dst = src if in_place else torch.full_like(src, 0xAB)
    _lib.check(getattr(hip_lib, name)(C.c_void_p(src.data_ptr() + offset), n, C.c_void_p(dst.data_ptr() + offset), _stream(torch, dev)))
    torch.cuda.synchronize(dev)
    out = dst.cpu().numpy()
    if not in_place:                                         # nothing outside the n pixels is written
        assert (out[:offset] == 0xAB).all() and (out[offset + 3 * n:] == 0xAB).all()
    return out[offset:offset + 3 * n].reshape(n, 3)


# ------------------------------------------------------------------------------------------------------------- the transforms
@pytest.fixture(scope="module")
def lattice_lab():
    colours = fr.lattice()
    return colours, fr.bgr_to_lab_gamma(colours)


def test_transforms_equal_the_restatement_on_the_lattice(hip_lib, lattice_lab):
    colours, lab = lattice_lab
    assert len(np.unique(lab, axis=0)) > 100000                       # a kernel that writes a constant must not pass
    np.testing.assert_array_equal(_transform(hip_lib, "fw_bgr_to_lab_u8", colours), lab)
    np.testing.assert_array_equal(_transform(hip_lib, "fw_lab_to_bgr_u8", lab), fr.lab_to_bgr_gamma(lab))
    np.testing.assert_array_equal(_transform(hip_lib, "fw_bgr_to_lab_u8", colours, in_place=True), lab)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 257])
def test_transform_vector_tails(hip_lib, n, offset):
    rng = np.random.default_rng(100 * n + offset)
    px = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    np.testing.assert_array_equal(_transform(hip_lib, "fw_bgr_to_lab_u8", px, offset=offset), fr.bgr_to_lab_gamma(px))
    lab = fr.bgr_to_lab_gamma(px)
    np.testing.assert_array_equal(_transform(hip_lib, "fw_lab_to_bgr_u8", lab, offset=offset), fr.lab_to_bgr_gamma(lab))


def test_transform_with_differently_aligned_buffers(hip_lib):
    """Source and destination that do not share their alignment go byte by byte."""
    torch, dev = _torch()
    px = np.random.default_rng(9).integers(0, 256, (301, 3), dtype=np.uint8)
    src = torch.zeros(3 * 301 + 8, dtype=torch.uint8, device=dev)
    src[1:1 + 903] = torch.from_numpy(px.reshape(-1)).to(dev)
    dst = torch.zeros_like(src)
    _lib.check(hip_lib.fw_bgr_to_lab_u8(C.c_void_p(src.data_ptr() + 1), 301, C.c_void_p(dst.data_ptr() + 2), _stream(torch, dev)))
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(dst.cpu().numpy()[2:2 + 903].reshape(301, 3), fr.bgr_to_lab_gamma(px))


def test_library_tables_equal_the_contract_on_the_gpu_box(hip_lib):
    for which, want in enumerate([fr.gamma_tables()["decode"], fr.gamma_tables()["encode"], fr.encode_thresholds()]):
        got = np.zeros(want.size, np.int32)
        assert hip_lib.fw_gamma_lab_tables(which, C.c_void_p(got.ctypes.data), got.size) == want.size
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------- fw_lab_l_sums_u8
def _l_sums(hip_lib, frames, dirty=None):
    torch, dev = _torch()
    clip = torch.from_numpy(np.stack(frames)).to(dev)
    count, h, w = clip.shape[:3]
    sums = torch.full((count,), -12345 if dirty is None else dirty, dtype=torch.int64, device=dev)
    _lib.check(hip_lib.fw_lab_l_sums_u8(_p(clip), count, h, w, _p(sums), _stream(torch, dev)))
    torch.cuda.synchronize(dev)
    return sums.cpu().numpy().tolist()


@pytest.mark.parametrize("count", [1, 7])
@pytest.mark.parametrize("h,w", [(1, 9), (5, 3), (37, 53), (270, 480)])
def test_l_sums_equal_the_restatement(hip_lib, h, w, count):
    rng = np.random.default_rng(h * 31 + w + count)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 2 else
              np.ascontiguousarray(synthetic_frames(1, max(h, 8), max(w, 8), seed=k + h)[0, :h, :w]) for k in range(count)]
    want = [int(fr.bgr_to_lab_gamma(f)[..., 0].astype(np.int64).sum()) for f in frames]
    assert min(want) > 0 and (count == 1 or len(set(want)) == count)  # different frames, different sums
    got = _l_sums(hip_lib, frames)
    assert got == want
    assert _l_sums(hip_lib, frames, dirty=7 << 40) == want           # the call zeroes its output: a dirty buffer gives the same numbers


def test_l_sum_of_an_8k_white_frame_crosses_2_to_32(hip_lib):
    torch, dev = _torch()
    h, w = 4320, 7680
    one = int(fr.bgr_to_lab_gamma(np.full((1, 3), 255, np.uint8))[0, 0])
    assert one == 255 and one * h * w > 2 ** 32
    clip = torch.full((1, h, w, 3), 255, dtype=torch.uint8, device=dev)
    sums = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(hip_lib.fw_lab_l_sums_u8(_p(clip), 1, h, w, _p(sums), _stream(torch, dev)))
    torch.cuda.synchronize(dev)
    assert int(sums.cpu()[0]) == one * h * w


# ------------------------------------------------------------------------------------------------------------- fw_deflicker_lab_u8
def _deflicker(hip_lib, frames, luts, in_place=False):
    torch, dev = _torch()
    clip = torch.from_numpy(np.stack(frames)).to(dev)
    count, h, w = clip.shape[:3]
    out = clip if in_place else torch.full_like(clip, 0xAB)
    _lib.check(hip_lib.fw_deflicker_lab_u8(_p(clip), count, h, w, _p(torch.from_numpy(np.ascontiguousarray(luts)).to(dev)), _p(out),
                                           _stream(torch, dev)))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _deflicker_ref(frames, luts):
    out = []
    for f, lut in zip(frames, luts):
        lab = fr.bgr_to_lab_gamma(f)
        lab[..., 0] = lut[lab[..., 0]]
        out.append(fr.lab_to_bgr_gamma(lab))
    return np.stack(out)


def test_identity_lut_is_the_round_trip(hip_lib):
    frames = list(synthetic_frames(2, 37, 53, seed=8))
    luts = np.tile(np.arange(256, dtype=np.uint8), (2, 1))
    want = np.stack([fr.lab_to_bgr_gamma(fr.bgr_to_lab_gamma(f)) for f in frames])
    got = _deflicker(hip_lib, frames, luts)
    np.testing.assert_array_equal(got, want)
    # and it is the two transform entries chained
    via = _transform(hip_lib, "fw_lab_to_bgr_u8", _transform(hip_lib, "fw_bgr_to_lab_u8", frames[0].reshape(-1, 3)))
    np.testing.assert_array_equal(got[0].reshape(-1, 3), via)


def test_a_different_lut_per_frame_and_in_place(hip_lib):
    rng = np.random.default_rng(77)
    frames = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8) if k % 2 else f for k, f in enumerate(synthetic_frames(7, 37, 53, seed=9))]
    luts = rng.integers(0, 256, (7, 256), dtype=np.uint8)
    want = _deflicker_ref(frames, luts)
    assert len({want[k].tobytes() for k in range(7)}) == 7
    # a frame-index mistake must show: frame k under the LUT of another frame is another image
    assert all((_deflicker_ref([frames[k]], [luts[(k + 1) % 7]])[0] != want[k]).any() for k in range(7))
    np.testing.assert_array_equal(_deflicker(hip_lib, frames, luts), want)
    np.testing.assert_array_equal(_deflicker(hip_lib, frames, luts, in_place=True), want)


# ------------------------------------------------------------------------------------------------------------- DeviceFlickerReducer
@pytest.fixture(scope="module")
def clip_and_ref():
    clip = fr.flicker_clip()
    return clip, fr.python_deflicker(clip)


def test_reduce_flicker_equals_the_restatement(hip_lib, clip_and_ref):
    torch, dev = _torch()
    clip, want = clip_and_ref
    assert len(clip) == 23 and clip[0].shape == (40, 56, 3)
    # liveliness, which the restatement alone satisfies (tests/test_flicker_ref_host.py establishes the same on the CPU)
    target = fr.target_brightness(clip)
    adj = [target - fr.bgr_to_lab_gamma(f)[..., 0].astype(np.int64).sum() / (40 * 56) for f in clip]
    assert any(abs(a) > 20 for a in adj) and any(abs(a) < 20 for a in adj)
    assert sum((o != f).any(axis=2).mean() > 0.5 for o, f in zip(want, clip)) > len(clip) / 2
    std = lambda fs: float(np.std([fr.gray(f).mean() for f in fs]))
    assert std(want) < std(clip)

    reducer = TD.DeviceFlickerReducer(chunk_size=10)                  # three batches: 10, 10, 3
    got, res = reducer.reduce_flicker(clip)
    assert res == fr.reduce_flicker(clip)[1]
    assert len(got) == 23
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert reducer.target_brightness(clip) == target
    # the resident forms: a list of frames and a stack, whole-clip batches
    reducer = TD.DeviceFlickerReducer()
    devs = [torch.from_numpy(f).to(dev) for f in clip]
    out_list = reducer.reduce_flicker_device(devs)
    out_stack = reducer.reduce_flicker_device(torch.stack(devs))
    torch.cuda.synchronize(dev)
    assert isinstance(out_list, list) and len(out_list) == 23 and tuple(out_stack.shape) == (23, 40, 56, 3)
    np.testing.assert_array_equal(torch.stack(out_list).cpu().numpy(), np.stack(want))
    np.testing.assert_array_equal(out_stack.cpu().numpy(), np.stack(want))
    np.testing.assert_array_equal(torch.stack(devs).cpu().numpy(), np.stack(clip))      # the inputs are left untouched


def test_analyze_flicker_and_the_adaptive_mode(hip_lib, clip_and_ref):
    clip, _ = clip_and_ref
    reducer = TD.DeviceFlickerReducer()
    assert reducer.reduce_flicker(clip[:3])[1]["mode_used"] == "adaptive"          # no analysis yet: the mode stays as it was given
    metrics = reducer.analyze_flicker(clip, sample_rate=2, max_samples=8)
    want = TD.flicker_metrics_from_brightness([fr.gray(f).astype(np.int64).sum() / (40 * 56) for f in clip], 2, 8)
    assert metrics == want and metrics["severity"] >= 0.3
    assert reducer.reduce_flicker(clip[:3])[1]["mode_used"] == "aggressive"
    assert TD.DeviceFlickerReducer(mode=TD.FlickerMode.LIGHT).reduce_flicker(clip[:3])[1]["mode_used"] == "light"
    assert reducer.analyze_flicker(clip[:2])["severity"] == 0.0                    # fewer than three frames
    assert reducer.reduce_flicker([]) == ([], {"frames_processed": 0, "mode_used": None})


# ------------------------------------------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def driver_runs():
    """25 noisy frames of a flickering scene through `denoise_clip`, shared by the driver tests."""
    rng = np.random.default_rng(3)
    frames = [np.clip(f.astype(np.int16) + rng.integers(-6, 7, f.shape), 0, 255).astype(np.uint8) for f in fr.flicker_clip(25)]
    cfg = lambda chunk: TD.TemporalDenoiseConfig(temporal_radius=1, chunk_size=chunk)
    runs = {"frames": frames}
    runs["device50"] = TD.DeviceTemporalDenoiser(cfg(50), device_flicker=True).denoise_clip(frames)
    runs["device10"] = TD.DeviceTemporalDenoiser(cfg(10), device_flicker=True).denoise_clip(frames)
    reducer = TD.DeviceFlickerReducer()
    runs["hook"] = TD.DeviceTemporalDenoiser(cfg(50)).denoise_clip(frames, deflicker_fn=lambda fs: reducer.reduce_flicker(fs)[0])
    runs["plain"] = TD.DeviceTemporalDenoiser(cfg(50)).denoise_clip(frames)
    return runs


def test_denoise_clip_with_device_flicker_equals_the_host_hook(hip_lib, driver_runs):
    out, res = driver_runs["device50"]
    hook_out, hook_res = driver_runs["hook"]
    assert len(out) == 25 and res.flicker_reduction_applied is True and hook_res.flicker_reduction_applied is True
    np.testing.assert_array_equal(np.stack(out), np.stack(hook_out))
    assert res.scene_changes_detected == hook_res.scene_changes_detected and res.avg_noise_reduction == hook_res.avg_noise_reduction
    assert res.frames_processed == 25 and res.frames_failed == 0


def test_denoise_clip_with_device_flicker_differs_from_the_run_without(hip_lib, driver_runs):
    out, _ = driver_runs["device50"]
    plain_out, plain_res = driver_runs["plain"]
    assert plain_res.flicker_reduction_applied is False
    assert (np.stack(out) != np.stack(plain_out)).mean() > 0.25


def test_denoise_clip_with_device_flicker_does_not_depend_on_chunk_size(hip_lib, driver_runs):
    np.testing.assert_array_equal(np.stack(driver_runs["device10"][0]), np.stack(driver_runs["device50"][0]))
    assert driver_runs["device10"][1].flicker_reduction_applied is True


def test_device_flicker_and_the_hook_exclude_each_other(hip_lib, driver_runs):
    frames = driver_runs["frames"][:3]
    with pytest.raises(ValueError, match="not both"):
        TD.DeviceTemporalDenoiser(device_flicker=True).denoise_clip(frames, deflicker_fn=lambda fs: fs)
    # the flag alone does nothing where the config switches flicker reduction off
    off = TD.DeviceTemporalDenoiser(TD.TemporalDenoiseConfig(temporal_radius=1, enable_flicker_reduction=False), device_flicker=True)
    out, res = off.denoise_clip(frames)
    ref_out, _ = TD.DeviceTemporalDenoiser(TD.TemporalDenoiseConfig(temporal_radius=1, enable_flicker_reduction=False)).denoise_clip(frames)
    assert res.flicker_reduction_applied is False
    np.testing.assert_array_equal(np.stack(out), np.stack(ref_out))
    assert TD.create_temporal_denoiser(device_flicker=True).device_flicker is True and TD.create_temporal_denoiser().device_flicker is False


def test_denoise_frames_directory_form_follows_the_flag(hip_lib, driver_runs, tmp_path):
    from PIL import Image
    frames = driver_runs["frames"][:4]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for k, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(src / f"frame_{k:04d}.png"))
    den = TD.DeviceTemporalDenoiser(TD.TemporalDenoiseConfig(temporal_radius=1), device_flicker=True)
    res = den.denoise_frames(src, dst)
    want, _ = den.denoise_clip(frames)
    assert res.flicker_reduction_applied is True and res.frames_processed == 4
    for k, w in enumerate(want):
        got = np.asarray(Image.open(str(dst / f"frame_{k:04d}.png")).convert("RGB"))[:, :, ::-1]
        np.testing.assert_array_equal(got, w)


# ------------------------------------------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments_are_reported_and_nothing_is_launched(hip_lib):
    torch, dev = _torch()
    buf = torch.full((4 * 6 * 3 * 2,), 0xAB, dtype=torch.uint8, device=dev)
    src = torch.zeros_like(buf)
    sums = torch.full((2,), -5, dtype=torch.int64, device=dev)
    luts = torch.zeros(512, dtype=torch.uint8, device=dev)
    st = _stream(torch, dev)
    INV = _lib.FW_ERR_INVALID
    bad = []
    bad.append(hip_lib.fw_bgr_to_lab_u8(None, 8, _p(buf), st))
    bad.append(hip_lib.fw_bgr_to_lab_u8(_p(src), 8, None, st))
    bad.append(hip_lib.fw_bgr_to_lab_u8(_p(src), 0, _p(buf), st))
    bad.append(hip_lib.fw_bgr_to_lab_u8(_p(src), -3, _p(buf), st))
    bad.append(hip_lib.fw_lab_to_bgr_u8(None, 8, _p(buf), st))
    bad.append(hip_lib.fw_lab_to_bgr_u8(_p(src), 8, None, st))
    bad.append(hip_lib.fw_lab_to_bgr_u8(_p(src), 0, _p(buf), st))
    bad.append(hip_lib.fw_lab_l_sums_u8(None, 2, 4, 6, _p(sums), st))
    bad.append(hip_lib.fw_lab_l_sums_u8(_p(src), 2, 4, 6, None, st))
    for count, h, w in [(0, 4, 6), (-1, 4, 6), (65536, 4, 6), (2, 0, 6), (2, 4, 0), (2, -4, 6), (1, 65536, 65536)]:
        bad.append(hip_lib.fw_lab_l_sums_u8(_p(src), count, h, w, _p(sums), st))
        assert hip_lib.fw_last_error().startswith(b"fw_lab_l_sums_u8: ")
        bad.append(hip_lib.fw_deflicker_lab_u8(_p(src), count, h, w, _p(luts), _p(buf), st))
        assert hip_lib.fw_last_error().startswith(b"fw_deflicker_lab_u8: ")
    bad.append(hip_lib.fw_deflicker_lab_u8(None, 2, 4, 6, _p(luts), _p(buf), st))
    bad.append(hip_lib.fw_deflicker_lab_u8(_p(src), 2, 4, 6, None, _p(buf), st))
    bad.append(hip_lib.fw_deflicker_lab_u8(_p(src), 2, 4, 6, _p(luts), None, st))
    assert b"null pointer" in hip_lib.fw_last_error()
    assert bad == [INV] * len(bad)
    torch.cuda.synchronize(dev)
    assert (buf.cpu().numpy() == 0xAB).all() and sums.cpu().numpy().tolist() == [-5, -5]      # nothing ran
    with pytest.raises(ValueError):
        TD.DeviceFlickerReducer().deflicker_batch_device(torch.zeros((2, 4, 6), dtype=torch.uint8, device=dev), 100.0)
    with pytest.raises(ValueError):
        TD.DeviceFlickerReducer(chunk_size=0)
