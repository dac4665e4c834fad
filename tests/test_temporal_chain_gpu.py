"""csrc/temporal_chain.hip and the classes built on it (DeviceClipAnalyzer, DeviceTemporalConsistencyFilter, DeviceTemporalDenoiser)
against tests/temporal_chain_ref.py.  Everything here is exact: integer statistics, float64 accumulation in the restatement's order,
float32 blends with the restatement's roundings.  The flow maps the consistency filter consumes are downloaded from the device and
fed to the restatement, so these tests compare this file's subject and not Farneback's flow (tests/test_flow_gpu.py does that)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import temporal_chain_ref as tr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402
from framewright_amd.synth import synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------- fw_frame_stats_u8
SIZES = [(1, 9), (5, 3), (37, 53), (270, 480), (1080, 1920)]


def _stats_frames(kind, count, h, w):
    rng = np.random.default_rng(h * 7919 + w * 31 + count)
    noise = lambda: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":
        return [np.full((h, w, 3), (90, 140, 200), np.uint8)] * count
    if kind == "noise":
        return [noise() for _ in range(count)]
    if kind == "synthetic":
        return list(synthetic_frames(count, max(h, 8), max(w, 8), seed=h + w)[:, :h, :w])
    return [np.full((h, w, 3), 17, np.uint8), noise()] + list(synthetic_frames(count - 2, max(h, 8), max(w, 8), seed=3)[:, :h, :w])  # mixed


def _assert_live(frames):
    """A kernel that writes zeros must not pass: over the frames of a non-constant case the restatement's histograms occupy at
    least 64 bins - or, where the case holds fewer than 128 pixels, at least half as many bins as it has pixels - and the summed
    squared Laplacian is positive."""
    hist = sum(tr.frame_stats(f)[0] for f in frames)
    s2 = sum(tr.frame_stats(f)[2] for f in frames)
    n_px = sum(f.shape[0] * f.shape[1] for f in frames)
    occupied = int((hist > 0).sum())
    print(f"liveliness: {occupied} occupied bins over {n_px} pixels, sum lap^2 = {s2}")
    assert occupied >= min(64, n_px // 2) and s2 > 0


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind,count", [("constant", 1), ("noise", 1), ("synthetic", 1), ("mixed", 7)])
def test_frame_stats_equal_the_restatement(hip_lib, kind, count, h, w):
    torch, dev = _torch()
    frames = _stats_frames(kind, count, h, w)
    if kind != "constant":
        _assert_live(frames)
    analyzer = TD.DeviceClipAnalyzer()
    hist, sums = analyzer.stats_device(torch.from_numpy(np.stack(frames)).to(dev))
    assert hist.shape == (count, 256) and sums.shape == (count, 2)
    for k, f in enumerate(frames):
        want_hist, s1, s2 = tr.frame_stats(f)
        np.testing.assert_array_equal(hist[k].astype(np.int64), want_hist)
        assert (int(sums[k, 0]), int(sums[k, 1])) == (s1, s2)
    if kind == "constant":
        assert sums.tolist() == [[0, 0]] * count and int(hist.max()) == h * w
    # the outputs are zeroed by the call itself: a second call into a dirty buffer gives the same numbers
    hist2, sums2 = analyzer.stats_device(torch.from_numpy(np.stack(frames)).to(dev))
    np.testing.assert_array_equal(hist2, hist)
    np.testing.assert_array_equal(sums2, sums)


def test_frame_stats_host_batches_equal_one_batch(hip_lib):
    frames = list(synthetic_frames(23, 40, 56, seed=4))
    analyzer = TD.DeviceClipAnalyzer(TD.TemporalDenoiseConfig(chunk_size=10))
    hist, sums = analyzer.frame_stats(frames)
    for k, f in enumerate(frames):
        want_hist, s1, s2 = tr.frame_stats(f)
        np.testing.assert_array_equal(hist[k].astype(np.int64), want_hist)
        assert (int(sums[k, 0]), int(sums[k, 1])) == (s1, s2)
    assert analyzer.laplacian_variances(frames) == [tr.laplacian_variance(f) for f in frames]


# ------------------------------------------------------------------------------------------------------------ fw_add_weighted_u8
def _add_weighted(hip_lib, a, alpha, b, beta, offset=0):
    torch, dev = _torch()
    n = a.size
    ta, tb = (torch.zeros(n + 8, dtype=torch.uint8, device=dev) for _ in range(2))
    ta[offset:offset + n] = torch.from_numpy(a.reshape(-1)).to(dev)
    tb[offset:offset + n] = torch.from_numpy(b.reshape(-1)).to(dev)
    out = torch.full((n + 8,), 77, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(hip_lib.fw_add_weighted_u8(C.c_void_p(ta.data_ptr() + offset), alpha, C.c_void_p(tb.data_ptr() + offset), beta, n,
                                          C.c_void_p(out.data_ptr() + offset), st))
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert (got[:offset] == 77).all() and (got[offset + n:] == 77).all()          # nothing outside the n bytes is written
    return got[offset:offset + n].reshape(a.shape)


@pytest.mark.parametrize("alpha,beta", [(0.5, 0.5), (0.7, 0.3), (0.75, 0.25), (1.0, 0.0), (0.0, 1.0)])
def test_add_weighted_full_grid(hip_lib, alpha, beta):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    want = tr.add_weighted(a, alpha, b, beta)
    if (alpha, beta) == (0.5, 0.5):
        ties = ((a.astype(int) + b.astype(int)) % 2 == 1).mean()
        assert ties == 0.5                                   # half of the grid sits on an exact .5 tie, a quarter of it rounds down
        assert ((want.astype(int) * 2 < a.astype(int) + b) & (want % 2 == 0)).mean() == 0.25
    np.testing.assert_array_equal(_add_weighted(hip_lib, a, alpha, b, beta), want)
    np.testing.assert_array_equal(_add_weighted(hip_lib, a[:, :251], alpha, b[:, :251], beta, offset=1),
                                  want[:, :251])             # unaligned pointers and a ragged length: the bytewise path


def test_add_weighted_saturates(hip_lib):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for alpha, beta in [(1.5, 1.0), (-1.0, 2.0), (2.0, -1.0)]:
        want = tr.add_weighted(a, alpha, b, beta)
        assert want.min() == 0 and want.max() == 255
        np.testing.assert_array_equal(_add_weighted(hip_lib, a, alpha, b, beta), want)


# ------------------------------------------------------------------------------------------------- the temporal-consistency filter
def _noisy_clip(n, h, w, seed, sigma=12.0):
    rng = np.random.default_rng(seed)
    return [np.clip(f.astype(np.float64) + rng.normal(0, sigma, f.shape), 0, 255).astype(np.uint8) for f in synthetic_frames(n, h, w, seed)]


def _device_maps(est, frames, center, radius):
    """maps[j] = (flow_x, flow_y, confidence) of neighbour j onto the centre frame, as `maps_device` leaves them on the device."""
    torch, dev = _torch()
    devs = [torch.from_numpy(f).to(dev) for f in frames]
    maps = [None] * len(frames)
    for j in range(max(0, center - radius), min(len(frames), center + radius + 1)):
        if j != center:
            fx, fy, _, conf = est.maps_device(devs[j], devs[center])
            torch.cuda.synchronize(dev)
            maps[j] = (fx.cpu().numpy(), fy.cpu().numpy(), conf.cpu().numpy())
    return maps


@pytest.mark.parametrize("center", [0, 3, 6])
@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("strength", [0.0, 0.3, 0.5, 1.0])
def test_consistency_flow_guided_bit_exact(hip_lib, strength, radius, center):
    torch, dev = _torch()
    frames = _noisy_clip(7, 72, 96, seed=11)
    est = TD.DeviceFlowEstimator()
    filt = TD.DeviceTemporalConsistencyFilter(strength=strength, temporal_radius=radius, flow_estimator=est)
    maps = _device_maps(est, frames, center, radius)
    want = tr.consistency_flow_guided(frames, center, radius, strength, maps)
    changed = (want != frames[center]).mean()
    print(f"strength {strength} radius {radius} frame {center}: {changed:.3f} of the bytes differ from the centre frame")
    if strength >= 0.3:
        assert changed > 0.5
    else:
        np.testing.assert_array_equal(want, frames[center])
    got = filt.apply_device([torch.from_numpy(f).to(dev) for f in frames], center)
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_consistency_sequence_simple_form_and_single_frame(hip_lib):
    frames = _noisy_clip(6, 40, 56, seed=5)
    for strength, radius in [(0.5, 2), (1.0, 1), (0.3, 3)]:
        filt = TD.DeviceTemporalConsistencyFilter(strength=strength, temporal_radius=radius, use_optical_flow=False)
        assert filt.flow_estimator is None
        got = list(filt.apply_sequence(frames))
        assert len(got) == len(frames)
        for i, g in enumerate(got):
            np.testing.assert_array_equal(g, tr.consistency_simple(frames, i, radius, strength))
        assert (got[2] != frames[2]).mean() > 0.25
    # a window of one frame takes the simple form also when optical flow is asked for (:932): the blend leaves the frame as it is
    filt = TD.DeviceTemporalConsistencyFilter(strength=0.8, temporal_radius=2)
    got = list(filt.apply_sequence(frames[:1]))
    np.testing.assert_array_equal(got[0], tr.consistency_simple(frames[:1], 0, 2, 0.8))
    np.testing.assert_array_equal(got[0], frames[0])
    # the whole sequence, flow-guided, against the restatement frame by frame
    est = TD.DeviceFlowEstimator()
    filt = TD.DeviceTemporalConsistencyFilter(strength=0.5, temporal_radius=2, flow_estimator=est)
    for i, g in enumerate(filt.apply_sequence(frames)):
        np.testing.assert_array_equal(g, tr.consistency_flow_guided(frames, i, 2, 0.5, _device_maps(est, frames, i, 2)))


class _FailingEstimator:
    """A flow estimator that raises for one neighbour frame (by its device address) and defers to a real one otherwise."""

    def __init__(self, real):
        self.real, self.bad_ptr = real, None

    def maps_device(self, t1, t2, weight_map=False):
        if t1.data_ptr() == self.bad_ptr:
            raise RuntimeError("flow failed")
        return self.real.maps_device(t1, t2, weight_map=weight_map)


def test_consistency_failing_flow_takes_the_scalar_weight(hip_lib):
    torch, dev = _torch()
    frames = _noisy_clip(5, 40, 56, seed=8)
    real = TD.DeviceFlowEstimator()
    est = _FailingEstimator(real)
    filt = TD.DeviceTemporalConsistencyFilter(strength=0.6, temporal_radius=2, flow_estimator=est)
    devs = [torch.from_numpy(f).to(dev) for f in frames]
    est.bad_ptr = devs[1].data_ptr()
    maps = _device_maps(real, frames, 2, 2)
    whole = tr.consistency_flow_guided(frames, 2, 2, 0.6, maps)
    maps[1] = None
    want = tr.consistency_flow_guided(frames, 2, 2, 0.6, maps)
    assert (want != whole).any()
    got = filt.apply_device(devs, 2)
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- the analysis
def _darkened_clip(n, cut, h=72, w=96, seed=1):
    return [f if i < cut else f // 3 for i, f in enumerate(synthetic_frames(n, h, w, seed))]


@pytest.mark.parametrize("n,cut,sample_rate,flicker", [(12, 5, 5, True), (12, 7, 5, True), (12, 5, 1, False), (7, 3, 5, True), (2, 1, 5, True)])
def test_analyze_equals_the_restatement(hip_lib, n, cut, sample_rate, flicker):
    frames = _darkened_clip(n, cut)
    cfg = TD.TemporalDenoiseConfig(enable_flicker_reduction=flicker, chunk_size=10)
    got = TD.DeviceClipAnalyzer(cfg).analyze(frames, sample_rate)
    want = tr.analyze(frames, sample_rate, cfg.scene_change_threshold, cfg.temporal_radius, cfg.noise_strength, flicker, cfg.flicker_mode.value)
    assert got == want
    assert list(got) == list(want) and got["scene_changes"] and got["noise_level"] > 0
    if flicker and n >= 12:
        assert got["flicker_metrics"]["severity"] > 0
    if not flicker:
        assert got["flicker_metrics"] == {}


# ------------------------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def clip25():
    rng = np.random.default_rng(25)
    frames = _darkened_clip(25, 5)
    return [np.clip(f.astype(np.float64) + rng.normal(0, 6, f.shape), 0, 255).astype(np.uint8) for f in frames]


@pytest.fixture(scope="module")
def clip25_result(hip_lib, clip25):
    calls = []
    outs, res = TD.DeviceTemporalDenoiser(TD.TemporalDenoiseConfig()).denoise_clip(clip25, progress_callback=calls.append)
    return outs, res, calls


def test_denoise_clip_equals_its_parts(hip_lib, clip25, clip25_result):
    outs, res, calls = clip25_result
    cfg = TD.TemporalDenoiseConfig()
    n = len(clip25)
    analysis = TD.DeviceClipAnalyzer(cfg).analyze(clip25)
    assert analysis["scene_changes"] == [5] == tr.scene_changes(clip25, 5, cfg.scene_change_threshold)
    est = TD.DeviceFlowEstimator()
    acc = TD.DeviceTemporalAccumulator(temporal_weight_decay=cfg.temporal_weight_decay, flow_estimator=est)
    mid = list(acc.denoise_sequence(clip25, cfg.temporal_radius, cfg.preserve_edges, cfg.edge_threshold, cfg.noise_strength,
                                    [c for c in analysis["scene_changes"] if c < n]))
    want = list(TD.DeviceTemporalConsistencyFilter(cfg.noise_strength, cfg.temporal_radius, True, est).apply_sequence(mid))
    assert len(outs) == n
    for i in range(n):
        np.testing.assert_array_equal(outs[i], want[i], err_msg=f"frame {i}")
    assert (np.stack(outs) != np.stack(clip25)).mean() > 0.5
    # the record
    assert res.frames_processed == n and res.frames_failed == 0
    assert res.scene_changes_detected == [5]
    assert res.flicker_reduction_applied is False
    assert 0.0 <= res.avg_noise_reduction <= 1.0
    assert res.avg_noise_reduction == tr.noise_reduction(clip25[:20], want[:20]) and res.avg_noise_reduction > 0
    assert res.processing_time_seconds > 0
    assert calls[:2] == [0.02, 0.05] and calls[-1] == 1.0 and calls == sorted(calls) and 0.25 in calls and 0.85 in calls
    # the frame at the cut is denoised from itself alone: the chain on a one-frame clip gives the same bytes, a full window others
    alone = list(acc.denoise_sequence([clip25[5]], cfg.temporal_radius, cfg.preserve_edges, cfg.edge_threshold, cfg.noise_strength))[0]
    np.testing.assert_array_equal(mid[5], alone)
    windowed = list(acc.denoise_sequence(clip25[2:9], cfg.temporal_radius, cfg.preserve_edges, cfg.edge_threshold, cfg.noise_strength))[3]
    assert (windowed != alone).any()


def test_denoise_clip_does_not_depend_on_chunk_size(hip_lib, clip25, clip25_result):
    outs, res, _ = clip25_result
    small, res_small = TD.DeviceTemporalDenoiser(TD.TemporalDenoiseConfig(chunk_size=10)).denoise_clip(clip25)
    assert len(small) == len(outs)
    for i, (a, b) in enumerate(zip(small, outs)):
        np.testing.assert_array_equal(a, b, err_msg=f"frame {i}")
    assert res_small.avg_noise_reduction == res.avg_noise_reduction and res_small.scene_changes_detected == res.scene_changes_detected


def test_denoise_clip_simple_windows_deflicker_hook_and_dropped_cut(hip_lib):
    # 7 frames with frame 5 alone darkened: the analysis reports [5, 10]; 10 is beyond the clip and is dropped, not an error
    frames = [f // 3 if i == 5 else f for i, f in enumerate(_noisy_clip(7, 40, 56, seed=2, sigma=5.0))]
    cfg = TD.TemporalDenoiseConfig(enable_optical_flow=False, temporal_radius=2, noise_strength=0.4)
    seen = []

    def deflicker(fs):
        seen.append(len(fs))
        return [np.clip(f.astype(int) + 1, 0, 255).astype(np.uint8) for f in fs]

    outs, res = TD.DeviceTemporalDenoiser(cfg).denoise_clip(frames, deflicker_fn=deflicker)
    assert res.scene_changes_detected == [5, 10] and res.flicker_reduction_applied is True and seen == [7]
    shifted = deflicker(frames)
    acc = TD.DeviceTemporalAccumulator(temporal_weight_decay=cfg.temporal_weight_decay)
    spatial = TD.DeviceSpatialDenoiser()
    mid = []
    for i in range(7):
        window = shifted[i:i + 1] if i == 5 else shifted[max(0, i - 2):i + 3]
        d = spatial.denoise(acc.denoise_simple(window), cfg.noise_strength)          # `_denoise_simple`'s centre is the window's middle
        mid.append(acc.preserve_edges(shifted[i], d, cfg.edge_threshold))
    for i, o in enumerate(outs):
        np.testing.assert_array_equal(o, tr.consistency_simple(mid, i, 2, 0.4), err_msg=f"frame {i}")
    # flicker reduction asked for, no hook: not an error, and the metrics are still there
    den = TD.create_temporal_denoiser(strength=0.2, temporal_radius=1, enable_optical_flow=False)
    outs2, res2 = den.denoise_clip(frames)
    assert res2.flicker_reduction_applied is False and len(outs2) == 7
    assert den.analyze(frames, 1)["flicker_metrics"]["severity"] > 0


def test_denoise_frames_directory_form(hip_lib, clip25, clip25_result, tmp_path):
    from PIL import Image
    outs, res, _ = clip25_result
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    names = [f"frame_{i:04d}.png" for i in range(len(clip25))]
    for name, f in zip(names, clip25):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(src / name)
    calls = []
    got = TD.DeviceTemporalDenoiser().denoise_frames(src, dst, progress_callback=calls.append)
    assert sorted(p.name for p in dst.iterdir()) == names
    for name, want in zip(names, outs):
        np.testing.assert_array_equal(np.asarray(Image.open(dst / name).convert("RGB"))[:, :, ::-1], want, err_msg=name)
    assert got.frames_processed == len(clip25) and got.output_dir == dst and got.scene_changes_detected == [5]
    assert got.avg_noise_reduction == res.avg_noise_reduction and calls[0] == 0.02 and calls[-1] == 1.0
    empty = TD.DeviceTemporalDenoiser().denoise_frames(tmp_path / "nothing_here", tmp_path / "out2")
    assert empty.frames_processed == 0 and empty.output_dir is None
