"""Dense Farneback optical flow on the device (csrc/optical_flow.hip, framewright_amd.temporal_denoise.DeviceFlowEstimator) against the
float64 numpy restatement of OpenCV's algorithm in tests/farneback_ref.py, and the flow-compensated temporal denoise that never
leaves the device against the existing host-fed path.  cv2 is not installed here: parity with cv2 itself is unpinned.

The unit of the flow bound is e32, the largest deviation of the float32 restatement from the float64 one on the same input (every
pixel counted): the device must stay within 4 e32 + 1e-4 px of the float64 contract.  Measured device maxima (MI355X) are listed
in DESIGN.md."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import farneback_ref as fr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402
from framewright_amd.synth import synthetic_frames  # noqa: E402
from oracle import temporal_ref as oref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {name: (a, b) for name, a, b in fr.gpu_cases()}
SENTINEL = 4096     # guard elements in front of and behind every output and the scratch


def _guarded(n, dtype, fill, dev):
    import torch
    t = torch.full((n + 2 * SENTINEL,), fill, dtype=dtype, device=dev)
    return t, t[SENTINEL:SENTINEL + n]


def _guards_intact(t, fill):
    return bool((t[:SENTINEL] == fill).all()) and bool((t[-SENTINEL:] == fill).all())


def _device_flow_guarded(lib, a, b, **over):
    """fw_farneback_flow_u8 through the raw C-ABI with sentinel margins around flow_x, flow_y and the scratch."""
    import torch
    dev = torch.device("cuda", 0)
    h, w = a.shape[:2]
    p = {**TD.FARNEBACK_PARAMS, **over}
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    nb = int(lib.fw_farneback_scratch_bytes(h, w, p["levels"]))
    assert nb > 0
    gs, scratch = _guarded(nb, torch.uint8, 0xA5, dev)
    gx, fx = _guarded(h * w, torch.float32, -777.0, dev)
    gy, fy = _guarded(h * w, torch.float32, -777.0, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.fw_farneback_flow_u8(C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), 1 if a.ndim == 2 else 3, h, w, p["pyr_scale"],
                                        p["levels"], p["winsize"], p["iterations"], p["poly_n"], p["poly_sigma"], p["flags"],
                                        C.c_void_p(scratch.data_ptr()), C.c_void_p(fx.data_ptr()), C.c_void_p(fy.data_ptr()), st))
    torch.cuda.synchronize(dev)
    assert _guards_intact(gs, 0xA5) and _guards_intact(gx, -777.0) and _guards_intact(gy, -777.0), "a kernel wrote outside its buffers"
    return fx.reshape(h, w).cpu().numpy(), fy.reshape(h, w).cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_flow_against_float64_contract(hip_lib, name):
    a, b = CASES[name]
    f64 = fr.farneback(a, b, np.float64)
    f32 = fr.farneback(a, b, np.float32)
    e32 = max(float(np.abs(f32[i].astype(np.float64) - f64[i]).max()) for i in range(2))
    got = _device_flow_guarded(hip_lib, a, b)
    assert got[0].dtype == np.float32 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    err = max(float(np.abs(got[i].astype(np.float64) - f64[i]).max()) for i in range(2))
    vs32 = max(float(np.abs(got[i] - f32[i]).max()) for i in range(2))
    print(f"{name}: device max |err| vs float64 {err:.3e} px, e32 {e32:.3e}, bound {4 * e32 + 1e-4:.3e}, device vs float32 restatement {vs32:.3e}")
    assert err <= 4 * e32 + 1e-4, f"{name}: device {err:.3e} px from the float64 contract, e32 {e32:.3e}, bound {4 * e32 + 1e-4:.3e}"


def test_gray_entry_equals_bgr_entry_and_magnitude_is_numpys(hip_lib):
    """The BGR entry converts with cv2's 14-bit weights: the flow of a BGR pair equals, bit for bit, the flow of its gray planes
    (tests/farneback_ref.bgr2gray_u8 = oracle/temporal_ref.bgr2gray_u8).  magnitude = numpy's float32 sqrt(fx**2 + fy**2)."""
    import torch
    a, b = CASES["synthetic_bgr_96x128"]
    np.testing.assert_array_equal(fr.bgr2gray_u8(a), oref.bgr2gray_u8(a))
    est = TD.DeviceFlowEstimator()
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fx3, fy3 = (t.cpu().numpy() for t in est.flow_device(up(a), up(b)))
    fx1, fy1 = (t.cpu().numpy() for t in est.flow_device(up(fr.bgr2gray_u8(a)), up(fr.bgr2gray_u8(b))))
    np.testing.assert_array_equal(fx3, fx1)
    np.testing.assert_array_equal(fy3, fy1)
    # estimate(a, b): the field that warps a onto b = cv2's flow with (b, a) as (prev, next); convention="cv2" is the reference's call
    fx, fy, mag, conf = (t.cpu().numpy() for t in TD.DeviceFlowEstimator(convention="cv2").estimate_device(up(a), up(b)))
    np.testing.assert_array_equal(fx, fx3)
    np.testing.assert_array_equal(mag, np.sqrt(fx ** 2 + fy ** 2))
    fx, fy, mag, conf = (t.cpu().numpy() for t in est.estimate_device(up(b), up(a)))
    np.testing.assert_array_equal(fx, fx3)
    np.testing.assert_array_equal(fy, fy3)
    np.testing.assert_array_equal(mag, np.sqrt(fx ** 2 + fy ** 2))
    assert mag.dtype == np.float32 and conf.dtype == np.float32


@pytest.mark.parametrize("name", ["texture_271x483_affine", "synthetic_bgr_96x128", "texture_45x67_shift"])
def test_variance_confidence_and_percentiles(hip_lib, name):
    """variance / confidence within 4 x the float32-vs-float64 deviation of the restatement on the same (device) flow; the two
    percentiles equal np.percentile of the downloaded maps exactly (numpy >= 2 interpolates a float32 array in float32, and
    temporal_denoise._percentile_sorted repeats those operations)."""
    import torch
    a, b = CASES[name]
    est = TD.DeviceFlowEstimator()
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fx_d, fy_d = est.flow_device(up(b), up(a))               # = the field of estimate(a, b)
    h, w = fx_d.shape
    _, mag_g = _guarded(h * w, torch.float32, -777.0, dev)
    gv, var_d = _guarded(h * w, torch.float32, -777.0, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(hip_lib.fw_flow_stats_f32(C.c_void_p(fx_d.data_ptr()), C.c_void_p(fy_d.data_ptr()), h, w, C.c_void_p(mag_g.data_ptr()),
                                         C.c_void_p(var_d.data_ptr()), st))
    torch.cuda.synchronize(dev)
    assert _guards_intact(gv, -777.0)
    fx, fy = fx_d.cpu().numpy(), fy_d.cpu().numpy()
    var, mag = var_d.reshape(h, w).cpu().numpy(), mag_g.reshape(h, w).cpu().numpy()
    v64, v32 = fr.flow_variance(fx, fy, np.float64), fr.flow_variance(fx, fy, np.float32)
    dev32 = float(np.abs(v32 - v64).max())
    err = float(np.abs(var - v64).max())
    print(f"{name}: variance device err {err:.3e}, float32 restatement {dev32:.3e}")
    assert err <= 4 * dev32 + 1e-12
    # percentiles, taken on the device, against numpy on the downloaded maps
    p95 = TD._percentile_sorted(torch.sort(var_d).values, 95).cpu().numpy()[0]
    p90 = TD._percentile_sorted(torch.sort(mag_g).values, 90).cpu().numpy()[0]
    assert p95 == np.float32(np.percentile(var, 95)) and p90 == np.float32(np.percentile(mag, 90))
    # confidence through the estimator
    _, _, mag2, conf = (t.cpu().numpy() for t in est.estimate_device(up(a), up(b)))
    np.testing.assert_array_equal(mag2, mag)
    c64, c32 = fr.flow_confidence((fx, fy), np.float64), fr.flow_confidence((fx, fy), np.float32)
    cdev = float(np.abs(c32 - c64).max())
    cerr = float(np.abs(conf - c64).max())
    print(f"{name}: confidence device err {cerr:.3e}, float32 restatement {cdev:.3e}")
    assert cerr <= 4 * cdev + 1e-7 and conf.min() >= 0 and conf.max() <= 1
    # the weight map: confidence, halved above the magnitude's 90th percentile
    wm = est.maps_device(up(a), up(b), weight_map=True)[4].cpu().numpy()
    np.testing.assert_array_equal(wm, np.where(mag > np.percentile(mag, 90), conf * np.float32(0.5), conf))


@pytest.mark.parametrize("n,center,decay", [(7, 3, 0.5), (4, 0, 0.2), (3, 2, 1.0)])
def test_device_window_equals_host_fed_path(hip_lib, n, center, decay):
    """flow_estimator= (everything on the device) against the existing path fed with flow_fn = estimator.estimate (the same device
    flows, downloaded and uploaded again): byte for byte, for the window shapes of tests/test_temporal_gpu.py."""
    frames = list(synthetic_frames(n, 41, 59, seed=n))
    est = TD.DeviceFlowEstimator()
    got = TD.DeviceTemporalAccumulator(temporal_weight_decay=decay, flow_estimator=est).denoise_with_flow(center, frames)
    want = TD.DeviceTemporalAccumulator(temporal_weight_decay=decay, flow_fn=est.estimate).denoise_with_flow(center, frames)
    np.testing.assert_array_equal(got, want)
    # and the host-fed path is the oracle's, given those flows
    flows = [None if i == center else est.estimate(f, frames[center]) for i, f in enumerate(frames)]
    oflows = [None if fl is None else dict(flow_x=fl.flow_x, flow_y=fl.flow_y, magnitude=fl.magnitude, confidence=fl.confidence) for fl in flows]
    np.testing.assert_array_equal(got, oref.denoise_with_flow(center, frames, oflows, decay))


def _moving_clip(n, h, w, sigma=10.0, step=2.0, seed=3):
    tex = fr.texture_fn(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng(seed)
    clean = [np.clip(tex(ys + 300.0, xs + 300.0 - step * i), 0, 255) for i in range(n)]
    noisy = [np.clip(np.rint(c + rng.normal(0, sigma, c.shape)), 0, 255).astype(np.uint8) for c in clean]
    return [np.repeat(c[:, :, None], 3, 2) for c in clean], [np.ascontiguousarray(np.repeat(f[:, :, None], 3, 2)) for f in noisy]


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_denoise_sequence_equals_per_frame_calls(hip_lib):
    _, noisy = _moving_clip(7, 120, 160)
    acc = TD.DeviceTemporalAccumulator(flow_estimator=TD.DeviceFlowEstimator())
    seq = list(acc.denoise_sequence(noisy, temporal_radius=3))
    assert len(seq) == 7
    for i, out in enumerate(seq):
        lo, hi = max(0, i - 3), min(7, i + 4)
        np.testing.assert_array_equal(out, acc.denoise_with_flow(i - lo, noisy[lo:hi]))
    # preserve_edges chained on the device = the existing call on the downloaded frames
    pe = list(acc.denoise_sequence(noisy[:3], temporal_radius=1, preserve_edges=True))
    plain = list(acc.denoise_sequence(noisy[:3], temporal_radius=1))
    for o, d, e in zip(noisy[:3], plain, pe):
        np.testing.assert_array_equal(e, acc.preserve_edges(o, d, 30))


def test_flow_compensation_beats_simple_average_on_a_moving_clip(hip_lib):
    """A clean texture translating 2 px per frame plus seeded Gaussian noise (sigma 10): the flow-compensated result is closer to the
    clean centre frame than the plain weighted average and than the noisy frame (orderings, not thresholds).  Measured on an MI355X:
    flow-compensated 35.00 dB, simple average 28.56 dB, noisy frame 28.05 dB.  With the reference's own cv2 call
    (`DeviceFlowEstimator(convention="cv2")`: the flow from the neighbour to the centre, then the neighbour sampled at p + flow) the
    neighbours move AWAY from the centre frame and the result is worse than doing nothing - 23.98 dB; asserted too, so that the
    reason for the default stays visible."""
    clean, noisy = _moving_clip(7, 120, 160)
    acc = TD.DeviceTemporalAccumulator(flow_estimator=TD.DeviceFlowEstimator())
    out = acc.denoise_with_flow(3, noisy)
    inner = (slice(16, -16), slice(16, -16))
    flow_psnr = _psnr(out[inner], clean[3][inner])
    simple_psnr = _psnr(acc.denoise_simple(noisy)[inner], clean[3][inner])
    noisy_psnr = _psnr(noisy[3][inner], clean[3][inner])
    print(f"PSNR vs clean centre: flow-compensated {flow_psnr:.2f} dB, simple average {simple_psnr:.2f} dB, noisy {noisy_psnr:.2f} dB")
    assert flow_psnr > simple_psnr and flow_psnr > noisy_psnr
    ref_call = TD.DeviceTemporalAccumulator(flow_estimator=TD.DeviceFlowEstimator(convention="cv2")).denoise_with_flow(3, noisy)
    ref_psnr = _psnr(ref_call[inner], clean[3][inner])
    print(f"the reference's call order: {ref_psnr:.2f} dB")
    assert ref_psnr < noisy_psnr


def test_1080p_radius3_deterministic_and_one_wait_per_frame(hip_lib, monkeypatch):
    import torch
    frames = [np.ascontiguousarray(f) for f in synthetic_frames(7, 1080, 1920, seed=9)]
    acc = TD.DeviceTemporalAccumulator(flow_estimator=TD.DeviceFlowEstimator())
    first = acc.denoise_with_flow(3, frames)
    calls = {"n": 0}
    dev_sync, stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

    def counted_dev(*a, **k):
        calls["n"] += 1
        return dev_sync(*a, **k)

    def counted_stream(self, *a, **k):
        calls["n"] += 1
        return stream_sync(self, *a, **k)

    monkeypatch.setattr(torch.cuda, "synchronize", counted_dev)
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted_stream)
    second = acc.denoise_with_flow(3, frames)
    monkeypatch.undo()
    assert calls["n"] == 1, f"{calls['n']} host waits for one output frame (six neighbours)"
    np.testing.assert_array_equal(first, second)            # no float atomics anywhere: the same bytes on every run
    assert np.abs(first.astype(int) - frames[3].astype(int)).max() > 0


def test_unchanged_default_and_refusals_on_the_device(hip_lib):
    """Without the new argument the accumulator is today's: no estimator, every neighbour falls back to the unaligned frame."""
    frames = list(synthetic_frames(5, 30, 44, seed=3))
    acc = TD.DeviceTemporalAccumulator(temporal_weight_decay=0.5)
    assert acc.flow_estimator is None
    np.testing.assert_array_equal(acc.denoise_with_flow(2, frames), oref.denoise_with_flow(2, frames, [None] * 5, 0.5))
    with pytest.raises(RuntimeError, match="OpenCV required for optical flow estimation"):
        TD._default_flow_fn(frames[0], frames[1])
    est = TD.DeviceFlowEstimator(poly_n=7)
    with pytest.raises(_lib.FramewrightHipError, match="poly_n"):
        est.estimate(frames[0], frames[1])
    fl = TD.DeviceFlowEstimator(TD.OpticalFlowMethod.RAFT).estimate(frames[0], frames[1])      # falls back to Farneback
    ref = TD.DeviceFlowEstimator().estimate(frames[0], frames[1])
    np.testing.assert_array_equal(fl.flow_x, ref.flow_x)
    assert (fl.frame_idx_from, fl.frame_idx_to) == (0, 1)
    assert all(getattr(fl, k).dtype == np.float32 and getattr(fl, k).shape == (30, 44) for k in ("flow_x", "flow_y", "magnitude", "confidence"))
    warped = TD.DeviceFlowEstimator().warp_frame(frames[0], ref)
    np.testing.assert_array_equal(warped, oref.warp_frame(frames[0], ref.flow_x, ref.flow_y))
