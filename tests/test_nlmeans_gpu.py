"""Non-local-means spatial denoise on the device (csrc/nlmeans.hip, framewright_amd.temporal_denoise.DeviceSpatialDenoiser) against
the integer restatement in tests/nlmeans_ref.py: BIT-EXACT, every pixel - every step behind the construction of the tables is
integer arithmetic, so no tolerance is needed and none is allowed.  cv2 is not installed here: parity with cv2 itself is unpinned.
tests/test_nlmeans_ref_host.py holds the cases to a liveliness condition (a case whose only non-zero weight is the centre would
pass with a broken kernel)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nlmeans_ref as nr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402
from framewright_amd.synth import synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 4096     # guard bytes in front of and behind every output and the scratch


def _guarded(n, fill, dev):
    import torch
    t = torch.full((n + 2 * SENTINEL,), fill, dtype=torch.uint8, device=dev)
    return t, t[SENTINEL:SENTINEL + n]


def _guards_intact(t, fill, n):
    return bool((t[:SENTINEL] == fill).all()) and bool((t[SENTINEL + n:] == fill).all())


def _core_guarded(lib, plane, h, template=7, search=21, expect=_lib.FW_OK):
    """fw_nlmeans_u8 through the raw C-ABI with sentinel margins around the output and the scratch."""
    import torch
    dev = torch.device("cuda", 0)
    hh, ww, c = plane.shape
    src = torch.from_numpy(np.ascontiguousarray(plane)).to(dev)
    nb = max(int(lib.fw_nlmeans_scratch_bytes(hh, ww, search)), 256)
    gs, scratch = _guarded(nb, 0xA5, dev)
    gd, dst = _guarded(plane.size, 0x5A, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    status = lib.fw_nlmeans_u8(C.c_void_p(src.data_ptr()), c, hh, ww, float(h), template, search, C.c_void_p(scratch.data_ptr()),
                               C.c_void_p(dst.data_ptr()), st)
    torch.cuda.synchronize(dev)
    assert status == expect, lib.fw_last_error()
    assert _guards_intact(gs, 0xA5, nb) and _guards_intact(gd, 0x5A, plane.size), "a kernel wrote outside its buffers"
    if expect != _lib.FW_OK:
        assert bool((dst == 0x5A).all()) and bool((scratch == 0xA5).all()), "a refused call wrote something"
        return None
    np.testing.assert_array_equal(src.cpu().numpy(), plane)
    return dst.reshape(hh, ww, c).cpu().numpy()


def _colored_guarded(lib, bgr, h, h_color, template=7, search=21, expect=_lib.FW_OK):
    import torch
    dev = torch.device("cuda", 0)
    hh, ww = bgr.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(bgr)).to(dev)
    nb = max(int(lib.fw_nlmeans_scratch_bytes(hh, ww, search)), 256)
    gs, scratch = _guarded(nb, 0xA5, dev)
    gd, dst = _guarded(bgr.size, 0x5A, dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    status = lib.fw_nlmeans_colored_u8(C.c_void_p(src.data_ptr()), hh, ww, float(h), float(h_color), template, search,
                                       C.c_void_p(scratch.data_ptr()), C.c_void_p(dst.data_ptr()), st)
    torch.cuda.synchronize(dev)
    assert status == expect, lib.fw_last_error()
    assert _guards_intact(gs, 0xA5, nb) and _guards_intact(gd, 0x5A, bgr.size), "a kernel wrote outside its buffers"
    if expect != _lib.FW_OK:
        assert bool((dst == 0x5A).all()) and bool((scratch == 0xA5).all()), "a refused call wrote something"
        return None
    return dst.reshape(hh, ww, 3).cpu().numpy()


@pytest.mark.parametrize("case", nr.core_cases(), ids=lambda c: c[0])
def test_core_bit_exact(hip_lib, case):
    name, plane, h, template, search, _ = case
    want = nr.nlmeans(plane, h, template, search)
    got = _core_guarded(hip_lib, plane, h, template, search)
    differ = int((got != want).any(axis=2).sum())
    print(f"{name}: {differ} of {want.shape[0] * want.shape[1]} pixels differ from the restatement; "
          f"{int((want != plane).any(axis=2).sum())} differ from the input")
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("case", nr.colored_cases(), ids=lambda c: c[0])
def test_coloured_bit_exact(hip_lib, case):
    name, bgr, h, h_color = case
    want = nr.nlmeans_colored(bgr, h, h_color)
    got = _colored_guarded(hip_lib, bgr, h, h_color)
    print(f"{name}: {int((got != want).any(axis=2).sum())} of {bgr.shape[0] * bgr.shape[1]} pixels differ from the restatement")
    np.testing.assert_array_equal(got, want)
    assert (got != bgr).any()


def test_spatial_denoiser_surface(hip_lib):
    import torch
    frame = np.ascontiguousarray(synthetic_frames(1, 54, 70, seed=21)[0])
    sd = TD.DeviceSpatialDenoiser()
    np.testing.assert_array_equal(sd.denoise(frame, 0.5), nr.nlmeans_colored(frame, 6, 6))
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(frame).to(dev)
    out = sd.denoise_device(t, 10, 6)
    assert out.data_ptr() != t.data_ptr() and out.dtype == torch.uint8 and tuple(out.shape) == frame.shape
    np.testing.assert_array_equal(t.cpu().numpy(), frame)                      # the input is left untouched
    np.testing.assert_array_equal(out.cpu().numpy(), nr.nlmeans_colored(frame, 10, 6))
    plane = nr.noisy_pattern(37, 53, 1, 4.0, 101)
    got = sd.nlmeans_device(torch.from_numpy(plane[:, :, 0].copy()).to(dev), 6)
    np.testing.assert_array_equal(got.cpu().numpy(), nr.nlmeans(plane, 6)[:, :, 0])
    small = TD.DeviceSpatialDenoiser(template_window=3, search_window=7)
    np.testing.assert_array_equal(small.denoise(frame, 0.5), nr.nlmeans_colored(frame, 6, 6, 3, 7))
    with pytest.raises(_lib.FramewrightHipError, match="even sizes are rejected"):
        TD.DeviceSpatialDenoiser(template_window=6).denoise(frame, 0.5)


def test_denoise_sequence_with_the_spatial_step(hip_lib):
    """Device-resident chain == the same steps composed by hand from separately tested calls; None and 0.3 reproduce the output
    without the spatial step; a scene-cut frame equals the single-frame chain; host-fed path == device-resident path."""
    import torch
    frames = [np.ascontiguousarray(f) for f in synthetic_frames(4, 54, 70, seed=31)]
    est = TD.DeviceFlowEstimator()
    acc = TD.DeviceTemporalAccumulator(flow_estimator=est)
    dev = torch.device("cuda", 0)
    devs = [torch.from_numpy(f).to(dev) for f in frames]
    got = list(acc.denoise_sequence(frames, temporal_radius=1, noise_strength=0.5, preserve_edges=True))
    assert len(got) == 4
    for i, out in enumerate(got):
        lo, hi = max(0, i - 1), min(4, i + 2)
        window = acc._window_device(i - lo, devs[lo:hi]).cpu().numpy()
        nlm = nr.nlmeans_colored(window, 6, 6)
        assert (nlm != window).any()
        np.testing.assert_array_equal(out, acc.preserve_edges(frames[i], nlm, 30))
    plain = list(acc.denoise_sequence(frames, temporal_radius=1, preserve_edges=True))
    for strength in (None, 0.3):
        for a, b in zip(plain, acc.denoise_sequence(frames, temporal_radius=1, preserve_edges=True, noise_strength=strength)):
            np.testing.assert_array_equal(a, b)
    assert any((a != b).any() for a, b in zip(plain, got))
    # a scene cut: frame 2 from a window of itself alone
    cut = list(acc.denoise_sequence(frames, temporal_radius=1, noise_strength=0.5, preserve_edges=True, scene_changes=[2]))
    alone = list(acc.denoise_sequence(frames[2:3], temporal_radius=1, noise_strength=0.5, preserve_edges=True))[0]
    np.testing.assert_array_equal(cut[2], alone)
    np.testing.assert_array_equal(alone, acc.preserve_edges(frames[2], nr.nlmeans_colored(frames[2], 6, 6), 30))
    for i in (0, 1, 3):
        np.testing.assert_array_equal(cut[i], got[i])
    # the host-fed path, given the same flows
    host = TD.DeviceTemporalAccumulator(flow_fn=est.estimate)
    for a, b in zip(cut, host.denoise_sequence(frames, temporal_radius=1, noise_strength=0.5, preserve_edges=True, scene_changes=[2])):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="scene_changes"):
        next(acc.denoise_sequence(frames, scene_changes=[4]))


def test_invalid_arguments_are_refused_and_nothing_is_written(hip_lib):
    plane = nr.noisy_pattern(20, 24, 1, 4.0, 7)
    bgr = np.ascontiguousarray(synthetic_frames(1, 20, 24, seed=5)[0])
    for kw in [dict(h=0), dict(h=-2), dict(template=6), dict(template=9), dict(template=0), dict(search=20), dict(search=43),
               dict(search=-1), dict(h=200)]:
        args = dict(h=6, template=7, search=21)
        args.update(kw)
        _core_guarded(hip_lib, plane, expect=_lib.FW_ERR_INVALID, **args)
        assert len(hip_lib.fw_last_error()) > 0
        _colored_guarded(hip_lib, bgr, args["h"], 6, args["template"], args["search"], expect=_lib.FW_ERR_INVALID)
    _colored_guarded(hip_lib, bgr, 6, 0, expect=_lib.FW_ERR_INVALID)
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 2048)
    assert hip_lib.fw_nlmeans_u8(p, 4, 20, 24, 6.0, 7, 21, None, q, None) == _lib.FW_ERR_INVALID          # channels
    assert b"channels" in hip_lib.fw_last_error()
    assert hip_lib.fw_nlmeans_u8(p, 0, 20, 24, 6.0, 7, 21, None, q, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_nlmeans_u8(p, 1, 20, 24, 6.0, 7, 21, None, p, None) == _lib.FW_ERR_INVALID          # in place
    assert hip_lib.fw_nlmeans_u8(None, 1, 20, 24, 6.0, 7, 21, None, p, None) == _lib.FW_ERR_INVALID       # NULL pointers
    assert hip_lib.fw_nlmeans_u8(p, 1, 20, 24, 6.0, 7, 21, None, None, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_nlmeans_u8(p, 1, 1, 24, 6.0, 7, 21, None, q, None) == _lib.FW_ERR_INVALID   # a 1-px side
    assert b"1 px" in hip_lib.fw_last_error()
    assert hip_lib.fw_nlmeans_colored_u8(p, 20, 1, 6.0, 6.0, 7, 21, p, q, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_nlmeans_colored_u8(p, 20, 24, 6.0, 6.0, 7, 21, None, p, None) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize(dev)
    assert not bool(buf.any())


def test_1080p_coloured_call(hip_lib):
    """The whole frame runs; a 64 x 64 region is held bit-exact: the restatement's Lab planes of the frame (elementwise, fast), the
    core on the region cut out with its 13-px context, the inverse transform - and the device's output there."""
    frame = np.ascontiguousarray(synthetic_frames(1, 1080, 1920, seed=9)[0])
    got = _colored_guarded(hip_lib, frame, 6, 6)
    assert got.shape == frame.shape and got.dtype == np.uint8
    assert float((got != frame).any(axis=2).mean()) > 0.5
    lab = nr.bgr_to_lab(frame)
    for y0, x0 in ((500, 900), (1080 - 64, 1920 - 64), (0, 0)):
        ys, xs = np.arange(y0 - 13, y0 + 64 + 13), np.arange(x0 - 13, x0 + 64 + 13)
        refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
        ctx = lab[refl(ys, 1080)][:, refl(xs, 1920)]                      # the region with its context, the frame's own border rule
        L = nr.nlmeans(np.ascontiguousarray(ctx[:, :, :1]), 6)[13:-13, 13:-13]
        ab = nr.nlmeans(np.ascontiguousarray(ctx[:, :, 1:]), 6)[13:-13, 13:-13]
        want = nr.lab_to_bgr(np.concatenate([L, ab], axis=2))
        np.testing.assert_array_equal(got[y0:y0 + 64, x0:x0 + 64], want)
