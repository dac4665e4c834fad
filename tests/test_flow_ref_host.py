"""The numpy restatement of Farneback's dense optical flow (tests/farneback_ref.py: the contract of csrc/optical_flow.hip) recovers
known motion, has OpenCV's structure (levels, sizes, sign), and its float32 form is well conditioned on the inputs of the GPU test;
the flow confidence against scipy.ndimage; the public surface and the argument checks that need no GPU."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import farneback_ref as fr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402
from oracle import temporal_ref as oref  # noqa: E402

INTERIOR = 24      # endpoint errors are taken at least this far from the border

# (shape, motion, asserted ceiling on the mean interior endpoint error in px) - the ceilings are 1.5 x the values the float64
# restatement gave when this test was written (inputs are fixed by their seeds; the headroom covers nothing else).  270 x 480 runs
# all four pyramid scales; 96 x 128 stops after two, so the 4.5 and 6 px shifts are restricted to the larger shape.
KNOWN_MOTION = [
    ((270, 480), ("shift", 0.5, -0.25), 0.0281),        # measured 0.01869,
    ((270, 480), ("shift", 2.0, 1.0), 0.00246),        # measured 0.00164,
    ((270, 480), ("shift", -4.5, 3.0), 0.0234),        # measured 0.01557,
    ((270, 480), ("shift", 6.0, 0.5), 0.0238),        # measured 0.01583,
    ((270, 480), ("affine", 0.01, 1.01), 0.0482),        # measured 0.03209,
    ((96, 128), ("shift", 1.5, 1.0), 0.0271),        # measured 0.01800
]


# warping by the flow must bring the second frame onto the first: the interior mean |difference| fell from 8.657 to 0.632 (a factor 13.7)
# when this was written; asserted with the same 1.5 x headroom
SIGN_DROP = 9.1


@pytest.mark.parametrize("shape,motion,ceiling", KNOWN_MOTION)
def test_known_motion_is_recovered(shape, motion, ceiling):
    f1, f2, dx, dy = fr.moving_pair(*shape, motion)
    fx, fy = fr.farneback(f1, f2, np.float64)
    c = (slice(INTERIOR, -INTERIOR), slice(INTERIOR, -INTERIOR))
    epe = float(np.hypot(fx - dx, fy - dy)[c].mean())
    mag = float(np.hypot(dx, dy)[c].mean())
    print(f"{shape} {motion}: mean interior endpoint error {epe:.5f} px, motion {mag:.3f} px")
    assert epe <= ceiling
    if fr.usable_levels(*shape) == 3:
        assert epe < 0.1 * mag                               # the sanity condition, independent of the measured ceiling


def test_zero_flow_sign_and_levels():
    f1, f2, dx, dy = fr.moving_pair(96, 128, ("shift", 1.5, 1.0))
    # Identical frames.  Under the usual description of the algorithm (a sample point outside the second image falls back to the first
    # image's own values) the flow would be exactly 0 in float64.  OpenCV's FarnebackUpdateMatrices does something else there - r2 = r3 =
    # 0: the second image contributes nothing to b - and it treats the last row and column as outside even at zero displacement
    # ((unsigned)x1 < width - 1).  The restatement follows OpenCV, so what is exactly 0 is the right-hand side h everywhere but on that
    # row and column; the box mean and the coarse-to-fine passes spread their contribution (0.082 px at most on this input, measured).
    R = fr.poly_exp(f1.astype(np.float64), np.float64)
    M = fr.update_matrices(R, R, np.zeros(f1.shape), np.zeros(f1.shape), np.float64)
    assert not M[3:, :-1, :-1].any() and M[3:, -1, :].any() and M[3:, :, -1].any()
    zx, zy = fr.farneback(f1, f1, np.float64)
    assert 0 < np.hypot(zx, zy).max() < 0.1
    M[3:, -1, :] = 0
    M[3:, :, -1] = 0
    sx, sy = fr.solve_flow(M, 15, np.float64)
    assert not sx.any() and not sy.any()                     # without that row and column: exactly zero
    # sign: frame2(p) = frame1(p - d), so warping frame2 back by the flow (sampling it at p + flow) lands on frame1
    fx, fy = fr.farneback(f1, f2, np.float64)
    bgr = lambda g: np.repeat(g[:, :, None], 3, 2)
    warped = oref.warp_frame(bgr(f2), fx.astype(np.float32), fy.astype(np.float32))[:, :, 0]
    c = (slice(INTERIOR, -INTERIOR), slice(INTERIOR, -INTERIOR))
    before = np.abs(f2.astype(int) - f1.astype(int))[c].mean()
    after = np.abs(warped.astype(int) - f1.astype(int))[c].mean()
    print(f"interior mean |difference| to frame1: {before:.3f} before, {after:.3f} after warping by the flow")
    assert after * SIGN_DROP <= before
    assert [len(fr.level_plan(h, w)) for h, w in [(45, 67), (96, 128), (270, 480), (1080, 1920)]] == [1, 2, 4, 4]
    # odd sizes: level sizes round half to even (135.5 -> 136, 67.75 -> 68, 241.5 -> 242, 60.375 -> 60)
    assert [(p[4], p[5]) for p in fr.level_plan(271, 483)] == [(34, 60), (68, 121), (136, 242), (271, 483)]
    assert [p[3] for p in fr.level_plan(1080, 1920)] == [19, 9, 3, 3]
    assert fr.cv_round(2.5) == 2 and fr.cv_round(3.5) == 4 and fr.cv_round(17.5) == 18
    fx, fy = fr.farneback(*fr.moving_pair(271, 483, ("shift", 2.0, -1.0))[:2])
    assert fx.shape == (271, 483) and np.isfinite(fx).all() and np.isfinite(fy).all()


def test_single_precision_cost_is_even_over_the_gpu_inputs():
    """e32 = max |float32 restatement - float64 restatement| per input of the GPU test list, every pixel counted: the unit of the device
    bound (4 e32 + 1e-4 px).  The inputs must be textured enough that none is ill conditioned: no e32 above 10 x the list's median.
    Values when this was written are in DESIGN.md."""
    e32 = {}
    for name, a, b in fr.gpu_cases():
        f64, f32 = fr.farneback(a, b, np.float64), fr.farneback(a, b, np.float32)
        assert f32[0].dtype == np.float32 and f64[0].dtype == np.float64
        e32[name] = max(float(np.abs(f32[i].astype(np.float64) - f64[i]).max()) for i in range(2))
        print(f"e32 {name}: {e32[name]:.3e} px")
    med = float(np.median(list(e32.values())))
    assert med > 0
    worst = max(e32, key=e32.get)
    assert e32[worst] <= 10 * med, f"{worst}: e32 {e32[worst]:.3e} against a median of {med:.3e}"


def test_flow_confidence_against_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(5)
    for h, w in [(40, 56), (7, 9), (64, 33)]:
        fx, fy = rng.standard_normal((h, w)).astype(np.float32) * 2, rng.standard_normal((h, w)).astype(np.float32)
        box = lambda a: ndimage.uniform_filter(a.astype(np.float64), 5, mode="mirror")        # mirror = BORDER_REFLECT_101
        var = box((fx - box(fx)) ** 2) + box((fy - box(fy)) ** 2)
        np.testing.assert_allclose(fr.flow_variance(fx, fy, np.float64), var, rtol=1e-6, atol=1e-12)   # the kernel is float32's 1 / 25
        conf = 1.0 - np.clip(var / (np.percentile(var, 95) + 1e-6), 0, 1)
        got = fr.flow_confidence(np.stack([fx, fy], 2), np.float64)
        np.testing.assert_allclose(got, conf, rtol=0, atol=1e-6)
        assert np.abs(fr.flow_confidence((fx, fy), np.float32) - got).max() < 1e-5
        np.testing.assert_array_equal(fr.flow_magnitude_f32(fx, fy), np.sqrt(fx ** 2 + fy ** 2))


def test_public_surface():
    assert {m.name: m.value for m in TD.OpticalFlowMethod} == {"FARNEBACK": "farneback", "LUCAS_KANADE": "lucas_kanade", "DIS": "dis",
                                                               "RAFT": "raft", "RIFE": "rife"}
    assert TD.FARNEBACK_PARAMS == dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.1, flags=0)
    with pytest.raises(NotImplementedError, match="DIS"):
        TD.DeviceFlowEstimator(TD.OpticalFlowMethod.DIS)
    with pytest.raises(NotImplementedError, match="LUCAS_KANADE"):
        TD.DeviceFlowEstimator(TD.OpticalFlowMethod.LUCAS_KANADE)
    with pytest.raises(ValueError, match="convention"):
        TD.DeviceFlowEstimator(convention="backward")
    with pytest.raises(ValueError, match="not both"):
        TD.DeviceTemporalAccumulator(flow_fn=lambda a, b: None, flow_estimator=object())
    z = np.zeros((3, 4), np.float32)
    fl = TD.FlowField(z, z, z, z)
    assert (fl.frame_idx_from, fl.frame_idx_to) == (0, 1) and fl.flow_x.dtype == np.float32
    # np.percentile's index arithmetic for a float32 array, repeated on the host for the device path
    rng = np.random.default_rng(2)
    import torch
    for n in (7, 2419, 129600):
        a = (rng.random(n) ** 2).astype(np.float32)
        for q in (90, 95):
            got = TD._percentile_sorted(torch.sort(torch.from_numpy(a)).values, q).numpy()[0]
            assert got == np.percentile(a, q)


def test_farneback_argument_checks_need_no_gpu(hip_lib):
    """Everything the kernels do not implement is refused with FW_ERR_INVALID and a message before any device call."""
    one = C.c_void_p(256)      # never dereferenced: the checks come first
    ok = dict(prev=one, next=one, channels=3, h=64, w=64, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.1, flags=0,
              scratch=one, fx=one, fy=one)

    def call(**over):
        a = {**ok, **over}
        return hip_lib.fw_farneback_flow_u8(a["prev"], a["next"], a["channels"], a["h"], a["w"], a["pyr_scale"], a["levels"], a["winsize"],
                                            a["iterations"], a["poly_n"], a["poly_sigma"], a["flags"], a["scratch"], a["fx"], a["fy"], None)

    for over, word in [(dict(poly_n=7), b"poly_n"), (dict(winsize=16), b"winsize"), (dict(channels=2), b"channels"),
                       (dict(scratch=None), b"null"), (dict(flags=256), b"flags"), (dict(flags=4), b"flags"),
                       (dict(pyr_scale=1.0), b"pyr_scale"), (dict(h=2048, w=2048, levels=5), b"19 taps"), (dict(iterations=0), b"iterations")]:
        assert call(**over) == _lib.FW_ERR_INVALID, over
        assert word in hip_lib.fw_last_error(), (over, hip_lib.fw_last_error())
    assert hip_lib.fw_farneback_scratch_bytes(0, 10, 3) == 0
    assert hip_lib.fw_farneback_scratch_bytes(1080, 1920, 3) >= 27 * 1080 * 1920 * 4
    assert hip_lib.fw_flow_stats_f32(None, one, 4, 4, None, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_flow_confidence_f32(one, None, None, None, 4, 4, one, None, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_flow_confidence_f32(one, one, None, None, 4, 4, None, one, None) == _lib.FW_ERR_INVALID     # weight map without magnitude
    assert hip_lib.fw_abi_version() == 4
