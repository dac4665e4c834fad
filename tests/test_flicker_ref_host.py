"""The contract of the flicker reduction (tests/flicker_ref.py) and the host half of its implementation (fw_gamma_lab_tables,
DeviceFlickerReducer.l_luts: csrc/flicker.hip, temporal_denoise.py), no GPU needed.  cv2 is not installed here: the transforms are
the sRGB / CIE Lab formulas in fixed point and parity with cv2 itself is unpinned."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flicker_ref as fr  # noqa: E402
import nlmeans_ref as nr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402

NEW_ENTRIES = ["fw_bgr_to_lab_u8", "fw_lab_to_bgr_u8", "fw_lab_l_sums_u8", "fw_deflicker_lab_u8", "fw_gamma_lab_tables"]


# ------------------------------------------------------------------------------------------------ the two transforms
def test_integer_transforms_stay_within_one_lsb_of_the_textbook():
    """K10's bound for the linear pair, for the gamma pair: forward on every 5th level plus 255 per channel (53^3 colours) and the
    256 grays, inverse on the Lab bytes those colours produce."""
    colours = fr.lattice()
    assert colours.shape == (53 ** 3 + 256, 3)
    lab = fr.bgr_to_lab_gamma(colours)
    d_fwd = np.abs(lab.astype(int) - fr.bgr_to_lab_gamma_textbook(colours).astype(int))
    d_inv = np.abs(fr.lab_to_bgr_gamma(lab).astype(int) - fr.lab_to_bgr_gamma_textbook(lab).astype(int))
    print(f"forward: max {d_fwd.max()} LSB, {100 * (d_fwd > 0).any(axis=1).mean():.2f} % of the colours differ; "
          f"inverse: max {d_inv.max()} LSB, {100 * (d_inv > 0).any(axis=1).mean():.2f} %")
    assert d_fwd.max() <= 1 and d_inv.max() <= 1


def test_transform_landmarks():
    px = lambda *v: np.array([v], np.uint8)
    np.testing.assert_array_equal(fr.bgr_to_lab_gamma(px(255, 255, 255)), px(255, 128, 128))      # white lands on the last f(t) entry
    np.testing.assert_array_equal(fr.bgr_to_lab_gamma(px(0, 0, 0)), px(0, 128, 128))
    np.testing.assert_array_equal(fr.lab_to_bgr_gamma(px(255, 128, 128)), px(255, 255, 255))
    np.testing.assert_array_equal(fr.lab_to_bgr_gamma(px(0, 128, 128)), px(0, 0, 0))
    grays = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    lab = fr.bgr_to_lab_gamma(grays)
    assert (np.diff(lab[:, 0].astype(int)) >= 0).all() and np.abs(lab[:, 1:].astype(int) - 128).max() <= 1
    # the gamma is in: mid-gray 128 is L* ~ 53.6, far from the 76.1 of the linear pair
    assert abs(int(lab[128, 0]) - round(53.585 * 2.55)) <= 1 and int(nr.bgr_to_lab(grays)[128, 0]) > int(lab[128, 0]) + 40
    assert np.abs(fr.lab_to_bgr_gamma(lab).astype(int) - grays).max() <= 2


def test_encode_thresholds_are_the_encode_table():
    enc, thr = fr.gamma_tables()["encode"], fr.encode_thresholds()
    assert thr.shape == (255,) and (np.diff(thr) > 0).all() and thr[-1] <= fr.LIN_MAX
    np.testing.assert_array_equal(np.searchsorted(thr, np.arange(fr.LIN_MAX + 1), side="right"), enc)


def test_library_tables_equal_the_contract(hip_lib):
    want = [fr.gamma_tables()["decode"], fr.gamma_tables()["encode"], fr.encode_thresholds()]
    for which, w in enumerate(want):
        n = hip_lib.fw_gamma_lab_tables(which, None, 0)
        assert n == w.size
        got = np.zeros(n, np.int32)
        assert hip_lib.fw_gamma_lab_tables(which, C.c_void_p(got.ctypes.data), n) == n
        np.testing.assert_array_equal(got, w)
        assert hip_lib.fw_gamma_lab_tables(which, C.c_void_p(got.ctypes.data), n - 1) == 0
    assert hip_lib.fw_gamma_lab_tables(3, None, 0) == 0 and b"which" in hip_lib.fw_last_error()
    assert hip_lib.fw_gamma_lab_tables(-1, None, 0) == 0


# ------------------------------------------------------------------------------------------------ the fallback's arithmetic
@pytest.mark.parametrize("lut_fn", [fr.l_lut, lambda s, n, t: TD.DeviceFlickerReducer.l_luts([s], n, t)[0]], ids=["contract", "product"])
def test_l_lut(lut_fn):
    levels = np.arange(256)
    n = 1000
    shifted = lambda d: np.clip(levels + d, 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(lut_fn(100 * n, n, 100.0), levels)                  # adj = 0
    np.testing.assert_array_equal(lut_fn(100 * n, n, 120.0), shifted(10))             # adj = +20 exactly
    np.testing.assert_array_equal(lut_fn(100 * n, n, 80.0), shifted(-10))             # adj = -20 exactly
    np.testing.assert_array_equal(lut_fn(100 * n, n, 190.0), shifted(10))             # beyond the clamp
    np.testing.assert_array_equal(lut_fn(200 * n, n, 3.5), shifted(-10))
    # truncation, not rounding: adj * 0.5 = 2.9 maps L to L + 2, and -2.9 maps L to L - 3 (L - 2.9 is positive: truncated down)
    np.testing.assert_array_equal(lut_fn(100 * n, n, 105.8), shifted(2))
    np.testing.assert_array_equal(lut_fn(100 * n, n, 94.2), shifted(-3))
    assert lut_fn(100 * n, n, 105.8)[250:].tolist() == [252, 253, 254, 255, 255, 255]
    # the mean is the exact quotient: l_sum / n_pixels in float64
    np.testing.assert_array_equal(lut_fn(100 * n + 1, n, 100.0 + 6.001), shifted(3))
    np.testing.assert_array_equal(lut_fn(100 * n + 2, n, 100.0 + 6.001), shifted(2))
    assert lut_fn(0, 1, 0.0).dtype == np.uint8


def test_numpy_promotion_the_lut_relies_on():
    """`l.astype(np.float32) + adjustment * 0.5` is float64 under NumPy >= 2 because np.clip of a float64 scalar is an np.float64."""
    adj = np.clip(np.median([1.5, 2.5]) - np.mean(np.zeros((2, 2), np.uint8)), -20, 20)
    assert isinstance(adj, np.float64)
    if int(np.__version__.split(".")[0]) >= 2:
        assert (np.zeros(3, np.float32) + adj * 0.5).dtype == np.float64


def test_target_brightness_even_and_odd_sample_counts():
    flat = lambda v: np.full((4, 6, 3), v, np.uint8)
    clip = [flat(0)] * 21
    clip[0], clip[10], clip[20] = flat(10), flat(60), flat(30)
    assert fr.target_brightness(clip) == 30.0                       # three samples: the middle one
    assert fr.target_brightness(clip[:20]) == 35.0                  # two samples: their mean
    assert fr.target_brightness(clip[:1]) == 10.0
    # at most 50 samples: frame 500 is not read
    assert fr.target_brightness([flat(7)] * 500 + [flat(255)]) == 7.0
    # the mean gray is the exact integer sum over N, of cvtColor's 14-bit gray
    f = np.zeros((1, 3, 3), np.uint8)
    f[0, 0] = (255, 0, 0)
    assert fr.gray(f)[0, 0] == (1868 * 255 + 8192) >> 14 == 29 and fr.target_brightness([f]) == 29 / 3


def test_reduce_flicker_dict_and_adaptive_thresholds():
    clip = fr.flicker_clip(3)
    out, res = fr.reduce_flicker(clip)
    assert res == {"success": True, "frames_processed": 3, "method": "python_brightness_normalization", "mode_used": "adaptive"}
    for o, w in zip(out, fr.python_deflicker(clip)):
        np.testing.assert_array_equal(o, w)
    for sev, want in [(0.0, "light"), (0.0999, "light"), (0.1, "medium"), (0.2999, "medium"), (0.3, "aggressive"), (1.0, "aggressive")]:
        assert fr.reduce_flicker(clip, "adaptive", sev)[1]["mode_used"] == want
        assert fr.reduce_flicker(clip, "light", sev)[1]["mode_used"] == "light"
    assert fr.reduce_flicker([], "adaptive", 0.5) == ([], {"frames_processed": 0, "mode_used": None})
    # the mode changes no pixel on this path
    for o, w in zip(fr.reduce_flicker(clip, "aggressive", 0.9)[0], out):
        np.testing.assert_array_equal(o, w)


def test_the_gpu_clip_is_lively_under_the_restatement_alone():
    """What tests/test_flicker_gpu.py asks of the 23-frame clip, established here on the CPU: [::10] samples three frames, at least
    one frame hits the +-20 clamp and one does not, more than half of the frames change in more than half of their pixels, and the
    standard deviation of the per-frame mean gray falls."""
    clip = fr.flicker_clip()
    assert len(clip) == 23 and clip[0].shape == (40, 56, 3) and len(clip[::10][:50]) == 3
    target = fr.target_brightness(clip)
    adj = [target - fr.bgr_to_lab_gamma(f)[..., 0].astype(np.int64).sum() / (40 * 56) for f in clip]
    assert any(abs(a) > 20 for a in adj) and any(abs(a) < 20 for a in adj)
    out = fr.python_deflicker(clip)
    changed = [(o != f).any(axis=2).mean() for o, f in zip(out, clip)]
    assert sum(c > 0.5 for c in changed) > len(clip) / 2
    std = lambda fs: float(np.std([fr.gray(f).mean() for f in fs]))
    print(f"target {target:.2f}, adjustments {min(adj):.1f} .. {max(adj):.1f}, std of mean gray {std(clip):.2f} -> {std(out):.2f}")
    assert std(out) < std(clip)


# ------------------------------------------------------------------------------------------------ the public surface
def test_new_entries_are_exported_and_declared(hip_lib):
    header = (Path(__file__).resolve().parent.parent / "include" / "framewright_hip.h").read_text()
    declared = set(re.findall(r"\b(fw_[a-z0-9_]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in declared and hasattr(hip_lib, name)
    assert "Additive entries no longer bump the version" in header and hip_lib.fw_abi_version() == 4


def test_driver_surface():
    import inspect
    sig = inspect.signature(TD.DeviceFlickerReducer.__init__).parameters
    assert sig["mode"].default is TD.FlickerMode.ADAPTIVE and sig["preserve_brightness_changes"].default is True and sig["gpu_id"].default == 0
    for name in ("analyze_flicker", "reduce_flicker_device", "reduce_flicker"):
        assert callable(getattr(TD.DeviceFlickerReducer, name))
    assert inspect.signature(TD.DeviceTemporalDenoiser.__init__).parameters["device_flicker"].default is False
    assert inspect.signature(TD.create_temporal_denoiser).parameters["device_flicker"].default is False
