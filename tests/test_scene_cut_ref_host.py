"""tests/scene_cut_ref.py, the contract of csrc/scene_cuts.hip, against the host functions it restates (no GPU): the integer-moment
SSIM against `policy.ssim_gray_u8`, the counts against np.histogram, the decisions against `policy.scene_change` on the reference
run's clip (tests/golden/interpolator_reference.*), and the C-ABI's new names."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_cut_ref as sr  # noqa: E402

from framewright_amd import _lib, policy  # noqa: E402

GOLD = Path(__file__).parent / "golden"
J = json.loads((GOLD / "interpolator_reference.json").read_text())
CLIP = np.load(GOLD / "interpolator_reference.npz")["clip"]

SHAPES = [(7, 7), (7, 64), (64, 7), (9, 13), (16, 70), (33, 131), (64, 96), (70, 300), (270, 480)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_ssim_restatement_equals_the_host_ssim(h, w):
    """1e-12 is the tolerance tests/test_interpolator_host.py holds `policy.ssim_gray_u8` to against scipy; the two forms differ by
    a few roundings per map value (observed below 1e-14)."""
    for kind in sr.PAIR_KINDS:
        a, b = sr.make_pair(kind, h, w)
        got, want = sr.ssim_frames(a, b), policy.ssim_gray_u8(sr.mean_gray(a), sr.mean_gray(b))
        assert abs(got - want) <= 1e-12, (kind, got, want)
        assert -1.0 <= got <= 1.0
    a, _ = sr.make_pair("const255", h, w)
    assert sr.ssim_frames(a, a) == 1.0                     # numerator and denominator are the same float64 products
    a, _ = sr.make_pair("random", h, w)
    assert sr.ssim_frames(a, a) == 1.0
    assert sr.ssim_frames(*sr.make_pair("complement", h, w)) < 0.0


def test_moments_are_exact_and_within_int32():
    """The extremes of the integers the kernel keeps in 32 bits: all 255 (sums at their maximum), half 0 / half 255 (the largest
    central moment) and its complement (the most negative cross moment)."""
    a = np.full((7, 7), 255, np.int64)
    assert a.sum() == 12495 and (a * a).sum() == 3186225 < 2 ** 22
    assert 2 * 12495 * 12495 < 2 ** 31 and 49 * 3186225 < 2 ** 28
    x = np.zeros(49, np.int64)
    x[:24] = 255
    y = 255 - x
    mxx, mxy = 49 * (x * x).sum() - x.sum() ** 2, 49 * (x * y).sum() - x.sum() * y.sum()
    assert 0 < mxx < 2 ** 26 and -2 ** 26 < mxy < 0


def test_mean_gray_is_the_integer_third_for_all_766_sums():
    for s in range(766):
        c0 = min(s, 255)
        c1 = min(s - c0, 255)
        px = np.array([[[c0, c1, s - c0 - c1]]], np.uint8)
        assert int(px.astype(int).sum()) == s
        assert sr.mean_gray(px)[0, 0] == np.mean(px, axis=2).astype(np.uint8)[0, 0] == s // 3
        assert sr.mean_gray(px[:, :, ::-1])[0, 0] == s // 3


@pytest.mark.parametrize("h,w", [(1, 1), (5, 9), (9, 13), (40, 56)])
def test_histogram_counts_equal_numpy(h, w):
    rng = np.random.default_rng(h * 100 + w)
    for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 3), 255, np.uint8), np.full((h, w, 3), 131, np.uint8)):
        want = np.stack([np.histogram(img[:, :, c], bins=64, range=(0, 256))[0] for c in range(3)])
        assert np.array_equal(sr.hist64x3(img), want)
        assert sr.hist64x3(img).sum() == h * w * 3


def test_decisions_equal_the_host_policy():
    # the reference run's clip: its histogram-branch flags and the boundaries of the full test, in either channel order
    n = len(CLIP)
    flags = [sr.histogram_decision(sr.hist64x3(CLIP[k]), sr.hist64x3(CLIP[k + 1]), 0.3) for k in range(n - 1)]
    assert flags == J["pair_flags"] == [policy.scene_change_by_histogram(CLIP[k], CLIP[k + 1], 0.3) for k in range(n - 1)]
    assert flags == [sr.scene_change(CLIP[k], CLIP[k + 1], 0.3, use_ssim=False) for k in range(n - 1)]
    assert sr.detect_clip(CLIP, 0.3) == J["scene_boundaries"]
    assert sr.detect_clip(CLIP[:, :, :, ::-1], 0.3) == J["scene_boundaries"]
    for thr in (0.1, 0.3, 0.5, 0.9):
        for k in range(n - 1):
            assert sr.scene_change(CLIP[k], CLIP[k + 1], thr) == policy.scene_change(CLIP[k], CLIP[k + 1], thr)
    # synthetic pairs, the fallback sizes included (a side shorter than 7, frames of different sizes)
    for h, w in [(5, 9), (9, 5), (4, 4), (9, 13), (33, 131)]:
        for kind in sr.PAIR_KINDS:
            a, b = sr.make_pair(kind, h, w)
            for thr in (0.3, 0.5):
                assert sr.scene_change(a, b, thr) == policy.scene_change(a, b, thr), (h, w, kind, thr)
    a, b = sr.make_pair("random", 9, 13)[0], sr.make_pair("random", 16, 70)[0]
    assert sr.scene_change(a, b) == policy.scene_change(a, b)


def test_the_c_abi_names_the_scene_cut_entries():
    for name in ("fw_scene_ssim_u8", "fw_scene_ssim_workspace_bytes", "fw_hist64x3_u8"):
        assert name in _lib.EXPORTS


def test_entries_refuse_bad_arguments_without_a_device(hip_lib):
    """Argument checks come before any launch, so they run without a GPU; the workspace helper is a host function."""
    import ctypes as C
    one = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert hip_lib.fw_scene_ssim_workspace_bytes(1, 1080, 1920) == 8 * 30 * 34        # 64 x 32 tiles of the 1074 x 1914 map
    assert hip_lib.fw_scene_ssim_workspace_bytes(5, 7, 7) == 8 * 5
    assert hip_lib.fw_scene_ssim_workspace_bytes(1, 6, 64) == 0 and hip_lib.fw_scene_ssim_workspace_bytes(0, 64, 64) == 0
    assert hip_lib.fw_scene_ssim_u8(one, one, 0, 1, 5, 9, one, one, None) == _lib.FW_ERR_INVALID
    assert b"fw_scene_ssim_u8" in hip_lib.fw_last_error() and b"window" in hip_lib.fw_last_error()
    assert hip_lib.fw_scene_ssim_u8(None, one, 0, 1, 9, 9, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_scene_ssim_u8(one, one, 0, 0, 9, 9, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_scene_ssim_u8(one, one, 0, 2, 9, 9, one, one, None) == _lib.FW_ERR_INVALID       # two pairs, no stride
    assert hip_lib.fw_scene_ssim_u8(one, one, -1, 1, 9, 9, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_hist64x3_u8(None, 1, 4, 4, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_hist64x3_u8(one, 0, 4, 4, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_hist64x3_u8(one, 1, 0, 4, one, None) == _lib.FW_ERR_INVALID
    assert b"fw_hist64x3_u8" in hip_lib.fw_last_error()


def test_interpolator_flag_is_keyword_only_and_off_by_default():
    from framewright_amd import rife as RF
    assert RF.FrameInterpolator()._device_scene_detection is False
    assert RF.FrameInterpolator(device_scene_detection=True)._device_scene_detection is True
    with pytest.raises(TypeError):
        RF.FrameInterpolator("rife-v4.6", 0, None, True)
