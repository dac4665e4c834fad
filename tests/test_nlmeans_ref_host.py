"""The contract of the non-local-means spatial denoise (tests/nlmeans_ref.py) and the host half of its implementation
(fw_nlmeans_weight_table, fw_nlmeans_lab_tables: csrc/nlmeans.hip), no GPU needed.  cv2 is not installed here: the restatement is
OpenCV's 8-bit algorithm as recalled and parity with cv2 itself is unpinned."""
import ctypes as C
import inspect
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nlmeans_ref as nr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import temporal_denoise as TD  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("channels,template,search", [(1, 7, 21), (2, 7, 21), (3, 7, 21), (1, 3, 7), (2, 3, 7), (3, 5, 9)])
def test_fast_restatement_equals_literal(channels, template, search):
    """Running box sums against four nested loops that sum every patch term by term; sides shorter than the border included."""
    plane = nr.noisy_pattern(9, 12, channels, 4.0, seed=channels)
    fast = nr.nlmeans(plane, 6, template, search)
    np.testing.assert_array_equal(fast, nr.nlmeans_literal(plane, 6, template, search))
    assert (fast != plane).any()


def test_even_windows_are_forced_odd_in_the_restatement():
    plane = nr.noisy_pattern(10, 11, 1, 4.0, seed=5)
    np.testing.assert_array_equal(nr.nlmeans(plane, 6, 4, 8), nr.nlmeans(plane, 6, 5, 9))


def test_constant_image_is_returned_unchanged():
    for c in (1, 2, 3):
        plane = np.full((12, 15, c), 77 + c, np.uint8)
        np.testing.assert_array_equal(nr.nlmeans(plane, 6), plane)
    with pytest.raises(ValueError):
        nr.nlmeans(np.zeros((1, 9, 1), np.uint8), 6)


def test_table_constants():
    assert nr.table_constants(7, 21) == (19096, 6, 64.0 / 49.0)
    assert nr.table_constants(3, 7)[1] == 4
    assert len(nr.weight_table(5, 1)) == 49785 and len(nr.weight_table(5, 2)) == 99570


# ------------------------------------------------------------------------------------------------ the library's host functions
def _lib_table(lib, h, channels, template=7, search=21):
    n = lib.fw_nlmeans_weight_table(float(h), channels, template, search, None, 0)
    out = np.zeros(max(n, 1), np.int32)
    assert lib.fw_nlmeans_weight_table(float(h), channels, template, search, C.c_void_p(out.ctypes.data), n) == n
    return out[:n]


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_weight_table_equals_the_restatement(hip_lib, channels):
    for h in range(3, 11):
        want = nr.weight_table(h, channels)
        got = _lib_table(hip_lib, h, channels)
        assert len(got) == nr.table_length(want)
        np.testing.assert_array_equal(got, want[:len(got)])
        assert got[0] == 19096 and got[-1] > 0
    for template, search in ((3, 7), (5, 11)):
        want = nr.weight_table(6, channels, template, search)
        got = _lib_table(hip_lib, 6, channels, template, search)
        np.testing.assert_array_equal(got, want[:nr.table_length(want)])


def test_weight_table_lengths_and_refusals(hip_lib):
    lengths = {(c, h): hip_lib.fw_nlmeans_weight_table(float(h), c, 7, 21, None, 0) for c in (1, 2) for h in (5, 6, 10)}
    assert [lengths[1, h] for h in (5, 6, 10)] == [132, 190, 528]
    assert [lengths[2, h] for h in (5, 6, 10)] == [264, 380, 1055]
    buf = np.zeros(8, np.int32)
    for bad in [(0.0, 1, 7, 21), (-1.0, 1, 7, 21), (6.0, 0, 7, 21), (6.0, 4, 7, 21), (6.0, 1, 6, 21), (6.0, 1, 7, 20), (6.0, 1, 0, 21),
                (6.0, 1, 7, -3), (float("nan"), 1, 7, 21)]:
        assert hip_lib.fw_nlmeans_weight_table(*bad, None, 0) == 0, bad
    assert hip_lib.fw_nlmeans_weight_table(6.0, 1, 7, 21, C.c_void_p(buf.ctypes.data), 8) == 0      # capacity too small
    assert b"capacity" in hip_lib.fw_last_error() and not buf.any()
    assert hip_lib.fw_nlmeans_scratch_bytes(1080, 1920, 21) >= 6 * 1080 * 1920
    for bad in [(1, 64, 21), (64, 1, 21), (64, 64, 20), (64, 64, 0), (64, 64, 43), (-5, 64, 21)]:
        assert hip_lib.fw_nlmeans_scratch_bytes(*bad) == 0, bad


def _lab_table(lib, which):
    n = lib.fw_nlmeans_lab_tables(which, None, 0)
    out = np.zeros(n, np.int32)
    assert n > 0 and lib.fw_nlmeans_lab_tables(which, C.c_void_p(out.ctypes.data), n) == n
    return out


def test_colour_tables_equal_the_restatement(hip_lib):
    t = nr.lab_tables()
    np.testing.assert_array_equal(_lab_table(hip_lib, 0), t["cbrt"])
    np.testing.assert_array_equal(_lab_table(hip_lib, 1), t["fwd_coef"].reshape(-1))
    np.testing.assert_array_equal(_lab_table(hip_lib, 2), np.concatenate([t["fy"], t["yl"], t["ax"], t["bz"]]))
    np.testing.assert_array_equal(_lab_table(hip_lib, 3), np.concatenate([t["inv_coef"].reshape(-1), t["inv_const"]]))
    assert (t["fwd_coef"].astype(np.int64).sum(axis=1) == 1 << nr.COEF_BITS).all()
    assert hip_lib.fw_nlmeans_lab_tables(4, None, 0) == 0


def _cube_chunks():
    g = np.arange(256, dtype=np.uint8)
    for first in range(0, 256, 16):
        yield np.stack(np.meshgrid(g[first:first + 16], g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_colour_transforms_within_one_lsb_of_the_textbook_over_both_cubes():
    """Every one of the 2^24 BGR colours and every one of the 2^24 Lab triples: the integer transform is within 1 LSB per channel of
    the formula evaluated in float64, rounded and saturated."""
    worst_f = worst_i = 0
    for cube in _cube_chunks():
        worst_f = max(worst_f, int(np.abs(nr.bgr_to_lab(cube).astype(np.int16) - nr.bgr_to_lab_textbook(cube).astype(np.int16)).max()))
        worst_i = max(worst_i, int(np.abs(nr.lab_to_bgr(cube).astype(np.int16) - nr.lab_to_bgr_textbook(cube).astype(np.int16)).max()))
    print(f"largest deviation from the float64 formulas: forward {worst_f} LSB, inverse {worst_i} LSB")
    assert worst_f <= 1 and worst_i <= 1


def test_colour_anchor_values():
    lab = nr.bgr_to_lab(np.array([[255, 255, 255], [0, 0, 0], [128, 128, 128]], np.uint8))
    np.testing.assert_array_equal(lab[0], [255, 128, 128])
    np.testing.assert_array_equal(lab[1], [0, 128, 128])
    assert lab[2, 1] == 128 and lab[2, 2] == 128
    np.testing.assert_array_equal(nr.lab_to_bgr(lab[:2]), [[255, 255, 255], [0, 0, 0]])


# ------------------------------------------------------------------------------------------------ the Python surface, without a GPU
def test_h_for_strength_and_signatures():
    assert [TD.DeviceSpatialDenoiser.h_for_strength(s) for s in (0.31, 0.5, 1.0)] == [5, 6, 10]
    assert [nr.h_for_strength(s) for s in (0.31, 0.5, 1.0)] == [5, 6, 10]
    sig = inspect.signature(TD.DeviceSpatialDenoiser.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("gpu_id", 0), ("template_window", 7), ("search_window", 21)]
    for name in ("denoise_device", "denoise", "nlmeans_device"):
        assert callable(getattr(TD.DeviceSpatialDenoiser, name))
    seq = inspect.signature(TD.DeviceTemporalAccumulator.denoise_sequence).parameters
    assert seq["noise_strength"].default is None and tuple(seq["scene_changes"].default) == ()
    assert seq["preserve_edges"].default is False and seq["temporal_radius"].default == 3        # today's defaults stay


def test_denoise_sequence_arguments_are_validated_without_a_gpu():
    chk = TD.DeviceTemporalAccumulator._check_sequence_args
    assert chk(5, 3, None, ()) == (False, set())
    assert chk(5, 3, 0.3, ()) == (False, set())                   # `> 0.3`, as the reference
    assert chk(5, 3, 0.31, [4, 0, 4]) == (True, {0, 4})
    assert chk(5, 1, 0.5, (np.int64(2),)) == (True, {2})
    for bad in [dict(temporal_radius=0), dict(noise_strength=-0.1), dict(noise_strength=float("nan")), dict(noise_strength="0.5"),
                dict(noise_strength=True), dict(scene_changes=[5]), dict(scene_changes=[-1]), dict(scene_changes=[1.0])]:
        args = dict(n=5, temporal_radius=3, noise_strength=None, scene_changes=())
        args.update(bad)
        with pytest.raises(ValueError):
            chk(**args)


# ------------------------------------------------------------------------------------------------ the GPU cases are not degenerate
@pytest.mark.parametrize("case", nr.core_cases(), ids=lambda c: c[0])
def test_core_cases_are_lively(case):
    """A condition on the INPUTS of tests/test_nlmeans_gpu.py: where the centre is the only offset with weight, non-local means
    returns its input and a broken kernel would pass.  Every case but the one named degenerate changes at least half of its pixels
    and gives weight to at least 20 offsets per pixel on average."""
    name, plane, h, template, search, exempt = case
    changed, offsets = nr.liveliness(plane, h, template, search)
    print(f"{name}: {100 * changed:.1f} % of the pixels change, {offsets:.1f} non-zero-weight offsets per pixel")
    if exempt:
        assert "degenerate" in name and offsets < 20
    else:
        assert changed >= 0.5 and offsets >= 20


@pytest.mark.parametrize("case", nr.colored_cases(), ids=lambda c: c[0])
def test_coloured_cases_are_lively_on_their_lab_planes(case):
    name, bgr, h, h_color = case
    lab = nr.bgr_to_lab(bgr)
    for plane_name, plane, hh in (("L", lab[:, :, :1], h), ("ab", lab[:, :, 1:], h_color)):
        changed, offsets = nr.liveliness(np.ascontiguousarray(plane), hh)
        print(f"{name} {plane_name}: {100 * changed:.1f} % of the pixels change, {offsets:.1f} non-zero-weight offsets per pixel")
        assert changed >= 0.5 and offsets >= 20
