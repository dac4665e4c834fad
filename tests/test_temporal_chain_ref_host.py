"""The contract of the clip analysis and the temporal-consistency pass (tests/temporal_chain_ref.py) against hand-checkable cases,
and the pure host half of framewright_amd.temporal_denoise against that contract.  No GPU needed."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import temporal_chain_ref as tr  # noqa: E402

from framewright_amd import temporal_denoise as TD  # noqa: E402
from framewright_amd.synth import synthetic_frames  # noqa: E402

THRESHOLD = 0.7        # TemporalDenoiseConfig.scene_change_threshold
MARGIN = 0.1           # every asserted cut / no-cut decision is at least this far from the threshold


def darkened_clip(n, cut, end=None, h=72, w=96, seed=1):
    """A synthetic clip whose frames cut .. end - 1 (to the last one by default) are divided by three: a hard change of the gray
    histogram at `cut`, and back at `end`."""
    frames = list(synthetic_frames(n, h, w, seed))
    return [f // 3 if cut <= i < (n if end is None else end) else f for i, f in enumerate(frames)]


# ---------------------------------------------------------------------------------------------------------- hand-checkable cases
def test_laplacian_of_an_impulse():
    gray = np.zeros((5, 7), np.uint8)
    gray[2, 3] = 10
    lap = tr.laplacian(gray)
    want = np.zeros((5, 7), np.int64)
    want[2, 3] = -40
    want[1, 3] = want[3, 3] = want[2, 2] = want[2, 4] = 10
    np.testing.assert_array_equal(lap, want)
    # at the border the missing neighbour is the mirror image of the opposite one (reflect-101): it counts twice
    gray = np.zeros((4, 4), np.uint8)
    gray[0, 1] = 5
    lap = tr.laplacian(gray)
    assert lap[0, 1] == -20 and lap[1, 1] == 5 and lap[0, 0] == 5 + 5 and lap[0, 2] == 5
    gray = np.zeros((4, 4), np.uint8)
    gray[1, 2] = 5
    assert tr.laplacian(gray)[0, 2] == 5 + 5 and tr.laplacian(gray)[2, 2] == 5
    # a one-pixel side mirrors onto itself: only the long direction contributes
    row = np.array([[1, 4, 9, 16]], np.uint8)
    np.testing.assert_array_equal(tr.laplacian(row), [[2 * 4 - 2 * 1, 1 + 9 - 2 * 4, 4 + 16 - 2 * 9, 2 * 9 - 2 * 16]])


def test_histogram_of_a_two_level_image_and_gray_weights():
    frame = np.zeros((6, 10, 3), np.uint8)
    frame[:, :4] = 200                                  # gray of (v, v, v) is v: the weights sum to 2^14
    hist, s1, s2 = tr.frame_stats(frame)
    assert hist[200] == 24 and hist[0] == 36 and hist.sum() == 60
    assert s1 == 0 and s2 == 6 * 2 * 200 * 200          # the step: one column of +200 and one of -200 in every row
    assert tr.gray_u8(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() == [[29, 150, 76]]
    assert TD.brightness_from_hist(hist) == tr.brightness(frame) == 80.0


def test_correlation_of_a_histogram_with_itself_is_one():
    h = tr.normalised_hist(synthetic_frames(1, 40, 56, 3)[0])
    assert abs(tr.correlation(h, h) - 1.0) < 1e-12
    assert tr.correlation(np.ones(256, np.float32), np.ones(256, np.float32)) == 1.0     # no variance: OpenCV's 1.0
    rev = h[::-1].copy()
    assert tr.correlation(h, rev) < 0.9


# ---------------------------------------------------------------------------------------------------------------- the scene loop
@pytest.mark.parametrize("n,cut,end,sample_rate,want", [(12, 5, None, 1, [5]), (12, 5, None, 5, [5]), (12, 7, None, 5, [10]),
                                                        (7, 5, 6, 5, [5, 10])])
def test_scene_loop(n, cut, end, sample_rate, want):
    """The loop compares (i, min(i + rate, n - 1)) and records i + rate: a cut between two sampled frames is reported at the later
    one, and the last pair of a short clip, (5, 6) of 7 frames, records 10 - an index beyond the clip.  (The 7-frame clip darkens
    frame 5 alone, so that both of its pairs, (0, 5) and (5, 6), straddle a change.)"""
    frames = darkened_clip(n, cut, end)
    pairs = tr.scene_pairs(frames, sample_rate)
    assert [(i, j) for i, j, _ in pairs] == [(i, min(i + sample_rate, n - 1)) for i in range(0, n - 1, sample_rate)]
    for i, j, corr in pairs:
        print(f"pair ({i}, {j}): correlation {corr:.4f}")
        assert abs(corr - THRESHOLD) >= MARGIN, (i, j, corr)
    assert tr.scene_changes(frames, sample_rate, THRESHOLD) == want
    hists = [tr.histogram(tr.gray_u8(f)) for f in frames]
    assert TD.scene_changes_from_hists(hists, sample_rate, THRESHOLD) == want
    if n == 7:
        assert max(want) >= n                                                            # the index the driver has to drop


def test_a_change_of_seed_is_not_a_cut():
    a, b = synthetic_frames(1, 72, 96, 1)[0], synthetic_frames(1, 72, 96, 2)[0]
    corr = tr.correlation(tr.normalised_hist(a), tr.normalised_hist(b))
    assert corr >= THRESHOLD + MARGIN
    assert tr.scene_changes([a, b], 1, THRESHOLD) == []
    assert tr.scene_changes([a], 1, THRESHOLD) == [] and TD.scene_changes_from_hists([None], 1, THRESHOLD) == []


# -------------------------------------------------------------------------------------------------- exact variance against numpy
@pytest.mark.parametrize("h,w,seed", [(72, 96, 1), (37, 53, 2), (270, 480, 3), (1, 9, 4)])
def test_exact_variance_against_numpy(h, w, seed):
    """(N S2 - S1^2) / N^2 from exact integer sums against np.var of the float64 Laplacian.  numpy's pairwise sums over <= 2^23
    positive terms err by about 23 eps ~ 3e-15 relative: 1e-12 leaves three orders of margin."""
    rng = np.random.default_rng(seed)
    frame = np.clip(synthetic_frames(1, h, w, seed)[0].astype(int) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    hist, s1, s2 = tr.frame_stats(frame)
    want = tr.laplacian(tr.gray_u8(frame)).astype(np.float64).var()
    got = tr.variance_exact(h * w, s1, s2)
    assert want > 0 and abs(got - want) <= 1e-12 * want
    assert TD.laplacian_variance(h * w, s1, s2) == got
    assert TD.brightness_from_hist(hist) == tr.brightness(frame)


# ------------------------------------------------------------------------------------ the library's host functions = the contract
def flickering_clip(n, amp):
    frames = synthetic_frames(n, 40, 56, 7).astype(int)
    return [np.clip(f + amp * (-1) ** i + 3 * (i % 3), 0, 255).astype(np.uint8) for i, f in enumerate(frames)]


@pytest.mark.parametrize("n,amp,sample_rate", [(12, 0, 1), (12, 30, 1), (31, 8, 5), (40, 60, 2), (2, 30, 1), (10, 30, 5)])
def test_flicker_metrics_equal_the_restatement(n, amp, sample_rate):
    frames = flickering_clip(n, amp)
    got = TD.flicker_metrics_from_brightness([TD.brightness_from_hist(tr.histogram(tr.gray_u8(f))) for f in frames], sample_rate)
    assert got == tr.flicker_metrics(frames, sample_rate)
    if n == 2 or (n == 10 and sample_rate == 5):
        assert got["severity"] == 0.0 and "mean_brightness_diff" not in got                # fewer than three samples
    if amp >= 30 and n >= 12:
        assert got["recommended_mode"] == "aggressive" and got["frequency"] > 0


def test_noise_level_and_noise_reduction_equal_the_restatement():
    rng = np.random.default_rng(5)
    clean = list(synthetic_frames(14, 40, 56, 5))
    noisy = [np.clip(f.astype(int) + rng.normal(0, 12, f.shape), 0, 255).astype(np.uint8) for f in clean]
    var = lambda f: TD.laplacian_variance(f.shape[0] * f.shape[1], *tr.frame_stats(f)[1:])
    for rate in (1, 5):
        got = TD.noise_level_from_variances([var(f) for f in noisy], rate)
        assert got == tr.noise_level(noisy, rate) and 0 < got < 1
    assert TD.noise_level_from_variances([], 5) == 0.0
    assert TD.noise_level_from_variances([1e9], 1) == 1.0
    got = TD.noise_reduction_from_variances([var(f) for f in noisy], [var(f) for f in clean])
    assert got == tr.noise_reduction(noisy, clean) and 0.3 < got < 1
    assert TD.noise_reduction_from_variances([var(f) for f in clean], [var(f) for f in noisy]) == 0.0   # clipped below
    assert TD.noise_reduction_from_variances([], []) == 0.0 and TD.noise_reduction_from_variances([0.0], [1.0]) == 0.0


@pytest.mark.parametrize("noise,cuts,severity,mode", [(0.1, 0, 0.0, "light"), (0.3, 11, 0.5, "aggressive"), (0.8, 2, 0.31, "medium"),
                                                      (0.5, 0, 0.3, "medium"), (0.2, 10, 0.0, "light")])
def test_recommendations_equal_the_restatement(noise, cuts, severity, mode):
    analysis = {"noise_level": noise, "scene_changes": list(range(cuts)), "flicker_metrics": {"severity": severity, "recommended_mode": mode}}
    cfg = TD.TemporalDenoiseConfig(enable_flicker_reduction=False)
    got = TD.generate_recommendations(analysis, cfg)
    assert got == tr.recommendations(analysis, 3, 0.5, False, "adaptive")
    assert got["enable_flicker_reduction"] == (severity > 0.3)
    assert TD.generate_recommendations({}, cfg) == tr.recommendations({}, 3, 0.5, False, "adaptive")


def test_add_weighted_restatement_rounds_half_to_even_and_saturates():
    a = np.array([1, 2, 3, 255, 0, 255], np.uint8)
    b = np.array([2, 3, 4, 255, 0, 0], np.uint8)
    np.testing.assert_array_equal(tr.add_weighted(a, 0.5, b, 0.5), [2, 2, 4, 255, 0, 128])   # 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 127.5 -> 128
    np.testing.assert_array_equal(tr.add_weighted(a, 1.5, b, 1.0), [4, 6, 8, 255, 0, 255])   # 3.5 -> 4, 8.5 -> 8, saturated
    np.testing.assert_array_equal(tr.add_weighted(a, -1.0, b, 0.0), [0, 0, 0, 0, 0, 0])


def test_consistency_restatement_strength_zero_and_single_frame_return_the_centre():
    frames = list(synthetic_frames(5, 24, 32, 9))
    z = np.zeros((24, 32), np.float32)
    maps = [(z, z, np.full((24, 32), 0.5, np.float32))] * 5
    np.testing.assert_array_equal(tr.consistency_flow_guided(frames, 2, 2, 0.0, maps), frames[2])
    np.testing.assert_array_equal(tr.consistency_simple(frames[:1], 0, 2, 0.8), frames[0])
    # zero flow, constant confidence: the flow-guided average is the plain weighted average with the centre at weight 1
    got = tr.consistency_flow_guided(frames, 2, 1, 1.0, maps)
    tw = np.exp(-0.5)
    acc = frames[1].astype(np.float64) * (tw * 0.5) + frames[2].astype(np.float64) + frames[3].astype(np.float64) * (tw * 0.5)
    np.testing.assert_array_equal(got, (acc / (tw * 0.5 + 1.0 + tw * 0.5)).astype(np.uint8))


# -------------------------------------------------------------------------------------------- configuration and argument checks
def test_config_is_the_references():
    c = TD.TemporalDenoiseConfig()
    assert (c.temporal_radius, c.noise_strength, c.method, c.enable_optical_flow, c.optical_flow_method, c.enable_flicker_reduction,
            c.flicker_mode, c.preserve_edges, c.edge_threshold, c.temporal_weight_decay, c.scene_change_threshold, c.gpu_id,
            c.chunk_size) == (3, 0.5, TD.DenoiseMethod.OPTICAL_FLOW_WARP, True, TD.OpticalFlowMethod.FARNEBACK, True,
                              TD.FlickerMode.ADAPTIVE, True, 30, 0.5, 0.7, 0, 50)
    assert [m.name for m in TD.DenoiseMethod] == ["MULTI_FRAME_AVERAGE", "OPTICAL_FLOW_WARP", "NON_LOCAL_MEANS_TEMPORAL",
                                                  "BILATERAL_TEMPORAL", "VBM4D"]
    assert [m.value for m in TD.DenoiseMethod] == [1, 2, 3, 4, 5]
    assert [m.value for m in TD.FlickerMode] == ["light", "medium", "aggressive", "adaptive"]
    r = TD.TemporalDenoiseResult()
    assert (r.frames_processed, r.frames_failed, r.output_dir, r.scene_changes_detected, r.avg_noise_reduction,
            r.flicker_reduction_applied, r.processing_time_seconds, r.peak_memory_mb) == (0, 0, None, [], 0.0, False, 0.0, 0)
    assert TD.TemporalDenoiseResult().scene_changes_detected is not r.scene_changes_detected


@pytest.mark.parametrize("kwargs,word", [(dict(temporal_radius=0), "temporal_radius"), (dict(noise_strength=1.5), "noise_strength"),
                                         (dict(noise_strength=-0.1), "noise_strength"), (dict(temporal_weight_decay=2.0), "temporal_weight_decay"),
                                         (dict(scene_change_threshold=-1.0), "scene_change_threshold"), (dict(chunk_size=9), "chunk_size")])
def test_config_validation_raises_as_the_references(kwargs, word):
    with pytest.raises(ValueError, match=word):
        TD.TemporalDenoiseConfig(**kwargs)


def test_argument_validation_needs_no_gpu():
    with pytest.raises(ValueError, match="strength"):
        TD.DeviceTemporalConsistencyFilter(strength="0.5")
    with pytest.raises(ValueError, match="strength"):
        TD.DeviceTemporalConsistencyFilter(strength=float("nan"))
    with pytest.raises(ValueError, match="temporal_radius"):
        TD.DeviceTemporalConsistencyFilter(temporal_radius=-1)
    with pytest.raises(ValueError, match="sample_rate"):
        TD.scene_changes_from_hists([np.ones(256)] * 3, 0, 0.7)
    with pytest.raises(ValueError, match="uint8 BGR"):
        TD._check_clip([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError, match="one size"):
        TD._check_clip([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(ValueError, match="noise_strength"):
        TD.create_temporal_denoiser(strength=2.0)


def test_new_entries_reject_bad_arguments_without_launching(hip_lib):
    """The C entries check their arguments before anything touches a device."""
    import ctypes as C
    from framewright_amd import _lib
    one = C.c_void_p(8)
    assert hip_lib.fw_frame_stats_u8(None, 1, 4, 4, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_frame_stats_u8(one, 0, 4, 4, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_frame_stats_u8(one, 1, 0, 4, one, one, None) == _lib.FW_ERR_INVALID
    assert b"fw_frame_stats_u8" in hip_lib.fw_last_error()
    assert hip_lib.fw_flow_accumulate_affine_u8(one, one, None, None, 1.0, 0.0, 0, 4, 4, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_flow_accumulate_affine_u8(one, None, None, None, 1.0, 0.0, 0, 4, 0, one, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_add_weighted_u8(one, float("nan"), one, 0.5, 16, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_add_weighted_u8(None, 0.5, one, 0.5, 16, one, None) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_add_weighted_u8(one, 0.5, one, 0.5, 0, one, None) == _lib.FW_OK          # nothing to do
