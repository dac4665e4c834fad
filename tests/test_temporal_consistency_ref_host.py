"""Host: tests/temporal_consistency_ref.py, the contract of csrc/temporal_consistency.hip and `framewright_amd.temporal_consistency`,
against what tools/gen_temporal_consistency_golden.py recorded from the reference's own code (tests/golden/
temporal_consistency_reference.json / .npz), and the parts of the driver that need no GPU."""
import hashlib
import json
import re

import numpy as np
import pytest

import temporal_consistency_ref as R
from framewright_amd import _lib
from framewright_amd import temporal_consistency as TC


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden(golden_dir):
    js = json.loads((golden_dir / "temporal_consistency_reference.json").read_text())
    npz = np.load(golden_dir / "temporal_consistency_reference.npz")
    return js, npz


@pytest.fixture(scope="module")
def clips(golden):
    js, npz = golden
    out = {}
    for k, (name, (n, cuts, digests)) in enumerate(js["clips"].items()):
        out[name] = R.flicker_clip(n, js["height"], js["width"], 11 + k, tuple(cuts))
        assert [sha(f) for f in out[name]] == digests, name           # the inputs are the recorded ones
    for name in ("plain9", "twocuts9"):
        assert np.array_equal(np.stack(out[name]), npz[f"input|{name}"])
    return out


def test_frame_methods_equal_the_recorded_outputs(golden, clips):
    js, npz = golden
    assert len(js["cases"]) == 16
    for key, case in js["cases"].items():
        for name, digests in case["sha256"].items():
            frames = clips[name]
            got = [R.apply_frame(frames, i, case["method"], case["flicker_threshold"], case["blend_strength"]) for i in range(len(frames))]
            assert [sha(g) for g in got] == digests, (key, name)
            if len(frames) < 3:
                assert all(g is f for g, f in zip(got, frames))
        if f"output|frames|{key}" in npz:
            want = npz[f"output|frames|{key}"]
            got = [R.apply_frame(clips["plain9"], i, case["method"], case["flicker_threshold"], case["blend_strength"]) for i in range(9)]
            assert np.array_equal(np.stack(got), want)
            assert np.mean(np.any(want != np.stack(clips["plain9"]), axis=3)) > 0.02      # the stage had something to do
    assert "output|frames|optical_flow|s0.8|t0.02" in npz


def test_k_over_256_is_the_float32_blur_bit_for_bit(golden, clips):
    js, npz = golden
    plain = clips["plain9"]
    for threshold in (0.02, 0.1):
        for i, row in enumerate(js["masks"][f"t{threshold:g}"]):
            p, n = R.neighbours(9, i)
            blurred = R.detect_flicker(plain[p], plain[i], plain[n], threshold)
            k = R.blur_k(R.binary_mask(plain[p], plain[i], plain[n], threshold))
            assert blurred.dtype == np.float32 and k.min() >= 0 and k.max() <= 256
            assert np.array_equal(blurred.view(np.uint32), R.mask_from_k(k).view(np.uint32))
            assert sha(blurred) == row["sha256"] and R.area_numerator(k) == row["area_sum"]
            assert float(np.mean(blurred)) == row["area_f32"] == float(R.area_value(row["area_sum"], k.size))
            assert R.area_decision(row["area_sum"], k.size) == row["above"] == R.reference_area_decision(blurred)
            if threshold == 0.02:
                assert np.array_equal(k, npz["output|mask_k|t0.02"][i])
    # any 0 / 1 plane, odd sizes, a plane of ones (k = 256 everywhere) and the smallest frame
    rng = np.random.default_rng(3)
    for shape in ((3, 3), (5, 7), (33, 130), (45, 67)):
        for plane in (rng.random(shape) < 0.4, np.ones(shape, bool), np.zeros(shape, bool)):
            k = R.blur_k(plane.astype(np.uint8))
            blurred = R.fr.gaussian_blur(plane.astype(np.float32), 5, 0, np.float32)
            assert np.array_equal(blurred.view(np.uint32), R.mask_from_k(k).view(np.uint32))
            # summation order does not matter: columns first gives the same bits
            assert np.array_equal(R.fr.gaussian_blur(plane.astype(np.float32).T.copy(), 5, 0, np.float32).T, blurred)
    assert R.blur_k(np.ones((4, 6), np.uint8)).min() == 256


def test_area_decision_and_its_guard():
    """Up to 2^16 pixels `area_decision` is the reference's expression; beyond, every case keeps the derived distance from 0.01."""
    rng = np.random.default_rng(5)
    for shape, p in (((24, 40), 0.004), ((24, 40), 0.02), ((256, 256), 0.0101), ((256, 256), 0.0099), ((200, 300), 0.01)):
        plane = rng.random(shape) < p
        k = R.blur_k(plane.astype(np.uint8))
        mask = R.mask_from_k(k)
        assert k.size <= 1 << 16 and R.area_guard(k.size) == 0.0
        assert np.mean(mask) == R.area_value(R.area_numerator(k), k.size)
        assert R.area_decision(R.area_numerator(k), k.size) == R.reference_area_decision(mask)
    for shape, p in (((300, 300), 0.004), ((300, 300), 0.03), ((1080, 1920), 0.0098), ((1080, 1920), 0.0102)):
        plane = rng.random(shape) < p
        k = R.blur_k(plane.astype(np.uint8))
        s, n = R.area_numerator(k), k.size
        guard = R.area_guard(n)
        assert 0 < guard < 3e-6 and R.area_distance(s, n) > guard                   # the case is outside the distance ...
        assert abs(float(np.mean(R.mask_from_k(k))) / (s / 256.0 / n) - 1.0) <= guard   # ... the reference's float32 sum inside it
        assert R.area_decision(s, n) == R.reference_area_decision(R.mask_from_k(k)) == (s / 256.0 / n > float(np.float32(0.01)))
    assert R.pairwise_depth(128) == 18 and R.pairwise_depth(7680 * 4320) == 36
    assert float(TC.area_value(12345, 960)) == float(R.area_value(12345, 960))


def test_scene_test_equals_the_recorded_correlations(golden, clips):
    js, _ = golden
    for name, row in js["scenes"].items():
        if name == "flat":
            flat = np.full((24, 40, 3), 77, np.uint8)
            assert R.scene_correlation(flat, flat) == 1.0 and R.scene_changes([flat, flat, flat]) == []    # den2 = 0: 1
            assert TC.hist_correlation(R.gray_hist(flat), R.gray_hist(flat)) == 1.0
            continue
        frames = clips[name]
        hist = [R.gray_hist(f) for f in frames]
        assert all(h.sum() == 24 * 40 for h in hist)
        assert [R.scene_correlation(frames[i - 1], frames[i]) for i in range(1, 9)] == row["correlation"]
        assert [TC.hist_correlation(hist[i - 1], hist[i]) for i in range(1, 9)] == row["correlation"]        # the driver's host arithmetic
        assert R.scene_changes(frames) == row["cuts"] == list(js["clips"][name][1])
    assert js["scenes"]["twocuts9"]["cuts"] == [3, 5]


def test_clip_driver_equals_the_recorded_driver(golden, clips):
    js, npz = golden
    assert len(js["driver"]) == 25
    for key, row in js["driver"].items():
        parts = key.split("|")
        frames = clips[parts[0]]
        if len(parts) == 4:                                              # frame 3 unreadable: it and both its neighbours fail
            assert row["frames_failed"] == 3 and row["frames_processed"] == 6 and row["skipped"] == 1 and row["failed"] == 2
            assert row["written"] == [f"frame_{i:08d}.png" for i in (0, 1, 5, 6, 7, 8)]
            assert row["copied"] == [f"frame_{i:08d}.png" for i in (2, 4)] and len(row["progress"]) == 8     # the fallback copies
            continue
        want, cuts = R.apply_clip(frames, row["method"], row["attention_window"])
        assert cuts == row["scene_changes_detected"] and [sha(w) for w in want] == row["sha256"], key
        assert row["frames_processed"] == len(frames) and row["frames_failed"] == 0 and row["flicker_regions_fixed"] == 0
        assert row["written"] == "all" and row["progress"] == [(i + 1) / len(frames) for i in range(len(frames))]
        half = row["attention_window"] // 2
        for i, (w, f) in enumerate(zip(want, frames)):
            assert (w is f) == (any(abs(i - c) <= half for c in cuts) or len(frames) < 3), (key, i)
        if f"output|driver|{key}" in npz:
            assert np.array_equal(np.stack(want), npz[f"output|driver|{key}"])
    two = js["driver"]["twocuts9|hybrid|w7"]                             # two cuts closer than the window: one joined span
    assert two["sha256"] == [sha(f) for f in clips["twocuts9"]]
    assert js["driver"]["twocuts9|hybrid|w1"]["sha256"][4] != sha(clips["twocuts9"][4])


def test_stream_hold_back_is_stated_and_equals_the_clip_driver(golden, clips):
    js, _ = golden
    assert js["hold_back"] == {"1": 1, "3": 2, "7": 4} == {str(w): R.stream_hold_back(w) for w in (1, 3, 7)}
    for name in ("plain9", "cut9", "twocuts9", "three", "two", "one"):
        for method in (R.OPTICAL_FLOW, R.HYBRID):
            for window in (1, 3, 7):
                want = R.apply_clip(clips[name], method, window)[0]
                got = R.stream_clip(clips[name], method, window)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (name, method, window)
    called_clip, called_stream = [], []
    hook = lambda frames, i: 255 - frames[i]                             # noqa: E731
    want = R.apply_clip(clips["cut9"], R.HYBRID, 3, attention_fn=hook, called=called_clip)[0]
    got = R.stream_clip(clips["cut9"], R.HYBRID, 3, attention_fn=hook, called=called_stream)
    assert called_clip == called_stream and called_clip and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_config_validation_matches_the_recorded_behaviour(golden):
    js, _ = golden
    cfg = TC.CrossAttentionConfig()
    plain = lambda v: v.value if isinstance(v, TC.TemporalMethod) else v           # noqa: E731
    assert {k: plain(v) for k, v in cfg.__dict__.items()} == js["defaults"]
    for bad, message in js["rejected"]:
        with pytest.raises(ValueError, match=re.escape(message)):
            TC.CrossAttentionConfig(**bad)
    for good in js["accepted"]:
        TC.CrossAttentionConfig(**good)
    assert TC.CrossAttentionConfig(method="optical_flow").method is TC.TemporalMethod.OPTICAL_FLOW
    assert {"TemporalMethod": {m.name: m.value for m in TC.TemporalMethod}} == js["enums"]
    result = TC.TemporalConsistencyResult()
    assert result.flicker_areas == [] and {k: v for k, v in result.__dict__.items() if k != "flicker_areas"} == js["result_defaults"]
    # the restorer's own driver cannot run: what it passes and calls does not exist in the reference, and does not here
    assert js["restorer"]["process_frame"] is False and not hasattr(TC.DeviceTemporalConsistencyProcessor, "process_frame")
    assert "window_size" in js["restorer"]["window_size"] and "processed_frames" in js["restorer"]["processed_frames"]
    assert "method_used" in js["restorer"]["method_used"] and js["restorer"]["default_blend_strength"] == 0.5
    with pytest.raises(TypeError):
        TC.CrossAttentionConfig(window_size=7)


def test_cross_attention_without_a_hook_is_refused_and_the_factory_builds_the_config(golden):
    js, _ = golden
    with pytest.raises(ValueError, match="the cross-attention network is not built"):
        TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="cross_attention"))
    with pytest.raises(ValueError, match="the cross-attention network is not built"):
        TC.create_temporal_processor("cross_attention")
    made = TC.create_temporal_processor("optical_flow", 5, 0.25, 1)               # needs no GPU until a frame arrives
    plain = lambda v: v.value if isinstance(v, TC.TemporalMethod) else v           # noqa: E731
    assert {k: plain(v) for k, v in made.config.__dict__.items()} == js["created"]
    assert made.is_available() and made._backend == "optical_flow"
    hooked = TC.create_temporal_processor("hybrid", attention_fn=lambda frames, i: frames[i])
    assert hooked._backend == "cross_attention"
    made.close()
    assert not made.is_available()


def test_header_declares_the_entries_and_the_build_keeps_contraction_off():
    import framewright_amd
    from framewright_amd import build as fw_build
    for name in ("fw_tcons_gray_hist_u8", "fw_tcons_apply_u8"):
        assert name in _lib.EXPORTS
    table = {name: (restype, argtypes) for name, restype, argtypes in _lib._SIGNATURES}
    import ctypes as C
    assert table["fw_tcons_apply_u8"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 4)
    assert table["fw_tcons_gray_hist_u8"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    assert fw_build.PER_FILE_FLAGS["temporal_consistency.hip"] == ["-ffp-contract=off"]
    assert framewright_amd.DeviceTemporalConsistencyProcessor is TC.DeviceTemporalConsistencyProcessor


def test_entries_refuse_bad_arguments_without_a_gpu(hip_lib):
    import ctypes as C
    buf = np.zeros(4096, np.uint8)
    a, b, c, d = (C.c_void_p(buf.ctypes.data + 1024 * i) for i in range(4))
    call = hip_lib.fw_tcons_apply_u8
    assert call(None, b, c, 8, 8, 0.02, 0.8, d, None, None, None) == _lib.FW_ERR_INVALID
    assert call(a, b, c, 8, 8, 0.02, 0.8, None, None, None, None) == _lib.FW_ERR_INVALID and b"nothing to write" in hip_lib.fw_last_error()
    assert call(a, b, c, 2, 8, 0.02, 0.8, d, None, None, None) == _lib.FW_ERR_INVALID and b"3 .. 16384" in hip_lib.fw_last_error()
    assert call(a, b, c, 8, 16385, 0.02, 0.8, d, None, None, None) == _lib.FW_ERR_INVALID
    assert call(a, b, c, 8, 8, float("nan"), 0.8, d, None, None, None) == _lib.FW_ERR_INVALID
    assert call(a, b, c, 8, 8, 0.02, 1.5, d, None, None, None) == _lib.FW_ERR_INVALID and b"[0, 1]" in hip_lib.fw_last_error()
    assert call(a, b, c, 8, 8, 0.02, 0.8, None, C.c_void_p(buf.ctypes.data + 3074), None, None) == _lib.FW_ERR_INVALID
    assert call(a, b, c, 8, 8, 0.02, 0.8, None, None, C.c_void_p(buf.ctypes.data + 3076), None) == _lib.FW_ERR_INVALID
    assert call(a, b, c, 8, 8, 0.02, 0.8, C.c_void_p(buf.ctypes.data + 2048 + 100), None, None, None) == _lib.FW_ERR_INVALID
    assert b"overlaps" in hip_lib.fw_last_error()
    hist = hip_lib.fw_tcons_gray_hist_u8
    assert hist(None, 8, 8, d, None) == _lib.FW_ERR_INVALID and hist(a, 0, 8, d, None) == _lib.FW_ERR_INVALID
    assert hist(a, 8, 8, C.c_void_p(buf.ctypes.data + 3073), None) == _lib.FW_ERR_INVALID
