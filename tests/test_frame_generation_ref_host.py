"""CPU: tests/frame_generation_ref.py, the contract of csrc/frame_generation.hip, against what the reference's own
`MissingFrameGenerator` methods answered when tools/gen_frame_generation_golden.py ran them (tests/golden/frame_generation_reference.*),
byte for byte; the reflect border; the gap rule; the value types of framewright_amd.frame_generation; and the standard-deviation rule:
the inputs of tests/test_frame_generation_gpu.py keep every deviation clear of a float32 rounding boundary, so no GPU case may use
the exception, and the reference's float32 np.std stays within a derived number of ulps of the contract's value."""
import hashlib
import json
import logging

import numpy as np
import pytest

import frame_generation_ref as R
import frame_generation_cases as K
from framewright_amd import frame_generation as FG


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "frame_generation_reference.json").read_text()), np.load(golden_dir / "frame_generation_reference.npz")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_restatement_equals_the_reference_on_every_case(golden):
    js, npz = golden
    assert len(js["cases"]) == 28
    models = {c["model"] for c in js["cases"].values()}
    assert models == {"interpolate_blend", "optical_flow_warp"} and {c["gap_size"] for c in js["cases"].values()} >= {1, 2, 4, 10}
    assert {c["blend_edges"] for c in js["cases"].values()} == {0, 1, 3} and any(not c["has_after"] for c in js["cases"].values())
    for key, c in js["cases"].items():
        before, after = npz["input|" + c["before"]], (npz["input|after"] if c["has_after"] else None)
        got = R.fill_gap(before, after, c["start_frame"], c["gap_size"], c["backend"], c["match_grain"], c["blend_edges"], c["seed"])
        assert [sha(g) for g in got] == c["sha256"], key
        if "output|" + key in npz:
            np.testing.assert_array_equal(np.stack(got), npz["output|" + key])
    c = js["cases"]["interpolate_blend|gap2|blend3|grain1|ref_le_cur"]
    assert c["grain_added"] == [False, False] and all(js["cases"]["optical_flow_warp|gap4|blend3|grain1"]["grain_added"])


def test_a_gap_shorter_than_blend_edges_blends_one_frame_twice():
    assert R.edge_blends(0, 1, 3, True) == (0.5, 0.5) and R.edge_blends(0, 1, 3, False) == (0.5, None)
    assert [R.edge_blends(i, 4, 3, True) for i in range(4)] == [(0.25, None), (0.5, 0.75), (0.75, 0.5), (None, 0.25)]
    assert R.edge_blends(2, 10, 0, True) == (None, None) and R.edge_blends(5, 10, 3, True) == (None, None)
    assert all(FG.edge_blends(i, n, b, a) == R.edge_blends(i, n, b, a) for n in (1, 2, 4, 10) for i in range(n) for b in (0, 1, 3) for a in (True, False))


def test_driver_paths_of_the_reference_are_recorded(golden):
    js, npz = golden
    d = js["driver"]
    assert d["after_only"]["frames_generated"] == 2 and d["after_only"]["written"] == ["frame_00000005.png", "frame_00000006.png"]
    for name in ("both", "before_only"):                       # `before or after` on an array: every gap with a before frame fails
        assert d[name]["frames_failed"] == 2 and d[name]["gaps_processed"] == 0 and "truth value of an array" in d[name]["errors"][0]
    want = R.fill_gap(None, npz["input|after"], 4, 2, R.INTERPOLATE, True, 3, 5)
    np.testing.assert_array_equal(np.stack(want), npz["output|driver_after_only"])
    assert js["restorer_calls"]["fill_gap"] is False and "gaps_detected" in js["restorer_calls"]["gaps_detected"]


def test_reflect_border_far_outside_the_frame(golden):
    _, npz = golden
    assert list(R.reflect(np.arange(-7, 8), 3)) == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]       # ...cba|abc|cba...
    assert list(R.reflect(np.array([-1, 0, 5, 6, 11, 12, -13]), 6)) == [0, 0, 5, 5, 0, 0, 0] and list(R.reflect(np.array([-3, 9]), 1)) == [0, 0]
    before, after = npz["input|before"], npz["input|after"]
    h, w = before.shape[:2]
    fx, fy = np.full((h, w), -6.0 * w + 0.3, np.float32), np.full((h, w), 4.0 * h - 0.7, np.float32)
    np.testing.assert_array_equal(R.warp_blend(before, after, (fx, fy), (fx, fy), 0.5), npz["output|far_flow"])
    # an integer displacement of whole periods is the identity; of one width, the mirror image
    zero = np.zeros((h, w), np.float32)
    np.testing.assert_array_equal(R.remap_linear_reflect(before, np.arange(w, dtype=np.float32)[None, :] + zero + 4 * w, np.arange(h, dtype=np.float32)[:, None] + zero), before)
    np.testing.assert_array_equal(R.remap_linear_reflect(before, np.arange(w, dtype=np.float32)[None, :] + zero + w, np.arange(h, dtype=np.float32)[:, None] + zero),
                                  before[:, ::-1])
    from oracle import temporal_ref as oref
    assert oref._reflect101 is not R.reflect                   # the oracle's own border function is back in its place


def test_detect_gaps_patterns_rule_and_end_gap(golden, tmp_path):
    js, _ = golden
    assert len(js["detect_gaps"]) == 18
    for key, c in js["detect_gaps"].items():
        d = tmp_path / key.replace("|", "_")
        d.mkdir()
        for n in c["names"]:
            (d / n).write_bytes(b"")
        assert [list(g) for g in R.detect_gaps(c["names"], c["expected_count"], c["max_gap_frames"])] == c["gaps"], key
        gen = FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(max_gap_frames=c["max_gap_frames"]))
        found = gen.detect_gaps(d, c["expected_count"])
        assert [[g.start_frame, g.end_frame, g.gap_size, g.after_path is not None] for g in found] == c["gaps"], key
        assert all(g.before_path is not None and g.before_path.parent == d for g in found)
    assert js["detect_gaps"]["plain|max10"]["gaps"] == [[1, 4, 2, True]] and js["detect_gaps"]["plain|max2"]["gaps"] == [[1, 4, 2, True]]
    assert js["detect_gaps"]["expected|max10"]["gaps"] == [[0, 2, 1, True], [2, 5, 3, False]] and js["detect_gaps"]["expected|max2"]["gaps"] == [[0, 2, 1, True]]
    gen = FG.DeviceMissingFrameGenerator()
    got = gen.gaps_from_numbers([7, 0, 1, 4], expected_count=10)
    assert [(g.start_frame, g.end_frame, g.gap_size, g.before_path, g.after_path) for g in got] == [(1, 4, 2, None, None), (4, 7, 2, None, None), (7, 9, 2, None, None)]
    assert [(g.start_frame, g.end_frame, g.gap_size) for g in got] == [g[:3] for g in R.gaps_from_numbers([7, 0, 1, 4], 10)]
    assert [FG.parse_frame_number(n) for n in ("Frame-0003.png", "0005.png", "shot_0009.png", "frame12.png", "notes.png")] == [3, 5, 9, 12, None]


def test_value_types_are_the_references(golden, caplog):
    js, _ = golden
    show = lambda cfg: {k: (v.value if isinstance(v, FG.GenerationModel) else v) for k, v in cfg.__dict__.items()}    # noqa: E731
    assert show(FG.FrameGenerationConfig()) == js["defaults"]
    assert {m.name: m.value for m in FG.GenerationModel} == js["enums"]["GenerationModel"]
    for bad, message in js["rejected"]:
        if bad == {"model": "optical_flow"}:                   # what the restorer passes: an alias here, an error in the reference
            assert FG.FrameGenerationConfig(**bad).model is FG.GenerationModel.OPTICAL_FLOW_WARP
            continue
        with pytest.raises(ValueError) as e:
            FG.FrameGenerationConfig(**bad)
        assert str(e.value) == message
    with caplog.at_level(logging.WARNING, logger="framewright_amd.frame_generation"):
        backends = {m.value: FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(model=m))._backend for m in FG.GenerationModel}
    assert backends == js["backends"] and "SVD not available, falling back to interpolation" in caplog.text
    made = FG.create_frame_generator("optical_flow_warp", 4, False, 1)
    assert show(made.config) == js["created"] and made.is_available()
    res = {k: v for k, v in FG.FrameGenerationResult().__dict__.items()}
    assert {k: (None if v is None else v) for k, v in res.items()} == {k: (None if v == "None" else v) for k, v in js["result_defaults"].items()}
    assert {k: v for k, v in FG.GapInfo(1, 3, 1).__dict__.items()} == {k: (None if v == "None" else v) for k, v in js["gap_defaults"].items()}
    np.testing.assert_array_equal(FG.gaussian17_coeffs(), np.array(js["gaussian17"], np.float32))
    np.testing.assert_array_equal(FG.gaussian17_coeffs(), R.gaussian17_coeffs())
    import framewright_amd
    assert framewright_amd.DeviceMissingFrameGenerator is FG.DeviceMissingFrameGenerator and framewright_amd.create_frame_generator is FG.create_frame_generator


def test_noise_keys_are_the_counter_generators():
    from qp_artifact_ref import frame_key
    assert FG.noise_key(5, 11, FG.TAG_GRAIN) == frame_key(5, R.noise_index(11, R.TAG_GRAIN))
    assert FG.noise_key(5, 11, FG.TAG_EXTRAPOLATE) == frame_key(5, R.noise_index(11, R.TAG_EXTRAPOLATE)) != FG.noise_key(5, 11, FG.TAG_GRAIN)
    assert FG.DeviceMissingFrameGenerator()._seed(None) == 0 and FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(seed=9))._seed(None) == 9


# ---- the standard-deviation rule -------------------------------------------------------------------------------------------------
def test_every_gpu_input_is_clear_of_a_rounding_boundary():
    """The device reduces in another order than numpy; both are float64 sums of exact terms.  Every frame whose deviation a GPU test
    compares lies further than `std_epsilon` from a float32 rounding boundary, and every grain decision further than that from
    ref = cur: checked here, so that the GPU tests assert byte equality with no exception."""
    frames = K.statistic_frames()
    assert len(frames) >= 12
    for name, frame in frames.items():
        eps = R.std_epsilon(R.grain_plane(frame))
        assert eps < 1e-10, (name, eps)
        assert R.clear_of_rounding_boundary(R.grain_std64(frame), eps), name
    for name, (ref, cur) in K.grain_decisions().items():
        eps = max(R.std_epsilon(R.grain_plane(ref)), R.std_epsilon(R.grain_plane(cur)))
        a, b = R.grain_std64(ref), R.grain_std64(cur)
        assert abs(a - b) > eps * (a + b), name


def test_the_references_float32_std_is_within_the_derived_ulps(golden):
    js, npz = golden
    for name, s in js["stds"].items():
        frame = npz["input|" + name]
        assert R.grain_std64(frame) == s["contract_f64"] and float(R.grain_std(frame)) == s["contract_f32"]
        assert float(R.grain_std_reference(frame)) == s["reference_f32"]
        apart, bound = R.ulps_apart(s["reference_f32"], s["contract_f32"]), R.std_f32_ulp_bound(frame.shape[0] * frame.shape[1])
        print(f"{name}: the reference's float32 np.std is {apart} ulps from the contract, bound {bound}")
        assert apart <= bound, (name, apart, bound)
    assert R.std_f32_ulp_bound(24 * 40) == 13 and R.std_f32_ulp_bound(1080 * 1920) == 19      # k = 16 + 3 and 16 + 14 levels
