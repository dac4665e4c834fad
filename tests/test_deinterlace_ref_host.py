"""CPU: tests/deinterlace_ref.py (the contract of csrc/deinterlace.hip and framewright_amd/deinterlace.py) against what
tools/gen_deinterlace_golden.py recorded from the reference's own `processors/format/interlace.py`."""
import json
from pathlib import Path

import numpy as np
import pytest

import deinterlace_ref as R

GOLD = Path(__file__).resolve().parent / "golden"
REL = 2.0 ** -23        # two float32 roundings: the reference's float32 means of exact partial sums (frames under 65 793 pixels)
MARGIN = 1e-4


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "deinterlace_reference.json").read_text())


@pytest.fixture(scope="module")
def arrays():
    return np.load(GOLD / "deinterlace_reference.npz")


@pytest.fixture(scope="module")
def frame_clips():
    return R.frame_clips()


@pytest.fixture(scope="module")
def analysis_clips():
    return R.analysis_clips()


@pytest.mark.parametrize("method", ["yadif", "bwdif", "bob", "weave"])
def test_frames_equal_the_reference_byte_for_byte(gold, arrays, frame_clips, method):
    for name, clip in frame_clips.items():
        for order in ("tff", "bff"):
            got = R.deinterlace(clip, method, order)
            assert [R.sha256(a) for a in got] == gold["frames"][f"{name}/{order}/{method}"], (name, order)
            key = f"{name}/{order}/{method}"
            if key in arrays.files:
                np.testing.assert_array_equal(np.stack(got), arrays[key])
    assert R.deinterlace(frame_clips["5x3x1"], "bob", "tff")[0].shape == (5, 3) and len(R.deinterlace(frame_clips["5x3x1"], "bob", "tff")) == 8


def test_neural_nnedi_and_unknown_methods_fall_back(frame_clips):
    clip = frame_clips["9x16x3"]
    for m in ("neural", "nnedi"):
        assert all(np.array_equal(a, b) for a, b in zip(R.deinterlace(clip, m, "tff"), R.bwdif(clip, 1)))
    assert all(np.array_equal(a, b) for a, b in zip(R.deinterlace(clip, "something", "bff"), R.yadif(clip, 0)))


def test_wrong_variants_are_rejected(gold, frame_clips):
    """BWDIF with temporal weight (prev + next) / 4 and YADIF that rounds instead of truncating both change recorded frames."""
    for method, kw in (("bwdif", {"temporal_quarter": True}), ("yadif", {"rounding": True})):
        wrong = 0
        for name, clip in frame_clips.items():
            for order, parity in (("tff", 1), ("bff", 0)):
                got = {"yadif": R.yadif, "bwdif": R.bwdif}[method](clip, parity, **kw)
                wrong += [R.sha256(a) for a in got] != gold["frames"][f"{name}/{order}/{method}"]
        assert wrong >= 8, (method, wrong)


def test_small_heights_copy_what_the_ranges_leave_out():
    rng = np.random.default_rng(0)
    for h in (1, 2, 3, 4, 5):
        f = rng.integers(0, 256, size=(h, 4), dtype=np.uint8)
        for parity in (0, 1):
            y = R.yadif_frame(f, parity)
            b = R.bwdif_frame(f, f, f, parity)
            for row in range(h):
                if not (1 <= row <= h - 2 and row % 2 == parity):
                    np.testing.assert_array_equal(y[row], f[row])
                if not (2 <= row <= h - 3 and row % 2 == parity):
                    np.testing.assert_array_equal(b[row], f[row])
    with pytest.raises(ValueError):
        R.bob_field(np.zeros((1, 4), np.uint8), 0)
    with pytest.raises(ValueError):
        R.analyze([np.zeros((3, 4), np.uint8)])


def test_analysis_equals_the_reference(gold, analysis_clips):
    seen = set()
    for name, clip in analysis_clips.items():
        rec = gold["analysis"][name]
        a = R.analyze(clip)
        for k in ("is_interlaced", "field_order", "telecine_pattern", "recommended_method", "progressive_percentage", "tff_percentage",
                  "bff_percentage", "combing_percentage", "confidence"):
            assert getattr(a, k) == rec["analyze"][k], (name, k)
        if rec["analyze"]["diff_variance"] is None:
            assert "telecine" not in a.details
        else:
            # the reference's variance is NumPy's float32 variance of its float32 frame differences (every frame is sampled here, so
            # these are all consecutive pairs): formed the same way from the recorded differences it is the recorded value exactly.
            # The contract's own value is the float64 variance of the exact means: four float32 roundings away at the most (the
            # mean, a deviation, its square, the final mean of squares) - 4 * 2^-23 relative, twice the issue's bound per statistic
            diffs32 = [np.float32(f["frame_difference"]) for f in rec["frames"] if "frame_difference" in f]
            assert float(np.var(diffs32)) == rec["analyze"]["diff_variance"]
            got_var = a.details["telecine"]["diff_variance"]
            assert abs(got_var - rec["analyze"]["diff_variance"]) <= 4 * REL * rec["analyze"]["diff_variance"], (name, got_var)
        assert R.detect_telecine(clip) == rec["detect_telecine"]
        assert R.inverse_telecine_indices(clip) == rec["inverse_telecine"]
        assert R.inverse_telecine_indices(clip, "3:2") == rec["inverse_telecine_3_2"]
        order = R.resolve_order(clip, "auto")
        assert order == (rec["auto_order"] if rec["auto_order"] != "unknown" else "tff")
        assert [R.sha256(x) for x in R.deinterlace(clip, "bwdif", order)] == rec["auto_bwdif_sha256"]
        h, w = clip[0].shape[:2]
        assert h * w < 65793
        for i, (f, fr) in enumerate(zip(clip, rec["frames"])):
            st = R.stats(f)
            assert list(st) == fr["stats"] and R.order_hint(st, h, w) == fr["hint"] and R.comb_ratio(st, h) == fr["comb_ratio"]
            r = h // 2
            for mine, key in ((st[1] / (r * w), "diff"), (st[2] / ((r - 1) * w), "odd_gradient"), (st[3] / ((r - 1) * w), "even_gradient")):
                assert abs(mine - fr[key]) <= REL * abs(fr[key]), (name, i, key)
            if "frame_difference" in fr:
                assert abs(R.frame_difference(f, clip[i + 1]) - fr["frame_difference"]) <= REL * fr["frame_difference"]
        seen.add((rec["analyze"]["field_order"], rec["analyze"]["telecine_pattern"], rec["analyze"]["is_interlaced"], len(clip) < 10))
    # every branch: TFF, BFF, progressive, 3:2, 2:2, fewer than ten frames
    assert {s[0] for s in seen} >= {"tff", "bff", "unknown"} and {s[1] for s in seen} >= {"3:2", "2:2", "none"}
    assert {s[2] for s in seen} == {True, False} and {s[3] for s in seen} == {True, False}


def test_fixture_statistics_keep_their_distance_from_every_threshold(gold):
    """No fixture statistic lies within 1e-4 relative of a threshold it is compared with, so the float32 means of the reference and
    the exact ones here decide alike.  Of the recorded values `frame_difference`, `hint` and `comb_ratio` are the reference's own
    return values; `diff`, `odd_gradient`, `even_gradient` and `row_means` are locals of the reference's functions that it does
    not return, recorded from `deinterlace_ref.stats_float32`, which forms them with the reference's types and operation order -
    the generator asserts that the hint and the ratio they lead to are the reference's on every frame."""
    def far(v, t):
        return abs(v - t) >= MARGIN * abs(t)

    for name, rec in gold["analysis"].items():
        diffs = [f["frame_difference"] for f in rec["frames"] if "frame_difference" in f]
        for f in rec["frames"]:
            assert far(f["diff"], 5.0), name
            assert all(far(m, 30.0) for m in f["row_means"]), name
            if f["diff"] >= 5:
                assert far(f["odd_gradient"], f["even_gradient"] * 1.1) and far(f["even_gradient"], f["odd_gradient"] * 1.1), name
        # the duplicate thresholds of analyze (all sampled pairs), detect_telecine (the first 60) and inverse_telecine (all)
        for subset in (diffs, diffs[:60]):
            if subset:
                t = float(np.mean(subset)) * 0.3
                assert all(far(d, t) for d in subset), name
