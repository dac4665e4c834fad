"""CPU: tests/aspect_ref.py against what tools/gen_aspect_golden.py recorded from the reference's own `processors/format/aspect.py`
(tests/golden/aspect_reference.json and .npz): every digest, every analysis field, which outputs are the input object.  The generator
asserted the equality with the reference when it ran; this holds the restatement to that record.  Exact equality throughout."""
import json
from pathlib import Path

import numpy as np
import pytest

import aspect_ref as R

GOLD = Path(__file__).resolve().parent / "golden"
CLIPS = R.clips()
FRAMES = R.convert_frames()


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "aspect_reference.json").read_text())


def bars(handler, clip):
    return [[a.top_bar, a.bottom_bar, a.left_bar, a.right_bar] for a in map(handler.analyze_frame, clip)]


def test_the_recorded_cases_are_the_fixtures_cases(gold):
    assert sorted(gold["analysis"]) == sorted(CLIPS) and len(CLIPS) == 61
    assert sorted(gold["crops"]) == sorted(f"{n}|{a}" for n in CLIPS for a in R.CROP_ALIGNS)
    keys = [c[0] for name, frames in FRAMES.items() for c in R.convert_cases(name, frames)]
    assert sorted(gold["convert"]) == sorted(keys) and len(keys) == 192
    assert gold["gauss99"] == R.gauss99_table().tolist() and sum(gold["gauss99"]) == 256 and gold["gauss99"] == gold["gauss99"][::-1]


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_analysis_equals_the_recorded_fields(gold, name):
    clip, rec, h = CLIPS[name], gold["analysis"][name], R.AspectHandler()
    assert R.analysis_record(h.analyze_frame(clip[0])) == rec["frame0"]
    assert R.analysis_record(h.analyze(clip)) == rec["clip"]
    assert bars(h, clip) == rec["bars"]
    assert float(h.detect_aspect(clip[0])) == rec["detect_aspect"] and bool(h.detect_letterbox(clip[0])) == rec["detect_letterbox"]
    rows, cols = R.bar_sums(clip[0])
    assert rows.dtype == cols.dtype == np.uint32 and (R.sha256(rows), R.sha256(cols)) == (rec["row_sums_sha256"], rec["column_sums_sha256"])


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_crop_equals_the_recorded_digest(gold, name):
    clip = CLIPS[name]
    for align in R.CROP_ALIGNS:
        got = R.AspectHandler(R.AspectConfig(align_to=align)).crop_letterbox(clip)
        digest, shape, same_list = gold["crops"][f"{name}|{align}"]
        assert (got is clip) == same_list and list(got[0].shape) == shape and R.digest(got) == digest


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_convert_equals_the_recorded_digest(gold, name):
    frames = FRAMES[name]
    for key, method, fill, target in R.convert_cases(name, frames):
        got = R.handler_for(method, fill).convert_aspect(frames, target)
        digest, shape, same = gold["convert"][key]
        assert "".join("01"[a is b] for a, b in zip(got, frames)) == same, key
        assert list(got[0].shape) == shape and R.digest(got) == digest, key


def test_whole_outputs_equal_the_recorded_frames():
    with np.load(GOLD / "aspect_reference.npz") as z:
        assert len(z.files) == 4
        for key in z.files:
            name, method, fill, label = key.split("|")
            case = next(c for c in R.convert_cases(name, FRAMES[name]) if c[0] == key)
            got = R.handler_for(method, fill).convert_aspect(FRAMES[name], case[3])
            assert np.array_equal(np.stack(got), z[key]), key


def test_the_clips_reach_the_cases_they_exist_for(gold):
    an, crops, conv = gold["analysis"], gold["crops"], gold["convert"]
    # a row / column whose gray sum is threshold * length is still bar, one more is content
    for name in ("threshold/37x33", "threshold/64x258/gray"):
        f = CLIPS[name][0]
        rows, cols = R.bar_sums(f)
        h, w = f.shape[:2]
        assert (int(rows[2]), int(rows[3])) == (16 * w, 16 * w + 1) and (int(cols[2]), int(cols[3])) == (16 * h, 16 * h + 1)
        assert (an[name]["frame0"]["top_bar"], an[name]["frame0"]["left_bar"]) == (3, 3)
    # a bar that ends at h // 3 - 1 is found, one that reaches h // 3 counts as 0 (the same for columns)
    for h, w in ((37, 33), (48, 64), (64, 258)):
        found, lost = an[f"edge_found/{h}x{w}"]["frame0"], an[f"edge_lost/{h}x{w}"]["frame0"]
        assert (found["top_bar"], found["left_bar"]) == (h // 3 - 1, w // 3 - 1)
        assert (lost["top_bar"], lost["bottom_bar"], lost["left_bar"], lost["right_bar"]) == (0, 0, 0, 0)
        # asymmetric bars more than 5 apart lower the confidence, once per direction
        assert abs(found["top_bar"] - found["bottom_bar"]) > 5 and found["confidence"] == 1.0 - 0.1 - 0.1
    assert an["letterbox/37x33"]["frame0"]["confidence"] == 1.0
    # an all-black frame, and the 2 x 2 frame whose thirds are empty
    assert an["black/48x64"]["bars"] == [[0, 0, 0, 0]] * 2 and not an["black/48x64"]["clip"]["has_letterbox"]
    assert all(an[n]["bars"][0] == [0, 0, 0, 0] for n in an if n.endswith("/2x2"))
    # bars that vary over the clip
    v = an["variable/37x33"]
    assert v["clip"]["is_variable"] and np.std([b[0] for b in v["bars"]]) > 5 and v["clip"]["confidence"] < 1.0
    assert not an["letterbox/37x33"]["clip"]["is_variable"]
    # an even sample count whose median ends in .5: int() takes it down
    m = an["median_half/37x33"]
    tops, bottoms = sorted(b[0] for b in m["bars"]), sorted(b[1] for b in m["bars"])
    assert len(tops) == 4 and np.median(tops) == 4.5 and np.median(bottoms) == 6.5 and (m["clip"]["top_bar"], m["clip"]["bottom_bar"]) == (4, 6)
    # a bar below min_bar_size: the frame analysis tests the sum of the two bars with >=, the clip analysis zeroes each bar
    s = an["small_bar/48x64"]
    assert s["bars"][0] == [2, 1, 3, 3] and not s["frame0"]["has_letterbox"] and s["frame0"]["has_pillarbox"]
    assert s["clip"]["crop_region"] == [0, 0, 64, 48] and not s["clip"]["has_pillarbox"] and crops["small_bar/48x64|2"][2] is True
    # a crop floored by align_to 2 and 16; one that aligns to no columns at all
    assert an["letterbox/48x64"]["clip"]["crop_region"] == [0, 8, 64, 31]
    assert crops["letterbox/48x64|2"][1] == [30, 64, 3] and crops["letterbox/48x64|16"][1] == [16, 64, 3]
    assert crops["letterbox/32x8|16"][1] == [16, 0, 3]
    # more than 20 frames; no bars: the list itself
    assert len(CLIPS["long/37x33"]) > 20 and crops["long/37x33|2"][2] is False and crops["plain/37x33|2"][2] is True
    # conversions: the frame itself at its own ratio, the unknown spelling falls back to 16:9, a mirror bar wider than the frame
    assert conv["37x33|pad|black|same"][2] == "11" and conv["37x33|pad|black|wider"][2] == "00"
    assert conv["37x33|fit|mirror|str-2.0:1"][1] == [int(33 / (16 / 9)), 33, 3] and conv["37x33|pad|black|str-4:3"][1] == [37, int(37 * (4 / 3)), 3]
    h, w = conv["37x33|pad|mirror|wider3"][1][:2]
    assert h == 37 and (w - 33) // 2 > 33
    assert conv["37x33/gray|pad|color|wider"][1] == [37, int(37 * (33 / 37 * 1.5))]
    assert conv["37x120|pad|blur|wider"][1][1] > 120 > R.GAUSS_TAPS and conv["32x8|pad|blur|wider"][1][1] < 49


def test_value_types():
    S = R.StandardAspectRatio
    assert S.from_string("16:9") is S.RATIO_16_9 and S.from_string(" 4:3 ") is S.RATIO_4_3 and S.from_string("2.0:1") is None
    assert S.from_string("2.36/1") is S.RATIO_2_35_1 and S.from_decimal(2.34) is S.RATIO_2_35_1 and S.from_string("x") is None
    assert R.parse_target("2.0:1") == 16 / 9 and R.parse_target(S.RATIO_1_1) == 1.0 and R.parse_target(2) == 2.0
    with pytest.raises(ValueError):
        R.AspectConfig(black_threshold=256)
    with pytest.raises(ValueError):
        R.AspectConfig(min_bar_size=-1)
    a = R.AspectHandler().analyze(CLIPS["letterbox/48x64"])
    assert a.crop_region.as_tuple() == (0, 8, 64, 31) and a.crop_region.as_ffmpeg_filter() == "crop=64:31:0:8"
    assert a.bar_percentage == (1 - 64 * 31 / (64 * 48)) * 100 and a.summary().startswith("Frame: 64x48\nContent: 64x31 (")
    assert R.AspectAnalysis().bar_percentage == 0.0 and R.AspectHandler().analyze([]).summary() == "Full frame content at 0.00:1"
    assert R.create_aspect_handler("4:3", "PAD", "nonsense").config == R.AspectConfig(target_ratio="4:3", method=R.ConversionMethod.PAD)


def test_blur_border_and_weights():
    k = R.gauss99_table()
    assert k.sum() == 256 and k.min() == 0 and k.max() == 7 and (k[:49] == k[:49:-1]).all()     # the carried error alternates 6 and 7 at the top
    assert R.reflect101(np.array([-1, -3, 3, 5, 7, -7]), 3).tolist() == [1, 1, 1, 1, 1, 1] and R.reflect101(np.array([-5, 9]), 1).tolist() == [0, 0]
    flat = np.full((5, 7, 3), 93, np.uint8)
    assert np.array_equal(R.gaussian_blur_99(flat), flat)             # weights that sum to 256 keep a constant
    one = np.arange(6, dtype=np.uint8).reshape(1, 6) * 40
    assert R.gaussian_blur_99(one).shape == (1, 6)
