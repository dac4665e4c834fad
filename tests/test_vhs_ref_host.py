"""CPU: tests/vhs_ref.py, the contract of csrc/vhs.hip, against what tools/gen_vhs_golden.py recorded from the reference's own
`processors/format/vhs.py` (tests/golden/vhs_reference.json / .npz).  Every comparison is exact equality."""
import json
from pathlib import Path

import numpy as np
import pytest

import vhs_ref as R

GOLD = Path(__file__).resolve().parent / "golden"
ANALYSIS_FIELDS = ("head_switching_detected", "head_switching_position", "head_switching_severity", "tracking_errors", "tracking_severity",
                   "tracking_line_positions", "dropout_detected", "dropout_count", "chroma_bleed", "chroma_bleed_severity", "rainbow_effect",
                   "dot_crawl", "jitter_detected", "jitter_severity", "overall_degradation", "detected_quality", "artifact_types")


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "vhs_reference.json").read_text())


@pytest.fixture(scope="module")
def clips():
    return R.clips()


def run_case(clip, method, strength, seed, log=None):
    np.random.seed(seed)
    cfg = R.Config()
    if method == "process":
        return R.process(clip, cfg)
    if method == "dropout":
        return R.fix_dropout(clip, cfg, strength, log)
    return R.METHODS[method](clip, cfg, strength)


def rainbow_ratio(stats):
    return stats["rainbow_diag_max"] / (5 * stats["rainbow_mean_mag"]) if stats["rainbow_mean_mag"] else 0.0


def test_every_recorded_frame(gold, clips):
    """The five methods and `process` on every clip: the reference's digests, and the same frames returned as they are."""
    npz = np.load(GOLD / "vhs_reference.npz")
    n = 0
    for name, clip in clips.items():
        for method, s in R.recorded_cases(name) + [("process", 0.0)]:
            key = R.case_key(name, method, s)
            want_digest, want_same, seed = gold["cases"][key]
            assert seed == R.seed_of(name, method, s)
            log = []
            got = run_case(clip, method, s, seed, log)
            assert R.digest(got) == want_digest, key
            assert "".join("01"[a is b] for a, b in zip(got, clip)) == want_same, key
            if method == "dropout":
                assert name not in gold["dropout_log"] or [[list(b), how, src] for b, how, src in log] == gold["dropout_log"][name], key
            if key in npz.files:
                assert np.array_equal(np.stack(got), npz[key]), key
            n += 1
    assert n == len(gold["cases"]) and n > 150


def test_nothing_to_do_returns_the_list(clips):
    clip = clips["mix_low/37x33"]
    cfg = R.Config()
    for fn in R.METHODS.values():
        assert fn(clip, cfg, 0.0) is clip and fn([], cfg, 0.5) == []
    gray_clip = clips["mix_low/37x33/gray"]
    assert all(a is b for a, b in zip(R.reduce_chroma_bleed(gray_clip, cfg, 0.5), gray_clip))
    assert all(a is b for a, b in zip(R.remove_rainbow_artifacts(gray_clip, cfg, 0.5), gray_clip))


def test_analysis_fields_and_integer_statistics(gold, clips):
    for name, clip in clips.items():
        rec = gold["analysis"][name]
        np.random.seed(rec["seed"])
        a = R.analyze(clip[R.ANALYSIS_FRAME], R.Config())
        for k in ANALYSIS_FIELDS:
            assert getattr(a, k) == rec[k], (name, k)
        assert [list(p) for p in a.dropout_positions] == rec["dropout_positions"], name
        st, mine = gold["stats"][name], R.stats_record(clip[R.ANALYSIS_FRAME])
        for k in ("jitter_shifts", "n_edges"):
            assert mine.get(k) == st.get(k), (name, k)


def test_the_clips_reach_the_cases_they_exist_for(gold, clips):
    an = gold["analysis"]
    for size in ("37x33", "48x64", "64x258"):
        h = int(size.split("x")[0])
        for kind in ("mix_low", "mix_high"):
            if f"{kind}/{size}" not in an:
                continue
            lines = an[f"{kind}/{size}"]["tracking_line_positions"]
            assert 1 in lines and h - 31 in lines and h - 9 not in lines         # the row inside the bottom 30 is filtered out
        assert {"temporal", "spatial", "none"} <= {how for _, how, _ in gold["dropout_log"][f"mix_low/{size}"]}
        srcs = {src for _, how, src in gold["dropout_log"][f"mix_low/{size}"] if how == "temporal"}
        assert 0 in srcs and max(srcs) >= 2                                      # a previous frame, and a next frame behind dirty ones
        assert an[f"chroma5/{size}"]["chroma_bleed_severity"] == 1.0 and an[f"chroma2/{size}"]["chroma_bleed_severity"] == 0.4
        assert 0 < gold["stats"][f"few_edges/{size}"]["n_edges"] < 10
        assert an[f"grating/{size}"]["rainbow_effect"] and not an[f"plain/{size}"]["rainbow_effect"]
        assert an[f"dot_crawl/{size}"]["dot_crawl"] and an[f"jitter/{size}"]["jitter_detected"]
        assert set(gold["stats"][f"jitter/{size}"]["jitter_shifts"]) == {3, -3}
    positions = {an[n]["head_switching_position"] for n in an if an[n]["head_switching_detected"]}
    assert any(p > 16 for p in positions) and any(p <= 16 for p in positions)
    assert not an["dot_crawl/32x8"]["dot_crawl"]                          # fewer than 10 columns of differences
    # overlapping merged boxes: one temporal pair, one spatial pair
    boxes = an["mix_low/48x64"]["dropout_positions"]
    overlaps = [(a, b) for i, a in enumerate(boxes) for b in boxes[i + 1:]
                if a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]]
    assert len(overlaps) == 2


def test_rainbow_fixtures_keep_their_margin(gold):
    """The device's FFT is not NumPy's: the rainbow decision is compared only where the recorded ratio diag_max / (5 mean_mag) is at
    least 1e-6 relative away from 1, and every fixture has to be there."""
    for name, st in gold["stats"].items():
        if "rainbow_diag_max" in st:
            assert abs(rainbow_ratio(st) - 1.0) >= 1e-6, name
            assert (rainbow_ratio(st) > 1.0) == gold["analysis"][name]["rainbow_effect"], name


def test_border_pixels_are_blended_not_copied(clips):
    """float32(0.9) * v + float32(0.1) * v truncates below v for 76 byte values; 0.5, 0.7 and 1.0 give v back for every byte."""
    v = np.arange(256, dtype=np.float32)
    dropped = {s: int(((np.float32(s) * v + np.float32(1 - s) * v).astype(np.uint8) != np.arange(256)).sum()) for s in R.RAINBOW_STRENGTHS}
    assert dropped == {0.5: 0, 0.7: 0, 1.0: 0, 0.9: 76}
    for f in clips["plain/37x33"]:
        assert not np.array_equal(R.rainbow_frame(f, 0.9), R.rainbow_frame(f, 0.9, copy_borders=True))
        assert np.array_equal(R.rainbow_frame(f, 0.7), R.rainbow_frame(f, 0.7, copy_borders=True))


def test_merge_and_groups_are_the_sequential_rule():
    runs = [(10, 3, 10, 1), (30, 3, 10, 1), (15, 4, 20, 1), (0, 9, 5, 1)]
    assert R.merge_dropouts(sorted(runs, key=lambda r: (r[1], r[0]))) == [(10, 3, 10, 1), (15, 3, 25, 2), (0, 9, 5, 1)]
    assert R.merge_dropouts([]) == []
    g = np.full((4, 12), 100, np.uint8)
    g[1, 0:5], g[2, 7:12], g[3, 3:7] = 255, 0, 251
    assert R.dropout_runs(g, 5) == [(0, 1, 5, 1), (7, 2, 5, 1)]
    assert R.dropout_runs(g, 4) == [(0, 1, 5, 1), (7, 2, 5, 1), (3, 3, 4, 1)]


def test_jitter_is_numpys_correlation_on_integers(clips):
    g = R.gray(clips["jitter/48x64"][0])
    for y in (1, 6, 11):
        c = np.correlate(g[y].astype(np.float32), g[y - 1].astype(np.float32), mode="same")   # exact below 2^24: W <= 258
        w = g.shape[1]
        mine = [int(sum(int(g[y][n + j - w // 2]) * int(g[y - 1][n]) for n in range(w) if 0 <= n + j - w // 2 < w)) for j in range(w)]
        assert mine == c.astype(np.int64).tolist()
