"""GPU: csrc/quality.hip and framewright_amd/quality.py against the contract in tests/quality_ref.py and the results recorded from the
reference (tests/golden/quality_reference.json).  The statistics are equal integer for integer; the scores, issue lists and reports
are equal to the record, the sharpness and noise scores and what is formed from them within the float bound of DESIGN K19
(`quality_ref.score_tolerances`)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import quality_ref as R
from framewright_amd import _lib
from framewright_amd import quality as Q

pytestmark = pytest.mark.gpu
GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "quality_reference.json").read_text())
CLIPS = R.clips()
# the kernel's tile is 32 rows x 64 columns: sizes one row or column to either side of its seams are the even neighbours 30 / 34 and
# 62 / 66 (odd sides are refused), next to the sizes the block boundaries and the thumbnail paths change at
SIZES = [(2, 2), (16, 16), (18, 26), (34, 38), (66, 130), (130, 66), (64, 258), (270, 480), (30, 62), (32, 64), (34, 66), (64, 128), (96, 190),
         (32, 32), (64, 64), (2, 300), (300, 2)]


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def scorer(torch_mod):
    return Q.DeviceFrameQualityScorer()


def frame(h, w, seed):
    rng = np.random.default_rng(seed)
    f = R._scene(rng, h, w, texture=12.0)
    f[:, : w // 2] = np.clip(f[:, : w // 2].astype(np.int64) + rng.integers(-90, 91, (h, w // 2, 3)), 0, 255)   # strong and weak gradients
    return f


def assert_statistics(got, f):
    want = R.frame_statistics(f)
    for k in R.SCALARS:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in R.ARRAYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), k


@pytest.mark.parametrize("h,w", SIZES)
def test_statistics_equal_the_contract(torch_mod, scorer, h, w):
    f = frame(h, w, 100 * h + w)
    assert_statistics(scorer.frame_statistics([torch_mod.from_numpy(f).cuda()])[0], f)


@pytest.mark.parametrize("h,w", [(512, 2048), (520, 4160)])          # the second: 17 x 65 tiles, more than the 1024 workgroups of a frame
def test_accumulator_widths(torch_mod, scorer, h, w):
    board = np.zeros((h, w, 3), np.uint8)
    board[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = 255
    white = np.full((h, w, 3), 255, np.uint8)
    got = scorer.frame_statistics([torch_mod.from_numpy(board).cuda(), torch_mod.from_numpy(white).cuda()])
    n = h * w
    # known answers, so the large frames need no CPU pass: every Laplacian of the board is +-1020 (the border reflects onto the other
    # colour), the blur is (6 + 6 * 6 + ... ) of one colour: 128 of 256 weights -> (255 * 128 + 128) >> 8 = 128 -> d = 128 or 127
    assert got[0]["lap_sum"] == 0 and got[0]["lap_sq_sum"] == 1020 * 1020 * n
    assert got[0]["noise_sum"] == (128 + 127) * n // 2 and got[0]["noise_sq_sum"] == (128 * 128 + 127 * 127) * n // 2
    assert got[0]["edge_sum"] == 0 and got[0]["row_pair_sum"] == got[0]["col_pair_sum"] == 255 * n // 2
    assert got[0]["byte_sum"] == 255 * 3 * n // 2 and got[0]["byte_sq_sum"] == 255 * 255 * 3 * n // 2
    assert got[0]["gray_hist"][0] == got[0]["gray_hist"][255] == n // 2 and got[0]["byte_hist"][255] == 3 * n // 2
    assert (got[0]["block_rows"] == 255 * w).all() and (got[0]["block_cols"] == 255 * h).all()
    assert len(got[0]["block_rows"]) == len(range(8, h - 8, 8)) and len(got[0]["block_cols"]) == len(range(8, w - 8, 8))
    assert got[0]["strong"] == 0 and got[0]["weak"] == 0               # [1 2 1] x [-1 0 1] of a checkerboard cancels
    assert got[1]["byte_sum"] == 255 * 3 * n and got[1]["byte_sq_sum"] == 255 * 255 * 3 * n and got[1]["gray_hist"][255] == n
    assert got[1]["lap_sq_sum"] == got[1]["noise_sq_sum"] == got[1]["edge_sum"] == 0 and (got[1]["thumbnail"] == 255).all()
    if h == 512:
        assert_statistics(got[0], board)


def test_a_batch_equals_single_calls_and_runs_are_identical(torch_mod, scorer):
    frames = [frame(66, 130, s) for s in range(5)]
    dev = [torch_mod.from_numpy(f).cuda() for f in frames]
    batch = scorer.frame_statistics(dev)
    again = scorer.frame_statistics(dev)
    for i, f in enumerate(frames):
        single = scorer.frame_statistics([dev[i]])[0]
        assert R.statistics_equal(batch[i], single) and R.statistics_equal(batch[i], again[i])
        assert_statistics(batch[i], f)
    many = [dev[i % 5] for i in range(Q.BATCH + 3)]                   # more than one launch
    for i, s in enumerate(scorer.frame_statistics(many)):
        assert R.statistics_equal(s, batch[i % 5])


def test_statistics_device_and_reused_destinations(torch_mod, scorer):
    small, large = frame(18, 26, 1), frame(130, 66, 2)
    ds, dl = torch_mod.from_numpy(small).cuda(), torch_mod.from_numpy(large).cuda()
    out = torch_mod.full((scorer.statistics_bytes(2, 130, 66) + 8,), 0xA5, dtype=torch_mod.uint8, device="cuda")
    for frames, hosts in (([dl, dl], [large, large]), ([ds], [small]), ([dl], [large]), ([ds, ds], [small, small])):
        v = scorer.statistics_device(frames, out=out)
        h, w = hosts[0].shape[:2]
        assert v["sums"].dtype == torch_mod.int64 and tuple(v["sums"].shape) == (len(frames), 12) and v["sums"].is_cuda
        assert tuple(v["histograms"].shape) == (len(frames), 512) and tuple(v["thumbnails"].shape) == (len(frames), 1024)
        assert tuple(v["block_sums"].shape) == (len(frames), len(range(8, h - 8, 8)) + len(range(8, w - 8, 8)))
        for got, f in zip(scorer._fetch_statistics(v, frames[0].device, h, w), hosts):
            assert_statistics(got, f)
        assert int(out[-1]) == 0xA5
    fresh = scorer.statistics_device([ds])
    assert fresh["sums"].data_ptr() != out.data_ptr()
    # the stage's scratch, reused across sizes
    for f, d in ((large, dl), (small, ds), (large, dl)):
        assert_statistics(scorer.frame_statistics([d])[0], f)
    with pytest.raises(ValueError, match="out must be"):
        scorer.statistics_device([dl], out=out[:100])
    with pytest.raises(ValueError, match="out must be"):
        scorer.statistics_device([ds], out=out[1:])


@pytest.mark.parametrize("name", sorted(n for n, c in CLIPS.items() if not c.get("raises")))
def test_scores_and_report_equal_the_record(torch_mod, name):
    clip, rec = CLIPS[name], GOLD["clips"][name]
    seen = []
    scorer = Q.DeviceFrameQualityScorer(progress_callback=lambda k, end: seen.append(k), **R.scorer_arguments(clip))
    dev = [torch_mod.from_numpy(f).cuda() for f in clip["frames"]]
    n = dev[0].shape[0] * dev[0].shape[1] if dev else 0
    report = scorer.analyze_frames(dev, clip["fps"], video_path=name, **R.loop_arguments(clip))
    R.assert_report_matches(report, rec["report"], n)
    assert seen == [r["frame_number"] for r in rec["scores"]]
    by_number = {f.frame_number: f for f in report.problem_frames}
    for want in rec["scores"]:
        if want["frame_number"] in rec["report"]["problem_frames"]:
            R.assert_score_matches(by_number[want["frame_number"]], want, n)
    # the same through score_frame, one call a frame, and through the numpy form
    scorer.reset()
    for want in rec["scores"]:
        R.assert_score_matches(scorer.score_frame(dev[want["frame_number"]], want["frame_number"], clip["fps"]), want, n)
    R.assert_report_matches(scorer.analyze_frames_host(clip["frames"], clip["fps"], video_path=name, **R.loop_arguments(clip)), rec["report"], n)
    assert isinstance(report, Q.QualityReport) and all(isinstance(i, Q.QualityIssue) for f in report.problem_frames for i in f.issues)


def test_the_value_types_and_thresholds_are_the_contracts(torch_mod, scorer, tmp_path):
    assert [(i.name, i.value) for i in Q.QualityIssue] == [(i.name, i.value) for i in R.QualityIssue]
    for name in ("BLUR_THRESHOLD", "NOISE_THRESHOLD", "OVEREXPOSED_THRESHOLD", "UNDEREXPOSED_THRESHOLD", "BLACK_FRAME_THRESHOLD", "DUPLICATE_THRESHOLD"):
        assert getattr(Q.DeviceFrameQualityScorer, name) == getattr(R.FrameQualityScorer, name)
    assert Q._SENTENCES == R.RECOMMENDATIONS and Q.DeviceFrameQualityScorer(sample_rate=0).sample_rate == 1
    clip = CLIPS["issues/48x64"]
    report = scorer.analyze_frames([torch_mod.from_numpy(f).cuda() for f in clip["frames"]], 25.0, video_path="clip")
    want = R.FrameQualityScorer().analyze_frames(clip["frames"], 25.0, video_path="clip")
    assert [f.frame_number for f in report.get_worst_frames(3)] == [f.frame_number for f in want.get_worst_frames(3)]
    assert [f.frame_number for f in report.get_frames_with_issue(Q.QualityIssue.BLUR)] == [f.frame_number for f in want.get_frames_with_issue(R.QualityIssue.BLUR)]
    report.save(tmp_path / "report.json")
    saved = json.loads((tmp_path / "report.json").read_text())
    assert saved.keys() == want.to_dict().keys() and saved["issue_counts"] == want.issue_counts and saved["recommendations"] == want.recommendations


def test_duplicate_state(torch_mod):
    scorer = Q.DeviceFrameQualityScorer()
    clip = CLIPS["duplicates/48x64"]["frames"]
    scene, flat = torch_mod.from_numpy(clip[0]).cuda(), torch_mod.from_numpy(clip[2]).cuda()
    dup = lambda s: Q.QualityIssue.DUPLICATE in s.issues            # noqa: E731
    assert not dup(scorer.score_frame(scene, 0, 30.0)) and dup(scorer.score_frame(scene, 1, 30.0))     # across calls
    assert scorer.score_frame(flat, 2, 30.0).issues == [Q.QualityIssue.CORRUPTED]
    assert dup(scorer.score_frame(scene, 3, 30.0))                   # the corrupted frame left the state alone
    scorer.reset()
    assert scorer._prev_frame_hash is None and not dup(scorer.score_frame(scene, 4, 30.0))
    assert scorer._prev_frame_hash.nbytes == 1024                    # what is kept of a frame
    report = scorer.analyze_frames([scene], 30.0)                    # cleared by analyze_frames: no duplicate of the call before
    assert report.issue_counts["duplicate"] == 0 and report.analyzed_frames == 1


def test_empty_clip_and_window(torch_mod, scorer):
    report = scorer.analyze_frames([], 25.0, video_path="nothing")
    assert report.analyzed_frames == 0 and report.recommendations == [R.RECOMMENDATIONS["none"]] and report.average_score == 0
    d = [torch_mod.from_numpy(f).cuda() for f in CLIPS["sampled/32x48"]["frames"]]
    s = Q.DeviceFrameQualityScorer(sample_rate=2)
    assert s.analyze_frames(d, 24.0, start_frame=1).analyzed_frames == 3 and s.analyze_frames(d, 24.0, start_frame=1, end_frame=4).analyzed_frames == 2
    assert s.analyze_frames(d, 24.0, start_frame=9).analyzed_frames == 0 and s.analyze_frames(d, 24.0, total_frames=3).analyzed_frames == 2


def test_refusals(torch_mod, scorer):
    good = torch_mod.zeros((16, 16, 3), dtype=torch_mod.uint8, device="cuda")
    cases = [([torch_mod.zeros((16, 16), dtype=torch_mod.uint8, device="cuda")], "BGR frames H x W x 3 expected"),
             ([good.float()], "uint8 tensors expected"), ([good.cpu()], "the scorer's device, expected"),
             ([good, torch_mod.zeros((16, 18, 3), dtype=torch_mod.uint8, device="cuda")], "of one shape expected"),
             ([torch_mod.zeros((15, 16, 3), dtype=torch_mod.uint8, device="cuda")], "even number of rows and columns"),
             ([torch_mod.zeros((16, 17, 3), dtype=torch_mod.uint8, device="cuda")], "even number of rows and columns"),
             ([np.zeros((16, 16, 3), np.uint8)], "uint8 tensors expected"), ([], "at least one frame expected")]
    for frames, message in cases:
        with pytest.raises(ValueError, match=message):
            scorer.statistics_device(frames)
        if frames:
            with pytest.raises(ValueError, match=message):
                scorer.score_frame(frames[0], 0, 25.0) if len(frames) == 1 else scorer.analyze_frames(frames, 25.0)
    for clip in ("odd_height/33x48", "odd_width/32x47"):                # a ValueError, as the reference raises one
        with pytest.raises(ValueError):
            scorer.analyze_frames([torch_mod.from_numpy(f).cuda() for f in CLIPS[clip]["frames"]], 25.0)


def test_cabi_refusals(torch_mod, scorer):
    lib = _lib.load()
    f = torch_mod.zeros((16, 16, 3), dtype=torch_mod.uint8, device="cuda")
    out = torch_mod.zeros(8192 + 4096, dtype=torch_mod.uint8, device="cuda")
    p = lambda off: C.c_void_p(out.data_ptr() + off)                 # noqa: E731
    st = _lib.stream_ptr(f.device)
    table = _lib.ptr_table([f])

    def call(frames=table, n=1, h=16, w=16, scratch=p(8192), sums=p(0), hists=p(1024), blocks=p(4096), thumbs=p(5120)):
        return lib.fw_quality_stats_u8(frames, n, h, w, scratch, sums, hists, blocks, thumbs, st)

    assert lib.fw_quality_scratch_bytes(1, 16, 16) == 96 + 2048 and lib.fw_quality_scratch_bytes(0, 16, 16) == 0
    assert lib.fw_quality_scratch_bytes(1, 4320, 7680) == 1024 * (96 + 2048) and lib.fw_quality_scratch_bytes(32, 4320, 7680) == 32 * 64 * (96 + 2048)
    assert call() == 0
    for kwargs, message in (({"n": 0}, "1 .. 32 frames"), ({"n": 33}, "1 .. 32 frames"), ({"h": 15}, "even number"), ({"w": 0}, "1 .. 16384"),
                            ({"h": 16386}, "1 .. 16384"), ({"frames": None}, "null pointer"), ({"sums": None}, "null pointer"),
                            ({"thumbs": None}, "null pointer"), ({"frames": (C.c_void_p * 1)(None)}, "null pointer"),
                            ({"hists": C.c_void_p(f.data_ptr() + 8)}, "overlaps a frame"), ({"scratch": None}, "null pointer"),
                            ({"scratch": p(8196)}, "8-byte aligned"), ({"sums": p(4)}, "8-byte aligned"), ({"scratch": p(1024)}, "overlaps the scratch"),
                            ({"scratch": C.c_void_p(f.data_ptr())}, "overlaps a frame")):
        assert call(**kwargs) != 0
        assert message in lib.fw_last_error().decode(), (kwargs, lib.fw_last_error())
