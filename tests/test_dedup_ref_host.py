"""tests/dedup_ref.py, the contract of csrc/dedup_hash.hip and framewright_amd/dedup.py, on the CPU: byte for byte against Pillow
itself (both thumbnails), the library's host tap table against the contract's integer for integer, the hash formats, the decision
loop, the result type, the directory methods, and the pixel-hash path against what the reference's own `FrameDeduplicator` found
(tests/golden/dedup_reference.json, written by tools/gen_dedup_golden.py)."""
import ctypes as C
import json
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dedup_ref as dr  # noqa: E402

from framewright_amd import dedup as DD  # noqa: E402

GOLD = Path(__file__).parent / "golden"
SHAPES = [(16, 17), (8, 9), (9, 13), (16, 70), (33, 17), (64, 64), (33, 131), (70, 300), (135, 240), (1080, 1920)]
TAP_PAIRS = [(1920, 17), (1080, 16), (7680, 17), (9, 17), (17, 17), (131, 64), (13, 64)]


@pytest.mark.parametrize("i,shape", list(enumerate(SHAPES)))
def test_contract_equals_pillow_byte_for_byte(i, shape):
    """Every shape once, the four kinds in turn (every kind at two shapes or more), both paths."""
    h, w = shape
    for kind in ([dr.KINDS[i % 4]] if (h, w) == (1080, 1920) else dr.KINDS):
        f = dr.make_frame(kind, h, w)
        im = Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]))
        want_d = np.asarray(im.convert("L").resize((17, 16), Image.Resampling.LANCZOS))
        want_p = np.asarray(im.resize((64, 64), Image.Resampling.LANCZOS).convert("L"))
        assert np.array_equal(dr.thumb(f, 17, 16, True), want_d), (kind, "gray first")
        assert np.array_equal(dr.thumb(f, 64, 64, False), want_p), (kind, "resize first")


@pytest.mark.parametrize("in_size,out_size", TAP_PAIRS)
def test_library_tap_table_equals_the_contract(hip_lib, in_size, out_size):
    xmin, count, table = dr.taps(in_size, out_size)
    ks = hip_lib.fw_pil_lanczos_taps(in_size, out_size, None, None, None, 0)
    assert ks == dr.ksize(in_size, out_size) == table.shape[1]
    gx, gc, gt = np.full(out_size, -1, np.int32), np.full(out_size, -1, np.int32), np.full(out_size * ks, -1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert hip_lib.fw_pil_lanczos_taps(in_size, out_size, p(gx), p(gc), p(gt), gt.size) == ks
    assert np.array_equal(gx, xmin) and np.array_equal(gc, count)
    assert np.array_equal(gt.reshape(out_size, ks), table)
    assert int(count.max()) <= ks and (xmin >= 0).all() and (xmin + count <= in_size).all()
    # refused: too small a capacity, a NULL among the pointers, sizes out of range - nothing is written
    gt[:] = -1
    assert hip_lib.fw_pil_lanczos_taps(in_size, out_size, p(gx), p(gc), p(gt), gt.size - 1) == 0
    assert hip_lib.fw_pil_lanczos_taps(in_size, out_size, p(gx), None, p(gt), gt.size) == 0
    assert hip_lib.fw_pil_lanczos_taps(0, out_size, None, None, None, 0) == 0
    assert hip_lib.fw_pil_lanczos_taps(in_size, 0, None, None, None, 0) == 0
    assert (gt == -1).all()


def test_window_sizes_the_kernels_are_shaped_for():
    assert int(dr.taps(1920, 17)[1].max()) in (677, 678, 679) and int(dr.taps(1080, 16)[1].max()) in (404, 405, 406)
    assert int(dr.taps(9, 17)[1].max()) <= 7 and int(dr.taps(8, 16)[1].max()) <= 7


def test_hex_format_and_hamming_distance():
    bits = np.zeros(256, bool)
    assert dr.bits_to_hex(bits) == "0" * 64
    bits[0] = True
    assert dr.bits_to_hex(bits) == "8" + "0" * 63                    # the first bit is the most significant
    bits[255] = True
    assert dr.bits_to_hex(bits) == "8" + "0" * 62 + "1"
    assert dr.bits_to_bytes(bits) == bytes([0x80] + [0] * 30 + [1])
    nine = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1], bool)               # hash_size 3: 9 bits, ceil(9 / 4) = 3 digits, 2 bytes
    assert dr.bits_to_hex(nine) == "101" and dr.bits_to_bytes(nine) == bytes([0x01, 0x01])
    assert DD._bits_to_hex(dr.bits_to_bytes(nine), 3) == "101" and DD._bits_to_hex(dr.bits_to_bytes(bits), 16) == dr.bits_to_hex(bits)
    assert dr.hamming_hex("8" + "0" * 63, "8" + "0" * 62 + "1") == 1 and dr.hamming_hex("ff", "00") == 8
    f = dr.make_frame("gradient", 33, 131)
    px = dr.thumb(f, 17, 16, True)
    want = "".join("1" if px[r, c + 1] > px[r, c] else "0" for r in range(16) for c in range(16))
    assert dr.dhash_hex(f) == format(int(want, 2), "064x") and len(dr.dhash_hex(f)) == 64
    assert len(dr.dhash_hex(f, 3)) == 3 and len(dr.dhash_hex(f, 8)) == 16


def _flip(hex_str, positions):
    v = int(hex_str, 16)
    for p in positions:
        v ^= 1 << p
    return format(v, "064x")


def test_decision_loop_threshold_and_last_unique():
    base = "5a" * 32
    d5, d6 = _flip(base, [0, 9, 77, 130, 255]), _flip(base, [0, 9, 77, 130, 255, 31])
    assert dr.hamming_hex(base, d5) == 5 and dr.hamming_hex(base, d6) == 6
    assert DD.hash_similarity(base, d5, True) == 1.0 - 5 / 256 >= 0.98 > 1.0 - 6 / 256 == DD.hash_similarity(base, d6, True)
    cfg = DD.DeduplicationConfig()
    r = DD.analyze_hashes([base, d5, d6, d5, base], cfg, 25.0, True)      # d5 is one bit from d6: a duplicate of frame 2; base is 6 from it
    assert r.unique_indices == [0, 2, 4] and r.frame_mapping == {0: 0, 1: 0, 2: 2, 3: 2, 4: 4}
    # a chain that drifts three bits a frame: every frame is within 3 bits of the one before, but frame 2 is 6 from frame 0.
    # Comparison with the previous frame would call all of them duplicates.
    chain = [base, _flip(base, [1, 2, 3]), _flip(base, [1, 2, 3, 4, 5, 6]), _flip(base, [1, 2, 3, 4, 5, 6, 7, 8, 10])]
    assert all(dr.hamming_hex(chain[i], chain[i + 1]) == 3 for i in range(3))
    r = DD.analyze_hashes(chain, cfg, 25.0, True)
    assert r.unique_indices == [0, 2] and r.frame_mapping == {0: 0, 1: 0, 2: 2, 3: 2}
    # the pixel-hash comparison is equality
    r = DD.analyze_hashes([base, d5, d5, base], cfg, 25.0, False)
    assert r.unique_indices == [0, 1, 3] and r.frame_mapping == {0: 0, 1: 1, 2: 1, 3: 3}
    for hashes, perceptual in [([base, d5, d6, d5, base], True), (chain, True), ([base, d5, d5, base], False), ([], True), ([base], False)]:
        got = DD.analyze_hashes(hashes, cfg, 24.0, perceptual)
        want = dr.analyze_hashes(hashes, perceptual, target_fps=24.0)
        assert {k: getattr(got, k) for k in want} == want
    assert DD.analyze_hashes([base, d6], DD.DeduplicationConfig(similarity_threshold=0.97), 25.0, True).unique_indices == [0]


def test_result_properties_and_summary():
    r = DD.DeduplicationResult()
    assert (r.total_frames, r.unique_frames, r.duplicate_frames, r.detected_source_fps, r.target_fps) == (0, 0, 0, 0.0, 25.0)
    assert r.frame_mapping == {} and r.unique_indices == [] and r.duplication_ratio == 0.0 and r.estimated_original_fps == 25.0
    r = DD.DeduplicationResult(total_frames=25, unique_frames=18, duplicate_frames=7, target_fps=25.0)
    assert r.duplication_ratio == 7 / 25 and r.estimated_original_fps == 25.0 * (18 / 25)
    assert r.summary() == "Frames: 18/25 unique (7 duplicates, 28.0% reduction)\nEstimated original FPS: 18.0 (target: 25.0fps)"
    c = DD.DeduplicationConfig()
    assert (c.similarity_threshold, c.use_perceptual_hash, c.hash_size, c.pixel_sample_rate, c.min_unique_ratio,
            c.expected_source_fps) == (0.98, True, 16, 4, 0.3, None)


def test_extract_and_reconstruct_on_a_directory(hip_lib, tmp_path):
    src, uniq, enh, out = tmp_path / "in", tmp_path / "unique", tmp_path / "enh", tmp_path / "out"
    src.mkdir()
    for i in range(6):
        Image.fromarray(np.full((4, 5, 3), 10 * i, np.uint8)).save(src / f"frame_{i:08d}.png")
    res = DD.DeduplicationResult(total_frames=6, unique_frames=3, duplicate_frames=3, unique_indices=[0, 2, 5],
                                 frame_mapping={0: 0, 1: 0, 2: 2, 3: 2, 4: 2, 5: 5})
    dd = DD.DeviceFrameDeduplicator(imagehash_available=False)
    seen = []
    got_dir, got_res = dd.extract_unique_frames(src, uniq, res, progress_callback=seen.append)
    assert got_dir == uniq and got_res is res and seen == [0.0, 1.0]
    assert sorted(p.name for p in uniq.glob("*.png")) == [f"frame_{i:08d}.png" for i in (0, 2, 5)]
    with pytest.raises(ValueError):
        dd.extract_unique_frames(src, uniq, DD.DeduplicationResult())
    # "enhanced" frames: unique frame 2 is missing, so its three positions take the nearest number there is (0: |0 - 2| < |5 - 2|)
    enh.mkdir()
    for i in (0, 5):
        (enh / f"frame_{i:08d}.png").write_bytes((uniq / f"frame_{i:08d}.png").read_bytes())
    seen = []
    assert dd.reconstruct_sequence(enh, out, res, seen.append) == out and seen == [0.0, 1.0]
    files = sorted(out.glob("frame_*.png"))
    assert [p.name for p in files] == [f"frame_{i:08d}.png" for i in range(6)]
    value = [int(np.asarray(Image.open(p))[0, 0, 0]) for p in files]
    assert value == [0, 0, 0, 0, 0, 50]
    (enh / "frame_00000002.png").write_bytes((uniq / "frame_00000002.png").read_bytes())
    dd.reconstruct_sequence(enh, out, res)
    assert [int(np.asarray(Image.open(p))[0, 0, 0]) for p in sorted(out.glob("frame_*.png"))] == [0, 0, 20, 20, 20, 50]
    # the device form repeats objects, it does not copy them
    objs = [object(), object(), object()]
    seq = DD.DeviceFrameDeduplicator.reconstruct_device(objs, res)
    assert [objs.index(o) for o in seq] == [0, 0, 1, 1, 1, 2] and seq[2] is seq[4]
    with pytest.raises(ValueError):
        DD.DeviceFrameDeduplicator.reconstruct_device(objs[:2], res)


def test_pixel_hash_path_equals_the_reference_run():
    J = json.loads((GOLD / "dedup_reference.json").read_text())
    assert len(J["cases"]) >= 3
    for case in J["cases"]:
        clip = dr.make_clip(case["h"], case["w"])
        rate = case["pixel_sample_rate"]
        assert [dr.pixel_md5(f, rate) for f in clip] == case["hashes"]
        want = dict(case["result"], frame_mapping={int(k): v for k, v in case["result"]["frame_mapping"].items()})
        assert dr.analyze(clip, False, sample_rate=rate) == want
        got = DD.analyze_hashes(case["hashes"], DD.DeduplicationConfig(pixel_sample_rate=rate), 25.0, False)
        assert {k: getattr(got, k) for k in want} == want
        assert got.summary() == case["summary"] and got.duplication_ratio == case["duplication_ratio"]
        assert got.estimated_original_fps == case["estimated_original_fps"]
        # the clip is what make_clip promises: an exact repeat, a near repeat that the pixel hash tells apart, a run of three
        assert want["frame_mapping"][1] == 0 and want["frame_mapping"][3] == 3 and [want["frame_mapping"][i] for i in (5, 6, 7)] == [4, 4, 4]


def test_imagehash_probe_and_empty_directory(hip_lib, caplog):
    dd = DD.DeviceFrameDeduplicator()
    assert dd.imagehash_available == DD._imagehash_importable() and isinstance(dd.perceptual, bool)
    assert DD.DeviceFrameDeduplicator(imagehash_available=True).perceptual
    assert not DD.DeviceFrameDeduplicator(DD.DeduplicationConfig(use_perceptual_hash=False), imagehash_available=True).perceptual
    with caplog.at_level(logging.WARNING):
        assert dd.analyze_frames(Path("/nonexistent-frames-dir")).total_frames == 0
    assert "No frames found" in caplog.text
