"""csrc/scene_cuts.hip on the MI355X against its contract, tests/scene_cut_ref.py: fw_scene_ssim_u8 (value, bit equality between
runs, batches and pointer forms), fw_hist64x3_u8 (exact counts), the decisions of `DeviceSceneCutDetector`, and
`FrameInterpolator(device_scene_detection=True)` against the host path.

Shapes: 7 x 7 is one map value; 7 x 64 and 64 x 7 one map row / column; 9 x 13 has an odd H W 3 = 351, so every second frame of a
contiguous clip starts at an odd byte; 16 x 70 and 33 x 131 are ragged inside one or a few 64 x 32 tiles; 70 x 300 crosses the tile
in both directions with ragged edges (64 x 294 map values: 2 x 5 tiles).

Value bound: |device - contract| <= (N + 8) 2^-53, N = (H - 6)(W - 6).  Each map value S is seven correctly rounded float64
operations on exact integers, the same in both, with |S| <= 1; the contract's sum is exactly rounded, and any summation order of N
such terms errs by at most (N - 1) 2^-53 mean|S| on the mean; the two final divisions add one rounding each.
"""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_cut_ref as sr  # noqa: E402

from framewright_amd import _lib, policy  # noqa: E402
from framewright_amd import rife as RF  # noqa: E402
from framewright_amd.scene_cuts import DeviceSceneCutDetector  # noqa: E402
from framewright_amd.synth import synthetic_frames, synthetic_ifnet_state  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden"
SHAPES = [(7, 7), (7, 64), (64, 7), (9, 13), (16, 70), (33, 131), (70, 300)]


def bound(h, w):
    return ((h - 6) * (w - 6) + 8) * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def pairs_of(h, w):
    """{kind: (a, b, contract SSIM)} for one shape, computed once."""
    out = {}
    for kind in sr.PAIR_KINDS:
        a, b = sr.make_pair(kind, h, w)
        out[kind] = (a, b, sr.ssim_frames(a, b))
    return out


@functools.lru_cache(maxsize=None)
def clip_of(h, w):
    """Six frames whose five consecutive pairs are of five kinds, and the contract SSIM of each pair."""
    p = pairs_of(h, w)
    a, b = p["noise3"][:2]
    frames = [a, b, 255 - b, np.full_like(a, 255), np.zeros_like(a), p["gradient_shift"][0]]
    return np.stack(frames), [sr.ssim_frames(frames[i], frames[i + 1]) for i in range(5)]


@pytest.fixture(scope="module")
def det(hip_lib):
    return DeviceSceneCutDetector(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("h,w", SHAPES)
def test_ssim_of_one_pair_meets_the_derived_bound(det, h, w):
    for kind, (a, b, want) in pairs_of(h, w).items():
        got = det.ssim_pair_device(dev(a), dev(b))
        print(f"{h}x{w} {kind}: device {got!r} contract {want!r} |diff| {abs(got - want):.3e} bound {bound(h, w):.3e}")
        assert abs(got - want) <= bound(h, w), (kind, got, want)
    assert det.ssim_pair_device(dev(pairs_of(h, w)["const255"][0]), dev(pairs_of(h, w)["const255"][1])) == 1.0
    assert det.ssim_pair_device(dev(pairs_of(h, w)["const0"][0]), dev(pairs_of(h, w)["const0"][1])) == 1.0
    assert det.ssim_pair_device(dev(pairs_of(h, w)["complement"][0]), dev(pairs_of(h, w)["complement"][1])) < 0.0


@pytest.mark.parametrize("h,w", SHAPES)
def test_ssim_batch_of_five_value_and_bit_equality(det, h, w):
    frames, want = clip_of(h, w)
    t = dev(frames)
    got = det.ssim_pairs_device(t)
    assert len(got) == 5
    for i in range(5):
        print(f"{h}x{w} pair {i}: device {got[i]!r} contract {want[i]!r} |diff| {abs(got[i] - want[i]):.3e} bound {bound(h, w):.3e}")
        assert abs(got[i] - want[i]) <= bound(h, w), (i, got[i], want[i])
    as_bits = lambda v: np.asarray(v, np.float64).view(np.uint64).tolist()
    assert as_bits(det.ssim_pairs_device(t)) == as_bits(got)                                  # two runs
    for i in range(5):
        alone = det.ssim_pairs_device(t[i:i + 2])                                             # a batch of one, contiguous form
        two = det.ssim_pair_device(t[i].clone(), t[i + 1].clone())                            # two unrelated tensors
        assert as_bits(alone) == as_bits([got[i]]) == as_bits([two]), (i, alone, two, got[i])
    assert det.ssim_pairs_device(t[:1]) == []


def test_ssim_from_misaligned_frames(det):
    """9 x 13 frames at every byte offset inside one buffer: the staging reads aligned words around any start."""
    a, b, want = pairs_of(9, 13)["random"]
    n = a.size
    buf = torch.zeros(2 * n + 16, dtype=torch.uint8, device="cuda")
    ref = det.ssim_pair_device(dev(a), dev(b))
    for off in range(4):
        buf[off:off + n] = dev(a).reshape(-1)
        buf[off + n:off + 2 * n] = dev(b).reshape(-1)
        got = det.ssim_pairs_device(buf[off:off + 2 * n].view(2, 9, 13, 3))
        assert got == [ref] and abs(got[0] - want) <= bound(9, 13)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 9), (9, 13), (33, 131), (70, 300)])
def test_histograms_equal_the_contract_exactly(det, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    frames = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 3), 255, np.uint8),
                       np.full((h, w, 3), 131, np.uint8), rng.integers(0, 64, (h, w, 3), dtype=np.uint8),
                       sr.make_pair("gradient_shift", h, w)[0]])
    want = np.stack([sr.hist64x3(f) for f in frames])
    got = det.histograms_device(dev(frames))
    assert got.shape == (5, 3, 64) and np.array_equal(got, want)
    assert np.array_equal(det.histograms_device(dev(frames)), want)
    for i in (0, 1, 4):                                               # one frame alone; in a clip of odd frame size it may be misaligned
        assert np.array_equal(det.histograms_device(dev(frames)[i:i + 1]), want[i:i + 1])


def test_histogram_of_more_pixels_than_one_workgroup_takes(det):
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (2, 95, 173, 3), dtype=np.uint8)    # 16435 pixels: three workgroups, a ragged last one
    assert np.array_equal(det.histograms_device(dev(frames)), np.stack([sr.hist64x3(f) for f in frames]))
    assert np.array_equal(det.histograms_device(dev(frames)[1:]), np.stack([sr.hist64x3(frames[1])]))   # an odd byte offset: the byte path


def test_decisions_on_the_reference_clip_and_synthetic_pairs(det):
    J = json.loads((GOLD / "interpolator_reference.json").read_text())
    clip = np.load(GOLD / "interpolator_reference.npz")["clip"]
    n, thr = len(clip), 0.3
    want_ssim = [sr.ssim_frames(clip[k], clip[k + 1]) for k in range(n - 1)]
    assert all(abs(s - (1.0 - thr)) >= 1e-6 for s in want_ssim)       # every pair is decided: none sits at the threshold
    t = dev(clip)
    assert det.detect_clip_device(t, thr) == J["scene_boundaries"] == sr.detect_clip(clip, thr)
    assert det.detect_clip_device(dev(clip[:, :, :, ::-1]), thr) == J["scene_boundaries"]     # BGR, as `_stream` uploads
    assert [det.scene_change_device(t[k], t[k + 1], thr, use_ssim=False) for k in range(n - 1)] == J["pair_flags"]
    assert [det.scene_change_device(t[k], t[k + 1], thr) for k in range(n - 1)] == \
        [policy.scene_change(clip[k], clip[k + 1], thr) for k in range(n - 1)]
    for h, w in [(9, 13), (33, 131)]:
        for kind, (a, b, s) in pairs_of(h, w).items():
            for thr in (0.3, 0.5):
                assert abs(s - (1.0 - thr)) >= 1e-6, (h, w, kind, thr)
                assert det.scene_change_device(dev(a), dev(b), thr) == policy.scene_change(a, b, thr), (h, w, kind, thr)


def test_short_frames_fall_back_to_the_histogram_and_the_entry_refuses_them(det, hip_lib):
    for kind in sr.PAIR_KINDS:
        a, b = sr.make_pair(kind, 5, 9)
        for thr in (0.3, 0.5):
            assert det.scene_change_device(dev(a), dev(b), thr) == policy.scene_change(a, b, thr), (kind, thr)
    a, b = sr.make_pair("random", 5, 9)
    clip = np.stack([a, b, 255 - b, a])
    assert det.detect_clip_device(dev(clip), 0.3) == [i + 1 for i in range(3) if policy.scene_change(clip[i], clip[i + 1], 0.3)]
    ta, tb = dev(a), dev(b)
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.fw_scene_ssim_u8(p(ta), p(tb), 0, 1, 5, 9, p(out), p(ws), st) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize()
    assert out.item() == -7.0                                         # nothing was launched
    with pytest.raises(_lib.FramewrightHipError):
        det.ssim_pair_device(ta, tb)
    # frames of different sizes: the host's SSIM raises and it takes the histogram branch; so does the device
    big = sr.make_pair("random", 9, 13)[0]
    assert det.scene_change_device(ta, dev(big), 0.3) == policy.scene_change(a, big, 0.3)


def test_interpolator_with_device_scene_detection_equals_the_host_path(hip_lib, tmp_path, monkeypatch):
    """One cut in a four-frame PNG directory: same boundaries, byte-identical output files, same `_scene_boundaries`, monotone
    progress that ends at 1.0 - and every PNG decoded once, against twice on the host path."""
    from PIL import Image
    src = tmp_path / "in"
    src.mkdir()
    frames = list(synthetic_frames(4, 40, 64, seed=21))
    frames[2:] = [255 - f[::-1] for f in frames[2:]]                  # a hard cut between frames 1 and 2
    for i, f in enumerate(frames):
        Image.fromarray(f[:, :, ::-1]).save(src / f"frame_{i + 1:08d}.png")
    thr = 0.5
    assert all(abs(sr.ssim_frames(frames[i], frames[i + 1]) - (1.0 - thr)) >= 1e-6 for i in range(3))
    eng = RF.IFNetEngine("f16")
    eng.load_state_dict(synthetic_ifnet_state())
    cfg = lambda: RF.InterpolationConfig(smoothness="medium", enable_scene_detection=True, scene_threshold=thr)
    host = RF.FrameInterpolator(config=cfg(), engine=eng)
    devi = RF.FrameInterpolator(config=cfg(), engine=eng, device_scene_detection=True)
    reads = []
    real = RF._imread
    monkeypatch.setattr(RF, "_imread", lambda p: (reads.append(Path(p).name), real(p))[1])

    seen_h, seen_d = [], []
    assert host.detect_all_scene_changes(src, seen_h.append) == [2]
    assert devi.detect_all_scene_changes(src, seen_d.append) == [2] == devi._scene_boundaries
    assert seen_d == seen_h and seen_d[-1] == 1.0
    assert sorted(reads) == sorted(2 * [f"frame_{i + 1:08d}.png" for i in range(4)])          # once per file and instance
    files = sorted(src.glob("*.png"))
    for a, b in [(files[0], files[1]), (files[1], files[2])]:
        assert devi.detect_scene_change(a, b) == host.detect_scene_change(a, b)
    assert devi.detect_scene_change(frames[1][:, :, ::-1], frames[2][:, :, ::-1]) is True
    assert devi.detect_scene_change(frames[0][:, :, ::-1], frames[1][:, :, ::-1]) is False

    for fps in (48, 60):                                              # x2, and x4 with a refinement pass
        outs, seen = {}, {}
        for name, fi in (("host", host), ("device", devi)):
            fi._scene_boundaries = []
            del reads[:]
            seen[name] = []
            res = fi.interpolate_frames(src, tmp_path / f"{name}_{fps}", 24.0,
                                        RF.InterpolationConfig(target_fps=fps, smoothness="medium", scene_threshold=thr),
                                        seen[name].append)
            outs[name] = [p.read_bytes() for p in sorted(Path(res["output_dir"]).glob("*.png"))]
            assert res["scene_changes"] == [2] == fi._scene_boundaries
            assert seen[name] == sorted(seen[name]) and seen[name][-1] == 1.0 and seen[name][0] > 0.0
            assert len(reads) == (8 if name == "host" else 4) and set(reads) == {f.name for f in files}
        assert len(outs["host"]) == (7 if fps == 48 else 13) and outs["host"] == outs["device"]
    # scene detection off in the config: the flag changes nothing, no cut is taken
    off = RF.InterpolationConfig(target_fps=48, smoothness="low", enable_scene_detection=False)
    devi._scene_boundaries = []
    del reads[:]
    a = [p.read_bytes() for p in sorted(devi.interpolate(src, tmp_path / "off_d", 24.0, config=off).glob("*.png"))]
    assert len(reads) == 4 and devi._scene_boundaries == []
    b = [p.read_bytes() for p in sorted(host.interpolate(src, tmp_path / "off_h", 24.0, config=off).glob("*.png"))]
    assert a == b
    eng.close()
