"""GPU: csrc/temporal_consistency.hip and `framewright_amd.temporal_consistency` against tests/temporal_consistency_ref.py, byte for
byte and bit for bit: no tolerance anywhere.

The tile of fw_tcons_apply_u8 is TC_TW = 64 columns by TC_TH = 32 rows with a halo of 2 (a workgroup stages 36 rows of up to 68
columns); the shapes below are one less than, equal to and one more than the tile in each direction, the sizes the issue names, and
the smallest frame the reflect-101 halo allows.  Frames are cut from one stacked tensor, so for an odd H W 3 the second and third
frame start at an odd byte: the staged rows are read as aligned words from any alignment."""
import json

import numpy as np
import pytest

import temporal_consistency_ref as R
from framewright_amd import _lib
from framewright_amd import temporal_consistency as TC

pytestmark = pytest.mark.gpu
TILE_H, TILE_W = 32, 64
SHAPES = [(3, 3), (3, 40), (40, 3), (5, 7), (33, 130), (45, 67),
          (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H - 1, TILE_W + 1), (TILE_H + 1, TILE_W - 1)]
FULL = [s for s in SHAPES if min(s) >= 31]                       # frames large enough for 7 x 7 blobs on every border and a centre


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def proc(torch_mod):
    p = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="optical_flow"))
    yield p
    p.close()


def device_frames(torch, arrays):
    """The frames as views of one allocation (frame i starts at byte i H W 3)."""
    return list(torch.from_numpy(np.stack(arrays)).cuda().unbind(0))


def run_kernel(torch, hip_lib, triple, threshold, strength):
    """One launch with all three outputs: (out bytes, mask float32, area numerator)."""
    p, c, n = device_frames(torch, triple)
    h, w = triple[0].shape[:2]
    out, mask = torch.empty_like(c), torch.empty((h, w), dtype=torch.float32, device="cuda")
    area = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _lib.check(hip_lib.fw_tcons_apply_u8(_lib.ptr(p), _lib.ptr(c), _lib.ptr(n), h, w, float(np.float32(threshold)), float(np.float32(strength)),
                                         _lib.ptr(out), _lib.ptr(mask), _lib.ptr(area), _lib.stream_ptr(c.device)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy(), int(area.item())


def expect(triple, threshold, strength):
    k = R.blur_k(R.binary_mask(*triple, threshold))
    mask = R.detect_flicker(*triple, threshold)
    assert np.array_equal(mask.view(np.uint32), R.mask_from_k(k).view(np.uint32))
    return R.blend_frame(triple[0], triple[1], triple[2], mask, strength), mask, k


def triple_for(shape):
    h, w = shape
    triple = R.flicker_triple(h, w, 100 * h + w)
    if shape == (3, 3):                                          # the centre pixel by hand
        prev = np.full((3, 3, 3), 90, np.uint8)
        cur = prev.copy()
        cur[1, 1] = (150, 20, 200)
        triple = (prev, cur, prev + 2)
    return triple


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_equals_the_restatement(torch_mod, hip_lib, shape):
    triple = triple_for(shape)
    assert np.abs(triple[0].astype(int) - triple[2].astype(int)).max() <= 3
    want, mask, k = expect(triple, 0.02, 0.8)
    changed = np.mean(np.any(want != triple[1], axis=2))
    partial = np.mean((k > 0) & (k < 256))
    print(f"{shape}: k max {k.max()}, 0 < k < 256 on {partial:.3f}, changed pixels {changed:.3f}")
    assert partial >= 0.1 and changed >= 0.1                      # the stage has something to do ...
    if shape in FULL or shape in ((33, 130), (45, 67)):
        assert (k == 256).any()                                  # ... and the inside of a blob is fully masked
    if shape == (3, 3):
        assert k[1, 1] == 64 == k.max() and want[1, 1, 0] != triple[1][1, 1, 0]       # (6 + 1 + 1) ^ 2: columns -1 and 3 reflect onto the centre
    out, got_mask, area = run_kernel(torch_mod, hip_lib, triple, 0.02, 0.8)
    assert np.array_equal(got_mask.view(np.uint32), mask.view(np.uint32))
    assert area == R.area_numerator(k)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("threshold", [0.02, 0.1])
def test_decision_sweep_walks_the_score_across_the_threshold(torch_mod, hip_lib, threshold):
    """Every (prev, cur, next) triple of equal-channel greys from {0 .. 47} u {48, 56, .. 248} u {255}, 75^3 pixels as 5625 x 75: the
    score crosses the threshold from both sides, pixel by pixel."""
    triple = R.sweep_triple()
    assert triple[0].shape == (5625, 75, 3)
    want, mask, k = expect(triple, threshold, 0.8)
    binary = R.binary_mask(*triple, threshold)
    score = R.flicker_score(*triple)
    assert 0.01 < binary.mean() < 0.99 and (k == 256).any() and (k == 0).any()
    just = np.abs(score - np.float32(threshold)) < 0.004        # pixels whose score is within one grey code of the threshold
    assert just.sum() > 1000 and binary[just].any() and not binary[just].all()
    out, got_mask, area = run_kernel(torch_mod, hip_lib, triple, threshold, 0.8)
    assert np.array_equal(got_mask.view(np.uint32), mask.view(np.uint32)) and area == R.area_numerator(k)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("strength", [0.0, 0.5, 0.8, 1.0])
def test_blend_strengths(torch_mod, hip_lib, strength):
    triple = R.flicker_triple(45, 67, 9)
    want, mask, k = expect(triple, 0.02, strength)
    out, _, _ = run_kernel(torch_mod, hip_lib, triple, 0.02, strength)
    assert np.array_equal(out, want)
    if strength == 0.0:
        assert np.array_equal(out, triple[1])
    else:
        assert np.mean(np.any(out != triple[1], axis=2)) >= 0.1


def test_extremes(torch_mod, hip_lib, proc):
    lo, hi = np.zeros((33, 70, 3), np.uint8), np.full((33, 70, 3), 255, np.uint8)
    for triple, value in (((lo, hi, lo), 50), ((hi, lo, hi), 204)):           # 255 * (1 - 0.8) = 50.999996, 255 * 0.8 = 204.0
        want, mask, k = expect(triple, 0.02, 0.8)
        assert (k == 256).all() and (want == value).all()
        out, got_mask, area = run_kernel(torch_mod, hip_lib, triple, 0.02, 0.8)
        assert np.array_equal(out, want) and (got_mask == 1.0).all() and area == 256 * 33 * 70
    # an all-equal clip: den2 of the histogram correlation is 0, the correlation 1, no cut, and nothing changes
    flat = [np.full((33, 70, 3), 77, np.uint8)] * 4
    frames = device_frames(torch_mod, flat)
    assert proc.scene_changes_device(frames) == [] and not proc.detect_scene_change_device(frames[0], frames[1])
    out = proc.apply_device(frames)
    assert all(np.array_equal(o.cpu().numpy(), f) for o, f in zip(out, flat))


def test_histograms(torch_mod, hip_lib, proc):
    rng = np.random.default_rng(4)
    for shape in ((45, 67), (130, 257), (3, 3)):
        arrays = [rng.integers(0, 256, shape + (3,), dtype=np.uint8), np.full(shape + (3,), 201, np.uint8),
                  rng.integers(0, 256, shape + (3,), dtype=np.uint8)]
        frames = device_frames(torch_mod, arrays)              # the second and third frame of an odd size start at an odd byte
        first = proc.gray_hists_device(frames).cpu().numpy()
        second = proc.gray_hists_device(frames).cpu().numpy()
        assert first.dtype == np.int32 and np.array_equal(first, second)      # the same bits on two runs
        for got, a in zip(first, arrays):
            assert np.array_equal(got, R.gray_hist(a)) and got.sum() == shape[0] * shape[1]
        assert first[1].max() == shape[0] * shape[1]
        a, b = arrays[0], arrays[2]
        assert proc.detect_scene_change_device(frames[0], frames[2]) == R.detect_scene_change(a, b)
        assert TC.hist_correlation(first[0], first[2]) == R.scene_correlation(a, b)


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


CLIPS = {"cut9": (9, (4,)), "twocuts9": (9, (3, 5)), "plain9": (9, ()), "three": (3, ()), "two": (2, ()), "one": (1, ())}


@pytest.fixture(scope="module")
def clips():
    return {name: R.flicker_clip(n, 40, 70, 31 + k, cuts) for k, (name, (n, cuts)) in enumerate(CLIPS.items())}


@pytest.mark.parametrize("method", ["optical_flow", "hybrid"])
@pytest.mark.parametrize("window", [1, 3, 7])
def test_clip_driver_and_stream_equal_the_restatement(torch_mod, clips, method, window):
    p = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method=method, attention_window=window))
    for name, (n, cuts) in CLIPS.items():
        arrays = clips[name]
        want, want_cuts = R.apply_clip(arrays, method, window)
        assert want_cuts == list(cuts)
        frames = device_frames(torch_mod, arrays)
        assert p.scene_changes_device(frames) == want_cuts
        out = p.apply_device(frames)
        assert same(host(out), want), name
        passed = [i for i in range(n) if R.in_cut_window(i, cuts, window) or n < 3]
        assert all((out[i] is frames[i]) == (i in passed) for i in range(n))      # a frame in a cut's window is the input tensor itself
        made = [out[i] for i in range(n) if i not in passed]
        if len(made) > 1:                                                         # every processed frame is a view of one allocation
            assert len({t.untyped_storage().data_ptr() for t in made}) == 1
        if name in ("cut9", "plain9") and window == 3:
            assert sum(not np.array_equal(w, a) for w, a in zip(want, arrays)) >= 2   # the stage changed frames
        assert same(host(p.apply_device(frames, scene_changes=want_cuts)), want)
        assert same(host(p.stream(iter(frames))), want), name
        assert same(p.apply(arrays), want)
    i = 2
    assert np.array_equal(p.apply_frame_device(device_frames(torch_mod, clips["plain9"]), i).cpu().numpy(),
                          R.apply_frame(clips["plain9"], i, method))
    p.close()


def test_stream_is_behind_its_input_by_the_stated_count(torch_mod, clips):
    for window in (1, 3, 7):
        p = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="optical_flow", attention_window=window))
        fed = []

        def feed():
            for f in device_frames(torch_mod, clips["plain9"]):
                fed.append(1)
                yield f

        lags = [len(fed) - 1 - i for i, _ in enumerate(p.stream(feed()))]
        assert max(lags) == max(R.stream_hold_back(window), 2) and len(lags) == 9      # nothing leaves before three frames have arrived


@pytest.mark.parametrize("strength", [0.5, 1.0])
def test_hybrid_calls_the_hook_where_the_area_decides(torch_mod, clips, strength):
    arrays = clips["cut9"]
    called_ref, called = [], []
    want = R.apply_clip(arrays, R.HYBRID, 3, blend_strength=strength, attention_fn=lambda fr, i: 255 - fr[i], called=called_ref)[0]
    assert called_ref and len(called_ref) < 9 - 3                                  # some frames above 0.01, some below, some in the window

    frames = device_frames(torch_mod, arrays)
    where = [f.data_ptr() for f in frames]

    def hook(held, i):
        """Records the clip index of the centre: from `stream` the list is the frames that are held and i the centre's place in it."""
        assert all(f.data_ptr() in where for f in held)
        called.append(where.index(held[i].data_ptr()))
        return 255 - held[i]

    p = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="hybrid", attention_window=3, blend_strength=strength), hook)
    out = p.apply_device(frames)
    assert called == called_ref and same(host(out), want)
    areas = [p.flicker_area_device(frames[max(0, i - 1)], frames[i], frames[min(8, i + 1)]) for i in range(9)]
    for i, a in enumerate(areas):
        k = R.blur_k(R.binary_mask(arrays[max(0, i - 1)], arrays[i], arrays[min(8, i + 1)]))
        assert a == float(R.area_value(R.area_numerator(k), k.size))
    del called[:]
    assert same(host(p.stream(iter(frames))), want) and called == called_ref
    # CROSS_ATTENTION with a hook: every frame outside the window; without one it is refused
    del called[:]
    q = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="cross_attention", attention_window=3, blend_strength=strength), hook)
    out = host(q.apply_device(frames))
    assert called == [0, 1, 2, 6, 7, 8]
    for i in called:
        assert np.array_equal(out[i], R.add_weighted(arrays[i], 1 - strength, 255 - arrays[i], strength) if strength < 1 else 255 - arrays[i])
    with pytest.raises(ValueError, match="the cross-attention network is not built"):
        TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="cross_attention"))
    # a short clip: the area still decides, the classical path returns the centre
    two = device_frames(torch_mod, clips["two"])
    where = [f.data_ptr() for f in two]
    del called[:]
    called_ref = []
    want = R.apply_clip(clips["two"], R.HYBRID, 3, blend_strength=strength, attention_fn=lambda fr, i: 255 - fr[i], called=called_ref)[0]
    assert same(host(p.apply_device(two)), want) and called == called_ref


def test_apply_consistency_with_readers_and_writers_in_memory(torch_mod, clips, golden_dir, tmp_path):
    js = json.loads((golden_dir / "temporal_consistency_reference.json").read_text())
    recorded = js["driver"]["plain9|hybrid|w7|none3"]
    arrays = clips["plain9"]
    names = [f"frame_{i:08d}.png" for i in range(9)]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for n in names:
        (src / n).write_bytes(n.encode())
    images = dict(zip(names, arrays))
    for none_at in (None, 3):
        written, progress = {}, []
        p = TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method="hybrid"))
        res = p.apply_consistency(src, dst, progress.append, read_image=lambda path: None if none_at is not None and path.name == names[none_at]
                                  else images[path.name], write_image=lambda path, a: written.__setitem__(path.name, a))
        want = R.apply_clip(arrays, R.HYBRID, 7)[0]
        if none_at is None:
            assert (res.frames_processed, res.frames_failed, res.scene_changes_detected) == (9, 0, [])
            assert sorted(written) == names and same([written[n] for n in names], want) and progress == [(i + 1) / 9 for i in range(9)]
            ks = [R.blur_k(R.binary_mask(arrays[max(0, i - 1)], arrays[i], arrays[min(8, i + 1)])) for i in range(9)]
            assert res.flicker_areas == [float(R.area_value(R.area_numerator(k), k.size)) for k in ks]
        else:                                                    # what the reference's own driver did with the same hole
            assert (res.frames_processed, res.frames_failed) == (recorded["frames_processed"], recorded["frames_failed"]) == (6, 3)
            assert sorted(written) == recorded["written"] and len(progress) == len(recorded["progress"])
            assert sorted(f.name for f in dst.iterdir()) == recorded["copied"]
            assert all(np.array_equal(written[n], want[names.index(n)]) for n in written)
        assert res.output_dir == dst and res.flicker_regions_fixed == 0


def test_refusals(torch_mod, proc):
    torch = torch_mod
    good = device_frames(torch, R.flicker_triple(12, 16, 1))
    wrong = "uint8 CUDA tensors H x W x 3"
    for bad in ([good[0], good[1].float(), good[2]], [good[0], good[1][:, :8], good[2]], [good[0], good[1].cpu(), good[2]],
                [good[0][:, :, 0], good[1][:, :, 0], good[2][:, :, 0]]):
        with pytest.raises(ValueError, match=wrong + "|the processor's device"):
            proc.apply_device(bad)
    for small in ((2, 16), (16, 2)):
        with pytest.raises(ValueError, match="3 .. 16384 pixels a side"):
            proc.apply_device(device_frames(torch, R.flicker_triple(*small, 1, blobs=False)))
    with pytest.raises(ValueError, match="a destination overlaps a source frame"):
        proc.apply_frame_device(good, 1, out=good[2])
    with pytest.raises(ValueError, match="a frame index inside the clip"):
        proc.apply_frame_device(good, 3)
    assert proc.apply_device([]) == [] and list(proc.stream(iter([]))) == [] and proc.apply([]) == []
    with pytest.raises(ValueError, match="uint8 arrays H x W x 3"):
        proc.apply([np.zeros((8, 8), np.uint8)])
    closed = TC.DeviceTemporalConsistencyProcessor()
    closed.close()
    with pytest.raises(ValueError, match="the processor is closed"):
        closed.apply_device(good)
    # the C entry refuses an overlapping destination itself
    lib, p = _lib.load(), _lib.ptr
    assert lib.fw_tcons_apply_u8(p(good[0]), p(good[1]), p(good[2]), 12, 16, 0.02, 0.8, p(good[1]), None, None, None) == _lib.FW_ERR_INVALID
