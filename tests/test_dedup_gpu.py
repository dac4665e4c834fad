"""csrc/dedup_hash.hip on the MI355X against its contract, tests/dedup_ref.py (itself held against Pillow byte for byte by
tests/test_dedup_ref_host.py): fw_pil_thumb_u8 and fw_dhash_pack_u8 by exact equality, bit equality between runs, batches and
pointer forms, `DeviceFrameDeduplicator` on clips and directories, and the deduplicating `DeviceRestorationPipeline`.

Shapes (H x W): 16 x 17 leaves out both dHash passes; 8 x 9 and 9 x 13 are upscaling with fs = 1 and windows of at most 7 taps, and
9 x 13 x 3 = 351 is odd, so every second frame of a clip starts on an odd byte; 16 x 70 leaves out the vertical dHash pass, 33 x 17
the horizontal one, 64 x 64 both pixel-hash passes; 33 x 131 and 70 x 300 are ragged with windows clipped at both edges; 135 x 240
is 1080p / 8, windows of about 85 and 51 taps, more than one lane round per window and several workgroups per frame.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dedup_ref as dr  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import dedup as DD  # noqa: E402
from framewright_amd import pipeline as P  # noqa: E402
from framewright_amd import realesrgan as R  # noqa: E402
from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(16, 17), (8, 9), (9, 13), (16, 70), (33, 17), (64, 64), (33, 131), (70, 300), (135, 240)]
MODES = [(17, 16, True), (64, 64, False)]                            # (out_w, out_h, gray_first): the dHash and the pixel-hash thumbnail


@functools.lru_cache(maxsize=None)
def frames_of(h, w):
    """{kind: (frame, {mode: contract thumbnail})} for one shape, computed once."""
    out = {}
    for kind in dr.KINDS:
        f = dr.make_frame(kind, h, w)
        out[kind] = (f, {m: dr.thumb(f, *m) for m in MODES})
    return out


@functools.lru_cache(maxsize=None)
def clip_of(h, w):
    """The first six frames of make_clip (a distinct frame, its repeat, a distinct one, its near repeat, a distinct one, its repeat)
    and the contract thumbnails of each."""
    clip = dr.make_clip(h, w)[:6]
    return clip, {m: np.stack([dr.thumb(f, *m) for f in clip]) for m in MODES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return C.c_void_p(t.data_ptr())


def thumbs_device(lib, t, stride, n, h, w, mode):
    """fw_pil_thumb_u8 on the n frames at t.data_ptr() + f * stride -> numpy n x out_h x out_w."""
    out_w, out_h, gray_first = mode
    out = torch.full((n, out_h, out_w), 7, dtype=torch.uint8, device="cuda")
    nws = lib.fw_pil_thumb_workspace_bytes(n, h, w, out_w, out_h, int(gray_first))
    assert nws == n * (1 if gray_first else 3) * h * out_w
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.fw_pil_thumb_u8(p(t), stride, n, h, w, out_w, out_h, int(gray_first), p(out), p(ws), st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_thumbnails_and_hashes_equal_the_contract(hip_lib, h, w):
    dd_d = DD.DeviceFrameDeduplicator(imagehash_available=True)
    dd_p = DD.DeviceFrameDeduplicator(imagehash_available=False)
    for kind, (f, want) in frames_of(h, w).items():
        t = dev(f)
        for m in MODES:
            got = thumbs_device(hip_lib, t, 0, 1, h, w, m)[0]
            assert np.array_equal(got, want[m]), (kind, m, int(np.abs(got.astype(int) - want[m]).max()))
        # the dHash bytes of the contract's thumbnail, and the two hex strings through the class
        thumb = dev(want[MODES[0]][None])
        bits = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
        _lib.check(hip_lib.fw_dhash_pack_u8(p(thumb), 1, 16, p(bits), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert bits.cpu().numpy().tobytes() == dr.bits_to_bytes(dr.dhash_bits(f))
        assert dd_d.hashes_device(t.unsqueeze(0)) == [dr.dhash_hex(f)]
        assert dd_p.hashes_device([t]) == [dr.pixel_md5(f)]


def test_other_hash_sizes_and_sample_rates(hip_lib):
    f = dr.make_frame("noise", 70, 300)
    t = dev(f).unsqueeze(0)
    for hs in (2, 3, 8, 64):                                          # 3: 9 bits in 2 bytes, 7 zero bits in front; 64: a 65 x 64 thumbnail
        dd = DD.DeviceFrameDeduplicator(DD.DeduplicationConfig(hash_size=hs), imagehash_available=True)
        assert dd.hashes_device(t) == [dr.dhash_hex(f, hs)], hs
    for rate in (1, 3):
        dd = DD.DeviceFrameDeduplicator(DD.DeduplicationConfig(pixel_sample_rate=rate), imagehash_available=False)
        assert dd.hashes_device(t) == [dr.pixel_md5(f, rate)], rate


@pytest.mark.parametrize("h,w", SHAPES)
def test_clip_in_one_launch_equals_single_launches_and_itself(hip_lib, h, w):
    clip, want = clip_of(h, w)
    n, fb = len(clip), h * w * 3
    t = dev(clip)
    padded = torch.zeros((n, fb + 5), dtype=torch.uint8, device="cuda")   # frames 5 bytes apart: every alignment occurs
    padded[:, :fb] = t.reshape(n, fb)
    singles = [t[i].clone() for i in range(n)]
    for m in MODES:
        got = thumbs_device(hip_lib, t, fb, n, h, w, m)
        assert np.array_equal(got, want[m]), m
        assert np.array_equal(thumbs_device(hip_lib, t, fb, n, h, w, m), got)                    # a second run
        assert np.array_equal(thumbs_device(hip_lib, padded, fb + 5, n, h, w, m), got)           # the strided form
        for i in range(n):                                                                       # one pointer per frame
            assert np.array_equal(thumbs_device(hip_lib, singles[i], 0, 1, h, w, m)[0], got[i]), (m, i)
            assert np.array_equal(thumbs_device(hip_lib, t[i], fb, 1, h, w, m)[0], got[i]), (m, i)


def _fields(res):
    return dict(total_frames=res.total_frames, unique_frames=res.unique_frames, duplicate_frames=res.duplicate_frames,
                detected_source_fps=res.detected_source_fps, target_fps=res.target_fps, frame_mapping=res.frame_mapping,
                unique_indices=res.unique_indices)


@pytest.mark.parametrize("perceptual", [True, False])
def test_analyze_clip_device_equals_the_contract(hip_lib, perceptual):
    dd = DD.DeviceFrameDeduplicator(imagehash_available=perceptual)
    for h, w in [(33, 131), (135, 240)]:
        clip = dr.make_clip(h, w)
        want = dr.analyze(clip, perceptual, target_fps=24.0)
        assert 1 < want["unique_frames"] < len(clip)
        assert _fields(dd.analyze_clip_device(dev(clip), 24.0)) == want
        assert _fields(dd.analyze_clip_device([dev(f) for f in clip], 24.0)) == want
    assert dd.analyze_clip_device(dev(clip)[:0]).total_frames == 0


@pytest.mark.parametrize("perceptual", [True, False])
def test_analyze_frames_on_a_directory_with_host_branch_files(hip_lib, tmp_path, perceptual):
    from PIL import Image
    h, w = 70, 300
    clip = dr.make_clip(h, w)
    rgba = np.dstack([clip[2][:, :, ::-1], np.full((h, w), 255, np.uint8)])       # opaque: Pillow's RGBA resize gives the RGB bytes
    for i, f in enumerate(clip):
        img = Image.fromarray(np.ascontiguousarray(f[:, :, ::-1]))
        if i == 3:
            img = Image.fromarray(rgba)                                # frame 3 is frame 2 again, as RGBA: the host branch
        if i == 9:
            img = Image.fromarray(dr.gray_bgr(clip[9]))               # the constant frame as an L file: the host branch
        img.save(tmp_path / f"frame_{i + 1:08d}.png")
    frames = list(clip)
    frames[3] = clip[2]
    frames[9] = np.repeat(dr.gray_bgr(clip[9])[:, :, None], 3, axis=2)
    want = dr.analyze(frames, perceptual)
    dd = DD.DeviceFrameDeduplicator(imagehash_available=perceptual)
    seen = []
    got = dd.analyze_frames(tmp_path, 25.0, seen.append, block=4)
    assert _fields(got) == want and seen == [1.0]
    assert want["frame_mapping"][3] == 2 and want["frame_mapping"][1] == 0
    files = sorted(tmp_path.glob("frame_*.png"))
    hashes = [dr.dhash_hex(f) if perceptual else dr.pixel_md5(f) for f in frames]
    assert [dd._hash_cache[q] for q in files] == hashes
    # a second call hashes nothing: the cache answers (a poisoned entry shows it is read)
    dd._hash_cache[files[1]] = hashes[8]
    assert dd.analyze_frames(tmp_path, 25.0).frame_mapping[1] == 1


def test_refused_arguments_launch_nothing(hip_lib):
    h, w = 9, 13
    t = dev(dr.make_frame("noise", h, w))
    out = torch.full((1, 16, 17), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(4 * 16384, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda stride, n, hh, ww, ow, oh: hip_lib.fw_pil_thumb_u8(p(t), stride, n, hh, ww, ow, oh, 1, p(out), p(ws), st)
    for args in [(0, 0, h, w, 17, 16), (0, 1, 0, w, 17, 16), (0, 1, h, -1, 17, 16), (0, 1, h, w, 66, 16), (0, 1, h, w, 17, 66),
                 (0, 1, h, w, 0, 16), (0, 1, 16385, w, 17, 16), (0, 1, h, 16385, 17, 16), (-1, 1, h, w, 17, 16), (0, 2, h, w, 17, 16)]:
        assert call(*args) == _lib.FW_ERR_INVALID, args
        assert hip_lib.fw_last_error()
    assert hip_lib.fw_pil_thumb_u8(None, 0, 1, h, w, 17, 16, 1, p(out), p(ws), st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_pil_thumb_u8(p(t), 0, 1, h, w, 17, 16, 1, None, p(ws), st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_pil_thumb_u8(p(t), 0, 1, h, w, 17, 16, 1, p(out), None, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_pil_thumb_workspace_bytes(1, h, w, 66, 16, 1) == 0 and hip_lib.fw_pil_thumb_workspace_bytes(0, h, w, 17, 16, 1) == 0
    bits = torch.full((32,), 7, dtype=torch.uint8, device="cuda")
    for n, hs in [(0, 16), (1, 1), (1, 65)]:
        assert hip_lib.fw_dhash_pack_u8(p(out), n, hs, p(bits), st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_dhash_pack_u8(None, 1, 16, p(bits), st) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((bits == 7).all())          # nothing was launched
    with pytest.raises(ValueError):
        DD.DeviceFrameDeduplicator(imagehash_available=True).hashes_device(t)        # three dimensions where a clip is expected


def test_pipeline_upscales_only_unique_frames(hip_lib):
    src = list(synthetic_frames(3, 32, 48, seed=12))
    frames = [src[0], src[0].copy(), src[1], src[2], src[2].copy(), src[2].copy()]
    sr = R.RRDBNetEngine(2, 2, "f16")
    sr.load_state_dict(synthetic_rrdbnet_state(2, 2, seed=5))
    calls = []
    real = sr.upscale_device

    class Counting:
        device_id = sr.device_id

        def upscale_device(self, f):
            calls.append(1)
            return real(f)

    for perceptual in (False, True):
        dd = DD.DeviceFrameDeduplicator(imagehash_available=perceptual)
        want = dr.analyze(frames, perceptual)
        assert want["unique_indices"] == [0, 2, 3]
        plain = P.DeviceRestorationPipeline(upscaler=sr).run(frames)
        del calls[:]
        pipe = P.DeviceRestorationPipeline(upscaler=Counting(), deduplicator=dd)
        got = pipe.run(frames)
        assert len(got) == len(frames) and len(calls) == want["unique_frames"] == pipe.last_dedup_result.unique_frames
        assert _fields(pipe.last_dedup_result) == want
        for i, g in enumerate(got):
            assert g.shape == (64, 96, 3) and np.array_equal(g, sr.upscale(frames[want["frame_mapping"][i]])), i
            assert np.array_equal(g, plain[i])                         # repeated frames are equal bytes: the same as upscaling all
        del calls[:]
        no_dd = P.DeviceRestorationPipeline(upscaler=Counting())
        out = no_dd.run(frames)
        assert len(calls) == len(frames) and no_dd.last_dedup_result is None
        assert all(np.array_equal(a, b) for a, b in zip(out, plain))
    sr.close()
