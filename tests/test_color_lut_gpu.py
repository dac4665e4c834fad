"""GPU: the colour-grade kernels (csrc/color_lut.hip) and their host layer (framewright_amd/color_grade.py) against the contract in
tests/color_lut_ref.py and the outputs recorded from the reference (tests/golden/color_lut_reference.*).  Every comparison is
exact equality."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import color_lut_ref as R
from framewright_amd import _lib
from framewright_amd import color_grade as G

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
LDS_LAST = 17          # the largest table csrc/color_lut.hip holds in LDS; 18 is the first it reads through L2


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "color_lut_reference.json").read_text())


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


_tables = {}


def table(size, season="autumn", strength=0.7):
    key = (size, season, strength)
    if key not in _tables:
        _tables[key] = G.create_seasonal_lut(season, strength, size).table_f32()
    return _tables[key]


def dev_of(torch, a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def host_of(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if np.dtype(dtype) == np.uint16 else a


def raw_apply(torch, lib, src_t, src_stride, n, h, w, tab_t, size, bgr, dst_t, dst_stride, wide, src_off=0, dst_off=0):
    fn = lib.fw_lut3d_apply_u16 if wide else lib.fw_lut3d_apply_u8
    st = fn(C.c_void_p(src_t.data_ptr() + src_off), src_stride, n, h, w, C.c_void_p(tab_t.data_ptr()), size, int(bgr),
            C.c_void_p(dst_t.data_ptr() + dst_off), dst_stride, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("size", R.TABLE_SIZES)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_images_equal_contract_and_golden(torch_mod, gold, size, dtype):
    """Every image size, a batch of three (3 x 5 uint8: frame 1 starts on byte 45), both channel orders, sizes on both sides of the
    LDS limit."""
    assert LDS_LAST in R.TABLE_SIZES and LDS_LAST + 1 in R.TABLE_SIZES
    tab = table(size)
    for bgr in (True, False):
        lut = G.create_seasonal_lut("autumn", 0.7, size)
        grader = G.DeviceColorGrader(lut, bgr=bgr)
        for h, w in R.IMAGE_SIZES:
            clip = R.test_image(h, w, dtype, n=3)
            want = R.apply_lut3d(clip, tab, bgr=bgr)
            got = host_of(grader.apply_device(dev_of(torch_mod, clip)), dtype)
            np.testing.assert_array_equal(got, want, err_msg=f"{size} {h}x{w} bgr={bgr}")
            if bgr:                                                                           # the recorded image is the n = 1 draw
                single = host_of(grader.apply_device(dev_of(torch_mod, R.test_image(h, w, dtype))), dtype)
                assert R.sha256(single[0]) == gold["image_sha256"][f"{size}/{h}x{w}/{np.dtype(dtype).name}"]
            one = host_of(grader.apply_device(dev_of(torch_mod, clip[1:2])), dtype)           # n = 1 against the batch
            np.testing.assert_array_equal(one[0], got[1])


@pytest.mark.parametrize("key,season,strength,size", [("autumn_0.7_33", "autumn", 0.7, 33), ("winter_1.0_17", "winter", 1.0, 17)])
def test_whole_cube_digest(torch_mod, gold, key, season, strength, size):
    """All 2^24 8-bit colours: a complete proof for 8-bit input at this table."""
    torch = torch_mod
    i = torch.arange(R.CUBE_SIDE * R.CUBE_SIDE, dtype=torch.int32, device="cuda")
    img = torch.stack([i & 255, (i >> 8) & 255, i >> 16], dim=-1).to(torch.uint8).reshape(1, R.CUBE_SIDE, R.CUBE_SIDE, 3)
    np.testing.assert_array_equal(img[0, 5:6].cpu().numpy(), R.cube_rows(5, 1))
    grader = G.DeviceColorGrader(G.create_seasonal_lut(season, strength, size))
    out = grader.apply_device(img)
    assert hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() == gold["cube_sha256"][key]
    again = grader.apply_device(img)
    assert torch.equal(out, again)                                                            # bit-identical between runs


@pytest.mark.parametrize("key,season,strength,size", [("autumn_0.7_33", "autumn", 0.7, 33), ("winter_1.0_17", "winter", 1.0, 17)])
def test_hard_colours_and_full_range_u16(torch_mod, gold, key, season, strength, size):
    grader = G.DeviceColorGrader(G.create_seasonal_lut(season, strength, size))
    for dtype in ("uint8", "uint16"):
        for variant, rec in gold["hard"][key][dtype].items():
            if not rec["colours"]:
                continue
            colours = np.asarray(rec["colours"], dtype).reshape(1, -1, 1, 3)
            got = host_of(grader.apply_device(dev_of(torch_mod, colours)), dtype)
            np.testing.assert_array_equal(got.reshape(-1, 3), np.asarray(rec["out"], dtype), err_msg=f"{dtype} {variant}")
    full = R.full_range_u16()
    got = host_of(grader.apply_device(dev_of(torch_mod, full[None])), np.uint16)[0]
    np.testing.assert_array_equal(got, R.apply_lut3d(full, table(size, season, strength)))
    assert R.sha256(got) == gold["full_range_u16_sha256"][key]


def test_identity_returns_the_input(torch_mod, gold):
    grader = G.DeviceColorGrader(G.create_identity_lut(33))
    for dtype in (np.uint8, np.uint16):
        img = R.test_image(64, 64, dtype)
        got = host_of(grader.apply_device(dev_of(torch_mod, img)), dtype)
        assert R.sha256(got[0]) == gold["identity"][np.dtype(dtype).name]["sha256"]
        if gold["identity"][np.dtype(dtype).name]["returns_input"]:
            np.testing.assert_array_equal(got, img)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None, None], 3, axis=3)
    np.testing.assert_array_equal(host_of(grader.apply_device(dev_of(torch_mod, ramp)), np.uint8), ramp)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("size", [LDS_LAST, 33])
def test_layouts_in_place_and_sentinels(torch_mod, hip_lib, dtype, size):
    """Contiguous, strided and per-frame pointers agree; in place equals out of place; the bytes around every destination frame
    stay what they were.  3 x 5 frames: with a stride of 45 + 9 bytes (uint8) the frames start on bytes 1, 55, 109 of the buffer."""
    torch = torch_mod
    wide = np.dtype(dtype) == np.uint16
    item = 2 if wide else 1
    h, w, n = 3, 5, 3
    tab = table(size)
    tab_t = torch.from_numpy(tab).cuda()
    clip = R.test_image(h, w, dtype, n=n, seed=3)
    want = R.apply_lut3d(clip, tab)
    fb = h * w * 3 * item
    lead, gap = (2 if wide else 1), (10 if wide else 9)
    stride = fb + gap
    total = lead + n * stride + 16

    def buffer_with(frames):
        buf = np.full(total, 0xA5, np.uint8)
        for k in range(n):
            buf[lead + k * stride: lead + k * stride + fb] = frames[k].reshape(-1).view(np.uint8)
        return buf

    src = torch.from_numpy(buffer_with(clip)).cuda()
    dst = torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda")
    assert raw_apply(torch, hip_lib, src, stride, n, h, w, tab_t, size, True, dst, stride, wide, lead, lead) == _lib.FW_OK
    expect = np.full(total, 0x5A, np.uint8)
    for k in range(n):
        expect[lead + k * stride: lead + k * stride + fb] = want[k].reshape(-1).view(np.uint8)
    np.testing.assert_array_equal(dst.cpu().numpy(), expect)                                  # strided, and the sentinels
    # per-frame pointers
    dst2 = torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda")
    for k in range(n):
        assert raw_apply(torch, hip_lib, src, 0, 1, h, w, tab_t, size, True, dst2, 0, wide, lead + k * stride, lead + k * stride) == _lib.FW_OK
    assert torch.equal(dst, dst2)
    # in place, strided: the source buffer becomes the expectation with its own sentinels
    assert raw_apply(torch, hip_lib, src, stride, n, h, w, tab_t, size, True, src, stride, wide, lead, lead) == _lib.FW_OK
    expect_in = buffer_with(want)
    np.testing.assert_array_equal(src.cpu().numpy(), expect_in)
    # contiguous through the host layer, out of place and in place
    grader = G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, size))
    t = dev_of(torch, clip)
    out = grader.apply_device(t)
    np.testing.assert_array_equal(host_of(out, dtype), want)
    np.testing.assert_array_equal(host_of(t, dtype), clip)
    same = grader.apply_device(t, inplace=True)
    assert same.data_ptr() == t.data_ptr()
    np.testing.assert_array_equal(host_of(t, dtype), want)
    # a list of frames, and a strided view of a larger clip
    outs = grader.apply_device([dev_of(torch, f) for f in clip])
    np.testing.assert_array_equal(np.stack([host_of(o, dtype) for o in outs]), want)
    big = dev_of(torch, np.concatenate([clip, clip], axis=0))
    np.testing.assert_array_equal(host_of(grader.apply_device(big[::2]), dtype), want[[0, 2, 1]])


def test_refused_arguments(torch_mod, hip_lib):
    torch = torch_mod
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    tab_t = torch.from_numpy(table(5)).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    bad = [
        (p(src), 12, 1, 2, 2, p(tab_t), 1, 1, p(dst), 12, st),           # size below 2
        (p(src), 12, 1, 2, 2, p(tab_t), 66, 1, p(dst), 12, st),          # size above 65
        (None, 12, 1, 2, 2, p(tab_t), 5, 1, p(dst), 12, st),
        (p(src), 12, 1, 2, 2, None, 5, 1, p(dst), 12, st),
        (p(src), 12, 1, 2, 2, p(tab_t), 5, 1, None, 12, st),
        (p(src), 12, 0, 2, 2, p(tab_t), 5, 1, p(dst), 12, st),
        (p(src), 12, 1, 0, 2, p(tab_t), 5, 1, p(dst), 12, st),
        (p(src), 12, 1, 2, -1, p(tab_t), 5, 1, p(dst), 12, st),
        (p(src), -12, 2, 2, 2, p(tab_t), 5, 1, p(dst), 12, st),
        (p(src), 0, 2, 2, 2, p(tab_t), 5, 1, p(dst), 12, st),
    ]
    for fn in (hip_lib.fw_lut3d_apply_u8, hip_lib.fw_lut3d_apply_u16):
        for args in bad:
            assert fn(*args) == _lib.FW_ERR_INVALID, args
            assert b"fw_lut3d_apply" in hip_lib.fw_last_error()
    assert hip_lib.fw_lut3d_apply_u16(C.c_void_p(src.data_ptr() + 1), 24, 1, 2, 2, p(tab_t), 5, 1, p(dst), 24, st) == _lib.FW_ERR_INVALID
    tabs = torch.zeros(768, dtype=torch.uint8, device="cuda")
    assert hip_lib.fw_table3_apply_u8(p(src), 12, 1, 2, 2, None, p(dst), 12, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_table3_apply_u8(None, 12, 1, 2, 2, p(tabs), p(dst), 12, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_table3_apply_u8(p(src), 12, 1, 2, 0, p(tabs), p(dst), 12, st) == _lib.FW_ERR_INVALID
    assert b"fw_table3_apply_u8" in hip_lib.fw_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7).all())                                        # nothing was launched
    with pytest.raises(ValueError):
        G.DeviceColorGrader(G.create_identity_lut(66))


def test_table3_against_the_1d_golden(torch_mod, hip_lib, gold):
    torch = torch_mod
    contrast = G.create_contrast_lut(1.2, 33)
    grader = G.DeviceColorGrader(contrast)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None, None], 3, axis=3)
    np.testing.assert_array_equal(grader.apply(ramp[0])[:, 0, :], np.asarray(gold["ramp_1d_contrast"], np.uint8))
    odd = gold["odd_1d"]
    lut = G.LUT(lut_type=G.LUTType.LUT_1D, size=len(odd["data"]), domain_min=tuple(odd["domain_min"]), domain_max=tuple(odd["domain_max"]),
                data_1d=np.asarray(odd["data"], np.float64))
    img = np.asarray(odd["image"], np.uint8)[:, None, :]
    np.testing.assert_array_equal(G.DeviceColorGrader(lut).apply(img)[:, 0, :], np.asarray(odd["out"], np.uint8))
    # ragged sizes, a batch with odd frame starts, in place
    tabs = G.byte_tables_1d(lut)
    g = G.DeviceColorGrader(lut)
    for h, w in R.IMAGE_SIZES[:4]:
        clip = R.test_image(h, w, np.uint8, n=3, seed=5)
        t = dev_of(torch, clip)
        np.testing.assert_array_equal(g.apply_device(t).cpu().numpy(), R.apply_table3(clip, tabs))
        g.apply_device(t, inplace=True)
        np.testing.assert_array_equal(t.cpu().numpy(), R.apply_table3(clip, tabs))
    with pytest.raises(ValueError):
        g.apply(R.test_image(3, 5, np.uint16)[0])


def test_apply_and_grade_directory(torch_mod, tmp_path, caplog):
    from PIL import Image
    tab = table(33)
    grader = G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7))
    for dtype in (np.uint8, np.uint16):
        img = R.test_image(33, 131, dtype, seed=9)[0]
        np.testing.assert_array_equal(grader.apply(img), R.apply_lut3d(img, tab))
    frames = R.test_image(24, 40, np.uint8, n=4, seed=2)                 # BGR
    for k, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(tmp_path / f"frame_{k:08d}.png")
    (tmp_path / "frame_00000009.png").write_bytes(b"not a png")          # a frame that fails is skipped
    seen = []
    assert G.DeviceColorGrader.grade_directory(tmp_path, "autumn", 0.7, progress=seen.append) == 4
    assert seen == [0.0, 1.0]
    for k, f in enumerate(frames):
        got = np.asarray(Image.open(tmp_path / f"frame_{k:08d}.png").convert("RGB"))[:, :, ::-1]
        np.testing.assert_array_equal(got, R.apply_lut3d(f, tab))
    assert (tmp_path / "frame_00000009.png").read_bytes() == b"not a png"
    empty = tmp_path / "empty"
    empty.mkdir()
    with caplog.at_level("WARNING"):
        assert G.DeviceColorGrader.grade_directory(empty, "winter") == 0
    assert "No frames found" in caplog.text


def test_pipeline_with_color_grader(torch_mod):
    """run_device and stream_device with color_grader= equal grading the output of the same pipeline without it."""
    torch = torch_mod
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.rife import IFNetEngine
    from framewright_amd.synth import synthetic_frames, synthetic_ifnet_state
    eng = IFNetEngine("f16", device_id=0)
    eng.load_state_dict(synthetic_ifnet_state(seed=3))
    frames = synthetic_frames(3, 64, 96, seed=4)
    grader = G.DeviceColorGrader(G.create_seasonal_lut("winter", 1.0))
    tab = table(33, "winter", 1.0)
    plain = DeviceRestorationPipeline(interpolator=eng)
    graded = DeviceRestorationPipeline(interpolator=eng, color_grader=grader)
    base = [t.cpu().numpy() for t in plain.run_device(frames)]
    assert len(base) == 5
    for got in ([t.cpu().numpy() for t in graded.run_device(frames)], [t.cpu().numpy() for t in graded.stream_device(iter(frames))]):
        assert len(got) == len(base)
        for a, b in zip(got, base):
            np.testing.assert_array_equal(a, R.apply_lut3d(b, tab))
    again = [t.cpu().numpy() for t in plain.run_device(frames)]          # with None the pipeline does what it did
    for a, b in zip(again, base):
        np.testing.assert_array_equal(a, b)
    only = DeviceRestorationPipeline(color_grader=grader).run_device(frames)
    np.testing.assert_array_equal(only[0].cpu().numpy(), R.apply_lut3d(frames[0], tab))
    eng.close()
