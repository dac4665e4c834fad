"""GPU: csrc/aspect.hip and framewright_amd/aspect.py against the contract in tests/aspect_ref.py and the results recorded from the
reference (tests/golden/aspect_reference.json).  Every comparison is exact equality."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import aspect_ref as R
from framewright_amd import _lib
from framewright_amd import aspect as A

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
CLIPS = R.clips()
FRAMES = R.convert_frames()
CASES = {c[0]: (name, c) for name, frames in FRAMES.items() for c in R.convert_cases(name, frames)}
SENTINEL, PAD = 0xA5, 64


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "aspect_reference.json").read_text())


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def handler(torch_mod):
    return A.DeviceAspectHandler()


def upload(torch, clip, offset=None):
    """The clip on the device: one tensor per frame, or (``offset``) views that start that many bytes into a padded allocation."""
    if offset is None:
        return [torch.from_numpy(f).cuda() for f in clip]
    host = np.stack(clip)
    flat = np.full(host.size + 2 * PAD, SENTINEL, np.uint8)
    flat[PAD + offset: PAD + offset + host.size] = host.reshape(-1)
    buf = torch.from_numpy(flat).cuda()
    return list(buf[PAD + offset: PAD + offset + host.size].view(host.shape).unbind(0))


def host(frames):
    return [t.cpu().numpy() for t in frames]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def device_handler(method, fill):
    return R.handler_for(method, fill, A.DeviceAspectHandler, A.AspectConfig, A.ConversionMethod, A.FillMode)


def bars(analyses):
    return [[a.top_bar, a.bottom_bar, a.left_bar, a.right_bar] for a in analyses]


# ---- statistics and analysis --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_bar_sums_equal_numpy(torch_mod, handler, gold, name):
    clip = CLIPS[name]
    rows, cols = handler.bar_sums_device(upload(torch_mod, clip))
    assert rows.dtype == cols.dtype == np.uint32 and rows.shape == (len(clip), clip[0].shape[0]) and cols.shape == (len(clip), clip[0].shape[1])
    for i, f in enumerate(clip):
        g = R.gray(f).astype(np.int64)
        assert np.array_equal(rows[i], g.sum(axis=1)) and np.array_equal(cols[i], g.sum(axis=0)), i
    assert (R.sha256(rows[0]), R.sha256(cols[0])) == (gold["analysis"][name]["row_sums_sha256"], gold["analysis"][name]["column_sums_sha256"])


def test_bar_sums_of_frames_at_any_byte_and_of_more_than_a_batch(torch_mod, handler):
    base = CLIPS["edge_found/64x258"] + CLIPS["letterbox/64x258"]
    clip = [base[(5 * i) % len(base)] for i in range(37)]            # two launches
    want = [R.bar_sums(f) for f in clip]
    for offset in (None, 3):
        for _ in range(2):                                            # integer atomics: the same in every run
            rows, cols = handler.bar_sums_device(upload(torch_mod, clip, offset))
            assert all(np.array_equal(rows[i], want[i][0]) and np.array_equal(cols[i], want[i][1]) for i in range(len(clip)))


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_analysis_equals_the_contract(torch_mod, handler, gold, name):
    clip, ref, rec = CLIPS[name], R.AspectHandler(), gold["analysis"][name]
    dev = upload(torch_mod, clip)
    assert R.analysis_record(handler.analyze_frame(dev[0])) == R.analysis_record(ref.analyze_frame(clip[0])) == rec["frame0"]
    assert bars(handler.analyze_frame(t) for t in dev) == rec["bars"]
    calls = []
    assert R.analysis_record(handler.analyze(dev, progress_callback=calls.append)) == R.analysis_record(ref.analyze(clip)) == rec["clip"]
    assert calls and calls[-1] == 1.0
    assert handler.detect_aspect(dev[0]) == rec["detect_aspect"] and handler.detect_letterbox(dev[0]) == rec["detect_letterbox"]


def test_analysis_of_nothing(handler):
    assert handler.analyze([]) == A.AspectAnalysis() and handler.analyze_frame(None) == A.AspectAnalysis()
    assert handler.detect_aspect(None) == 16 / 9 and handler.detect_letterbox(None) is False
    assert handler.crop_letterbox([]) == [] and handler.convert_aspect([], 2.0) == []


# ---- crop -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CLIPS))
@pytest.mark.parametrize("align", R.CROP_ALIGNS)
def test_crop_letterbox_equals_the_contract(torch_mod, gold, name, align):
    clip = CLIPS[name]
    dev = upload(torch_mod, clip)
    h = A.DeviceAspectHandler(A.AspectConfig(align_to=align))
    want = R.AspectHandler(R.AspectConfig(align_to=align)).crop_letterbox(clip)
    digest, shape, same_list = gold["crops"][f"{name}|{align}"]
    if want is not clip and 0 in shape:                              # the deliberate difference: the reference returns empty arrays
        with pytest.raises(ValueError, match="leaves no rows or no columns"):
            h.crop_letterbox(dev)
        return
    got = h.crop_letterbox(dev)
    assert (got is dev) == (want is clip) == same_list
    assert same(host(got), want) and R.digest(host(got)) == digest and all(t.is_contiguous() for t in got)


def test_crop_with_a_given_analysis_and_at_any_byte(torch_mod, handler):
    clip = CLIPS["edge_found/48x64"]
    analysis = R.AspectHandler().analyze(clip)
    want = R.AspectHandler().crop_letterbox(clip, analysis)
    given = handler.analyze(upload(torch_mod, clip))
    for offset in (None, 0, 5):                                       # aligned frames, aligned views, frames that start at an odd byte
        assert same(host(handler.crop_letterbox(upload(torch_mod, clip, offset), given)), want)
    wide = CLIPS["letterbox/48x64"]                                   # whole rows of 192 bytes: the 16-byte path, and its byte twin
    for offset in (None, 5):
        assert same(host(handler.crop_letterbox(upload(torch_mod, wide, offset))), R.AspectHandler().crop_letterbox(wide))
    for flip, view in ((1, lambda f: f[2:9, 3:20][:, ::-1]), (2, lambda f: f[2:9, 3:20][::-1])):
        assert same(host(handler.crop_device(upload(torch_mod, clip), 3, 2, 17, 7, flip=flip)), [view(f) for f in clip])


@pytest.mark.parametrize("name", ["letterbox/37x33", "long/37x33", "long/37x33/gray", "plain/48x64", "edge_found/64x258"])
@pytest.mark.parametrize("block", [1, 2, 5])
def test_stream_equals_the_list_form(torch_mod, handler, name, block):
    clip = CLIPS[name]
    dev = upload(torch_mod, clip)
    whole = handler.crop_letterbox(dev)
    assert same(host(whole), R.AspectHandler().crop_letterbox(clip))
    got = list(handler.stream(iter(dev), block=block))
    assert same(host(got), host(whole))
    if whole is dev:
        assert all(a is b for a, b in zip(got, dev))


def test_long_list_crosses_the_batches(torch_mod, handler):
    base = CLIPS["letterbox/37x33"]
    clip = [base[(3 * i) % 5] for i in range(40)]
    assert same(host(handler.crop_letterbox(upload(torch_mod, clip))), R.AspectHandler().crop_letterbox(clip))


# ---- conversion -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CASES))
def test_convert_aspect_equals_the_contract(torch_mod, gold, key):
    name, (_, method, fill, target) = CASES[key]
    frames = FRAMES[name]
    dev = upload(torch_mod, frames)
    if isinstance(target, R.StandardAspectRatio):
        target_dev = A.StandardAspectRatio(target.value)
    else:
        target_dev = target
    got = device_handler(method, fill).convert_aspect(dev, target_dev)
    want = R.handler_for(method, fill).convert_aspect(frames, target)
    digest, shape, flags = gold["convert"][key]
    assert "".join("01"[a is b] for a, b in zip(got, dev)) == flags                # the input tensors themselves where the reference says so
    assert same(host(got), want) and R.digest(host(got)) == digest and all(t.is_contiguous() for t in got)


def test_pad_at_any_byte_and_pillarbox_letterbox_names(torch_mod):
    frames = FRAMES["48x64"]
    for fill in ("mirror", "color", "blur"):
        for target in (64 / 48 / 1.5, 64 / 48 * 1.5, 64 / 48 / 3.5):
            want = R.handler_for("pad", fill).convert_aspect(frames, target)
            for offset in (None, 7):
                assert same(host(device_handler("pad", fill).convert_aspect(upload(torch_mod, frames, offset), target)), want), (fill, target, offset)
    h = device_handler("crop", "black")                                # PAD whatever the configured method
    assert same(host(h.add_pillarbox(upload(torch_mod, frames), 2.0)), R.AspectHandler().add_pillarbox(frames, 2.0))
    assert same(host(h.add_letterbox(upload(torch_mod, frames), 0.5)), R.AspectHandler().add_letterbox(frames, 0.5))


def test_blur_equals_the_contract(torch_mod, handler):
    for name in ("37x33", "32x8", "2x2", "37x120", "37x33/gray"):     # narrower than 49: the reflection repeats; wider than the kernel
        f = FRAMES[name][0]
        assert np.array_equal(handler.gauss99_device(torch_mod.from_numpy(f).cuda()).cpu().numpy(), R.gaussian_blur_99(f)), name
    assert np.array_equal(A.gauss99_table(), R.gauss99_table())


def test_numpy_forms(handler):
    clip = CLIPS["letterbox/48x64"]
    assert R.analysis_record(handler.analyze_host(clip)) == R.analysis_record(R.AspectHandler().analyze(clip))
    assert same(handler.crop_letterbox_host(clip), R.AspectHandler().crop_letterbox(clip))
    plain = CLIPS["plain/37x33"]
    assert handler.crop_letterbox_host(plain) is plain
    got = handler.convert_aspect_host(plain, 33 / 37)
    assert all(a is b for a, b in zip(got, plain))
    assert same(device_handler("fit", "black").convert_aspect_host(plain, "16:9"), R.handler_for("fit", "black").convert_aspect(plain, "16:9"))
    made = A.create_aspect_handler("4:3", "PAD", "nonsense")
    assert made.config == A.AspectConfig(target_ratio="4:3", method=A.ConversionMethod.PAD) and _lib.owner_device(made).index == 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_entries_answer_invalid_arguments_and_run_nothing(torch_mod, hip_lib):
    torch = torch_mod
    src = [torch.full((16, 16, 3), 7, dtype=torch.uint8, device="cuda") for _ in range(33)]
    dst = [torch.full((32, 32, 3), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(33)]
    sums = torch.full((4 * 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    tmp = torch.full((2 * 16 * 16 * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    table = lambda ts: _lib.ptr_table(ts)                             # noqa: E731
    null_entry = (C.c_void_p * 1)(None)
    col = (C.c_uint8 * 3)(1, 2, 3)
    weights = (C.c_uint16 * 99)(*[int(v) for v in A.gauss99_table()])
    bad_weights = (C.c_uint16 * 99)(*([3] * 99))
    st = _lib.stream_ptr(src[0].device)
    p = _lib.ptr
    L = hip_lib
    bad = [
        L.fw_aspect_bar_sums_u8(None, 1, 16, 16, 3, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(null_entry, 1, 16, 16, 3, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(table(src[:1]), 0, 16, 16, 3, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(table(src), 33, 16, 16, 3, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(table(src[:1]), 1, 16, 16, 2, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(table(src[:1]), 1, 16, 16385, 3, p(sums), p(sums[8192:]), st),
        L.fw_aspect_bar_sums_u8(table(src[:1]), 1, 16, 16, 3, None, p(sums[8192:]), st),
        L.fw_aspect_crop_u8(None, table(dst[:1]), 1, 16, 16, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), None, 1, 16, 16, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 0, 16, 16, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src), table(dst), 33, 16, 16, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 2, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16385, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 9, 0, 8, 8, 0, st),       # a crop outside the frame
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 0, -1, 8, 8, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 0, 0, 8, 0, 0, st),
        L.fw_aspect_crop_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 0, 0, 8, 8, 3, st),
        L.fw_aspect_crop_u8(table(src[:1]), (C.c_void_p * 1)(src[0].data_ptr() + 100), 1, 16, 16, 3, 0, 0, 8, 8, 0, st),   # dst inside src
        L.fw_aspect_crop_u8(table(src[:2]), (C.c_void_p * 2)(dst[0].data_ptr(), dst[0].data_ptr() + 8), 2, 16, 16, 3, 0, 0, 8, 8, 0, st),
        L.fw_aspect_pad_u8(None, table(dst[:1]), 1, 16, 16, 3, 32, 32, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 0, 16, 16, 3, 32, 32, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src), table(dst), 33, 16, 16, 3, 32, 32, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 2, 32, 32, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 16385, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 32, 17, 8, 0, col, None, None, st),   # the source leaves the output
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 32, 8, 8, 3, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 32, 8, 8, 0, None, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 32, 8, 8, 2, col, None, None, st),    # mode 2 without a background
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 4, 4, 3, 4, 32, 14, 0, 1, col, None, None, st),      # a wide bar without its strip
        L.fw_aspect_pad_u8(table(src[:1]), (C.c_void_p * 1)(src[0].data_ptr() + 64), 1, 16, 16, 3, 32, 32, 8, 8, 0, col, None, None, st),
        L.fw_aspect_pad_u8(table(src[:1]), table(dst[:1]), 1, 16, 16, 3, 32, 32, 8, 8, 2, col, table(dst[:1]), None, st),   # dst is its background
        L.fw_aspect_gauss99_u8(None, 16, 16, 3, weights, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16, 3, None, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16, 3, weights, None, p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16, 2, weights, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 0, 16, 3, weights, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16385, 3, weights, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16, 3, bad_weights, p(tmp), p(dst[0]), st),
        L.fw_aspect_gauss99_u8(p(src[0]), 16, 16, 3, weights, p(tmp), p(src[0]), st),
    ]
    assert bad == [_lib.FW_ERR_INVALID] * len(bad)
    assert hip_lib.fw_last_error().decode().startswith("fw_aspect_gauss99_u8: ")
    torch.cuda.synchronize()
    assert all(int(t.min()) == int(t.max()) == SENTINEL for t in dst) and all(int(t.min()) == int(t.max()) == 7 for t in src)
    assert bool((sums == SENTINEL).all()) and bool((tmp == SENTINEL).all())


def test_driver_refusals(torch_mod, handler):
    torch = torch_mod
    clip = CLIPS["letterbox/32x8"]
    dev = upload(torch, clip)
    with pytest.raises(ValueError, match="aligned to 16 leaves no rows or no columns"):
        A.DeviceAspectHandler(A.AspectConfig(align_to=16)).crop_letterbox(dev)
    with pytest.raises(ValueError, match="aspect: uint8 tensors expected"):
        handler.analyze([dev[0].float()])
    with pytest.raises(ValueError, match="aspect: uint8 tensors expected"):
        handler.crop_letterbox([clip[0]])
    with pytest.raises(ValueError, match="of one shape expected"):
        handler.crop_letterbox([dev[0], dev[1][:-1]])
    with pytest.raises(ValueError, match="of one shape expected"):
        handler.convert_aspect([torch.zeros((4, 4, 2), dtype=torch.uint8, device="cuda")], 2.0)
    with pytest.raises(ValueError, match="the handler's device, expected"):
        handler.analyze([dev[0].cpu()])
    with pytest.raises(ValueError, match="unknown conversion method"):
        handler.convert_aspect(dev, 2.0, method="crop")
    odd = A.DeviceAspectHandler()
    odd.config.fill_mode = "mirror"
    with pytest.raises(ValueError, match="unknown fill mode"):
        odd.convert_aspect(dev, 2.0)
    with pytest.raises(ValueError, match="1 .. 16384 pixels a side"):
        handler.analyze_frame(torch.zeros((1, 16385), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="beyond 16384 pixels a side"):
        device_handler("pad", "black").convert_aspect([torch.zeros((4, 9000), dtype=torch.uint8, device="cuda")], 9000 / 4 * 2)
    with pytest.raises(ValueError, match="leaves no rows or no columns"):
        device_handler("crop", "black").convert_aspect(upload(torch, FRAMES["2x2"]), 1 / 3.5)
    with pytest.raises(ValueError, match="leaves no rows or no columns"):
        device_handler("scale", "black").convert_aspect(upload(torch, FRAMES["2x2"]), 1 / 3.5)
    with pytest.raises(ValueError, match="block must be >= 1"):
        list(handler.stream(iter(dev), block=0))
    with pytest.raises(ValueError):
        A.AspectConfig(black_threshold=300)
