"""GPU: csrc/deinterlace.hip and framewright_amd/deinterlace.py against the contract in tests/deinterlace_ref.py and the results
recorded from the reference (tests/golden/deinterlace_reference.json).  Every comparison is exact equality."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import deinterlace_ref as R
from framewright_amd import _lib
from framewright_amd import deinterlace as D

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 16, 17]
WIDTHS = [1, 2, 3, 5, 7, 16, 33, 85]
LENGTHS = [1, 2, 5]
SENTINEL = 0xA5
PAD = 64
MODES = {"yadif": D.FW_DEINTERLACE_YADIF, "bwdif": D.FW_DEINTERLACE_BWDIF, "bob": D.FW_DEINTERLACE_BOB}


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "deinterlace_reference.json").read_text())


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def deint(torch_mod):
    return D.DeviceDeinterlacer(D.InterlaceConfig(field_order=D.FieldOrder.TFF))


def views_at(torch, host: np.ndarray, offset: int, fill=None):
    """The n frames of ``host`` (n x H x W [x 3]) as views that start ``offset`` bytes into a padded allocation (the allocation
    itself is 256-byte aligned); with ``fill`` the buffer holds that byte everywhere instead of the frames."""
    flat = np.full(host.size + 2 * PAD, SENTINEL if fill is None else fill, np.uint8)
    if fill is None:
        flat[PAD + offset: PAD + offset + host.size] = host.reshape(-1)
    buf = torch.from_numpy(flat).cuda()
    clip = buf[PAD + offset: PAD + offset + host.size].view(host.shape)
    return buf, list(clip.unbind(0))


def reference(clip, mode, parity):
    if mode == "yadif":
        return R.yadif(clip, parity)
    if mode == "bwdif":
        return R.bwdif(clip, parity)
    return [R.bob_field(f, parity) for f in clip]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("mode", ["yadif", "bwdif", "bob"])
def test_frames_equal_the_contract(torch_mod, deint, mode, c):
    """The full cross: every height x width, both parities, lists of 1, 2 and 5, sources at byte offsets 0 .. 3 with the
    destination aligned alike and, at offset 2, differently, the batched and the single entry.  The padded destination is compared
    whole: the bytes around the frames stay as they were."""
    torch = torch_mod
    rng = np.random.default_rng(7 + c)
    runs = []
    for h in HEIGHTS:
        if mode == "bob" and h < 2:
            continue
        for w in WIDTHS:
            for parity in (0, 1):
                for n in LENGTHS:
                    host = rng.integers(0, 256, size=(n, h, w) + ((3,) if c == 3 else ()), dtype=np.uint8)
                    host[:, :, : max(1, w // 3)] = 255                                       # BWDIF's clamp at the top
                    want = np.stack(reference(list(host), mode, parity)).reshape(-1)
                    for off in (0, 1, 2, 3):
                        _, src = views_at(torch, host, off)
                        for dst_off in ((off, 0) if off == 2 else (off,)):
                            exp = np.full(host.size + 2 * PAD, SENTINEL, np.uint8)
                            exp[PAD + dst_off: PAD + dst_off + host.size] = want
                            for batched in (True, False):
                                buf, outs = views_at(torch, host, dst_off, fill=SENTINEL)
                                deint.interpolate_device(src, MODES[mode], parity, batched=batched, outs=outs)
                                runs.append((buf, exp, (h, w, parity, off, dst_off, n, batched)))
    torch.cuda.synchronize()
    for buf, exp, what in runs:
        np.testing.assert_array_equal(buf.cpu().numpy(), exp, err_msg=str(what))


def test_list_entry_allocates_and_equals_the_contract(torch_mod, gold):
    """`deinterlace` on the recorded clips: every method and order, outputs equal to the reference's digests; WEAVE returns its
    input list; NEURAL equals BWDIF; an unknown method is YADIF."""
    torch = torch_mod
    for name in ("9x16x3", "17x33x1", "5x3x1", "6x7x3"):
        clip = R.frame_clips()[name]
        dev = [torch.from_numpy(f).cuda() for f in clip]
        for order in ("tff", "bff"):
            d = D.create_deinterlacer("yadif", order)
            for m in ("yadif", "bwdif", "bob"):
                out = d.deinterlace(dev, D.DeinterlaceMethod(m))
                assert [R.sha256(t.cpu().numpy()) for t in out] == gold["frames"][f"{name}/{order}/{m}"], (name, order, m)
            assert d.deinterlace(dev, D.DeinterlaceMethod.WEAVE) is dev
            neural = d.deinterlace(dev, D.DeinterlaceMethod.NEURAL)
            assert [R.sha256(t.cpu().numpy()) for t in neural] == gold["frames"][f"{name}/{order}/bwdif"]
            assert [R.sha256(t.cpu().numpy()) for t in d.deinterlace(dev, "no such method")] == gold["frames"][f"{name}/{order}/yadif"]
    assert D.create_deinterlacer("nonsense", "nonsense").config == D.InterlaceConfig()
    assert D.DeinterlaceMethod.BOB.doubles_framerate and D.DeinterlaceMethod.NNEDI.requires_neural
    with pytest.raises(ValueError):
        D.InterlaceConfig(comb_threshold=1.5)


def test_stream_equals_the_list_call(torch_mod):
    torch = torch_mod
    clip = [torch.from_numpy(f).cuda() for f in R.noise_clip(7, 9, 16, 3, 5)]
    for m in (D.DeinterlaceMethod.BWDIF, D.DeinterlaceMethod.YADIF, D.DeinterlaceMethod.BOB, D.DeinterlaceMethod.WEAVE):
        d = D.DeviceDeinterlacer(D.InterlaceConfig(method=m, field_order=D.FieldOrder.BFF))
        whole = d.deinterlace(clip)
        for block in (1, 2, 3, 7, 8):
            got = list(d.stream(iter(clip), block=block))
            assert len(got) == len(whole) and all(torch.equal(a, b) for a, b in zip(got, whole)), (m, block)
    with pytest.raises(ValueError):
        list(D.DeviceDeinterlacer(D.InterlaceConfig()).stream(iter(clip)))


def test_views_and_foreign_neighbours(torch_mod, deint):
    """Non-contiguous frames (the BGR part of BGRA buffers, a column slice of gray ones) give the bytes of their contiguous copies,
    in `deinterlace`, in `stream` across block borders and as ``prev`` / ``nxt``; a neighbour or a streamed frame of another
    shape, dtype or kind is refused before anything is launched."""
    torch = torch_mod
    rng = np.random.default_rng(3)
    for shape, cut in (((7, 9, 12, 4), lambda t: t[..., :3]), ((7, 9, 20), lambda t: t[..., 2:18])):
        host = rng.integers(0, 256, size=shape, dtype=np.uint8)
        views = list(cut(torch.from_numpy(host).cuda()).unbind(0))
        assert not views[0].is_contiguous()
        want = R.bwdif([np.ascontiguousarray(f) for f in cut(host)], 0)
        d = D.DeviceDeinterlacer(D.InterlaceConfig(method=D.DeinterlaceMethod.BWDIF, field_order=D.FieldOrder.BFF))
        whole = d.deinterlace(views)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(whole, want))
        for block in (1, 2, 3):
            got = list(d.stream(iter(views), block=block))
            assert len(got) == len(want) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), block
        mid = deint.interpolate_device(views[2:5], D.FW_DEINTERLACE_BWDIF, 0, prev=views[1], nxt=views[5])
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(mid, want[2:5]))
    a = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
    foreign = [torch.zeros((8, 12), dtype=torch.uint8, device="cuda"), torch.zeros((8, 16), dtype=torch.int16, device="cuda"),
               torch.zeros((8, 16, 3), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1), dtype=torch.uint8, device="cuda").expand(4, 16),
               torch.zeros((8, 16), dtype=torch.uint8), np.zeros((8, 16), np.uint8)]
    for bad in foreign:
        with pytest.raises(ValueError):
            deint.interpolate_device([a], D.FW_DEINTERLACE_BWDIF, 1, prev=bad)
        with pytest.raises(ValueError):
            deint.interpolate_device([a], D.FW_DEINTERLACE_BWDIF, 1, nxt=bad)
        with pytest.raises(ValueError):
            list(D.DeviceDeinterlacer(D.InterlaceConfig(method=D.DeinterlaceMethod.BWDIF, field_order=D.FieldOrder.TFF)).stream(iter([a, a, bad]), block=2))
    zero_stride = torch.zeros((1, 16), dtype=torch.uint8, device="cuda").expand(8, 16)           # right shape, 16 bytes of storage
    out = deint.interpolate_device([a], D.FW_DEINTERLACE_BWDIF, 1, prev=zero_stride, nxt=zero_stride)
    assert int(out[0].max()) == 0


def test_overlapping_destination_is_refused(torch_mod, deint, hip_lib):
    torch = torch_mod
    buf = torch.zeros(6 * 8 * 16, dtype=torch.uint8, device="cuda")
    a = buf[: 8 * 16].view(8, 16)
    b = buf[8: 8 + 8 * 16].view(8, 16)                      # shares all but 8 bytes with a
    far = buf[2 * 8 * 16: 3 * 8 * 16].view(8, 16)
    with pytest.raises(ValueError):
        deint.interpolate_device([a], D.FW_DEINTERLACE_BWDIF, 1, outs=[b])
    with pytest.raises(ValueError):
        deint.interpolate_device([a], D.FW_DEINTERLACE_YADIF, 1, outs=[a])
    with pytest.raises(ValueError):
        deint.interpolate_device([a], D.FW_DEINTERLACE_BWDIF, 1, nxt=far, outs=[far])
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    for cur, prev, nxt, dst, mode in ((a, a, a, a, 0), (a, a, a, b, 1), (a, far, a, far, 1), (a, a, far, far, 1)):
        assert hip_lib.fw_deinterlace_u8(p(cur), p(prev), p(nxt), p(dst), 8, 16, mode, 1, None) == _lib.FW_ERR_INVALID
        assert b"overlaps" in hip_lib.fw_last_error()
    # a destination that overlaps a source of ANOTHER frame of the call
    c, c8 = buf[3 * 8 * 16: 4 * 8 * 16].view(8, 16), buf[8 + 3 * 8 * 16: 8 + 4 * 8 * 16].view(8, 16)
    e = buf[5 * 8 * 16: 6 * 8 * 16].view(8, 16)
    for entries, mode, want in ((((a, a, a, far), (far, far, far, c)), 0, _lib.FW_ERR_INVALID),       # dst 0 is cur 1
                                (((a, a, a, c), (far, c8, far, e)), 1, _lib.FW_ERR_INVALID),           # dst 0 overlaps prev 1
                                (((a, a, a, c), (far, far, c8, e)), 1, _lib.FW_ERR_INVALID),           # dst 0 overlaps next 1
                                (((far, far, c8, e), (a, a, a, c)), 1, _lib.FW_ERR_INVALID),           # dst 1 overlaps next 0
                                (((a, a, a, c), (far, a, far, e)), 1, _lib.FW_OK)):                    # apart: runs
        table = (C.c_void_p * 8)(*[t.data_ptr() for entry in entries for t in entry])
        assert hip_lib.fw_deinterlace_batch_u8(table, 2, 8, 16, mode, 1, None) == want, (mode, want)
    torch.cuda.synchronize()
    assert int(buf.max()) == 0


def test_c_entries_reject_bad_arguments_without_a_launch(torch_mod, hip_lib):
    torch = torch_mod
    src = torch.full((8 * 16,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8 * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    st64 = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    s, d, null = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), None
    one = hip_lib.fw_deinterlace_u8
    bad = [one(null, s, s, d, 8, 16, 0, 1, None), one(s, s, s, null, 8, 16, 0, 1, None), one(s, null, s, d, 8, 16, 1, 1, None),
           one(s, s, null, d, 8, 16, 1, 1, None), one(s, s, s, d, 0, 16, 0, 1, None), one(s, s, s, d, 8, 0, 0, 1, None),
           one(s, s, s, d, 8, 16, 3, 1, None), one(s, s, s, d, 8, 16, -1, 1, None), one(s, s, s, d, 8, 16, 0, 2, None),
           one(s, s, s, d, 8, 16, 0, -1, None), one(s, s, s, d, 1, 16, 2, 0, None)]
    table = (C.c_void_p * 4)(src.data_ptr(), src.data_ptr(), src.data_ptr(), dst.data_ptr())
    nulled = (C.c_void_p * 4)(src.data_ptr(), src.data_ptr(), src.data_ptr(), None)
    batch = hip_lib.fw_deinterlace_batch_u8
    bad += [batch(None, 1, 8, 16, 0, 1, None), batch(table, 0, 8, 16, 0, 1, None), batch(nulled, 1, 8, 16, 0, 1, None),
            batch(table, 1, 0, 16, 0, 1, None), batch(table, 1, 8, 0, 0, 1, None), batch(table, 1, 8, 16, 5, 1, None),
            batch(table, 1, 8, 16, 0, 7, None), batch(table, 1, 1, 16, 2, 1, None)]
    frames = (C.c_void_p * 1)(src.data_ptr())
    none1 = (C.c_void_p * 1)(None)
    o = C.c_void_p(st64.data_ptr())
    stats, pair = hip_lib.fw_interlace_stats_u8, hip_lib.fw_frame_absdiff_sum_u8
    bad += [stats(None, 1, 8, 16, 1, o, None), stats(frames, 1, 8, 16, 1, None, None), stats(none1, 1, 8, 16, 1, o, None),
            stats(frames, 0, 8, 16, 1, o, None), stats(frames, 1, 0, 16, 1, o, None), stats(frames, 1, 8, 0, 1, o, None),
            stats(frames, 1, 8, 16, 2, o, None), pair(None, frames, 1, 8, 16, 1, o, None), pair(frames, None, 1, 8, 16, 1, o, None),
            pair(frames, none1, 1, 8, 16, 1, o, None), pair(frames, frames, 1, 8, 16, 4, o, None), pair(frames, frames, 1, 8, 16, 1, None, None)]
    assert bad == [_lib.FW_ERR_INVALID] * len(bad)
    torch.cuda.synchronize()
    assert int(dst.min()) == SENTINEL == int(dst.max()) and int(st64.max()) == -1 == int(st64.min())
    # YADIF and BOB do not read prev and next
    assert one(s, null, null, d, 8, 16, 0, 1, None) == _lib.FW_OK and one(s, null, null, d, 8, 16, 2, 1, None) == _lib.FW_OK
    torch.cuda.synchronize()


def stat_frames(h, w, c):
    rng = np.random.default_rng(h * 100 + w + c)
    shape = (h, w) if c == 1 else (h, w, 3)
    alt = np.zeros(shape, np.uint8)
    alt[1::2] = 255
    return [rng.integers(0, 256, size=shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8), alt,
            rng.integers(100, 140, size=shape, dtype=np.uint8)]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w", [(4, 1), (5, 3), (16, 33), (17, 85), (64, 48)])
def test_statistics_are_the_exact_integers(torch_mod, deint, h, w, c):
    torch = torch_mod
    host = stat_frames(h, w, c)
    dev = [torch.from_numpy(f).cuda() for f in host]
    got = deint.stats_device(dev).cpu().numpy()
    assert got.dtype == np.int64
    want = np.array([R.stats(f) for f in host], np.int64)
    np.testing.assert_array_equal(got, want)
    assert want[3, 0] == h // 2 and want[1].sum() == 0 and want[2].sum() == 0          # alternating rows: every pair combs
    np.testing.assert_array_equal(deint.stats_device(dev).cpu().numpy(), got)          # the same int64s in a second run
    one = np.concatenate([deint.stats_device([f]).cpu().numpy() for f in dev])         # one frame alone, as in the batch
    np.testing.assert_array_equal(one, got)
    a, b = dev, dev[1:] + dev[:1]
    pairs = deint.pair_sums_device(a, b).cpu().numpy()
    np.testing.assert_array_equal(pairs, np.array([R.pair_sum(x, y) for x, y in zip(host, host[1:] + host[:1])], np.int64))
    np.testing.assert_array_equal(deint.pair_sums_device(a, b).cpu().numpy(), pairs)


def test_more_frames_than_one_launch_holds(torch_mod, deint):
    """40 frames: two launches of the 32-frame argument block."""
    torch = torch_mod
    host = R.noise_clip(40, 6, 7, 3, 9)
    dev = [torch.from_numpy(f).cuda() for f in host]
    out = deint.interpolate_device(dev, D.FW_DEINTERLACE_BWDIF, 0)
    for g, w in zip(out, R.bwdif(host, 0)):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    np.testing.assert_array_equal(deint.stats_device(dev).cpu().numpy(), np.array([R.stats(f) for f in host], np.int64))
    np.testing.assert_array_equal(deint.pair_sums_device(dev[:-1], dev[1:]).cpu().numpy(),
                                  np.array([R.pair_sum(a, b) for a, b in zip(host[:-1], host[1:])], np.int64))


def test_analysis_equals_the_recorded_reference(torch_mod, gold):
    torch = torch_mod
    clips = R.analysis_clips()
    for name, clip in clips.items():
        rec = gold["analysis"][name]
        dev = [torch.from_numpy(f).cuda() for f in clip]
        d = D.DeviceDeinterlacer(D.InterlaceConfig(method=D.DeinterlaceMethod.BWDIF))
        a = d.analyze(dev)
        want = R.analyze(clip)
        for k in ("is_interlaced", "confidence", "combing_percentage", "progressive_percentage", "tff_percentage", "bff_percentage"):
            assert getattr(a, k) == rec["analyze"][k] == getattr(want, k), (name, k)
        for k in ("field_order", "telecine_pattern", "recommended_method"):
            assert getattr(a, k).value == rec["analyze"][k], (name, k)
        assert a.details == want.details                                               # the variance from the same exact means
        assert d.detect_interlacing(dev) == rec["analyze"]["is_interlaced"] and d.detect_field_order(dev).value == rec["analyze"]["field_order"]
        assert isinstance(a.summary(), str)
        assert d.detect_telecine(dev).value == rec["detect_telecine"]
        kept = d.inverse_telecine(dev)
        assert [next(i for i, f in enumerate(dev) if f is k) for k in kept] == rec["inverse_telecine"]
        forced = d.inverse_telecine(dev, D.TelecinePattern.PATTERN_3_2)
        assert [next(i for i, f in enumerate(dev) if f is k) for k in forced] == rec["inverse_telecine_3_2"]
        order = d.resolve_field_order(dev)
        assert order.value == (rec["auto_order"] if rec["auto_order"] != "unknown" else "tff")
        assert [R.sha256(t.cpu().numpy()) for t in d.deinterlace(dev)] == rec["auto_bwdif_sha256"]       # AUTO, as recorded
    with pytest.raises(ValueError):
        D.DeviceDeinterlacer().analyze([torch.zeros((3, 8), dtype=torch.uint8, device="cuda")])
    assert D.DeviceDeinterlacer().analyze([]).is_interlaced is False
