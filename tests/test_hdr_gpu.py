"""GPU: `framewright_amd.hdr.DeviceHDRConverter` (csrc/hdr.hip) against tests/hdr_ref.py, tables built on the same host.

Byte equality for every config in which a quantising step is on and the curve is rational, at the smallest shapes at which the kernels
can go wrong - 8 x 8 (one-pixel CLAHE tiles, clip limit 1), 16 x 24, 37 x 53 (both sides padded; odd pixel count, so the frames of a
batch start off a dword), 40 x 53 (one side padded by a full 8), 72 x 136 (tiles 9 x 17), 270 x 480 (several workgroups a tile row) - for
uint8 and uint16 input; float32 bit equality of the planes in front of the first quantisation; the derived rules of DESIGN K20 for the
float path and MOBIUS.  `hdr_ref.content_frame` reaches every branch: random samples, a ramp whose CLAHE tiles clip, pure grays, a block
at the highlight threshold (codes on both sides of 250 / 64225) and all 256 codes."""
import itertools

import numpy as np
import pytest

import hdr_ref as R
from framewright_amd import _lib
from framewright_amd import hdr as H

pytestmark = pytest.mark.gpu
SHAPES = [(8, 8), (16, 24), (37, 53), (40, 53), (72, 136), (270, 480)]
DTYPES = [np.uint8, np.uint16]
RATIONAL = ("reinhard", "aces", "hable")
SWITCHES = [(True, 1.1), (True, 1.0), (False, 1.1)]                                # (local contrast, boost): a quantising step is on
f32 = np.float32


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda().view(
        torch.uint16 if a.dtype == np.uint16 else torch.uint8)


def down(torch, t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


_CONVERTERS = {}


def converter(**fields):
    key = tuple(sorted(fields.items()))
    if key not in _CONVERTERS:
        _CONVERTERS[key] = H.DeviceHDRConverter(H.HDRConfig(**fields))
    return _CONVERTERS[key]


def exact_configs():
    for tm, fmt, cs, (lc, sat), hr in itertools.product(RATIONAL, ("hdr10", "hlg"), ("bt2020", "rec709"), SWITCHES, (True, False)):
        yield dict(tone_mapping=tm, target_format=fmt, color_space=cs, enable_local_contrast=lc, saturation_boost=sat, highlight_recovery=hr)
    for tm, fmt, peak in itertools.product(RATIONAL, ("hdr10", "hlg"), (400, 4000)):
        yield dict(tone_mapping=tm, target_format=fmt, peak_brightness=peak)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_convert_frame_equals_the_restatement(torch_mod, shape, dtype):
    """All 84 exact configs on one frame.  The restatement's planes are computed once per (curve, matrix, peak), its bytes once more per
    switch pair; the device converts the frame anew for every config."""
    frame = R.content_frame(*shape, dtype)
    t_frame = up(torch_mod, frame)
    planes, chains, n = {}, {}, 0
    for fields in exact_configs():
        config = H.HDRConfig(**fields)
        tables = R.build_tables(config)
        pk = (fields["tone_mapping"], fields.get("color_space", "bt2020"), config.peak_brightness)
        if pk not in planes:
            planes[pk] = R.quantise8(R.tone_mapped_plane(frame, config, tables))
        ck = pk + (config.enable_local_contrast, config.saturation_boost)
        if ck not in chains:
            chains[ck] = R.chain_bytes(planes[pk], config)
        want = R.tail_lookup(chains[ck], frame, config, tables)
        got = converter(**fields).convert_frame(t_frame)
        assert got.dtype == torch_mod.uint16 and tuple(got.shape) == frame.shape
        got = down(torch_mod, got)
        assert np.array_equal(got, want), (fields, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
        n += 1
    assert n == 84
    if shape == (37, 53):                                                           # the composed helpers are `convert_frame` itself
        config = H.HDRConfig()
        assert np.array_equal(R.convert_frame(frame, config), R.tail_lookup(chains[("aces", "bt2020", 1000, True, 1.1)], frame, config, R.build_tables(config)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("shape", [(37, 53), (16, 24)], ids=["37x53", "16x24"])
def test_a_batch_equals_frame_by_frame(torch_mod, shape, dtype):
    conv = converter()
    frames = [R.content_frame(*shape, dtype, seed=s) for s in range(3)]
    stack = up(torch_mod, np.stack(frames))                                         # 37 x 53: frames 1 and 2 start off a dword
    tensors = list(stack.unbind(0))
    outs = conv.convert_frames(tensors + [tensors[1]])                              # one tensor twice in the list
    assert len(outs) == 4 and len({o.data_ptr() for o in outs}) == 4
    single = [down(torch_mod, conv.convert_frame(t.clone())) for t in tensors]
    for o, want, frame in zip(outs, single + [single[1]], frames + [frames[1]]):
        assert np.array_equal(down(torch_mod, o), want) and np.array_equal(want, R.convert_frame(frame, conv.config))
    assert [down(torch_mod, o).tobytes() for o in conv.stream(iter(tensors))] == [s.tobytes() for s in single]
    mixed = conv.convert_device([tensors[0], up(torch_mod, R.content_frame(8, 8, dtype)), tensors[2]])         # shapes change inside a list
    assert np.array_equal(down(torch_mod, mixed[1]), R.convert_frame(R.content_frame(8, 8, dtype), conv.config))
    assert np.array_equal(down(torch_mod, mixed[2]), single[2])
    view = up(torch_mod, np.concatenate([frames[0], frames[1]], axis=1))[:, :shape[1]]                          # not contiguous
    assert not view.is_contiguous() and np.array_equal(down(torch_mod, conv.convert_frame(view)), single[0])
    assert np.array_equal(conv.convert_numpy(frames[2]), single[2])
    assert conv.convert_device([]) == []


def test_more_frames_than_one_launch_takes(torch_mod):
    conv = converter(tone_mapping="reinhard")
    frames = [R.content_frame(8, 16, np.uint8, seed=s) for s in range(H.BATCH + 3)]
    outs = conv.convert_device([up(torch_mod, f) for f in frames])
    for k in (0, H.BATCH - 1, H.BATCH, H.BATCH + 2):
        assert np.array_equal(down(torch_mod, outs[k]), R.convert_frame(frames[k], conv.config))


def test_convert_directory_has_the_references_order_counters_and_failure_handling(torch_mod, tmp_path):
    """The image readers and writers are injected (cv2 is absent): the 'png' files here hold np.save's bytes."""
    conv = converter(tone_mapping="reinhard", enable_local_contrast=False)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = {name: R.content_frame(16, 24, np.uint8, seed=i) for i, name in enumerate(("b.png", "a.png", "d.png"))}
    for name, f in frames.items():
        with open(src / name, "wb") as fh:
            np.save(fh, f)
    (src / "c.png").write_bytes(b"")                                                # cannot be read: imread's None
    (src / "e.png").write_bytes(b"not an image")                                    # the reader raises: copied as it is
    with open(src / "z.jpg", "wb") as fh:                                           # ignored: there are PNGs
        np.save(fh, frames["a.png"])
    written, progress = {}, []

    def read(path):
        if path.stat().st_size == 0:
            return None
        with open(path, "rb") as fh:
            return np.load(fh)

    def write(path, array):
        written[path.name] = array

    res = conv.convert_directory(src, dst, progress.append, read=read, write=write)
    assert (res.frames_processed, res.frames_converted, res.frames_skipped, res.failed_frames) == (4, 3, 0, 2) and res.output_dir == dst
    assert (res.max_cll, res.max_fall, res.avg_dynamic_range_stops) == (0, 0, 0.0)   # not measured: analyze_dynamic_range is not built
    assert list(written) == ["a.png", "b.png", "d.png"] and progress == [1 / 5, 2 / 5, 4 / 5, 5 / 5]
    for name, got in written.items():
        assert got.dtype == np.uint16 and np.array_equal(got, R.convert_frame(frames[name], conv.config))
    assert (dst / "e.png").read_bytes() == b"not an image" and not (dst / "c.png").exists()
    only_jpg = tmp_path / "jpg"
    only_jpg.mkdir()
    with open(only_jpg / "k.jpg", "wb") as fh:
        np.save(fh, frames["a.png"])
    written.clear()
    res = conv.convert_directory(only_jpg, tmp_path / "out2", read=read, write=write)
    assert res.frames_converted == 1 and list(written) == ["k.png"]
    empty = tmp_path / "empty"
    empty.mkdir()
    res = conv.convert_directory(empty, tmp_path / "out3", read=read, write=write)
    assert (res.frames_processed, res.frames_converted, res.failed_frames) == (0, 0, 0) and (tmp_path / "out3").is_dir()


# ---- the stages alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("shape", [(37, 53), (72, 136)], ids=["37x53", "72x136"])
def test_tone_mapped_and_quantised_planes_are_bit_equal(torch_mod, shape, dtype):
    frame = R.content_frame(*shape, dtype)
    t_frame = up(torch_mod, frame)
    for tm, cs, peak in itertools.product(RATIONAL, ("bt2020", "rec709", "p3"), (400, 1000, 10000)):
        conv = converter(tone_mapping=tm, color_space=cs, peak_brightness=peak)
        want = R.tone_mapped_plane(frame, conv.config)
        got = down(torch_mod, conv.tone_mapped_plane(t_frame))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tm, cs, peak, int((got != want).sum()))
        assert np.array_equal(down(torch_mod, conv.quantised_plane(t_frame)), R.quantise8(want)), (tm, cs, peak)
        # the highlight step of the float path: times 0.95 where the flag is set
        rec = R.recover_highlights(frame, want, R.build_tables(conv.config))
        assert np.array_equal(down(torch_mod, conv.tone_mapped_plane(t_frame, recover=True)).view(np.uint32), rec.view(np.uint32)), (tm, cs, peak)
        assert (rec != want).any()


@pytest.mark.parametrize("shape", SHAPES + [(9, 8), (8, 15)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_clahe_is_byte_equal_on_given_planes(torch_mod, shape):
    conv = converter()
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    planes = {"random": rng.integers(0, 256, shape).astype(np.uint8),
              "ramp": ((np.arange(w)[None, :] * 255 // max(w - 1, 1)) + np.zeros((h, 1), np.int64)).astype(np.uint8),
              "constant": np.full(shape, 100, np.uint8),
              "narrow": rng.integers(120, 124, shape).astype(np.uint8),
              "L": R.bgr2lab(R.content_frame(h, w))[:, :, 0].copy()}
    for name, plane in planes.items():
        got = down(torch_mod, conv.clahe(up(torch_mod, plane)))
        want = R.clahe(plane)
        assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
    if shape == (16, 24):
        assert (down(torch_mod, conv.clahe(up(torch_mod, planes["constant"]))) == 128).all()     # worked in tests/test_hdr_ref_host.py


def test_the_hsv_step_is_byte_equal_on_given_bytes(torch_mod):
    rng = np.random.default_rng(8)
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    v = np.arange(256, dtype=np.uint8)
    sweeps = [np.stack(p, axis=1) for p in ([v, 255 - v, np.full(256, 255, np.uint8)], [np.full(256, 200, np.uint8), v, 255 - v],
                                            [255 - v, np.full(256, 7, np.uint8), v], [v, v, 255 - v], [v, np.zeros(256, np.uint8), v])]
    pixels = np.concatenate([rng.integers(0, 256, (200001, 3)).astype(np.uint8), gray] + sweeps)        # 4 does not divide the count
    t = up(torch_mod, pixels)
    for boost in (0.8, 0.95, 1.1, 1.25, 1.5):
        got = down(torch_mod, converter().saturate(t, boost))
        want = R.adjust_saturation_u8(pixels[None], boost)[0]
        assert np.array_equal(got, want), (boost, int((got != want).any(axis=1).sum()), pixels[np.argwhere((got != want).any(axis=1))[:3, 0]].tolist())
    frame = R.content_frame(37, 53)
    assert np.array_equal(down(torch_mod, converter(saturation_boost=1.3).saturate(up(torch_mod, frame))), R.adjust_saturation_u8(frame, 1.3))


# ---- the float path: neither quantising step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,peak", [("hdr10", 400), ("hdr10", 1000), ("hdr10", 10000), ("hlg", 1000)])
def test_the_float_path_meets_its_rule(torch_mod, fmt, peak):
    """Steps 1 - 3 and the highlight step are bit-equal (test above, and here through `tone_mapped_plane(recover=True)`); the 16-bit
    output may differ from trunc of the float64 transfer of that float32 plane only within epsilon of an integer, and then by one."""
    for tm, hr, (shape, dtype) in itertools.product(RATIONAL, (True, False), [((37, 53), np.uint8), ((72, 136), np.uint16), ((270, 480), np.uint8)]):
        conv = converter(target_format=fmt, peak_brightness=peak, tone_mapping=tm, highlight_recovery=hr, enable_local_contrast=False, saturation_boost=1.0)
        frame = R.content_frame(*shape, dtype)
        t_frame = up(torch_mod, frame)
        plane = R.tone_mapped_plane(frame, conv.config)
        if hr:
            plane = R.recover_highlights(frame, plane, R.build_tables(conv.config))
        t_plane = conv.tone_mapped_plane(t_frame, recover=hr)
        assert np.array_equal(down(torch_mod, t_plane).view(np.uint32), plane.view(np.uint32))
        got = down(torch_mod, conv.convert_frame(t_frame))
        assert np.array_equal(got, down(torch_mod, conv.transfer(t_plane)))          # the stage alone is the frame path's arithmetic
        bad = R.float_rule_violations(got, plane, conv.config)
        v = R.transfer64(plane, conv.config)
        print(f"{fmt} {peak} {tm} hr={hr} {shape}: {(got != np.floor(v)).sum()} of {got.size} differ from trunc(float64), "
              f"{(got != R.transfer_and_quantise(plane, conv.config)).sum()} from numpy float32; violations {bad}")
        assert bad == 0
    ramp = np.linspace(0, 1, 1 << 16, dtype=f32)                                     # the transfer on a given plane: every region of the curve
    conv = converter(target_format=fmt, peak_brightness=peak, enable_local_contrast=False, saturation_boost=1.0)
    assert R.float_rule_violations(down(torch_mod, conv.transfer(torch_mod.from_numpy(ramp).cuda())), ramp, conv.config) == 0


# ---- MOBIUS -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("peak", [400, 1000, 4000])
def test_mobius_plane_within_its_bound_and_the_chain_behind_it_exact(torch_mod, peak, dtype):
    frame = R.content_frame(72, 136, dtype)
    t_frame = up(torch_mod, frame)
    for cs, (lc, sat), fmt in itertools.product(("bt2020", "rec709"), SWITCHES, ("hdr10", "hlg")):
        conv = converter(tone_mapping="mobius", peak_brightness=peak, color_space=cs, enable_local_contrast=lc, saturation_boost=sat, target_format=fmt)
        plane = down(torch_mod, conv.tone_mapped_plane(t_frame))
        d = R.ulp_distance(plane, R.mobius_plane64(R.linear_plane(frame, conv.config), conv.config))
        assert d.max() <= R.MOBIUS_ULPS, d.max()
        # the whole chain equals the restatement fed with the device's own tone-mapped plane: a one-code flip at the uint8 truncation
        # that a last-bit difference of exp causes is a difference of the planes, not of the chain
        want = R.convert_frame(frame, conv.config, tone_mapped=plane)
        got = down(torch_mod, conv.convert_frame(t_frame))
        assert np.array_equal(got, want), (cs, lc, sat, fmt, int((got != want).sum()))
        host = R.quantise8(R.tone_mapped_plane(frame, conv.config))
        print(f"mobius {peak} {cs}: {d.max():.2f} ulp; {(R.quantise8(plane) != host).sum()} of {host.size} bytes differ from the host's np.exp")
