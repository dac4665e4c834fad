"""GPU: csrc/frame_generation.hip and framewright_amd.frame_generation against tests/frame_generation_ref.py, byte for byte, on
45 x 67, 64 x 96 and 33 x 130 frames (tests/frame_generation_cases.py).  The flows of the warp are inputs here - the device's own
Farneback flows, downloaded, and synthetic ones - as the flow itself is tests/test_flow_gpu.py's subject.  The grain deviation is
compared bit for bit: tests/test_frame_generation_ref_host.py shows on the CPU that no input lies within the reduction's epsilon of
a float32 rounding boundary."""
import ctypes as C

import numpy as np
import pytest

import frame_generation_cases as K
import frame_generation_ref as R
from framewright_amd import _lib
from framewright_amd import frame_generation as FG
from framewright_amd.qp_artifacts import normal_quantiles

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def dev(torch_mod):
    return torch_mod.device("cuda", 0)


def up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def guarded(shape, dev, fill=0xA5):
    """(whole, view): a uint8 destination of ``shape`` with GUARD bytes of ``fill`` on both sides."""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def intact(whole, fill=0xA5):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def device_flows(a, b, dev):
    est = FG.DeviceMissingFrameGenerator()._flow_estimator()
    return tuple(t.cpu().numpy() for t in est.flow_device(up(a, dev), up(b, dev)))


# ---- fw_framegen_warp_blend_u8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", K.SIZES)
def test_warp_blend_equals_the_restatement(hip_lib, dev, h, w):
    import torch
    before, after = K.pair(h, w)
    cases = {name: (f, f) for name, f in K.flows(h, w).items()}
    cases["computed"] = (device_flows(before, after, dev), device_flows(after, before, dev))
    cases["outward_and_constant"] = (K.flows(h, w)["outward"], K.flows(h, w)["constant"])
    tb, ta = up(before, dev), up(after, dev)
    for name, (fwd, bwd) in cases.items():
        planes = [up(p, dev) for p in (*fwd, *bwd)]
        for t in (1 / 3, 0.5, 10 / 11):
            whole, out = guarded((h, w, 3), dev)
            _lib.check(hip_lib.fw_framegen_warp_blend_u8(ptr(tb), ptr(ta), *[ptr(p) for p in planes], h, w, t, ptr(out), stream(dev)))
            torch.cuda.synchronize(dev)
            assert intact(whole), name
            np.testing.assert_array_equal(out.cpu().numpy(), R.warp_blend(before, after, fwd, bwd, t), err_msg=f"{name} t={t}")
    moved = np.abs(cases["computed"][0][0]).max()
    assert moved > 0.5                                           # the computed flow is a flow: the frames are two pixels apart


# ---- fw_framegen_grain_std_u8 ----------------------------------------------------------------------------------------------------
def grain_std(hip_lib, frame, dev):
    import torch
    h, w = frame.shape[:2]
    nb = int(hip_lib.fw_framegen_grain_scratch_bytes(h, w))
    assert nb == ((w + 63) // 64) * ((h + 15) // 16) * 16
    scratch = torch.full((nb + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((3,), -7.0, dtype=torch.float32, device=dev)
    g17 = FG.gaussian17_coeffs()
    _lib.check(hip_lib.fw_framegen_grain_std_u8(ptr(up(frame, dev)), h, w, g17.ctypes.data_as(C.c_void_p), ptr(scratch[GUARD:GUARD + nb]),
                                                ptr(out[1:2]), stream(dev)))
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert got[0] == -7.0 and got[2] == -7.0 and intact(scratch, 0x5A)
    return got[1]


def test_grain_std_equals_the_restatement_bit_for_bit_on_every_run(hip_lib, dev):
    frames = K.statistic_frames()
    for name, frame in frames.items():
        want = R.grain_std(frame)
        got = grain_std(hip_lib, frame, dev)
        print(f"{name}: device {got!r}, contract {want!r} (float64 {R.grain_std64(frame)!r})")
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), name
        assert grain_std(hip_lib, frame, dev).tobytes() == got.tobytes(), name      # fixed order, no atomics: the same bits again
    flat = np.full((33, 130, 3), 77, np.uint8)
    assert 0.0 <= grain_std(hip_lib, flat, dev) < 1e-5 and R.grain_std(flat) < 1e-5   # the blur of a constant is the constant but for rounding


# ---- fw_framegen_finish_u8 -------------------------------------------------------------------------------------------------------
DEVIATIONS = {"add": (7.25, 5.5), "ref_below_cur": (5.5, 7.25), "equal": (6.0, 6.0), "cur_zero": (3.0, 0.0), "small": (1.0000001, 1.0)}
BLENDS = {"none": (None, None), "before": (0.25, None), "after": (None, 2 / 3), "both": (0.5, 0.5)}


@pytest.mark.parametrize("h,w", K.SIZES)
def test_finish_on_explicit_deviations(hip_lib, dev, h, w):
    import torch
    before, after = K.pair(h, w)
    gen = R.generate_interpolated(before, after, 2)[0]
    tb, ta, tg = up(before, dev), up(after, dev), up(gen, dev)
    draws = R.grain_draws(h, w, 11, 1234)
    explicit = np.random.default_rng(h).standard_normal((h, w)) * 3.0
    td, tq = up(explicit, dev), up(normal_quantiles(), dev)
    key = FG.noise_key(11, 1234, FG.TAG_GRAIN)
    for dname, (ref, cur) in DEVIATIONS.items():
        stds = up(np.array([ref, cur], np.float32), dev)
        for bname, (ab, aa) in BLENDS.items():
            for plane, z in ((None, draws), (td, explicit)):
                want = R.finish(gen, ref, cur, z, before, ab, after, aa)
                whole, out = guarded((h, w, 3), dev)
                _lib.check(hip_lib.fw_framegen_finish_u8(ptr(tg), ptr(out), h, w, ptr(stds[0:1]), ptr(stds[1:2]), ptr(plane), ptr(tq), key,
                                                         ptr(tb) if ab is not None else None, ab or 0.0, ptr(ta) if aa is not None else None,
                                                         aa or 0.0, stream(dev)))
                torch.cuda.synchronize(dev)
                assert intact(whole)
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{dname} {bname} {'counter' if plane is None else 'explicit'}")
    assert not np.array_equal(R.finish(gen, 7.25, 5.5, draws, None, None, None, None), gen)
    assert np.array_equal(R.finish(gen, 5.5, 7.25, draws, None, None, None, None), gen)
    # no grain step at all, and in place
    place = tg.clone()
    _lib.check(hip_lib.fw_framegen_finish_u8(ptr(place), ptr(place), h, w, None, None, None, None, 0, ptr(tb), 0.25, ptr(ta), 0.75, stream(dev)))
    np.testing.assert_array_equal(place.cpu().numpy(), R.finish(gen, None, None, None, before, 0.25, after, 0.75))


# ---- fw_framegen_extrapolate_u8 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", K.SIZES)
def test_extrapolate_equals_the_restatement(hip_lib, dev, h, w):
    import torch
    ref, _ = K.pair(h, w)
    ref = ref.copy()
    ref[:3], ref[-3:] = 1, 254                                   # rows that clip on both sides
    tr = up(ref, dev)
    table = up(R.extrapolation_table(), dev)
    explicit = (np.random.default_rng(w).standard_normal((h, w, 3)) * 2.0).astype(np.float32)
    for plane, noise, key in ((None, R.extrapolation_noise(ref.shape, 4, 77), FG.noise_key(4, 77, FG.TAG_EXTRAPOLATE)), (up(explicit, dev), explicit, 0)):
        whole, out = guarded((h, w, 3), dev)
        _lib.check(hip_lib.fw_framegen_extrapolate_u8(ptr(tr), ptr(out), h, w, ptr(plane), ptr(table), key, stream(dev)))
        torch.cuda.synchronize(dev)
        assert intact(whole)
        np.testing.assert_array_equal(out.cpu().numpy(), R.extrapolate_frame(ref, noise))


# ---- misuse ----------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_a_message(hip_lib, dev):
    import torch
    h, w = 20, 24
    f = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(3)]
    fl = [torch.zeros((h, w), dtype=torch.float32, device=dev) for _ in range(4)]
    big = torch.zeros(2 * h * w * 3, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(64, dtype=torch.uint8, device=dev)
    stds = torch.ones(2, dtype=torch.float32, device=dev)
    q = torch.zeros(65536, dtype=torch.float64, device=dev)
    g17 = FG.gaussian17_coeffs().ctypes.data_as(C.c_void_p)
    st, P = stream(dev), ptr
    lib = hip_lib

    def refused(status, *words):
        assert status == _lib.FW_ERR_INVALID
        message = lib.fw_last_error().decode()
        assert all(word in message for word in words), message

    warp = lambda **k: lib.fw_framegen_warp_blend_u8(k.get("before", P(f[0])), k.get("after", P(f[1])), k.get("fx", P(fl[0])), P(fl[1]), P(fl[2]),   # noqa: E731
                                                     k.get("by", P(fl[3])), k.get("h", h), k.get("w", w), k.get("t", 0.5), k.get("out", P(f[2])), st)
    assert warp() == _lib.FW_OK
    refused(warp(before=None), "fw_framegen_warp_blend_u8", "null pointer")
    refused(warp(by=None), "null pointer")
    refused(warp(out=None), "null pointer")
    for t in (0.0, 1.0, -0.25, 1.5, float("nan")):
        refused(warp(t=t), "t in (0, 1)")
    refused(warp(h=0), "pixels a side")
    refused(warp(w=16385), "pixels a side")
    refused(warp(out=P(f[0])), "out overlaps a frame")
    refused(warp(before=P(big), out=C.c_void_p(big.data_ptr() + h * w * 3 - 1)), "out overlaps a frame")
    refused(warp(fx=C.c_void_p(fl[0].data_ptr() + 2)), "4-byte aligned")

    std = lambda **k: lib.fw_framegen_grain_std_u8(k.get("frame", P(f[0])), k.get("h", h), k.get("w", w), k.get("g", g17), k.get("scratch", P(scratch)),   # noqa: E731
                                                   k.get("out", P(stds)), st)
    assert std() == _lib.FW_OK
    refused(std(frame=None), "fw_framegen_grain_std_u8", "null pointer")
    refused(std(g=None), "null pointer")
    refused(std(scratch=None), "null pointer")
    refused(std(h=15), "16 .. 16384")
    refused(std(w=15), "16 .. 16384")
    refused(std(scratch=C.c_void_p(scratch.data_ptr() + 4)), "8-byte aligned")
    assert lib.fw_framegen_grain_scratch_bytes(15, 64) == 0 and lib.fw_framegen_grain_scratch_bytes(64, 16385) == 0
    assert lib.fw_framegen_grain_scratch_bytes(16, 16) == 16

    fin = lambda **k: lib.fw_framegen_finish_u8(k.get("gen", P(f[0])), k.get("out", P(f[2])), h, k.get("w", w), k.get("ref", P(stds[0:1])),   # noqa: E731
                                                k.get("cur", P(stds[1:2])), None, k.get("q", P(q)), 0, k.get("before", P(f[1])), k.get("ab", 0.5),
                                                k.get("after", None), k.get("aa", 0.0), st)
    assert fin() == _lib.FW_OK and fin(out=P(f[0])) == _lib.FW_OK          # in place
    refused(fin(gen=None), "fw_framegen_finish_u8", "null pointer")
    refused(fin(cur=None), "both deviations or neither")
    refused(fin(q=None), "null pointer")
    refused(fin(ab=float("inf")), "finite alpha")
    refused(fin(after=P(f[1]), aa=float("nan")), "finite alpha")
    assert fin(before=None, ab=float("nan")) == _lib.FW_OK                  # no blend due: its alpha is not read
    refused(fin(out=P(f[1])), "out overlaps a frame")
    refused(fin(gen=P(big), out=C.c_void_p(big.data_ptr() + 5)), "out overlaps a frame")
    refused(fin(w=0), "pixels a side")

    ext = lambda **k: lib.fw_framegen_extrapolate_u8(k.get("ref", P(f[0])), k.get("out", P(f[2])), h, w, k.get("noise", None), k.get("table", P(q)), 0, st)   # noqa: E731
    assert ext() == _lib.FW_OK
    refused(ext(ref=None), "fw_framegen_extrapolate_u8", "null pointer")
    refused(ext(table=None), "null pointer")
    refused(ext(out=P(f[0])), "out overlaps reference")
    torch.cuda.synchronize(dev)


# ---- the drivers -----------------------------------------------------------------------------------------------------------------
def config_args(cfg):
    return dict(backend=FG.DeviceMissingFrameGenerator(cfg)._backend, max_gap_frames=cfg.max_gap_frames, match_grain=cfg.match_grain,
                blend_edges_n=cfg.blend_edges, seed=cfg.seed or 0)


@pytest.mark.parametrize("grain,blend", [(True, 3), (False, 1), (True, 0)])
def test_fill_device_stream_and_fill_equal_the_restatements_driver(torch_mod, dev, grain, blend):
    clip = K.clip()
    cfg = FG.FrameGenerationConfig(match_grain=grain, blend_edges=blend, seed=K.SEED)
    gen = FG.DeviceMissingFrameGenerator(cfg)
    want, want_numbers = R.fill(clip, K.CLIP_NUMBERS, K.CLIP_EXPECTED, **config_args(cfg))
    assert want_numbers == list(range(10))
    tensors = [up(f, dev) for f in clip]
    got, numbers = gen.fill_device(tensors, K.CLIP_NUMBERS, K.CLIP_EXPECTED)
    assert numbers == want_numbers
    for n, g, w_ in zip(numbers, got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg=f"frame {n}")
    # the inputs are in the result as they are, and the generated frames are views of one allocation
    assert all(got[n] is t for n, t in zip(K.CLIP_NUMBERS, tensors))
    made = [got[n] for n in range(10) if n not in K.CLIP_NUMBERS]
    base = made[0].data_ptr()
    assert [m.data_ptr() - base for m in made] == [i * made[0].numel() for i in range(len(made))]
    assert len({m.untyped_storage().data_ptr() for m in made}) == 1
    streamed = list(gen.stream(zip(K.CLIP_NUMBERS, tensors), K.CLIP_EXPECTED))
    assert [n for n, _ in streamed] == want_numbers
    for (n, g), w_ in zip(streamed, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg=f"stream frame {n}")
    host, host_numbers = gen.fill(clip, K.CLIP_NUMBERS, K.CLIP_EXPECTED)
    assert host_numbers == want_numbers and all(np.array_equal(a, b) for a, b in zip(host, want))
    # no expected count: no end gap; a gap above max_gap_frames stays; nothing to fill returns the inputs
    short, short_numbers = gen.fill_device(tensors, K.CLIP_NUMBERS)
    assert short_numbers == list(range(8))
    tight = FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(max_gap_frames=1, match_grain=grain, blend_edges=blend, seed=K.SEED))
    assert tight.fill_device(tensors, K.CLIP_NUMBERS)[1] == [0, 1, 4, 5, 6, 7]
    same, same_numbers = gen.fill_device(tensors[:2], [0, 1])
    assert same_numbers == [0, 1] and same[0] is tensors[0]
    with pytest.raises(ValueError, match="strictly rising"):
        gen.fill_device(tensors[:2], [3, 3])
    gen.close()
    with pytest.raises(ValueError, match="closed"):
        gen.fill_device(tensors, K.CLIP_NUMBERS)


def test_optical_flow_driver_equals_the_restatement_on_the_devices_flows(torch_mod, dev):
    clip = K.clip()
    cfg = FG.FrameGenerationConfig(model="optical_flow", seed=K.SEED)
    gen = FG.DeviceMissingFrameGenerator(cfg)
    assert gen._backend == "optical_flow"
    flow = lambda a, b: device_flows(a, b, dev)                  # noqa: E731
    want, want_numbers = R.fill(clip, K.CLIP_NUMBERS, K.CLIP_EXPECTED, flow=flow, **config_args(cfg))
    # the standard-deviation rule for the warped frames, which exist only with the device's flows: checked on the CPU, here
    frames = dict(zip(K.CLIP_NUMBERS, clip))
    for start, end, size, has_after in R.gaps_from_numbers(K.CLIP_NUMBERS, K.CLIP_EXPECTED):
        if has_after:
            for g in R.generate_optical_flow(frames[start], frames[end], size, flow):
                eps = R.std_epsilon(R.grain_plane(g))
                a, b = R.grain_std64(frames[start]), R.grain_std64(g)
                assert R.clear_of_rounding_boundary(b, eps) and abs(a - b) > eps * (a + b)
    got, numbers = gen.fill_device([up(f, dev) for f in clip], K.CLIP_NUMBERS, K.CLIP_EXPECTED)
    assert numbers == want_numbers
    for n, g, w_ in zip(numbers, got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg=f"frame {n}")
    blended = R.fill(clip, K.CLIP_NUMBERS, K.CLIP_EXPECTED, **{**config_args(cfg), "backend": R.INTERPOLATE})[0]
    assert not np.array_equal(want[2], blended[2])               # the warp is not the blend


def test_generate_missing_writes_what_the_restatement_generates(torch_mod, dev, tmp_path):
    clip = dict(zip(K.CLIP_NUMBERS, K.clip()))
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for n in clip:
        (src / f"frame_{n:08d}.png").write_bytes(b"%d" % n)
    (src / "frame_00000007.png").unlink()                        # the gap behind 5 loses its after frame
    (src / "notes.jpg").write_bytes(b"")
    written, progress = {}, []
    read = lambda path: clip[FG.parse_frame_number(path.name)].copy()      # noqa: E731
    cfg = FG.FrameGenerationConfig(seed=K.SEED)
    gen = FG.DeviceMissingFrameGenerator(cfg)
    gaps = gen.detect_gaps(src, expected_count=8)
    assert [(g.start_frame, g.end_frame, g.gap_size) for g in gaps] == [(1, 4, 2), (5, 7, 2)] and gaps[1].after_path is None
    gaps.append(FG.GapInfo(20, 23, 2, None, src / "frame_00000004.png"))             # no before frame: backward extrapolation
    gaps.append(FG.GapInfo(30, 32, 1, None, None))                                   # no boundary at all: failed
    res = gen.generate_missing(src, dst, gaps, progress.append, read_image=read, write_image=lambda p, a: written.__setitem__(p.name, a))
    assert (res.frames_generated, res.frames_failed, res.gaps_processed, res.output_dir) == (6, 1, 3, dst)
    assert progress == [2 / 7, 4 / 7, 6 / 7]                    # the reference's `continue` skips the report of a gap without boundaries
    assert sorted(p.name for p in dst.iterdir()) == sorted(p.name for p in src.iterdir())
    args = config_args(cfg)
    args.pop("max_gap_frames")
    want = {2: R.fill_gap(clip[1], clip[4], 1, 2, **args), 6: R.fill_gap(clip[5], None, 5, 2, **args), 21: R.fill_gap(None, clip[4], 20, 2, **args)}
    assert sorted(written) == [f"frame_{n:08d}.png" for n in (2, 3, 6, 7, 21, 22)]
    for first, frames in want.items():
        for i, f in enumerate(frames):
            np.testing.assert_array_equal(written[f"frame_{first + i:08d}.png"], f, err_msg=f"frame {first + i}")
