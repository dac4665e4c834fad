"""GPU: csrc/qp_artifacts.hip and `framewright_amd.qp_artifacts` against tests/qp_artifact_ref.py - byte for byte, no tolerance anywhere.

Shapes: 1 x 1, 3 x 5 (smaller than every radius: the border reflects several times), 17 x 23, 33 x 70 and 40 x 72 (both cross the
bilateral's 32 x 16 tiles and the 32-pixel hysteresis tiles and are no multiple of 8).  Contents: seeded random frames, hard 8 x 8 blocks,
a serpentine of weak edges attached to one strong spot that winds through all six hysteresis tiles of the 40 x 72 frame, a smooth ramp.
qp 18, 28 and 40 at multiplier 1 give the bilateral d = 6, 8 and 12 (radius 3, 4 and 6); the bilateral's own entry is also run at
d = 7, 11 and 15 (radius 3, 5 and 7) and at the smallest radii.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import qp_artifact_ref as R
from framewright_amd import _lib
from framewright_amd import qp_artifacts as Q

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 5), (17, 23), (33, 70), (40, 72)]
QPS = (18, 28, 40)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


# ---- contents ------------------------------------------------------------------------------------------------------------------------
def random_frame(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def block_frame(h, w):
    y, x = np.mgrid[0:h, 0:w]
    v = (x // 8 * 53 + y // 8 * 101) % 200 + 20
    return np.stack([v, (v + 40) % 256, 255 - v], axis=2).astype(np.uint8)


def ramp_frame(h, w):
    y, x = np.mgrid[0:h, 0:w]
    v = 30 + x + y
    return np.stack([v, v + 10, v + 20], axis=2).astype(np.uint8)


def serpentine_frame(h=40, w=72, strong=True):
    """A band 20 gray levels above the ground (Sobel magnitude 80: between the thresholds 50 and 150) that winds from the top left to
    the bottom; its outline is one connected chain of weak edge pixels.  Only the 3 x 3 spot at its start is above the high threshold."""
    g = np.full((h, w), 100, np.int32)
    tops = list(range(4, h - 5, 10))
    for i, y in enumerate(tops):
        g[y:y + 4, 4:w - 4] = 120
        if i + 1 < len(tops):
            if i % 2 == 0:
                g[y:tops[i + 1] + 4, w - 8:w - 4] = 120
            else:
                g[y:tops[i + 1] + 4, 4:8] = 120
    if strong:
        g[3:6, 2:5] = 250
    return np.repeat(g.astype(np.uint8)[:, :, None], 3, axis=2)


CONTENT = {"random": random_frame, "blocks": block_frame, "ramp": ramp_frame, "serpentine": serpentine_frame}


@functools.lru_cache(maxsize=None)
def frame_of(content, shape):
    f = CONTENT[content](*shape)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def noise_plane(shape, seed=0):
    n = (np.random.default_rng(77 + seed).standard_normal(shape + (3,)) * 3).astype(np.float32)
    n.setflags(write=False)
    return n


class Cfg:
    def __init__(self, types, block_size=8, multiplier=1.0):
        self.artifact_types, self.block_size, self.strength_multiplier = list(types), block_size, multiplier


@functools.lru_cache(maxsize=None)
def reference(content, shape, qp, types, block_size=8, noise=("plane", 0), multiplier=1.0):
    """The restatement's answer, computed once a case.  ``noise``: ("plane", seed) or ("counter", seed, frame index)."""
    n = noise_plane(shape, noise[1]) if noise[0] == "plane" else (noise[1], noise[2])
    out = R.process_frame(frame_of(content, shape), qp, Cfg(types, block_size, multiplier), n)
    out.setflags(write=False)
    return out


def remover(types=("all",), block_size=8, seed=0, multiplier=1.0):
    return Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(artifact_types=[Q.ArtifactType(t) for t in types], block_size=block_size, seed=seed,
                                                        strength_multiplier=multiplier))


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                          # a copy: the cached frames are read-only


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- the steps through their own entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("d", [2, 5, 6, 7, 8, 11, 12, 15])
def test_bilateral_entry(torch_mod, shape, d):
    r = remover()
    strength = {2: 0.1, 5: 0.1, 6: 0.1, 7: 0.25, 8: 13 / 35, 11: 0.6, 12: 25 / 35, 15: 1.0}[d]
    sigma = 30 + strength * 70
    for content in ("random", "blocks"):
        f = frame_of(content, shape)
        t = dev(torch_mod, f)
        got = r.bilateral(t, d, sigma, sigma)
        assert got.data_ptr() != t.data_ptr() and np.array_equal(host(torch_mod, t), f)
        assert np.array_equal(host(torch_mod, got), R.bilateral_u8c3(f, d, sigma, sigma)), (content, shape, d)


def test_bilateral_with_a_narrow_colour_sigma_and_a_constant_frame(torch_mod):
    r = remover()
    f = frame_of("random", (33, 70))
    for d, sc, ss in ((15, 3.0, 100.0), (9, 1e30, 2.0), (12, 30.7, 30.7)):      # denormal colour weights; the space kernel alone
        assert np.array_equal(host(torch_mod, r.bilateral(dev(torch_mod, f), d, sc, ss)), R.bilateral_u8c3(f, d, sc, ss)), (d, sc, ss)
    c = np.empty((40, 72, 3), np.uint8)
    c[:] = (3, 250, 128)
    assert np.array_equal(host(torch_mod, r.bilateral(dev(torch_mod, c), 15, 100.0, 100.0)), c)


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian5_entry(torch_mod, shape):
    r = remover()
    for content in ("random", "blocks", "ramp"):
        f = frame_of(content, shape)
        assert np.array_equal(host(torch_mod, r.gaussian5(dev(torch_mod, f))), R.gaussian5_u8(f)), (content, shape)
    if shape == (17, 23):
        imp = np.zeros((17, 23, 3), np.uint8)
        imp[8, 11] = (255, 128, 1)
        k = np.array([1, 4, 6, 4, 1])
        got = host(torch_mod, r.gaussian5(dev(torch_mod, imp)))
        assert np.array_equal(got[6:11, 9:14, 0], (np.outer(k, k) * 255 + 128) >> 8) and np.array_equal(got, R.gaussian5_u8(imp))


# ---- the whole stage through fw_qp_artifacts_u8 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("types", [("all",), ("blocking",), ("ringing",), ("banding",)])
def test_stage_with_an_explicit_noise_plane(torch_mod, shape, qp, types):
    r = remover(types)
    assert Q.blocking_params(r.strength_for_qp(qp))[0] == {18: 6, 28: 8, 40: 12}[qp]
    for content in ("random", "blocks", "ramp"):
        f = frame_of(content, shape)
        t = dev(torch_mod, f)
        got = r.process_device([t], qp, [dev(torch_mod, noise_plane(shape))])[0]
        assert got.data_ptr() != t.data_ptr() and np.array_equal(host(torch_mod, t), f)
        assert np.array_equal(host(torch_mod, got), reference(content, shape, qp, types)), (content, shape, qp, types)


@pytest.mark.parametrize("block_size", [4, 8, 16, 32])
@pytest.mark.parametrize("types", [("all",), ("blocking",)])
def test_every_block_size(torch_mod, block_size, types):
    r = remover(types, block_size)
    for shape in ((33, 70), (40, 72), (3, 5)):
        for content in ("blocks", "random"):
            got = r.process_device([dev(torch_mod, frame_of(content, shape))], 34, [dev(torch_mod, noise_plane(shape))])[0]
            assert np.array_equal(host(torch_mod, got), reference(content, shape, 34, types, block_size)), (content, shape, block_size)


def test_type_subsets_the_half_multiplier_and_no_type_at_all(torch_mod):
    shape = (33, 70)
    f = frame_of("blocks", shape)
    for types in (("blocking", "banding"), ("ringing", "banding"), ("blocking", "ringing")):
        got = remover(types).process_device([dev(torch_mod, f)], 40, [dev(torch_mod, noise_plane(shape))])[0]
        assert np.array_equal(host(torch_mod, got), reference("blocks", shape, 40, types)), types
    for qp in (10, 34, 51):
        got = remover(multiplier=0.5).process_device([dev(torch_mod, f)], qp, [dev(torch_mod, noise_plane(shape))])[0]
        assert np.array_equal(host(torch_mod, got), reference("blocks", shape, qp, ("all",), 8, ("plane", 0), 0.5)), qp
    t = dev(torch_mod, f)
    got = remover(("mosquito",)).process_device([t], 40)[0]
    assert got.data_ptr() != t.data_ptr() and np.array_equal(host(torch_mod, got), f)


@pytest.mark.parametrize("types", [("all",), ("banding",)])
def test_the_counter_generator_with_two_seeds_and_two_frame_indices(torch_mod, types):
    shape = (33, 70)
    seen = []
    for seed in (0, 2 ** 40 + 9):
        r = remover(types, seed=seed)
        for index in (0, 7):
            for content in ("ramp", "random"):
                got = host(torch_mod, r.process_device([dev(torch_mod, frame_of(content, shape))], 40, None, index)[0])
                assert np.array_equal(got, reference(content, shape, 40, types, 8, ("counter", seed, index))), (seed, index, content)
                if content == "ramp":
                    seen.append(got)
    assert all(not np.array_equal(a, b) for i, a in enumerate(seen) for b in seen[:i])       # the dither is keyed by both


def test_the_serpentine_of_weak_edges_through_six_hysteresis_tiles(torch_mod):
    shape = (40, 72)
    f = frame_of("serpentine", shape)
    edges = R.canny_u8(R.bgr2gray_u8(f), 50, 150) > 0
    assert not R.canny_u8(R.bgr2gray_u8(serpentine_frame(strong=False)), 50, 150).any()        # weak everywhere without the spot
    assert edges.sum() > 400 and all(edges[ty:ty + 32, tx:tx + 32].sum() >= 9 for ty in (0, 32) for tx in (0, 32, 64))
    want = reference("serpentine", shape, 40, ("ringing",))
    assert (want != f).sum() > 1000                                                            # the chain was followed to its end
    r = remover(("ringing",))
    assert np.array_equal(host(torch_mod, r.process_device([dev(torch_mod, f)], 40)[0]), want)
    got = remover().process_device([dev(torch_mod, f)], 28, [dev(torch_mod, noise_plane(shape))])[0]
    assert np.array_equal(host(torch_mod, got), reference("serpentine", shape, 28, ("all",)))


def test_a_smooth_ramp_takes_the_whole_dither(torch_mod):
    shape = (40, 72)
    f = frame_of("ramp", shape)
    assert np.abs(R.banding_mask(f)[8:-8, 8:-8] - 1).max() < 1e-5                              # the Laplacian of a plane is 0 (off the border)
    got = host(torch_mod, remover(("banding",)).process_device([dev(torch_mod, f)], 40, [dev(torch_mod, noise_plane(shape))])[0])
    assert np.array_equal(got, reference("ramp", shape, 40, ("banding",))) and (got != f).mean() > 0.5


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_stream_equals_process_device_and_runs_repeat(torch_mod):
    shape = (33, 70)
    clip = [frame_of(c, shape) for c in ("random", "blocks", "ramp", "random")]
    r = remover(seed=3)
    tensors = [dev(torch_mod, f) for f in clip]
    whole = r.process_device(tensors, 34)
    first = [host(torch_mod, t) for t in whole]
    for i, f in enumerate(clip):
        assert np.array_equal(first[i], R.process_frame(f, 34, Cfg(("all",)), (3, i))), i
    assert not np.array_equal(first[0], first[3])                                               # one frame twice: another dither
    assert len({t.data_ptr() for t in whole} | {t.data_ptr() for t in tensors}) == 8
    assert all(np.array_equal(host(torch_mod, t), f) for t, f in zip(tensors, clip))
    again = [host(torch_mod, t) for t in r.process_device(tensors, 34)]
    streamed = [host(torch_mod, t) for t in r.stream(iter(tensors), 34)]
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(first, again, streamed))
    shifted = [host(torch_mod, t) for t in r.process_device(tensors[2:], 34, None, 2)]
    assert np.array_equal(shifted[0], first[2]) and np.array_equal(shifted[1], first[3])
    hosted = r.process([f.copy() for f in clip], 34)
    assert all(isinstance(a, np.ndarray) and np.array_equal(a, b) for a, b in zip(hosted, first))
    assert np.array_equal(host(torch_mod, r.process_frame(tensors[1], 34, None, 1)), first[1])
    assert r.process_device([]) == []


def test_qp_falls_back_to_manual_qp_then_28(torch_mod):
    shape = (17, 23)
    f = frame_of("random", shape)
    n = [dev(torch_mod, noise_plane(shape))]
    assert np.array_equal(host(torch_mod, remover().process_device([dev(torch_mod, f)], None, n)[0]), reference("random", shape, 28, ("all",)))
    r = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(manual_qp=40))
    assert np.array_equal(host(torch_mod, r.process_device([dev(torch_mod, f)], None, n)[0]), reference("random", shape, 40, ("all",)))
    assert np.array_equal(host(torch_mod, r.process_device([dev(torch_mod, f)], 18, n)[0]), reference("random", shape, 18, ("all",)))


def test_a_caller_s_destination(torch_mod):
    shape = (17, 23)
    f = frame_of("blocks", shape)
    t, out = dev(torch_mod, f), torch_mod.zeros(shape + (3,), dtype=torch_mod.uint8, device="cuda")
    r = remover()
    got = r.process_device([t], 28, [dev(torch_mod, noise_plane(shape))], 0, out=[out])
    assert got[0] is out and np.array_equal(host(torch_mod, out), reference("blocks", shape, 28, ("all",)))
    with pytest.raises(ValueError, match="qp_artifacts: a destination overlaps a source frame"):
        r.process_device([t], 28, out=[t])
    buf = torch_mod.zeros(17 * 23 * 3 + 30, dtype=torch_mod.uint8, device="cuda")
    a, b = buf[:17 * 23 * 3].view(17, 23, 3), buf[30:].view(17, 23, 3)
    with pytest.raises(ValueError, match="qp_artifacts: a destination overlaps a source frame"):
        r.process_device([a], 28, out=[b])
    with pytest.raises(ValueError, match="qp_artifacts: contiguous uint8 destinations"):
        r.process_device([t], 28, out=[torch_mod.zeros((17, 24, 3), dtype=torch_mod.uint8, device="cuda")])
    with pytest.raises(ValueError, match="qp_artifacts: one destination per frame expected"):
        r.process_device([t], 28, out=[])


def test_misuse_is_refused_with_the_stage_s_message(torch_mod):
    torch = torch_mod
    r = remover()
    good = dev(torch, frame_of("random", (17, 23)))
    wrong = "qp_artifacts: uint8 CUDA tensors H x W x 3 \\(BGR\\) expected"
    for bad in (good[:, :, 0].contiguous(), torch.zeros((17, 23, 4), dtype=torch.uint8, device="cuda"), good.float(), good.to(torch.int16),
                frame_of("random", (17, 23))):
        with pytest.raises(ValueError, match=wrong):
            r.process_device([bad], 28)
    with pytest.raises(ValueError, match=wrong):
        r.process_device([good, dev(torch, frame_of("random", (3, 5)))], 28)                 # two shapes in one call
    with pytest.raises(ValueError, match="qp_artifacts: frames on cuda:0, the remover's device, expected"):
        r.process_device([good.cpu()], 28)
    with pytest.raises(ValueError, match="qp_artifacts: strength 1.429 \\(qp 40 x multiplier 2.0\\) is above 1"):
        remover(multiplier=2.0).process_device([good], 40)
    assert remover(multiplier=2.0).process_device([good], 28)[0].shape == good.shape           # 0.743: the pair is what is refused
    noise = "qp_artifacts: noise as float32 CUDA tensors H x W x 3 on the frames' device expected, one per frame"
    plane = dev(torch, noise_plane((17, 23)))
    for bad in ([plane[:16]], [plane.double()], [plane.cpu()], [plane, plane], [plane[:, :, 0]], [noise_plane((17, 23))]):
        with pytest.raises(ValueError, match=noise):
            r.process_device([good], 28, bad)
    with pytest.raises(ValueError, match=wrong):
        r.bilateral(good[:, :, 0].contiguous(), 7, 50.0, 50.0)
    with pytest.raises(ValueError, match=wrong):
        r.gaussian5(good.float())
    with pytest.raises(ValueError, match="qp_artifacts: uint8 arrays H x W x 3 \\(BGR\\) expected"):
        r.process([np.zeros((4, 4), np.uint8)], 28)
    r.close()
    assert not r.is_available() and r._scratch is None and r._tables == {}
    with pytest.raises(ValueError, match="qp_artifacts: the remover is closed"):
        r.process_device([good], 28)


def test_the_c_abi_refuses_bad_arguments(torch_mod, hip_lib):
    torch = torch_mod
    f = dev(torch, frame_of("random", (17, 23)))
    out = torch.empty_like(f)
    color, space = (dev(torch, a) for a in Q.bilateral_tables(8, 50.0, 50.0))
    table = dev(torch, Q.noise_table(0.5))
    g15 = Q.gaussian15_coeffs()
    scratch = torch.empty(int(hip_lib.fw_qp_artifacts_scratch_bytes(17, 23)), dtype=torch.uint8, device="cuda")
    assert hip_lib.fw_qp_artifacts_scratch_bytes(0, 23) == 0 and hip_lib.fw_qp_artifacts_scratch_bytes(17, 16385) == 0
    p = _lib.ptr

    def stage(frame=f, dst=out, h=17, w=23, c=3, d=8, col=color, sp=space, g=g15, strength=0.5, block=8, mask=7, noise=None, tab=table,
              scr=scratch):
        return hip_lib.fw_qp_artifacts_u8(p(frame), p(dst), h, w, c, d, p(col), p(sp), None if g is None else g.ctypes.data_as(C.c_void_p),
                                          strength, block, mask, p(noise), p(tab), 5, p(scr), None)

    def refused(status, text):
        assert status == _lib.FW_ERR_INVALID and text in hip_lib.fw_last_error().decode(), hip_lib.fw_last_error()

    refused(stage(frame=None), "fw_qp_artifacts_u8: null pointer")
    refused(stage(dst=None), "fw_qp_artifacts_u8: null pointer")
    refused(stage(h=0), "1 .. 16384 pixels a side expected")
    refused(stage(w=16385), "1 .. 16384 pixels a side expected")
    refused(stage(c=1), "3 (BGR) channels expected")
    refused(stage(c=4), "1 (gray) or 3 (BGR) channels expected")
    refused(stage(dst=f), "fw_qp_artifacts_u8: out overlaps frame")
    refused(stage(d=1), "d 2 .. 15 expected")
    refused(stage(d=16), "d 2 .. 15 expected")
    refused(stage(col=None), "null pointer")
    refused(stage(block=12), "block size 4, 8, 16 or 32 expected")
    refused(stage(mask=8), "a type mask 0 .. 7 expected")
    refused(stage(strength=1.25), "a strength in (0, 1] expected")
    refused(stage(strength=0.0), "a strength in (0, 1] expected")
    refused(stage(g=None), "null pointer")
    refused(stage(tab=None), "null pointer")
    refused(stage(scr=None), "a 256-byte aligned scratch")
    refused(stage(scr=scratch[1:]), "a 256-byte aligned scratch")
    assert stage(mask=2, col=None, sp=None, g=None, tab=None) == _lib.FW_OK                     # ringing alone needs no table
    refused(hip_lib.fw_bilateral_u8c3(p(f), p(f), 17, 23, 3, 8, p(color), p(space), None), "fw_bilateral_u8c3: out overlaps frame")
    refused(hip_lib.fw_bilateral_u8c3(p(f), p(out), 17, 23, 3, 8, None, p(space), None), "fw_bilateral_u8c3: null pointer")
    refused(hip_lib.fw_bilateral_u8c3(p(f), p(out), 17, 23, 1, 8, p(color), p(space), None), "3 (BGR) channels expected")
    refused(hip_lib.fw_gaussian5_u8(p(f), p(f), 17, 23, 3, None), "fw_gaussian5_u8: out overlaps frame")
    refused(hip_lib.fw_gaussian5_u8(None, p(out), 17, 23, 3, None), "fw_gaussian5_u8: null pointer")
    refused(hip_lib.fw_gaussian5_u8(p(f), p(out), 17, 0, 3, None), "1 .. 16384 pixels a side expected")
    torch.cuda.synchronize()
