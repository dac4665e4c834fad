"""tests/ifnet_glue_ref.py (the float64 references that tests/test_ifnet_glue_gpu.py holds the IFNet glue kernels to) pinned to torch
in float64 on the CPU: F.interpolate, F.grid_sample through oracle.ifnet_ref.warp, F.pixel_unshuffle, F.pixel_shuffle of
conv_transpose2d, torch.sigmoid, and ifnet_ref.ifblock's own front end.  Agreement is asked to float64 rounding (1e-12 relative to the
data's scale; the warps 1e-9, because grid_sample normalises the coordinate to [-1, 1] and back).  Also: the bounds hold for an fp32
numpy evaluation of the kernels' expressions, and the uint8 rounding window stays under 0.5 % of the elements for every input the GPU
test uses.  The arithmetic is IFNet_HDv3 v4.6 as oracle/ifnet_ref.py restates it: **parity vs upstream stays unpinned**."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ifnet_glue_ref as G
from framewright_amd import rife as RF
from oracle import ifnet_ref

EPS = 1e-12


@pytest.fixture()
def f64_default():
    """oracle.ifnet_ref.warp builds its base grid with torch.linspace in the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _nchw(a):
    return torch.from_numpy(np.asarray(a)).double().permute(2, 0, 1).unsqueeze(0)


def _hwc(t):
    return t[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("sf", [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0])
def test_resize_bilinear_is_torch_interpolate(sf):
    rng = np.random.default_rng(int(sf * 8))
    hs, ws = (64, 96) if sf < 1 else (6, 9)
    src = rng.standard_normal((hs, ws, 5)).astype(np.float32)
    val, bound = G.resize_bilinear(src, sf, 0.5)
    want = 0.5 * _hwc(F.interpolate(_nchw(src), scale_factor=sf, mode="bilinear", align_corners=False))
    assert np.abs(val.reshape(want.shape) - want).max() <= EPS * 8
    assert (bound > 0).all() and bound.max() < 1e-5
    with pytest.raises(AssertionError):
        G.resize_bilinear(src, 3.0)                    # not a power of two: coordinates are not exact, no bound is claimed


@pytest.mark.parametrize("H,W", [(32, 32), (19, 45), (1, 1), (1, 7), (5, 1)])
@pytest.mark.parametrize("img_kind", G.IMAGE_KINDS)
@pytest.mark.parametrize("flow_kind", G.FLOW_KINDS)
def test_warp_and_build_x_are_grid_sample(f64_default, H, W, img_kind, flow_kind):
    rng = np.random.default_rng(H * 100 + W)
    i0, i1 = G.make_images(img_kind, H, W, rng)
    flow, mask = G.make_flow(flow_kind, H, W, rng), G.make_mask(H, W, rng)
    val, bound = G.build_x(i0, i1, flow, mask, 0.25)
    val, bound = val.reshape(H, W, 8), bound.reshape(H, W, 8)
    if H > 1 and W > 1:                                 # ifnet_ref.warp divides by (w - 1) / 2
        fl = _nchw(flow)
        w0, w1 = _hwc(ifnet_ref.warp(_nchw(i0), fl[:, :2])), _hwc(ifnet_ref.warp(_nchw(i1), fl[:, 2:4]))
        assert np.abs(val[..., :3] - w0).max() <= 1e-9 and np.abs(val[..., 3:6] - w1).max() <= 1e-9
    assert (val[..., 6] == 0.25).all() and np.array_equal(val[..., 7], mask.astype(np.float64))
    assert (bound[..., 6:] == 0).all() and (bound[..., :6] > 0).all()
    # the kernel's expression evaluated in fp32 numpy (no contraction) stays inside the bound
    f32 = np.float32
    y, x = np.mgrid[0:H, 0:W]
    for img, c0, k in ((i0, 0, 0), (i1, 3, 2)):
        sx = np.clip(x.astype(f32) + flow[..., k], f32(0), f32(W - 1))
        sy = np.clip(y.astype(f32) + flow[..., k + 1], f32(0), f32(H - 1))
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        wx, wy = (sx - x0.astype(f32))[..., None], (sy - y0.astype(f32))[..., None]
        one = f32(1)
        got = (img[y0, x0] * (one - wx) + img[y0, x1] * wx) * (one - wy) + (img[y1, x0] * (one - wx) + img[y1, x1] * wx) * wy
        assert got.dtype == np.float32
        r = np.abs(got.astype(np.float64) - val[..., c0:c0 + 3]) / bound[..., c0:c0 + 3]
        assert r.max() <= 1.0, r.max()
    v7, b7 = G.build_x(i0, i1, None, None, 0.5)
    assert np.array_equal(v7[:, :3], i0.reshape(-1, 3).astype(np.float64)) and np.array_equal(v7[:, 3:6], i1.reshape(-1, 3).astype(np.float64))
    assert (v7[:, 6] == 0.5).all() and (b7 == 0).all()


def test_position_term_follows_the_coordinate_and_the_slope():
    """On a ramp of slope g along x the position term is half an fp32 ulp of the coordinate times g, and none where both clamps apply."""
    H, W = 4, 2048
    img = np.repeat((np.arange(W, dtype=np.float32) * np.float32(2.0 ** -12))[None, :, None], H, 0).repeat(3, 2)
    ys, xs = np.array([1, 1, 1]), np.array([3, 1500, 1500])
    fx = np.array([0.3, 0.3, 1e4], np.float32)
    _, b = G.warp(img, fx, np.zeros(3, np.float32), ys, xs)
    arith = G.gamma(G.K_BILIN) * np.array([3.3, 1500.3, 2047.0]) * 2.0 ** -12
    pos = np.array([0.5 * 2.0 ** -22, 0.5 * 2.0 ** -13, 0.0]) * 2.0 ** -12
    assert np.allclose(b[:, 0], arith + pos + G.TINY, rtol=1e-6)


def test_unshuffle_and_depth_to_space_are_torch_pixel_shuffles():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((12, 20, 9)).astype(np.float32)
    got = G.unshuffle2(x, 7, 32)
    want = _hwc(F.pixel_unshuffle(_nchw(x[:, :, :7]), 2))
    assert np.array_equal(got[..., :28].astype(np.float64), want) and (got[..., 28:] == 0).all()
    ri = lambda *shape: torch.randint(-3, 4, shape).double()          # small integers: every sum is exact, in fp32 as well
    xs, wt, bt = ri(1, 6, 8, 10), ri(6, 24, 4, 4), ri(24)
    want = F.pixel_shuffle(F.conv_transpose2d(xs, wt, bt, stride=2, padding=1), 2)
    w3, b3 = RF.convtranspose_as_3x3(wt.numpy(), bt.numpy())
    y = F.conv2d(xs, torch.from_numpy(w3).double(), torch.from_numpy(b3).double(), padding=1)
    src = np.concatenate([_hwc(y), np.full((8, 10, 4), 7.0)], 2)              # a channel stride of 100
    assert np.array_equal(G.depth_to_space4(src), _hwc(want))
    # the permuted layout the fused accumulate reads = the engine's row permutation of depth_to_space4's layout
    assert np.array_equal(G.tmp_to_t96(G.depth_to_space4(src)), G.d2s_rows_to_t96(src))
    t = G.tmp_to_t96(G.depth_to_space4(src), cs=98, fill=-1.0)
    assert t.shape == (8, 10, 98) and (t[..., 96:] == -1).all()


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("first", [True, False])
def test_accumulate_is_interpolate_times_scale(scale, first):
    rng = np.random.default_rng(scale)
    H, W = 32, 64
    tmp = rng.standard_normal((H // scale, W // scale, 6)).astype(np.float32)
    flow, mask = rng.standard_normal((H, W, 4)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
    f, fb, m, mb = G.accumulate(tmp, H, W, float(scale), flow, mask, first)
    up = _hwc(F.interpolate(_nchw(tmp), scale_factor=float(scale), mode="bilinear", align_corners=False))
    wf = up[..., :4] * scale + (0 if first else flow.astype(np.float64))
    wm = up[..., 4] + (0 if first else mask.astype(np.float64))
    assert np.abs(f.reshape(H, W, 4) - wf).max() <= 50 * EPS and np.abs(m.reshape(H, W) - wm).max() <= 50 * EPS
    assert (fb > 0).all() and (mb > 0).all() and fb.max() < 1e-4


class _Stop(Exception):
    pass


class _CaptureF:
    """torch.nn.functional with a conv2d that keeps its input and stops the block there."""

    def __init__(self):
        self.x = None

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, *a, **k):
        self.x = x
        raise _Stop


@pytest.mark.parametrize("s", [8, 4, 2, 1])
@pytest.mark.parametrize("first", [True, False])
def test_stage_input_is_ifblocks_own_front_end(f64_default, monkeypatch, s, first):
    rng = np.random.default_rng(s + 10 * first)
    H, W = 32, 64
    i0, i1 = G.make_images("noise", H, W, rng)
    flow, mask = (None, None) if first else (G.make_flow("rand6", H, W, rng), G.make_mask(H, W, rng))
    t = torch.full((1, 1, H, W), 0.25)
    if first:
        x, fl = torch.cat([_nchw(i0), _nchw(i1), t], 1), None
    else:
        fl = _nchw(flow)
        x = torch.cat([ifnet_ref.warp(_nchw(i0), fl[:, :2]), ifnet_ref.warp(_nchw(i1), fl[:, 2:4]), t, _nchw(mask[..., None])], 1)
    cap = _CaptureF()
    monkeypatch.setattr(ifnet_ref, "F", cap)
    with pytest.raises(_Stop):
        ifnet_ref.ifblock({"p.conv0.0.0.weight": None, "p.conv0.0.0.bias": None}, "p.", x, fl, s)
    monkeypatch.undo()
    cin = 7 if first else 12
    want = _hwc(F.pixel_unshuffle(cap.x, 2))
    val, bound = G.stage_input(i0, i1, flow, mask, 0.25, s, 64)
    val, bound = val.reshape(want.shape[0], want.shape[1], 64), bound.reshape(want.shape[0], want.shape[1], 64)
    assert want.shape[2] == 4 * cin
    assert np.abs(val[..., :4 * cin] - want).max() <= 1e-9
    assert (val[..., 4 * cin:] == 0).all() and (bound[..., 4 * cin:] == 0).all() and (bound[..., :4 * cin] > 0).all()
    # points: the same values as the whole map
    pts = (np.array([0, H // s // 2 - 1]), np.array([1, W // s // 2 - 1]))
    v2, _ = G.stage_input(i0, i1, flow, mask, 0.25, s, 64, pts)
    assert np.array_equal(v2, val[pts[0], pts[1]])


def test_sigmoid_blend_and_the_uint8_window(f64_default):
    rng = np.random.default_rng(11)
    Hp, Wp, H, W = 96, 128, 70, 100
    i0, i1 = G.make_images("noise", Hp, Wp, rng)
    flow, mask = G.make_flow("rand6", Hp, Wp, rng), G.make_mask(Hp, Wp, rng)
    m, rm = G.sigmoid(mask)
    assert np.abs(m - torch.sigmoid(torch.from_numpy(mask).double()).numpy()).max() <= EPS
    assert rm.max() <= (G.EXPF_REL + 2.1 * G.U) * 1.01 and np.abs(mask).max() == 20
    val, bound = G.blend(i0, i1, flow, mask, H, W)
    fl, mm = _nchw(flow), torch.sigmoid(_nchw(mask[..., None]))
    want = _hwc(ifnet_ref.warp(_nchw(i0), fl[:, :2]) * mm + ifnet_ref.warp(_nchw(i1), fl[:, 2:4]) * (1 - mm))[:H, :W]
    assert np.abs(val.reshape(H, W, 3) - want).max() <= 1e-9
    lo, hi, share = G.u8_window(val, bound)
    assert share <= G.U8_WINDOW_SHARE and ((hi - lo) >= 0).all() and ((hi - lo) <= 1).all()
    r = np.rint(np.clip(val, 0, 1) * 255).astype(int)
    assert ((lo <= r) & (r <= hi)).all()


@pytest.mark.parametrize("H,W", [(1080, 1920), (70, 100), (1, 1), (64, 96)])
def test_uint8_window_share_of_every_gpu_blend_input(H, W):
    """The same seeded inputs as test_ifnet_glue_gpu.py::test_blend: at most 0.5 % of the elements may take either neighbour."""
    for case in G.blend_cases(H, W):
        i0, i1, flow, mask, pts = G.blend_inputs(H, W, *case)
        val, bound = G.blend(i0, i1, flow, mask, H, W, pts)
        assert G.u8_window(val, bound)[2] <= G.U8_WINDOW_SHARE, case


def test_casts_and_typed_ulp():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096) * np.exp(rng.uniform(-30, 10, 4096)), [0.0, 1.0, 65504.0, 2.0 ** -24, 2.0 ** -14]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(G.to_bits(x, "bf16"), want)
    assert np.array_equal(G.from_bits(want, "bf16"), torch.from_numpy(x).to(torch.bfloat16).double().numpy())
    h = x[np.abs(x) < 60000].astype(np.float16)
    assert np.array_equal(G.from_bits(h.view(np.uint16), "f16"), h.astype(np.float64))
    assert np.array_equal(G.typed_ulp(h.astype(np.float64), "f16"), np.spacing(np.abs(h)).astype(np.float64))
    assert G.typed_ulp(np.array([1.0, 1.5, 2.0, 0.0]), "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]
    img = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    v, b = G.u8_to_rgb(img, 32, 32)
    assert np.array_equal(v[:3, :5], img[:, :, ::-1] / 255.0) and (v[3:] == 0).all() and (v[:, 5:] == 0).all() and (b <= G.gamma(1)).all()
