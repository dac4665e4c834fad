"""Host side of tests/conv_epilogue_ref.py: the restatements are pinned to torch in float64 (F.conv2d, F.prelu, the ResConv form
F.leaky_relu(conv * beta + x), F.pixel_shuffle + F.interpolate(nearest) for scales 1 to 4), every listed defect, computed exactly,
leaves the bound of the GPU tests by at least 100x on the inputs those tests use, and every uint8 input set stays within the 0.5 %
window cap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R

DTYPES = ["f16", "bf16"]


def _t(a):
    """(H, W, C) -> (1, C, H, W) float64 tensor."""
    return torch.from_numpy(np.asarray(a, np.float64)).permute(2, 0, 1)[None]


def _hwc(t):
    return t[0].permute(1, 2, 0).numpy()


def _worst(wrong, ref, bound):
    return float((np.abs(wrong - ref) / bound).max())


@pytest.mark.parametrize("chunks,ct", [(1, 1), (2, 2)])
def test_conv_prelu_and_resconv_are_torchs(chunks, ct):
    H, W = 5, 3
    _, _, b, xv, wv = R.conv_inputs(H, W, chunks, ct, "f16")
    t, A = R.conv3x3(xv, wv, b)
    conv = F.conv2d(_t(xv), torch.from_numpy(wv), torch.from_numpy(b).double(), 1, 1)
    assert np.abs(t - _hwc(conv)).max() <= 1e-13 * np.abs(t).max() and (A >= np.abs(t) - 1e-12).all()
    assert (t > 0).any() and (t < 0).any()                                       # the outputs straddle zero
    slopes = R.channel_vector(32 * ct, 1)
    y, bound = R.prelu(t, A, slopes, chunks)
    assert np.abs(y - _hwc(F.prelu(conv, torch.from_numpy(slopes).double()))).max() <= 1e-13 * np.abs(t).max()
    assert (bound > 0).all()
    if ct == 2:
        beta = R.channel_vector(64, 2)
        r1, r2 = R.residual_buffers(H, W)
        x1, x2 = r1[:, :, 64:128], r2[:, :, 64:128]
        y, _ = R.residual(t, A, chunks, beta, 1.0, x1, post_act=1)
        want = F.leaky_relu(conv * torch.from_numpy(beta).double().view(1, 64, 1, 1) + _t(x1), 0.2)      # ResConv
        assert np.abs(y - _hwc(want)).max() <= 1e-13 * np.abs(y).max()
        y, _ = R.residual(t, A, chunks, np.ones(64), 0.2, x1, 0.2, x2)
        want = (conv * float(np.float32(0.2)) + _t(x1)) * float(np.float32(0.2)) + _t(x2)                 # the RRDB's two residuals
        assert np.abs(y - _hwc(want)).max() <= 1e-13 * np.abs(y).max()


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_shuffle_tail_is_pixel_shuffle_plus_nearest(s):
    for H, W in R.TAIL_SHAPES:
        conv, img = R.tail_inputs(H, W, s, 64)
        got, bound = R.shuffle_tail(conv, img, s)
        x = _t(img[:, :, ::-1].astype(np.float64) / 255.0)
        want = F.pixel_shuffle(_t(conv[:, :, :3 * s * s]), s) + F.interpolate(x, scale_factor=s, mode="nearest")
        assert got.shape == (H * s, W * s, 3) and np.abs(got - _hwc(want)).max() <= 1e-15
        assert (bound >= 0).all() and bound.max() < 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_u8_to_nhwc_both_forms_agree_on_every_level(dtype):
    """The kernel multiplies by fp32(1 / 255), the contract divides by fp32(255): the typed results are the same bits for all 256 levels."""
    img = R.levels_image()
    assert all(len(set(img[:, :, c].reshape(-1).tolist())) == 256 for c in range(3))
    a, b = R.u8_to_nhwc(img, dtype, 40), R.u8_to_nhwc(img, dtype, 40, reciprocal=True)
    assert np.array_equal(a, b) and (a[:, :, 3:] == 0).all()
    want = (torch.from_numpy(img[:, :, ::-1].astype(np.float32)) / 255.0).to(torch.float16 if dtype == "f16" else torch.bfloat16)
    assert np.array_equal(a[:, :, :3], want.view(torch.int16).numpy().view(np.uint16))
    assert not np.array_equal(R.u8_to_nhwc(img, dtype, 40, defect="bgr_kept"), a)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("H,W", R.CONV_SHAPES)
def test_conv_epilogue_bounds_reject_defects(dtype, chunks, H, W):
    for ct in (1, 2):
        _, _, b, xv, wv = R.conv_inputs(H, W, chunks, ct, dtype)
        t, A = R.conv3x3(xv, wv, b)
        slopes = R.channel_vector(32 * ct, 1)
        assert len(set(slopes.tolist())) == 32 * ct and slopes.min() < 0 and slopes.max() > 1 and (slopes == 0).any()
        ref, bound = R.prelu(t, A, slopes, chunks)
        worst = _worst(R.prelu(t, A, slopes, chunks, "slope_n16")[0], ref, bound)
        print(f"PReLU {H}x{W} chunks {chunks} tiles {ct} {dtype}: slope of channel n + 16: {worst:.0f} x the bound")
        assert worst >= 100
        assert _worst(np.maximum(t, 0.2 * t), ref, bound) >= 100                 # LeakyReLU in its place
    _, _, b, xv, wv = R.conv_inputs(H, W, chunks, 2, dtype)
    t, A = R.conv3x3(xv, wv, b)
    beta = R.channel_vector(64, 2)
    r1, r2 = R.residual_buffers(H, W)
    x1, x2 = r1[:, :, 64:128], r2[:, :, 64:128]
    for post_act in (0, 1):
        for two in (False, True):
            kw = dict(s2=0.5, res2=x2) if two else {}
            ref, bound = R.residual(t, A, chunks, beta, 0.2, x1, post_act=post_act, **kw)
            wrong = {"gamma_n4": R.residual(t, A, chunks, beta, 0.2, x1, post_act=post_act, defect="gamma_n4", **kw)[0],
                     "coff_ignored": R.residual(t, A, chunks, beta, 0.2, r1[:, :, :64], post_act=post_act,
                                                **(dict(s2=0.5, res2=r2[:, :, :64]) if two else {}))[0]}
            if post_act:
                wrong["post_act_first"] = R.residual(t, A, chunks, beta, 0.2, x1, post_act=1, defect="post_act_first", **kw)[0]
            assert set(wrong) <= set(R.DEFECTS_RES)
            for name, y in wrong.items():
                worst = _worst(y, ref, bound)
                print(f"residual {H}x{W} chunks {chunks} post_act {post_act} res2 {two} {dtype} {name}: {worst:.0f} x the bound")
                assert worst >= 100, name


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", R.TAIL_SHAPES)
def test_tail_bounds_reject_defects_and_the_window_is_narrow(s, H, W):
    for cstride in (64, 3 * s * s):
        conv, img = R.tail_inputs(H, W, s, cstride)
        ref, bound = R.shuffle_tail(conv, img, s)
        lo, hi, share = R.u8_window(ref, bound)
        assert share <= R.U8_WINDOW_SHARE, share
        want = R.to_bytes(ref)
        assert ((want >= lo[:, :, ::-1]) & (want <= hi[:, :, ::-1])).all()
        if H * W > 1:
            assert (ref < 0).any() and (ref > 1).any()                           # both clamps are met
        for defect in ("sub_transposed", "bgr_kept"):
            if defect == "sub_transposed" and s == 1:
                continue                                                          # one sub-position: nothing to transpose
            worst = _worst(R.shuffle_tail(conv, img, s, defect)[0], ref, bound)
            print(f"tail {H}x{W} s {s} cstride {cstride} {defect}: {worst:.0f} x the bound")
            assert worst >= 100, defect
        trunc = R.to_bytes(ref, defect="truncate")[:, :, ::-1]                    # RGB order, as lo / hi
        off = np.abs(trunc - 255.0 * np.clip(ref, 0, 1)) - 0.5                    # how far outside the rounding cell of rint
        outside = (trunc < lo) | (trunc > hi)
        print(f"tail {H}x{W} s {s} truncation: {outside.mean():.2f} of the bytes outside the window, {float((off / (255 * bound)).max()):.0f} x the bound")
        assert (off / (255 * bound)).max() >= 100
        assert outside.mean() > 0.25 if H * W * s * s >= 100 else outside.any()


def test_u16_window_is_the_analogue_of_u8_window():
    rng = np.random.default_rng(5)
    v = rng.uniform(-0.1, 1.1, 20000)
    lo, hi, share = R.u16_window(v, 1e-7 * np.ones_like(v))
    assert share <= R.U8_WINDOW_SHARE * 8 and (lo <= hi).all() and lo.min() == 0 and hi.max() == 65535
    assert ((np.rint(np.clip(v, 0, 1) * 65535) >= lo) & (np.rint(np.clip(v, 0, 1) * 65535) <= hi)).all()
