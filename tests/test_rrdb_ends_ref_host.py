"""tests/rrdb_ends_ref.py on the CPU: every restatement pinned to torch in float64 (F.conv2d, F.pixel_unshuffle on F.pad(..., "reflect"),
F.interpolate(nearest), F.leaky_relu), the input sets of the two GPU tests checked for what those tests rely on (both clamps met, the
share of bytes a bound leaves open under U8_WINDOW_SHARE), and every planted defect shown to leave the bound the GPU tests assert.

Where no error bound rejects a defect, the assertion that does is named:

  * "truncate": a float plane says nothing about how it is quantised.  tests/test_rrdb_tail_ops_gpu.py and tests/test_rrdb_ends_gpu.py
    require the image to equal rint(clip(plane, 0, 1) * top) of the kernel's own float plane bit for bit; the u8 window of the float64
    reference rejects it as well (shown here).
  * "crop_stride_W": a kernel that stores plane AND image with row stride W keeps the image equal to the rint of its own plane.  What
    rejects it is the per-sample bound of the cropped float plane (shown here) - and the guards behind the buffers, which such a
    kernel writes past.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrdb_ends_ref as E
from ifnet_glue_ref import from_bits, to_bits

TT = {"f16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("f16", "bf16")


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(2, 0, 1)[None]


def _nhwc(t):
    return t[0].permute(1, 2, 0).contiguous().numpy()


def _conv(x, w, b):
    return _nhwc(F.conv2d(_nchw(x), torch.from_numpy(np.asarray(w, np.float64)), torch.from_numpy(np.asarray(b, np.float64)), padding=1))


def _close(a, b, rel=1e-12):
    return np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300)


# ---- head --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("top", [255, 65535])
def test_reciprocal_and_division_give_the_same_typed_sample_at_every_level(dtype, top):
    """The kernel multiplies by the fp32 constant 1 / top, the contract divides: the same bits for each of the top + 1 levels."""
    v = np.arange(top + 1, dtype=np.float32)
    assert np.array_equal(to_bits(v / np.float32(top), dtype), to_bits(v * (np.float32(1.0) / np.float32(top)), dtype))


def _torch_head(frame, dtype, scale):
    top = 255.0 if frame.dtype == np.uint8 else 65535.0
    x = (torch.from_numpy(frame.astype(np.float32)) / np.float32(top)).to(TT[dtype]).to(torch.float64)
    x = x.flip(2).permute(2, 0, 1)[None]                              # BGR -> RGB, NCHW
    if scale == 2:
        x = F.pixel_unshuffle(F.pad(x, (0, x.shape[3] % 2, 0, x.shape[2] % 2), "reflect"), 2)
    return _nhwc(x)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_equals_torch(dtype, scale, bits):
    sd = E.ends_state(scale)
    for H, W in E.HEAD_FRAMES[scale]:
        frame = E.head_frame(H, W, bits)
        if H * W >= 256:                                              # the frames are what the GPU test says they are
            lv = np.arange(256) if bits == 8 else np.array([0, 65535] + [1 << k for k in range(16)])
            assert all(np.isin(lv, frame[:, :, c]).all() for c in range(3))
        x = E.frame_to_nhwc(frame, dtype, scale)
        want = _torch_head(frame, dtype, scale)
        cin = want.shape[2]
        assert cin == (12 if scale == 2 else 3) and x.shape == want.shape[:2] + (32,)
        assert np.array_equal(x[:, :, :cin], want) and not x[:, :, cin:].any()
        t, A = E.conv_first(x, sd, dtype)
        w = E.rnd(sd["conv_first.weight"], dtype)
        assert _close(t, _conv(want, w, sd["conv_first.bias"]))
        assert _close(A, _conv(np.abs(want), np.abs(w), np.abs(sd["conv_first.bias"])))


@pytest.mark.parametrize("defect", E.HEAD_DEFECTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_defects_leave_conv_firsts_bound(dtype, defect):
    """Each on the x2 model at an odd frame (the reflect row and column exist), 16-bit for the 16-bit defect."""
    sd = E.ends_state(2)
    frame = E.head_frame(33, 65, 16 if defect == "div255_on_u16" else 8)
    t, A = E.conv_first(E.frame_to_nhwc(frame, dtype, 2), sd, dtype)
    td, _ = E.conv_first(E.frame_to_nhwc(frame, dtype, 2, defect), sd, dtype)
    over = np.abs(td - t) > E.bound_first(A)
    assert over.any()
    if defect == "zero_pad":                                          # only the last trunk row and column (and their neighbours' taps) see the pad
        assert not over[:-2, :-2].any() and over[-1].any() and over[:, -1].any()
    else:
        assert over.mean() > 0.5
    print(f"{defect} {dtype}: {over.mean():.3f} of conv_first's outputs beyond gamma(10) A_t, worst {(np.abs(td - t) / E.bound_first(A)).max():.3g} of it")


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_trunk_is_exact_in_fp32(dtype):
    Fv = E.RB.lively_trunk(5, 9, 1)
    hi, lo = E.RB._hi_lo(Fv.astype(np.float64), dtype)
    got = E.head_trunk(Fv, dtype, True)
    assert np.array_equal(got.astype(np.float64), hi + lo)            # the fp32 sum of the pair is exact
    assert (got != Fv).any() and np.abs(got.astype(np.float64) - Fv).max() <= 2.0 ** -17 * np.abs(Fv).max()
    assert E.head_trunk(Fv, dtype, False) is not None and np.array_equal(E.head_trunk(Fv, dtype, False), Fv)


# ---- tail, op level ------------------------------------------------------------------------------------------------------------------
def _op_reference(H, W, dtype):
    xb, x, w_hr, b_hr, w_last, b_last = E.tail_op_inputs(H, W, dtype)
    h, A_h = E.conv_hr(x, E.rnd(w_hr, dtype), b_hr)
    ht = E.round_to(h, dtype)
    v, Sm = E.conv_last(ht, E.rnd(w_last, dtype), b_last)
    return x, h, A_h, ht, v, Sm, (w_hr, b_hr, w_last, b_last)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_ops_equal_torch(dtype):
    H, W = 17, 33
    x, _, _, ht, v, Sm, (w_hr, b_hr, w_last, b_last) = _op_reference(H, W, dtype)
    h2, A2 = E.conv_hr(x, E.rnd(w_hr, dtype), b_hr, slope=0.2)
    assert _close(h2, _nhwc(F.leaky_relu(_nchw(_conv(x, E.rnd(w_hr, dtype), b_hr)), 0.2)))
    assert _close(A2, _conv(np.abs(x), np.abs(E.rnd(w_hr, dtype)), np.abs(b_hr)))
    assert _close(v, _conv(ht, E.rnd(w_last, dtype), b_last)) and _close(Sm, _conv(np.abs(ht), np.abs(E.rnd(w_last, dtype)), np.abs(b_last)))
    for top in (255, 65535):
        want = (torch.from_numpy(v).clamp(0, 1) * top).round().flip(2).numpy().astype(np.int64)      # torch.round is half-to-even
        assert np.array_equal(E.to_image(v, top), want)
        # the float32 form on the fp32 plane: one apart at the most, and only where the product is within its own fp32 rounding
        # (2^-24 relative) of a half
        v32 = v.astype(np.float32)
        d = (E.to_image_f32(v32, top) - E.to_image(v32.astype(np.float64), top))[:, :, ::-1]
        p = np.clip(v32.astype(np.float64), 0, 1) * top
        assert np.abs(d).max() <= 1 and (np.abs(p - np.floor(p) - 0.5)[d != 0] <= top * 2.0 ** -24).all()
    assert np.array_equal(E.crop(v, 16, 32).reshape(16, 32, 3), v[:16, :32])


OP_SETS = [(d, H, W) for d in DTYPES for H, W in E.OP_SHAPES] + [("f16", E.OP_WIDE_ROWS, E.wide_width())]    # (on another device the GPU test asserts the same of its own set)


@pytest.mark.parametrize("dtype,H,W", OP_SETS, ids=[f"{d}-{h}x{w}" for d, h, w in OP_SETS])
def test_op_inputs_meet_both_clamps_and_leave_few_bytes_open(dtype, H, W):
    _, _, _, _, v, Sm, _ = _op_reference(H, W, dtype)
    _, _, share = E.u8_window(v, E.bound_plane(Sm, fused=False))
    below, above = float((v < 0).mean()), float((v > 1).mean())
    print(f"{dtype} {H}x{W}: plane [{v.min():.2f}, {v.max():.2f}], {below:.3f} below 0, {above:.3f} above 1, open bytes {share:.4f}")
    assert share <= E.U8_WINDOW_SHARE
    if H * W >= 400:                                                  # (a handful of samples cannot meet both)
        assert below >= 0.01 and above >= 0.01


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_defects(dtype):
    H, W = 17, 31
    _, _, _, ht, v, Sm, (w_hr, b_hr, w_last, b_last) = _op_reference(H, W, dtype)
    tight = E.bound_plane(Sm, fused=True)
    # h outside the image as lrelu(bias): the ring of border samples leaves even the wider of the two plane bounds, nothing else moves
    vd, _ = E.conv_last(ht, E.rnd(w_last, dtype), b_last, "h_outside_lrelu_bias", b_hr)
    over = np.abs(vd - v) > E.bound_plane(Sm, fused=False)
    assert over[0].all() and over[-1].all() and over[:, 0].all() and over[:, -1].all() and not over[1:-1, 1:-1].any()
    # the crop with row stride W: the float plane leaves its bound (module docstring)
    good, bad = E.crop(v, 16, 30), E.crop(v, 16, 30, "crop_stride_W")
    assert (np.abs(bad - good) > E.crop(tight, 16, 30)).mean() > 0.9
    assert np.array_equal(E.crop(v, H, W, "crop_stride_W"), E.crop(v, H, W))         # (no crop, no difference)
    # truncation: the plane is untouched, so no plane bound sees it; the u8 window does, and so does the rint of the own plane
    lo, hi, _ = E.u8_window(v, E.bound_plane(Sm, fused=False))
    tr = E.to_image(v, 255, "truncate")[:, :, ::-1]
    assert ((tr < lo) | (tr > hi)).mean() > 0.3
    assert (E.to_image(v, 255, "truncate") != E.to_image_f32(v.astype(np.float32), 255)).mean() > 0.3
    ok = E.to_image(v, 255)[:, :, ::-1]
    assert ((ok >= lo) & (ok <= hi)).all()
    # x 255 on the 16-bit image
    lo, hi, share = E.u16_window(v, E.bound_plane(Sm, fused=False))
    bad = E.to_image(v, 65535, "top255_on_u16")[:, :, ::-1]
    assert ((bad < lo) | (bad > hi)).mean() > 0.9
    ok = E.to_image(v, 65535)[:, :, ::-1]
    assert ((ok >= lo) & (ok <= hi)).all()
    print(f"{dtype}: the u16 window is open for {share:.3f} of the samples")


def test_fused_bound_is_well_under_what_the_fused_against_unfused_test_allows():
    assert E.FUSED_ROUNDINGS == 2 + 2 + 3
    assert E.bound_plane(1.0, fused=True) + E.bound_plane(1.0, fused=False) < 2.0 ** -17 / 4


# ---- tail, engine level ----------------------------------------------------------------------------------------------------------------
def _torch_tail(feat, trunk, sd):
    c = lambda t, k: F.conv2d(t, torch.from_numpy(sd[k + ".weight"].astype(np.float64)), torch.from_numpy(sd[k + ".bias"].astype(np.float64)), padding=1)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    y = c(_nchw(trunk), "conv_body") + _nchw(feat)
    y = F.leaky_relu(c(up(y), "conv_up1"), 0.2)
    y = F.leaky_relu(c(up(y), "conv_up2"), 0.2)
    return _nhwc(c(F.leaky_relu(c(y, "conv_hr"), 0.2), "conv_last"))


def test_tail_exact_equals_torch():
    sd = E.ends_state(4)
    feat, trunk, _ = E.tail_inputs(5, 9)
    assert _close(E.tail_exact(feat, trunk, sd), _torch_tail(feat, trunk, sd))


PATHS = [(d, E.TailPath(p, w)) for d in DTYPES for p in (True, False) for w in (False, True) if not (w and (d != "f16" or not p))]


@pytest.mark.parametrize("scale", [4, 2])
def test_engine_inputs_meet_both_clamps(scale):
    sd = E.ends_state(scale)
    for (Ht, Wt), _ in E.TAIL_TRUNKS[scale]:
        if Ht * Wt < 32:
            continue
        feat, trunk, _ = E.tail_inputs(Ht, Wt)
        v = E.tail_exact(feat, trunk, sd)
        print(f"x{scale} {Ht}x{Wt}: plane [{v.min():.2f}, {v.max():.2f}], {(v < 0).mean():.4f} below 0, {(v > 1).mean():.4f} above 1")
        assert (v < 0).any() and (v > 1).any()


@pytest.mark.parametrize("dtype,path", PATHS, ids=[f"{d}-{'phase' if p.phase else 'gather'}{'-wino' if p.wino else ''}" for d, p in PATHS])
def test_tail_defects_leave_the_yardstick(dtype, path):
    sd = E.ends_state(4)
    feat, trunk, other = E.tail_inputs(5, 9)
    exact = E.tail_exact(feat, trunk, sd)
    rounded = E.tail_rounded(feat, trunk, sd, dtype, path)
    err, q, lim, merr, mlim = E.bounds(rounded, exact, rounded)
    assert 0 < q < 1e-2 * np.abs(exact).max() and err <= lim and merr <= mlim
    for defect in E.TAIL_DEFECTS:
        got = E.tail_rounded(feat, trunk, sd, dtype, path, defect, other)
        err, q, lim, merr, mlim = E.bounds(got, exact, rounded)
        print(f"{defect} {dtype} {path}: error / limit {err / lim:.1f}, mean error / limit {merr / mlim:.1f}")
        assert err > 10 * lim and merr > 10 * mlim, defect
        # the exact chain with the same defect moves the same way: the defect models are the float64 defects, rounded
        assert np.abs(got - E.tail_exact(feat, trunk, sd, defect, other)).max() <= 4 * np.abs(got - exact).max() * 2.0 ** -7


@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_and_gather_models_differ(dtype):
    """The phase kernels round the SUM of the taps once, the gathering form sums typed taps: different operands, so the GPU test claims
    no byte identity between FW_RRDB_UP_PHASE 0 and 1 and holds each to its own q."""
    sd = E.ends_state(4)
    for (Ht, Wt), _ in E.TAIL_TRUNKS[4]:
        feat, trunk, _ = E.tail_inputs(Ht, Wt)
        a = E.tail_rounded(feat, trunk, sd, dtype, E.TailPath(True, False))
        b = E.tail_rounded(feat, trunk, sd, dtype, E.TailPath(False, False))
        assert not np.array_equal(a, b)
