"""The RRDBNet's tail kernels on their own, each against float64: fw_conv3x3_hr_last_nhwc with fused = 0 (conv3x3_mfma.hip's EPI_STORE
and EPI_IMAGE launches) and fused = 1 (conv3x3_hr_last.hip), f16 and bf16, chunk-planar input, every output between guards.
tests/test_tail_fused_gpu.py compares the two forms with each other; here each has a reference of its own (tests/rrdb_ends_ref.py,
whose docstring counts the bounds):

  * the scratch h of the unfused form within typed_allowance(h_ref, gamma(19) A_h) of the float64 h;
  * the float plane of each form within gamma(19) S (unfused) / gamma(8) S (fused) of float64 conv_last of THAT scratch, every sample;
  * the u8 and u16 images, both written by the same launch, bit for bit rint(clip(plane, 0, 1) * top) in float32 from the launch's own
    float plane, BGR; the u8 image inside u8_window of the float64 reference at the form's own plane bound, the u16 image inside u16_window
    (lo <= got <= hi).

conv_last.weight is 8 times test_tail_fused_gpu's, so that the plane meets both clamps (tests/test_rrdb_ends_ref_host.py asserts it, and
the share of bytes the bound leaves open, for every input set used here).  The fused form gets the scratch too and must leave it alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guarded
import rrdb_ends_ref as E
from framewright_amd import _lib
from test_tail_fused_gpu import _column_straddling_width, _host_pack

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(H, W, dtype):
    """(x bits, weights, h_ref, A_h), computed once per input set and left unchanged."""
    xb, x, w_hr, b_hr, w_last, b_last = E.tail_op_inputs(H, W, dtype)
    h, A_h = E.conv_hr(x, E.rnd(w_hr, dtype), b_hr)
    return xb, (w_hr, b_hr, w_last, b_last), h, A_h


class Problem:
    def __init__(self, lib, dtype, H, W):
        self.lib, self.dtype, self.H, self.W = lib, dtype, H, W
        xb, (w_hr, b_hr, w_last, b_last), self.h_ref, self.A_h = _reference(H, W, dtype)
        self.w_last, self.b_last = w_last, b_last
        self.x = guarded.dev(np.ascontiguousarray(xb.reshape(H * W, 2, 32).transpose(1, 0, 2)))      # chunk-planar [2][H * W][32]
        dt = guarded.dtype_id(dtype)
        pw = lambda w: C.c_void_p(w.ctypes.data)
        self.wp_hr = _host_pack(lambda *a: lib.fw_pack_conv3x3(dt, pw(w_hr), 64, 64, 2, 2, *a))
        self.wp_last = _host_pack(lambda *a: lib.fw_pack_conv3x3(dt, pw(w_last), 3, 64, 1, 2, *a))
        self.wp_pw = _host_pack(lambda *a: lib.fw_pack_conv_last_pointwise(dt, pw(w_last), *a))
        self.bias_hr = guarded.dev(b_hr)
        b32 = np.zeros(32, np.float32)
        b32[:3] = b_last
        self.bias_last = guarded.dev(b32)

    def call(self, fused, img, u3, u8, u16, rgb):
        H, W = self.H, self.W
        p = lambda g: g.ptr() if g is not None else None
        return self.lib.fw_conv3x3_hr_last_nhwc(guarded.dtype_id(self.dtype), fused, guarded.ptr(self.x), 32, H * W * 32, H, W, guarded.ptr(self.wp_hr),
                                                guarded.ptr(self.bias_hr), guarded.ptr(self.wp_last), guarded.ptr(self.wp_pw), guarded.ptr(self.bias_last),
                                                p(u3), img[0], img[1], p(u8), p(u16), p(rgb), guarded.stream())

    def run(self, fused, img=None):
        """One launch that writes all three outputs -> (scratch bits (H, W, 64) or None, float plane, u8 image, u16 image), the last
        three (img_H, img_W, 3); every guard checked, every sample written, the fused form's scratch untouched."""
        H, W = self.H, self.W
        img = img or (H, W)
        n = img[0] * img[1] * 3
        u3, u8, u16, rgb = guarded.Guarded(2 * H * W * 32, "u16"), guarded.Guarded(n, "u8"), guarded.Guarded(n, "u16"), guarded.Guarded(n, "f32")
        assert self.call(fused, img, u3, u8, u16, rgb) == _lib.FW_OK, self.lib.fw_last_error()
        torch.cuda.synchronize()
        s, f = u3.take(), rgb.take()
        assert not (f == guarded.SENT["f32"]).any(), "a sample of the float plane was not written"
        if fused:
            assert guarded.untouched(s, "u16"), "the fused form wrote to the scratch"
            s = None
        else:
            assert not (s == guarded.SENT["u16"]).any(), "an element of the scratch was not written"
            s = s.reshape(2, H * W, 32).transpose(1, 0, 2).reshape(H, W, 64)
        return s, guarded.f32(f).reshape(img + (3,)), u8.take().reshape(img + (3,)), u16.take().reshape(img + (3,))


def _check(name, t, img=None):
    """Both forms of one problem against float64; returns the printed ratios."""
    H, W, dtype = t.H, t.W, t.dtype
    img = img or (H, W)
    scratch, f0, b0, s0 = t.run(0, img)
    # the unfused h against the float64 h
    h = E.from_bits(scratch, dtype).reshape(H, W, 64)
    eh = np.abs(h - t.h_ref)
    allow = E.allow_h(t.h_ref, t.A_h, dtype)
    # float64 conv_last of that scratch: the reference of both float planes
    v, Sm = E.conv_last(h, E.rnd(t.w_last, dtype), t.b_last)
    v, Sm = v[:img[0], :img[1]], Sm[:img[0], :img[1]]
    if H * W >= 400:                                                  # both clamps are met by the input set this device runs
        assert (v < 0).mean() >= 0.01 and (v > 1).mean() >= 0.01, ((v < 0).mean(), (v > 1).mean())
    _, f1, b1, s1 = t.run(1, img)
    line, bad = [f"h {(eh / allow).max():.3f}"], []
    if not (eh <= allow).all():
        bad.append(("h", int((eh > allow).sum()), float((eh / allow).max())))
    for fused, f, b8, b16 in ((0, f0, b0, s0), (1, f1, b1, s1)):
        form = "fused" if fused else "unfused"
        assert np.isfinite(f).all()
        bound = E.bound_plane(Sm, bool(fused))
        err = np.abs(f.astype(np.float64) - v)
        line.append(f"{form} plane {(err / bound).max():.3f}")
        if not (err <= bound).all():
            bad.append((form, "plane", int((err > bound).sum()), float((err / bound).max())))
        # the images: from the launch's own plane, bit for bit; and inside the reference's windows
        if not np.array_equal(b8.astype(np.int64), E.to_image_f32(f, 255)):
            bad.append((form, "u8 is not rint of the own plane", int((b8 != E.to_image_f32(f, 255)).sum())))
        if not np.array_equal(b16.astype(np.int64), E.to_image_f32(f, 65535)):
            bad.append((form, "u16 is not rint of the own plane", int((b16 != E.to_image_f32(f, 65535)).sum())))
        lo, hi, share = E.u8_window(v, bound)
        assert share <= E.U8_WINDOW_SHARE, (form, share)             # (the host test asserts it of the float64 h, here it is the scratch's)
        got = b8.astype(np.int64)[:, :, ::-1]
        if not ((lo <= got) & (got <= hi)).all():
            bad.append((form, "u8 outside its window", int(((got < lo) | (got > hi)).sum())))
        lo, hi, _ = E.u16_window(v, bound)
        got = b16.astype(np.int64)[:, :, ::-1]
        if not ((lo <= got) & (got <= hi)).all():
            bad.append((form, "u16 outside its window", int(((got < lo) | (got > hi)).sum())))
    print(f"{name} {dtype} {H}x{W} -> {img[0]}x{img[1]}: max |err| / bound: " + ", ".join(line))
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("H,W", E.OP_SHAPES, ids=[f"{h}x{w}" for h, w in E.OP_SHAPES])
def test_tail_kernels_against_float64(hip_lib, dtype, H, W):
    """Measured on an MI355X: DESIGN.md (What pins the RRDBNet's two ends)."""
    _check("whole", Problem(hip_lib, dtype, H, W))


def test_tail_kernels_against_float64_more_tiles_than_workgroups(hip_lib):
    """83 rows at the width that gives 1.5 tiles per workgroup: runs of the fused kernel that start mid-column (f16 only: the float64
    reference of this one case is 12 GFLOP)."""
    W = _column_straddling_width()
    assert W == E.wide_width(torch.cuda.get_device_properties(0).multi_processor_count)      # the host test checks this set at 256 compute units
    _check("wide", Problem(hip_lib, "f16", E.OP_WIDE_ROWS, W))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("full,img", E.OP_CROPS, ids=[f"{f[0]}x{f[1]}-to-{i[0]}x{i[1]}" for f, i in E.OP_CROPS])
def test_tail_kernels_crop(hip_lib, dtype, full, img):
    """The x2 model's crop: 17x33 -> 16x32 leaves a whole tile row and column of the unfused form outside the image, 17x31 -> 16x30 of
    the fused form.  Row stride img_W: a stride of W would misplace every row but the first and write past the guard."""
    _check("crop", Problem(hip_lib, dtype, *full), img)


def test_tail_entry_refuses_what_it_cannot_run(hip_lib):
    t = Problem(hip_lib, "f16", 5, 7)
    n = 5 * 7 * 3
    u3, rgb = guarded.Guarded(2 * 5 * 7 * 32, "u16"), guarded.Guarded(n, "f32")
    for fused in (0, 1):
        assert t.call(fused, (5, 7), u3, None, None, None) == _lib.FW_ERR_INVALID and b"no output" in hip_lib.fw_last_error()
        for img in ((6, 7), (5, 8), (0, 7), (5, 0)):
            assert t.call(fused, img, u3, None, None, rgb) == _lib.FW_ERR_INVALID and b"size" in hip_lib.fw_last_error(), img
    torch.cuda.synchronize()
    assert guarded.untouched(rgb.take(), "f32") and guarded.untouched(u3.take(), "u16"), "a refused call launched something"
