"""fw_conv3x3_nhwc_ex, the only C-ABI route to PReLU (act == 2), to chan_scale in front of the residual add, to post_act and to
f32_cstride / f32_coff (csrc/conv3x3_mfma.hip), against the float64 restatements and per-element bounds of tests/conv_epilogue_ref.py,
in f16 and bf16.  Every output buffer is pre-filled with a sentinel and guarded on both sides (tests/guarded.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from framewright_amd import _lib
import conv_epilogue_ref as R
from guarded import Guarded, dev, dtype_id, f32, ptr, stream, untouched

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]


def _pack(lib, dtype, w, ct, ch):
    cout, cin = w.shape[:2]
    n = lib.fw_pack_conv3x3(dtype_id(dtype), None, cout, cin, ct, ch, None)
    dst = np.zeros(n, np.uint16)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.fw_pack_conv3x3(dtype_id(dtype), C.c_void_p(wc.ctypes.data), cout, cin, ct, ch, C.c_void_p(dst.ctypes.data)) == n
    return dev(dst)


def _ex(lib, dtype, x, ch, H, W, wp, bias, ct, act, res1, s1, res2, s2, cs, post_act, f32_cstride, f32_coff, out, out_cstride, out_f32):
    return lib.fw_conv3x3_nhwc_ex(dtype_id(dtype), ptr(x), 32 * ch, 0, ch, H, W, ptr(wp), ptr(bias), ct, act, 0, res1, s1, res2, s2,
                                  ptr(cs) if cs is not None else None, post_act, f32_cstride, f32_coff, out, out_cstride, 0, 0, out_f32, stream())


def _report(name, err, bound, count):
    A = bound / R.gamma(count)
    print(f"{name}: max |err| / (2^-24 A) = {float((err / np.maximum(2.0 ** -24 * A, 1e-300)).max()):.2f}, "
          f"max |err| / bound = {float((err / bound).max()):.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ct", [1, 2])
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("H,W", R.CONV_SHAPES)
def test_prelu(hip_lib, dtype, ct, chunks, H, W):
    xb, w, b, xv, wv = R.conv_inputs(H, W, chunks, ct, dtype)
    slopes = R.channel_vector(32 * ct, 1)
    N, ocs = 32 * ct, 32 * ct + 8
    x, wp, bias, cs = dev(xb), _pack(hip_lib, dtype, w, ct, chunks), dev(b), dev(slopes)
    t, A = R.conv3x3(xv, wv, b)
    ref, bound = R.prelu(t, A, slopes, chunks)
    assert (ref > 0).any() and ((ref < 0).any() or H * W == 1)
    # typed store plus the fp32 copy
    out, o32 = Guarded(H * W * ocs, "u16"), Guarded(H * W * N, "f32")
    _lib.check(_ex(hip_lib, dtype, x, chunks, H, W, wp, bias, ct, 2, None, 1.0, None, 1.0, cs, 0, 0, 0, out.ptr(), ocs, o32.ptr()))
    # out == NULL, out_f32 only: SRVGG's last conv
    only = Guarded(H * W * N, "f32")
    _lib.check(_ex(hip_lib, dtype, x, chunks, H, W, wp, bias, ct, 2, None, 1.0, None, 1.0, cs, 0, 0, 0, None, 0, only.ptr()))
    torch.cuda.synchronize()
    got32 = f32(o32.take()).reshape(H, W, N)
    err = np.abs(got32.astype(np.float64) - ref)
    _report(f"PReLU {H}x{W} chunks {chunks} tiles {ct} {dtype}", err, bound, 9 * chunks + 1)
    assert np.isfinite(got32).all() and (err <= bound).all()
    typed = out.take().reshape(H, W, ocs)
    assert untouched(typed[:, :, N:], "u16"), "lanes behind 32 * cout_tiles were written"
    np.testing.assert_array_equal(typed[:, :, :N], R.to_bits(got32, dtype))
    np.testing.assert_array_equal(only.take(), got32.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("H,W", R.CONV_SHAPES)
def test_residual_with_chan_scale(hip_lib, dtype, chunks, H, W):
    xb, w, b, xv, wv = R.conv_inputs(H, W, chunks, 2, dtype)
    beta = R.channel_vector(64, 2)
    r1, r2 = R.residual_buffers(H, W)
    x, wp, bias, cs, d1, d2 = dev(xb), _pack(hip_lib, dtype, w, 2, chunks), dev(b), dev(beta), dev(r1), dev(r2)
    t, A = R.conv3x3(xv, wv, b)
    for post_act in (0, 1):
        for two in (False, True):
            out, o32 = Guarded(H * W * 72, "u16"), Guarded(H * W * 160, "f32")
            _lib.check(_ex(hip_lib, dtype, x, chunks, H, W, wp, bias, 2, 0, ptr(d1), 0.2, ptr(d2) if two else None, 0.5, cs, post_act, 160, 64,
                           out.ptr(), 72, o32.ptr()))
            torch.cuda.synchronize()
            kw = dict(s2=0.5, res2=r2[:, :, 64:128]) if two else {}
            ref, bound = R.residual(t, A, chunks, beta, 0.2, r1[:, :, 64:128], post_act=post_act, **kw)
            wide = o32.take().reshape(H, W, 160)
            assert untouched(wide[:, :, :64], "f32") and untouched(wide[:, :, 128:], "f32"), "fp32 channels outside [64, 128) were written"
            got32 = f32(wide[:, :, 64:128])
            err = np.abs(got32.astype(np.float64) - ref)
            _report(f"residual {H}x{W} chunks {chunks} post_act {post_act} res2 {two} {dtype}", err, bound, 9 * chunks + 6)
            assert np.isfinite(got32).all() and (err <= bound).all()
            typed = out.take().reshape(H, W, 72)
            assert untouched(typed[:, :, 64:], "u16")
            np.testing.assert_array_equal(typed[:, :, :64], R.to_bits(got32, dtype))
            if post_act:
                assert (ref < 0).any() or H * W == 1                      # the activation's branch is met
    np.testing.assert_array_equal(d1.cpu().numpy(), r1)                    # the residual buffers are read only
    np.testing.assert_array_equal(d2.cpu().numpy(), r2)


def test_prelu_argument_errors(hip_lib):
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = ptr(d)
    call = lambda act, res1, cs: hip_lib.fw_conv3x3_nhwc_ex(_lib.FW_DTYPE_F16, p, 64, 0, 2, 4, 4, p, p, 2, act, 0, res1, 1.0, None, 1.0, cs, 0,
                                                            0, 0, p, 64, 0, 0, None, stream())
    assert call(2, None, None) == _lib.FW_ERR_INVALID and b"PReLU" in hip_lib.fw_last_error()      # no slopes
    assert call(2, p, p) == _lib.FW_ERR_INVALID and b"PReLU" in hip_lib.fw_last_error()            # with a residual
    torch.cuda.synchronize()
    assert bool((d == 0).all())
