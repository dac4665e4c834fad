"""SRVGGNetCompact's two ends through the C-ABI (csrc/frame_ops.hip: fw_u8_to_nhwc, fw_pixel_shuffle_add_u8 at scales 1 to 4) against
tests/conv_epilogue_ref.py, and the engine at the scales 1, 2 and 3 that fw_srvgg_create accepts beside the published 4, against
oracle/srvgg_ref.py with the bounds tests/test_srvgg_gpu.py uses."""
import math

import numpy as np
import pytest
import torch

from framewright_amd import _lib
from framewright_amd import srvgg as S
from framewright_amd.synth import synthetic_frames
from oracle import srvgg_ref
import conv_epilogue_ref as R
from guarded import Guarded, dev, dtype_id, f32, ptr, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("cstride", [32, 40])
def test_u8_to_nhwc_every_level(hip_lib, dtype, cstride):
    img = R.levels_image()
    H, W, _ = img.shape
    out, dimg = Guarded(H * W * cstride, "u16"), dev(img)
    _lib.check(hip_lib.fw_u8_to_nhwc(dtype_id(dtype), ptr(dimg), H, W, out.ptr(), cstride, stream()))
    torch.cuda.synchronize()
    got = out.take().reshape(H, W, cstride)
    assert (got[:, :, 3:] == 0).all(), "channels [3, out_cstride) must be zeros"
    np.testing.assert_array_equal(got, R.u8_to_nhwc(img, dtype, cstride))          # typed(fp32(v) / fp32(255)), BGR -> RGB


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", R.TAIL_SHAPES)
def test_pixel_shuffle_add_u8(hip_lib, s, H, W):
    for cstride in (64, 3 * s * s):
        conv, img = R.tail_inputs(H, W, s, cstride)
        ref, bound = R.shuffle_tail(conv, img, s)
        lo, hi, _ = R.u8_window(ref, bound)
        lo, hi = lo[:, :, ::-1], hi[:, :, ::-1]                                     # BGR, as the bytes come out
        dconv, dimg = dev(conv), dev(img)
        n = H * s * W * s * 3
        res = {}
        for mode in ("u8", "f32", "both"):
            u8 = Guarded(n, "u8") if mode != "f32" else None
            rgb = Guarded(n, "f32") if mode != "u8" else None
            _lib.check(hip_lib.fw_pixel_shuffle_add_u8(ptr(dconv), cstride, ptr(dimg), H, W, s, u8.ptr() if u8 else None,
                                                       rgb.ptr() if rgb else None, stream()))
            torch.cuda.synchronize()
            res[mode] = (u8.take().reshape(H * s, W * s, 3) if u8 else None, f32(rgb.take()).reshape(H * s, W * s, 3) if rgb else None)
        for mode in ("f32", "both"):
            err = np.abs(res[mode][1].astype(np.float64) - ref)
            assert (err <= bound).all(), (mode, float((err / bound).max()))
        for mode in ("u8", "both"):
            b = res[mode][0].astype(np.int64)
            assert ((b >= lo) & (b <= hi)).all(), mode
        assert np.array_equal(res["u8"][0], res["both"][0]) and np.array_equal(res["f32"][1], res["both"][1])
        print(f"tail {H}x{W} s {s} cstride {cstride}: max |err| / bound = {float((np.abs(res['f32'][1] - ref) / bound).max()):.3f}")


def test_pixel_shuffle_add_rejects_a_short_channel_stride(hip_lib):
    d = torch.zeros(256, dtype=torch.float32, device="cuda")
    assert hip_lib.fw_pixel_shuffle_add_u8(ptr(d), 11, ptr(d), 1, 1, 2, ptr(d), None, stream()) != _lib.FW_OK       # 3 * 2^2 = 12 > 11
    assert hip_lib.fw_pixel_shuffle_add_u8(ptr(d), 64, ptr(d), 1, 1, 5, ptr(d), None, stream()) != _lib.FW_OK


def _oracle(sd, x_rgb, num_conv, scale):
    x = torch.from_numpy(x_rgb).permute(2, 0, 1).unsqueeze(0)
    with torch.no_grad():
        y = srvgg_ref.srvgg_forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, num_conv, scale)
    return y.squeeze(0).permute(1, 2, 0).numpy()


@pytest.mark.parametrize("dtype,max_abs,min_psnr", [("f16", 1e-3, 60.0), ("bf16", 1e-2, 50.0)])       # the bounds of test_srvgg_vs_oracle
@pytest.mark.parametrize("scale", [1, 2, 3])
def test_engine_at_the_other_scales(hip_lib, dtype, max_abs, min_psnr, scale):
    H, W = 13, 9
    sd = S.synthetic_srvgg_state(2, scale, seed=3)
    frame = synthetic_frames(1, H, W, seed=8)[0]
    eng = S.SRVGGNetEngine(2, scale, dtype)
    eng.load_state_dict(sd)
    rgb = torch.empty((H * scale, W * scale, 3), dtype=torch.float32, device="cuda")
    u8 = eng.upscale_device(torch.from_numpy(frame).cuda(), out_rgb_f32=rgb)
    torch.cuda.synchronize()
    want = _oracle(sd, frame[:, :, ::-1].astype(np.float32) / 255.0, 2, scale)
    got = rgb.cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() < max_abs
    want_u8 = np.rint(np.clip(want, 0, 1) * 255.0).astype(np.uint8)[:, :, ::-1]
    mse = np.mean((u8.cpu().numpy().astype(np.float64) - want_u8.astype(np.float64)) ** 2)
    assert (99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)) >= min_psnr
    assert want.std() > 0.05
    if scale == 2 and dtype == "f16":                        # the same through upscale on a 16-bit frame
        f16 = frame.astype(np.uint16) * 257 + 13
        got16 = eng.upscale(f16)
        assert got16.dtype == np.uint16 and got16.shape == (H * 2, W * 2, 3)
        want16 = np.rint(np.clip(_oracle(sd, f16[:, :, ::-1].astype(np.float32) / 65535.0, 2, 2), 0, 1) * 65535.0).astype(np.int64)[:, :, ::-1]
        assert np.abs(got16.astype(np.int64) - want16).max() <= 66                      # 1e-3 of the range
    eng.close()
