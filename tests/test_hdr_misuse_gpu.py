"""GPU: what `DeviceHDRConverter` and the `fw_hdr_*` entries refuse, in the project's wording, before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from framewright_amd import _lib
from framewright_amd import hdr as H

pytestmark = pytest.mark.gpu
WRONG = "hdr: uint8 or uint16 CUDA tensors H x W x 3 \\(BGR\\) expected"


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def conv(torch_mod):
    return H.DeviceHDRConverter()


def test_frames_that_are_refused(torch_mod, conv):
    torch = torch_mod
    good = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((16, 16, 3), dtype=torch.uint8),                         # a CPU tensor
                torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda"),        # a wrong dtype
                torch.zeros((16, 16), dtype=torch.uint8, device="cuda"),             # a gray frame
                torch.zeros((16, 16, 1), dtype=torch.uint8, device="cuda"),
                torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device="cuda"),
                np.zeros((16, 16, 3), np.uint8)):
        for call in (conv.convert_frame, lambda f: conv.convert_frames([good, f]), conv.tone_mapped_plane, conv.quantised_plane,
                     lambda f: list(conv.stream([f]))):
            with pytest.raises(ValueError, match=WRONG):
                call(bad)
    for shape in ((7, 16, 3), (16, 7, 3), (0, 16, 3)):                               # a side below 8
        with pytest.raises(ValueError, match="hdr: frames of 8 .. 16384 pixels a side expected"):
            conv.convert_frame(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="hdr: a uint8 CUDA tensor H x W on the converter's device expected"):
        conv.clahe(good)
    with pytest.raises(ValueError, match="hdr: frames of 8 .. 16384 pixels a side expected"):
        conv.clahe(good[:7, :, 0])
    with pytest.raises(ValueError, match="hdr: a float32 CUDA tensor on the converter's device expected"):
        conv.transfer(good)
    with pytest.raises(ValueError, match="hdr: a uint8 CUDA tensor \\[...\\] x 3 \\(BGR\\) on the converter's device expected"):
        conv.saturate(good[:, :, :2])
    with pytest.raises(ValueError, match="hdr: a uint8 or uint16 array H x W x 3 \\(BGR\\) expected"):
        conv.convert_numpy(np.zeros((16, 16), np.uint8))
    assert conv.convert_frame(good).shape == (16, 16, 3)                             # the converter still works


def test_a_frame_on_another_device_is_refused(torch_mod, conv):
    if torch_mod.cuda.device_count() < 2:
        # one GPU: the converter of a device that is not there cannot be made, and a frame cannot lie elsewhere; the check itself is
        # reached with a converter that believes it lives on device 1
        other = H.DeviceHDRConverter()
        other._dev, other.gpu_id = torch_mod.device("cuda", 1), 1
        with pytest.raises(ValueError, match="hdr: frames on cuda:1, the converter's device, expected"):
            other._check(torch_mod.zeros((16, 16, 3), dtype=torch_mod.uint8, device="cuda:0"))
        return
    with pytest.raises(ValueError, match="hdr: frames on cuda:0, the converter's device, expected"):
        conv.convert_frame(torch_mod.zeros((16, 16, 3), dtype=torch_mod.uint8, device="cuda:1"))


def test_config_misuse_never_reaches_the_device():
    for bad in ({"peak_brightness": 399}, {"saturation_boost": 1.6}, {"shadow_detail": 2.5}, {"tone_mapping": "filmic"}):
        with pytest.raises(ValueError):
            H.DeviceHDRConverter(H.HDRConfig(**bad))
    with pytest.raises(ValueError):
        H.create_hdr_converter("hdr11")
    made = H.create_hdr_converter("HLG", 600, "Hable", False)
    assert (made.config.target_format, made.config.peak_brightness, made.config.tone_mapping, made.config.enable_local_contrast) == \
        (H.HDRFormat.HLG, 600, H.ToneMapping.HABLE, False)


def test_the_c_abi_refuses_with_a_message(torch_mod, conv, hip_lib):
    torch = torch_mod
    src = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((16, 16, 3), dtype=torch.int16, device="cuda")
    params, gamma, tail, div = C.byref(conv._params[1]), _lib.ptr(conv._gamma[1]), _lib.ptr(conv._tail), _lib.ptr(conv._div)
    scratch = torch.zeros(int(hip_lib.fw_hdr_scratch_bytes(1)), dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr(src.device)

    def refused(status, text):
        assert status == _lib.FW_ERR_INVALID and text in hip_lib.fw_last_error().decode(), hip_lib.fw_last_error()

    table = lambda *t: _lib.ptr_table(t)                                             # noqa: E731
    call = hip_lib.fw_hdr_convert
    refused(call(table(src), table(dst), 1, 7, 16, 1, params, gamma, tail, div, _lib.ptr(scratch), st), "8 .. 16384 pixels a side expected")
    refused(call(table(src), table(dst), 1, 16, 16, 3, params, gamma, tail, div, _lib.ptr(scratch), st), "1 (uint8) or 2 (uint16) bytes a sample expected")
    refused(call(table(src), table(dst), 0, 16, 16, 1, params, gamma, tail, div, _lib.ptr(scratch), st), "1 .. 32 frames a call expected")
    refused(call(table(src), table(dst), 1, 16, 16, 1, None, gamma, tail, div, _lib.ptr(scratch), st), "null pointer")
    refused(call(table(src), table(dst), 1, 16, 16, 1, params, gamma, tail, div, None, st), "scratch")
    refused(call(table(src), table(src), 1, 16, 16, 1, params, gamma, tail, div, _lib.ptr(scratch), st), "overlaps")
    refused(call(table(src, src), table(dst, dst), 2, 16, 16, 1, params, gamma, tail, div, _lib.ptr(scratch), st), "overlaps")
    assert hip_lib.fw_hdr_scratch_bytes(0) == 0 and hip_lib.fw_hdr_scratch_bytes(33) == 0
    assert hip_lib.fw_hdr_scratch_bytes(2) == 2 * 64 * 256 * 5
    bad = H.make_params(H.HDRConfig(), 250)
    bad.curve = 4
    refused(call(table(src), table(dst), 1, 16, 16, 1, C.byref(bad), gamma, tail, div, _lib.ptr(scratch), st), "curve 0 (reinhard) .. 3 (mobius) expected")
    refused(hip_lib.fw_hdr_clahe_u8(_lib.ptr(src), 4, 16, _lib.ptr(scratch), _lib.ptr(dst), st), "8 .. 16384 pixels a side expected")
    refused(hip_lib.fw_hdr_saturation_u8(_lib.ptr(src), 0, div, 1.1, 0.0333, _lib.ptr(dst), st), "pixels expected")
    refused(hip_lib.fw_hdr_transfer_f32(None, 10, params, _lib.ptr(dst), st), "null pointer")
    refused(hip_lib.fw_hdr_tonemap_f32(_lib.ptr(src), 16, 16, 1, params, None, 0, _lib.ptr(dst), st), "null pointer")
    refused(hip_lib.fw_hdr_quantise_u8(_lib.ptr(src), 16, 20000, 1, params, gamma, _lib.ptr(dst), st), "8 .. 16384 pixels a side expected")
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0                                                 # nothing was launched
