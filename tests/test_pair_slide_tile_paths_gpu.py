"""The window pair kernel (csrc/conv3x3_pair_slide.hip) on the paths between its items: the warm-up that fills the carried
x_a rows of a run starting mid-column, the carry hand-over from tile to tile, runs that wrap from the bottom of one column to
the top of the next, stores that retire behind the next tile's first item, and partial last tile rows / columns.

The ring kernel (csrc/conv3x3_pair.hip) is the same computation with no carry and no warm-up, and accumulates every output in
the same order, so the expected difference is exactly zero bytes.  Tiles are 16 rows x 30 columns, tiles_y = (H + 16) / 16, a
launch has at most one workgroup per CU (256) and a workgroup's run is contiguous in the column-major tile index:

  H = 80,  W = 90:  6 x 3 = 18 tiles, one per workgroup: every run below a column top is a warm-up followed by a single tile
  H = 320, W = 390: 21 x 13 = 273 tiles on 256 workgroups: runs of one and two tiles, some across a column wrap
  H = 77,  W = 61:  a partial last tile row and a partial last tile column (30 + 30 + 1)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from framewright_amd import _lib

pytestmark = pytest.mark.gpu

TDT = {_lib.FW_DTYPE_BF16: torch.bfloat16, _lib.FW_DTYPE_F16: torch.float16}
# tests/test_conv3x3_gpu.py::test_conv_pair_fused: x_a within TOL, x_b within 2 TOL of the fp32 reference on rounded operands
TOL = {_lib.FW_DTYPE_BF16: 2e-2, _lib.FW_DTYPE_F16: 3e-3}
SHAPES = [(80, 90), (320, 390), (77, 61)]


def _pack(lib, dtype, w, ch):
    cout, cin = w.shape[:2]
    n = lib.fw_pack_conv3x3(dtype, None, cout, cin, 1, ch, None)
    dst = np.zeros(n, np.uint16)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.fw_pack_conv3x3(dtype, C.c_void_p(wc.ctypes.data), cout, cin, 1, ch, C.c_void_p(dst.ctypes.data)) == n
    return torch.from_numpy(dst.view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def _problem(dtype, na, H, W):
    rng = np.random.default_rng(1000 * na + 7 * H + W)
    cin = 32 * na
    x = torch.from_numpy(rng.standard_normal((na, H, W, 32)).astype(np.float32)).cuda().to(TDT[dtype])
    wa = (rng.standard_normal((32, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    wb = (rng.standard_normal((32, cin + 32, 3, 3)) / np.sqrt(9 * (cin + 32))).astype(np.float32)
    ba, bb = rng.standard_normal(32).astype(np.float32), rng.standard_normal(32).astype(np.float32)
    return x, wa, wb, ba, bb


def _run(lib, dtype, na, H, W, slide, monkeypatch):
    x, wa, wb, ba, bb = _problem(dtype, na, H, W)
    monkeypatch.setenv("FW_PAIR_SLIDE", slide)
    pa, pb = _pack(lib, dtype, wa, na), _pack(lib, dtype, wb, na + 1)
    ta, tb = torch.from_numpy(ba).cuda(), torch.from_numpy(bb).cuda()
    oa = torch.full((H, W, 32), 5.0, dtype=TDT[dtype], device="cuda")
    ob = torch.full((H, W, 32), 5.0, dtype=TDT[dtype], device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.fw_conv3x3_pair_nhwc(dtype, p(x), 32, H * W * 32, na, H, W, p(pa), p(ta), p(pb), p(tb), p(oa), p(ob), 32, None))
    torch.cuda.synchronize()
    return oa, ob


def _assert_same_bytes(got, want, what):
    same = torch.equal(got.view(torch.int16), want.view(torch.int16))
    if not same:
        bad = (got.view(torch.int16) != want.view(torch.int16)).any(dim=2).nonzero()
        rows, cols = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, 1].tolist()))
        pytest.fail(f"{what}: {bad.shape[0]} pixels differ from the ring kernel; rows {rows[:12]} columns {cols[:12]}")


@pytest.mark.parametrize("dtype", [_lib.FW_DTYPE_F16, _lib.FW_DTYPE_BF16])
@pytest.mark.parametrize("na", [2, 4])   # 64 -> 32 / 96 -> 32 and 128 -> 32 / 160 -> 32
@pytest.mark.parametrize("H,W", SHAPES)
def test_window_kernel_matches_ring_kernel_bytes(hip_lib, dtype, na, H, W, monkeypatch):
    ring_a, ring_b = _run(hip_lib, dtype, na, H, W, "0", monkeypatch)
    win_a, win_b = _run(hip_lib, dtype, na, H, W, "1", monkeypatch)
    _assert_same_bytes(win_a, ring_a, "x_a")
    _assert_same_bytes(win_b, ring_b, "x_b")


@pytest.mark.parametrize("na", [1, 3, 7])
def test_warm_up_batches_of_other_chunk_counts(hip_lib, na, monkeypatch):
    """The warm-up takes its chunks in batches of four, then three: one chunk, a short batch, and two batches that use every
    weight slot (the launcher takes 1 to 8 shared chunks; RRDBNet has 2 and 4)."""
    H, W = SHAPES[0]
    ring_a, ring_b = _run(hip_lib, _lib.FW_DTYPE_F16, na, H, W, "0", monkeypatch)
    win_a, win_b = _run(hip_lib, _lib.FW_DTYPE_F16, na, H, W, "1", monkeypatch)
    _assert_same_bytes(win_a, ring_a, "x_a")
    _assert_same_bytes(win_b, ring_b, "x_b")


@pytest.mark.parametrize("dtype", [_lib.FW_DTYPE_F16, _lib.FW_DTYPE_BF16])
@pytest.mark.parametrize("na", [2, 4])
def test_window_kernel_against_fp32_reference(hip_lib, dtype, na, monkeypatch):
    H, W = SHAPES[0]
    x, wa, wb, ba, bb = _problem(dtype, na, H, W)
    win_a, win_b = _run(hip_lib, dtype, na, H, W, "1", monkeypatch)

    def conv(inp_hwc, w, b):
        wq = torch.from_numpy(w).cuda().to(TDT[dtype]).float()
        y = F.conv2d(inp_hwc.float().permute(2, 0, 1).unsqueeze(0), wq, torch.from_numpy(b).cuda(), 1, 1)
        return F.leaky_relu(y, 0.2).squeeze(0).permute(1, 2, 0)

    x_hwc = x.permute(1, 2, 0, 3).reshape(H, W, 32 * na)
    ref_a = conv(x_hwc, wa, ba)
    ref_b = conv(torch.cat([x_hwc, ref_a.to(TDT[dtype])], dim=2), wb, bb)
    err_a = (win_a.float() - ref_a).abs().max().item()
    err_b = (win_b.float() - ref_b).abs().max().item()
    print(f"x_a max-abs {err_a:.3e} (bound {TOL[dtype]:.0e}), x_b max-abs {err_b:.3e} (bound {2 * TOL[dtype]:.0e})")
    assert err_a < TOL[dtype]
    assert err_b < 2 * TOL[dtype]
