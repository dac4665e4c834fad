"""The fused tail (csrc/conv3x3_hr_last.hip: conv_last(lrelu(conv_hr(x))) in one launch, the 64-channel map never stored) against
the two launches it replaces, at the op level through fw_conv3x3_hr_last_nhwc (fused 1 against 0) and at the engine level through
FW_RRDB_HR_LAST (1 against 0, against the fp32 oracle, and replayed from a hipGraph).

Op-level bound on the float planes: |fused - unfused| <= 2^-17 S per sample, S = |b| + sum |W_last| |h| in float64 from the
unfused call's own 64-channel map h.  Each path rounds fewer than 64 partial sums, each bounded by S, to fp32 (2^-24 relative
each); two fp32 orders of this sum on the CPU differ by at most 0.034 of the bound.  One f16 rounding flip in h moves a term by
2^-11 of its size and breaks it, so the bound also says that conv_hr's K loop kept its summation order.  The unfused form, the
reference here, gets a float64 reference of its own in tests/test_rrdb_tail_ops_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from framewright_amd import _lib
from framewright_amd import realesrgan as R
from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state
from oracle import rrdbnet_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 4096
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
TORCH_T = {"f16": torch.float16, "bf16": torch.bfloat16}
DT = {"f16": _lib.FW_DTYPE_F16, "bf16": _lib.FW_DTYPE_BF16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_pack(fn, *args):
    n = fn(*args, None)
    dst = np.zeros(n, np.uint16)
    assert n > 0 and fn(*args, C.c_void_p(dst.ctypes.data)) == n
    return torch.from_numpy(dst.view(np.int16)).cuda()


class Guarded:
    """An output image of n elements between two guards, everything filled with a pattern first."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.dev = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")

    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + GUARD * self.dev.element_size())

    def take(self):
        a = self.dev.cpu().numpy()
        guards = np.concatenate([a[:GUARD], a[GUARD + self.n:]])
        assert (guards == guards.dtype.type(self.fill)).all(), "written outside the image"
        return a[GUARD:GUARD + self.n].copy()


class Tail:
    """One tail problem: seeded input x (H, W, 64) in chunk-planar layout, the weights of synthetic_rrdbnet_state(1, 4, seed)."""

    def __init__(self, lib, dtype, H, W, seed):
        self.lib, self.dtype, self.H, self.W = lib, dtype, H, W
        tt = TORCH_T[dtype]
        sd = synthetic_rrdbnet_state(1, 4, seed)
        rng = np.random.default_rng(seed * 7919 + H * 31 + W)
        x = torch.from_numpy(rng.uniform(-1, 1, (H, W, 64)).astype(np.float32)).to(tt)
        self.x = x.reshape(H * W, 2, 32).permute(1, 0, 2).contiguous().cuda()
        w_hr = np.ascontiguousarray(sd["conv_hr.weight"], np.float32)
        self.w_last = np.ascontiguousarray(sd["conv_last.weight"], np.float32)
        self.b_last = sd["conv_last.bias"].astype(np.float32)
        pw = lambda w: C.c_void_p(w.ctypes.data)
        self.wp_hr = _host_pack(lambda *a: lib.fw_pack_conv3x3(DT[dtype], pw(w_hr), 64, 64, 2, 2, *a))
        self.wp_last = _host_pack(lambda *a: lib.fw_pack_conv3x3(DT[dtype], pw(self.w_last), 3, 64, 1, 2, *a))
        self.wp_pw = _host_pack(lambda *a: lib.fw_pack_conv_last_pointwise(DT[dtype], pw(self.w_last), *a))
        self.bias_hr = torch.from_numpy(sd["conv_hr.bias"].astype(np.float32)).cuda()
        b32 = np.zeros(32, np.float32)
        b32[:3] = self.b_last
        self.bias_last = torch.from_numpy(b32).cuda()
        self.u3 = torch.zeros((2, H * W, 32), dtype=tt, device="cuda")

    def run(self, fused, img_H=None, img_W=None, u16=False):
        """-> (float RGB plane, integer BGR image), both (img_H, img_W, 3); the guards around both are checked."""
        H, W = self.H, self.W
        img_H, img_W = img_H or H, img_W or W
        n = img_H * img_W * 3
        rgb = Guarded(n, torch.float32, -777.0)
        q = Guarded(n, torch.int16 if u16 else torch.uint8, 0x5A5A if u16 else 0x5A)
        st = self.lib.fw_conv3x3_hr_last_nhwc(DT[self.dtype], fused, P(self.x), 32, H * W * 32, H, W, P(self.wp_hr), P(self.bias_hr),
                                              P(self.wp_last), P(self.wp_pw), P(self.bias_last), P(self.u3), img_H, img_W,
                                              None if u16 else q.ptr(), q.ptr() if u16 else None, rgb.ptr(), _stream())
        assert st == 0, self.lib.fw_last_error()
        torch.cuda.synchronize()
        f = rgb.take().reshape(img_H, img_W, 3)
        i = q.take()
        i = (i.view(np.uint16) if u16 else i).reshape(img_H, img_W, 3)
        assert (f != np.float32(-777.0)).all(), "a sample of the image was not written"
        return f, i

    def bound_scale(self):
        """S (H, W, 3) in float64 from the 64-channel map the unfused call left in its scratch."""
        tt = TORCH_T[self.dtype]
        h = self.u3.cpu().to(torch.float64).permute(1, 0, 2).reshape(self.H, self.W, 64)
        w = torch.from_numpy(self.w_last).to(tt).to(torch.float64)   # the operand-typed weights both paths multiply by
        s = F.conv2d(h.abs().permute(2, 0, 1).unsqueeze(0), w.abs(), padding=1)[0].permute(1, 2, 0).numpy()
        return s + np.abs(self.b_last.astype(np.float64))


def _column_straddling_width():
    """83 rows are 6 steps; the width that gives 1.5 tiles per workgroup, so that runs start mid-column and cross column tops
    (1900 on 256 compute units)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return 30 * max(1, ncu // 4) - 20


# (H, W, variant): one step and one column, then one more in each direction; several of both; more tiles than workgroups
OP_CASES = [(1, 1, ""), (2, 3, ""), (15, 29, ""), (16, 30, ""), (17, 31, ""), (33, 61, ""), (83, None, ""), (33, 61, "u16"), (33, 61, "crop")]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("H,W,variant", OP_CASES, ids=[f"{h}x{w or 'wide'}{'-' + v if v else ''}" for h, w, v in OP_CASES])
def test_fused_tail_equals_the_two_launches(hip_lib, dtype, H, W, variant):
    W = W or _column_straddling_width()
    t = Tail(hip_lib, dtype, H, W, seed=1234)
    u16 = variant == "u16"
    img = (H - 1, W - 1) if variant == "crop" else (H, W)
    f0, i0 = t.run(0, *img, u16=u16)
    S = t.bound_scale()[:img[0], :img[1]]
    f1, i1 = t.run(1, *img, u16=u16)
    f2, i2 = t.run(1, *img, u16=u16)
    assert f1.tobytes() == f2.tobytes() and i1.tobytes() == i2.tobytes()   # determinism
    bound = 2.0 ** -17 * S
    err = np.abs(f1.astype(np.float64) - f0.astype(np.float64))
    print(f"{dtype} {H}x{W} {variant}: max |fused - unfused| / bound = {(err / bound).max():.4f}")
    assert np.isfinite(f1).all()
    assert (err <= bound).all(), f"{(err > bound).sum()} samples beyond 2^-17 S, worst {(err / bound).max():.3f} of it"
    # integer image: BGR of the same planes; at most 1 LSB apart, and only next to a rounding boundary
    scale = 65535.0 if u16 else 255.0
    d = np.abs(i1.astype(np.int64) - i0.astype(np.int64))[:, :, ::-1]
    assert d.max() <= 1
    v = np.clip(f0.astype(np.float64), 0.0, 1.0) * scale
    dist = np.abs(v - (np.floor(v) + 0.5))
    assert (dist[d > 0] <= scale * bound[d > 0]).all()


def _engine_outputs(sd, frame, nb, scale):
    """A new engine (it reads its switches from the environment when it is created) -> (float RGB, uint8 BGR) of one frame."""
    eng = R.RRDBNetEngine(nb, scale, "f16")
    eng.load_state_dict(sd)
    t = torch.from_numpy(frame).cuda()
    rgb = torch.empty((frame.shape[0] * scale, frame.shape[1] * scale, 3), dtype=torch.float32, device="cuda")
    u8 = torch.empty(rgb.shape, dtype=torch.uint8, device="cuda")
    eng.upscale_device(t, out=u8, out_rgb_f32=rgb)
    torch.cuda.synchronize()
    eng.close()
    return rgb.cpu().numpy(), u8.cpu().numpy()


def _oracle(sd, frame, nb, scale):
    x = torch.from_numpy(frame[:, :, ::-1].astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    if scale == 2:
        x = F.pad(x, (0, x.shape[3] % 2, 0, x.shape[2] % 2), "reflect")
    with torch.no_grad():
        y = ref.rrdbnet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, x, nb, scale)
    return y[:, :, :frame.shape[0] * scale, :frame.shape[1] * scale].squeeze(0).permute(1, 2, 0).numpy()


# (scale, H, W, against the oracle too): 21x475 has more tiles than workgroups; 37x45 at x2 is the mod-pad crop
@pytest.mark.parametrize("scale,H,W,with_oracle", [(4, 40, 56, True), (4, 21, 475, False), (2, 37, 45, True)])
def test_engine_fused_tail_equals_unfused(hip_lib, monkeypatch, scale, H, W, with_oracle):
    sd = synthetic_rrdbnet_state(2, scale, seed=H * 1000 + W)
    frame = synthetic_frames(1, H, W, seed=W)[0]
    outs = []
    for v in ("1", "0"):
        monkeypatch.setenv("FW_RRDB_HR_LAST", v)
        outs.append(_engine_outputs(sd, frame, 2, scale))
    (rgb_a, u8_a), (rgb_b, u8_b) = outs
    assert np.isfinite(rgb_a).all()
    print(f"x{scale} {H}x{W}: fused against unfused max-abs {np.abs(rgb_a - rgb_b).max():.3g}")
    assert np.abs(rgb_a - rgb_b).max() < 2e-4
    assert np.abs(u8_a.astype(int) - u8_b.astype(int)).max() <= 1
    if with_oracle:
        want = _oracle(sd, frame, 2, scale)
        print(f"x{scale} {H}x{W}: fused against the oracle max-abs {np.abs(rgb_a - want).max():.3g}")
        assert np.abs(rgb_a - want).max() < 1e-3


def test_engine_fused_tail_from_a_graph_equals_direct_launches(hip_lib, monkeypatch):
    sd = synthetic_rrdbnet_state(2, 4, seed=8)
    frame = synthetic_frames(1, 40, 56, seed=3)[0]
    monkeypatch.setenv("FW_RRDB_HR_LAST", "1")
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("FW_RRDB_GRAPH", mode)
        outs.append(_engine_outputs(sd, frame, 2, 4))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
