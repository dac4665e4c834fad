"""IFNet at the engine level, block by block: the flow and mask each IFBlock leaves behind (fw_ifnet_last_flow) against the float64
oracle, arbitrary timesteps, and the hipGraph cache's key.

Per-block flow.  With lastconv's weight and bias zeroed for blocks k + 1 .. 3 those blocks add exactly zero, so the flow and mask
read out after a forward are block k's cumulative result.  They are compared with oracle/ifnet_ref.py run in float64.  The yardstick
is not a fixed number: the same float64 oracle is run once more with the conv weights and every conv input rounded to the operand
type (the operand-rounded model), q = max |rounded - exact| per block, and the engine must satisfy

    max |engine - exact| <= 2 q + 1e-6 max |exact|

for the flow and for the mask.  The factor 2 covers what the model leaves out: the accumulation order of the fp32 accumulator, the
hi + lo split of the 64-channel block's trunk and beta folded into its weights.  A wrong scale factor in one block's increment or a
mask taken from the wrong lastconv row shows up here at the block that has it, at the default flow gain.  Parity vs upstream
(rife-ncnn-vulkan) stays unpinned."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from framewright_amd import rife as RF
from framewright_amd.synth import synthetic_frames, synthetic_ifnet_state
from oracle import ifnet_ref

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}


class _RoundingF:
    """torch.nn.functional whose convolutions round their input to the operand type first."""

    def __init__(self, tdt):
        self.tdt = tdt

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, *a, **k):
        return F.conv2d(x.to(self.tdt).double(), *a, **k)

    def conv_transpose2d(self, x, *a, **k):
        return F.conv_transpose2d(x.to(self.tdt).double(), *a, **k)


def _frames64(fr):
    t = lambda f: torch.from_numpy(f[:, :, ::-1].astype(np.float64) / 255.0).permute(2, 0, 1).unsqueeze(0)
    return t(fr[0]), t(fr[1])


def _block_flows(sd, img0, img1, timestep):
    """oracle.ifnet_ref.ifnet_forward's loop (its own ifblock and warp), keeping the flow and mask after every block: float64,
    padded frame, [(Hp, Wp, 4), (Hp, Wp)] x 4."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # ifnet_ref.warp's base grid and the timestep plane
    try:
        _, _, h, w = img0.shape
        ph, pw = ((h - 1) // 32 + 1) * 32, ((w - 1) // 32 + 1) * 32
        i0, i1 = F.pad(img0, (0, pw - w, 0, ph - h)), F.pad(img1, (0, pw - w, 0, ph - h))
        t = torch.full((1, 1, ph, pw), float(timestep))
        flow = mask = None
        w0, w1 = i0, i1
        out = []
        with torch.no_grad():
            for i, s in enumerate(ifnet_ref.SCALES):
                if flow is None:
                    flow, mask = ifnet_ref.ifblock(sd, f"block{i}.", torch.cat([i0, i1, t], 1), None, s)
                else:
                    fd, md = ifnet_ref.ifblock(sd, f"block{i}.", torch.cat([w0, w1, t, mask], 1), flow, s)
                    flow, mask = flow + fd, mask + md
                w0, w1 = ifnet_ref.warp(i0, flow[:, :2]), ifnet_ref.warp(i1, flow[:, 2:4])
                out.append((flow[0].permute(1, 2, 0).numpy().copy(), mask[0, 0].numpy().copy()))
        return out
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def _exact(H, W, gain):
    sd = {k: torch.from_numpy(v).double() for k, v in synthetic_ifnet_state(seed=2468, flow_gain=gain).items()}
    return _block_flows(sd, *_frames64(synthetic_frames(2, H, W, seed=H)), 0.5)


def _rounded(H, W, gain, dtype, monkeypatch):
    tdt = TDT[dtype]
    sd = {k: (torch.from_numpy(v).to(tdt).double() if k.endswith("conv.weight") or k.endswith(".0.weight") else torch.from_numpy(v).double())
          for k, v in synthetic_ifnet_state(seed=2468, flow_gain=gain).items()}
    with monkeypatch.context() as m:
        m.setattr(ifnet_ref, "F", _RoundingF(tdt))
        return _block_flows(sd, *_frames64(synthetic_frames(2, H, W, seed=H)), 0.5)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("gain", [1.0, 12.0])
@pytest.mark.parametrize("H,W", [(64, 96), (70, 100), (192, 256)])
def test_per_block_flow_and_mask_against_the_float64_oracle(hip_lib, monkeypatch, H, W, gain, dtype):
    """Measured on an MI355X: error / (2 q + 1e-6 max |exact|) between 0.44 and 0.59 for every block, size, gain, type and engine
    configuration (the engine's error equals the model's q); DESIGN.md (K7) holds the table."""
    sd = synthetic_ifnet_state(seed=2468, flow_gain=gain)
    fr = synthetic_frames(2, H, W, seed=H)
    a, b = torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1]).cuda()
    exact, rounded = _exact(H, W, gain), _rounded(H, W, gain, dtype, monkeypatch)
    failures = []
    for k in range(4):
        sdk = dict(sd)
        for j in range(k + 1, 4):
            for key in (f"block{j}.lastconv.0.weight", f"block{j}.lastconv.0.bias"):
                sdk[key] = np.zeros_like(sd[key])
        configs = [("1", "1")] if k < 3 else [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")]
        for fuse, split in configs:
            monkeypatch.setenv("FW_IFNET_FUSE_GLUE", fuse)
            monkeypatch.setenv("FW_IFNET_SPLIT_TRUNK", split)
            eng = RF.IFNetEngine(dtype)
            eng.load_state_dict(sdk)
            eng.interpolate_device(a, b, 0.5)
            flow, mask = eng.last_flow(H, W)
            torch.cuda.synchronize()
            got = (flow.cpu().numpy().astype(np.float64), mask.cpu().numpy().astype(np.float64))
            eng.close()
            for name, g, e, r in (("flow", got[0], exact[k][0], rounded[k][0]), ("mask", got[1], exact[k][1], rounded[k][1])):
                assert g.shape == e.shape
                err, q = np.abs(g - e).max(), np.abs(r - e).max()
                lim = 2 * q + 1e-6 * np.abs(e).max()
                print(f"{dtype} {H}x{W} gain {gain:g} block {k} fuse={fuse} split={split} {name}: engine error {err:.3e}, q {q:.3e}, "
                      f"max |exact| {np.abs(e).max():.3e}, error / (2 q + 1e-6 max) {err / lim:.3f}")
                if not err <= lim:
                    failures.append((k, fuse, split, name, err, lim))
    assert not failures, failures


def test_last_flow_needs_a_forward_of_that_size(hip_lib):
    eng = RF.IFNetEngine("f16")
    eng.load_state_dict(synthetic_ifnet_state())
    with pytest.raises(RF.FramewrightHipError) as ei:
        eng.last_flow(64, 96)
    assert ei.value.code == RF._lib.FW_ERR_INVALID
    fr = synthetic_frames(2, 64, 96, seed=1)
    eng.interpolate_device(torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1]).cuda(), 0.5)
    flow, mask = eng.last_flow(64, 96)
    assert flow.shape == (64, 96, 4) and mask.shape == (64, 96)
    with pytest.raises(RF.FramewrightHipError):
        eng.last_flow(70, 100)
    eng.close()


@pytest.mark.parametrize("timestep", [0.25, 0.75])
@pytest.mark.parametrize("dtype,tol,lsb", [("f16", 4e-3, 2), ("bf16", 3e-2, 8)])
@pytest.mark.parametrize("H,W,gain", [(64, 96, 1.0), (70, 100, 1.0), (96, 128, 12.0)])
def test_ifnet_vs_oracle_at_other_timesteps(hip_lib, dtype, tol, lsb, H, W, gain, timestep):
    """tests/test_rife_gpu.py::test_ifnet_vs_oracle's check and tolerances away from the mid frame; the frame must not be the 0.5 one."""
    sd = synthetic_ifnet_state(seed=2468, flow_gain=gain)
    eng = RF.IFNetEngine(dtype)
    eng.load_state_dict(sd)
    fr = synthetic_frames(2, H, W, seed=H)
    a, b = torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1]).cuda()
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    eng.interpolate_device(a, b, timestep, out=u8, out_rgb_f32=rgb)
    mid = eng.interpolate_device(a, b, 0.5).cpu().numpy()
    torch.cuda.synchronize()
    t = lambda f: torch.from_numpy(f[:, :, ::-1].astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    with torch.no_grad():
        want = ifnet_ref.ifnet_forward({k: torch.from_numpy(v) for k, v in sd.items()}, t(fr[0]), t(fr[1]), timestep)
    want = want[0].permute(1, 2, 0).numpy()
    err = np.abs(rgb.cpu().numpy() - want).max()
    want_u8 = (np.clip(want, 0, 1) * 255.0).round().astype(np.uint8)[:, :, ::-1]
    d = np.abs(u8.cpu().numpy().astype(int) - want_u8.astype(int))
    mse = np.mean(d.astype(np.float64) ** 2)
    psnr = 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)
    print(f"{dtype} {H}x{W} t={timestep}: max-abs {err:.2e}, uint8 max diff {d.max()}, PSNR {psnr:.1f} dB, "
          f"{int((u8.cpu().numpy() != mid).sum())} uint8 elements differ from the t = 0.5 frame")
    assert err < tol and d.max() <= lsb and psnr >= 50.0
    assert not np.array_equal(u8.cpu().numpy(), mid)
    assert np.array_equal(eng.interpolate(fr[0], fr[1], timestep), u8.cpu().numpy())
    eng.close()


def test_graph_cache_is_keyed_by_the_timestep(hip_lib, monkeypatch):
    """FW_IFNET_GRAPH=1: the timestep is an argument baked into the captured launches.  Six calls on one engine with the same buffers,
    the timestep alternating 0.25 / 0.5, must each give the direct-launch frame of their own timestep, bit for bit."""
    H, W = 96, 160
    sd = synthetic_ifnet_state(seed=7)
    fr = synthetic_frames(2, H, W, seed=3)
    a, b = torch.from_numpy(fr[0]).cuda(), torch.from_numpy(fr[1]).cuda()
    monkeypatch.setenv("FW_IFNET_GRAPH", "0")
    direct = RF.IFNetEngine("f16")
    direct.load_state_dict(sd)
    want = {}
    for t in (0.25, 0.5):
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        u8 = direct.interpolate_device(a, b, t, out=torch.empty((H, W, 3), dtype=torch.uint8, device="cuda"), out_rgb_f32=rgb)
        torch.cuda.synchronize()
        want[t] = (u8.clone(), rgb.clone())
    direct.close()
    assert not torch.equal(want[0.25][1], want[0.5][1])
    monkeypatch.setenv("FW_IFNET_GRAPH", "1")
    eng = RF.IFNetEngine("f16")
    eng.load_state_dict(sd)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    for i, t in enumerate([0.25, 0.5, 0.25, 0.5, 0.25, 0.5]):
        u8.fill_(0)
        rgb.fill_(-1.0)
        eng.interpolate_device(a, b, t, out=u8, out_rgb_f32=rgb)
        torch.cuda.synchronize()
        assert torch.equal(u8, want[t][0]) and torch.equal(rgb, want[t][1]), f"call {i} (timestep {t}) is not the direct-launch frame"
    eng.close()
