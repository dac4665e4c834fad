"""tests/nafblock_ref.py on the CPU: its exact mode is the oracle, its operand-rounded model has every rounding point it lists, and the
bounds that tests/test_nafblock_gpu.py derives from it reject wrong blocks."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nafblock_ref as R
import test_nafblock_gpu as G          # its bound functions are plain numpy; only the CU count comes from the device
from oracle import nafnet_ref

CASES = [(32, 1, "encoders.0.0.", 32, 6, 10), (64, 1, "encoders.0.0.", 64, 16, 32), (64, 1, "middle_blks.0.", 128, 9, 7),
         (64, 2, "middle_blks.0.", 256, 9, 7)]
PATHS = [("plain", "act_scale"), ("pw_dw", "act_scale"), ("pw_dw", "tail128"), ("pw_dw_mfma", "tail128"), ("plain", "w3_scale")]


@functools.lru_cache(maxsize=None)
def _case(width, levels, key, c, H, W):
    sd = R.lively_state(width, levels)
    x = R.lively_stream(H, W, c, seed=H * 1000 + W)
    return sd, R.block_weights(sd, key), x, R.nafblock(x, R.block_weights(sd, key))


@pytest.mark.parametrize("width,levels,key,c,H,W", CASES)
def test_exact_block_is_the_oracle(width, levels, key, c, H, W):
    sd, w, x, (out, sca, parts) = _case(width, levels, key, c, H, W)
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith(key)}
    xt = torch.from_numpy(x).double().permute(2, 0, 1).unsqueeze(0)
    want = nafnet_ref.nafblock(sd64, key, xt)[0].permute(1, 2, 0).numpy()
    assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max()
    # the SCA vector: the oracle's expression on the oracle's gated tensor
    t = F.conv2d(nafnet_ref.layernorm2d(xt, sd64[key + "norm1.weight"], sd64[key + "norm1.bias"]), sd64[key + "conv1.weight"], sd64[key + "conv1.bias"])
    g = nafnet_ref.simple_gate(F.conv2d(t, sd64[key + "conv2.weight"], sd64[key + "conv2.bias"], padding=1, groups=2 * c))
    s = F.conv2d(F.adaptive_avg_pool2d(g, 1), sd64[key + "sca.1.weight"], sd64[key + "sca.1.bias"]).reshape(c).numpy()
    assert np.abs(sca - s).max() <= 1e-12 * np.abs(s).max()
    assert np.abs(parts["g"] - g[0].permute(1, 2, 0).numpy()).max() <= 1e-12


@pytest.mark.parametrize("level,H,W", [(0, 6, 10), (1, 4, 6), (2, 2, 10)])
def test_exact_resamples_are_the_oracle(level, H, W):
    sd = R.lively_state(64, 3)
    c = 64 << level
    x = R.lively_stream(H, W, c, seed=level)
    xt = torch.from_numpy(x).double().permute(2, 0, 1).unsqueeze(0)
    wd, bd = sd[f"downs.{level}.weight"], sd[f"downs.{level}.bias"]
    want = F.conv2d(xt, torch.from_numpy(wd).double(), torch.from_numpy(bd).double(), stride=2)[0].permute(1, 2, 0).numpy()
    got = R.down(x, wd, bd)
    assert got.shape == (H // 2, W // 2, 2 * c) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the step INTO `level`: ups[levels - 1 - level] takes 2c channels
    wu = sd[f"ups.{3 - 1 - level}.0.weight"]
    assert wu.shape == (4 * c, 2 * c, 1, 1)
    lo = R.lively_stream(H, W, 2 * c, seed=10 + level)
    skip = R.lively_stream(2 * H, 2 * W, c, seed=20 + level)
    lt = torch.from_numpy(lo).double().permute(2, 0, 1).unsqueeze(0)
    want = (F.pixel_shuffle(F.conv2d(lt, torch.from_numpy(wu).double()), 2)[0].permute(1, 2, 0).numpy() + skip.astype(np.float64))
    got = R.up(lo, wu, skip)
    assert got.shape == (2 * H, 2 * W, c) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_rounding_is_round_to_nearest_even_through_float32():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -65504.0, 1e-8, 0.1])
    for rt, tdt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        want = torch.from_numpy(v).float().to(tdt).double().numpy()
        assert np.array_equal(R.round_to(v, rt), want)
    assert R.round_to(1.0 + 2.0 ** -11, "f16") == 1.0 and R.round_to(1.0 + 3 * 2.0 ** -11, "f16") == 1.0 + 2.0 ** -9   # ties to even
    assert R.round_to(1.0 + 2.0 ** -8, "bf16") == 1.0 and R.round_to(1.0 + 3 * 2.0 ** -8, "bf16") == 1.0 + 2.0 ** -6


@pytest.mark.parametrize("rt", ["f16", "bf16"])
@pytest.mark.parametrize("front,tail", PATHS)
def test_rounded_model_has_every_rounding_point_of_its_path(front, tail, rt):
    """Leaving one rounding point out changes the model's result: each listed point is live on each path that has it."""
    sd, w, x, (exact, sca, _) = _case(64, 1, "middle_blks.0.", 128, 9, 7)
    full, sfull, _ = R.nafblock(x, w, rt, front, tail)
    u = 2.0 ** (-11 if rt == "f16" else -8)
    q = np.abs(full - exact).max()
    assert 0.05 * u < q < 50 * u, q                  # the model differs from the exact mode by rounding-sized amounts
    points = [p for p in R.POINTS if p != "taps" or front == "pw_dw_mfma"]
    for point in points:
        part, spart, _ = R.nafblock(x, w, rt, front, tail, skip=(point,))
        assert not np.array_equal(part, full), point
        if point in ("ln1", "w1", "t") or point == "taps":
            assert not np.array_equal(spart, sfull), point    # in front of the pooling: the SCA vector responds too
        else:
            assert np.array_equal(spart, sfull), point        # the pooling sums the unrounded gated values
    none, _, _ = R.nafblock(x, w, rt, front, tail, skip=R.POINTS)
    folded = front != "plain" or tail == "tail128"
    assert np.abs(none - exact).max() <= (1e-5 if folded else 1e-12)   # what is left is the fp32 rounding of the folded weights and biases
    if front != "pw_dw_mfma":
        assert np.array_equal(R.nafblock(x, w, rt, front, tail, skip=("taps",))[0], full)
    # the paths differ from each other
    other = R.nafblock(x, w, rt, "plain" if front != "plain" else "pw_dw", tail)[0]
    assert not np.array_equal(other, full)


@pytest.mark.parametrize("rt", ["f16", "bf16"])
@pytest.mark.parametrize("width,levels,key,c,H,W", CASES)
def test_the_gpu_bounds_reject_wrong_blocks(monkeypatch, width, levels, key, c, H, W, rt):
    """Every defect, computed exactly on the CPU, is outside at least the bound meant for it, on every path's model: the block bound
    2 q + 1e-6 max |exact|, or - for a pooling that loses a row - the SCA bound of the GPU test around the model's SCA vector."""
    monkeypatch.setattr(G, "_cus", lambda: 256)
    sd, w, x, (exact, sca, _) = _case(width, levels, key, c, H, W)
    wrong = {d: R.nafblock(x, w, defect=d) for d in R.DEFECTS}
    for front, tail in PATHS:
        rounded, srounded, mparts = R.nafblock(x, w, rt, front, tail)
        lim = 2 * np.abs(rounded - exact).max() + 1e-6 * np.abs(exact).max()
        slim = G._sca_bound(w, mparts, rt, front, H, W, c)
        margin = G._lost_row_margin(w, mparts, slim, front if c in (64, 128) else "plain", H, W, c)
        assert margin > 1.5, (front, tail, margin)          # any single row of `partial` lost: outside the SCA bound
        for d, (out, s, _) in wrong.items():
            err, serr = np.abs(out - exact).max(), (np.abs(s - srounded) / slim).max()
            print(f"c {c} {rt} {front}/{tail} {d}: block error / bound {err / lim:.1f}, SCA error / bound {serr:.1f}")
            if d == "sca_row":
                assert serr > 3, (front, tail, d, serr)
            else:
                assert err > 3 * lim, (front, tail, d, err, lim)
            if d in ("eps", "gate", "dw_clamp"):
                assert serr > 3, (front, tail, d, serr)      # in front of the pooling: the SCA check sees them as well
        # liveness, as the GPU test asserts it: the block does something, and both of its halves do
        assert np.abs(exact - x).max() > 100 * lim
        for name in ("beta", "gamma"):
            w0 = dict(w)
            w0[name] = np.zeros_like(w[name])
            assert np.abs(R.nafblock(x, w0)[0] - exact).max() > 10 * lim, name


@pytest.mark.parametrize("rt", ["f16", "bf16"])
def test_resample_models_round_and_their_bounds_reject_a_wrong_tap(rt):
    sd = R.lively_state(64, 3)
    x = R.lively_stream(6, 10, 128, seed=3)
    wd, bd = sd["downs.1.weight"], sd["downs.1.bias"]
    exact, rounded = R.down(x, wd, bd), R.down(x, wd, bd, rt)
    lim = 2 * np.abs(rounded - exact).max() + 1e-6 * np.abs(exact).max()
    assert 0 < np.abs(rounded - exact).max() < 0.05 * np.abs(exact).max()
    assert np.abs(R.down(x, wd[:, :, :, ::-1], bd) - exact).max() > 3 * lim          # dx taps swapped
    assert np.abs(R.down(x, wd, 0 * bd) - exact).max() > 3 * lim                      # bias dropped
    wu = sd["ups.0.0.weight"]                                                         # into level 2: 512 -> 4 x 256
    lo, skip = R.lively_stream(3, 5, 512, seed=4), R.lively_stream(6, 10, 256, seed=5)
    exact, rounded = R.up(lo, wu, skip), R.up(lo, wu, skip, rt)
    lim = 2 * np.abs(rounded - exact).max() + 1e-6 * np.abs(exact).max()
    assert 0 < np.abs(rounded - exact).max() < 0.05 * np.abs(exact).max()
    swapped = wu.reshape(256, 2, 2, 512)[:, ::-1].reshape(wu.shape)                   # PixelShuffle rows swapped
    assert np.abs(R.up(lo, swapped, skip) - exact).max() > 3 * lim
    assert np.abs(R.up(lo, wu, 0 * skip) - exact).max() > 3 * lim                     # the skip not added
