"""tests/restormer_block_ref.py on the CPU: its exact mode is the oracle, its operand-rounded model has every rounding point it lists,
its input streams are lively, and the bounds that tests/test_restormer_blocks_gpu.py derives from it reject wrong blocks and steps."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import restormer_block_ref as R
from oracle import restormer_ref

# (block, H, W): a block at each of c = 48, 96 (heads 2 and heads 1), 192, 384; sizes a forward can issue, two fused-front tiles at c = 48
CASES = [("encoder_level1.0.", 16, 32), ("encoder_level2.0.", 12, 20), ("decoder_level1.0.", 8, 16), ("encoder_level3.0.", 10, 6), ("latent.0.", 5, 7)]
# (front, merge_proj) of the GPU test's path table
PATHS = {48: [("pw_dw", True), ("pw_dw", False), ("staged", True), ("pw_dw_mfma", True)], 96: [("pw_dw", True), ("pw_dw", False), ("staged", True), ("pw_dw_mfma", True)],
         192: [("staged", True), ("staged", False)], 384: [("staged", True), ("staged", False)]}
STEP_CASES = [("down1_2", 6, 10), ("down2_3", 6, 10), ("down3_4", 4, 6), ("up4_3", 3, 5), ("up3_2", 3, 5), ("up2_1", 5, 3), ("output", 5, 7)]


@functools.lru_cache(maxsize=None)
def _state(gelu_tail=False):
    return R.lively_state(gelu_tail=gelu_tail)


@functools.lru_cache(maxsize=None)
def _case(key, H, W, gelu_tail=False):
    c, heads = R.BLOCKS[key]
    w = R.block_weights(_state(gelu_tail), key)
    x = R.lively_stream(H, W, c, seed=H * 1000 + W)
    return c, heads, w, x, R.restormer_block(x, w, heads)


def _step_inputs(step, H, W):
    sd = _state()
    w3, wred = R.step_weights(sd, step)
    x = R.lively_stream(H, W, w3.shape[1], seed=11 + R.STEPS.index(step))
    skip = R.lively_stream(2 * H, 2 * W, w3.shape[0] // 4, seed=23 + R.STEPS.index(step)) if step.startswith("up") else None
    return w3, wred, x, skip


@pytest.mark.parametrize("key,H,W", CASES)
def test_exact_block_is_the_oracle(key, H, W):
    c, heads, w, x, (out, attn, mid) = _case(key, H, W)
    sd64 = {k: torch.from_numpy(v).double() for k, v in _state().items() if k.startswith(key)}
    xt = torch.from_numpy(x).double().permute(2, 0, 1).unsqueeze(0)
    want = restormer_ref.block(sd64, key, xt, heads)[0].permute(1, 2, 0).numpy()
    assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max()
    # the attention matrix: the oracle's expression on the oracle's q and k
    n1 = restormer_ref.layer_norm(xt, sd64[key + "norm1.body.weight"], sd64[key + "norm1.body.bias"])
    qkv = F.conv2d(F.conv2d(n1, sd64[key + "attn.qkv.weight"]), sd64[key + "attn.qkv_dwconv.weight"], None, 1, 1, 1, 3 * c)
    q, k, _ = (t.reshape(1, heads, c // heads, H * W) for t in qkv.chunk(3, dim=1))
    a = ((F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * sd64[key + "attn.temperature"]).softmax(dim=-1)[0].numpy()
    assert np.abs(attn - a).max() <= 1e-12
    assert np.abs(attn.sum(-1) - 1).max() <= 1e-12


@pytest.mark.parametrize("step,H,W", STEP_CASES)
def test_exact_steps_are_the_oracle(step, H, W):
    """The expressions of oracle/restormer_ref.restormer_forward between its stages, in torch float64."""
    sd = _state()
    w3, wred, x, skip = _step_inputs(step, H, W)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double().permute(2, 0, 1).unsqueeze(0)
    key = "output.weight" if step == "output" else f"{step}.body.0.weight"
    y = F.conv2d(t(x), torch.from_numpy(sd[key]).double(), None, 1, 1)
    if step.startswith("down"):
        y = F.pixel_unshuffle(y, 2)
    elif step.startswith("up"):
        y = torch.cat([F.pixel_shuffle(y, 2), t(skip)], 1)
        if wred is not None:
            y = F.conv2d(y, torch.from_numpy(sd["reduce_chan_level3.weight" if step == "up4_3" else "reduce_chan_level2.weight"]).double())
    want = y[0].permute(1, 2, 0).numpy()
    got = R.run_step(step, x, w3, wred, skip)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_rounding_is_round_to_nearest_even_through_float32():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -65504.0, 1e-8, 0.1, -0.3, 1234.567])
    for rt, tdt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        want = torch.from_numpy(v).float().to(tdt).double().numpy()
        assert np.array_equal(R.round_to(v, rt), want)
    assert R.round_to(1.0 + 2.0 ** -11, "f16") == 1.0 and R.round_to(1.0 + 3 * 2.0 ** -11, "f16") == 1.0 + 2.0 ** -9   # ties to even
    assert R.round_to(1.0 + 2.0 ** -8, "bf16") == 1.0 and R.round_to(1.0 + 3 * 2.0 ** -8, "bf16") == 1.0 + 2.0 ** -6


@pytest.mark.parametrize("gelu_tail", [False, True])
@pytest.mark.parametrize("key,H,W", CASES)
def test_streams_are_lively(key, H, W, gelu_tail):
    """Both halves of the block change the stream by at least 5 % of its standard deviation, and no softmax row is a one-hot."""
    c, heads, w, x, (out, attn, mid) = _case(key, H, W, gelu_tail)
    sdev = x.astype(np.float64).std()
    a_half, f_half = (mid - x).std() / sdev, (out - mid).std() / sdev
    print(f"{key} {H}x{W}: attention half {a_half:.3f}, GDFN half {f_half:.3f} of the stream's deviation; largest softmax entry {attn.max():.3f}, "
          f"smallest row maximum {attn.max(-1).min():.3f}")
    assert a_half >= 0.05 and f_half >= 0.05
    assert attn.max() <= 0.9
    assert attn.max(-1).min() > 1.2 / attn.shape[-1]          # ... nor flat: the temperature matters
    if gelu_tail:                                             # x1 of the GDFN: in the tail, every channel of every pixel
        d = R._front(mid, w["n2w"], w["n2b"], w["pin"], w["dffn"], ("ln2", "w2", "t2", "taps2"), None, "staged", lambda name, v: v, 1e-5, None)
        x1 = d[..., :w["pout"].shape[1]]
        print(f"    x1 in [{x1.min():.2f}, {x1.max():.2f}]")
        assert -4.5 < x1.min() and x1.max() < -1.8


@pytest.mark.parametrize("rt", ["f16", "bf16"])
@pytest.mark.parametrize("key,H,W", [CASES[1], CASES[3]])
def test_rounded_model_has_every_rounding_point_of_its_path(key, H, W, rt):
    """Leaving one rounding point out changes the model's result: each listed point is live on each path that has it."""
    c, heads, w, x, (exact, attn, _) = _case(key, H, W)
    u = 2.0 ** (-11 if rt == "f16" else -8)
    for front, merge in PATHS[c]:
        full = R.restormer_block(x, w, heads, rt, front, merge)[0]
        q = np.abs(full - exact).max()
        assert 0.05 * u < q / np.abs(exact).max() < 50 * u, q
        dead = {"taps1", "taps2"} if front != "pw_dw_mfma" else set()
        dead |= {"attn", "av", "wproj"} if merge else {"pa"}
        for point in R.POINTS:
            part = R.restormer_block(x, w, heads, rt, front, merge, skip=(point,))[0]
            assert np.array_equal(part, full) == (point in dead), (front, merge, point)
        none = R.restormer_block(x, w, heads, rt, front, merge, skip=R.POINTS)[0]
        assert np.abs(none - exact).max() <= (1e-5 if front != "staged" else 1e-12) * np.abs(exact).max()   # what is left: the fp32 rounding of the folded weights and biases
    models = [R.restormer_block(x, w, heads, rt, front, merge)[0] for front, merge in PATHS[c]]
    for i in range(len(models)):
        for j in range(i):
            assert not np.array_equal(models[i], models[j]), (PATHS[c][i], PATHS[c][j])


def block_bounds(exact, rounded):
    """(max bound, mean bound) of the GPU test."""
    return (2 * np.abs(rounded - exact).max() + 1e-6 * np.abs(exact).max(), 2 * np.abs(rounded - exact).mean() + 1e-6 * np.abs(exact).mean())


@pytest.mark.parametrize("rt", ["f16", "bf16"])
@pytest.mark.parametrize("key,H,W", CASES)
def test_the_gpu_bounds_reject_wrong_blocks(key, H, W, rt):
    """Every defect, computed in float64 on the CPU, is outside the bound 2 q + 1e-6 max |exact| of the stream or of the attention
    matrix, on every path's model.  The tanh form of GELU is told from the erf form on the state whose x1 lies in GELU's tail
    (restormer_block_ref.lively_state): with x1 = O(1) it is within the typing of x1, which no honest bound can look below."""
    c, heads, w, x, (exact, attn, _) = _case(key, H, W)
    wrong = {d: R.restormer_block(x, w, heads, defect=d) for d in R.DEFECTS if d != "gelu_tanh"}
    _, _, wt, xt, (exact_t, attn_t, _) = _case(key, H, W, True)
    tanh_t = R.restormer_block(xt, wt, heads, defect="gelu_tanh")
    for front, merge in PATHS[c]:
        rounded, rattn, _ = R.restormer_block(x, w, heads, rt, front, merge)
        lim, _ = block_bounds(exact, rounded)
        alim, _ = block_bounds(attn, rattn)
        lim_t, mlim_t = block_bounds(exact_t, R.restormer_block(xt, wt, heads, rt, front, merge)[0])
        err_t = np.abs(tanh_t[0] - exact_t)
        print(f"{key} {rt} {front} merge {merge} gelu_tanh (tail state): stream error / bound {err_t.max() / lim_t:.1f}, mean error / bound {err_t.mean() / mlim_t:.1f}")
        assert err_t.max() > lim_t, (front, merge, err_t.max(), lim_t)
        for d, (out, a, _) in wrong.items():
            if d == "temp_head0" and heads == 1:
                assert np.array_equal(out, exact)                  # one head: nothing to confuse
                continue
            err, aerr = np.abs(out - exact).max(), np.abs(a - attn).max()
            print(f"{key} {rt} {front} merge {merge} {d}: stream error / bound {err / lim:.1f}, attention error / bound {aerr / alim:.1f}")
            assert err > lim, (front, merge, d, err, lim)
            if d in ("gram_slot", "temp_head0"):
                assert aerr > alim, (front, merge, d, aerr, alim)  # the attention check sees them on its own


@pytest.mark.parametrize("rt", ["f16", "bf16"])
@pytest.mark.parametrize("step,H,W", STEP_CASES)
def test_step_models_round_and_their_bounds_reject_wrong_steps(step, H, W, rt):
    w3, wred, x, skip = _step_inputs(step, H, W)
    exact, rounded = R.run_step(step, x, w3, wred, skip), R.run_step(step, x, w3, wred, skip, rt)
    lim, _ = block_bounds(exact, rounded)
    assert 0 < np.abs(rounded - exact).max() < 0.05 * np.abs(exact).max()
    points = [p for p in R.STEP_POINTS if wred is not None or p in ("x", "w")]
    for point in points:
        assert not np.array_equal(R.run_step(step, x, w3, wred, skip, rt, skip=(point,)), rounded), point
    assert np.abs(R.run_step(step, x, w3[:, :, :, ::-1], wred, skip) - exact).max() > lim      # dx taps swapped
    assert np.abs(R.run_step(step, x, w3[:, :, ::-1], wred, skip) - exact).max() > lim         # dy taps swapped
    if step.startswith("up"):
        assert np.abs(R.run_step(step, x, w3, wred, skip, defect="group_off") - exact).max() > lim
        assert np.abs(R.run_step(step, x, w3, wred, 0 * skip) - exact).max() > lim             # the skip not copied
        swapped = w3.reshape(-1, 2, 2, *w3.shape[1:])[:, ::-1].reshape(w3.shape)               # PixelShuffle rows swapped
        assert np.abs(R.run_step(step, x, swapped, wred, skip) - exact).max() > lim
