"""Restormer's transformer block and the seven steps between its stages in numpy float64 on NHWC arrays - the yardstick of
tests/test_restormer_blocks_gpu.py.

Two evaluation modes of the same functions:

  * exact (``rt=None``): plain float64 with the exact erf, the arithmetic of oracle/restormer_ref.py
    (tests/test_restormer_block_ref_host.py pins the two against each other at 1e-12);
  * operand-rounded (``rt="f16"`` / ``"bf16"``): float64 with values rounded to the operand type (through float32, as the kernels
    do) at exactly the points where the engine path under test rounds them.  Every sum stays float64: the model holds the
    roundings of a path, not its summation order.

Rounding points, read from csrc/ (names as accepted by ``skip=``; the attention half's carry a 1, the GDFN half's a 2):

  front "pw_dw"       pw_dw_fused.hip pw_dw_kernel, PWDW_NONE (qkv) and PWDW_GATE_GELU (GDFN), c = 48 / 96:
                        ln1 / ln2    (x - mean) * rstd WITHOUT the affine part, typed                (phase A, Op<T>::pack4)
                        w1 / w2      fp32(W * ln_w), typed; the bias is fp32(W . ln_b), not typed    (pack_pw_dw_blocks)
                        t1 / t2      the 1x1 output + folded bias, typed, zero outside the image     (the LDS image the depthwise conv reads)
                        qkv          the depthwise output, typed                                     (pack4 into the LDS image; q / k: the same bits go to qT)
                        g            gelu(x1) * x2 in fp32, typed
                      depthwise taps stay fp32.
  front "pw_dw_mfma"  pw_dw_mfma_kernel (FW_PW_DW_MFMA=1): the same, plus
                        taps1 / taps2  the depthwise taps, typed                                     (pack_pw_dw_blocks, taps16)
  front "staged"      layernorm_nhwc_*_kernel, pointwise_mfma / pw_gemm (PW_STORE), dwconv3x3_nhwc[_wide]_kernel (c = 192 / 384, and
                      c = 48 / 96 with FW_REST_FUSE_FRONT=0):
                        ln1 / ln2    the LayerNorm output with the affine part, typed
                        w1 / w2      the packed weights, typed                                       (pack_pointwise_weights / pack_pointwise_weights16)
                        t1 / t2      the GEMM output, typed                                          (PW_STORE epilogue)
                        qkv / g      the depthwise output / gelu(x1) * x2, typed
                      depthwise taps stay fp32.
  attention           q and k enter as the typed depthwise outputs (from qT, from qk_transpose_kernel's copy or from the pixel-major
                      tensor: the same bits); Gram sums, norms, temperature and softmax are fp32 in the kernels and float64 here.
                      merge_proj (default):
                        pa           fp32(project_out . attn), typed once                            (attn_proj_pack_kernel)
                                     applied to typed v, fp32 residual
                      FW_REST_MERGE_PROJ=0:
                        attn         the attention matrix, typed                                     (attn_pack_kernel)
                        av           attn . v, typed                                                 (PW_STORE epilogue)
                        wproj        project_out, typed                                              (pack_pointwise_weights)
  GDFN tail           typed g through
                        wout         project_out, typed, K = hp with zero rows hid .. hp             (pack_pointwise_weights)
                      into the fp32 residual.
  steps               x            the stream, typed                                                (fw_f32_to_planar)
                      w            the 3x3 weights, typed                                           (pack_conv3x3_weights); fp32 out
                      cat          the concatenated stream, typed in the reduce GEMM's staging       (pointwise_mfma, a_f32)
                      wred         reduce_chan, typed
                      PixelShuffle, PixelUnshuffle and the skip copy move fp32 bits.

The ``defect=`` argument builds wrong blocks and steps on purpose (the host test shows that the GPU test's bounds reject them)."""
import numpy as np
import torch

FRONTS = ("staged", "pw_dw", "pw_dw_mfma")
POINTS = ("ln1", "w1", "t1", "taps1", "qkv", "pa", "attn", "av", "wproj", "ln2", "w2", "t2", "taps2", "g", "wout")
STEP_POINTS = ("x", "w", "cat", "wred")
DEFECTS = ("dw_clamp", "not_zeroed", "gram_slot", "temp_head0", "x2_offset", "gelu_tanh", "eps")
STEP_DEFECTS = ("group_off",)
STEPS = ("down1_2", "down2_3", "down3_4", "up4_3", "up3_2", "up2_1", "output")
# block key -> (c, heads) on the engine of the GPU test: num_blocks (1, 1, 1, 1), no refinement blocks, heads (1, 2, 4, 8)
ENGINE_ARGS = dict(num_blocks=(1, 1, 1, 1), num_refinement_blocks=0, heads=(1, 2, 4, 8))
BLOCKS = {"encoder_level1.0.": (48, 1), "encoder_level2.0.": (96, 2), "encoder_level3.0.": (192, 4), "latent.0.": (384, 8),
          "decoder_level1.0.": (96, 1)}


def stream_pad(c):
    return (c + 31) // 32 * 32


def round_to(v, rt):
    """float64 -> float32 -> f16 / bf16 (round to nearest even) -> float64."""
    f = np.asarray(v, np.float64).astype(np.float32)
    if rt == "f16":
        return f.astype(np.float16).astype(np.float64)
    if rt == "bf16":
        u = np.ascontiguousarray(f).view(np.uint32)
        u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)    # finite values far from the largest: no carry out
        return u.view(np.float32).astype(np.float64)
    raise ValueError(rt)


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _erf(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v, np.float64))).numpy()


def block_weights(sd, prefix):
    """The block's tensors as float64 matrices: qkv [3c][c], project_out [c][c], project_in [2 hid][c], ffn project_out [c][hid],
    depthwise filters [n][3][3], temperature [heads]."""
    g = lambda k: np.asarray(sd[prefix + k], np.float64)
    c = g("norm1.body.weight").size
    hid = g("ffn.project_out.weight").shape[1]
    return dict(n1w=g("norm1.body.weight"), n1b=g("norm1.body.bias"), n2w=g("norm2.body.weight"), n2b=g("norm2.body.bias"),
                temp=g("attn.temperature").reshape(-1), wqkv=g("attn.qkv.weight").reshape(3 * c, c), dqkv=g("attn.qkv_dwconv.weight").reshape(3 * c, 3, 3),
                proj=g("attn.project_out.weight").reshape(c, c), pin=g("ffn.project_in.weight").reshape(2 * hid, c),
                dffn=g("ffn.dwconv.weight").reshape(2 * hid, 3, 3), pout=g("ffn.project_out.weight").reshape(c, hid))


def _normalise(x, eps):
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + eps)


def _dwconv3x3(t, wdw, clamp=False, outside=None):
    """Depthwise 3x3 on [H][W][n]; outside the image the input is zero, the border value (clamp) or the vector ``outside``."""
    H, W, n = t.shape
    out = np.empty_like(t)
    for c0 in range(0, n, 64):                           # channel blocks: the nine shifted products stay in cache at 100 k pixels
        s = slice(c0, min(c0 + 64, n))
        if clamp:
            p = np.pad(t[..., s], ((1, 1), (1, 1), (0, 0)), mode="edge")
        else:
            p = np.zeros((H + 2, W + 2, s.stop - s.start))
            if outside is not None:
                p[:] = outside[s]
            p[1:-1, 1:-1] = t[..., s]
        acc = np.zeros((H, W, s.stop - s.start))
        for dy in range(3):
            for dx in range(3):
                acc += p[dy:dy + H, dx:dx + W] * wdw[s, dy, dx]
        out[..., s] = acc
    return out


def _front(x, lnw, lnb, w, wdw, names, rt, front, R, eps, defect):
    """LayerNorm -> 1x1 -> depthwise 3x3 (unrounded) on one of the three front paths; names = the rounding points (ln, w, t, taps)."""
    n = _normalise(x, eps)
    if front == "staged":
        a, w1, b1 = R(names[0], n * lnw + lnb), R(names[1], w), 0.0
    else:
        F = (lambda v: v) if rt is None else _f32
        a, w1, b1 = R(names[0], n), R(names[1], F(w * lnw)), F(w @ lnb)
    t = R(names[2], a @ w1.T + b1)
    taps = R(names[3], wdw) if front == "pw_dw_mfma" else wdw
    return _dwconv3x3(t, taps, clamp=defect == "dw_clamp", outside=(w @ lnb) if defect == "not_zeroed" else None)


def attention_matrix(q, k, temp, heads, defect=None):
    """q, k: [M][c] -> softmax(normalize(q)^T normalize(k) * temperature) per head, [heads][ch][ch] (rows: q's channels)."""
    M, c = q.shape
    ch = c // heads
    if defect == "gram_slot":      # a slot of qT / kT that is no pixel of the image and holds something: one more term in every sum over the pixels
        q, k = np.concatenate([q, q[M // 2:M // 2 + 1] + 1.0]), np.concatenate([k, k[M // 3:M // 3 + 1] - 1.0])
    qn = q / np.maximum(np.sqrt((q * q).sum(0)), 1e-12)
    kn = k / np.maximum(np.sqrt((k * k).sum(0)), 1e-12)
    out = np.empty((heads, ch, ch))
    for h in range(heads):
        s = slice(h * ch, (h + 1) * ch)
        logits = (qn[:, s].T @ kn[:, s]) * temp[0 if defect == "temp_head0" else h]
        e = np.exp(logits - logits.max(-1, keepdims=True))
        out[h] = e / e.sum(-1, keepdims=True)
    return out


def _block_diag(attn):
    heads, ch, _ = attn.shape
    A = np.zeros((heads * ch, heads * ch))
    for h in range(heads):
        A[h * ch:(h + 1) * ch, h * ch:(h + 1) * ch] = attn[h]
    return A


def restormer_block(x, w, heads, rt=None, front="staged", merge_proj=True, skip=(), defect=None):
    """x: [H][W][c] float64 (the real channels); w: block_weights().  Returns (out [H][W][c], attn [heads][ch][ch], mid [H][W][c]) -
    mid is the stream between the attention half and the GDFN half."""
    assert front in FRONTS and (defect is None or defect in DEFECTS)
    x = np.asarray(x, np.float64)
    H, W, c = x.shape
    hid = w["pout"].shape[1]
    R = (lambda name, v: v) if rt is None else (lambda name, v: v if name in skip else round_to(v, rt))
    eps = 1e-6 if defect == "eps" else 1e-5
    qkv = R("qkv", _front(x, w["n1w"], w["n1b"], w["wqkv"], w["dqkv"], ("ln1", "w1", "t1", "taps1"), rt, front, R, eps, defect)).reshape(H * W, 3 * c)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    attn = attention_matrix(q, k, w["temp"], heads, defect)
    if merge_proj:
        y = v @ R("pa", w["proj"] @ _block_diag(attn)).T
    else:
        y = R("av", v @ R("attn", _block_diag(attn)).T) @ R("wproj", w["proj"]).T
    mid = x + y.reshape(H, W, c)
    d = _front(mid, w["n2w"], w["n2b"], w["pin"], w["dffn"], ("ln2", "w2", "t2", "taps2"), rt, front, R, eps, defect)
    x1, x2 = d[..., :hid], d[..., hid:]
    if defect == "x2_offset":      # the padded layout holds x1 at 0, zeros in rows hid .. hp, x2 at hp: read at hid, x2 comes out hp - hid rows late
        late = stream_pad(hid) - hid
        x2 = np.concatenate([np.zeros((H, W, late)), x2[..., :hid - late]], -1)
    if defect == "gelu_tanh":
        act = 0.5 * x1 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x1 + 0.044715 * x1 ** 3)))
    else:
        act = 0.5 * x1 * (1.0 + _erf(x1 / np.sqrt(2.0)))
    g = R("g", act * x2)
    return mid + g @ R("wout", w["pout"]).T, attn, mid


# ---- the steps between the stages -------------------------------------------------------------------------------------------------
def conv3x3(x, weight):
    """x [H][W][cin], weight [cout][cin][3][3], zero padding -> [H][W][cout]."""
    H, W, _ = x.shape
    p = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((H, W, weight.shape[0]))
    for dy in range(3):
        for dx in range(3):
            out += p[dy:dy + H, dx:dx + W] @ weight[:, :, dy, dx].T
    return out


def pixel_unshuffle(y):
    H, W, c = y.shape
    return y.reshape(H // 2, 2, W // 2, 2, c).transpose(0, 2, 4, 1, 3).reshape(H // 2, W // 2, 4 * c)     # channel c * 4 + dy * 2 + dx


def pixel_shuffle(y):
    H, W, c4 = y.shape
    return y.reshape(H, W, c4 // 4, 2, 2).transpose(0, 3, 1, 4, 2).reshape(2 * H, 2 * W, c4 // 4)


def step_weights(sd, step):
    """(3x3 weight [cout][cin][3][3], reduce_chan [cout][cin] or None) of a step."""
    key = "output.weight" if step == "output" else f"{step}.body.0.weight"
    red = {"up4_3": "reduce_chan_level3.weight", "up3_2": "reduce_chan_level2.weight"}.get(step)
    wr = np.asarray(sd[red], np.float64) if red else None
    return np.asarray(sd[key], np.float64), (wr.reshape(wr.shape[0], wr.shape[1]) if red else None)


def run_step(step, x, w3, wred=None, skip_stream=None, rt=None, skip=(), defect=None):
    """One of STEPS on x [H][W][cin] (and the encoder's skip stream for the up steps): the real channels of what the engine writes."""
    assert step in STEPS and (defect is None or defect in STEP_DEFECTS)
    R = (lambda name, v: v) if rt is None else (lambda name, v: v if name in skip else round_to(v, rt))
    y = conv3x3(R("x", np.asarray(x, np.float64)), R("w", w3))
    if step.startswith("down"):
        return pixel_unshuffle(y)
    if step == "output":
        return y
    if defect == "group_off":      # the second 64-channel output group lands where the third belongs
        y = np.concatenate([y[..., :64], np.zeros_like(y[..., :64]), y[..., 64:128], y[..., 192:]], -1)
    cat = np.concatenate([pixel_shuffle(y), np.asarray(skip_stream, np.float64)], -1)
    return cat if wred is None else R("cat", cat) @ R("wred", wred).T


# ---- the data both test files use ------------------------------------------------------------------------------------------------
def lively_state(seed=97, gelu_tail=False):
    """synthetic_restormer_state for ENGINE_ARGS with a livelier attention and larger residual branches: the synthetic q and k are
    uncorrelated (every logit ~ 1 / sqrt(pixels): a flat softmax at any temperature, which one temperature for all heads would pass) and
    the project_out gains make a block the identity plus a few percent.  Here k's 1x1 rows and filters are q's, rotated by 5 channels
    within the head's 48 / 96 and mixed with k's own, temperatures are 2 .. 6 and differ per head, and both project_out are O(1).

    ``gelu_tail``: the GDFN's x1 sits near -3 in every channel and pixel.  With x1 = O(1) the tanh form of GELU is within 5e-4 of the erf
    form - below what typing x1 to bf16 does to it - so no honest bound on the O(1) state can tell the two apart.  At -3 they differ by
    10 % of the value while the typed x1 moves it by 2 % (bf16) / 0.2 % (f16); the A&S 7.1.28 erf of the kernels is within 0.02 % there.
    x2 and project_out are scaled up so that the GDFN half stays a visible part of the stream."""
    from framewright_amd.restormer import synthetic_restormer_state
    sd = synthetic_restormer_state(seed=seed, **ENGINE_ARGS)
    rng = np.random.default_rng(seed + 1)
    for key, (c, heads) in BLOCKS.items():
        ch = c // heads
        perm = np.concatenate([h * ch + np.roll(np.arange(ch), 5) for h in range(heads)])
        for name in ("attn.qkv.weight", "attn.qkv_dwconv.weight"):
            wt = sd[key + name]
            wt[c:2 * c] = np.float32(0.7) * wt[:c][perm] + np.float32(0.7) * wt[c:2 * c]
        sd[key + "attn.temperature"] = rng.uniform(2.0, 6.0, size=sd[key + "attn.temperature"].shape).astype(np.float32)
        sd[key + "attn.project_out.weight"] *= np.float32(6.0)
        sd[key + "ffn.project_out.weight"] *= np.float32(3.0)
        for name in ("norm1.body.bias", "norm2.body.bias"):
            sd[key + name] = (rng.uniform(0.3, 1.0, size=c) * rng.choice([-1.0, 1.0], size=c)).astype(np.float32)   # the folded W . ln_b is no small term
        if gelu_tail:
            hid = sd[key + "ffn.project_out.weight"].shape[1]
            sd[key + "norm2.body.bias"] = np.full(c, 0.5, np.float32)
            pin, dw = sd[key + "ffn.project_in.weight"], sd[key + "ffn.dwconv.weight"]
            # x1 = centre tap (1) x (row . norm2's output): the row's constant part meets LayerNorm's zero-mean output only through the bias
            pin[:hid] = (-3.0 / (0.5 * c) + (0.2 / np.sqrt(c)) * rng.standard_normal((hid, c, 1, 1))).astype(np.float32)
            dw[:hid] = (0.01 * rng.standard_normal((hid, 1, 3, 3))).astype(np.float32)
            dw[:hid, 0, 1, 1] = 1.0
            dw[hid:] *= np.float32(8.0)
            sd[key + "ffn.project_out.weight"] *= np.float32(8.0)
    return sd


def lively_stream(H, W, c, seed):
    """fp32 [H][W][c]: per-channel scales 10^U(-0.5, 0.5) and means up to the scale - LayerNorm has something to do - and a quarter of the
    pixels scaled down to a variance over the channels near 1e-5, where LayerNorm's eps (1e-5) is a visible part of the result."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-0.5, 0.5, size=c)
    mean = scale * rng.uniform(-1.0, 1.0, size=c)
    x = mean + scale * rng.standard_normal((H, W, c))
    quiet = rng.random((H, W)) < 0.25
    quiet.flat[(H * W) // 2] = True
    x[quiet] *= 2e-3
    return x.astype(np.float32)


def padded(x):
    """[H][W][c] -> [H][W][stream_pad(c)] with zeros behind c: the engine's stream layout."""
    H, W, c = x.shape
    out = np.zeros((H, W, stream_pad(c)), np.float32)
    out[..., :c] = x
    return out
