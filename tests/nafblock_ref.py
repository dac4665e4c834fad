"""NAFNet's block and level changes in numpy float64 on NHWC arrays - the yardstick of tests/test_nafblock_gpu.py.

Two evaluation modes of the same functions:

  * exact (``rt=None``): plain float64, the arithmetic of oracle/nafnet_ref.py (tests/test_nafblock_ref_host.py pins the two
    against each other at 1e-12);
  * operand-rounded (``rt="f16"`` / ``"bf16"``): float64 with values rounded to the operand type (through float32, as the kernels
    do) at exactly the points where the engine path under test rounds them.  Every sum stays float64: the model holds the
    roundings of a path, not its summation order.

Rounding points, read from csrc/ (names as accepted by ``skip=``):

  front "plain"    LayerNorm2d kernel or LayerNorm inside pointwise_mfma's staging, pointwise conv1, dwconv3x3_gate (c = 32, c >= 256,
                   and c = 64 / 128 with FW_NAF_FUSE_FRONT=0):
                     ln1   norm1's output, affine part applied, typed            (layernorm2d_kernel / pack8f in the staging)
                     w1    conv1's weights                                       (pack_pointwise_weights / pack_pointwise_weights16)
                     t     conv1's output + bias, typed                          (PW_STORE epilogue)
                     g     the gated depthwise output, typed                     (pack8f in dwconv3x3_gate*_kernel)
                   depthwise taps and bias stay fp32; the SCA pooling sums the UNROUNDED gated values.
  front "pw_dw"    pw_dw_fused.hip, PWDW_GATE_MUL (c = 64, 128):
                     ln1   (x - mean) * rstd WITHOUT the affine part, typed      (phase A)
                     w1    fp32(conv1.weight * norm1.weight), typed; the bias is fp32(conv1.bias + conv1.weight . norm1.bias) (pack_pw_dw_blocks)
                     t     conv1's output + folded bias, typed, zero outside the image
                     g     the gated depthwise output, typed
  front "pw_dw_mfma"  the same with FW_PW_DW_MFMA=1, plus
                     taps  the depthwise taps, typed                             (pack_pw_dw_blocks, taps16)
  tail "act_scale" pointwise_mfma with a_scale, naf_tail64_kernel (c = 32, c = 64, c = 128 with FW_NAF_FUSE_TAIL=0, c >= 256 with
                   FW_NAF_GEMM=0):
                     xs    typed(g) * sca, typed again                           (aconv / the staging of naf_tail64)
                     w3, w4, w5  the packed weights
                     ln2   norm2's output, affine part applied, typed
                     h     SimpleGate(conv4 + bias), typed                       (PW_GATE epilogue / put4)
  tail "w3_scale"  pointwise_gemm.hip (c >= 256): as "act_scale", except that the activations stay typed(g) and
                     xs    typed(w3) * sca, typed again                          (pw16_scale_weights_kernel)
  tail "tail128"   naf_tail128.hip (c = 128): "w3_scale" (naf_tail128_scale_w3_kernel), and norm2's affine part folded into conv4:
                     ln2   (y - mean) * rstd, typed
                     w4    fp32(conv4.weight * norm2.weight), typed; bias fp32(conv4.bias + conv4.weight . norm2.bias)
  down             x typed (pack8f of the gathered fp32 stream), weights typed; fp32 out
  up               x typed, weights typed; PixelShuffle and the add in fp32

The ``defect=`` argument builds wrong blocks on purpose (the host test shows that the GPU test's bound rejects them)."""
import numpy as np

FRONTS = ("plain", "pw_dw", "pw_dw_mfma")
TAILS = ("act_scale", "w3_scale", "tail128")
POINTS = ("ln1", "w1", "t", "taps", "g", "xs", "w3", "ln2", "w4", "h", "w5")
DEFECTS = ("eps", "gate", "sca_row", "beta", "dw_clamp")


def round_to(v, rt):
    """float64 -> float32 -> f16 / bf16 (round to nearest even) -> float64."""
    f = np.asarray(v, np.float64).astype(np.float32)
    if rt == "f16":
        return f.astype(np.float16).astype(np.float64)
    if rt == "bf16":
        u = np.ascontiguousarray(f).view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        return u.view(np.float32).astype(np.float64)
    raise ValueError(rt)


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def block_weights(sd, prefix):
    """The block's tensors as float64 matrices: conv1 [2c][c], conv2 [2c][3][3], conv3 / sca / conv5 [c][c], conv4 [2c][c], vectors [c]."""
    g = lambda k: np.asarray(sd[prefix + k], np.float64)
    c = g("beta").size
    return dict(n1w=g("norm1.weight"), n1b=g("norm1.bias"), n2w=g("norm2.weight"), n2b=g("norm2.bias"), beta=g("beta").reshape(c),
                gamma=g("gamma").reshape(c), w1=g("conv1.weight").reshape(2 * c, c), b1=g("conv1.bias"), wdw=g("conv2.weight").reshape(2 * c, 3, 3),
                bdw=g("conv2.bias"), w3=g("conv3.weight").reshape(c, c), b3=g("conv3.bias"), wsca=g("sca.1.weight").reshape(c, c),
                bsca=g("sca.1.bias"), w4=g("conv4.weight").reshape(2 * c, c), b4=g("conv4.bias"), w5=g("conv5.weight").reshape(c, c), b5=g("conv5.bias"))


def _normalise(x, eps):
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + eps)


def _dwconv3x3(t, wdw, bdw, clamp=False):
    H, W, _ = t.shape
    p = np.pad(t, ((1, 1), (1, 1), (0, 0)), mode="edge" if clamp else "constant")
    out = np.zeros_like(t) + bdw
    for dy in range(3):
        for dx in range(3):
            out += p[dy:dy + H, dx:dx + W] * wdw[:, dy, dx]
    return out


def nafblock(x, w, rt=None, front="plain", tail="act_scale", skip=(), defect=None):
    """x: [H][W][c] float64; w: block_weights().  Returns (out [H][W][c], sca [c], parts) - parts holds the gated tensor ``g`` (unrounded),
    its pooled mean and ``sens`` for the SCA bound of the GPU test."""
    assert front in FRONTS and tail in TAILS and (defect is None or defect in DEFECTS)
    x = np.asarray(x, np.float64)
    H, W, c = x.shape
    R = (lambda name, v: v) if rt is None else (lambda name, v: v if name in skip else round_to(v, rt))
    F = (lambda v: v) if rt is None else _f32
    eps = 1e-5 if defect == "eps" else 1e-6
    n = _normalise(x, eps)
    if front == "plain":
        a, w1, b1 = R("ln1", n * w["n1w"] + w["n1b"]), R("w1", w["w1"]), w["b1"]
    else:
        a, w1, b1 = R("ln1", n), R("w1", F(w["w1"] * w["n1w"])), F(w["b1"] + w["w1"] @ w["n1b"])
    t = R("t", a @ w1.T + b1)
    taps = R("taps", w["wdw"]) if front == "pw_dw_mfma" else w["wdw"]
    d = _dwconv3x3(t, taps, w["bdw"], clamp=defect == "dw_clamp")
    x2 = d[..., c:]
    if defect == "gate":      # x1 * x2 commutes, so "the wrong half" is a wrong partner: x2's two halves swapped
        x2 = np.roll(x2, c // 2, -1)
    g = d[..., :c] * x2
    pooled = (g[:-1].sum((0, 1)) if defect == "sca_row" and H > 1 else g.sum((0, 1))) / (H * W)
    # per channel, the rms over the pixels of sum_i |tap_i t_i| |partner| over both halves: how far one typed conv1 output that comes
    # out as its neighbour moves a gated value, per unit of relative change (the SCA bound of the GPU test)
    da = _dwconv3x3(np.abs(t), np.abs(taps), 0.0)
    sens = np.sqrt(((da[..., :c] * np.abs(d[..., c:]) + np.abs(d[..., :c]) * da[..., c:]) ** 2).mean((0, 1)))
    parts = dict(g=g, pooled=pooled, sens=sens, w1_mean_abs=np.abs(w1).mean())
    s = w["wsca"] @ pooled + w["bsca"]
    gq = R("g", g)
    if tail == "act_scale":
        xs, w3 = R("xs", gq * s), R("w3", w["w3"])
    else:
        xs, w3 = gq, R("xs", R("w3", w["w3"]) * s[None, :])
    beta = 0.0 if defect == "beta" else w["beta"]
    y = x + (xs @ w3.T + w["b3"]) * beta
    n2 = _normalise(y, eps)
    if tail == "tail128":
        a2, w4, b4 = R("ln2", n2), R("w4", F(w["w4"] * w["n2w"])), F(w["b4"] + w["w4"] @ w["n2b"])
    else:
        a2, w4, b4 = R("ln2", n2 * w["n2w"] + w["n2b"]), R("w4", w["w4"]), w["b4"]
    u = a2 @ w4.T + b4
    h = R("h", u[..., :c] * u[..., c:])
    out = y + (h @ R("w5", w["w5"]).T + w["b5"]) * w["gamma"]
    return out, s, parts


def partial_rows(front, H, W, c, cus):
    """[c // 8 or 1][H][W] int: the row of the `partial` buffer (the workgroup) whose pooled sum a pixel of a channel group lands in, and
    the number of rows - from pw_dw_blocks / the tile walk of pw_dw_kernel, dwconv_blocks and the grid-stride loops of the two
    depthwise kernels."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if front != "plain":                                   # pw_dw: 14 x 30 tiles in row-major order, workgroup b walks tiles [b T / G, (b + 1) T / G)
        tx = -(-W // 30)
        tiles = -(-H // 14) * tx
        G = min(tiles, cus)
        tile = (yy // 14) * tx + xx // 30
        return (((tile + 1) * G - 1) // tiles)[None], G    # the b with b T / G <= tile < (b + 1) T / G (integer division)
    col = (yy // 3) * W + xx                               # (3-row strip, column)
    if c >= 256:                                           # wide: a block walks columns cb * 8 + cl, + rows * 8, ...
        cols = -(-H // 3) * W
        rows = min(-(-cols // 8), 768 // (c // 256))
        return ((col % (rows * 8)) // 8)[None], rows
    groups = c // 8                                        # narrow: item (strip, x, group), group fastest, 256 items per block, grid-stride
    total = -(-H // 3) * W * groups
    blocks = min(-(-total // 256), 768)
    idx = col[None] * groups + np.arange(groups)[:, None, None]
    return (idx % (blocks * 256)) // 256, blocks


def lost_row_effects(g, wsca, rows, nrows):
    """[nrows][c]: by how much the SCA vector moves when row r of `partial` is not summed."""
    H, W, c = g.shape
    per = c // rows.shape[0]
    sums = np.zeros((nrows, c))
    for k in range(rows.shape[0]):
        np.add.at(sums[:, k * per:(k + 1) * per], rows[k].reshape(-1), g[..., k * per:(k + 1) * per].reshape(H * W, per))
    return (sums / (H * W)) @ wsca.T


def down(x, weight, bias, rt=None):
    """2x2 stride-2 conv: x [H][W][c], weight [2c][c][2][2] -> [H/2][W/2][2c]."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    if rt is not None:
        x, weight = round_to(x, rt), round_to(weight, rt)
    H, W, c = x.shape
    out = np.zeros((H // 2, W // 2, weight.shape[0])) + np.asarray(bias, np.float64)
    for dy in range(2):
        for dx in range(2):
            out += x[dy::2, dx::2] @ weight[:, :, dy, dx].T
    return out


def up(x, weight, skip, rt=None):
    """1x1 conv without bias, pixel_shuffle(2), + skip: x [H][W][C], weight [2C][C] -> [2H][2W][C/2]."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64).reshape(-1, np.shape(x)[-1])
    if rt is not None:
        x, weight = round_to(x, rt), round_to(weight, rt)
    H, W, C = x.shape
    y = (x @ weight.T).reshape(H, W, C // 2, 2, 2)            # conv channel co * 4 + dy * 2 + dx
    return np.asarray(skip, np.float64) + y.transpose(0, 3, 1, 4, 2).reshape(2 * H, 2 * W, C // 2)


# ---- the data both test files use ------------------------------------------------------------------------------------------------
def engine_args(width, num_levels):
    """The shallowest NAFNet that has a block of every width up to width << num_levels: one block at level 0, one in the middle."""
    return dict(width=width, middle_blk_num=1, enc_blk_nums=(1,) + (0,) * (num_levels - 1), dec_blk_nums=(0,) * num_levels)


def lively_state(width, num_levels, seed=97):
    """synth.synthetic_nafnet_state with beta, gamma, sca.1.*, the biases of conv3 / conv5 of every block and of the down convs replaced by O(1) values (the
    synthetic ones are small: a block would be the identity plus a few percent, and the SCA scale its bias)."""
    from framewright_amd.synth import synthetic_nafnet_state
    sd = synthetic_nafnet_state(seed=seed, **engine_args(width, num_levels))
    rng = np.random.default_rng(seed + 1)
    for key in sorted(sd):
        shape = sd[key].shape
        if key.endswith("beta") or key.endswith("gamma") or key.endswith("sca.1.bias") or key.endswith("conv3.bias") or key.endswith("conv5.bias") or \
                (key.startswith("downs.") and key.endswith("bias")):
            sd[key] = (rng.uniform(0.5, 1.5, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
        elif key.endswith("sca.1.weight"):
            sd[key] = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    return sd


def lively_stream(H, W, c, seed):
    """fp32 [H][W][c]: per-channel scales 10^U(-1, 1) and means up to twice the scale - LayerNorm has something to do - and a quarter
    of the pixels scaled down to a variance over the channels near 1e-5, where LayerNorm's eps (1e-6) is a visible part of the result."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-1.0, 1.0, size=c)
    mean = scale * rng.uniform(-2.0, 2.0, size=c)
    x = mean + scale * rng.standard_normal((H, W, c))
    quiet = rng.random((H, W)) < 0.25
    quiet.flat[(H * W) // 2] = True
    x[quiet] *= 5e-4
    return x.astype(np.float32)
