"""NAFNet block by block and level change by level change: what the engine runs for ONE block (fw_nafnet_run_block) or one down / up
step (fw_nafnet_run_resample) against tests/nafblock_ref.py in float64, on every kernel path a forward can take.

Yardstick (the form and factor of tests/test_ifnet_blocks_gpu.py): the float64 block is evaluated once more with values rounded to
the operand type at the rounding points of the path under test (nafblock_ref lists them per path), q = max |rounded - exact|, and

    max |engine - exact| <= 2 q + 1e-6 max |exact|        and        mean |engine - exact| <= 2 mean |rounded - exact| + 1e-6 mean |exact|

(a bias across the tensor does not hide under a max).  The SCA vector is held to the rounded model's SCA vector within a bound of fp32
terms only, derived in _sca_bound; per shape and type the test also shows, on the CPU, that losing any single row of the pooling's
partial sums would exceed it.

Engines are as deep as the block needs (nafblock_ref.engine_args): width 64 with 1 / 2 / 3 / 4 levels has its middle block at
c = 128 / 256 / 512 / 1024 and a level-0 block at c = 64; width 32 gives c = 32.  A middle block sees any size, a level-0 block of a
one-level net even sides: every shape below is one a forward can issue.

The switches FW_NAF_FUSE_FRONT / FUSE_TAIL / FUSE_LN / GEMM are read at create and set per engine here; FW_PW_DW_MFMA is read per
launch.  FW_NAF_DW_WIDE, FW_PW_SMALL_MAX_M and FW_PW_GEMM_HALF are latched once per process: they are left alone (their defaults are
what a forward runs), and no child process is spawned for them.  Which fused kernels a block dispatches to is asserted on the
handle (fw_nafnet_block_paths); the choices made per launch follow from the shapes, as noted next to them:
pointwise_small_kernel takes typed STORE / RESIDUAL GEMMs of at most 16384 pixels and 12 cout tiles (c = 32: conv1, conv5; c = 64 / 128 unfused:
conv5; c = 256 with FW_NAF_GEMM=0: conv5), pointwise_mfma_kernel the rest; dwconv3x3_gate_wide_kernel is c >= 256.  That these ran is on
record: profiles/nafblock_kernel_stats.csv is the kernel trace of this file on an MI355X (every form named here, pw_gemm in its full and
its half form included)."""
import functools
import math

import numpy as np
import pytest
import torch

import nafblock_ref as R
from framewright_amd import _lib
from framewright_amd.tap_denoise import NAFNetEngine

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
FRONT, TAIL128, TAIL64, GEMM, FUSE_LN = (_lib.FW_NAF_PATH_FRONT, _lib.FW_NAF_PATH_TAIL128, _lib.FW_NAF_PATH_TAIL64, _lib.FW_NAF_PATH_GEMM,
                                         _lib.FW_NAF_PATH_FUSE_LN)
# c -> (width, levels, key of the block, key of a block of another width on the same handle)
BLOCKS = {32: (32, 1, "encoders.0.0.", "middle_blks.0."), 64: (64, 1, "encoders.0.0.", "middle_blks.0."), 128: (64, 1, "middle_blks.0.", "encoders.0.0."),
          256: (64, 2, "middle_blks.0.", "encoders.0.0."), 512: (64, 3, "middle_blks.0.", "encoders.0.0."), 1024: (64, 4, "middle_blks.0.", "encoders.0.0.")}
# (c, environment, front model, tail model, dispatch flags of the handle)
PATHS = [
    (32, {}, "plain", "act_scale", 0),                                                           # layernorm2d + pointwise_small / _mfma + narrow dwconv + SCA
    (64, {}, "pw_dw", "act_scale", FRONT | TAIL64),                                              # pw_dw (2 chunks) + naf_tail64
    (64, {"FW_NAF_FUSE_FRONT": "0"}, "plain", "act_scale", TAIL64 | FUSE_LN),                    # norm1 inside conv1's staging, narrow dwconv
    (64, {"FW_NAF_FUSE_TAIL": "0"}, "pw_dw", "act_scale", FRONT | FUSE_LN),                      # a_scale conv3, norm2 inside conv4's staging, gate, conv5
    (64, {"FW_NAF_FUSE_FRONT": "0", "FW_NAF_FUSE_TAIL": "0", "FW_NAF_FUSE_LN": "0"}, "plain", "act_scale", 0),   # layernorm2d_kernel (16 lanes per pixel) for both norms
    (64, {"FW_NAF_FUSE_LN": "0"}, "pw_dw", "act_scale", FRONT | TAIL64),                         # the switch alone: the fused kernels still take the block
    (64, {"FW_PW_DW_MFMA": "1"}, "pw_dw_mfma", "act_scale", FRONT | TAIL64),
    (128, {}, "pw_dw", "tail128", FRONT | TAIL128),                                              # pw_dw (4 chunks) + naf_tail128
    (128, {"FW_NAF_FUSE_FRONT": "0"}, "plain", "tail128", TAIL128),                              # layernorm2d (32 lanes per pixel)
    (128, {"FW_NAF_FUSE_TAIL": "0"}, "pw_dw", "act_scale", FRONT),
    (128, {"FW_PW_DW_MFMA": "1"}, "pw_dw_mfma", "tail128", FRONT | TAIL128),
    (256, {}, "plain", "w3_scale", GEMM), (256, {"FW_NAF_GEMM": "0"}, "plain", "act_scale", 0),   # layernorm2d (64 lanes) + GEMM STORE / GATE / RESIDUAL + wide dwconv
    (512, {}, "plain", "w3_scale", GEMM), (512, {"FW_NAF_GEMM": "0"}, "plain", "act_scale", 0),
    (1024, {}, "plain", "w3_scale", GEMM), (1024, {"FW_NAF_GEMM": "0"}, "plain", "act_scale", 0),
]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _shapes(c, front="pw_dw"):
    """[(H, W, why)] - derived from the dispatch code; the CU count is the device's."""
    cus = _cus()
    if c == 32:      # dwconv3x3_gate_kernel: one thread per (3-row strip, column, 8 channels), 256 per block; pointwise tiles of 256 / 64 pixels
        return [(2, 2, "4 pixels: one partial tile everywhere"), (6, 10, "dwconv_blocks = 1, two full strips; 60 pixels < a 64-pixel tile"),
                (8, 10, "last strip of GATE_ROWS = 3 has 2 rows"), (16, 22, "3 dwconv blocks, ragged strip, 352 pixels: 2 tiles of 256, 6 of 64")]
    if c in (64, 128):
        ty = cus // 15 + 1     # 15 tile columns x ty tile rows > front_cus(): some workgroup of pw_dw walks a second tile (tail64 / tail128: > 256 tiles too)
        big = (14 * (ty - 1) + 2, 30 * 14 + 2, f"{15 * ty} pw_dw tiles on {cus} CUs: a workgroup takes a second tile; last tile row and column 2 wide")
        small = [(6, 10, "60 pixels: below one 64-pixel wave slice; narrow dwconv: one block"), (18, 14, "252 pixels: a 256-pixel tile short of 4")] if c == 64 else \
                [(9, 7, "63 pixels, odd sides"), (17, 25, "425 pixels: 2 tiles of 256, the second 169 = 2 wave slices + 41")]
        # (the many-tile shape is 100 k pixels and there for pw_dw's tile walk: not run where the fused front is off)
        return small + [(16, 16, "pw_dw: two tile rows, the second with 2 rows; narrow dwconv: ragged strip"), (16, 32, "pw_dw: two tile columns, the second 2 wide"),
                        (48, 64, "pw_dw: 4 x 3 tiles; 3072 pixels")] + ([big] if front != "plain" else [])
    # c >= 256: GEMM tiles of 256 pixels x 256 (half form: 128) channels; the half form runs while 2 * tiles <= gemm_cus()
    n5 = c // 256                                              # channel tiles of conv3 / conv5 (conv1: twice as many)
    m_tiles = cus // (2 * n5) + 1                             # 2 * m_tiles * n5 > cus: conv3 / conv5 too
    side = math.isqrt(256 * (m_tiles - 1)) + 1
    while side * side <= 256 * (m_tiles - 1):
        side += 1
    what = "every GEMM of the block in the full 256 x 256 form"
    rows_cap = 768 // (c // 256)
    cap = ((side + 2) // 3 * side + 7) // 8 > rows_cap
    return [(1, 1, "one pixel"), (3, 5, "15 pixels, odd sides"), (9, 7, "63 pixels"), (17, 25, "425 pixels: two pixel tiles; half form"),
            (side, side, f"{side * side} pixels: {what}" + ("; dwconv_wide_rows at its DW_MAX_BLOCKS cap" if cap else ""))]


@functools.lru_cache(maxsize=None)
def _state(width, levels):
    return R.lively_state(width, levels)


@functools.lru_cache(maxsize=None)
def _exact(c, H, W):
    width, levels, key, _ = BLOCKS[c]
    x = R.lively_stream(H, W, c, seed=H * 1000 + W)
    return x, R.nafblock(x, R.block_weights(_state(width, levels), key))


@functools.lru_cache(maxsize=None)
def _rounded(c, H, W, rt, front, tail):
    width, levels, key, _ = BLOCKS[c]
    return R.nafblock(_exact(c, H, W)[0], R.block_weights(_state(width, levels), key), rt, front, tail)


def _pool_depth(front, H, W, c, cus):
    """Upper bound on the number of fp32 additions a gated value passes through on its way into the pooled mean (the kernels' fixed trees)."""
    if front != "plain":                                       # pw_dw: 7 rows per lane and tile, one add per tile, 6 shuffle levels
        tiles = -(-H // 14) * -(-W // 30)
        blocks = min(tiles, cus)
        own = 7 + -(-tiles // blocks) + 6
    elif c >= 256:                                             # wide dwconv: 3 rows per item, items of a thread, 8 threads per channel
        cols = -(-H // 3) * W
        blocks = min(-(-cols // 8), 768 // (c // 256))
        own = 3 * -(-cols // (blocks * 8)) + 8
    else:                                                      # narrow dwconv: 3 rows per item, items of a thread, 256 / (c / 8) threads per channel
        total = -(-H // 3) * W * (c // 8)
        blocks = min(-(-total // 256), 768)
        own = 3 * -(-total // (blocks * 256)) + 2048 // c
    return own + -(-blocks // 16) + 16 + 12                    # sca_mean_kernel: blocks / 16 in sequence, 16 slices; 12: the 9 taps, bias and product of the value itself


def _sca_bound(w, parts, rt, front, H, W, c):
    """|sca_engine - sca_rounded|[n], against the operand-rounded MODEL's SCA vector (the roundings in front of the pooling - norm1's
    output, conv1's weights and output - are in the model, so they are no term here; the pooling sums the unrounded gated values, so
    their typed rounding is none either).  What is left:
      * fp32 summation of the H W gated values per channel in the kernel's fixed tree of depth D (_pool_depth): at most
        D 2^-24 mean |g_k| on the pooled mean of channel k, which reaches output n through |W[n][k]|;
      * the fp32 dot product of length c, 64 lanes with c / 64 terms each + 6 shuffle levels, the 1 / (H W) factor and the bias:
        (c / 64 + 12) 2^-24 (sum_k |W[n][k]| |mean_k| + |b_n|);
      * what the model cannot say: the engine forms norm1's and conv1's outputs in fp32 in its own order, so a typed value that sits
        within the fp32 error of a rounding midpoint comes out as its neighbour.  The fp32 error of a sum of c terms is about
        sqrt(c) 2^-24 relative, a value of the type is at least 2^-11 (f16) / 2^-8 (bf16) of itself away from its neighbour's midpoint
        range, so a conv1 output flips with probability p <= 2 sqrt(c) 2^-24 / 2^-11 (2^-8); a flipped norm1 output moves the 2 c
        conv1 outputs of its pixel by |w1| ulps and flips them in that proportion: p_eff = p (1 + c mean |w1|).  A flip moves a
        conv1 output by r = 2^-10 (2^-7) of itself at most and with it the 9 gated values it feeds - taken as moving together: a
        factor sqrt(9) - by r |tap t| |partner| each; parts["sens"] is the rms over the pixels of that sum over a gated value's 18
        inputs.  Flips are independent events with either sign, so the pooled mean of channel k moves by a random sum of standard
        deviation 3 r sqrt(p_eff / (H W)) sens_k at most, channels add in quadrature through W[n][k], and 6 standard deviations
        are allowed.
    Losing one row of `partial` moves the mean by that workgroup's share of it; _lost_row_margin shows on the CPU, per shape and type,
    that every single row's loss is outside this bound."""
    u = 2.0 ** -24
    A = np.abs(w["wsca"])
    D = _pool_depth(front, H, W, c, _cus())
    relulp, r = (2.0 ** -11, 2.0 ** -10) if rt == "f16" else (2.0 ** -8, 2.0 ** -7)
    p_eff = 2 * math.sqrt(c) * u / relulp * (1 + c * parts["w1_mean_abs"])
    flips = 6 * 3 * r * math.sqrt(p_eff / (H * W)) * np.sqrt((A * A) @ (parts["sens"] ** 2))
    return flips + A @ (D * u * np.abs(parts["g"]).mean((0, 1))) + (c // 64 + 12) * u * (A @ np.abs(parts["pooled"]) + np.abs(w["bsca"]))


def _lost_row_margin(w, parts, slim, front, H, W, c):
    """min over the rows of `partial` of max_n |effect of not summing that row on sca[n]| / bound[n]; inf where there is one row."""
    rows, nrows = R.partial_rows(front, H, W, c, _cus())
    if nrows < 2:
        return math.inf
    return float((np.abs(R.lost_row_effects(parts["g"], w["wsca"], rows, nrows)) / slim).max(1).min())


class _Guarded:
    """A float32 CUDA buffer of `shape` between two runs of sentinels."""
    PAD, SENTINEL = 4096, -12345.5

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * self.PAD,), self.SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.whole[self.PAD:self.PAD + n].view(*shape)

    def load(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        return self.t

    def intact(self):
        return bool((self.whole[:self.PAD] == self.SENTINEL).all() and (self.whole[-self.PAD:] == self.SENTINEL).all())


def _engine(width, levels, dtype):
    eng = NAFNetEngine(dtype=dtype, **R.engine_args(width, levels))
    eng.load_state_dict(_state(width, levels))
    return eng


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("c,env,front,tail,flags", PATHS, ids=[f"c{p[0]}-" + ("default" if not p[1] else "+".join(f"{k[3:]}={v}" for k, v in p[1].items())) for p in PATHS])
def test_block_against_float64(hip_lib, monkeypatch, c, env, front, tail, flags, dtype):
    """Measured on an MI355X: DESIGN.md (What pins K6's NAFNet paths) holds error / q per path and type."""
    for k in ("FW_NAF_FUSE_FRONT", "FW_NAF_FUSE_TAIL", "FW_NAF_FUSE_LN", "FW_NAF_GEMM", "FW_PW_DW_MFMA", "FW_NAF_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    width, levels, key, other = BLOCKS[c]
    sd = _state(width, levels)
    w = R.block_weights(sd, key)
    eng = _engine(width, levels, dtype)
    assert eng.block_paths(key) == flags, f"dispatch flags {eng.block_paths(key)}, expected {flags}"
    sca = torch.empty(c, dtype=torch.float32, device="cuda")
    c_other = R.block_weights(sd, other)["beta"].size
    failures = []
    for i, (H, W, why) in enumerate(_shapes(c, front)):
        x, (exact, s_exact, parts) = _exact(c, H, W)
        rounded, s_rounded, mparts = _rounded(c, H, W, dtype, front, tail)
        buf = _Guarded((H, W, c))
        eng.run_block(buf.load(x), key, sca_out=sca)
        got, s_got = buf.t.cpu().numpy().astype(np.float64), sca.cpu().numpy().astype(np.float64)
        assert buf.intact(), f"{H}x{W}: wrote outside the stream buffer"
        # the same block again, a block of another width in between (shared csum / sca / w3s scratch): bit-equal
        eng.run_block(torch.from_numpy(R.lively_stream(8, 8, c_other, seed=5)).cuda(), other)
        again = eng.run_block(buf.load(x), key).cpu().numpy()
        assert np.array_equal(again.astype(np.float64), got), f"{H}x{W}: second run differs"
        err, q = np.abs(got - exact).max(), np.abs(rounded - exact).max()
        lim = 2 * q + 1e-6 * np.abs(exact).max()
        merr, mlim = np.abs(got - exact).mean(), 2 * np.abs(rounded - exact).mean() + 1e-6 * np.abs(exact).mean()
        serr, slim = np.abs(s_got - s_rounded), _sca_bound(w, mparts, dtype, front, H, W, c)
        margin = _lost_row_margin(w, mparts, slim, front, H, W, c)
        print(f"c {c} {dtype} {front}/{tail} {H}x{W}: error {err:.3e}, q {q:.3e}, error / q {err / q:.3f}, error / bound {err / lim:.3f}; mean error / bound "
              f"{merr / mlim:.3f}; SCA |engine - model| / bound {(serr / slim).max():.3f} (error {serr.max():.3e}, model - exact {np.abs(s_rounded - s_exact).max():.3e}, weakest lost row / bound "
              f"{margin:.1f})   [{why}]")
        assert margin > 1.5, f"{H}x{W}: the SCA bound would let the loss of one row of partial sums pass ({margin:.2f})"
        if not err <= lim:
            failures.append((H, W, "block max", err, lim))
        if not merr <= mlim:
            failures.append((H, W, "block mean", merr, mlim))
        if not (serr <= slim).all():
            failures.append((H, W, "sca", serr.max(), float(slim[np.argmax(serr / slim)])))
        # neither half of the block is inert
        assert np.abs(got - x).max() > 100 * lim, (H, W, np.abs(got - x).max(), lim)
        if i == 1:
            for name in ("beta", "gamma"):
                zero = np.zeros_like(sd[key + name])
                _lib.check(eng._lib.fw_nafnet_set_tensor(eng._h, (key + name).encode(), zero.ctypes.data, zero.size))
                without = eng.run_block(buf.load(x), key).cpu().numpy().astype(np.float64)
                _lib.check(eng._lib.fw_nafnet_set_tensor(eng._h, (key + name).encode(), sd[key + name].ctypes.data, sd[key + name].size))
                assert np.abs(without - got).max() > 10 * lim, (name, np.abs(without - got).max(), lim)
            assert np.array_equal(eng.run_block(buf.load(x), key).cpu().numpy().astype(np.float64), got), "restoring beta / gamma does not restore the result"
    eng.close()
    assert not failures, failures


def test_run_block_rejects_what_it_cannot_run(hip_lib):
    eng = NAFNetEngine(dtype="f16", **R.engine_args(64, 1))
    x = torch.zeros((4, 4, 64), dtype=torch.float32, device="cuda")
    rc = eng._lib.fw_nafnet_run_block(eng._h, b"encoders.0.0.", x.data_ptr(), 4, 4, None, None)
    assert rc == _lib.FW_ERR_INVALID                                   # no weights yet: not finalizable
    eng.load_state_dict(_state(64, 1))
    for key in (b"encoders.0.1.", b"encoders.1.0.", b"middle_blks.1.", b"decoders.0.0.", b"nonsense", b"encoders.0.0.conv1.weight"):
        assert eng._lib.fw_nafnet_run_block(eng._h, key, x.data_ptr(), 4, 4, None, None) == _lib.FW_ERR_INVALID, key
    for h, w_ in ((0, 4), (4, 0), (-1, 4)):
        assert eng._lib.fw_nafnet_run_block(eng._h, b"encoders.0.0.", x.data_ptr(), h, w_, None, None) == _lib.FW_ERR_INVALID
    assert eng._lib.fw_nafnet_run_resample(eng._h, 1, 0, x.data_ptr(), 4, 4, x.data_ptr(), None) == _lib.FW_ERR_INVALID   # no such level
    assert eng._lib.fw_nafnet_run_resample(eng._h, 0, 0, x.data_ptr(), 3, 4, x.data_ptr(), None) == _lib.FW_ERR_INVALID   # odd side
    with pytest.raises(ValueError):
        eng.run_block(x, "middle_blks.0.")                             # 128 channels
    eng.close()


# ---- level changes ----------------------------------------------------------------------------------------------------------------
# (width, levels, level, H, W of the source, why).  Down: level l of an L-level net sees multiples of 2^(L - l) per side, so the output
# has an odd number of columns only at the deepest level; the shallower engines supply odd columns for the narrower convs.
DOWNS = [(32, 1, 0, 2, 2, "one output pixel, N_tiles = 2"), (32, 1, 0, 6, 10, "3 x 5 outputs: odd columns at c = 32"), (64, 1, 0, 18, 30, "9 x 15 outputs: odd columns at c = 64"),
         (64, 4, 0, 48, 32, "384 outputs: a ragged second pixel tile"), (64, 2, 1, 6, 10, "odd columns at c = 128"), (64, 4, 1, 8, 24, "c = 128, K = 512"),
         (64, 3, 2, 6, 10, "odd columns at c = 256"), (64, 4, 2, 4, 12, "c = 256, K = 1024"), (64, 4, 3, 6, 10, "3 x 5 outputs at c = 512, K = 2048: 64 chunks"),
         (64, 4, 3, 2, 2, "one output pixel at K = 2048")]
# up INTO `level`: the source has H x W pixels of 2 c' channels, N_tiles = 4 c' / 32
UPS = [(32, 1, 0, 1, 1, "N_tiles = 4: the smallest N_tiles % 4 == 0; one source pixel"), (32, 1, 0, 3, 5, "N_tiles = 4, odd sides"), (64, 1, 0, 9, 15, "N_tiles = 8, odd sides"),
       (64, 4, 0, 24, 16, "384 source pixels: a ragged second pixel tile"), (64, 4, 1, 4, 12, "N_tiles = 16"), (64, 4, 2, 2, 6, "N_tiles = 32"),
       (64, 4, 3, 3, 5, "N_tiles = 64, K = 1024, odd sides"), (64, 4, 3, 1, 1, "one source pixel at K = 1024")]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_level_changes_against_float64(hip_lib, dtype):
    """The 2x2 stride-2 convs (gather-2x2 pointwise, fp32 out) and the up steps (1x1, PixelShuffle, add into a non-zero skip buffer) with
    the PointwiseParams the forward builds: max and mean error within 2 q (+ 1e-6) of their own rounded model (x and weights typed)."""
    engines, failures = {}, []
    for kind, cases in (("down", DOWNS), ("up", UPS)):
        for width, levels, level, H, W, why in cases:
            if (width, levels) not in engines:
                engines[(width, levels)] = _engine(width, levels, dtype)
            eng, sd, c = engines[(width, levels)], _state(width, levels), width << level
            if kind == "down":
                x = R.lively_stream(H, W, c, seed=31 + level)
                wt, b = sd[f"downs.{level}.weight"], sd[f"downs.{level}.bias"]
                exact, rounded = R.down(x, wt, b), R.down(x, wt, b, dtype)
                src, dst = _Guarded((H, W, c)), _Guarded((H // 2, W // 2, 2 * c))
                dst.load(np.full((H // 2, W // 2, 2 * c), 7.0))                        # the conv overwrites
            else:
                x, skip = R.lively_stream(H, W, 2 * c, seed=41 + level), R.lively_stream(2 * H, 2 * W, c, seed=51 + level)
                wt = sd[f"ups.{levels - 1 - level}.0.weight"]
                exact, rounded = R.up(x, wt, skip), R.up(x, wt, skip, dtype)
                src, dst = _Guarded((H, W, 2 * c)), _Guarded((2 * H, 2 * W, c))
                dst.load(skip)
            eng.run_resample(src.load(x), level, kind == "up", dst.t)
            got = dst.t.cpu().numpy().astype(np.float64)
            assert src.intact() and dst.intact() and np.array_equal(src.t.cpu().numpy(), x), (kind, width, levels, level, H, W)
            err, q = np.abs(got - exact).max(), np.abs(rounded - exact).max()
            lim = 2 * q + 1e-6 * np.abs(exact).max()
            merr, mlim = np.abs(got - exact).mean(), 2 * np.abs(rounded - exact).mean() + 1e-6 * np.abs(exact).mean()
            print(f"{kind} {dtype} width {width} levels {levels} level {level} {H}x{W}: error {err:.3e}, q {q:.3e}, error / q {err / q:.3f}, error / bound {err / lim:.3f}, "
                  f"mean error / bound {merr / mlim:.3f}   [{why}]")
            if not (err <= lim and merr <= mlim):
                failures.append((kind, width, levels, level, H, W, err, lim, merr, mlim))
    for eng in engines.values():
        eng.close()
    assert not failures, failures


# ---- pre and post kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (37, 51)])
def test_tap_post_is_bit_exact(hip_lib, H, W):
    """fw_tap_post_u8: v = rgb + in / 255 in float32, uint8(clip(v * 255, 0, 255)) TRUNCATED (oracle/tap_ref.postprocess), RGB -> BGR; the
    crop from a padded width, the channel stride, the optional float32 output, and values on k / 255 and one float below."""
    rng = np.random.default_rng(H * 100 + W)
    Wp, cs = W + 11, 5
    frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rgb = rng.uniform(-0.6, 0.6, size=(H, Wp, cs)).astype(np.float32)
    k = rng.integers(0, 256, size=(H, W, 3)).astype(np.float32)
    on = k / np.float32(255.0)
    edge = np.where(rng.random((H, W, 3)) < 0.5, on, np.nextafter(on, np.float32(-1.0)))
    third = rng.random((H, W)) < 0.34
    frame[third] = 0                                               # in / 255 = 0: v is exactly k / 255 or the float below it
    rgb[:, :W, :3][third] = edge[third]
    if H * W > 1:
        rgb[0, 0, :3] = (-0.5, 2.0, 1.0)                           # clips at both ends (frame[0, 0] may add up to 1)
    v = rgb[:, :W, :3] + frame[:, :, ::-1].astype(np.float32) / np.float32(255.0)
    want = np.clip(v * np.float32(255.0), 0, 255).astype(np.uint8)[:, :, ::-1]
    rounded = np.clip(np.rint(v * np.float32(255.0)), 0, 255).astype(np.uint8)[:, :, ::-1]
    d_in, d_rgb = torch.from_numpy(frame).cuda(), torch.from_numpy(rgb).cuda()
    out = torch.full((H * W * 3 + 64,), 171, dtype=torch.uint8, device="cuda")
    f32 = torch.full((H * W * 3 + 64,), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(hip_lib.fw_tap_post_u8(d_in.data_ptr(), d_rgb.data_ptr(), H, W, Wp, cs, out.data_ptr(), f32.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(out[:H * W * 3].cpu().numpy().reshape(H, W, 3), want)
    assert np.array_equal(f32[:H * W * 3].cpu().numpy().reshape(H, W, 3), v)
    assert bool((out[H * W * 3:] == 171).all()) and bool((f32[H * W * 3:] == -7.0).all())
    if H * W > 1:
        assert not np.array_equal(want, rounded)                   # the data tells truncation from rounding
    only = torch.full((H * W * 3,), 171, dtype=torch.uint8, device="cuda")
    _lib.check(hip_lib.fw_tap_post_u8(d_in.data_ptr(), d_rgb.data_ptr(), H, W, Wp, cs, only.data_ptr(), None, None))    # the float32 output is optional
    torch.cuda.synchronize()
    assert torch.equal(only, out[:H * W * 3])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (37, 51)])
def test_u8_to_nhwc_padded_is_bit_exact(hip_lib, H, W, dtype):
    """NAFNet's pre-processing: BGR -> RGB, float32 division by 255 rounded once to the operand type, zeros in channels 3..31 and in the
    padding rows and columns."""
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    frame = np.random.default_rng(H + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    frame.flat[:3] = (0, 255, 128)
    out = torch.full((Hp * Wp * 32 + 64,), 3.0, dtype=TDT[dtype], device="cuda")
    _lib.check(hip_lib.fw_u8_to_nhwc_padded(_lib.DTYPES[dtype], torch.from_numpy(frame).cuda().data_ptr(), H, W, Hp, Wp, out.data_ptr(), None))
    torch.cuda.synchronize()
    want = torch.zeros((Hp, Wp, 32), dtype=TDT[dtype])
    want[:H, :W, :3] = torch.from_numpy(frame[:, :, ::-1].astype(np.float32) / np.float32(255.0)).to(TDT[dtype])
    got = out[:Hp * Wp * 32].cpu().view(Hp, Wp, 32)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool((out[Hp * Wp * 32:] == 3.0).all())
    assert hip_lib.fw_u8_to_nhwc_padded(_lib.DTYPES[dtype], out.data_ptr(), H, W, H - 1, Wp, out.data_ptr(), None) == _lib.FW_ERR_INVALID
