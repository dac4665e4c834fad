"""Restormer block by block and step by step: what the engine runs for ONE transformer block (fw_restormer_run_block) or between two
stages (fw_restormer_run_step) against tests/restormer_block_ref.py in float64, on every kernel path a forward can take.

Yardstick (the form and factor of tests/test_nafblock_gpu.py): the float64 block is evaluated once more with values rounded to the
operand type at the rounding points of the path under test (restormer_block_ref lists them per path), q = max |rounded - exact|, and

    max |engine - exact| <= 2 q + 1e-6 max |exact|        and        mean |engine - exact| <= 2 mean |rounded - exact| + 1e-6 mean |exact|

for the stream and, with its own q, for the softmaxed attention matrix (fw_restormer_run_block's attn_out).  The host test shows on the
CPU that these bounds reject a clamped depthwise border, an unzeroed halo, a dirty qT slot, one temperature for all heads, x2 rows read
at hid, LayerNorm's eps at 1e-6 and - on the state whose GDFN x1 lies in GELU's tail, which is run here too - the tanh form of GELU.

One engine per (dtype, environment): num_blocks (1, 1, 1, 1), no refinement blocks, heads (1, 2, 4, 8) - a block at c = 48 (one head of
48), 96 (two heads of 48: encoder_level2; one head of 96: decoder_level1), 192 and 384.  FW_REST_FUSE_FRONT / MERGE_PROJ / QK_DIRECT /
MERGE_GROUPS / GEMM16 are read at create and set per engine here; FW_PW_DW_MFMA is read per launch.  FW_REST_DW_WIDE, FW_PW_SMALL_MAX_M
and FW_PW_GEMM_HALF are latched once per process: they are left alone (their defaults are what a forward runs), and no child process
is spawned for them.  Which kernels a block dispatches to is asserted on the handle (fw_restormer_block_paths); the choices made per
launch follow from the shapes, as noted next to them (_shapes).  That these ran is on record:
profiles/restormer_block_kernel_stats.csv is the kernel trace of this file on an MI355X."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import guarded
import restormer_block_ref as R
from framewright_amd import _lib
from framewright_amd.restormer import RestormerEngine

pytestmark = pytest.mark.gpu

F_QKV, F_FFN, QK, MERGE, GEMM16 = (_lib.FW_REST_PATH_FRONT_QKV, _lib.FW_REST_PATH_FRONT_FFN, _lib.FW_REST_PATH_QK_DIRECT, _lib.FW_REST_PATH_MERGE_PROJ,
                                   _lib.FW_REST_PATH_GEMM16)
FUSED = F_QKV | F_FFN
SWITCHES = ("FW_REST_FUSE_FRONT", "FW_REST_MERGE_PROJ", "FW_REST_QK_DIRECT", "FW_REST_MERGE_GROUPS", "FW_REST_GEMM16", "FW_PW_DW_MFMA")
# (block, environment, front model, merge_proj of the model, dispatch flags of the handle)
_fused = lambda key: [(key, {}, "pw_dw", True, FUSED | QK | MERGE),                              # pw_dw NONE with qT + GATE_GELU, Gram from qT, one residual GEMM
                      (key, {"FW_REST_QK_DIRECT": "0"}, "pw_dw", True, FUSED | MERGE),           # q / k pixel-major, qk_transpose_kernel: the same roundings
                      (key, {"FW_REST_MERGE_PROJ": "0"}, "pw_dw", False, FUSED | QK),            # attn_pack, a typed attn . v, project_out on its own
                      (key, {"FW_REST_FUSE_FRONT": "0"}, "staged", True, MERGE),                 # layernorm (16 / 32 lanes per pixel), pointwise_mfma STORE, the narrow depthwise kernel
                      (key, {"FW_PW_DW_MFMA": "1"}, "pw_dw_mfma", True, FUSED | QK | MERGE)]
_staged = lambda key: [(key, {}, "staged", True, MERGE | GEMM16),                                # pw_gemm STORE (rows padded to 256), the wide depthwise kernel at 576 ... 2048 channels
                       (key, {"FW_REST_GEMM16": "0"}, "staged", True, MERGE),                    # qkv / project_in on pointwise_mfma: the same roundings
                       (key, {"FW_REST_MERGE_PROJ": "0"}, "staged", False, GEMM16)]
PATHS = _fused("encoder_level1.0.") + _fused("encoder_level2.0.") + [p for p in _fused("decoder_level1.0.") if not ({"FW_REST_MERGE_PROJ", "FW_PW_DW_MFMA"} & set(p[1]))] + \
    _staged("encoder_level3.0.") + _staged("latent.0.")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up(v, m):
    return (v + m - 1) // m * m


def _shapes(key, front):
    """[(H, W, why)] - derived from the dispatch code; the CU count is the device's.  Sides are multiples of what the block's level leaves
    of a frame whose sides are multiples of 8: 8 at level 1 (and decoder_level1), 4 at level 2, 2 at level 3, 1 in the latent."""
    c, _ = R.BLOCKS[key]
    cus = _cus()
    if c <= 96:
        # pw_dw_kernel: 14 x 30 output tiles, pw_dw_blocks = min(tiles, CUs) workgroups, 448 qT slots per tile; unfused: layernorm + pointwise_mfma
        # (256- and 64-pixel tiles) + dwconv3x3_nhwc_kernel (4-row strips) + qk_transpose / Gram over pad32(pixels)
        shapes = [(8, 8, "one partial tile: 64 of its 448 qT slots are pixels"), (16, 32, "2 x 2 tiles: the second tile row 2 high, the second tile column 2 wide"),
                  (48, 64, "4 x 3 tiles, three of them full; 3072 pixels")]
        if front != "staged":      # there for the tile walk of pw_dw: not run where the fused front is off
            # More tiles than CUs in the fewest pixels: one tile column 8 wide, CUs + 1 tile rows, the last 8 high (30 k pixels on 256 CUs; a
            # near-square shape with as many tiles has 100 k, and its float64 reference takes 20 s)
            H, W = _up(14 * cus + 1, 8), 8
            assert -(-H // 14) > cus and H % 14
            shapes.append((H, W, f"{-(-H // 14)} pw_dw tiles on {cus} CUs: a workgroup takes a second tile; tiles {W} wide, the last {H % 14} high"))
        return shapes
    # c = 192 / 384: qkv / project_in on pw_gemm_kernel, 256-pixel tiles x 256 (half form: 128) channels; the half form runs while
    # 2 * pixel tiles * (N / 256) <= CUs, N = 768 and 1024 (c = 192), 1280 and 2048 (c = 384): the full form for BOTH needs the smaller N
    n_min = _up(3 * c, 256) // 256
    m_tiles = cus // (2 * n_min) + 1
    side = math.isqrt(256 * (m_tiles - 1)) + 1
    if c == 192:
        side = _up(side, 2)
    assert 2 * -(-side * side // 256) * n_min > cus
    shapes = [(1, 1, "one pixel"), (3, 5, "15 pixels, odd sides"), (9, 7, "63 pixels"), (17, 25, "425 pixels: two 256-pixel GEMM tiles; half form"),
              (side, side, f"{side * side} pixels: qkv and project_in in the full 256 x 256 form")]
    if c == 192:   # the residual GEMMs (6 cout tiles) leave pointwise_small_kernel (<= 16384 pixels, <= 12 tiles) for pointwise_mfma_kernel: CT = 4, a ragged second group
        shapes.append((128, 130, "16640 pixels: just above the 16384 of pointwise_small_kernel"))
    return shapes


@functools.lru_cache(maxsize=None)
def _state(gelu_tail=False):
    return R.lively_state(gelu_tail=gelu_tail)


@functools.lru_cache(maxsize=None)
def _weights(key, gelu_tail=False):
    return R.block_weights(_state(gelu_tail), key)


@functools.lru_cache(maxsize=None)
def _exact(key, H, W, gelu_tail=False):
    c, heads = R.BLOCKS[key]
    x = R.lively_stream(H, W, c, seed=H * 1000 + W)
    return x, R.restormer_block(x, _weights(key, gelu_tail), heads)[:2]


@functools.lru_cache(maxsize=None)
def _rounded(key, H, W, rt, front, merge, gelu_tail=False):
    return R.restormer_block(_exact(key, H, W, gelu_tail)[0], _weights(key, gelu_tail), R.BLOCKS[key][1], rt, front, merge)[:2]


class _Buf:
    """A float32 device tensor of `shape` between two guards (tests/guarded.py)."""

    def __init__(self, shape, fill=None):
        self.shape = tuple(shape)
        self.g = guarded.Guarded(int(np.prod(shape)), "f32")
        self.t = self.g.body().view(torch.float32).view(*self.shape)
        if fill is not None:
            self.t.fill_(fill)

    def load(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        return self.t

    def take(self):
        """The body as float32 bits' values; asserts that both guards are untouched."""
        return guarded.f32(self.g.take()).reshape(self.shape)


_ENGINES = {}


def _engine(dtype, env, gelu_tail=False):
    """One handle per (dtype, environment, state); the caller has the environment set (monkeypatch) - create reads it."""
    k = (dtype, tuple(sorted(env.items())), gelu_tail)
    if k not in _ENGINES:
        eng = RestormerEngine(dtype=dtype, **R.ENGINE_ARGS)
        eng.load_state_dict(_state(gelu_tail))
        _ENGINES[k] = eng
    return _ENGINES[k]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bounds(got, exact, rounded):
    err, q = np.abs(got - exact).max(), np.abs(rounded - exact).max()
    lim = 2 * q + 1e-6 * np.abs(exact).max()
    merr, mlim = np.abs(got - exact).mean(), 2 * np.abs(rounded - exact).mean() + 1e-6 * np.abs(exact).mean()
    return err, q, lim, merr, mlim


def _ratio(e, q):
    return e / q if q else (0.0 if e == 0 else math.inf)      # one pixel: the normalised q and k are +-1 and the attention model rounds nothing


def _check_block(eng, key, H, W, dtype, front, merge, why, failures, gelu_tail=False):
    c, heads = R.BLOCKS[key]
    cp, ch = R.stream_pad(c), c // heads
    x, (exact, a_exact) = _exact(key, H, W, gelu_tail)
    rounded, a_rounded = _rounded(key, H, W, dtype, front, merge, gelu_tail)
    buf, abuf = _Buf((H, W, cp)), _Buf((heads, ch, ch), fill=7.0)
    eng.run_block(buf.load(R.padded(x)), key, attn_out=abuf.t)
    raw, attn32 = buf.take(), abuf.take()
    got, attn = raw[..., :c].astype(np.float64), attn32.astype(np.float64)
    assert not raw[..., c:].any(), f"{H}x{W}: stream lanes {c} .. {cp - 1} are not zero"
    again = _Buf((H, W, cp))
    eng.run_block(again.load(R.padded(x)), key)                      # fixed-order reductions: the same bytes; attn_out is optional
    assert np.array_equal(again.take().view(np.uint32), raw.view(np.uint32)), f"{H}x{W}: a second run differs"
    err, q, lim, merr, mlim = _bounds(got, exact, rounded)
    aerr, aq, alim, amerr, amlim = _bounds(attn, a_exact, a_rounded)
    rows = np.abs(attn.sum(-1) - 1).max()
    print(f"{key} {dtype} {front}{'' if merge else ' unmerged'}{' gelu-tail' if gelu_tail else ''} {H}x{W}: error {err:.3e}, q {q:.3e}, error / q {err / q:.3f}, error / bound {err / lim:.3f}; "
          f"mean error / bound {merr / mlim:.3f}; attention error / q {_ratio(aerr, aq):.3f}, error / bound {aerr / alim:.3f}, mean error / bound {amerr / amlim:.3f}, "
          f"row sums within {rows:.1e}   [{why}]")
    for name, e, l in (("stream max", err, lim), ("stream mean", merr, mlim), ("attention max", aerr, alim), ("attention mean", amerr, amlim), ("attention row sums", rows, 1e-5)):
        if not e <= l:
            failures.append((H, W, name, float(e), float(l)))


def _path_id(p):
    return p[0].rstrip(".") + "-" + ("default" if not p[1] else "+".join(f"{k[3:]}={v}" for k, v in p[1].items()))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("key,env,front,merge,flags", PATHS, ids=[_path_id(p) for p in PATHS])
def test_block_against_float64(hip_lib, monkeypatch, key, env, front, merge, flags, dtype):
    """Measured on an MI355X: DESIGN.md (What pins Restormer's block paths) holds error / q per path and type."""
    _set_env(monkeypatch, env)
    eng = _engine(dtype, {k: v for k, v in env.items() if k != "FW_PW_DW_MFMA"})
    assert eng.block_paths(key) == flags, f"dispatch flags {eng.block_paths(key)}, expected {flags}"
    failures = []
    for H, W, why in _shapes(key, front):
        _check_block(eng, key, H, W, dtype, front, merge, why, failures)
    assert not failures, failures


# the state whose GDFN x1 lies in GELU's tail (restormer_block_ref.lively_state): both GATE_GELU instances of pw_dw, both depthwise kernels in mode 1
TAIL = [("encoder_level1.0.", {}, "pw_dw", 16, 32), ("encoder_level1.0.", {"FW_REST_FUSE_FRONT": "0"}, "staged", 16, 32), ("encoder_level1.0.", {"FW_PW_DW_MFMA": "1"}, "pw_dw_mfma", 16, 32),
        ("encoder_level2.0.", {}, "pw_dw", 12, 20), ("encoder_level3.0.", {}, "staged", 10, 6), ("latent.0.", {}, "staged", 5, 7)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_gelu_tail_against_float64(hip_lib, monkeypatch, dtype):
    """x1 near -3 everywhere: erf GELU and its tanh form differ by more than the bound there (tests/test_restormer_block_ref_host.py)."""
    failures = []
    for key, env, front, H, W in TAIL:
        _set_env(monkeypatch, env)
        eng = _engine(dtype, {k: v for k, v in env.items() if k != "FW_PW_DW_MFMA"}, gelu_tail=True)
        _check_block(eng, key, H, W, dtype, front, True, "GELU's tail", failures, gelu_tail=True)
    assert not failures, failures


def test_single_steps_reject_what_they_cannot_run(hip_lib, monkeypatch):
    _set_env(monkeypatch, {})
    eng = RestormerEngine(dtype="f16", **R.ENGINE_ARGS)
    x = torch.zeros((8, 8, 64), dtype=torch.float32, device="cuda")
    run = lambda key, h=8, w=8: eng._lib.fw_restormer_run_block(eng._h, key, x.data_ptr(), h, w, None, None)
    assert run(b"encoder_level1.0.") == _lib.FW_ERR_INVALID                       # no weights yet: not finalizable
    eng.load_state_dict(_state())
    for key in (b"encoder_level1.1.", b"refinement.0.", b"nonsense", b"encoder_level1.0.attn.qkv.weight", b"encoder_level1.0", b""):
        assert run(key) == _lib.FW_ERR_INVALID, key
    for h, w in ((0, 8), (8, 0), (-1, 8), (16385, 8)):
        assert run(b"encoder_level1.0.", h, w) == _lib.FW_ERR_INVALID
    flags = C.c_int(0)
    assert eng._lib.fw_restormer_block_paths(eng._h, b"latent.1.", C.byref(flags)) == _lib.FW_ERR_INVALID
    step = lambda name, h, w, skip=None: eng._lib.fw_restormer_run_step(eng._h, name, x.data_ptr(), skip, h, w, x.data_ptr(), None)
    assert step(b"down4_5", 2, 2) == _lib.FW_ERR_INVALID                          # no such step
    assert step(b"down1_2", 3, 2) == _lib.FW_ERR_INVALID                          # odd side
    assert step(b"up2_1", 2, 2) == _lib.FW_ERR_INVALID                            # no skip stream
    assert step(b"output", 0, 2) == _lib.FW_ERR_INVALID
    with pytest.raises(ValueError):
        eng.run_block(x, "latent.0.")                                              # 384 channels
    with pytest.raises(ValueError):
        eng.run_step("down1_2", x, x)                                              # dst of the wrong shape
    eng.close()


# ---- the steps between the stages -------------------------------------------------------------------------------------------------
# source sizes: a few pixels, and about 300 pixels with odd sides at the low resolution (the down steps: of their output).  The merged conv
# launch (Conv3::wall) has 2 groups for down3_4 and 12 / 6 / 3 for the up convs; down1_2, down2_3 and output are single-group convs either way.
STEP_SHAPES = {"down": [(2, 2, "one output pixel"), (6, 10, "3 x 5 outputs"), (26, 46, "13 x 23 outputs: 299")],
               "up": [(1, 1, "one source pixel"), (3, 5, "odd sides"), (13, 23, "299 source pixels, odd sides")],
               "output": [(1, 1, "one pixel"), (5, 7, "odd sides"), (13, 23, "299 pixels, odd sides")]}


@functools.lru_cache(maxsize=None)
def _step_case(step, H, W):
    w3, wred = R.step_weights(_state(), step)
    i = R.STEPS.index(step)
    x = R.lively_stream(H, W, w3.shape[1], seed=31 + i)
    skip = R.lively_stream(2 * H, 2 * W, w3.shape[0] // 4, seed=41 + i) if step.startswith("up") else None
    return x, skip, R.run_step(step, x, w3, wred, skip), {rt: R.run_step(step, x, w3, wred, skip, rt) for rt in ("f16", "bf16")}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("env", [{}, {"FW_REST_MERGE_GROUPS": "0"}], ids=["default", "REST_MERGE_GROUPS=0"])
def test_steps_against_float64(hip_lib, monkeypatch, env, dtype):
    """The three down steps, the three up steps and the output conv with the launches a forward issues: max and mean error within 2 q
    (+ 1e-6) of their own rounded model, zeros in the lanes of dst behind the real channels, src and skip unchanged, guards untouched."""
    _set_env(monkeypatch, env)
    eng = _engine(dtype, env)
    failures = []
    for step in R.STEPS:
        for H, W, why in STEP_SHAPES[step.rstrip("0123456789_")]:
            x, skip, exact, rounded = _step_case(step, H, W)
            sshape, kshape, dshape = eng.step_shapes(step, H, W)
            src, dst = _Buf(sshape), _Buf(dshape, fill=7.0)                        # the step overwrites every lane of dst
            sk = _Buf(kshape) if kshape else None
            eng.run_step(step, src.load(R.padded(x)), dst.t, sk.load(R.padded(skip)) if sk else None)
            raw = dst.take()
            assert np.array_equal(src.take(), R.padded(x)) and (sk is None or np.array_equal(sk.take(), R.padded(skip))), (step, H, W)
            creal = exact.shape[-1]
            assert raw.shape[:2] == exact.shape[:2] and not raw[..., creal:].any(), (step, H, W, "lanes behind the real channels")
            again = _Buf(dshape, fill=-3.0)
            eng.run_step(step, src.t, again.t, sk.t if sk else None)
            assert np.array_equal(again.take().view(np.uint32), raw.view(np.uint32)), (step, H, W, "a second run differs")
            err, q, lim, merr, mlim = _bounds(raw[..., :creal].astype(np.float64), exact, rounded[dtype])
            print(f"{step} {dtype} {'merged' if not env else 'group by group'} {H}x{W}: error {err:.3e}, q {q:.3e}, error / q {err / q:.3f}, error / bound {err / lim:.3f}, "
                  f"mean error / bound {merr / mlim:.3f}   [{why}]")
            if not (err <= lim and merr <= mlim):
                failures.append((step, H, W, float(err), float(lim), float(merr), float(mlim)))
    assert not failures, failures
