"""The RRDBNet trunk RRDB by RRDB: what the engine runs for RRDBs first .. first + count - 1 (fw_rrdbnet_run_rrdbs: the loop body of
csrc/rrdbnet.hip's forward, with the workspace, buffer rotation and residual sources of a forward) against tests/rrdb_block_ref.py in
float64, on every kernel path a forward can take.

Yardstick (the form and factor of tests/test_nafblock_gpu.py and tests/test_restormer_blocks_gpu.py): the float64 RRDB is evaluated once
more with values rounded to the operand type at the rounding points of the path under test (rrdb_block_ref lists them per path),
q = max |rounded - exact|, and

    max |engine - exact| <= 2 q + 1e-6 max |exact|        and        mean |engine - exact| <= 2 mean |rounded - exact| + 1e-6 mean |exact|

for the trunk behind the RRDBs and, each with its own q, for x1 .. x4 of the last dense block (growth_out).  The state is
rrdb_block_ref.lively_state: conv5 unshrunk, so the dense blocks reach the trunk at 0.2 and not at 0.004 as in the whole-network tests.
The host test (tests/test_rrdb_block_ref_host.py) shows on the CPU that these bounds reject a missing LeakyReLU on conv2, a pair that
contracts one plane too few, x3 in x4's plane, rdb3's first residual from the RRDB input and s1 = 0.2 at rdb3.  A pair whose second conv
reads x_a unrounded is closer to the exact block, not further: what rejects it is that the growth planes hold the same bits whether the
pairs are fused or not (test_growth_planes_bit_identical_across_pair_forms).

The trunk's lo planes are pinned by the trunk-only state (every conv5 zero): the RRDB is elementwise there, and the engine is held to
rrdb_block_ref.trunk_only_run's model of the path's representation within its derived per-element bound - a few fp32 roundings, where
a dropped or misscaled lo plane is 50 to 1000 times that.

One engine per (dtype, environment, state), num_block 2, scale 4.  FW_RRDB_* are read at create and set per engine here; FW_PAIR_SLIDE
is read per launch.  Which kernel forms the RRDBs dispatch to is asserted on the handle (fw_rrdbnet_block_paths); that they ran is on
record: profiles/rrdb_block_kernel_stats.csv is the kernel trace of this file on an MI355X."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import guarded
import rrdb_block_ref as R
from framewright_amd import _lib
from framewright_amd.realesrgan import RRDBNetEngine
from ifnet_glue_ref import from_bits

pytestmark = pytest.mark.gpu

SWITCHES = ("FW_RRDB_FUSE_PAIRS", "FW_RRDB_FUSE_MASK", "FW_RRDB_SPLIT_TRUNK", "FW_RRDB_LO", "FW_RRDB_C5_WINO", "FW_RRDB_ABL_ALIAS", "FW_RRDB_ABL_RDB3",
            "FW_RRDB_GRAPH", "FW_PAIR_SLIDE", "FW_PAIR_SLIDE32")
CASES = [(pid, env, slide, dtype, model) for pid, env, slide, dtypes, model in R.ENGINE_PATHS for dtype in dtypes]
IDS = [f"{c[0]}-{c[3]}" for c in CASES]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _flags(env, dtype, model):
    fuse = env.get("FW_RRDB_FUSE_PAIRS", "1") != "0"
    mask = int(env.get("FW_RRDB_FUSE_MASK", "3"))
    split = env.get("FW_RRDB_SPLIT_TRUNK", "1") != "0"
    m = R.model_path(model, dtype)
    return ((_lib.FW_RRDB_PATH_PAIR12 if fuse and mask & 1 else 0) | (_lib.FW_RRDB_PATH_PAIR34 if fuse and mask & 2 else 0) |
            (_lib.FW_RRDB_PATH_SPLIT_TRUNK if split else 0) | (_lib.FW_RRDB_PATH_RRDB_LO if split and env.get("FW_RRDB_LO", "1") != "0" else 0) |
            (_lib.FW_RRDB_PATH_C5_WINO_RDB12 if m.wino12 else 0) | (_lib.FW_RRDB_PATH_C5_WINO_RDB3 if m.wino3 else 0))


@functools.lru_cache(maxsize=None)
def _state(trunk_only=False):
    return R.trunk_only_state() if trunk_only else R.lively_state()


@functools.lru_cache(maxsize=None)
def _exact(first, count, H, W):
    x = R.lively_trunk(H, W, 100 * first + count)
    return x, R.run_exact(x, _state(), first, count)


@functools.lru_cache(maxsize=None)
def _rounded(first, count, H, W, rt, model):
    return R.run_rounded(_exact(first, count, H, W)[0], _state(), first, count, rt, model)


_ENGINES = {}


def _set_env(monkeypatch, env, slide=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if slide is not None:
        monkeypatch.setenv("FW_PAIR_SLIDE", slide)


def _engine(monkeypatch, dtype, env, trunk_only=False):
    """One handle per (dtype, environment at create, state); create reads the environment."""
    k = (dtype, tuple(sorted(env.items())), trunk_only)
    if k not in _ENGINES:
        _set_env(monkeypatch, env)
        eng = RRDBNetEngine(R.NUM_BLOCK, R.SCALE, dtype)
        eng.load_state_dict(_state(trunk_only))
        _ENGINES[k] = eng
    return _ENGINES[k]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


class _Buf:
    """A device tensor of `shape` between two guards (tests/guarded.py): float32, or 16-bit operand-typed."""

    def __init__(self, shape, kind="f32"):
        self.shape, self.kind = tuple(shape), kind
        self.g = guarded.Guarded(int(np.prod(shape)), kind)
        self.t = self.g.body().view(torch.float32 if kind == "f32" else torch.int16).view(*self.shape)

    def load(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        return self.t

    def take(self):
        """The body (float32 values / uint16 bits); asserts that both guards are untouched."""
        a = self.g.take()
        return (guarded.f32(a) if self.kind == "f32" else a).reshape(self.shape)


def _run(eng, x, first, count, growth=True):
    """-> (trunk_out float32 (H, W, 64), growth bits uint16 (4, H, W, 32) or None); guards checked, the input unchanged, every output written."""
    H, W, _ = x.shape
    src, dst = _Buf((H, W, 64)), _Buf((H, W, 64))
    gb = _Buf((4, H, W, 32), "u16") if growth else None
    eng.run_rrdbs(src.load(x), first, count, dst.t, gb.t if gb else None)
    torch.cuda.synchronize()
    assert np.array_equal(src.take().view(np.uint32), x.view(np.uint32)), "trunk_in_f32 was written"
    out = dst.take()
    assert not (out.view(np.uint32) == guarded.SENT["f32"]).any(), "trunk_out_f32 keeps sentinel values"
    bits = gb.take() if gb else None
    return out, bits


def _ratio(e, q):
    return e / q if q else (0.0 if e == 0 else math.inf)


RUN_IDS = [f"blocks{f}+{c}" for f, c in R.RUNS]


@pytest.mark.parametrize("run", R.RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("pid,env,slide,dtype,model", CASES, ids=IDS)
def test_rrdbs_against_float64(hip_lib, monkeypatch, pid, env, slide, dtype, model, run):
    """Measured on an MI355X: DESIGN.md (What pins the RRDB trunk) holds the largest error / q per path and type."""
    eng = _engine(monkeypatch, dtype, env)
    _set_env(monkeypatch, env, slide)
    assert eng.block_paths() == _flags(env, dtype, model), f"dispatch flags {eng.block_paths()}, expected {_flags(env, dtype, model)}"
    first, count = run
    m = R.model_path(model, dtype)
    failures = []
    for H, W in R.SHAPES:
        x, (exact, gexact) = _exact(first, count, H, W)
        rounded, grounded = _rounded(first, count, H, W, dtype, m)
        out, bits = _run(eng, x, first, count)
        got = [out.astype(np.float64)] + [from_bits(bits[i], dtype).reshape(H, W, 32) for i in range(4)]
        line = []
        for name, g, e, r in zip(("trunk", "x1", "x2", "x3", "x4"), got, [exact] + gexact, [rounded] + grounded):
            assert np.isfinite(g).all(), (H, W, name)
            err, q, lim, merr, mlim = R.bounds(g, e, r)
            line.append(f"{name} error {err:.3e}, q {q:.3e}, error / q {_ratio(err, q):.3f} (mean error / bound {merr / mlim:.3f})")
            if not (err <= lim and merr <= mlim):
                failures.append((H, W, name, float(err), float(lim), float(merr), float(mlim)))
        print(f"{pid} {dtype} blocks {first}+{count} {H}x{W}: " + ", ".join(line))
    assert not failures, failures


@pytest.mark.parametrize("run", R.RUNS, ids=RUN_IDS)
def test_growth_planes_bit_identical_across_pair_forms(hip_lib, monkeypatch, run):
    """The ring kernel, the two window kernels, one pair fused and the other not, and one conv per launch: the same x1 .. x4 and the same
    trunk, bit for bit (f16, the default trunk) - tests/test_conv_pair_gpu.py::test_conv_pair_three_kernels_bit_identical at the level of
    the engine's wiring, and extended to the single launches, whose second conv can only read the typed x_a."""
    first, count = run
    forms = [({}, "0"), ({}, "1"), ({}, "2"), ({"FW_RRDB_FUSE_PAIRS": "0"}, None), ({"FW_RRDB_FUSE_MASK": "1"}, None), ({"FW_RRDB_FUSE_MASK": "2"}, None)]
    for H, W in R.SHAPES:
        x = _exact(first, count, H, W)[0]
        ref = None
        for env, slide in forms:
            eng = _engine(monkeypatch, "f16", env)
            _set_env(monkeypatch, env, slide)
            out, bits = _run(eng, x, first, count)
            if ref is None:
                ref = (out, bits)
            else:
                assert np.array_equal(bits, ref[1]), (H, W, env, slide, "growth planes differ", int((bits != ref[1]).sum()))
                assert np.array_equal(out.view(np.uint32), ref[0].view(np.uint32)), (H, W, env, slide, "trunk differs")


# ---- the trunk-only state: every conv5 zero, the RRDB elementwise ----------------------------------------------------------------------
TRUNK_MODELS = sorted({(dtype, model.trunk) for _, _, _, dtype, model in CASES})


def _trunk_shapes():
    cus = _cus()
    # many tiles; and more 16 x 32 conv tiles than CUs in the fewest pixels: one tile column 8 wide, CUs + 1 tile rows - a persistent
    # workgroup takes a second tile while rdb3 updates the RRDB input in place
    return R.SHAPES + [(333, 517), (16 * (cus + 1), 8)]


@pytest.mark.parametrize("run", R.RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("dtype,trunk", TRUNK_MODELS, ids=[f"{d}-{t}" for d, t in TRUNK_MODELS])
def test_trunk_only_against_elementwise_model(hip_lib, monkeypatch, dtype, trunk, run):
    """Every engine path whose trunk representation is `trunk`, on the state with every conv5 zero: |engine - model| within the derived
    per-element bound of rrdb_block_ref.trunk_only_run.  The growth buffer is left out here (it is optional)."""
    first, count = run
    paths = [c for c in CASES if c[3] == dtype and c[4].trunk == trunk]
    assert paths
    failures = []
    for H, W in _trunk_shapes():
        x = R.lively_trunk(H, W, 50 + 10 * first + count)
        want, bound = R.trunk_only_run(x, count, dtype, R.Path(trunk, False, False))
        for pid, env, slide, _, model in paths:
            eng = _engine(monkeypatch, dtype, env, trunk_only=True)
            _set_env(monkeypatch, env, slide)
            assert eng.block_paths() == _flags(env, dtype, model)
            out, _ = _run(eng, x, first, count, growth=False)
            err = np.abs(out.astype(np.float64) - want)
            worst = float((err / np.maximum(bound, 1e-300)).max()) if (err > 0).any() else 0.0
            print(f"{pid} {dtype} blocks {first}+{count} {H}x{W}: max error / bound {worst:.3f}, max error {err.max():.3e}")
            if not (err <= bound).all():
                failures.append((pid, H, W, worst, int((err > bound).sum())))
    assert not failures, failures


def test_run_rrdbs_refuses_what_it_cannot_run(hip_lib, monkeypatch):
    _set_env(monkeypatch, {})
    eng = RRDBNetEngine(R.NUM_BLOCK, R.SCALE, "f16")
    src, dst = _Buf((4, 4, 64)), _Buf((4, 4, 64))
    src.load(np.zeros((4, 4, 64), np.float32))
    run = lambda first, count, h=4, w=4: eng._lib.fw_rrdbnet_run_rrdbs(eng._h, first, count, src.g.ptr(), h, w, dst.g.ptr(), None, None)
    flags = C.c_int(0)
    assert run(0, 1) == _lib.FW_ERR_INVALID and b"missing" in eng._lib.fw_last_error()          # no weights yet: not finalised
    assert eng._lib.fw_rrdbnet_block_paths(eng._h, C.byref(flags)) == _lib.FW_ERR_INVALID
    eng.load_state_dict(_state())
    for first, count in ((0, 3), (1, 2), (2, 1), (-1, 1), (0, 0), (0, -1), (1, 2 ** 31 - 1)):
        assert run(first, count) == _lib.FW_ERR_INVALID, (first, count)
        assert b"blocks" in eng._lib.fw_last_error()
    for h, w in ((0, 4), (4, 0), (-1, 4), (16385, 4)):
        assert run(0, 1, h, w) == _lib.FW_ERR_INVALID, (h, w)
        assert b"size" in eng._lib.fw_last_error()
    assert eng._lib.fw_rrdbnet_run_rrdbs(eng._h, 0, 1, None, 4, 4, dst.g.ptr(), None, None) == _lib.FW_ERR_INVALID
    assert eng._lib.fw_rrdbnet_run_rrdbs(eng._h, 0, 1, src.g.ptr(), 4, 4, None, None, None) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize()
    assert guarded.untouched(dst.take().view(np.uint32), "f32"), "a refused call launched something"
    with pytest.raises(ValueError):
        eng.run_rrdbs(torch.zeros((4, 4, 32), dtype=torch.float32, device="cuda"), 0, 1)
    assert run(0, 2) == _lib.FW_OK
    eng.close()
