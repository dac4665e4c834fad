"""tests/rrdb_block_ref.py on the CPU: the float64 RRDB against oracle/rrdbnet_ref.py, the properties of its inputs, and the teeth of
the bounds that tests/test_rrdb_blocks_gpu.py applies to the engine - each defect of DEFECTS / TRUNK_DEFECTS, built into the rounded
model, leaves the bound meant for it at every shape, run and (dtype, path) of the GPU test.

"xa_unrounded" (the second conv of a fused pair reading x_a as fp32) is the one defect that a bound on the ERROR cannot see: it rounds
less, so it sits closer to the exact block than the model does (error / limit 0.5, below).  What rejects it is the equality the GPU
test asserts on the growth planes: with the pairs fused they hold the same bits as with one conv per launch (FW_RRDB_FUSE_PAIRS=0),
where conv2 / conv4 can only read the typed x_a from the concat buffer."""
import functools

import numpy as np
import pytest
import torch

import rrdb_block_ref as R
from ifnet_glue_ref import to_bits
from oracle import rrdbnet_ref

CASES = [(H, W, first, count) for H, W in R.SHAPES for first, count in R.RUNS]
MODELS = R.model_paths()
SPLIT_ONLY = ("rdb3_s1",)                  # the fp32 trunk has no s1 = 0.04: its rdb3 scales by s2


def _mid(m):
    rt, p = m
    return f"{rt}-{p.trunk}" + ("-wino12" if p.wino12 else "") + ("-wino3" if p.wino3 else "")


@functools.lru_cache(maxsize=None)
def _state():
    return R.lively_state()


@functools.lru_cache(maxsize=None)
def _exact(H, W, first, count):
    x = R.lively_trunk(H, W, 100 * first + count)
    return x, R.run_exact(x, _state(), first, count)


@functools.lru_cache(maxsize=None)
def _rounded(H, W, first, count, rt, path, defect=None):
    return R.run_rounded(_exact(H, W, first, count)[0], _state(), first, count, rt, path, defect)


def test_exact_block_is_the_oracles():
    sd = _state()
    tsd = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    for H, W in ((5, 7), (17, 33)):
        x = R.lively_trunk(H, W, 1)
        xt = torch.from_numpy(x.astype(np.float64)).permute(2, 0, 1)[None]
        for b in range(R.NUM_BLOCK):
            want = rrdbnet_ref.rrdb_forward(tsd, f"body.{b}", xt)[0].permute(1, 2, 0).numpy()
            got, growth = R.rrdb(x, R.block_weights(sd, b))
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (H, W, b)
            assert len(growth) == 4 and all(g.shape == (H, W, 32) for g in growth)


def test_lively_state_takes_both_lrelu_branches_on_every_growth_plane():
    for H, W, first, count in CASES:
        _, (_, growth) = _exact(H, W, first, count)
        for i, g in enumerate(growth):
            share = float((g < 0).mean())
            assert 0.2 <= share <= 0.8, (H, W, first, count, f"x{i + 1}", share)


def test_lively_trunk_has_both_signs_a_few_binades_and_lo_parts():
    for H, W in R.SHAPES:
        x = R.lively_trunk(H, W, 0)
        assert x.dtype == np.float32 and x.shape == (H, W, 64) and (x > 0).any() and (x < 0).any()
        assert np.abs(x).max() / np.abs(x).min() >= 8
        for rt in ("f16", "bf16"):
            t = R.lay_in(x, rt, R.Path("lo_rrdb", False, False))
            for plane in range(2):
                assert np.abs(t.lo[..., 32 * plane:32 * plane + 32]).max() > 0, (H, W, rt, plane)
            assert np.array_equal(t.hi + t.lo, R._f32(t.hi + t.lo)), "hi + lo is an fp32 number"
    # no lo is zero, and all but the few values beside a power of two (where the spacing changes) are a quarter of a spacing or more
    x = R.lively_trunk(17, 33, 0)
    for rt in ("f16", "bf16"):
        t = R.lay_in(x, rt, R.Path("lo_rrdb", False, False))
        big = np.abs(t.lo) >= 0.24 * R.typed_ulp(t.hi, rt)
        assert (t.lo != 0).all() and big.mean() >= 0.99, (rt, float(big.mean()))


def test_states():
    sd, t0 = _state(), R.trunk_only_state()
    assert sorted(sd) == sorted(t0)
    for k in sd:
        if ".conv5." in k:
            assert not t0[k].any() and sd[k].any()
        else:
            assert np.array_equal(sd[k], t0[k])


def _yardstick_rejects(H, W, first, count, rt, path, defect):
    """Whether one of the checks of test_rrdb_blocks_gpu.test_rrdbs_against_float64 fails for the defective block: max and mean of the
    trunk, max and mean of each growth plane, each against its own q."""
    _, (exact, gexact) = _exact(H, W, first, count)
    rounded, grounded = _rounded(H, W, first, count, rt, path)
    got, ggot = _rounded(H, W, first, count, rt, path, defect)
    worst = 0.0
    for g, e, r in [(got, exact, rounded)] + list(zip(ggot, gexact, grounded)):
        err, _, lim, merr, mlim = R.bounds(g, e, r)
        worst = max(worst, err / lim, merr / mlim)
    return worst


@pytest.mark.parametrize("model", MODELS, ids=[_mid(m) for m in MODELS])
def test_the_rounded_model_itself_sits_at_half_the_yardstick(model):
    rt, path = model
    for H, W, first, count in CASES:
        assert _yardstick_rejects(H, W, first, count, rt, path, None) <= 0.5 + 1e-9


@pytest.mark.parametrize("defect", [d for d in R.DEFECTS if d != "xa_unrounded"])
@pytest.mark.parametrize("model", MODELS, ids=[_mid(m) for m in MODELS])
def test_yardstick_rejects_each_defect(model, defect):
    rt, path = model
    if defect in SPLIT_ONLY and path.trunk == "f32":
        return
    for H, W, first, count in CASES:
        worst = _yardstick_rejects(H, W, first, count, rt, path, defect)
        assert worst > 1.0, (H, W, first, count, worst)


LO_ALL = [m for m in MODELS if m[1].trunk == "lo_all"]


@pytest.mark.parametrize("model", LO_ALL, ids=[_mid(m) for m in LO_ALL])
def test_yardstick_rejects_r_from_the_current_buffer(model):
    rt, path = model
    for H, W, first, count in CASES:
        assert _yardstick_rejects(H, W, first, count, rt, path, "r_from_cur") > 1.0, (H, W, first, count)


@pytest.mark.parametrize("model", MODELS, ids=[_mid(m) for m in MODELS])
def test_unrounded_x_a_is_invisible_to_an_error_bound_and_visible_in_the_bits(model):
    """The yardstick cannot reject it (it is closer to the exact block); the growth planes' bits can: x2 or x4 of the last dense block
    differ from those of the block that reads the typed x_a, at every shape and run."""
    rt, path = model
    for H, W, first, count in CASES:
        assert _yardstick_rejects(H, W, first, count, rt, path, "xa_unrounded") < 1.0
        _, good = _rounded(H, W, first, count, rt, path)
        _, bad = _rounded(H, W, first, count, rt, path, "xa_unrounded")
        assert any(not np.array_equal(to_bits(good[i], rt), to_bits(bad[i], rt)) for i in range(4)), (H, W, first, count)


# ---- the trunk-only state ------------------------------------------------------------------------------------------------------------
TRUNK_CASES = [(H, W, first, count) for H, W in R.SHAPES + [(64, 8)] for first, count in R.RUNS]
TRUNK_MODELS = sorted({(rt, p._replace(wino12=False, wino3=False)) for rt, p in MODELS})    # zero weights: the Winograd form is the same sum


def _applies(defect, path):
    if path.trunk == "f32":
        return False                                       # no lo planes, no chunk offsets: EPI_RESIDUAL reads res1 / res2
    if defect == "rdb1_lo_dropped":
        return path.trunk == "lo_all"                      # "with FW_RRDB_LO=0"
    if defect == "r_from_cur":
        # with lo planes behind every dense block the trunk-only state cannot see it: rdb1 and rdb2 are the identity there, so the current
        # buffer holds R itself, hi and lo.  The lively state sees it (test_yardstick_rejects_r_from_the_current_buffer)
        return path.trunk == "lo_rrdb"
    return True


@functools.lru_cache(maxsize=None)
def _trunk_only(H, W, count, rt, path, defect=None):
    return R.trunk_only_run(R.lively_trunk(H, W, 50 + count), count, rt, path, defect)


@pytest.mark.parametrize("model", TRUNK_MODELS, ids=[_mid(m) for m in TRUNK_MODELS])
def test_trunk_only_model_is_the_elementwise_rrdb(model):
    """y = 0.2 (0.2 * 0 + x_rdb) + R with x_rdb = R: 1.2 x per RRDB, to within the representation (half a spacing of T per typed-only
    hand-over, scaled by 0.2; 2^-22 / 2^-16 relative for hi + lo) - and the bound is small against it."""
    rt, path = model
    for H, W in R.SHAPES:
        x = R.lively_trunk(H, W, 51).astype(np.float64)
        y, bound = _trunk_only(H, W, 1, rt, path)
        rel = 2.0 ** (-11 if rt == "f16" else -8)
        assert np.abs(y - 1.2 * x).max() <= 0.5 * rel * np.abs(x).max()
        assert (bound <= (2.0 ** -19 if rt == "f16" else 2.0 ** -14) * np.abs(y)).all() and (bound >= 0).all()


@pytest.mark.parametrize("defect", R.TRUNK_DEFECTS)
@pytest.mark.parametrize("model", TRUNK_MODELS, ids=[_mid(m) for m in TRUNK_MODELS])
def test_trunk_only_bound_rejects_each_defect(model, defect):
    rt, path = model
    if not _applies(defect, path):
        return
    for H, W, first, count in TRUNK_CASES:
        y, bound = _trunk_only(H, W, count, rt, path)
        bad, _ = _trunk_only(H, W, count, rt, path, defect)
        ratio = np.abs(bad - y) / np.maximum(bound, 1e-300)
        assert (np.abs(bad - y) > bound).any(), (H, W, count)
        if defect in R.DROPPED_LO:
            assert ratio.max() >= 50, (H, W, count, float(ratio.max()))
