"""Host-only checks of oracle/winograd_ref.py, the float64 references that tests/test_conv_split_wino_gpu.py pins the conv5 kernels
to: the Winograd emulation is the contract when its roundings are taken out, the bounds accept a faithful kernel, and the same
bounds reject deliberately wrong variants of it (frequencies swapped, bias in the wrong frequency, U in bf16, the sign of the
frequency-3 identity flipped, the lo pass dropped) on the test's own inputs.  No GPU; the packer check calls the host-side packer
of the built library."""
import ctypes as C

import numpy as np
import pytest

from framewright_amd import _lib
from oracle import winograd_ref as wr


def _inputs(kind, H=9, W=13, chunks=6, n_id=4, wscale=1.0, seed=0):
    rng = np.random.default_rng(seed)
    shp = (H, W, 32 * chunks)
    if kind == "uniform":
        x = rng.uniform(-1, 1, shp)
    elif kind == "heavy":
        x = np.clip(rng.standard_normal(shp) * np.exp(2 * rng.standard_normal(shp)), -3e3, 3e3)
    else:   # "dc": cancellation in d0 - d2 and d1 - d3
        x = 512 + rng.standard_normal(shp)
    bound = 1 / np.sqrt(9 * 32 * chunks)
    w = (rng.uniform(-bound, bound, (64, 32 * chunks, 3, 3)) * wscale).astype(np.float32)
    b = rng.uniform(-1, 1, 64).astype(np.float32)
    planes = [wr.f16(rng.standard_normal((H, W, 32))) for _ in range(n_id)]
    return wr.f16(x), w, b, planes


CASE = dict(s1=0.04, in_id_scale=5.0, id_scale=(25.0, 25.0, 5.0, 5.0))


@pytest.mark.parametrize("kind", ["uniform", "heavy", "dc"])
def test_exact_emulation_is_the_contract(kind):
    x, w, b, planes = _inputs(kind)
    yc, A = wr.split_contract(x, w, b, planes=planes, **CASE)
    ye, Aw, _ = wr.winograd_emulation(x, w, b, planes=planes, exact=True, **CASE)
    assert np.abs(ye - yc).max() <= 1e-12 * A.max()
    assert (np.abs(ye - yc) <= 1e-12 * A).all()


def _verdict(hi, lo, x, w, b, planes):
    """The checks the GPU test applies to the Winograd kernel: against the faithful emulation (tight) and the contract (a priori)."""
    ye, Aw, apr = wr.winograd_emulation(x, w, b, planes=planes, **CASE)
    yc, A = wr.split_contract(x, w, b, planes=planes, **CASE)
    acc = wr.ACC_EPS_WINO * np.maximum(A, Aw)
    tight = wr.check_hi_lo(hi, lo, ye, acc)
    got = hi.astype(np.float64) + (lo.astype(np.float64) if lo is not None else 0)
    loose = wr.check_apriori(got, yc, apr, acc + np.spacing(np.abs(lo if lo is not None else hi)).astype(np.float64) / 2)
    return tight, loose


@pytest.mark.parametrize("kind", ["uniform", "heavy", "dc"])
def test_bounds_accept_a_faithful_kernel(kind):
    x, w, b, planes = _inputs(kind, seed=1)
    ye, _, _ = wr.winograd_emulation(x, w, b, planes=planes, **CASE)
    hi, lo = wr.split_hi_lo(ye)
    tight, loose = _verdict(hi, lo, x, w, b, planes)
    assert tight["ok"] and loose["ok"], (tight, loose)
    # and the direct kernel's stand-in against the contract
    yc, A = wr.split_contract(x, w, b, planes=planes, **CASE)
    hi, lo = wr.split_hi_lo(yc)
    assert wr.check_hi_lo(hi, lo, yc, wr.ACC_EPS_DIRECT * A)["ok"]


@pytest.mark.parametrize("kind", ["uniform", "heavy", "dc"])
@pytest.mark.parametrize("variant", ["swap12", "bias_m0", "u_bf16", "flip3", "no_lo"])
def test_bounds_reject_a_wrong_kernel(kind, variant):
    x, w, b, planes = _inputs(kind, seed=2)
    ye, _, _ = wr.winograd_emulation(x, w, b, planes=planes, variant=None if variant == "no_lo" else variant, **CASE)
    hi, lo = wr.split_hi_lo(ye)
    if variant == "no_lo":
        lo = np.zeros_like(lo)
    tight, loose = _verdict(hi, lo, x, w, b, planes)
    print(f"{kind:8s} {variant:8s}: emulation ratio {tight['ratio']:.3g}, a-priori ratio {loose['ratio']:.3g}")
    assert not (tight["ok"] and loose["ok"])
    assert tight["ratio"] > 4     # rejected with margin, not by a hair


def test_bounds_reject_frequency_swap_with_zero_sum_taps():
    """Taps whose three values in a row sum to ~0: U1 and U2 nearly cancel, the case where a relative bound on |U_f||V_f| would
    go blind; the transform-of-absolutes bound still accepts the faithful kernel, the tight one still rejects the swap."""
    x, w, b, planes = _inputs("uniform", seed=3)
    w[..., 2] = -(w[..., 0] + w[..., 1])
    ye, _, _ = wr.winograd_emulation(x, w, b, planes=planes, **CASE)
    tight, loose = _verdict(*wr.split_hi_lo(ye), x, w, b, planes)
    assert tight["ok"] and loose["ok"], (tight, loose)
    ye, _, _ = wr.winograd_emulation(x, w, b, planes=planes, variant="swap12", **CASE)
    assert not _verdict(*wr.split_hi_lo(ye), x, w, b, planes)[0]["ok"]


def test_v_domain_of_f16():
    """The documented f16 domain of V (conv3x3_wino.hip header): finite up to |x| = 32752, inf one f16 step beyond."""
    lim = np.float16(wr.V_F16_DOMAIN)
    assert float(lim) == wr.V_F16_DOMAIN
    with np.errstate(over="ignore"):
        assert np.isfinite(lim + lim) and np.isfinite(-lim - lim)
        nxt = np.nextafter(lim, np.float16(np.inf))
        assert float(nxt) == 32768.0 and np.isinf(lim + nxt) and np.isinf(-lim - nxt)


@pytest.mark.parametrize("cout,cin,chunks", [(64, 192, 6), (64, 64, 2), (48, 70, 3)])
def test_wino_packer_is_the_emulations_u(hip_lib, cout, cin, chunks):
    """fw_pack_conv3x3_wino stores the emulation's U in fragment order [chunk][dy][f][16-channel tile][lane][e]."""
    rng = np.random.default_rng(cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    w[0, 0, 0] = [1e-6, -2e-6, 3e-7]                      # f16 subnormals
    n = hip_lib.fw_pack_conv3x3_wino(_lib.FW_DTYPE_F16, None, cout, cin, chunks, None)
    assert n == chunks * 3 * 4 * 4 * 64 * 8
    dst = np.zeros(n, np.uint16)
    assert hip_lib.fw_pack_conv3x3_wino(_lib.FW_DTYPE_F16, C.c_void_p(w.ctypes.data), cout, cin, chunks, C.c_void_p(dst.ctypes.data)) == n
    U = np.zeros((3, 4, 64, 32 * chunks), np.float16)
    U[:, :, :cout, :cin] = wr.wino_weights(w)
    lane = np.arange(64)
    want = np.empty((chunks, 3, 4, 4, 64, 8), np.float16)
    for c in range(chunks):
        for ct in range(4):
            for e in range(8):
                want[c, :, :, ct, :, e] = U[:, :, 16 * ct + (lane & 15), 32 * c + 8 * (lane >> 4) + e]
    np.testing.assert_array_equal(dst, want.reshape(-1).view(np.uint16))
    assert hip_lib.fw_pack_conv3x3_wino(_lib.FW_DTYPE_BF16, None, cout, cin, chunks, None) == 0    # f16 only
    assert hip_lib.fw_pack_conv3x3_wino(_lib.FW_DTYPE_F16, None, 65, cin, chunks, None) == 0
    assert hip_lib.fw_pack_conv3x3_wino(_lib.FW_DTYPE_F16, None, cout, 32 * chunks + 1, chunks, None) == 0


def test_winograd_launcher_checks_reject_each_field(hip_lib):
    """The Winograd launchers reject every ConvParams field their kernels would ignore (conv3x3_wino.hip, check_conv3x3_wino), one
    field at a time on an otherwise valid problem; the valid problems themselves pass."""
    names = ["post_act", "chan_scale", "res1", "res2", "out_f32", "n_groups", "act (split)", "in_id_scale", "id_scale",
             "out_f32 (store)", "n_groups (store)", "chan_scale (store)", "post_act (store)", "res1 (store)", "PReLU (store)",
             "out_lo (store)"]
    codes = (C.c_int * 32)()
    n = hip_lib.fw_conv3x3_wino_check_fields(codes, 32)
    assert n == len(names), (n, hip_lib.fw_last_error())
    assert all(codes[i] == _lib.FW_ERR_INVALID for i in range(n)), {names[i]: codes[i] for i in range(n)}
    assert b"conv3x3_wino" in hip_lib.fw_last_error()
