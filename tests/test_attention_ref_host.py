"""Host side of tests/attention_ref.py: its float64 restatements are pinned to torch in float64 (oracle.rrdbnet_ref.attention_forward,
project_out(attn @ v) as oracle/restormer_ref.py writes it, torch.softmax, torch's own f16 / bf16 casts), and every listed defect,
computed exactly, leaves the bound of the GPU test by at least 100x on the inputs that test uses.  The two largest P @ v cases
generate P on the device there; here the same generator runs on the CPU for a few rows (other noise, the same planted structure)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as R
import test_attention_ops_gpu as G          # its input generators are plain numpy / device-agnostic torch
from oracle import rrdbnet_ref


def _worst(wrong, ref, allow):
    return float((np.abs(wrong - ref) / allow).max())


def test_attention_block_is_attention_forward():
    x, w, asd, pre = G.block_inputs(9, 7)
    sd = {k: torch.from_numpy(v).double() for k, v in asd.items()}
    sd[pre + ".gamma"] = torch.from_numpy(w["gamma"]).double().view(1, 64, 1, 1)
    xt = torch.from_numpy(x).double().T.reshape(1, 64, 9, 7)
    want = rrdbnet_ref.attention_forward(sd, pre, xt)[0].reshape(64, 63).T.numpy()
    got = R.attention_block(x, w)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    for dtype in ("f16", "bf16"):
        q = np.abs(R.attention_block(x, w, dtype) - got).max()
        u = 2.0 ** (-11 if dtype == "f16" else -8)
        assert 0.05 * u < q < 50 * u * np.abs(got).max(), q       # the rounded model differs by rounding-sized amounts


def test_softmax_rows_is_torch_softmax():
    for d in (8, 5):
        _, _, q, k = R.softmax_inputs(97, d, "sharp", "f16", 40)
        want = torch.softmax(torch.from_numpy(q[:, :d]) @ torch.from_numpy(k[:, :d]).T, -1).numpy()
        got, bound, lo = R.softmax_rows(q, k, d)
        assert np.abs(got - want).max() <= 1e-14 and -20 <= lo <= 0
        rows = np.array([0, 5, 96])
        assert np.array_equal(R.softmax_rows(q, k, d, rows)[0], got[rows])
        assert (bound > 0).all() and (bound < 1e-4 * got).all()


def test_proj_fold_is_project_out_of_attn_times_v():
    for heads, ch in ((1, 48), (2, 48), (8, 48), (1, 96)):
        attn, wp = G.proj_inputs(heads, ch)
        dim, hw = heads * ch, 11
        v = torch.from_numpy(np.random.default_rng(heads).standard_normal((1, heads, ch, hw)))
        out = (torch.from_numpy(attn).double()[None] @ v).reshape(1, dim, hw, 1)                 # oracle/restormer_ref.py: (attn @ v).reshape(b, c, h, w)
        want = F.conv2d(out, torch.from_numpy(wp).double()[:, :, None, None])[0, :, :, 0].numpy()    # project_out
        fold, bound = R.proj_fold(attn, wp)
        got = fold @ v.reshape(dim, hw).numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert (bound >= 0).all() and bound.max() < 1e-4


def test_fragment_order_is_the_packers():
    """unpack_pointwise / pack_pointwise against the map csrc/nn_ops.hip documents for pack_pointwise_weights, element by element."""
    ct, k_pad = 2, 96
    m = np.arange(64 * k_pad, dtype=np.uint16).reshape(64, k_pad)
    want = np.empty((k_pad // 32, 2, ct, 64, 8), np.uint16)
    lane = np.arange(64)
    for c in range(k_pad // 32):
        for ks in range(2):
            for t in range(ct):
                for j in range(8):
                    want[c, ks, t, :, j] = m[32 * t + (lane & 31), 32 * c + 16 * ks + 8 * (lane >> 5) + j]
    assert np.array_equal(R.pack_pointwise(m, ct, k_pad), want.reshape(-1))
    assert np.array_equal(R.unpack_pointwise(want.reshape(-1), ct, k_pad), m)


@pytest.mark.parametrize("dtype,tdt", [("f16", torch.float16), ("bf16", torch.bfloat16)])
def test_casts_at_the_edges_are_torchs(dtype, tdt):
    v = R.cast_edge_values(dtype)
    with np.errstate(over="ignore"):
        got = R.to_bits(v, dtype)
    want = torch.from_numpy(v).to(tdt).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert len(set(got.tolist())) > 12
    x = np.arange(2 * 64, dtype=np.float32).reshape(2, 64)
    assert np.array_equal(R.from_bits(R.f32_to_planar(x, dtype), dtype).reshape(2, 2, 32)[1, 0], np.arange(32, 64))


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", [8, 5])
@pytest.mark.parametrize("M", G.SOFTMAX_M)
def test_softmax_bound_rejects_defects(dtype, d, M):
    for kind in ("engine", "sharp"):
        for stride, extra in G.softmax_variants(M):
            ldp = R.pad32(M) + extra
            _, _, q, k = R.softmax_inputs(M, d, kind, dtype, stride)
            rows = R.softmax_sample_rows(M) if M > 2000 else np.arange(M)
            ref, bound, lo = R.softmax_rows(q, k, d, rows)
            assert -20.0 <= lo <= 0.0, (kind, lo)
            allow = R.typed_allowance(ref, bound, dtype)
            if ldp > M:
                worst = _worst(R.softmax_rows(q, k, d, rows, ldp, "softmax_pad")[0], ref, allow)
                print(f"softmax M {M} d {d} {dtype} {kind} ldp {ldp}: padded columns in the softmax: {worst:.0f} x the bound")
                assert worst >= 100
            if 1 < M <= 2000 and stride == 32 and extra == 0:
                worst = _worst(R.softmax_rows(q, k, d, rows, ldp, "p_transposed")[0], ref, allow)
                print(f"softmax M {M} d {d} {dtype} {kind}: P transposed: {worst:.0f} x the bound")
                assert worst >= 100
            if d == 5 and M > 1:             # the channels behind d are live values: using them is far outside the bound as well
                assert _worst(R.softmax_rows(q, k, 8, rows)[0], ref, allow) >= 100


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("M,K", G.PV_CASES)
def test_pv_bound_rejects_defects(dtype, M, K):
    nrows = None if M <= 2000 else 48
    P, v = G.pv_inputs(M, K, dtype, "cpu", nrows)
    a = P.double().numpy()
    wt = np.zeros((64, K))
    wt[:, :M] = v.double().numpy().T
    assert (a[:, M:] == 0).all() and np.abs(a[:, [0, M - 1]]).min() >= 4 and np.abs(wt[:, [0, M - 1]]).min() >= 6
    n_mfma = R.pointwise_mfmas(M, K, False)
    assert n_mfma == (K // 16 if M > 16384 else 16 * -(-K // 256))
    for ldf in (64, 72):
        res, cs = G.pv_epilogue(M, ldf, nrows)
        assert len(set(cs.tolist())) == 64 and cs.min() < 0 and cs.max() > 1 and (cs == 0).any()
        ref, bound, _ = R.pointwise(a, wt, None, n_mfma, res[:, :64], cs)
        for defect in R.DEFECTS_PV:
            worst = _worst(R.pointwise(a, wt, None, n_mfma, res[:, :64], cs, defect)[0], ref, bound)
            print(f"P @ v M {M} K {K} {dtype} ldf {ldf} {defect}: {worst:.0f} x the bound")
            assert worst >= 100, defect
        worst = _worst(R.pointwise(a, wt, None, n_mfma, res[:, :64], np.zeros(64))[0], ref, bound)
        assert worst >= 100                                       # liveness: the product matters at this bound


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_projection_bound_rejects_a_dropped_bias_and_swapped_halves(dtype):
    rng = np.random.default_rng(3)
    x, w = R.rnd(rng.standard_normal((33, 64)), dtype), R.rnd(rng.standard_normal((64, 64)) / 8, dtype)
    bias = rng.standard_normal(64).astype(np.float32)
    ref, bound, _ = R.pointwise(x, w, bias, 4)
    allow = R.typed_allowance(ref, bound, dtype)
    assert _worst(R.pointwise(x, w, bias, 4, defect="swap_halves")[0], ref, allow) >= 100
    assert _worst(R.pointwise(x, w, 0 * bias, 4)[0], ref, allow) >= 100
