"""The kernels behind AESRGAN's AttentionBlock and Restormer's folded project_out, each on its own through the C-ABI against the
float64 restatements and per-element bounds of tests/attention_ref.py (derivations there), in f16 and bf16: fw_attn_softmax_rows,
fw_pack_pointwise_transposed, fw_pointwise_nhwc as the chain calls it (fp32 operand; K = the padded pixel count with the residual
epilogue), fw_f32_to_planar, fw_copy_channels_f32, fw_attn_proj_pack, and the five calls of the block composed on one fp32 stream.
Every output buffer is pre-filled with a sentinel and guarded on both sides (tests/guarded.py): nothing outside the documented region
may change.  Large operands are generated on the device from a seeded generator; only the rows the reference needs come back."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from framewright_amd import _lib
import attention_ref as R
from guarded import GUARD, SENT, TDT, Guarded, dev, dtype_id, f32, ptr, stream, untouched

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]
NP = lambda a: C.c_void_p(a.ctypes.data)


def _host_pack(lib, dtype, w):
    """fw_pack_pointwise of w (cout, K) fp32 on the host -> uint16 fragments."""
    w = np.ascontiguousarray(w, np.float32)
    cout, K = w.shape
    n = lib.fw_pack_pointwise(dtype_id(dtype), None, cout, K, None)
    assert n == (K // 32) * 2 * ((cout + 31) // 32) * 64 * 8
    dst = np.zeros(n, np.uint16)
    assert lib.fw_pack_pointwise(dtype_id(dtype), NP(w), cout, K, NP(dst)) == n
    return dst


def _report(name, err, A, bound):
    ratio = float((err / np.maximum(2.0 ** -24 * A, 1e-300)).max())
    print(f"{name}: max |err| / (2^-24 A) = {ratio:.2f}, max |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


# ---- fw_attn_softmax_rows --------------------------------------------------------------------------------------------------------
SOFTMAX_M = [1, 31, 32, 33, 63, 65, 97, 1665, 8200]


def softmax_variants(M):
    """(q / k stride, columns of P behind the padded M): all four at the small sizes, the two extremes at 8200."""
    return [(32, 0), (40, 32)] if M > 2000 else [(32, 0), (32, 32), (40, 0), (40, 32)]


def _run_softmax(lib, dtype, qb, kb, M, d, stride, ldp):
    P = Guarded(M * ldp, "u16")
    q, k = dev(qb), dev(kb)
    _lib.check(lib.fw_attn_softmax_rows(dtype_id(dtype), ptr(q), stride, ptr(k), stride, M, d, P.ptr(), ldp, stream()))
    torch.cuda.synchronize()
    return P


def _check_softmax(P, dtype, qv, kv, M, d, ldp, name):
    body = P.body().view(M, ldp)
    assert bool((body[:, M:] == 0).all()), "columns [M, p_stride) must be exact zeros"
    g = P.t.view(torch.int16)
    sent = int(np.array([SENT["u16"]], np.uint16).view(np.int16)[0])
    assert bool((g[:GUARD] == sent).all()) and bool((g[GUARD + P.n:] == sent).all()), "a guard was written"
    rows = R.softmax_sample_rows(M) if M > 2000 else np.arange(M)
    got = R.from_bits(body[torch.from_numpy(rows).cuda(), :M].cpu().numpy().view(np.uint16), dtype).reshape(rows.size, M)
    ref, bound, lo = R.softmax_rows(qv, kv, d, rows)
    assert -20.0 <= lo <= 0.0, lo
    err = np.abs(got - ref)
    allow = R.typed_allowance(ref, bound, dtype)
    print(f"{name}: expf range [{lo:.2f}, 0], max |err| / allowance = {float((err / allow).max()):.3f}")
    assert np.isfinite(got).all() and (err <= allow).all(), (name, float((err / allow).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [8, 5])
@pytest.mark.parametrize("M", SOFTMAX_M)
def test_softmax_rows(hip_lib, dtype, d, M):
    for kind in ("engine", "sharp"):
        for stride, extra in softmax_variants(M):
            ldp = R.pad32(M) + extra
            qb, kb, qv, kv = R.softmax_inputs(M, d, kind, dtype, stride)
            P = _run_softmax(hip_lib, dtype, qb, kb, M, d, stride, ldp)
            _check_softmax(P, dtype, qv, kv, M, d, ldp, f"softmax M {M} d {d} {dtype} {kind} stride {stride} ldp {ldp}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [33, 1665])
def test_softmax_rows_ignores_unused_key_channels(hip_lib, dtype, M):
    """d = 5: channels [5, 8) of k hold NaN patterns.  Only d channels are used (include/framewright_hip.h), so they must not reach P."""
    qb, kb, qv, kv = R.softmax_inputs(M, 5, "engine", dtype, 32)
    kb = kb.copy()
    kb[:, 5:8] = 0x7E00 if dtype == "f16" else 0x7FC0
    ldp = R.pad32(M)
    P = _run_softmax(hip_lib, dtype, qb, kb, M, 5, 32, ldp)
    _check_softmax(P, dtype, qv, kv, M, 5, ldp, f"softmax NaN in unused k channels M {M} {dtype}")


# ---- fw_pack_pointwise_transposed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k_valid,cout,k_pad", [(1, 64, 32), (31, 64, 32), (33, 64, 64), (1665, 64, 1696), (97, 40, 128)])
@pytest.mark.parametrize("src_stride", [64, 72])
def test_pack_pointwise_transposed(hip_lib, dtype, k_valid, cout, k_pad, src_stride):
    rng = np.random.default_rng([k_valid, cout, src_stride])
    src = R.to_bits(rng.standard_normal((k_valid, src_stride)) * 4, dtype).reshape(k_valid, src_stride)
    w = np.zeros((cout, k_pad), np.float32)
    w[:, :k_valid] = R.from_bits(src, dtype).reshape(k_valid, src_stride)[:, :cout].T      # exact typed values: the host packer rounds nothing
    want = _host_pack(hip_lib, dtype, w)
    out = Guarded(want.size, "u16")
    dsrc = dev(src)
    _lib.check(hip_lib.fw_pack_pointwise_transposed(dtype_id(dtype), ptr(dsrc), src_stride, k_valid, cout, k_pad, out.ptr(), stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.take(), want)


# ---- fw_pointwise_nhwc, (a): the q / k / v projections (fp32 operand, K = 64) ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ct", [1, 2, 3, 5])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1665])
def test_pointwise_f32_operand(hip_lib, dtype, ct, M):
    rng = np.random.default_rng([M, ct])
    N, ldo = 32 * ct, 32 * ct + 8
    w = (rng.standard_normal((N, 64)) / 8).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    wp, dbias = dev(_host_pack(hip_lib, dtype, w)), dev(bias)
    for lda in (64, 72):
        x = np.full((M, lda), np.nan, np.float32)                 # columns [64, lda) are not the kernel's to read
        x[:, :64] = rng.standard_normal((M, 64)) * np.exp(rng.standard_normal((M, 1)))
        out, dx = Guarded(M * ldo, "u16"), dev(x)
        _lib.check(hip_lib.fw_pointwise_nhwc(dtype_id(dtype), ptr(dx), 1, lda, M, 64, ptr(wp), ptr(dbias), ct, out.ptr(), ldo,
                                             None, 0, None, None, stream()))
        torch.cuda.synchronize()
        got = out.take().reshape(M, ldo)
        assert untouched(got[:, N:], "u16"), "lanes behind 32 * cout_tiles were written"
        ref, bound, A = R.pointwise(R.rnd(x[:, :64], dtype), R.rnd(w, dtype), bias, R.pointwise_mfmas(M, 64, True))
        err = np.abs(R.from_bits(got[:, :N], dtype).reshape(M, N) - ref)
        allow = R.typed_allowance(ref, bound, dtype)
        print(f"projection M {M} tiles {ct} lda {lda} {dtype}: max |err| / allowance = {float((err / allow).max()):.3f}")
        assert (err <= allow).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 257])
def test_pointwise_f32_operand_fp32_output(hip_lib, dtype, M):
    """The same launch with an fp32 output beside the typed one: the accumulation bound without the cast (the ratio the module
    docstring of tests/attention_ref.py records), and typed == RNE(fp32)."""
    rng = np.random.default_rng(M)
    w = (rng.standard_normal((64, 64)) / 8).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    x = (rng.standard_normal((M, 64)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
    out, o32 = Guarded(M * 64, "u16"), Guarded(M * 64, "f32")
    dx, wp, dbias = dev(x), dev(_host_pack(hip_lib, dtype, w)), dev(bias)
    _lib.check(hip_lib.fw_pointwise_nhwc(dtype_id(dtype), ptr(dx), 1, 64, M, 64, ptr(wp), ptr(dbias), 2,
                                         out.ptr(), 64, o32.ptr(), 64, None, None, stream()))
    torch.cuda.synchronize()
    got32 = f32(o32.take()).reshape(M, 64)
    ref, bound, A = R.pointwise(R.rnd(x, dtype), R.rnd(w, dtype), bias, R.pointwise_mfmas(M, 64, True))
    err = np.abs(got32.astype(np.float64) - ref)
    _report(f"projection fp32 out M {M} {dtype}", err, A, bound)
    assert (err <= bound).all()
    np.testing.assert_array_equal(out.take().reshape(M, 64), R.to_bits(got32, dtype))


# ---- fw_pointwise_nhwc, (b): P @ v with the gamma residual (typed operand, K = padded pixel count) ---------------------------------
PV_CASES = [(33, 64), (1665, 1696), (8200, 8224), (16400, 16416)]


def pv_inputs(M, K, dtype, device, nrows=None):
    """P (rows, K) and v (M, 64) in the operand type, from a seeded generator on `device`: small noise with planted structure - large
    entries of P and of v at k = 0, at k = M - 1 (the last valid one: it lies in the last, ragged chunk) and on both sides of every
    32-boundary; columns [M, K) of P are zero, as fw_attn_softmax_rows leaves them.  nrows: only that many rows of P (the host test)."""
    g = torch.Generator(device=device)
    g.manual_seed(1000 + M)
    rows = nrows or M
    sign = lambda *shape: (torch.randint(0, 2, shape, generator=g, device=device) * 2 - 1).float()
    P = (torch.rand((rows, K), generator=g, device=device) * 2 - 1) * 2.0 ** -6
    v = torch.rand((M, 64), generator=g, device=device) * 2 - 1
    for off in (31, 32):
        n = len(range(off, M, 32))
        P[:, off:M:32] = 0.5 * sign(rows, n)
        v[off:M:32] = 1.5 * sign(n, 64)
    for kk in (0, M - 1):
        P[:, kk] = 4.0 * sign(rows)
        v[kk] = 6.0 * sign(64)
    P[:, M:] = 0
    return P.to(TDT[dtype]), v.to(TDT[dtype])


def pv_epilogue(M, ldf, nrows=None):
    """The fp32 stream the product is added to, (rows, ldf), and a per-channel gamma with distinct values: negative, zero, above 1."""
    rng = np.random.default_rng(M)
    cs = np.linspace(-0.75, 1.5, 64)
    cs[np.abs(cs).argmin()] = 0.0
    cs = rng.permutation(cs).astype(np.float32)
    return rng.standard_normal((nrows or M, ldf)).astype(np.float32), cs


def pv_sample_rows(M):
    """First and last row and both sides of the 64- and 256-pixel workgroup boundaries, plus a seeded handful."""
    if M <= 2000:
        return np.arange(M)
    rng = np.random.default_rng(M)
    r = np.concatenate([[0, 1, 63, 64, 255, 256, M - 257, M - 256, M - 65, M - 64, M - 2, M - 1], M // 256 * 256 + np.array([-1, 0]),
                        M // 64 * 64 + np.array([-1, 0]), rng.integers(0, M, 16)])
    return np.unique(r[(r >= 0) & (r < M)])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", PV_CASES)
def test_pointwise_pv_residual(hip_lib, dtype, M, K):
    t0 = time.time()
    P, v = pv_inputs(M, K, dtype, "cuda")
    vv = R.from_bits(_bits(v), dtype).reshape(M, 64)
    wt = np.zeros((64, K), np.float32)
    wt[:, :M] = vv.T
    wp = dev(_host_pack(hip_lib, dtype, wt))
    rows = pv_sample_rows(M)
    a = R.from_bits(_bits(P[torch.from_numpy(rows).cuda()]), dtype).reshape(rows.size, K)
    n_mfma = R.pointwise_mfmas(M, K, False)
    for ldf in (64, 72):
        res, cs = pv_epilogue(M, ldf)
        dcs = dev(cs)
        ref, bound, A = R.pointwise(a, wt, None, n_mfma, res[rows, :64], cs)
        for in_place in (True, False):
            stream_buf = Guarded(M * ldf, "f32")
            body = stream_buf.body().view(M, ldf)              # the 64 live channels of every pixel; [64, ldf) keeps the sentinel
            body[:, :64] =dev(res[:, :64].copy().view(np.uint32)).view(torch.int32)
            out_buf = stream_buf if in_place else Guarded(M * ldf, "f32")
            _lib.check(hip_lib.fw_pointwise_nhwc(dtype_id(dtype), ptr(P), 0, K, M, K, ptr(wp), None, 2, None, 0, out_buf.ptr(), ldf,
                                                 stream_buf.ptr(), ptr(dcs), stream()))
            torch.cuda.synchronize()
            got_all = out_buf.take().reshape(M, ldf)
            assert untouched(got_all[:, 64:], "f32"), "channels behind 64 were written"
            if not in_place:
                np.testing.assert_array_equal(stream_buf.take().reshape(M, ldf)[:, :64], res[:, :64].view(np.uint32))   # the stream is read only
            got = f32(got_all[:, :64])
            assert np.isfinite(got).all()
            err = np.abs(got[rows].astype(np.float64) - ref)
            _report(f"P @ v M {M} K {K} {dtype} ldf {ldf} {'in place' if in_place else 'second buffer'} ({n_mfma} MFMAs)", err, A, bound)
            assert (err <= bound).all()
    print(f"P @ v M {M} {dtype}: {time.time() - t0:.2f} s")


# ---- fw_f32_to_planar, fw_copy_channels_f32 ----------------------------------------------------------------------------------------
def _edge_mix(rng, shape, dtype):
    x = (rng.standard_normal(shape) * np.exp(2 * rng.standard_normal(shape))).astype(np.float32)
    e = R.cast_edge_values(dtype)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, 4 * e.size)]
    flat[idx] = np.resize(e, idx.size)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_", [32, 64, 96])
@pytest.mark.parametrize("M", [1, 63, 1665])
def test_f32_to_planar(hip_lib, dtype, C_, M):
    x = _edge_mix(np.random.default_rng([M, C_]), (M, C_), dtype)
    out, dx = Guarded(M * C_, "u16"), dev(x)
    _lib.check(hip_lib.fw_f32_to_planar(dtype_id(dtype), ptr(dx), M, C_, out.ptr(), stream()))
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = R.f32_to_planar(x, dtype)
    np.testing.assert_array_equal(out.take().reshape(C_ // 32, M, 32), want)


@pytest.mark.parametrize("channels,coff,src_stride,dst_stride", [(5, 3, 7, 11), (24, 24, 24, 48), (7, 1, 8, 8), (48, 2, 50, 51)])
@pytest.mark.parametrize("M", [1, 63, 1665])
def test_copy_channels_f32(hip_lib, M, channels, coff, src_stride, dst_stride):
    rng = np.random.default_rng([M, channels])
    src = _edge_mix(rng, (M, src_stride), "f16")
    src[0, 0] = np.float32(1e-40)                                # an fp32 subnormal: a copy keeps it
    out, dsrc = Guarded(M * dst_stride, "f32"), dev(src)
    _lib.check(hip_lib.fw_copy_channels_f32(ptr(dsrc), src_stride, M, channels, out.ptr(), dst_stride, coff, stream()))
    torch.cuda.synchronize()
    got = out.take().reshape(M, dst_stride)
    np.testing.assert_array_equal(got[:, coff:coff + channels], src[:, :channels].view(np.uint32))
    assert untouched(got[:, :coff], "f32") and untouched(got[:, coff + channels:], "f32")


# ---- fw_attn_proj_pack -----------------------------------------------------------------------------------------------------------
def proj_inputs(heads, ch):
    rng = np.random.default_rng([heads, ch])
    dim = heads * ch
    logits = rng.standard_normal((heads, ch, ch)) * 2
    attn = np.exp(logits - logits.max(-1, keepdims=True))
    attn = (attn / attn.sum(-1, keepdims=True)).astype(np.float32)
    return attn, (rng.standard_normal((dim, dim)) / np.sqrt(dim)).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("more", [0, 1])
@pytest.mark.parametrize("heads,ch", [(1, 48), (2, 48), (8, 48), (1, 96)])
def test_attn_proj_pack(hip_lib, dtype, heads, ch, more):
    dim = heads * ch
    k_pad, ct = R.pad32(dim), (dim + 31) // 32 + more
    attn, wp = proj_inputs(heads, ch)
    n = (k_pad // 32) * 2 * ct * 64 * 8
    out, dattn, dwp = Guarded(n, "u16"), dev(attn), dev(wp)
    _lib.check(hip_lib.fw_attn_proj_pack(dtype_id(dtype), ptr(dattn), ptr(dwp), heads, ch, k_pad, ct, out.ptr(), stream()))
    torch.cuda.synchronize()
    m = R.unpack_pointwise(out.take(), ct, k_pad)
    live = np.zeros(m.shape, bool)
    live[:dim, :dim] = True
    assert (m[~live] == 0).all(), "padding must be exact zeros"
    ref, bound = R.proj_fold(attn, wp)
    err = np.abs(R.from_bits(m[:dim, :dim], dtype).reshape(dim, dim) - ref)
    allow = R.typed_allowance(ref, bound, dtype)
    print(f"proj_pack heads {heads} ch {ch} tiles {ct} {dtype}: max |err| / allowance = {float((err / allow).max()):.3f}")
    assert (err <= allow).all()


# ---- the composed AttentionBlock -------------------------------------------------------------------------------------------------
def block_inputs(H, W):
    from framewright_amd.synth import synthetic_attention_state
    asd = synthetic_attention_state(1, 1, seed=5)
    pre = sorted({k.rsplit(".", 2)[0] for k in asd if k.endswith("query.weight")})[0]
    w = {}
    for n in ("query", "key", "value"):
        w[n + "_w"] = asd[f"{pre}.{n}.weight"][:, :, 0, 0]
        w[n + "_b"] = asd[f"{pre}.{n}.bias"]
    rng = np.random.default_rng([H, W])
    w["gamma"] = rng.permutation(np.linspace(-0.75, 1.5, 64)).astype(np.float32)       # per channel, as the kernel takes it
    return (rng.standard_normal((H * W, 64)) * 0.25).astype(np.float32), w, asd, pre      # logits of a few units: P is not one-hot


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(37, 45), (9, 7)])
def test_attention_block_composed(hip_lib, dtype, H, W):
    lib, did, M = hip_lib, dtype_id(dtype), H * W
    x, w, _, _ = block_inputs(H, W)
    kp = R.pad32(M)
    xs = Guarded(M * 64, "f32")
    xs.fill(x)
    qkv, keep = [], []                        # keep: the device operands stay alive until the synchronize
    for n, ct in (("query", 1), ("key", 1), ("value", 2)):
        bias = np.zeros(32 * ct, np.float32)
        bias[:w[n + "_b"].size] = w[n + "_b"]
        o = Guarded(M * 32 * ct, "u16")
        keep += [dev(_host_pack(lib, dtype, w[n + "_w"])), dev(bias)]
        _lib.check(lib.fw_pointwise_nhwc(did, xs.ptr(), 1, 64, M, 64, ptr(keep[-2]), ptr(keep[-1]), ct, o.ptr(),
                                         32 * ct, None, 0, None, None, stream()))
        qkv.append(o)
    P = Guarded(M * kp, "u16")
    _lib.check(lib.fw_attn_softmax_rows(did, qkv[0].ptr(), 32, qkv[1].ptr(), 32, M, 8, P.ptr(), kp, stream()))
    vt = Guarded(lib.fw_pack_pointwise(did, None, 64, kp, None), "u16")
    _lib.check(lib.fw_pack_pointwise_transposed(did, qkv[2].ptr(), 64, M, 64, kp, vt.ptr(), stream()))
    y, dgamma = Guarded(M * 64, "f32"), dev(w["gamma"])
    _lib.check(lib.fw_pointwise_nhwc(did, P.ptr(), 0, kp, M, kp, vt.ptr(), None, 2, None, 0, y.ptr(), 64, xs.ptr(), ptr(dgamma), stream()))
    planar = Guarded(M * 64, "u16")
    _lib.check(lib.fw_f32_to_planar(did, y.ptr(), M, 64, planar.ptr(), stream()))
    torch.cuda.synchronize()
    got = f32(y.take()).reshape(M, 64)
    np.testing.assert_array_equal(f32(xs.take()).reshape(M, 64), x)
    np.testing.assert_array_equal(planar.take().reshape(2, M, 32), R.f32_to_planar(got, dtype))
    for b in qkv + [P, vt]:
        b.take()
    exact, rounded = R.attention_block(x, w), R.attention_block(x, w, dtype)
    q = np.abs(rounded - exact).max()
    lim = 2 * q + 1e-6 * np.abs(exact).max()
    err = np.abs(got - exact).max()
    print(f"attention block {H}x{W} {dtype}: max |err| {err:.3e}, limit {lim:.3e} (q {q:.3e})")
    assert np.abs(exact - x).max() > 50 * lim             # the block does something at this bound
    assert err <= lim
