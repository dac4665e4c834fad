"""ORACLE — test infrastructure only: float64 references of the two conv5 kernels of the split trunk, and the error bounds that
pin them (numpy only: no torch, no library, so the host-only sensitivity test can use it on a machine without a GPU).

Both kernels compute, for 64 output channels (csrc/fw_internal.h, EPI_RESIDUAL_SPLIT):

    y = s1 * (conv3x3(x) + bias + in_id_scale * x[0:64] + sum_{c < n_id} id_scale[c] * plane_c)    [; lrelu(y, 0.2) if post_act]
    hi = f16(y),  lo = f16(y - hi)

* ``split_contract`` is that formula in float64 on the exact f16 values the kernel reads, with f16-rounded weights: the direct
  kernel (csrc/conv3x3_mfma.hip) differs from it by fp32 accumulation alone.
* ``winograd_emulation`` is what the row-wise Winograd F(2, 3) kernel (csrc/conv3x3_wino.hip) computes at its rounding points:
  U = f16(0.5f * ((g0 + g1) + g2)) etc. from the fp32 weights (the packer's rule), V = B^T d in f16 arithmetic (RNE, as the packed
  f16 adds), products / sums / output transform in float64, the bias in m1, identity terms as + s I into frequency 0 (column 2j)
  and - s I into frequency 3 (column 2j + 1).  The kernel differs from it by fp32 accumulation alone.

Bounds are per output element, so they hold at any scale:

* accumulation (kernel vs its own reference): ``eps * A`` with A = |s1| * (sum |products| + |bias| + sum |identity terms|).
  For the Winograd kernel A is the larger of the direct form's and the Winograd form's own sum of magnitudes (its accumulators hold
  U_f V_f, whose magnitudes can exceed the direct form's).  eps comes from the accumulation depth, one fp32 rounding of the running
  sum per MFMA (products of f16 operands are exact in fp32): the direct kernel chains 9 taps x 6 chunks = 54 MFMAs plus at most
  8 identity MFMAs into an accumulator, 62 * 2^-24 < 2^-18 = ``ACC_EPS_DIRECT``; the Winograd kernel 3 tap rows x 6 chunks = 18
  plus at most 8 identity MFMAs per frequency and 2 adds of the output transform, 28 * 2^-24 < 2^-19 = ``ACC_EPS_WINO``.  Measured
  on the MI355X the direct kernel reaches 1.7 x 2^-20 A and the Winograd kernel 0.9 x 2^-20 A (the test prints the ratios), so
  16 ulp (2^-20) alone would be too tight for the direct kernel's 62-deep chains.
* Winograd vs the contract, a priori: ``2^-9 * |s1| * sum_{f, dy, ci} (G|g|)_f (B^T|d|)_f`` over the three frequencies that enter the
  output (f = 0, 1, 2 for column 2j, 1, 2, 3 for column 2j + 1), plus the accumulation bound, plus 2^-23 |s1| sum (B^T|d|)_f for
  f16 subnormal weights (absolute, not relative, rounding).  The transforms of the absolute taps and pixels are used, not
  |U_f||V_f|: where g0 + g1 + g2 ~ 0, U is small but the rounding of the individual taps is not.  Per product: U rounded once
  (2^-11), the fp32 weights against the contract's f16-rounded ones (2^-11), V rounded once (2^-11): 3 * 2^-11 < 2^-9.
* hi / lo: |hi + lo - y_ref| <= acc + ulp_f16(lo) / 2, and hi is the f16 nearest to hi + lo (|lo| <= half the gap to hi's
  neighbour on lo's side).

V is formed in f16, so d1 + d2 (and d0 - d2, d1 - d3) overflow where the direct form does not: the Winograd form is finite for
|x| <= ``V_F16_DOMAIN`` = 32752 (= 65504 / 2; the next f16, 32768, gives 32752 + 32768 = 65520, which rounds to inf).
"""
from __future__ import annotations

import numpy as np

ACC_EPS_DIRECT = 2.0 ** -18
ACC_EPS_WINO = 2.0 ** -19
APRIORI_EPS = 2.0 ** -9
SUBNORMAL_EPS = 2.0 ** -23
V_F16_DOMAIN = 32752.0
LRELU_SLOPE = 0.2


def f16(a) -> np.ndarray:
    """Round to f16 (RNE), the rounding of the kernels' f32 -> f16 conversions."""
    return np.asarray(a, np.float32).astype(np.float16)


def _pad(x: np.ndarray, r0: int, r1: int, npairs: int) -> np.ndarray:
    """Rows r0 - 1 .. r1 of x (H, W, C) with zero padding; column index k = image column k - 1, 2 * npairs + 2 columns."""
    H, W, C = x.shape
    out = np.zeros((r1 - r0 + 2, 2 * npairs + 2, C), x.dtype)
    a, b = max(r0 - 1, 0), min(r1 + 1, H)
    out[a - (r0 - 1):b - (r0 - 1), 1:W + 1] = x[a:b]
    return out


def _mm(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(..., K) @ (K, N) in float64."""
    return (a.reshape(-1, a.shape[-1]) @ b).reshape(a.shape[:-1] + (b.shape[-1],))


def _mm_abs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a| @ |b| for the magnitude sums that scale the bounds: fp32 (a relative error of 2^-24 * K is immaterial there), which
    halves the cost of a 1080p reference."""
    a32 = np.abs(a).astype(np.float32)
    return (a32.reshape(-1, a.shape[-1]) @ np.abs(b).astype(np.float32)).reshape(a.shape[:-1] + (b.shape[-1],)).astype(np.float64)


def wino_weights(w: np.ndarray) -> np.ndarray:
    """The packer's U = G g per tap row (csrc/conv3x3_wino.hip, pack_conv3x3_wino_weights): fp32 sums, rounded to f16 once.
    w: [cout][cin][3][3] fp32 -> U[dy][f][cout][cin] (f16)."""
    return wino_weights_f32(w).transpose(3, 0, 1, 2).astype(np.float16)


def wino_weights_f32(w: np.ndarray) -> np.ndarray:
    """U before its rounding to f16: [f][cout][cin][dy], float32 arithmetic in the packer's order."""
    g = np.asarray(w, np.float32)
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    half = np.float32(0.5)
    return np.stack([g0, half * ((g0 + g1) + g2), half * ((g0 - g1) + g2), g2])


def _identity_terms(x, planes, in_id_scale, id_scale, r0, r1, cout):
    """[(scale, 32- or 64-channel source rows r0..r1, first output channel)] of the identity terms."""
    terms = []
    if in_id_scale != 0:
        terms.append((float(in_id_scale), x[r0:r1, :, :min(64, x.shape[2])], 0))
    for c in range(len(id_scale)):
        terms.append((float(id_scale[c]), planes[c][r0:r1], 32 * (c & 1)))
    return terms


def split_contract(x, w, bias, s1=1.0, in_id_scale=0.0, planes=(), id_scale=(), post_act=False, act=0, rows=None):
    """The contract in float64 on f16 inputs with f16-rounded weights.  x: (H, W, 32 * cin_chunks) f16, w: [64][cin][3][3] fp32
    (cin <= x channels), planes: n_id arrays (H, W, 32) f16.  act = 1 is the STORE form's LeakyReLU (no identities, s1 = 1).
    Returns (y, A) for output rows rows = (r0, r1) (default all): y (r1 - r0, W, 64), A = the sum of magnitudes."""
    H, W, C = x.shape
    r0, r1 = rows or (0, H)
    cout, cin = w.shape[:2]
    wq = np.zeros((3, 3, C, cout))
    wq[:, :, :cin] = f16(w).astype(np.float64).transpose(2, 3, 1, 0)
    npairs = (W + 1) // 2
    xp = _pad(x, r0, r1, npairs).astype(np.float64)
    nr = r1 - r0
    y = np.zeros((nr, W, cout))
    A = np.zeros((nr, W, cout))
    for dy in range(3):
        for dx in range(3):
            xs = xp[dy:dy + nr, dx:dx + W]
            y += _mm(xs, wq[dy, dx])
            A += _mm_abs(xs, wq[dy, dx])
    b = np.asarray(bias, np.float32).astype(np.float64)[:cout]
    y += b
    A += np.abs(b)
    for sc, src, co in _identity_terms(x, planes, in_id_scale, id_scale, r0, r1, cout):
        t = sc * src.astype(np.float64)
        y[..., co:co + t.shape[-1]] += t
        A[..., co:co + t.shape[-1]] += np.abs(t)
    s1 = float(np.float32(s1))
    y *= s1
    A *= abs(s1)
    if post_act or act == 1:
        y = np.where(y >= 0, y, LRELU_SLOPE * y)
    return y, A


def winograd_emulation(x, w, bias, s1=1.0, in_id_scale=0.0, planes=(), id_scale=(), act=0, rows=None, exact=False, variant=None):
    """The Winograd kernel at its rounding points (module docstring).  Returns (y, A_w, apriori) for rows (r0, r1): y the output,
    A_w the Winograd form's own sum of magnitudes (|s1| included), apriori the transform-of-absolutes sum of the module docstring
    (|s1| included, the 2^-9 and subnormal factors not).
    exact = True: U = G g16 and V = B^T d in float64 (must reproduce split_contract).  variant: a deliberately wrong kernel for
    the sensitivity test - "swap12" (frequencies 1 and 2 swapped), "bias_m0" (the bias in m0), "u_bf16" (U rounded to bf16),
    "flip3" (+ s I into frequency 3), "no_lo" is applied by the caller."""
    H, W, C = x.shape
    r0, r1 = rows or (0, H)
    nr = r1 - r0
    cout, cin = w.shape[:2]
    npairs = (W + 1) // 2
    if exact:
        g = f16(w).astype(np.float64)
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
        U = np.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2]).transpose(3, 0, 1, 2)
    else:
        U = wino_weights(w).astype(np.float64)
        if variant == "u_bf16":
            U = _round_bf16(wino_weights_f32(w)).transpose(3, 0, 1, 2)
    if variant == "swap12":
        U = U[:, [0, 2, 1, 3]]
    Uk = np.zeros((3, 4, C, cout))
    Uk[:, :, :cin] = U.transpose(0, 1, 3, 2)
    xp = _pad(x, r0, r1, npairs)
    d = [xp[:, k:k + 2 * npairs:2] for k in range(4)]          # (nr + 2, npairs, C) f16, column 2j - 1 + k
    if exact:
        d = [v.astype(np.float64) for v in d]
    V = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]   # f16 arithmetic (RNE) unless exact
    V = [v.astype(np.float64) for v in V]
    m = [np.zeros((nr, npairs, cout)) for _ in range(4)]
    mag = [np.zeros((nr, npairs, cout)) for _ in range(4)]
    for dy in range(3):
        for f in range(4):
            vs = V[f][dy:dy + nr]
            m[f] += _mm(vs, Uk[dy, f])
            mag[f] += _mm_abs(vs, Uk[dy, f])
    b = np.asarray(bias, np.float32).astype(np.float64)[:cout]
    fb = 0 if variant == "bias_m0" else 1
    m[fb] += b
    mag[fb] += np.abs(b)
    s3 = 1.0 if variant == "flip3" else -1.0
    for sc, src, co in _identity_terms(x, planes, in_id_scale, id_scale, r0, r1, cout):
        t = np.zeros((nr, 2 * npairs, src.shape[-1]))
        t[:, :W] = sc * src.astype(np.float64)
        n = t.shape[-1]
        m[0][..., co:co + n] += t[:, 0::2]
        m[3][..., co:co + n] += s3 * t[:, 1::2]
        mag[0][..., co:co + n] += np.abs(t[:, 0::2])
        mag[3][..., co:co + n] += np.abs(t[:, 1::2])
    s1 = float(np.float32(s1))
    out = np.empty((nr, 2 * npairs, cout))
    out[:, 0::2] = m[0] + m[1] + m[2]
    out[:, 1::2] = m[1] - m[2] - m[3]
    A = np.empty_like(out)
    A[:, 0::2] = mag[0] + mag[1] + mag[2]
    A[:, 1::2] = mag[1] + mag[2] + mag[3]
    out *= s1
    A *= abs(s1)
    if act == 1:
        out = np.where(out >= 0, out, LRELU_SLOPE * out)
    apriori = _apriori(x, w, r0, r1, npairs) * abs(s1)
    return out[:, :W], A[:, :W], apriori[:, :W]


def _round_bf16(a: np.ndarray) -> np.ndarray:
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _apriori(x, w, r0, r1, npairs):
    """sum over dy, ci and the three frequencies entering each output of (G|g|)_f (B^T|d|)_f, plus 2^-23 / 2^-9 times
    sum (B^T|d|)_f (the absolute rounding of f16 subnormal weights, pre-scaled so that the caller's 2^-9 factor applies)."""
    H, W, C = x.shape
    cout, cin = w.shape[:2]
    a = np.abs(np.asarray(w, np.float64))
    S = a.sum(-1)                                              # |g0| + |g1| + |g2|   [cout][cin][dy]
    sub = SUBNORMAL_EPS / APRIORI_EPS
    # column 2j (f = 0, 1, 2): |g0| (|d0| + |d2|) + S (|d1| + |d2|) -> taps on |x| at columns 2j - 1, 2j, 2j + 1
    # column 2j + 1 (f = 1, 2, 3): S (|d1| + |d2|) + |g2| (|d1| + |d3|) -> taps at columns 2j, 2j + 1, 2j + 2
    ke = np.stack([a[..., 0] + sub, S + sub, a[..., 0] + S + 2 * sub], -1)
    ko = np.stack([S + a[..., 2] + 2 * sub, S + sub, a[..., 2] + sub], -1)
    kk = np.zeros((2, 3, 3, C, cout))                          # [parity][dy][tap][ci][co]
    kk[0, :, :, :cin] = ke.transpose(2, 3, 1, 0)
    kk[1, :, :, :cin] = ko.transpose(2, 3, 1, 0)
    xp = _pad(x, r0, r1, npairs)
    nr = r1 - r0
    out = np.zeros((nr, 2 * npairs, cout))
    for par in range(2):
        for dy in range(3):
            for t in range(3):
                # output column 2j + par reads padded column 2j + par + t (image column 2j + par + t - 1)
                out[:, par::2] += _mm_abs(xp[dy:dy + nr, par + t:par + t + 2 * npairs:2], kk[par, dy, t])
    return out


def split_hi_lo(y) -> tuple:
    """What a faithful kernel stores for a float64 result: y rounded to fp32 (its accumulator), hi = f16(y), lo = f16(y - hi)."""
    y32 = np.asarray(y, np.float32)
    hi = y32.astype(np.float16)
    lo = (y32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def check_hi_lo(hi, lo, y_ref, acc) -> dict:
    """The three hi / lo checks against a float64 reference (lo = None: hi alone, against acc + half an ulp of hi).
    Returns the measured numbers and ``ok``."""
    h = np.asarray(hi, np.float16)
    got = h.astype(np.float64)
    finite = bool(np.isfinite(got).all())
    if lo is not None:
        l16 = np.asarray(lo, np.float16)
        got = got + l16.astype(np.float64)
        slack = np.spacing(np.abs(l16)).astype(np.float64) / 2
        nb = np.nextafter(h, np.where(l16 < 0, np.float16(-np.inf), np.float16(np.inf)))
        gap = np.abs(nb.astype(np.float64) - h.astype(np.float64))
        nearest_ok = bool((np.abs(l16.astype(np.float64)) <= gap / 2).all())
        finite = finite and bool(np.isfinite(l16).all())
    else:
        slack = np.spacing(np.abs(h)).astype(np.float64) / 2
        nearest_ok = True
    err = np.abs(got - y_ref)
    bound = acc + slack
    big = np.abs(y_ref) > 1e-3 * max(float(np.abs(y_ref).max()), 1e-30)
    return {
        "max_abs": float(err.max()),
        "max_rel": float((err[big] / np.abs(y_ref[big])).max()) if big.any() else 0.0,
        "ratio": float((err / bound).max()),
        "nearest_ok": nearest_ok,
        "finite": finite,
        "ok": finite and nearest_ok and bool((err <= bound).all()),
    }


def check_apriori(y_kernel, y_contract, apriori, acc) -> dict:
    """The Winograd result (hi + lo, or the STORE form's hi plus its half ulp) against the contract, a priori."""
    err = np.abs(np.asarray(y_kernel, np.float64) - y_contract)
    bound = APRIORI_EPS * apriori + acc
    return {"max_abs": float(err.max()), "ratio": float((err / bound).max()), "ok": bool((err <= bound).all())}
