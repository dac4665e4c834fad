"""TEST INFRASTRUCTURE ONLY (never imported by the product): float64 restatements of the kernels behind AESRGAN's AttentionBlock
(csrc/aesrgan.hip: the pointwise GEMM of csrc/nn_ops.hip as that chain calls it, fw_attn_softmax_rows, fw_pack_pointwise_transposed,
fw_f32_to_planar) and of Restormer's fw_attn_proj_pack / fw_copy_channels_f32 (csrc/restormer_ops.hip), each with a per-element error
bound, in plain numpy.  tests/test_attention_ref_host.py pins the restatements to torch in float64 (oracle.rrdbnet_ref.attention_forward,
project_out(attn @ v) of oracle/restormer_ref.py) and shows that each listed defect leaves its bound; tests/test_attention_ops_gpu.py
holds the kernels to them.

Every function takes the values the kernel reads (typed operands as their exact values in float64, fp32 as fp32) and evaluates in
float64.  u = 2^-24, gamma(k) = k u / (1 - k u) (tests/ifnet_glue_ref.py, whose helpers are reused, not restated).  No term is fitted
to what a kernel returns:

* MFMA sums (the convention of oracle/winograd_ref.py): products of two typed operands are exact in fp32, one fp32 rounding of the
  running sum per MFMA chained into an accumulator.  Both pointwise kernels use v_mfma_f32_32x32x16: two MFMAs per 32-channel chunk.
    - pointwise_mfma_kernel (the 256-pixel kernel: fp32 operand, or more than 16384 pixels): K / 16 MFMAs;
    - pointwise_small_kernel (typed operand, at most 16384 pixels): K walked in stages of 8 chunks, every stage issues its 16 MFMAs
      (the chunks behind K multiply zeros; no credit is taken for that): 16 ceil(K / 256) MFMAs (``pointwise_mfmas``);
    - epilogue: ``acc + bias`` 1 rounding (counted where bias is NULL as well); the residual form ``res + o * chan_scale`` 2 more.
  Bound: gamma(count) * A with A = sum |a w| + |bias|, times |chan_scale| plus |res| for the residual form.
  Measured on the MI355X, max |err| / (2^-24 A) (the tests print it per case):
    - q / k / v projections, K = 64, count 5:                 f16 1.32, bf16 1.15
    - P @ v, K = 64 / 1696 / 8224 / 16416, count 19 / 115 / 531 / 1029:
                                                              f16 3.34 / 7.06 / 3.84 / 2.95, bf16 2.76 / 7.89 / 4.16 / 3.81
    (random signs: the measured ratio does not grow with the count the way the worst-case bound does.)
* fw_attn_softmax_rows: score = sum_{c < d} q_c k_c, 8 chained multiply-adds whatever d is: gamma(8) * sum |q_c k_c|, absolute
  (``e_s``).  p_j = expf(s_j - mx) * (1 / sum_j expf(s_j - mx)) is invariant under the kernel's own mx, so the score error enters p
  relatively, twice - e_s of the element in the numerator, the row's largest e_s through the row sum - as does the rounding of the
  subtraction (|s - mx| <= 20: 20 u) and expf (``EXPF_REL``, measured on [-20, 20]: the reference asserts s - rowmax in [-20, 0]).  The
  row sum adds gamma(ceil(M / 64) + 6): lane-strided partial sums and the 6-step butterfly.  Then the division and the product:
  gamma(2).  Then the cast (``typed_allowance``; f16 subnormals get the absolute half step 2^-25 there).
* fw_attn_proj_pack: Wc[co][h ch + c2] = sum_c1 Wp[co][h ch + c1] A[h][c1][c2] as a chain of ch fp32 multiply-adds:
  gamma(ch) * sum |w| |a|, then the cast.
* fw_pack_pointwise_transposed, fw_f32_to_planar, fw_copy_channels_f32 move or cast values: bit-exact (``to_bits``).
* The composed AttentionBlock (``attention_block``) is judged with the yardstick of tests/test_ifnet_blocks_gpu.py: the float64
  reference is run a second time with x, the weights, q, k, v and P rounded to the operand type at the kernel's rounding points,
  q = max |rounded - exact|, and the kernels must satisfy max |got - exact| <= 2 q + 1e-6 max |exact|.
"""
from __future__ import annotations

import numpy as np

from ifnet_glue_ref import EXPF_REL, U, from_bits, gamma, to_bits, typed_allowance   # noqa: F401  (re-exported to the tests)

SMALL_MAX_M = 16384          # pointwise_small_eligible (csrc/nn_ops.hip): at most this many pixels take the 64-pixel kernel
DEFECTS_SOFTMAX = ("softmax_pad", "p_transposed")
DEFECTS_PV = ("drop_last_chunk", "swap_halves", "gamma_n4")


def rnd(x, dtype: str) -> np.ndarray:
    """fp32 values rounded to the operand type (RNE), as float64."""
    x = np.asarray(x, np.float32)
    return from_bits(to_bits(x, dtype), dtype).reshape(x.shape)


def pad32(n: int) -> int:
    return (n + 31) // 32 * 32


# ---- fw_attn_softmax_rows --------------------------------------------------------------------------------------------------------
def softmax_rows(q, k, d: int, rows=None, p_stride: int | None = None, defect: str | None = None):
    """p[i][j] = softmax_j(sum_{c < d} q[i][c] k[j][c]) for the given rows i (default: all).  q, k: (M, >= d) exact typed values.
    Returns (p, bound, lo): (R, M) float64, the bound BEFORE the cast, and the smallest s - rowmax met (the expf range)."""
    q, k = np.asarray(q, np.float64)[:, :d], np.asarray(k, np.float64)[:, :d]
    M = k.shape[0]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    if defect == "p_transposed":
        full, bnd, lo = softmax_rows(q, k, d)
        return full.T[rows], bnd.T[rows], lo
    s = q[rows] @ k.T
    e_s = gamma(8) * (np.abs(q[rows]) @ np.abs(k.T))
    if defect == "softmax_pad":                     # the padded columns [M, p_stride) take part with score 0
        npad = (p_stride if p_stride is not None else pad32(M)) - M
        sp = np.concatenate([s, np.zeros((rows.size, npad))], 1)
        mx = sp.max(1, keepdims=True)
        ex = np.exp(sp - mx)
        p = (ex / ex.sum(1, keepdims=True))[:, :M]
    else:
        mx = s.max(1, keepdims=True)
        ex = np.exp(s - mx)
        p = ex / ex.sum(1, keepdims=True)
    lo = float((s - s.max(1, keepdims=True)).min())
    rel = (e_s + e_s.max(1, keepdims=True) + 2 * 20 * U + 2 * EXPF_REL + gamma((M + 63) // 64 + 6) + gamma(2)) * (1 + 2.0 ** -10)
    return p, p * rel, lo


# ---- the pointwise GEMM ----------------------------------------------------------------------------------------------------------
def pointwise_mfmas(M: int, K: int, a_is_f32: bool) -> int:
    """MFMAs chained into one accumulator element, from the kernel the launch takes (csrc/nn_ops.hip, launch_pointwise)."""
    if a_is_f32 or M > SMALL_MAX_M:
        return K // 16
    return 16 * ((K + 255) // 256)


def pointwise(a, w, bias, n_mfma: int, res=None, chan_scale=None, defect: str | None = None):
    """out[m][n] = sum_k a[m][k] w[n][k] + bias[n]; with res: res[m][n] + out[m][n] * chan_scale[n].  a (R, K), w (N, K): exact typed
    values; bias, chan_scale, res fp32.  Returns (ref, bound, A): A is the sum of magnitudes the bound scales with."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    K = a.shape[1]
    if defect == "drop_last_chunk":
        a = a.copy()
        a[:, K - 32:] = 0
    if defect == "swap_halves":
        w = w[:, np.arange(K) ^ 16]
    acc, A = a @ w.T, np.abs(a) @ np.abs(w.T)
    if bias is not None:
        b = np.asarray(bias, np.float64)
        acc, A = acc + b, A + np.abs(b)
    if res is None:
        return acc, gamma(n_mfma + 1) * A, A
    cs = np.asarray(chan_scale, np.float64)
    if defect == "gamma_n4":
        cs = np.roll(cs, -4)
    r = np.asarray(res, np.float64)
    A = np.abs(r) + A * np.abs(cs)
    return r + acc * cs, gamma(n_mfma + 3) * A, A


# ---- fragment order of fw_pack_pointwise -----------------------------------------------------------------------------------------
def unpack_pointwise(bits, cout_tiles: int, k_pad: int) -> np.ndarray:
    """[chunk][ks][cout tile][lane][8] (cout = 32 tile + (lane & 31), k = 32 chunk + 16 ks + 8 (lane >> 5) + j) -> (32 cout_tiles,
    k_pad) of the same uint16."""
    f = np.asarray(bits, np.uint16).reshape(k_pad // 32, 2, cout_tiles, 2, 32, 8)       # [c][ks][t][lane >> 5][lane & 31][j]
    return f.transpose(2, 4, 0, 1, 3, 5).reshape(32 * cout_tiles, k_pad)                # [t][lane & 31] x [c][ks][lane >> 5][j]


def pack_pointwise(mat_bits, cout_tiles: int, k_pad: int) -> np.ndarray:
    """The inverse: (cout, k) uint16, zero-padded to (32 cout_tiles, k_pad), in fragment order."""
    m = np.zeros((32 * cout_tiles, k_pad), np.uint16)
    m[:mat_bits.shape[0], :mat_bits.shape[1]] = mat_bits
    return m.reshape(cout_tiles, 32, k_pad // 32, 2, 2, 8).transpose(2, 3, 0, 4, 1, 5).reshape(-1)


# ---- fw_attn_proj_pack -----------------------------------------------------------------------------------------------------------
def proj_fold(attn, wp):
    """Wp x blockdiag(attn): attn (heads, ch, ch), wp (dim, dim) fp32 -> (dim, dim) float64 and the bound before the cast."""
    heads, ch, _ = attn.shape
    a, w = attn.astype(np.float64), wp.astype(np.float64)
    out, mag = np.zeros_like(w), np.zeros_like(w)
    for h in range(heads):
        sl = slice(h * ch, (h + 1) * ch)
        out[:, sl] = w[:, sl] @ a[h]
        mag[:, sl] = np.abs(w[:, sl]) @ np.abs(a[h])
    return out, gamma(ch) * mag


# ---- casts and copies ------------------------------------------------------------------------------------------------------------
def f32_to_planar(x, dtype: str) -> np.ndarray:
    """fp32 (M, C) -> uint16 chunk-planar (C / 32, M, 32)."""
    M, C = x.shape
    return to_bits(x, dtype).reshape(M, C // 32, 32).transpose(1, 0, 2)


def cast_edge_values(dtype: str) -> np.ndarray:
    """fp32 values on which a cast goes wrong first: ties (both parities), f16's overflow threshold, f16-subnormal magnitudes, +-0."""
    mant = 10 if dtype == "f16" else 7
    h = 2.0 ** -(mant + 1)
    v = [0.0, -0.0, 1.0, 1 + h, 1 + 3 * h, 1 + h * (1 + 2.0 ** -10), 1 + h * (1 - 2.0 ** -10), -(1 + h), -(1 + 3 * h),
         65504.0, 65519.0, 65519.996, 65520.0, -65520.0, 2.0 ** -14, 2.0 ** -24, 1.5 * 2.0 ** -24, 0.5 * 2.0 ** -24, 0.50001 * 2.0 ** -24,
         2.5 * 2.0 ** -24, -2.0 ** -25, 3.0e-5, 1.0 / 3.0, 255.0 / 256.0, 1000.5]
    return np.array(v, np.float32)


# ---- the composed AttentionBlock (csrc/aesrgan.hip, the five calls behind an RRDB) -----------------------------------------------
def attention_block(x, w, dtype: str | None = None):
    """x (M, 64) fp32; w: query / key (8, 64), value (64, 64) weights with their biases, gamma (64,), fp32.  out = x + gamma * (P @ v),
    P = softmax_rows(q, k).  dtype: round x, the weights, q, k, v and P to the operand type where the kernels do."""
    r = (lambda t: rnd(t, dtype)) if dtype else (lambda t: np.asarray(t, np.float64))
    xq = r(x)
    q, k, v = (r(xq @ r(w[n + "_w"]).T + w[n + "_b"].astype(np.float64)) for n in ("query", "key", "value"))
    p, _, _ = softmax_rows(q, k, 8)
    return x.astype(np.float64) + w["gamma"].astype(np.float64) * (r(p) @ v)


# ---- seeded inputs shared by the host and the GPU tests --------------------------------------------------------------------------
def softmax_inputs(M: int, d: int, kind: str, dtype: str, stride: int = 32):
    """Typed q, k as uint16 (M, stride) and their exact values.  "engine": scores of a few units, as a trained block has them;
    "sharp": every q row has sum |q_c| = 9.5 over the d channels, so that the spread of a row's scores is at most 19, and row 0 / key rows
    0 and M - 1 reach it.  Every seventh row (from row 1) points against key channel 0, which is positive in every key: all its scores
    are negative, so a padded column with score 0 would take the row over.  Channels [d, 8) hold large values the kernel must not use."""
    rng = np.random.default_rng([M, d, kind == "sharp"])
    k = rng.uniform(-1, 1, (M, stride))
    k[:, 0] = rng.uniform(0.5, 1, M)
    q = rng.uniform(-1, 1, (M, stride))
    if kind == "sharp":
        q[:, :d] *= 9.5 / np.abs(q[:, :d]).sum(1, keepdims=True)
        q[0, :d] = 9.5 / d
        k[0, :d], k[M - 1, :d] = 1.0, -1.0
        k[M - 1, 0] = 2.0 ** -6
        q[1::7, :d] = 0
        q[1::7, 0] = -9.5
    else:
        q[1::7, :d] *= 0.25
        q[1::7, 0] = -12.0
    q[:, d:8] = rng.uniform(-300, 300, (M, 8 - d))
    k[:, d:8] = rng.uniform(-300, 300, (M, 8 - d))
    qb, kb = to_bits(q, dtype).reshape(M, stride), to_bits(k, dtype).reshape(M, stride)
    return qb, kb, from_bits(qb, dtype).reshape(M, stride), from_bits(kb, dtype).reshape(M, stride)


def softmax_sample_rows(M: int) -> np.ndarray:
    """First and last row, both sides of the second trip of the row loop (8192 rows in flight), a seeded handful in between."""
    rng = np.random.default_rng(M)
    r = np.concatenate([[0, 1, 2, M - 2, M - 1, 8191, 8192, 8193], rng.integers(0, M, 24)])
    return np.unique(r[(r >= 0) & (r < M)])
