"""TEST INFRASTRUCTURE ONLY (never imported by the product): float64 restatements of the fused conv pair (csrc/conv3x3_pair.hip,
conv3x3_pair_slide.hip, conv3x3_pair_slide32.hip: x_a = lrelu(conv_a(x)), x_b = lrelu(conv_b(cat(x, x_a)))) and of the two forms of
lrelu(conv3x3(nearest_x2(x))) (csrc/conv_up2x_phase.hip, the four 2x2 phase convolutions; conv3x3_mfma.hip's ``upsample2x`` gather),
each with a per-element bound, in plain numpy.  tests/test_conv_pair_ref_host.py pins them to torch in float64 and shows that each
listed defect leaves its bound; tests/test_conv_pair_gpu.py holds the kernels to them.

Bounds (u = 2^-24, gamma(k) = k u / (1 - k u), helpers of tests/ifnet_glue_ref.py; A = sum |w x| + |bias|), none fitted to what a
kernel returns.  The convention is that of tests/conv_epilogue_ref.py: products of typed operands are exact and every
v_mfma_f32_16x16x32 rounds the running fp32 sum once.

* x_a: the accumulators start at bias_a (conv3x3_pair.hip, "accumulators start at the bias") and chain, per shared 32-channel chunk,
  the nine taps of ``conv_item`` / ``conv_item_lag`` (conv_pair_common.h: ``for t < 9`` with one ``mfma16`` per accumulator tile):
  9 * na MFMAs.  ``lrelu4`` (conv_common.h) is ``v_max_f32(v, v * 0.2f)``: one product more; LeakyReLU is Lipschitz with constant 1,
  so a t on the other side of zero than the reference's costs no more than its own error: gamma(9 na + 1) * A_a.  The constant is
  ``S`` = fp32(0.2), the kernel's.
* x_b: the same chain over na + 1 chunks, the last one the x_a tile in LDS: gamma(9 (na + 1) + 1) * A_b.  x_b is held to conv_b of
  THE KERNEL'S OWN stored x_a (decoded exactly from its bits), so nothing is lost to a rounding flip of x_a; the same comparison
  tests that the x_a tile in LDS holds the bytes that were stored, and zeros outside the image.
* both outputs are typed (``pair16``: RNE of the fp32 value): |got - ref| <= typed_allowance(ref, bound, dtype).
* the phase form: the packer sums the taps that a phase folds onto one source offset in float64 and rounds the sum to the operand
  type ONCE (include/framewright_hip.h, fw_pack_conv_up2x_phase); ``conv_item_up`` runs 8 steps = 4 taps x 2 column phases, each
  accumulator tile is touched by 4 of them per chunk, two chunks: gamma(4 * 2 + 1) * A with the activation's product.
* the gather form (fw_conv3x3_nhwc, upsample2x = 1) is the plain conv on the repeated pixels: gamma(9 * 2 + 1) * A on its fp32
  output; the typed output is the RNE of the fp32 output, bit for bit.
* phase against gather: the two differ a priori by the rounding of the weights only: per folded weight
  |rnd(sum w) - sum rnd(w)| <= ulp(sum w) / 2 + sum ulp(w) / 2 of the operand type (``phase_apriori``), times |x|, summed.

Measured on the MI355X, the largest max |err| / allowance over all cases and both layouts (the tests print it per case).  Half an
ulp of the output type alone accounts for up to 1, so these figures say that the bounds hold, not how much of the fp32 part is used;
the three pair kernels return the same bytes, hence the same figures:
    - ring kernel (FW_PAIR_SLIDE=0):        x_a / x_b  f16 0.995 / 0.988, bf16 0.999 / 0.998
    - window kernel (FW_PAIR_SLIDE=1):      x_a / x_b  f16 0.995 / 0.988, bf16 0.999 / 0.998
    - 32-column window (FW_PAIR_SLIDE=2):   x_a / x_b  f16 0.995 / 0.988, bf16 0.999 / 0.998
    - phase kernel:                         f16 0.997, bf16 0.999
    - gather, fp32 output, max |err| / bound:           f16 0.115, bf16 0.112
    - |phase - gather fp32| / (both bounds + a priori): f16 0.246, bf16 0.261

The defect ``double_rounded_sum`` (the summed phase weight rounded to fp32 first, then to the type) is the one the host test
treats apart: it moves a few of the 65536 weights by one ulp and leaves the allowance (by up to 54x) at a few outputs per thousand
only, on some input sets: tests/test_conv_pair_ref_host.py::test_double_rounded_sum.  The packer is therefore pinned bit for bit
(test_phase_packer_rounds_the_sum_once): it did round twice until these tests were written.
"""
from __future__ import annotations

import numpy as np

import conv_epilogue_ref as R
from ifnet_glue_ref import from_bits, gamma, to_bits, typed_allowance, typed_ulp   # noqa: F401  (re-exported)

S = float(np.float32(0.2))          # lrelu4's constant
DEFECTS_PAIR = ("xa_outside_bias", "xa_seam_tap", "xa_row_lag", "lrelu_missing_b", "bias_b_n16")
DEFECTS_PHASE = ("phase_rows_swapped", "double_rounded_sum")


def lrelu(t):
    return np.maximum(t, S * t)


def _band(H: int, rows):
    r0, r1 = (0, H) if rows is None else rows
    assert 0 <= r0 < r1 <= H
    return r0, r1


def _conv_rows(x, w, bias, r0: int, r1: int):
    """R.conv3x3 on output rows [r0, r1) of x (H, W, C): the halo rows come from x, zero padding outside the image."""
    H = x.shape[0]
    lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
    t, A = R.conv3x3(x[lo:hi], w, bias)
    return t[r0 - lo:r1 - lo], A[r0 - lo:r1 - lo]


# ---- the fused pair --------------------------------------------------------------------------------------------------------------
def pair_a(x, wa, ba, rows=None):
    """x (H, W, 32 na), wa (32, 32 na, 3, 3): exact typed values; ba fp32.  Returns lrelu(conv_a(x) + ba) and its fp32 bound on rows."""
    r0, r1 = _band(x.shape[0], rows)
    t, A = _conv_rows(x, wa, ba, r0, r1)
    return lrelu(t), gamma(9 * (x.shape[2] // 32) + 1) * A


def _xa_term(xa, wxa, r0: int, r1: int, shift: int = 0):
    """sum over the nine taps of x_a[y + shift + dy - 1, x + dx - 1] * w on rows [r0, r1): conv_b's last chunk alone."""
    H, W, _ = xa.shape
    ext = np.zeros((H + 2, W, 32))
    ext[:H] = xa
    return _conv_rows(ext, wxa, np.zeros(32), r0 + shift, r1 + shift)[0]


def pair_b_pre(x, xa, wb, bb, rows=None):
    """conv_b(cat(x, xa)) + bb and its magnitude sum on rows: what ``pair_b`` starts from (``pre=``: computed once, shared by the defects)."""
    r0, r1 = _band(x.shape[0], rows)
    return _conv_rows(np.concatenate([np.asarray(x, np.float64), xa], 2), wb, bb, r0, r1)


def pair_b(x, xa, wb, bb, rows=None, defect: str | None = None, ring=None, pre=None):
    """x_b = lrelu(conv_b(cat(x, xa)) + bb) on rows, xa (H, W, 32) the kernel's stored x_a decoded exactly.  Returns the value, its
    fp32 bound and the mask of the elements a defect touches (all of them without one).  ring (32): what "xa_outside_bias" finds
    outside the image."""
    assert defect is None or defect in DEFECTS_PAIR
    H, W, cin = x.shape
    na = cin // 32
    r0, r1 = _band(H, rows)
    wb = np.asarray(wb, np.float64)
    bb = np.asarray(bb, np.float64)
    t, A = pre if pre is not None else pair_b_pre(x, xa, wb, bb, rows)
    t = t.copy()
    wxa = wb[:, cin:]
    touched = np.ones(t.shape, bool)
    if defect == "xa_outside_bias":                       # x_a of the padding ring = lrelu(bias_a) where it has to be zero
        out = np.zeros((H + 2, W + 2, 32)) + np.asarray(ring, np.float64)
        out[1:-1, 1:-1] = 0
        t = t + R.conv3x3(out, wxa, np.zeros(32))[0][1:-1, 1:-1][r0:r1]
        touched[:] = False
        yy = np.arange(r0, r1)
        touched[(yy == 0) | (yy == H - 1)] = True
        touched[:, [0, W - 1]] = True
    elif defect == "xa_seam_tap":                         # output column 30 k + 29 misses x_a of column 30 k + 30 at tap dx = 2
        cols = np.arange(29, W - 1, 30)
        xp = np.zeros((H + 2, W, 32))
        xp[1:-1] = xa
        touched[:] = False
        for dy in range(3):
            t[:, cols] -= xp[r0 + dy:r1 + dy][:, cols + 1] @ wxa[:, :, dy, 2].T
        touched[:, cols] = True
    elif defect == "xa_row_lag":                          # rows 16 k take their x_a one row low
        yy = np.arange(r0, r1)
        sel = yy % 16 == 0
        t[sel] += (_xa_term(xa, wxa, r0, r1, 1) - _xa_term(xa, wxa, r0, r1))[sel]
        touched[:] = False
        touched[sel] = True
    elif defect == "bias_b_n16":
        t = t + (np.roll(bb, -16) - bb)
    if defect == "lrelu_missing_b":
        y, touched = t, t < 0
    else:
        y = lrelu(t)
    return y, gamma(9 * (na + 1) + 1) * A, touched


def pair(x, wa, ba, wb, bb, xa_bits, dtype: str, rows=None, defect: str | None = None):
    """The whole pair on rows: (ref_a, bound_a, ref_b, bound_b, touched_b).  xa_bits (H, W, 32) uint16: the stored x_a that conv_b
    is held to (the kernel's own on the GPU, the reference's own typed x_a on the host)."""
    ref_a, bound_a = pair_a(x, wa, ba, rows)
    xa = from_bits(xa_bits, dtype).reshape(x.shape[0], x.shape[1], 32)
    ref_b, bound_b, touched = pair_b(x, xa, wb, bb, rows, defect, ring=R.rnd(lrelu(np.asarray(ba, np.float64)), dtype))
    return ref_a, bound_a, ref_b, bound_b, touched


# ---- lrelu(conv3x3(nearest_x2(x))) -----------------------------------------------------------------------------------------------
_FOLD = {0: ([0], [1, 2]), 1: ([0, 1], [2])}


def phase_weights_ref(w):
    """The four 2x2 phase kernels of nearest-x2 + conv3x3 (csrc/conv_up2x_phase.hip): phase 0 folds taps {0} / {1, 2} onto source
    offsets 0 / 1, phase 1 folds {0, 1} / {2}.  Returns [a][b][cout][cin][2][2] in fp64."""
    w = w.astype(np.float64)
    out = np.zeros((2, 2) + w.shape[:2] + (2, 2))
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for s in range(2):
                    out[a, b, :, :, r, s] = w[:, :, _FOLD[a][r]][:, :, :, _FOLD[b][s]].sum(axis=(2, 3))
    return out


def rnd64(v, dtype: str) -> np.ndarray:
    """float64 -> the operand type, ONE round-to-nearest-even (the division by the type's spacing is exact)."""
    v = np.asarray(v, np.float64)
    ulp = typed_ulp(v, dtype)
    out = np.rint(v / ulp) * ulp
    assert np.abs(out).max(initial=0.0) < (65504.0 if dtype == "f16" else 3e38)
    return out


def phase_weights_typed(w, dtype: str, defect: str | None = None):
    wph = phase_weights_ref(w)
    if defect == "phase_rows_swapped":
        wph = wph[::-1]
    if defect == "double_rounded_sum":
        return R.rnd(wph.astype(np.float32), dtype)
    return rnd64(wph, dtype)


def up2x_phase(x, w, b, dtype: str, rows=None, defect: str | None = None):
    """x (h, w, 64) exact typed values, w (64, 64, 3, 3) fp32, b fp32.  Returns lrelu of the four phase convolutions on the output
    rows of SOURCE rows [r0, r1) - (2 (r1 - r0), 2 w, 64) - and its fp32 bound."""
    assert defect is None or defect in DEFECTS_PHASE
    x = np.asarray(x, np.float64)
    h, w_, _ = x.shape
    r0, r1 = _band(h, rows)
    n = r1 - r0
    wt = phase_weights_typed(np.asarray(w), dtype, defect)
    xp = np.zeros((h + 2, w_ + 2, 64))
    xp[1:-1, 1:-1] = x
    ax = np.abs(xp)
    bias = np.asarray(b, np.float64)
    t, A = np.zeros((2 * n, 2 * w_, 64)) + bias, np.zeros((2 * n, 2 * w_, 64)) + np.abs(bias)
    for a in range(2):
        for bb in range(2):
            for r in range(2):
                for s in range(2):
                    sl = (slice(r0 + a + r, r1 + a + r), slice(bb + s, bb + s + w_))
                    t[a::2, bb::2] += xp[sl] @ wt[a, bb, :, :, r, s].T
                    A[a::2, bb::2] += ax[sl] @ np.abs(wt[a, bb, :, :, r, s]).T
    return lrelu(t), gamma(4 * 2 + 1) * A


def up2x_gather(x, w, b, rows=None):
    """The nine-tap form on the repeated pixels: x (h, w, 64) and w (64, 64, 3, 3) exact typed values.  Returns lrelu(t) on the output
    rows of source rows [r0, r1) and the fp32 bound gamma(19) A."""
    x = np.asarray(x, np.float64)
    r0, r1 = _band(x.shape[0], rows)
    t, A = _conv_rows(np.repeat(np.repeat(x, 2, 0), 2, 1), w, b, 2 * r0, 2 * r1)
    return lrelu(t), gamma(9 * 2 + 1) * A


def phase_apriori(x, w, dtype: str, rows=None):
    """How far the phase form (typed sums of the fp32 taps) may sit from the nine-tap form (sums of the typed taps) a priori:
    sum |x| (ulp(sum w) / 2 + sum ulp(w) / 2), ulp of the operand type."""
    x = np.abs(np.asarray(x, np.float64))
    h, w_, _ = x.shape
    r0, r1 = _band(h, rows)
    n = r1 - r0
    w = np.asarray(w, np.float64)
    d = 0.5 * typed_ulp(phase_weights_ref(w), dtype) + phase_weights_ref(0.5 * typed_ulp(w, dtype))
    xp = np.zeros((h + 2, w_ + 2, 64))
    xp[1:-1, 1:-1] = x
    out = np.zeros((2 * n, 2 * w_, 64))
    for a in range(2):
        for bb in range(2):
            for r in range(2):
                for s in range(2):
                    out[a::2, bb::2] += xp[r0 + a + r:r1 + a + r, bb + s:bb + s + w_] @ d[a, bb, :, :, r, s].T
    return out


# ---- seeded inputs shared by the host and the GPU tests --------------------------------------------------------------------------
KINDS = ("scaled", "dc")
# (H, W): whole frame in float64.  One ring tile and one past it; the window kernels' tile and the second tile of
# tiles_y = (H + 16) / 16 that only carries conv_b's trailing row; a partial last tile row and column.
PAIR_WHOLE = [(1, 1), (2, 3), (1, 97), (97, 1), (14, 30), (15, 31), (16, 30), (16, 32), (17, 33), (31, 61), (33, 65), (77, 61)]
PAIR_DC = {(2, 3), (15, 31), (16, 32), (33, 65)}          # the shapes that take the "dc" inputs
PAIR_WARM = (80, 90)                                       # 18 tiles on 18 workgroups, na 1 / 3 / 7, f16
PAIR_LARGE = (320, 390)                                    # 273 / 273 / 299 tiles on 256 workgroups
# three bands of 20 rows: the top, the rows around the seam of tile rows 9 | 10 (160; the ring kernel's 11 | 12 at 154 lies inside),
# the bottom
PAIR_LARGE_BANDS = [(0, 20), (150, 170), (300, 320)]


def pair_cases():
    """(dtype, na, H, W, kind, bands) of tests/test_conv_pair_gpu.py::test_pair_kernels_against_float64."""
    out = []
    for dtype in ("f16", "bf16"):
        for na in (2, 4):
            out += [(dtype, na, H, W, "dc" if (H, W) in PAIR_DC else "scaled", None) for H, W in PAIR_WHOLE]
            out.append((dtype, na, *PAIR_LARGE, "dc" if na == 4 else "scaled", tuple(PAIR_LARGE_BANDS)))
    out += [("f16", na, *PAIR_WARM, "dc" if na == 3 else "scaled", None) for na in (1, 3, 7)]
    return out


def _acts(rng, H, W, c, kind):
    n = rng.standard_normal((H, W, c))
    if kind == "dc":
        return 64.0 + n                                               # the cancellation case
    return n * np.exp(rng.standard_normal((H, W, 1)))                  # per-pixel log-normal scales, all channels live


def pair_inputs(H: int, W: int, na: int, dtype: str, kind: str = "scaled"):
    """Typed x (H, W, 32 na) as uint16 bits, fp32 weights wa (32, 32 na, 3, 3) / wb (32, 32 na + 32, 3, 3) that are already exact
    typed values (the packer's rounding is the identity), fp32 biases whose outputs straddle zero, and x's exact values."""
    rng = np.random.default_rng([H, W, na, KINDS.index(kind), 41])
    cin = 32 * na
    xb = to_bits(_acts(rng, H, W, cin, kind), dtype).reshape(H, W, cin)
    wa = R.rnd(rng.standard_normal((32, cin, 3, 3)) / np.sqrt(9 * cin), dtype).astype(np.float32)
    wb = R.rnd(rng.standard_normal((32, cin + 32, 3, 3)) / np.sqrt(9 * (cin + 32)), dtype).astype(np.float32)
    ba, bb = (0.3 * rng.standard_normal(32)).astype(np.float32), (0.3 * rng.standard_normal(32)).astype(np.float32)
    return xb, wa, ba, wb, bb, from_bits(xb, dtype).reshape(H, W, cin)


UP_WHOLE = [(1, 1), (5, 3), (16, 32), (17, 33), (33, 65)]
UP_DC = {(5, 3), (17, 33)}
UP_LARGE = (368, 736)                                      # 529 source tiles: two or three per workgroup
UP_LARGE_BANDS = [(0, 8), (172, 180), (360, 368)]          # source rows: the top, around the seam of tile rows 10 | 11 (176), the bottom
GATHER_SHAPES = [(1, 1), (5, 3), (13, 21), (17, 33)]


def up_cases():
    out = [(dtype, h, w, "dc" if (h, w) in UP_DC else "scaled", None) for dtype in ("f16", "bf16") for h, w in UP_WHOLE]
    return out + [(dtype, *UP_LARGE, "scaled", tuple(UP_LARGE_BANDS)) for dtype in ("f16", "bf16")]


def up_inputs(h: int, w_: int, dtype: str, kind: str = "scaled"):
    """Typed x (h, w, 64) as uint16 bits, fp32 weights (64, 64, 3, 3) as a checkpoint holds them - NOT typed: the phase packer sums
    them before it rounds -, an fp32 bias, and x's exact values."""
    rng = np.random.default_rng([h, w_, KINDS.index(kind), 43])
    xb = to_bits(_acts(rng, h, w_, 64, kind), dtype).reshape(h, w_, 64)
    w = (rng.standard_normal((64, 64, 3, 3)) / np.sqrt(9 * 64)).astype(np.float32)
    b = (0.3 * rng.standard_normal(64)).astype(np.float32)
    return xb, w, b, from_bits(xb, dtype).reshape(h, w_, 64)
