"""Host side of tests/conv_pair_ref.py: the restatements are pinned to torch in float64 (F.leaky_relu(F.conv2d) chained through the
typed x_a; F.conv2d(F.interpolate(nearest)) for both forms of the up-conv), every listed defect, computed exactly, leaves the typed
allowance of the GPU tests by at least 100x at some element and at no less than 1 % of the elements it touches, on every input set
those tests use, and the input sets are what they claim to be.

What stays below the 100x is said so where it is asserted: the two bias-sized defects (``xa_outside_bias``, ``bias_b_n16``) on the
"dc" input sets, and ``double_rounded_sum``, which a typed output hides at all but a few elements per thousand (test_double_rounded_sum)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R
import conv_pair_ref as P

DTYPES = ["f16", "bf16"]


def _t(a):
    """(H, W, C) -> (1, C, H, W) float64 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(2, 0, 1)[None]


def _hwc(t):
    return t[0].permute(1, 2, 0).numpy()


def _conv(x, w, b):
    return F.leaky_relu(F.conv2d(_t(x), torch.from_numpy(np.asarray(w, np.float64)), torch.from_numpy(np.asarray(b, np.float64)), 1, 1), P.S)


def _bands(H, bands):
    return [(0, H)] if bands is None else list(bands)


def _host_xa_bits(xv, wa, ba, dtype, bands):
    """The reference's own typed x_a on the rows conv_b of ``bands`` reads (two rows around each: "xa_row_lag" looks one row further)."""
    H, W, _ = xv.shape
    bits = np.zeros((H, W, 32), np.uint16)
    for r0, r1 in _bands(H, bands):
        lo, hi = max(r0 - 2, 0), min(r1 + 2, H)
        bits[lo:hi] = P.to_bits(P.pair_a(xv, wa, ba, (lo, hi))[0], dtype).reshape(hi - lo, W, 32)
    return bits


def test_the_activation_constant_is_fp32s():
    assert P.S == float(np.float32(0.2)) and abs(P.S - 0.2) <= 2.0 ** -26 * 0.2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,H,W,kind", [(1, 1, 1, "scaled"), (2, 5, 3, "dc"), (3, 17, 33, "scaled"), (2, 33, 35, "dc")])
def test_pair_is_torchs_chained_convs(dtype, na, H, W, kind):
    xb, wa, ba, wb, bb, xv = P.pair_inputs(H, W, na, dtype, kind)
    assert np.array_equal(R.rnd(wa, dtype), wa) and np.array_equal(R.rnd(wb, dtype), wb)     # the packer's rounding is the identity
    want_a = _hwc(_conv(xv, wa, ba))
    xa_bits = P.to_bits(want_a, dtype).reshape(H, W, 32)
    ref_a, bound_a, ref_b, bound_b, touched = P.pair(xv, wa, ba, wb, bb, xa_bits, dtype)
    xa = P.from_bits(xa_bits, dtype).reshape(H, W, 32)
    want_b = _hwc(_conv(np.concatenate([xv, xa], 2), wb, bb))
    assert np.abs(ref_a - want_a).max() <= 1e-13 * np.abs(want_a).max()
    assert np.abs(ref_b - want_b).max() <= 1e-13 * np.abs(want_b).max()
    assert (bound_a > 0).all() and (bound_b > 0).all() and touched.all()
    assert (bound_a >= P.gamma(9 * na + 1) * np.abs(want_a) - 1e-18).all()                   # A >= |t|
    # a band is the same rows of the whole frame
    if H > 4:
        rows = (H // 3, H - 2)
        band = P.pair(xv, wa, ba, wb, bb, xa_bits, dtype, rows=rows)
        for whole, part in zip((ref_a, bound_a, ref_b, bound_b), band):
            assert np.abs(whole[rows[0]:rows[1]] - part).max() <= 1e-13 * np.abs(whole).max()


def _dyadic_weights(seed):
    """Multiples of 1 / 64 of at most 8 / 64: every fold of up to four of them is exact in f16 and in bf16."""
    return (np.random.default_rng(seed).integers(-8, 9, (64, 64, 3, 3)) / 64.0).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w_,kind", [(1, 1, "scaled"), (5, 3, "dc"), (13, 21, "scaled")])
def test_up2x_forms_are_torchs_conv_of_the_nearest_upsampling(dtype, h, w_, kind):
    _, w32, b, xv = P.up_inputs(h, w_, dtype, kind)

    def torch_form(w):
        return _hwc(F.leaky_relu(F.conv2d(F.interpolate(_t(xv), scale_factor=2, mode="nearest"), torch.from_numpy(w.astype(np.float64)),
                                          torch.from_numpy(b.astype(np.float64)), 1, 1), P.S))

    wt = R.rnd(w32, dtype)
    ref_g, bound_g = P.up2x_gather(xv, wt, b)
    want = torch_form(wt)
    assert ref_g.shape == (2 * h, 2 * w_, 64) and np.abs(ref_g - want).max() <= 1e-13 * np.abs(want).max() and (bound_g > 0).all()
    # with weights whose folds are exact the phase form IS the nine-tap form
    wd = _dyadic_weights(h + w_)
    assert np.array_equal(P.phase_weights_typed(wd, dtype), P.phase_weights_ref(wd))
    ref_p, bound_p = P.up2x_phase(xv, wd, b, dtype)
    want = torch_form(wd)
    assert np.abs(ref_p - want).max() <= 1e-13 * np.abs(want).max() and (bound_p > 0).all()
    # with a checkpoint's weights it stays within the a-priori weight-rounding distance of the nine-tap form of the typed taps
    ref_p, _ = P.up2x_phase(xv, w32, b, dtype)
    apr = P.phase_apriori(xv, w32, dtype)
    gap = np.abs(ref_p - ref_g)
    print(f"phase vs nine-tap {h}x{w_} {kind} {dtype}: max gap {gap.max():.3g}, gap / a-priori {float((gap / apr).max()):.3f}")
    assert (gap <= apr * (1 + 1e-12)).all() and gap.max() > 0
    if h > 4:
        rows = (1, h - 1)
        for whole, part in ((ref_p, P.up2x_phase(xv, w32, b, dtype, rows=rows)[0]), (ref_g, P.up2x_gather(xv, wt, b, rows=rows)[0]),
                            (apr, P.phase_apriori(xv, w32, dtype, rows=rows))):
            assert np.abs(whole[2 * rows[0]:2 * rows[1]] - part).max() <= 1e-13 * np.abs(whole).max()


def test_rnd64_rounds_once():
    """One RNE from float64: equal to numpy's own float64 -> float16 cast, and to the fp32 route wherever fp32 holds the value."""
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(20000) * np.exp(3 * rng.standard_normal(20000)), [0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                                                                                              1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11]])
    v = v[np.abs(v) < 60000]
    assert np.array_equal(P.rnd64(v, "f16"), v.astype(np.float16).astype(np.float64))
    v32 = v.astype(np.float32)
    for dtype in DTYPES:
        assert np.array_equal(P.rnd64(v32.astype(np.float64), dtype), R.rnd(v32, dtype))
    # the double rounding the defect "double_rounded_sum" stands for: just above a tie, fp32 rounds onto the tie, RNE then goes down
    x = 1 + 2.0 ** -11 + 2.0 ** -30
    assert P.rnd64(x, "f16") == 1 + 2.0 ** -10 and R.rnd(np.float32(x), "f16") == 1.0


# ---- the packed weights ----------------------------------------------------------------------------------------------------------
def _phase_layout(wt):
    """[a][b][cout][cin][r][s] in the packer's fragment order (csrc/conv_up2x_phase.hip: [a][chunk][step (tx, r, b)][tile][lane][j])."""
    steps = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 1), (2, 1, 1)]
    lane = np.arange(64)
    out = np.zeros((2, 2, 8, 4, 64, 8))
    for a in range(2):
        for c in range(2):
            for s, (tx, r, b) in enumerate(steps):
                for w in range(4):
                    for j in range(8):
                        out[a, c, s, w, :, j] = wt[a, b, 16 * w + (lane & 15), 32 * c + 8 * (lane >> 4) + j, r, tx - b]
    return out.reshape(-1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_packer_rounds_the_sum_once(hip_lib, dtype):
    """fw_pack_conv_up2x_phase: "sums in fp64, rounded to the operand type once" (include/framewright_hip.h), bit for bit, for the
    weights of every GPU case.  (The packer used to go through fp32: 7 of the 65536 f16 weights of the 16 x 32 case were one ulp off.)"""
    from framewright_amd import _lib
    did = _lib.FW_DTYPE_F16 if dtype == "f16" else _lib.FW_DTYPE_BF16
    twice = 0
    for _, h, w_, kind, _ in [c for c in P.up_cases() if c[0] == dtype]:
        _, w32, _, _ = P.up_inputs(h, w_, dtype, kind)
        n = hip_lib.fw_pack_conv_up2x_phase(did, None, None)
        pk = np.zeros(n, np.uint16)
        assert hip_lib.fw_pack_conv_up2x_phase(did, C.c_void_p(w32.ctypes.data), C.c_void_p(pk.ctypes.data)) == n
        want = P.phase_weights_typed(w32, dtype)
        np.testing.assert_array_equal(P.from_bits(pk, dtype), _phase_layout(want))
        twice += int((P.phase_weights_typed(w32, dtype, "double_rounded_sum") != want).sum())
    print(f"{dtype}: {twice} weights of these sets would differ after a detour through fp32")
    assert twice > 0                                           # the input sets can tell the two apart


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
def _beyond(wrong, ref, bound, dtype, touched):
    """max |wrong - ref| / allowance and the share of the touched elements outside the allowance."""
    r = (np.abs(wrong - ref) / P.typed_allowance(ref, bound, dtype))[touched]
    return float(r.max()), float((r > 1).mean())


PAIR_CASES = P.pair_cases()


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: f"{c[0]}-na{c[1]}-{c[2]}x{c[3]}-{c[4]}")
def test_pair_bounds_reject_defects_and_the_inputs_are_live(case):
    dtype, na, H, W, kind, bands = case
    xb, wa, ba, wb, bb, xv = P.pair_inputs(H, W, na, dtype, kind)
    ax = np.abs(xv)
    assert ax.max() < 65504 and np.isfinite(xv).all() and (xv[:, :, ::32] != 0).any()
    if kind == "scaled":
        if H * W >= 6:
            assert ax.max() >= 2.0 ** 8 * ax[ax > 0].min()                        # the dynamic range a trunk sees
    else:
        assert ax.min() > 32 and ax.max() < 128                                   # the offset dominates: cancellation
    xa_bits = _host_xa_bits(xv, wa, ba, dtype, bands)
    xa = P.from_bits(xa_bits, dtype).reshape(H, W, 32)
    ring = R.rnd(P.lrelu(ba.astype(np.float64)), dtype)
    worst = {d: [0.0, 0, 0] for d in P.DEFECTS_PAIR}                               # ratio, elements outside, elements touched
    sign = [False, False]
    for rows in _bands(H, bands):
        ref_a, bound_a = P.pair_a(xv, wa, ba, rows)
        pre = P.pair_b_pre(xv, xa, wb, bb, rows)
        ref_b, bound_b, _ = P.pair_b(xv, xa, wb, bb, rows, pre=pre)
        for ref in (ref_a, ref_b):
            assert np.abs(ref).max() < 65504 / 2
            sign = [sign[0] or bool((ref > 0).any()), sign[1] or bool((ref < 0).any())]
        # the reference's own typed x_a is inside its own allowance
        assert (np.abs(xa[rows[0]:rows[1]] - ref_a) <= P.typed_allowance(ref_a, bound_a, dtype)).all()
        for d in P.DEFECTS_PAIR:
            wrong, _, touched = P.pair_b(xv, xa, wb, bb, rows, d, ring=ring, pre=pre)
            assert np.array_equal(wrong[~touched], ref_b[~touched])
            if touched.any():
                ratio, share = _beyond(wrong, ref_b, bound_b, dtype, touched)
                n = int(touched.sum())
                worst[d] = [max(worst[d][0], ratio), worst[d][1] + round(share * n), worst[d][2] + n]
    assert all(sign)                                                              # outputs of both signs
    for d, (ratio, out, n) in worst.items():
        if n == 0:
            assert d == "xa_seam_tap" and W <= 30 or d == "lrelu_missing_b" and H * W == 1, d   # nothing for the defect to touch
            continue
        print(f"pair {H}x{W} na {na} {kind} {dtype} {d}: {ratio:.0f} x the allowance, {100.0 * out / n:.1f} % of {n} touched elements outside")
        assert out >= 0.01 * n, d
        # What cannot reach 100x: the two defects whose size is set by the biases (0.3 whatever the input: the ring of
        # "xa_outside_bias" holds lrelu(bias_a) and moves x_b by about 0.15, "bias_b_n16" by about 0.4) on the "dc" sets, whose
        # outputs are of size 64 |sum w|: half an ulp of the output type at 64 alone is 2^-5 in f16 and 2^-2 in bf16.  There they
        # still leave the allowance (by 17x to 175x) at far more than 1 % of the elements they touch, which is what fails the GPU
        # test; on the "scaled" sets they are held to the 100x like every other defect.
        assert ratio >= (1 if d in ("xa_outside_bias", "bias_b_n16") and kind == "dc" else 100), d


UP_CASES = P.up_cases()


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_phase_bound_rejects_swapped_row_phases_and_the_inputs_are_live(case):
    dtype, h, w_, kind, bands = case
    xb, w32, b, xv = P.up_inputs(h, w_, dtype, kind)
    ax = np.abs(xv)
    assert ax.max() < 65504
    if kind == "scaled":
        assert ax.max() >= 2.0 ** 8 * ax[ax > 0].min() or h * w_ < 6
    else:
        assert ax.min() > 32 and ax.max() < 128
    worst, out, n = 0.0, 0, 0
    for rows in _bands(h, bands):
        ref, bound = P.up2x_phase(xv, w32, b, dtype, rows)
        assert np.abs(ref).max() < 65504 / 2 and (ref > 0).any() and (ref < 0).any()
        wrong, _ = P.up2x_phase(xv, w32, b, dtype, rows, "phase_rows_swapped")
        ratio, share = _beyond(wrong, ref, bound, dtype, np.ones(ref.shape, bool))
        worst, out, n = max(worst, ratio), out + round(share * ref.size), n + ref.size
    print(f"phase {h}x{w_} {kind} {dtype} phase_rows_swapped: {worst:.0f} x the allowance, {100.0 * out / n:.1f} % of {n} elements outside")
    assert worst >= 100 and out >= 0.01 * n


def test_double_rounded_sum():
    """The summed weight rounded to fp32 first, then to the type.  It moves a weight by one ulp of the operand type where the fp32
    rounding lands on a tie of the type: a handful of the 65536 weights in f16, fewer in bf16, none for some sets.  That is NOT
    invisible in a typed output: where a moved weight meets a large input and a small output it leaves the allowance (by 54x at
    368 x 736 in f16, 15x at 16 x 32, 2x at 5 x 3 in bf16), so the GPU test fails on it, as it did on the packer before it rounded
    once.  It does so at a few elements per thousand only, below the 1 % (and the 100x) that the other defects are held to, and
    not on every input set; so it is pinned where it happens, bit for bit: test_phase_packer_rounds_the_sum_once."""
    seen = 0.0
    for dtype, h, w_, kind, bands in UP_CASES:
        xb, w32, b, xv = P.up_inputs(h, w_, dtype, kind)
        moved = int((P.phase_weights_typed(w32, dtype, "double_rounded_sum") != P.phase_weights_typed(w32, dtype)).sum())
        worst, share = 0.0, 0.0
        for rows in _bands(h, bands) if moved else []:
            ref, bound = P.up2x_phase(xv, w32, b, dtype, rows)
            wrong, _ = P.up2x_phase(xv, w32, b, dtype, rows, "double_rounded_sum")
            ratio, s = _beyond(wrong, ref, bound, dtype, np.ones(ref.shape, bool))
            worst, share = max(worst, ratio), max(share, s)
        print(f"phase {h}x{w_} {kind} {dtype} double_rounded_sum: {moved} weights moved, {worst:.2f} x the allowance, "
              f"at most {100.0 * share:.3f} % of a band's elements outside")
        assert share < 0.01                                                       # never by the measure of the other defects
        seen = max(seen, worst)
    assert seen > 1                                                               # but the GPU test does see it
