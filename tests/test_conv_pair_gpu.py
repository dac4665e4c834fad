"""The three fused conv-pair kernels (csrc/conv3x3_pair.hip, conv3x3_pair_slide.hip, conv3x3_pair_slide32.hip), the phase kernel
(csrc/conv_up2x_phase.hip) and the gather form of the up-conv (fw_conv3x3_nhwc, upsample2x = 1), each held on its own to the
float64 restatements and per-element bounds of tests/conv_pair_ref.py through the C-ABI, in f16 and bf16, on inputs with the
dynamic range of a trunk and with a DC offset.  x_b is held to conv_b of the kernel's OWN stored x_a.  Every layout the header
documents is run: chunk-planar in place as the engine runs it (the outputs are the next two planes of the buffer that is being
read), and interleaved input with a wide output.  Every buffer is guarded on both sides and pre-filled with a pattern that is a NaN
in both types: nothing but the outputs may change, and the outputs must be written everywhere."""
import ctypes as C
import functools
import hashlib
import time

import numpy as np
import pytest
import torch

from framewright_amd import _lib
import conv_epilogue_ref as R
import conv_pair_ref as P
from guarded import Guarded, dev, dtype_id, f32, ptr, stream

pytestmark = pytest.mark.gpu

SENT = 0x7FC1          # a NaN of f16 and of bf16
GUARD = 4096           # guard elements on both sides of every buffer
SLIDES = {"0": "ring", "1": "window", "2": "window32"}


class Buf:
    """An int16 device buffer [GUARD | n | GUARD], all of it the sentinel until ``fill``."""

    def __init__(self, n: int):
        self.n = int(n)
        self.t = torch.full((GUARD + self.n + GUARD,), int(np.array([SENT], np.uint16).view(np.int16)[0]), dtype=torch.int16, device="cuda")

    def ptr(self, elem_offset: int = 0):
        return C.c_void_p(self.t.data_ptr() + 2 * (GUARD + elem_offset))

    def fill(self, bits: np.ndarray, elem_offset: int = 0):
        flat = dev(np.ascontiguousarray(bits, np.uint16).reshape(-1))
        self.t[GUARD + elem_offset:GUARD + elem_offset + flat.numel()] = flat

    def take(self) -> np.ndarray:
        a = self.t.cpu().numpy().view(np.uint16)
        for name, g in (("front", a[:GUARD]), ("back", a[GUARD + self.n:])):
            bad = np.flatnonzero(g != SENT)
            assert bad.size == 0, f"{bad.size} elements of the {name} guard were written, first at {bad[:4]}"
        return a[GUARD:GUARD + self.n]


def _finite(bits: np.ndarray, dtype: str) -> bool:
    """No Inf, no NaN - the sentinel among them: every element was written."""
    mask = 0x7C00 if dtype == "f16" else 0x7F80
    return bool(((bits & mask) != mask).all())


def _pack(lib, dtype, w, ct, ch):
    cout, cin = w.shape[:2]
    n = lib.fw_pack_conv3x3(dtype_id(dtype), None, cout, cin, ct, ch, None)
    dst = np.zeros(n, np.uint16)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.fw_pack_conv3x3(dtype_id(dtype), C.c_void_p(wc.ctypes.data), cout, cin, ct, ch, C.c_void_p(dst.ctypes.data)) == n
    return dev(dst)


def _pack_phase(lib, dtype, w):
    n = lib.fw_pack_conv_up2x_phase(dtype_id(dtype), None, None)
    dst = np.zeros(n, np.uint16)
    wc = np.ascontiguousarray(w, np.float32)
    assert lib.fw_pack_conv_up2x_phase(dtype_id(dtype), C.c_void_p(wc.ctypes.data), C.c_void_p(dst.ctypes.data)) == n
    return dev(dst)


def _spare(shape, dtype, seed):
    """Live typed values for the channels a kernel has to leave alone."""
    return P.to_bits(np.random.default_rng(seed).standard_normal(shape) * 8, dtype).reshape(shape)


# ---- the fused pair --------------------------------------------------------------------------------------------------------------
class _Problem:
    """One case: its inputs, the float64 x_a reference per band, and the x_b references by the x_a bytes they were computed from."""

    def __init__(self, case):
        self.dtype, self.na, self.H, self.W, self.kind, bands = case
        self.xb, self.wa, self.ba, self.wb, self.bb, self.xv = P.pair_inputs(self.H, self.W, self.na, self.dtype, self.kind)
        self.bands = [(0, self.H)] if bands is None else list(bands)
        self.ref_a = [P.pair_a(self.xv, self.wa, self.ba, rows) for rows in self.bands]
        self._ref_b = {}

    def ref_b(self, xa_bits):
        """x_b of THIS x_a (the rows the bands read): computed once per distinct x_a."""
        H = self.H
        read = [xa_bits[max(r0 - 1, 0):min(r1 + 1, H)] for r0, r1 in self.bands]
        key = hashlib.sha1(b"".join(r.tobytes() for r in read)).digest()
        if key not in self._ref_b:
            xa = np.zeros((H, self.W, 32))
            for (r0, r1), r in zip(self.bands, read):
                xa[max(r0 - 1, 0):min(r1 + 1, H)] = P.from_bits(r, self.dtype).reshape(r.shape)
            self._ref_b[key] = [P.pair_b(self.xv, xa, self.wb, self.bb, rows)[:2] for rows in self.bands]
        return self._ref_b[key]


@functools.lru_cache(maxsize=1)      # one reference per case, shared by the three kernels and both layouts; the frames are large
def _problem(case):
    return _Problem(case)


def _run_pair(lib, pr, wpa, wpb, ba, bb, layout):
    """One launch; returns the stored x_a and x_b (H, W, 32) uint16 after the checks on everything that must not change."""
    H, W, na, dt = pr.H, pr.W, pr.na, dtype_id(pr.dtype)
    hw = H * W
    if layout == "inplace":          # [GUARD | na + 2 planes of H W 32 | GUARD]: the engine's dense-block buffer
        buf = Buf((na + 2) * hw * 32)
        planes = np.ascontiguousarray(pr.xb.reshape(hw, na, 32).transpose(1, 0, 2))
        buf.fill(planes)
        _lib.check(lib.fw_conv3x3_pair_nhwc(dt, buf.ptr(), 32, hw * 32, na, H, W, ptr(wpa), ptr(ba), ptr(wpb), ptr(bb),
                                            buf.ptr(na * hw * 32), buf.ptr((na + 1) * hw * 32), 32, stream()))
        torch.cuda.synchronize()
        body = buf.take().reshape(na + 2, hw, 32)
        assert np.array_equal(body[:na], planes), "the input planes were written"
        oa, ob = body[na].reshape(H, W, 32), body[na + 1].reshape(H, W, 32)
    else:                            # interleaved input with eight spare channels, outputs = channels [8, 40) and [48, 80) of 96
        cs = 32 * na + 8
        xin = np.concatenate([pr.xb, _spare((H, W, 8), pr.dtype, 1)], 2)
        src, out = Buf(hw * cs), Buf(hw * 96)
        src.fill(xin)
        _lib.check(lib.fw_conv3x3_pair_nhwc(dt, src.ptr(), cs, 0, na, H, W, ptr(wpa), ptr(ba), ptr(wpb), ptr(bb), out.ptr(8), out.ptr(48),
                                            96, stream()))
        torch.cuda.synchronize()
        assert np.array_equal(src.take(), xin.reshape(-1)), "the input was written"
        v = out.take().reshape(H, W, 96)
        oa, ob = v[:, :, 8:40], v[:, :, 48:80]
        rest = np.concatenate([v[:, :, :8], v[:, :, 40:48], v[:, :, 80:]], 2)
        assert (rest == SENT).all(), f"{int((rest != SENT).sum())} elements outside the two 32-channel slices were written"
    assert _finite(oa, pr.dtype) and _finite(ob, pr.dtype), "an output element is not finite or was never written"
    return oa.copy(), ob.copy()


PAIR_CASES = P.pair_cases()


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: f"{c[0]}-na{c[1]}-{c[2]}x{c[3]}-{c[4]}")
def test_pair_kernels_against_float64(hip_lib, case, monkeypatch):
    t0 = time.time()
    pr = _problem(case)
    wpa, wpb = _pack(hip_lib, pr.dtype, pr.wa, 1, pr.na), _pack(hip_lib, pr.dtype, pr.wb, 1, pr.na + 1)
    ba, bb = dev(pr.ba), dev(pr.bb)
    got = {}
    for layout in ("inplace", "interleaved"):
        for slide in SLIDES:
            monkeypatch.setenv("FW_PAIR_SLIDE", slide)
            got[layout, slide] = _run_pair(hip_lib, pr, wpa, wpb, ba, bb, layout)
    t_gpu = time.time() - t0
    worst = {}
    for (layout, slide), (oa, ob) in got.items():
        ref_b = pr.ref_b(oa)
        ra = rb = 0.0
        for (r0, r1), (ya, bound_a), (yb, bound_b) in zip(pr.bands, pr.ref_a, ref_b):
            ea = np.abs(P.from_bits(oa[r0:r1], pr.dtype).reshape(ya.shape) - ya) / P.typed_allowance(ya, bound_a, pr.dtype)
            eb = np.abs(P.from_bits(ob[r0:r1], pr.dtype).reshape(yb.shape) - yb) / P.typed_allowance(yb, bound_b, pr.dtype)
            ra, rb = max(ra, float(ea.max())), max(rb, float(eb.max()))
        worst[layout, slide] = (ra, rb)
    print(f"\npair {pr.H}x{pr.W} na {pr.na} {pr.kind} {pr.dtype}: max |err| / allowance x_a / x_b: "
          + "; ".join(f"{SLIDES[s]} {l} {a:.3f} / {b:.3f}" for (l, s), (a, b) in worst.items())
          + f"  ({len(pr._ref_b)} x_b reference(s), gpu {t_gpu:.1f} s, total {time.time() - t0:.1f} s)")
    for key, (ra, rb) in worst.items():
        assert ra <= 1.0, (key, "x_a", ra)
        assert rb <= 1.0, (key, "x_b", rb)
    # the three kernels accumulate every output in the same order: the same bytes, in either layout
    for key, (oa, ob) in got.items():
        assert np.array_equal(oa, got["inplace", "0"][0]), (key, "x_a differs from the ring kernel's")
        assert np.array_equal(ob, got["inplace", "0"][1]), (key, "x_b differs from the ring kernel's")


# ---- the up-conv -----------------------------------------------------------------------------------------------------------------
def _run_phase(lib, dtype, xb, wp, bias, layout):
    """One launch of the phase kernel; returns the typed output (2 h, 2 w, 64) uint16 after the checks on what must not change."""
    h, w_, _ = xb.shape
    dt, hw = dtype_id(dtype), h * w_
    if layout == "planar":           # two 32-channel planes in, two out: the RRDBNet tail's layout
        planes = np.ascontiguousarray(xb.reshape(hw, 2, 32).transpose(1, 0, 2))
        src, out = Buf(2 * hw * 32), Buf(2 * 4 * hw * 32)
        src.fill(planes)
        _lib.check(lib.fw_conv_up2x_phase_nhwc(dt, src.ptr(), 32, hw * 32, h, w_, ptr(wp), ptr(bias), 1, out.ptr(), 32, 4 * hw * 32, stream()))
        torch.cuda.synchronize()
        assert np.array_equal(src.take(), planes.reshape(-1)), "the input planes were written"
        got = out.take().reshape(2, 4 * hw, 32).transpose(1, 0, 2).reshape(2 * h, 2 * w_, 64)
    else:                            # 64 + 8 channels per pixel in, channels [8, 72) of 80 out
        xin = np.concatenate([xb, _spare((h, w_, 8), dtype, 2)], 2)
        src, out = Buf(hw * 72), Buf(4 * hw * 80)
        src.fill(xin)
        _lib.check(lib.fw_conv_up2x_phase_nhwc(dt, src.ptr(), 72, 0, h, w_, ptr(wp), ptr(bias), 1, out.ptr(8), 80, 0, stream()))
        torch.cuda.synchronize()
        assert np.array_equal(src.take(), xin.reshape(-1)), "the input was written"
        v = out.take().reshape(2 * h, 2 * w_, 80)
        assert (v[:, :, :8] == SENT).all() and (v[:, :, 72:] == SENT).all(), "channels outside [8, 72) were written"
        got = v[:, :, 8:72]
    assert _finite(got, dtype), "an output element is not finite or was never written"
    return np.ascontiguousarray(got)


UP_CASES = P.up_cases()


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_up2x_phase_against_float64(hip_lib, case):
    dtype, h, w_, kind, bands = case
    xb, w32, b, xv = P.up_inputs(h, w_, dtype, kind)
    wp, bias = _pack_phase(hip_lib, dtype, w32), dev(b)
    got = {layout: _run_phase(hip_lib, dtype, xb, wp, bias, layout) for layout in ("planar", "interleaved")}
    worst = {layout: 0.0 for layout in got}
    for r0, r1 in ([(0, h)] if bands is None else bands):
        ref, bound = P.up2x_phase(xv, w32, b, dtype, (r0, r1))
        allow = P.typed_allowance(ref, bound, dtype)
        for layout, o in got.items():
            err = np.abs(P.from_bits(o[2 * r0:2 * r1], dtype).reshape(ref.shape) - ref)
            worst[layout] = max(worst[layout], float((err / allow).max()))
    print(f"\nphase {h}x{w_} {kind} {dtype}: max |err| / allowance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.array_equal(got["planar"], got["interleaved"])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("h,w_", P.GATHER_SHAPES)
def test_up2x_gather_against_float64(hip_lib, dtype, h, w_):
    """fw_conv3x3_nhwc(upsample2x = 1): the fp32 output within gamma(19) A of the nine-tap form on the repeated pixels, the typed
    output its RNE; and the phase kernel within the two bounds plus the a-priori weight-rounding distance of it."""
    xb, w32, b, xv = P.up_inputs(h, w_, dtype, "dc" if (h, w_) in P.UP_DC else "scaled")
    bias = dev(b)
    src, out, o32 = Buf(h * w_ * 64), Buf(4 * h * w_ * 64), Guarded(4 * h * w_ * 64, "f32")
    src.fill(xb)
    _lib.check(hip_lib.fw_conv3x3_nhwc(dtype_id(dtype), src.ptr(), 64, 0, 2, 2 * h, 2 * w_, ptr(_pack(hip_lib, dtype, w32, 2, 2)), ptr(bias), 2, 1, 1,
                                       None, 1.0, None, 1.0, out.ptr(), 64, 0, 0, o32.ptr(), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(src.take(), xb.reshape(-1))
    got32 = f32(o32.take()).reshape(2 * h, 2 * w_, 64)
    ref_g, bound_g = P.up2x_gather(xv, R.rnd(w32, dtype), b)
    err = np.abs(got32.astype(np.float64) - ref_g)
    print(f"\ngather {h}x{w_} {dtype}: max |err| / bound {float((err / bound_g).max()):.3f}")
    assert np.isfinite(got32).all() and (err <= bound_g).all()
    np.testing.assert_array_equal(out.take().reshape(got32.shape), P.to_bits(got32, dtype).reshape(got32.shape))
    # phase against gather
    ph = P.from_bits(_run_phase(hip_lib, dtype, xb, _pack_phase(hip_lib, dtype, w32), bias, "planar"), dtype).reshape(got32.shape)
    ref_p, bound_p = P.up2x_phase(xv, w32, b, dtype)
    gap = np.abs(ph - got32.astype(np.float64))
    allow = P.typed_allowance(ref_p, bound_p, dtype) + bound_g + P.phase_apriori(xv, w32, dtype)
    print(f"phase vs gather {h}x{w_} {dtype}: max gap {gap.max():.3g}, gap / allowance {float((gap / allow).max()):.3f}")
    assert (gap <= allow).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_pair_rejects_bad_arguments(hip_lib):
    """FW_ERR_INVALID with a message and nothing launched.  Every refused call is built from valid buffers that are large enough for
    what the call describes, so a check that failed to fire could only compute garbage."""
    H, W, na = 6, 10, 2
    hw = H * W
    x = torch.zeros(12 * hw * 40, dtype=torch.int16, device="cuda")        # 12 planes of H W 40: every stride below stays inside
    w = torch.zeros(10 * 9 * 2 * 64 * 8, dtype=torch.int16, device="cuda")  # packed weights of up to 10 chunks
    bias = torch.zeros(32, dtype=torch.float32, device="cuda")
    out = Buf(2 * hw * 96)
    ok = dict(dtype=_lib.FW_DTYPE_F16, x=ptr(x), in_cstride=32, in_pstride=hw * 32, na=na, H=H, W=W, wa=ptr(w), ba=ptr(bias), wb=ptr(w),
              bb=ptr(bias), oa=out.ptr(), ob=out.ptr(hw * 96), out_cstride=32)

    def call(**kv):
        a = dict(ok, **kv)
        return hip_lib.fw_conv3x3_pair_nhwc(a["dtype"], a["x"], a["in_cstride"], a["in_pstride"], a["na"], a["H"], a["W"], a["wa"], a["ba"],
                                            a["wb"], a["bb"], a["oa"], a["ob"], a["out_cstride"], stream())

    bad = [dict(na=0), dict(na=9), dict(in_cstride=24), dict(in_cstride=36), dict(out_cstride=24), dict(out_cstride=36),
           dict(in_pstride=hw * 32 + 4), dict(in_pstride=0, in_cstride=32), dict(in_pstride=0, in_cstride=56, na=2),
           dict(x=None), dict(wa=None), dict(ba=None), dict(wb=None), dict(bb=None), dict(oa=None), dict(ob=None),
           dict(dtype=2), dict(dtype=-1), dict(H=0), dict(W=0)]
    for kv in bad:
        st = call(**kv)
        msg = hip_lib.fw_last_error().decode()
        assert st == _lib.FW_ERR_INVALID and msg, (kv, st, msg)
    torch.cuda.synchronize()
    assert (out.take() == SENT).all(), "a refused call wrote to its outputs"
    # the call they were all derived from is a valid one
    assert call() == _lib.FW_OK
    assert call(in_pstride=0, in_cstride=64) == _lib.FW_OK
    torch.cuda.synchronize()
    v = out.take()
    assert _finite(v[:hw * 32], "f16") and _finite(v[hw * 96:hw * 96 + hw * 32], "f16") and (v[hw * 32:hw * 96] == SENT).all()
