"""Every kernel of csrc/ifnet_ops.hip that IFNet uses, run on its own through the C-ABI against the float64 references and per-element
bounds of tests/ifnet_glue_ref.py (pinned to torch in float64 by tests/test_ifnet_glue_ref_host.py; parity vs upstream unpinned).
``err <= bound`` is asserted per element and the largest err / bound printed.  Output buffers are filled with a sentinel and guarded
on both sides; channels and pixels a kernel must not touch (dst_coff, the padding behind 4 C, everything outside the crop) must
still hold the sentinel or the zero the contract names.  Shapes: 32 x 32 (one tile of the fused input kernel at s = 8), 64 x 96, the
padded 1080p frame 1088 x 1920 (second trip of the 4096 x 256 grid-stride loops) and 2176 x 3840 at s = 1 (above the fused input
kernel's cap of 8192 workgroups); frames above 2^18 pixels are checked on a seeded sample of rows plus their outermost rows and
columns (ifnet_glue_ref.sample_points), the fused forms against the separate kernels on the whole frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import ifnet_glue_ref as G
from framewright_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = {np.dtype(np.float32): 0x7FC5A5A5, np.dtype(np.uint16): 0x7E5A, np.dtype(np.uint8): 0xA5}     # NaN patterns (fp32, f16 / bf16)
_TORCH = {np.dtype(np.float32): torch.int32, np.dtype(np.uint16): torch.int16, np.dtype(np.uint8): torch.uint8}
_VIEW = {np.dtype(np.float32): np.uint32, np.dtype(np.uint16): np.uint16, np.dtype(np.uint8): np.uint8}
DT = {"f16": _lib.FW_DTYPE_F16, "bf16": _lib.FW_DTYPE_BF16}
SHAPES = [(32, 32), (64, 96), (1088, 1920)]


def _sent(dt):
    s = SENT[np.dtype(dt)]
    return s - (1 << 32) if np.dtype(dt) == np.float32 and s >= 1 << 31 else s


class Out:
    """A device buffer of `shape`, sentinel-filled, with GUARD elements of sentinel in front of it and behind it."""

    def __init__(self, shape, dt, init=None):
        self.shape, self.dt = tuple(shape), np.dtype(dt)
        self.n = int(np.prod(self.shape))
        self.dev = torch.full((GUARD + self.n + GUARD,), _sent(dt), dtype=_TORCH[self.dt], device="cuda")
        if init is not None:
            signed = {4: np.int32, 2: np.int16, 1: np.uint8}[self.dt.itemsize]
            self.dev[GUARD:GUARD + self.n] = torch.from_numpy(np.ascontiguousarray(init, dt).reshape(-1).view(signed)).cuda()

    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + GUARD * self.dt.itemsize)

    def take(self):
        """What the kernel left in the buffer (bit patterns as `dt`); the guards must be untouched."""
        torch.cuda.synchronize()
        a = self.dev.cpu().numpy().view(_VIEW[self.dt])
        s = SENT[self.dt]
        for g in (a[:GUARD], a[GUARD + self.n:]):
            bad = np.flatnonzero(g != s)
            assert bad.size == 0, f"{bad.size} guard elements overwritten, first at {bad[:4]}"
        return a[GUARD:GUARD + self.n].reshape(self.shape).view(self.dt if self.dt != np.uint16 else np.uint16)

    def is_sentinel(self, a):
        return a.view(_VIEW[self.dt]) == SENT[self.dt]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ratio(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = float(np.nanmax(err / bound)) if err.size else 0.0
    print(f"{name}: max err {err.max():.3e}, max err / bound {r:.3f}")
    assert np.isfinite(np.asarray(got, np.float64)).all()
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} of {err.size} elements outside the bound, worst ratio {r:.3f}"
    return r


def _pick(a, pts):
    return a.reshape(-1, a.shape[-1]) if pts is None else a[pts[0], pts[1]]


# ---- u8_to_rgb -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1080, 1920), (70, 100), (1, 1), (32, 32)])
def test_u8_to_rgb(hip_lib, H, W):
    rng = np.random.default_rng(H + W)
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = Out((Hp, Wp, 3), np.float32)
    d_img = dev(img)
    _lib.check(hip_lib.fw_u8_to_rgb_f32(P(d_img), H, W, Hp, Wp, out.ptr(), None))
    got = out.take()
    ref, bound = G.u8_to_rgb(img, Hp, Wp)
    assert (got[H:] == 0).all() and (got[:, W:] == 0).all()                       # the zero fill, exactly
    _ratio(f"u8_to_rgb {H}x{W}", got[:H, :W], ref[:H, :W], bound[:H, :W] + G.TINY)


# ---- resize ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,ws,sf", [(64, 96, 0.125), (64, 96, 0.25), (64, 96, 0.5), (64, 96, 1.0), (16, 24, 2.0), (16, 24, 4.0), (16, 24, 8.0),
                                      (1088, 1920, 1.0), (1088, 1920, 0.5), (272, 480, 4.0)])
def test_resize_bilinear(hip_lib, hs, ws, sf):
    rng = np.random.default_rng(int(hs * sf))
    src = rng.standard_normal((hs, ws, 5)).astype(np.float32)
    hd, wd = int(hs * sf), int(ws * sf)
    out = Out((hd, wd, 8), np.float32)
    d_src = dev(src)
    _lib.check(hip_lib.fw_resize_bilinear_f32(P(d_src), hs, ws, 5, out.ptr(), hd, wd, 8, 2, sf, 0.375, None))
    got = out.take()
    assert out.is_sentinel(got[..., :2]).all() and out.is_sentinel(got[..., 7:]).all()      # channels outside dst_coff .. + C
    pts = G.sample_points(hd, wd, rng)
    ref, bound = G.resize_bilinear(src, sf, 0.375, pts)
    _ratio(f"resize {hs}x{ws} x{sf}", _pick(got[..., 2:7], pts), ref, bound)


# ---- warp / build_x --------------------------------------------------------------------------------------------------------------
def _bx_cases():
    for H, W in SHAPES:
        big = H * W > 1 << 18
        for ik in G.IMAGE_KINDS:
            for fk in G.FLOW_KINDS:
                if big and (ik, fk) not in (("step", "rand6"), ("step", "smooth"), ("noise", "edge"), ("noise", "huge")):
                    continue
                yield H, W, ik, fk


@pytest.mark.parametrize("H,W,img_kind,flow_kind", list(_bx_cases()))
def test_build_x_and_warp(hip_lib, H, W, img_kind, flow_kind):
    rng = np.random.default_rng([H, W, len(img_kind), G.FLOW_KINDS.index(flow_kind)])
    i0, i1 = G.make_images(img_kind, H, W, rng)
    flow, mask = G.make_flow(flow_kind, H, W, rng), G.make_mask(H, W, rng)
    t = 0.25 if flow_kind in ("smooth", "huge") else 0.5
    out = Out((H, W, 8), np.float32)
    d0, d1, df, dm = dev(i0), dev(i1), dev(flow), dev(mask)          # kept alive until the kernels have run
    _lib.check(hip_lib.fw_ifnet_build_x(P(d0), P(d1), P(df), P(dm), H, W, t, out.ptr(), None))
    got = out.take()
    pts = G.sample_points(H, W, rng)
    ref, bound = G.build_x(i0, i1, flow, mask, t, pts)
    g = _pick(got, pts)
    assert np.array_equal(g[:, 6:].astype(np.float64), ref[:, 6:])                      # timestep and mask: copies
    _ratio(f"build_x {H}x{W} {img_kind} {flow_kind}", g[:, :6], ref[:, :6], bound[:, :6])
    assert (got[..., 6] == np.float32(t)).all() and np.array_equal(got[..., 7], mask)
    if flow_kind == "zero":
        out7 = Out((H, W, 7), np.float32)
        _lib.check(hip_lib.fw_ifnet_build_x(P(d0), P(d1), None, None, H, W, t, out7.ptr(), None))
        g7 = out7.take()
        assert np.array_equal(g7[..., :3], i0) and np.array_equal(g7[..., 3:6], i1) and (g7[..., 6] == np.float32(t)).all()


# ---- pixel (un)shuffle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("h,w,C_,cs,cpad,typed", [
    (12, 20, 7, 7, 32, False), (64, 96, 12, 13, 64, False), (1088, 1920, 12, 12, 64, False),      # fp32 source: the cast
    (12, 20, 6, 10, 32, True), (64, 96, 32, 32, 128, True), (544, 960, 32, 32, 128, True),       # typed, even C: unshuffle_typed8_kernel
    (12, 20, 7, 10, 32, True), (12, 20, 6, 11, 32, True)])                                       # odd C / odd stride: the scalar kernel
def test_unshuffle2_cast_is_exact(hip_lib, dtype, h, w, C_, cs, cpad, typed):
    """Exact for every path: a typed source with even C and stride takes unshuffle_typed8_kernel (C < cpad / 4 leaves whole 16-byte
    groups of zeros, cs > C channels that must not be read into the output); an odd C or stride falls back to the scalar kernel and
    must give the same tensor."""
    rng = np.random.default_rng(h + C_ + cs)
    x = (rng.standard_normal((h, w, cs)) * np.exp(rng.uniform(-8, 4, (h, w, cs)))).astype(np.float32)
    bits = G.to_bits(x, dtype).reshape(h, w, cs)
    src = dev(bits.view(np.int16)) if typed else dev(x)
    out = Out((h // 2, w // 2, cpad), np.uint16)
    _lib.check(hip_lib.fw_unshuffle2_cast(DT[dtype], P(src), 0 if typed else 1, h, w, C_, cs, out.ptr(), cpad, None))
    assert np.array_equal(out.take(), G.unshuffle2(bits, C_, cpad))


@pytest.mark.parametrize("h,w,cs", [(1, 1, 96), (16, 20, 100), (272, 480, 96)])
def test_depth_to_space4_is_exact(hip_lib, h, w, cs):
    rng = np.random.default_rng(h)
    src = rng.standard_normal((h, w, cs)).astype(np.float32)
    out = Out((4 * h, 4 * w, 6), np.float32)
    d_src = dev(src)
    _lib.check(hip_lib.fw_depth_to_space4_f32(P(d_src), h, w, cs, out.ptr(), None))
    assert np.array_equal(out.take(), G.depth_to_space4(src))


# ---- accumulate, separate and reading lastconv's output in place -----------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("s", [8, 4, 2, 1])
@pytest.mark.parametrize("first", [1, 0])
def test_accumulate_and_accumulate_d2s(hip_lib, H, W, s, first):
    """Both accumulate kernels against the float64 reference, and against each other.  ifnet_accumulate_d2s_kernel reads through the
    permuted layout the very values ifnet_accumulate_kernel reads from the depth-to-space copy.  At s = 1 the bilinear weights are 0
    and 1, every product is exact and the two must agree bit for bit, which is asserted.  At s = 2, 4, 8 they do not: on the MI355X
    the masks are identical everywhere but up to 60 % of the flow elements differ in the last fp32 bit (2483136 of 8355840 at
    1088 x 1920, s = 8), with the same worst err / bound (0.41) for both.  The two kernels are different source (a loop over
    `(first ? 0 : flow) + v * scale` there, four float4 members here) and the compiler contracts the multiply-adds of the blend that
    feeds `v * scale + f` differently in each; neither order is the reference's.  Both forms are therefore held to the float64
    reference and its bound, element by element, and the count of differing elements is printed."""
    rng = np.random.default_rng([H, W, s, first])
    hf, wf = H // s // 4, W // s // 4
    src = (rng.standard_normal((hf, wf, 96)) * 3).astype(np.float32)                 # lastconv's output in depth_to_space4's row order
    tmp = G.depth_to_space4(src)
    flow0, mask0 = (rng.standard_normal((H, W, 4)) * 5).astype(np.float32), G.make_mask(H, W, rng)
    pts = G.sample_points(H, W, rng)
    rf, bf, rm, bm = G.accumulate(tmp, H, W, float(s), flow0, mask0, bool(first), pts)
    # separate kernels
    tmp_d = Out((4 * hf, 4 * wf, 6), np.float32)
    d_src = dev(src)
    _lib.check(hip_lib.fw_depth_to_space4_f32(P(d_src), hf, wf, 96, tmp_d.ptr(), None))
    fa, ma = Out((H, W, 4), np.float32, flow0), Out((H, W), np.float32, mask0)
    _lib.check(hip_lib.fw_ifnet_accumulate(tmp_d.ptr(), 4 * hf, 4 * wf, H, W, float(s), fa.ptr(), ma.ptr(), first, None))
    assert np.array_equal(tmp_d.take(), tmp)
    # in place, through the permuted layout with a channel stride of 98 (the two channels behind the 96 are never read)
    t96 = G.tmp_to_t96(tmp, cs=98, fill=np.float32(np.nan))
    assert np.array_equal(t96[..., :96], G.d2s_rows_to_t96(src))
    fb, mb = Out((H, W, 4), np.float32, flow0), Out((H, W), np.float32, mask0)
    d_t96 = dev(t96)
    _lib.check(hip_lib.fw_ifnet_accumulate_d2s(P(d_t96), hf, wf, 98, H, W, float(s), fb.ptr(), mb.ptr(), first, None))
    ga, gma, gb, gmb = fa.take(), ma.take(), fb.take(), mb.take()
    tag = f"{H}x{W} s={s} first={first}"
    _ratio(f"accumulate flow {tag}", _pick(ga, pts), rf, bf)
    _ratio(f"accumulate mask {tag}", _pick(gma[..., None], pts)[:, 0], rm, bm)
    _ratio(f"accumulate_d2s flow {tag}", _pick(gb, pts), rf, bf)
    _ratio(f"accumulate_d2s mask {tag}", _pick(gmb[..., None], pts)[:, 0], rm, bm)
    nf, nm = int((ga != gb).sum()), int((gma != gmb).sum())
    print(f"accumulate_d2s vs depth_to_space4 + accumulate {tag}: {nf} flow and {nm} mask elements differ")
    if s == 1:
        assert nf == 0 and nm == 0


# ---- an IFBlock's input ----------------------------------------------------------------------------------------------------------
def _si_cases():
    for H, W in SHAPES + [(2176, 3840)]:
        for s in (8, 4, 2, 1):
            if (H, W) == (2176, 3840) and s != 1:
                continue
            for first in (1, 0):
                # dtype, timestep, images and flows rotate over the cases; every value of each meets every scale
                k = (s.bit_length() + first + H // 32) % 2
                big = H * W > 1 << 18
                kinds = [("step", "rand6")] if big else [("noise", "smooth"), ("step", "rand6"), ("noise", "edge"), ("step", "huge"),
                                                        ("noise", "integer"), ("step", "zero")]
                for j, (ik, fk) in enumerate(kinds if not first else kinds[:2]):
                    yield H, W, s, first, ("f16", "bf16")[(k + j) % 2], (0.25, 0.5)[(k + j // 2) % 2], ik, fk
    yield 64, 96, 2, 0, "bf16", 0.25, "noise", "rand6"
    yield 64, 96, 4, 0, "f16", 0.25, "step", "smooth"


@pytest.mark.parametrize("H,W,s,first,dtype,t,img_kind,flow_kind", list(_si_cases()))
def test_stage_input(hip_lib, H, W, s, first, dtype, t, img_kind, flow_kind):
    """ifnet_stage_input_kernel against the float64 composition of ifnet_ref.ifblock's front end: the typed value within half an ulp of
    the output type plus the fp32 bound, zeros behind 4 cin, nothing outside the tensor.

    Against build_x -> resize -> resize -> unshuffle_cast on the whole frame: the kernel's comment claims the same expressions in the
    same order, so the copied channels (timestep, mask, and everything at s = 1, where the resize is the identity) must agree bit
    for bit.  The warped and resized channels are the same source expressions compiled in two kernels; the compiler may contract a
    multiply-add in one and not in the other, so an element may differ in its last fp32 bit and flip a rounding of the typed
    output.  Such elements are counted and printed; both forms are held to the same float64 reference and bound.  On the MI355X 70
    of the 76 cases agree in every element; the others differ in 1 to 111 elements (111 of 8355840 at 1088 x 1920, s = 2; 28 of
    133693440 at 2176 x 3840), a few of them in the timestep / mask / flow channels at s > 1, none in those at s = 1."""
    rng = np.random.default_rng([H, W, s, first, len(img_kind), G.FLOW_KINDS.index(flow_kind)])
    i0, i1 = G.make_images(img_kind, H, W, rng)
    flow, mask = (None, None) if first else (G.make_flow(flow_kind, H, W, rng), G.make_mask(H, W, rng))
    cin, cpad = (7, 32) if first else (12, 64)
    ho, wo = H // s // 2, W // s // 2
    d = {k: (dev(v) if v is not None else None) for k, v in dict(i0=i0, i1=i1, flow=flow, mask=mask).items()}
    out = Out((ho, wo, cpad), np.uint16)
    _lib.check(hip_lib.fw_ifnet_stage_input(DT[dtype], P(d["i0"]), P(d["i1"]), P(d["flow"]), P(d["mask"]), H, W, t, s, out.ptr(), cpad, None))
    bits = out.take()
    assert (bits[..., 4 * cin:] == 0).all()                                           # the padding behind 4 cin: zeros
    pts = G.sample_points(ho, wo, rng) if H * W > 1 << 18 else None
    ref, bound = G.stage_input(i0, i1, flow, mask, t, s, cpad, pts)
    tag = f"stage_input {H}x{W} s={s} first={first} {dtype} t={t} {img_kind} {flow_kind}"
    _ratio(tag, G.from_bits(_pick(bits, pts), dtype)[:, :4 * cin], ref[:, :4 * cin], G.typed_allowance(ref, bound, dtype)[:, :4 * cin])
    # the separate kernels
    X = Out((H, W, 7 if first else 8), np.float32)
    _lib.check(hip_lib.fw_ifnet_build_x(P(d["i0"]), P(d["i1"]), P(d["flow"]), P(d["mask"]), H, W, t, X.ptr(), None))
    xin = Out((H // s, W // s, cin), np.float32)
    _lib.check(hip_lib.fw_resize_bilinear_f32(X.ptr(), H, W, 7 if first else 8, xin.ptr(), H // s, W // s, cin, 0, 1.0 / s, 1.0, None))
    if not first:
        _lib.check(hip_lib.fw_resize_bilinear_f32(P(d["flow"]), H, W, 4, xin.ptr(), H // s, W // s, cin, 8, 1.0 / s, 1.0 / s, None))
    sep = Out((ho, wo, cpad), np.uint16)
    _lib.check(hip_lib.fw_unshuffle2_cast(DT[dtype], xin.ptr(), 1, H // s, W // s, cin, cin, sep.ptr(), cpad, None))
    X.take(), xin.take()
    sb = sep.take()
    _ratio(tag + " (separate kernels)", G.from_bits(_pick(sb, pts), dtype)[:, :4 * cin], ref[:, :4 * cin],
           G.typed_allowance(ref, bound, dtype)[:, :4 * cin])
    diff = bits != sb
    print(f"{tag}: {int(diff.sum())} of {diff.size} elements differ between the fused and the separate kernels "
          f"({int(diff[..., :24].sum())} of them in the image channels)")
    if s == 1:
        assert not diff[..., 24:32].any() and (first == 0 or not diff.any())          # identity resize of copies: bit for bit
    if not first and s == 1:
        assert not diff[..., 32:48].any()                                             # flow * 1 / 1


# ---- blend -----------------------------------------------------------------------------------------------------------------------
def _blend_params():
    for H, W in [(1080, 1920), (70, 100), (1, 1), (64, 96)]:
        for c in G.blend_cases(H, W):
            yield (H, W) + tuple(c)


@pytest.mark.parametrize("H,W,img_kind,flow_kind", list(_blend_params()))
def test_blend(hip_lib, H, W, img_kind, flow_kind):
    """The fp32 RGB frame inside the bound; the uint8 BGR frame exactly rint(255 clamp(ref)) outside the window around a half-integer
    and one of the two neighbours inside it; the window covers at most 0.5 % of the elements (a property of the reference)."""
    i0, i1, flow, mask, pts = G.blend_inputs(H, W, img_kind, flow_kind)
    Hp, Wp = mask.shape
    u8, rgb = Out((H, W, 3), np.uint8), Out((H, W, 3), np.float32)
    d0, d1, df, dm = dev(i0), dev(i1), dev(flow), dev(mask)          # kept alive until the kernels have run
    _lib.check(hip_lib.fw_ifnet_blend(P(d0), P(d1), P(df), P(dm), Hp, Wp, H, W, u8.ptr(), rgb.ptr(), None))
    ref, bound = G.blend(i0, i1, flow, mask, H, W, pts)
    tag = f"blend {H}x{W} {img_kind} {flow_kind}"
    _ratio(tag, _pick(rgb.take(), pts), ref, bound)
    lo, hi, share = G.u8_window(ref, bound)
    got = _pick(u8.take(), pts)[:, ::-1].astype(np.int64)                              # BGR -> RGB
    print(f"{tag}: uint8 window holds {100 * share:.3f} % of the elements, {int((got != lo).sum())} of them take the upper neighbour")
    assert share <= G.U8_WINDOW_SHARE
    assert ((got >= lo) & (got <= hi)).all(), f"{int(((got < lo) | (got > hi)).sum())} uint8 elements outside the window"
    # one output at a time gives the same frames
    only = Out((H, W, 3), np.uint8)
    _lib.check(hip_lib.fw_ifnet_blend(P(d0), P(d1), P(df), P(dm), Hp, Wp, H, W, only.ptr(), None, None))
    assert np.array_equal(only.take(), u8.take())


def test_blend_rounds_ties_to_even(hip_lib):
    """Pixels whose 255-fold is EXACTLY k + 0.5 in the kernel's own arithmetic: zero flow (weights 0 and 1: the warp returns the pixel),
    mask 0 (expf(-0) = 1, m = 0.5: v = 0.5 p + 0.5 p = p, no rounding anywhere) and p an fp32 number with fl(255 p) = k + 0.5, found
    here in IEEE fp32.  rint rounds them to the even neighbour; round-half-away would give k + 1 for every even k."""
    k = np.arange(255)
    p = ((k + 0.5) / 255.0).astype(np.float32)
    tie = (p * np.float32(255.0)) == (k + 0.5).astype(np.float32)
    k, p = k[tie], p[tie]
    assert k.size >= 64 and (k % 2 == 0).sum() >= 16, k.size
    H, W = 32, 32
    n = H * W
    plane = np.resize(p, n).reshape(H, W, 1).repeat(3, 2)
    want = np.resize(k + (k % 2), n).reshape(H, W, 1).repeat(3, 2).astype(np.uint8)
    u8 = Out((H, W, 3), np.uint8)
    img, zf, zm = dev(plane), torch.zeros((H, W, 4), device="cuda"), torch.zeros((H, W), device="cuda")
    _lib.check(hip_lib.fw_ifnet_blend(P(img), P(img), P(zf), P(zm), H, W, H, W, u8.ptr(), None, None))
    assert np.array_equal(u8.take(), want)


def test_sigmoid_of_the_blend(hip_lib):
    """i0 = 1, i1 = 0, zero flow: the fp32 output IS the kernel's m = 1 / (1 + expf(-mask)); its relative error against float64 must
    stay inside ifnet_glue_ref.sigmoid's bound over the whole mask range, the saturated ends included."""
    H, W = 64, 1024
    mask = np.linspace(-20, 20, H * W).astype(np.float32).reshape(H, W)
    one, zero = np.ones((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    rgb = Out((H, W, 3), np.float32)
    d1, d0, df, dm = dev(one), dev(zero), torch.zeros((H, W, 4), device="cuda"), dev(mask)
    _lib.check(hip_lib.fw_ifnet_blend(P(d1), P(d0), P(df), P(dm), H, W, H, W, None, rgb.ptr(), None))
    m, rm = G.sigmoid(mask)
    got = rgb.take()[..., 0].astype(np.float64)
    rel = np.abs(got - m) / m
    print(f"sigmoid: max relative error {rel.max():.3e} = {rel.max() / 2.0 ** -24:.2f} u, bound {rm.max() / 2.0 ** -24:.2f} u, max err / bound {(rel / rm).max():.3f}")
    assert (rel <= rm).all()


# ---- bad arguments of the two new entries ----------------------------------------------------------------------------------------
def test_entries_share_the_engine_launchers_6x10(hip_lib):
    """Every glue entry that has a launcher twin in the engine (csrc/ifnet_ops.hip: the fw_* entry checks its arguments and calls the
    launch_* that csrc/ifnet.hip sequences), on a 6 x 10 frame padded to 8 x 16: one block, a partial one.  The engine exposes no
    intermediate tensor, so each entry is held to its kernel's float64 reference and bound of tests/ifnet_glue_ref.py, exact where the
    kernel is a copy; at s = 1 the two accumulate forms must agree bit for bit, as in test_accumulate_and_accumulate_d2s."""
    H, W, Hp, Wp = 6, 10, 8, 16
    rng = np.random.default_rng(610)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    d_img, rgb = dev(img), Out((Hp, Wp, 3), np.float32)
    _lib.check(hip_lib.fw_u8_to_rgb_f32(P(d_img), H, W, Hp, Wp, rgb.ptr(), None))
    got = rgb.take()
    ref, bound = G.u8_to_rgb(img, Hp, Wp)
    assert (got[H:] == 0).all() and (got[:, W:] == 0).all()
    _ratio("6x10 u8_to_rgb", got[:H, :W], ref[:H, :W], bound[:H, :W] + G.TINY)

    i0, i1 = G.make_images("noise", Hp, Wp, rng)
    flow, mask = G.make_flow("rand6", Hp, Wp, rng), G.make_mask(Hp, Wp, rng)
    d0, d1, df, dm = dev(i0), dev(i1), dev(flow), dev(mask)
    X = Out((Hp, Wp, 8), np.float32)
    _lib.check(hip_lib.fw_ifnet_build_x(P(d0), P(d1), P(df), P(dm), Hp, Wp, 0.5, X.ptr(), None))
    x = X.take()
    ref, bound = G.build_x(i0, i1, flow, mask, 0.5)
    assert np.array_equal(x.reshape(-1, 8)[:, 6:].astype(np.float64), ref[:, 6:])
    _ratio("6x10 build_x", x.reshape(-1, 8)[:, :6], ref[:, :6], bound[:, :6])

    half = Out((Hp // 2, Wp // 2, 8), np.float32)
    _lib.check(hip_lib.fw_resize_bilinear_f32(P(df), Hp, Wp, 4, half.ptr(), Hp // 2, Wp // 2, 8, 2, 0.5, 0.5, None))
    h = half.take()
    assert half.is_sentinel(h[..., :2]).all() and half.is_sentinel(h[..., 6:]).all()
    ref, bound = G.resize_bilinear(flow, 0.5, 0.5)
    _ratio("6x10 resize", h[..., 2:6].reshape(-1, 4), ref, bound)

    for dtype in ("f16", "bf16"):
        bits = G.to_bits(x, dtype).reshape(Hp, Wp, 8)
        for typed, src in ((True, dev(bits.view(np.int16))), (False, dev(x))):
            us = Out((Hp // 2, Wp // 2, 32), np.uint16)
            _lib.check(hip_lib.fw_unshuffle2_cast(DT[dtype], P(src), 0 if typed else 1, Hp, Wp, 8, 8, us.ptr(), 32, None))
            assert np.array_equal(us.take(), G.unshuffle2(bits, 8, 32))
        for s_ in (1, 2):
            si = Out((Hp // s_ // 2, Wp // s_ // 2, 64), np.uint16)
            _lib.check(hip_lib.fw_ifnet_stage_input(DT[dtype], P(d0), P(d1), P(df), P(dm), Hp, Wp, 0.5, s_, si.ptr(), 64, None))
            sb = si.take()
            assert (sb[..., 48:] == 0).all()
            ref, bound = G.stage_input(i0, i1, flow, mask, 0.5, s_, 64)
            _ratio(f"6x10 stage_input s={s_} {dtype}", G.from_bits(sb.reshape(-1, 64), dtype)[:, :48], ref[:, :48],
                   G.typed_allowance(ref, bound, dtype)[:, :48])

    src96 = (rng.standard_normal((Hp // 4, Wp // 4, 96)) * 3).astype(np.float32)
    tmp = G.depth_to_space4(src96)
    d_src, tmp_d = dev(src96), Out((Hp, Wp, 6), np.float32)
    _lib.check(hip_lib.fw_depth_to_space4_f32(P(d_src), Hp // 4, Wp // 4, 96, tmp_d.ptr(), None))
    assert np.array_equal(tmp_d.take(), tmp)
    rf, bf, rm, bm = G.accumulate(tmp, Hp, Wp, 1.0, flow, mask, False)
    fa, ma = Out((Hp, Wp, 4), np.float32, flow), Out((Hp, Wp), np.float32, mask)
    _lib.check(hip_lib.fw_ifnet_accumulate(tmp_d.ptr(), Hp, Wp, Hp, Wp, 1.0, fa.ptr(), ma.ptr(), 0, None))
    d_t96 = dev(G.tmp_to_t96(tmp, cs=98, fill=np.float32(np.nan)))
    fb, mb = Out((Hp, Wp, 4), np.float32, flow), Out((Hp, Wp), np.float32, mask)
    _lib.check(hip_lib.fw_ifnet_accumulate_d2s(P(d_t96), Hp // 4, Wp // 4, 98, Hp, Wp, 1.0, fb.ptr(), mb.ptr(), 0, None))
    ga, gma, gb, gmb = fa.take(), ma.take(), fb.take(), mb.take()
    _ratio("6x10 accumulate flow", ga.reshape(-1, 4), rf, bf)
    _ratio("6x10 accumulate mask", gma.reshape(-1), rm, bm)
    assert np.array_equal(ga, gb) and np.array_equal(gma, gmb)

    u8, out_rgb = Out((H, W, 3), np.uint8), Out((H, W, 3), np.float32)
    _lib.check(hip_lib.fw_ifnet_blend(P(d0), P(d1), P(df), P(dm), Hp, Wp, H, W, u8.ptr(), out_rgb.ptr(), None))
    ref, bound = G.blend(i0, i1, flow, mask, H, W)
    _ratio("6x10 blend", out_rgb.take().reshape(-1, 3), ref, bound)
    lo, hi, _ = G.u8_window(ref, bound)
    g8 = u8.take().reshape(-1, 3)[:, ::-1].astype(np.int64)
    assert ((g8 >= lo) & (g8 <= hi)).all()


def test_stage_input_and_accumulate_d2s_reject_bad_arguments(hip_lib):
    H, W = 64, 96
    z = lambda *s: torch.zeros(s, device="cuda")
    i0, i1, flow, mask, dst = z(H, W, 3), z(H, W, 3), z(H, W, 4), z(H, W), torch.zeros(H * W * 64, dtype=torch.int16, device="cuda")
    F16 = _lib.FW_DTYPE_F16
    si = lambda *a: hip_lib.fw_ifnet_stage_input(*a)
    assert si(F16, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 64, None) == _lib.FW_OK
    bad = [
        (F16, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 72, None),       # dst_channels > 64
        (F16, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 60, None),       # not a multiple of 8
        (F16, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 40, None),       # below 4 * 12
        (F16, P(i0), P(i1), P(flow), P(mask), H, 100, 0.5, 4, P(dst), 64, None),     # W % (2 s) != 0
        (F16, P(i0), P(i1), P(flow), P(mask), 72, W, 0.5, 8, P(dst), 64, None),      # H % (2 s) != 0
        (F16, P(i0), P(i1), P(flow), None, H, W, 0.5, 2, P(dst), 64, None),          # flow without mask
        (F16, P(i0), P(i1), None, P(mask), H, W, 0.5, 2, P(dst), 32, None),          # mask without flow
        (7, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 64, None),         # dtype
        (F16, None, P(i1), P(flow), P(mask), H, W, 0.5, 2, P(dst), 64, None),
        (F16, P(i0), P(i1), P(flow), P(mask), H, W, 0.5, 0, P(dst), 64, None),
    ]
    for a in bad:
        assert si(*a) == _lib.FW_ERR_INVALID, a
        assert b"fw_ifnet_stage_input" in hip_lib.fw_last_error()
    t96 = z(4, 6, 98)
    acc = lambda *a: hip_lib.fw_ifnet_accumulate_d2s(*a)
    assert acc(P(t96), 4, 6, 98, H, W, 4.0, P(flow), P(mask), 1, None) == _lib.FW_OK
    bad = [
        (P(t96), 4, 6, 97, H, W, 4.0, P(flow), P(mask), 1, None),                    # odd channel stride
        (P(t96), 4, 6, 94, H, W, 4.0, P(flow), P(mask), 1, None),                    # below 96
        (C.c_void_p(t96.data_ptr() + 4), 4, 6, 98, H, W, 4.0, P(flow), P(mask), 1, None),       # t96 not 8-byte aligned
        (P(t96), 4, 6, 98, H, W, 4.0, C.c_void_p(flow.data_ptr() + 4), P(mask), 1, None),       # flow not 16-byte aligned
        (P(t96), 4, 6, 98, H, W, 0.5, P(flow), P(mask), 1, None),                    # scale < 1
        (P(t96), 4, 6, 98, H, W, 4.0, P(flow), None, 1, None),
        (None, 4, 6, 98, H, W, 4.0, P(flow), P(mask), 1, None),
    ]
    for a in bad:
        assert acc(*a) == _lib.FW_ERR_INVALID, a
        assert b"fw_ifnet_accumulate_d2s" in hip_lib.fw_last_error()
    torch.cuda.synchronize()
