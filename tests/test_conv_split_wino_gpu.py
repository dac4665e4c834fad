"""The two conv5 kernels of the split trunk, each pinned on its own to a float64 host reference (oracle/winograd_ref.py) through the
C-ABI: the direct kernel's EPI_RESIDUAL_SPLIT (csrc/conv3x3_mfma.hip) against the contract, the row-wise Winograd F(2, 3) kernel
(csrc/conv3x3_wino.hip) against an emulation of its own rounding points and, a priori, against the contract; its STORE form
(conv_hr's) the same way and against fw_conv3x3_nhwc.  Per-element bounds (module docstring of the oracle): they hold at any scale,
so the sweep runs the dynamic range of a trained trunk and beyond - heavy tails, a DC offset of 512 (cancellation in d0 - d2), weights
at 0.1x / 1x / 10x of the synthetic bound and rows of taps that sum to zero.  Every output buffer is pre-filled with a sentinel and
guarded on both sides: nothing outside the 64 channels x H x W may change."""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from framewright_amd import _lib
from oracle import winograd_ref as wr

pytestmark = pytest.mark.gpu

F16 = _lib.FW_DTYPE_F16
SENT = 0x7E5A          # a NaN pattern no kernel result can take
GUARD = 4096           # guard elements on both sides of every output buffer
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _acts(rng, kind, shape):
    if kind == "uniform":
        return rng.uniform(-1, 1, shape)
    if kind == "heavy":
        return np.clip(rng.standard_normal(shape) * np.exp(2 * rng.standard_normal(shape)), -1000, 1000)
    if kind == "dc":
        return 512 + rng.standard_normal(shape)
    raise ValueError(kind)


def _weights(rng, chunks, wk):
    cin = 32 * chunks
    bound = 1 / np.sqrt(9 * cin)
    if wk == "zerosum":      # the three taps of every row sum to ~0: U1 and U2 cancel
        w = rng.uniform(-bound, bound, (64, cin, 3, 3))
        w[..., 2] = -(w[..., 0] + w[..., 1])
    else:
        w = rng.uniform(-bound, bound, (64, cin, 3, 3)) * wk
    b = rng.uniform(-bound, bound, 64) * (wk if wk != "zerosum" else 1.0)
    return w.astype(np.float32), b.astype(np.float32)


class Inputs:
    """x (H, W, 32 chunks) and n_id residual planes (H, W, 32), f16, in one device buffer.  layout "inter": interleaved NHWC with
    in_cstride 200 and the planes side by side in a second region; "planar": chunk-planar (H*W*32 per chunk), planes behind."""

    def __init__(self, rng, H, W, chunks, n_id, kind, layout):
        self.H, self.W, self.chunks, self.n_id = H, W, chunks, n_id
        self.x = wr.f16(_acts(rng, kind, (H, W, 32 * chunks)))
        # residual planes: hi-like planes of the same range, lo-like planes (odd index pairs) a few ulp of it
        self.planes = []
        for c in range(n_id):
            v = _acts(rng, kind, (H, W, 32))
            self.planes.append(wr.f16(v if (c // 2) % 2 == 0 or n_id < 4 else v * 2.0 ** -11))
        hw = H * W
        if layout == "inter":
            self.cs, self.ps = 200, 0
            buf = np.zeros((2, hw, 200), np.float16)
            buf[0, :, :32 * chunks] = self.x.reshape(hw, -1)
            for c in range(n_id):
                buf[1, :, 32 * c:32 * c + 32] = self.planes[c].reshape(hw, 32)
            self.chunk_off = [(hw * 200 + 32 * c) * 2 for c in range(n_id)]
        else:
            self.cs, self.ps = 32, hw * 32
            buf = np.zeros((chunks + n_id, hw, 32), np.float16)
            buf[:chunks] = self.x.reshape(hw, chunks, 32).transpose(1, 0, 2)
            for c in range(n_id):
                buf[chunks + c] = self.planes[c].reshape(hw, 32)
            self.chunk_off = [(chunks + c) * hw * 32 * 2 for c in range(n_id)]
        self.dev = torch.from_numpy(buf.reshape(-1).view(np.int16)).cuda()


class Out:
    """A guarded, sentinel-filled output: layout "slice" = channels [64, 128) of a 256-channel NHWC buffer, "planar" = two
    32-channel planes with a gap between them."""

    def __init__(self, H, W, layout):
        self.H, self.W, self.layout = H, W, layout
        hw = H * W
        if layout == "slice":
            self.cs, self.coff, self.ps, n = 256, 64, 32, hw * 256
        else:
            self.cs, self.coff, self.ps = 32, 0, hw * 32 + 64
            n = 2 * self.ps
        self.n = n
        self.dev = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int16, device="cuda")

    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + GUARD * 2)

    def take(self):
        """(H, W, 64) f16 of what the kernel wrote; asserts that everything else still holds the sentinel."""
        a = self.dev.cpu().numpy().view(np.uint16).copy()
        body = a[GUARD:GUARD + self.n]
        H, W = self.H, self.W
        if self.layout == "slice":
            v = body.reshape(H, W, 256)
            out = v[..., 64:128].copy()
            v[..., 64:128] = SENT
        else:
            out = np.concatenate([body[h * self.ps:h * self.ps + H * W * 32].reshape(H, W, 32) for h in range(2)], -1)
            for h in range(2):
                body[h * self.ps:h * self.ps + H * W * 32] = SENT
        bad = np.flatnonzero(a != SENT)
        assert bad.size == 0, f"{bad.size} elements written outside the 64 x H x W output, first at {bad[:4] - GUARD}"
        return out.view(np.float16)


def _pack(lib, w, chunks, wino):
    cin = w.shape[1]
    wc = np.ascontiguousarray(w, np.float32)
    if wino:
        n = lib.fw_pack_conv3x3_wino(F16, None, 64, cin, chunks, None)
        dst = np.zeros(n, np.uint16)
        assert lib.fw_pack_conv3x3_wino(F16, C.c_void_p(wc.ctypes.data), 64, cin, chunks, C.c_void_p(dst.ctypes.data)) == n
    else:
        n = lib.fw_pack_conv3x3(F16, None, 64, cin, 2, chunks, None)
        dst = np.zeros(n, np.uint16)
        assert lib.fw_pack_conv3x3(F16, C.c_void_p(wc.ctypes.data), 64, cin, 2, chunks, C.c_void_p(dst.ctypes.data)) == n
    return torch.from_numpy(dst.view(np.int16)).cuda()


def _split(lib, wino, inp, wp, bias, s1, in_id, id_scale, post_act, out, out_lo):
    offs = (C.c_long * 6)(*inp.chunk_off)
    scs = (C.c_float * 6)(*id_scale)
    return lib.fw_conv3x3_split_nhwc(F16, wino, P(inp.dev), inp.cs, inp.ps, inp.chunks, inp.H, inp.W, P(wp), P(bias), s1, in_id,
                                     inp.n_id, offs, scs, post_act, out.ptr(), out_lo.ptr() if out_lo else None, out.cs, out.ps,
                                     out.coff, _stream())


ID_SCALES = {0: (), 2: (5.0, 5.0), 4: (25.0,) * 4, 6: (5.0, 5.0) + (25.0,) * 4}   # rdb1/2 lo planes; rdb3 R hi + lo; both

# (H, W, cin_chunks, n_id, in_id_scale, s1, input layout, output layout, activations, weights)
CASES = [
    (1, 1, 6, 6, 5.0, 0.04, "planar", "planar", "uniform", 1.0),
    (1, 2, 2, 2, 0.0, 0.2, "inter", "slice", "heavy", 0.1),
    (2, 3, 3, 0, 5.0, 0.2, "inter", "planar", "dc", 10.0),
    (3, 5, 4, 4, 5.0, 0.04, "planar", "slice", "uniform", "zerosum"),
    (15, 31, 5, 2, 5.0, 0.2, "inter", "slice", "heavy", 1.0),
    (16, 32, 6, 4, 5.0, 0.04, "planar", "planar", "dc", 1.0),
    (16, 32, 2, 0, 0.0, 0.2, "inter", "planar", "uniform", 10.0),
    (17, 33, 6, 6, 5.0, 0.04, "inter", "slice", "heavy", 10.0),
    (16, 34, 4, 2, 0.0, 0.2, "planar", "slice", "dc", 0.1),
    (33, 65, 6, 0, 5.0, 0.2, "planar", "planar", "heavy", "zerosum"),
    (33, 65, 3, 2, 5.0, 0.04, "inter", "slice", "dc", "zerosum"),
    (7, 1001, 6, 4, 5.0, 0.04, "planar", "planar", "uniform", 0.1),
    (1001, 7, 5, 4, 0.0, 0.2, "inter", "planar", "heavy", 1.0),
    (300, 600, 6, 6, 5.0, 0.04, "planar", "slice", "dc", 1.0),       # > 256 tiles: the persistent loop and the next-tile prefetch
    (300, 600, 6, 0, 5.0, 0.2, "inter", "planar", "uniform", 1.0),
    (1080, 1920, 6, 4, 5.0, 0.04, "planar", "planar", "uniform", 1.0),  # the 1080p trunk, rdb3's configuration
]


def _case_id(c):
    return f"{c[0]}x{c[1]}-ch{c[2]}-id{c[3]}-in{c[4]:g}-s{c[5]:g}-{c[6]}-{c[7]}-{c[8]}-w{c[9]}"


def _bands(H, band):
    return [(r, min(r + band, H)) for r in range(0, H, band)]


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_split_kernels_against_float64_references(hip_lib, case):
    H, W, chunks, n_id, in_id, s1, lay_in, lay_out, kind, wk = case
    t0 = time.time()
    rng = np.random.default_rng(H * 7919 + W * 31 + chunks * 5 + n_id)
    inp = Inputs(rng, H, W, chunks, n_id, kind, lay_in)
    w, b = _weights(rng, chunks, wk)
    id_scale = ID_SCALES[n_id]
    bias = torch.from_numpy(b).cuda()
    res = {}
    for wino in (0, 1):
        wp = _pack(hip_lib, w, chunks, wino)
        out, lo = Out(H, W, lay_out), Out(H, W, lay_out)
        _lib.check(_split(hip_lib, wino, inp, wp, bias, s1, in_id, id_scale + (0.0,) * (6 - n_id), 0, out, lo))
        # hi alone (out_lo = NULL): the same hi, and nothing else written
        out2 = Out(H, W, lay_out)
        _lib.check(_split(hip_lib, wino, inp, wp, bias, s1, in_id, id_scale + (0.0,) * (6 - n_id), 0, out2, None))
        torch.cuda.synchronize()
        res[wino] = (out.take(), lo.take())
        assert np.array_equal(out2.take().view(np.uint16), res[wino][0].view(np.uint16))
    t_gpu = time.time() - t0
    kw = dict(s1=s1, in_id_scale=in_id, planes=inp.planes, id_scale=id_scale)
    stats = {k: {"max_abs": 0.0, "max_rel": 0.0, "ratio": 0.0} for k in ("direct", "wino", "apriori")}
    ok = {k: True for k in stats}
    bands = _bands(H, 48)
    if H * W > 10 ** 6:
        # the float64 host reference takes ~100 s for a whole 1080p frame: first, middle and last bands here, the whole frame
        # (every workgroup's tiles) Winograd against direct on the GPU, within the a-priori bound
        bands = [bands[0], bands[len(bands) // 2], bands[-1]]
        _whole_frame_cross_check(inp, w, b, s1, in_id, id_scale, res)
    for r0, r1 in bands:
        yc, A = wr.split_contract(inp.x, w, b, rows=(r0, r1), **kw)
        ye, Aw, apr = wr.winograd_emulation(inp.x, w, b, rows=(r0, r1), **kw)
        acc_w = wr.ACC_EPS_WINO * np.maximum(A, Aw)
        d = wr.check_hi_lo(res[0][0][r0:r1], res[0][1][r0:r1], yc, wr.ACC_EPS_DIRECT * A)
        e = wr.check_hi_lo(res[1][0][r0:r1], res[1][1][r0:r1], ye, acc_w)
        hi, lo = res[1][0][r0:r1], res[1][1][r0:r1]
        a = wr.check_apriori(hi.astype(np.float64) + lo, yc, apr, acc_w + np.spacing(np.abs(lo)).astype(np.float64) / 2)
        for k, v in (("direct", d), ("wino", e), ("apriori", a)):
            ok[k] = ok[k] and v["ok"] and v.get("finite", True) and v.get("nearest_ok", True)
            for m in stats[k]:
                if m in v:
                    stats[k][m] = max(stats[k][m], v[m])
    print(f"\n{_case_id(case)}: |y| <= {np.abs(res[0][0].astype(np.float64)).max():.3g}; "
          + "; ".join(f"{k} max-abs {s['max_abs']:.3g} max-rel {s['max_rel']:.3g} err/bound {s['ratio']:.3g}" for k, s in stats.items())
          + f"  (gpu {t_gpu:.1f} s, total {time.time() - t0:.1f} s)")
    assert ok["direct"], stats["direct"]
    assert ok["wino"], stats["wino"]
    assert ok["apriori"], stats["apriori"]


def _whole_frame_cross_check(inp, w, b, s1, in_id, id_scale, res):
    """|wino - direct| (hi + lo each) <= 2^-9 a-priori + both kernels' accumulation bounds, with the bounds' magnitude sums as fp32
    torch convs on the GPU."""
    H, W = inp.H, inp.W
    with torch.no_grad():
        xt = torch.from_numpy(inp.x.astype(np.float32)).cuda().permute(2, 0, 1).unsqueeze(0).abs()
        a = torch.from_numpy(np.abs(w)).cuda()
        S = a.sum(-1)
        ke = torch.stack([a[..., 0], S, a[..., 0] + S], -1)
        ko = torch.stack([S + a[..., 2], S, a[..., 2]], -1)
        apr = F.conv2d(xt, ke, padding=1)
        apr[..., 1::2] = F.conv2d(xt, ko, padding=1)[..., 1::2]
        A = F.conv2d(xt, (2 * S).unsqueeze(-1).expand(-1, -1, -1, 3).contiguous(), torch.from_numpy(np.abs(b)).cuda(), padding=1)   # >= both forms' sums
        if in_id:
            A[:, :64] += abs(in_id) * xt[:, :64]
        for c, sc in enumerate(id_scale):
            A[:, 32 * (c & 1):32 * (c & 1) + 32] += abs(sc) * torch.from_numpy(inp.planes[c].astype(np.float32)).cuda().permute(2, 0, 1).abs()
        bound = abs(s1) * (wr.APRIORI_EPS * apr + (wr.ACC_EPS_DIRECT + wr.ACC_EPS_WINO) * A)
        del xt, apr, A
        y = [torch.from_numpy(res[k][0].astype(np.float32)).cuda().double() + torch.from_numpy(res[k][1].astype(np.float32)).cuda().double()
             for k in (0, 1)]
        gap = (y[1] - y[0]).abs().permute(2, 0, 1).unsqueeze(0)
        ulp = torch.from_numpy(np.spacing(np.abs(res[0][1])).astype(np.float32) + np.spacing(np.abs(res[1][1])).astype(np.float32)).cuda()
        bound = bound.double() + ulp.permute(2, 0, 1).unsqueeze(0).double() / 2
        ratio = (gap / bound).max().item()
    print(f"whole {H}x{W} frame: max |wino - direct| {gap.max().item():.3g}, err/bound {ratio:.3g}")
    assert ratio <= 1.0


def test_post_act_on_the_direct_split_kernel(hip_lib):
    """IFNet's ResConv form (LeakyReLU behind the residual add, in_id_scale 1, planes at scale 1) against the contract."""
    H, W, chunks, n_id = 19, 45, 2, 2
    rng = np.random.default_rng(11)
    inp = Inputs(rng, H, W, chunks, n_id, "uniform", "inter")
    w, b = _weights(rng, chunks, 1.0)
    out, lo = Out(H, W, "planar"), Out(H, W, "planar")
    _lib.check(_split(hip_lib, 0, inp, _pack(hip_lib, w, chunks, 0), torch.from_numpy(b).cuda(), 1.0, 1.0, (1.0, 1.0, 0, 0, 0, 0), 1,
                      out, lo))
    torch.cuda.synchronize()
    hi, lo = out.take(), lo.take()
    yc, A = wr.split_contract(inp.x, w, b, s1=1.0, in_id_scale=1.0, planes=inp.planes, id_scale=(1.0, 1.0), post_act=True)
    r = wr.check_hi_lo(hi, lo, yc, wr.ACC_EPS_DIRECT * A)
    print(f"post_act: max-abs {r['max_abs']:.3g} err/bound {r['ratio']:.3g}")
    assert r["ok"], r
    assert (yc < 0).any() and (yc > 0).any()


def test_winograd_at_the_edge_of_its_f16_domain(hip_lib):
    """Inputs at +-V_F16_DOMAIN (32752, conv3x3_wino.hip header): d1 + d2 and d0 - d2 reach 65504 and stay finite.  Pairs of
    equal-signed neighbours at the limit (the largest sums) and alternating signs (the largest differences)."""
    H, W, chunks = 16, 40, 2
    rng = np.random.default_rng(12)
    x = rng.standard_normal((H, W, 32 * chunks))
    lim = wr.V_F16_DOMAIN
    x[2:5, 4:12] = lim
    x[8:11, 10:20] = -lim
    x[12:14, 20:30] = lim * np.where(np.arange(10) % 2 == 0, 1, -1)[None, :, None]
    inp = Inputs(rng, H, W, chunks, 0, "uniform", "planar")
    inp.x = wr.f16(x)
    inp.dev[:H * W * 32 * chunks] = torch.from_numpy(inp.x.reshape(H * W, chunks, 32).transpose(1, 0, 2).reshape(-1).view(np.int16)).cuda()
    w, b = _weights(rng, chunks, 1e-4)        # small weights: the output stays inside f16 while V sits at its limit
    s1 = 1.0
    out, lo = Out(H, W, "planar"), Out(H, W, "planar")
    _lib.check(_split(hip_lib, 1, inp, _pack(hip_lib, w, chunks, 1), torch.from_numpy(b).cuda(), s1, 0.0, (0.0,) * 6, 0, out, lo))
    torch.cuda.synchronize()
    hi, lo = out.take(), lo.take()
    ye, Aw, apr = wr.winograd_emulation(inp.x, w, b, s1=s1)
    yc, A = wr.split_contract(inp.x, w, b, s1=s1)
    assert np.isfinite(ye).all()
    acc = wr.ACC_EPS_WINO * np.maximum(A, Aw)
    r = wr.check_hi_lo(hi, lo, ye, acc)
    a = wr.check_apriori(hi.astype(np.float64) + lo, yc, apr, acc + np.spacing(np.abs(lo)).astype(np.float64) / 2)
    print(f"V at its f16 limit: |y| <= {np.abs(ye).max():.3g}, err/bound {r['ratio']:.3g} (emulation) {a['ratio']:.3g} (a priori)")
    assert r["ok"] and a["ok"], (r, a)


STORE_SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (15, 31), (16, 32), (17, 33), (16, 34), (33, 65), (7, 1001), (1001, 7), (300, 600),
                (1080, 1920)]


def _direct_store(lib, inp, w, bias, act, out):
    wp = _pack(lib, w, inp.chunks, 0)
    return lib.fw_conv3x3_nhwc(F16, P(inp.dev), inp.cs, inp.ps, inp.chunks, inp.H, inp.W, P(wp), P(bias), 2, act, 0, None, 1.0, None,
                               1.0, out.ptr(), out.cs, out.ps, out.coff, None, _stream())


def _wino_store(lib, inp, w, bias, act, out):
    wp = _pack(lib, w, inp.chunks, 1)
    return lib.fw_conv3x3_wino_nhwc(F16, P(inp.dev), inp.cs, inp.ps, inp.chunks, inp.H, inp.W, P(wp), P(bias), act, out.ptr(), out.cs,
                                    out.ps, out.coff, _stream())


@pytest.mark.parametrize("H,W", STORE_SHAPES)
def test_winograd_store_form(hip_lib, H, W):
    """act(conv + bias), conv_hr's form: against the emulation, a priori against the contract, and against fw_conv3x3_nhwc."""
    rng = np.random.default_rng(H * 131 + W)
    chunks = 2 if H * W > 100000 else int(rng.integers(2, 7))
    kind = ("uniform", "heavy", "dc")[(H + W) % 3]
    inp = Inputs(rng, H, W, chunks, 0, kind, "planar" if (H + W) % 2 else "inter")
    w, b = _weights(rng, chunks, (0.1, 1.0, 10.0, "zerosum")[(H * W) % 4])
    bias = torch.from_numpy(b).cuda()
    for act in (0, 1):
        lay = "slice" if act else "planar"
        ow, od = Out(H, W, lay), Out(H, W, lay)
        _lib.check(_wino_store(hip_lib, inp, w, bias, act, ow))
        _lib.check(_direct_store(hip_lib, inp, w, bias, act, od))
        torch.cuda.synchronize()
        hw, hd = ow.take(), od.take()
        worst = {"wino": 0.0, "apriori": 0.0, "direct": 0.0}
        bands = _bands(H, 48)
        if H * W > 10 ** 6:   # first, middle and last bands (the whole frame of the STORE form: test_winograd_store_form_at_8k)
            bands = [bands[0], bands[len(bands) // 2], bands[-1]]
        for r0, r1 in bands:
            ye, Aw, apr = wr.winograd_emulation(inp.x, w, b, act=act, rows=(r0, r1))
            yc, A = wr.split_contract(inp.x, w, b, act=act, rows=(r0, r1))
            acc = wr.ACC_EPS_WINO * np.maximum(A, Aw)
            e = wr.check_hi_lo(hw[r0:r1], None, ye, acc)
            a = wr.check_apriori(hw[r0:r1], yc, apr, acc + np.spacing(np.abs(hw[r0:r1])).astype(np.float64) / 2)
            d = wr.check_hi_lo(hd[r0:r1], None, yc, wr.ACC_EPS_DIRECT * A)
            assert e["ok"] and a["ok"] and d["ok"], (act, r0, e, a, d)
            # the two kernels agree within the sum of their bounds (f16 outputs: half an ulp each)
            gap = np.abs(hw[r0:r1].astype(np.float64) - hd[r0:r1].astype(np.float64))
            assert (gap <= wr.APRIORI_EPS * apr + acc + wr.ACC_EPS_DIRECT * A
                    + np.spacing(np.abs(hw[r0:r1])).astype(np.float64) / 2 + np.spacing(np.abs(hd[r0:r1])).astype(np.float64) / 2).all()
            worst = {k: max(worst[k], v["ratio"]) for k, v in (("wino", e), ("apriori", a), ("direct", d))}
        print(f"store {H}x{W} ch{chunks} {kind} act={act}: err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_winograd_store_form_at_8k(hip_lib):
    """conv_hr's input of a 1080p frame: 4320 x 7680, chunk-planar (the second chunk lies more than 4 GiB into the buffer, the output
    planes 2 GiB apart), against the direct kernel and a torch fp32 conv of the same f16 operands on the GPU.  The torch conv runs on
    bands of 480 rows (plus their halo): run on the whole 8.5 GB fp32 tensor at once it returned wrong values in four rows
    (2746 - 2749, errors of 1.5) where both kernels agree with it band by band."""
    H, W, B = 4320, 7680, 480
    torch.backends.cudnn.allow_tf32 = False
    g = torch.Generator(device="cuda").manual_seed(8)
    hw = H * W
    x16 = torch.empty((2, hw, 32), dtype=torch.float16, device="cuda")
    x16.uniform_(-1, 1, generator=g)
    rng = np.random.default_rng(8)
    w, b = _weights(rng, 2, 1.0)
    bias = torch.from_numpy(b).cuda()
    outs = {}
    for name in ("wino", "direct"):
        o = torch.full((2, hw, 32), float("nan"), dtype=torch.float16, device="cuda")
        wp = _pack(hip_lib, w, 2, name == "wino")
        if name == "wino":
            st = hip_lib.fw_conv3x3_wino_nhwc(F16, P(x16), 32, hw * 32, 2, H, W, P(wp), P(bias), 1, P(o), 32, hw * 32, 0, _stream())
        else:
            st = hip_lib.fw_conv3x3_nhwc(F16, P(x16), 32, hw * 32, 2, H, W, P(wp), P(bias), 2, 1, 0, None, 1.0, None, 1.0, P(o), 32, hw * 32,
                                         0, None, _stream())
        _lib.check(st)
        outs[name] = o.view(2, H, W, 32)
    torch.cuda.synchronize()
    xv = x16.view(2, H, W, 32)
    wq = torch.from_numpy(w).cuda().half().float()
    a = torch.from_numpy(np.abs(w)).cuda()
    S = a.sum(-1)
    ke = torch.stack([a[..., 0], S, a[..., 0] + S], -1)       # a-priori bound of the Winograd form by output column parity
    ko = torch.stack([S + a[..., 2], S, a[..., 2]], -1)
    worst = {"wino": [0.0, 0.0], "direct": [0.0, 0.0], "gap": [0.0, 0.0]}
    with torch.no_grad():
        for r0 in range(0, H, B):
            r1 = min(r0 + B, H)
            lo_, hi_ = max(r0 - 1, 0), min(r1 + 1, H)
            xin = xv[:, lo_:hi_].permute(0, 3, 1, 2).reshape(1, 64, hi_ - lo_, W).float()
            xin = F.pad(xin, (1, 1, 1 if lo_ == r0 else 0, 1 if hi_ == r1 else 0))
            ref = F.leaky_relu(F.conv2d(xin, wq, bias), 0.2)
            A = F.conv2d(xin.abs(), wq.abs(), bias.abs())
            xa = xin.abs()
            apr = F.conv2d(xa, ke)
            apr[..., 1::2] = F.conv2d(xa, ko)[..., 1::2]
            ys = {}
            for name in ("wino", "direct"):
                y = outs[name][:, r0:r1].permute(0, 3, 1, 2).reshape(1, 64, r1 - r0, W).float()
                assert torch.isfinite(y).all(), name
                ys[name] = y
                half_ulp = y.abs() * 2.0 ** -11 + 2.0 ** -25
                err = (y - ref).abs()
                # torch's fp32 conv rounds on its own: it is granted the direct kernel's accumulation bound
                eps = wr.ACC_EPS_DIRECT + (wr.ACC_EPS_WINO if name == "wino" else wr.ACC_EPS_DIRECT)
                bound = eps * A + half_ulp + (wr.APRIORI_EPS * apr if name == "wino" else 0)
                worst[name] = [max(worst[name][0], err.max().item()), max(worst[name][1], (err / bound).max().item())]
                assert (err <= bound).all(), (name, r0, worst[name])
            gap = (ys["wino"] - ys["direct"]).abs()
            bound = wr.APRIORI_EPS * apr + (wr.ACC_EPS_DIRECT + wr.ACC_EPS_WINO) * A + ys["wino"].abs() * 2.0 ** -10 + 2.0 ** -24
            worst["gap"] = [max(worst["gap"][0], gap.max().item()), max(worst["gap"][1], (gap / bound).max().item())]
            assert (gap <= bound).all(), (r0, worst["gap"])
    print("store 4320x7680: " + ", ".join(f"{k} max-abs {v[0]:.3g} err/bound {v[1]:.3g}" for k, v in worst.items()))


def test_winograd_launchers_reject_what_they_do_not_implement(hip_lib):
    """Each field the Winograd kernels would ignore is an error (FW_ERR_INVALID with a message), never a silent drop."""
    H, W, chunks = 8, 16, 2
    rng = np.random.default_rng(13)
    inp = Inputs(rng, H, W, chunks, 2, "uniform", "planar")
    w, b = _weights(rng, chunks, 1.0)
    wp = _pack(hip_lib, w, chunks, 1)
    bias = torch.from_numpy(b).cuda()
    out = Out(H, W, "planar")

    def split(**kv):
        a = dict(dtype=F16, wino=1, s1=0.2, in_id=5.0, n_id=2, ids=(5.0, 5.0, 0, 0, 0, 0), post_act=0)
        a.update(kv)
        return hip_lib.fw_conv3x3_split_nhwc(a["dtype"], a["wino"], P(inp.dev), 32, H * W * 32, chunks, H, W, P(wp), P(bias), a["s1"],
                                             a["in_id"], a["n_id"], (C.c_long * 6)(*inp.chunk_off, 0, 0, 0, 0),
                                             (C.c_float * 6)(*a["ids"]), a["post_act"], out.ptr(), None, out.cs, out.ps, 0, _stream())

    def rejected(st, word):
        msg = hip_lib.fw_last_error().decode()
        assert st == _lib.FW_ERR_INVALID and word in msg, (st, msg)

    assert split() == _lib.FW_OK
    rejected(split(post_act=1), "post_act")
    rejected(split(in_id=0.1), "in_id_scale")
    rejected(split(ids=(5.0, 0.1, 0, 0, 0, 0)), "identity scale")
    rejected(split(dtype=_lib.FW_DTYPE_BF16), "f16")
    rejected(split(n_id=7), "n_id")
    # the direct kernel: in_id_scale must be exact as well
    rejected(split(wino=0, in_id=0.1, dtype=F16), "in_id_scale")
    rejected(hip_lib.fw_conv3x3_wino_nhwc(_lib.FW_DTYPE_BF16, P(inp.dev), 32, H * W * 32, chunks, H, W, P(wp), P(bias), 1, out.ptr(), 32,
                                          out.ps, 0, _stream()), "f16")
    rejected(hip_lib.fw_conv3x3_wino_nhwc(F16, P(inp.dev), 32, H * W * 32, chunks, H, W, P(wp), P(bias), 2, out.ptr(), 32, H * W * 32, 0,
                                          _stream()), "act_lrelu")
    torch.cuda.synchronize()
    out.take()
    # the launcher-level fields the C-ABI cannot express (chan_scale, res1 / res2, out_f32, n_groups, act in split mode) are checked
    # without a GPU: tests/test_winograd_ref_host.py::test_winograd_launcher_checks_reject_each_field
