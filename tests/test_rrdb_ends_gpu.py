"""The RRDBNet's two ends as the engine wires them: what a forward runs in front of RRDB 0 (fw_rrdbnet_run_head: frame -> NHWC,
conv_first) and behind the last RRDB (fw_rrdbnet_run_tail: conv_body + feat, the two up-convs, conv_hr, conv_last), with the workspace,
buffers and strides of a forward, against tests/rrdb_ends_ref.py in float64.  tests/test_rrdb_blocks_gpu.py does the same for the RRDBs
between them; the three entries together are the forward (test_head_rrdbs_tail_compose_to_the_forward).

Head: conv_first's fp32 output within gamma(10) A_t of the float64 conv_first of the exact typed samples, every element; what RRDB 0
reads bit for bit f32(T(F)) + f32(T(F - f32(T(F)))) of that output (split trunk) or F itself (fp32 trunk).  8-bit frames with all 256
levels in every channel, 16-bit frames that use all 16 bits, the x2 model's reflect row and column at odd sizes.

Tail: the 2 q yardstick of tests/test_rrdb_blocks_gpu.py, same form and factor, on the float RGB plane -

    max |engine - exact| <= 2 q + 1e-6 max |exact|        and        mean |engine - exact| <= 2 mean |rounded - exact| + 1e-6 mean |exact|

with q from the float64 chain evaluated again at the rounding points of the path (rrdb_ends_ref.tail_rounded) - and the u8 and u16
images bit for bit rint(clip(plane, 0, 1) * top) in float32 of the entry's own plane.  conv_last is unshrunk (x 8) and feat and trunk are
doubled lively trunks, so the plane meets both clamps (asserted on the host).  The host test shows that the yardstick rejects a dropped
or 0.2-scaled feat residual, conv_body reading another buffer, LeakyReLU on conv_body and none on up1.  The phase and the gathering
up-conv multiply by different operands (the once-rounded sum of the taps against the typed taps: the host models differ, asserted on
the host), so no byte identity is claimed between FW_RRDB_UP_PHASE 0 and 1: each is held to its own q.

One engine per (dtype, environment, scale), num_block 2; FW_RRDB_* are read at create and set per engine here.  With two RRDBs the
buffer the tail reads, 3 num_block mod the buffers in rotation, is buffer 0 on either trunk, and run_tail lays its trunk into the buffer
it reads, so the tail tests do not pin that index: the composition with one RRDB on the fp32 trunk, which reads buffer 1 from the
workspace, does.  Which forms the tail
dispatches to is asserted on the handle (fw_rrdbnet_tail_paths); that they ran is on record: profiles/rrdb_ends_kernel_stats.csv is the
kernel trace of this file on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guarded
import rrdb_ends_ref as E
from framewright_amd import _lib
from framewright_amd.realesrgan import RRDBNetEngine
from ifnet_glue_ref import typed_ulp
from test_rrdb_blocks_gpu import _Buf, _ratio

pytestmark = pytest.mark.gpu

SWITCHES = ("FW_RRDB_FUSE_PAIRS", "FW_RRDB_FUSE_MASK", "FW_RRDB_SPLIT_TRUNK", "FW_RRDB_LO", "FW_RRDB_C5_WINO", "FW_RRDB_ABL_ALIAS", "FW_RRDB_ABL_RDB3",
            "FW_RRDB_GRAPH", "FW_RRDB_UP_PHASE", "FW_RRDB_HR_LAST", "FW_RRDB_HR_WINO", "FW_PAIR_SLIDE", "FW_PAIR_SLIDE32")
_ENGINES = {}


def _engine(monkeypatch, dtype, env, scale, num_block=E.NUM_BLOCK):
    k = (dtype, tuple(sorted(env.items())), scale, num_block)
    if k not in _ENGINES:
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        for s, v in env.items():
            monkeypatch.setenv(s, v)
        eng = RRDBNetEngine(num_block, scale, dtype)
        eng.load_state_dict({key: v for key, v in E.ends_state(scale).items() if not key.startswith("body.") or int(key.split(".")[1]) < num_block})
        _ENGINES[k] = eng
    return _ENGINES[k]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _frame_dev(frame):
    return guarded.dev(frame)                                        # uint16 travels as int16, bit for bit


# ---- head --------------------------------------------------------------------------------------------------------------------------
def _run_head(eng, frame):
    H, W, _ = frame.shape
    Ht, Wt = ((H + 1) // 2, (W + 1) // 2) if eng.scale == 2 else (H, W)
    src = _frame_dev(frame)
    trunk, feat = _Buf((Ht, Wt, 64)), _Buf((Ht, Wt, 64))
    eng.run_head(src, trunk.t, feat.t)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(frame.dtype), frame), "the frame was written"
    t, f = trunk.take(), feat.take()
    for name, a in (("trunk_out_f32", t), ("feat_out_f32", f)):
        assert not (a.view(np.uint32) == guarded.SENT["f32"]).any(), f"{name} keeps sentinel values"
    return t, f


@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("split", [True, False], ids=["split-trunk", "f32-trunk"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_head_against_float64(hip_lib, monkeypatch, dtype, split, scale):
    """Measured on an MI355X: DESIGN.md (What pins the RRDBNet's two ends)."""
    eng = _engine(monkeypatch, dtype, {} if split else {"FW_RRDB_SPLIT_TRUNK": "0"}, scale)
    assert bool(eng.block_paths() & _lib.FW_RRDB_PATH_SPLIT_TRUNK) == split
    sd = E.ends_state(scale)
    failures = []
    for H, W in E.HEAD_FRAMES[scale]:
        for bits in (8, 16):
            frame = E.head_frame(H, W, bits)
            t, A = E.conv_first(E.frame_to_nhwc(frame, dtype, scale), sd, dtype)
            trunk, feat = _run_head(eng, frame)
            assert feat.shape == t.shape and np.isfinite(feat).all()
            err, bound = np.abs(feat.astype(np.float64) - t), E.bound_first(A)
            print(f"x{scale} {dtype} {'split' if split else 'f32'} {H}x{W} {bits}-bit: max |err| / bound {(err / bound).max():.3f}")
            if not (err <= bound).all():
                failures.append((H, W, bits, "feat", int((err > bound).sum()), float((err / bound).max())))
            want = E.head_trunk(feat, dtype, split)
            if not np.array_equal(trunk.view(np.uint32), want.view(np.uint32)):
                failures.append((H, W, bits, "trunk is not hi + lo of feat" if split else "trunk is not feat", int((trunk != want).sum())))
    assert not failures, failures


def test_head_refuses_what_it_cannot_run(hip_lib, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    eng = RRDBNetEngine(E.NUM_BLOCK, 2, "f16")
    frame = _frame_dev(E.head_frame(4, 6, 8))
    trunk, feat = _Buf((2, 3, 64)), _Buf((2, 3, 64))
    run = lambda h=4, w=6, bits=8, src=guarded.ptr(frame), a=trunk.g.ptr(), b=feat.g.ptr(): eng._lib.fw_rrdbnet_run_head(eng._h, src, bits, h, w, a, b, None)
    assert run() == _lib.FW_ERR_INVALID and b"missing" in eng._lib.fw_last_error()              # no weights yet: not finalised
    eng.load_state_dict(E.ends_state(2))
    for h, w in ((1, 6), (4, 1), (1, 1)):                                                       # the x2 model's refusal of a frame under 2 x 2
        assert run(h, w) == _lib.FW_ERR_INVALID and b"2x2" in eng._lib.fw_last_error(), (h, w)
    for h, w in ((0, 6), (4, 0), (-1, 6), (16385, 6)):
        assert run(h, w) == _lib.FW_ERR_INVALID and b"size" in eng._lib.fw_last_error(), (h, w)
    assert run(bits=12) == _lib.FW_ERR_INVALID
    assert run(src=None) == _lib.FW_ERR_INVALID and run(a=None) == _lib.FW_ERR_INVALID and run(b=None) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize()
    assert guarded.untouched(trunk.take().view(np.uint32), "f32") and guarded.untouched(feat.take().view(np.uint32), "f32"), "a refused call launched something"
    assert run() == _lib.FW_OK
    eng.close()


# ---- tail --------------------------------------------------------------------------------------------------------------------------
P, FU, WI = _lib.FW_RRDB_TAIL_UP_PHASE, _lib.FW_RRDB_TAIL_FUSED, _lib.FW_RRDB_TAIL_HR_WINO
# (id, FW_RRDB_* read at create, dtypes, the host model, the flags fw_rrdbnet_tail_paths must report)
TAIL_PATHS = [
    ("phase-fused", {"FW_RRDB_UP_PHASE": "1", "FW_RRDB_HR_LAST": "1"}, ("f16", "bf16"), E.TailPath(True, False), P | FU),
    ("phase-unfused", {"FW_RRDB_UP_PHASE": "1", "FW_RRDB_HR_LAST": "0"}, ("f16", "bf16"), E.TailPath(True, False), P),
    ("gather-fused", {"FW_RRDB_UP_PHASE": "0", "FW_RRDB_HR_LAST": "1"}, ("f16", "bf16"), E.TailPath(False, False), FU),
    ("gather-unfused", {"FW_RRDB_UP_PHASE": "0", "FW_RRDB_HR_LAST": "0"}, ("f16", "bf16"), E.TailPath(False, False), 0),
    ("hr-wino", {"FW_RRDB_HR_WINO": "1", "FW_RRDB_C5_WINO": "1"}, ("f16",), E.TailPath(True, True), P | WI),
    ("f32-trunk", {"FW_RRDB_SPLIT_TRUNK": "0", "FW_RRDB_HR_LAST": "1"}, ("f16",), E.TailPath(True, False), P | FU),   # two concat buffers in rotation
]
TAIL_CASES = [(pid, env, d, m, fl) for pid, env, ds, m, fl in TAIL_PATHS for d in ds]


@functools.lru_cache(maxsize=None)
def _exact(Ht, Wt):
    feat, trunk, _ = E.tail_inputs(Ht, Wt)
    return feat, trunk, E.tail_exact(feat, trunk, E.ends_state(4))   # (the two scales' states differ in conv_first alone)


@functools.lru_cache(maxsize=None)
def _rounded(Ht, Wt, rt, model):
    feat, trunk, _ = _exact(Ht, Wt)
    return E.tail_rounded(feat, trunk, E.ends_state(4), rt, model)


def _run_tail(eng, feat, trunk, img, bits):
    """-> (float RGB plane, integer BGR image), both img + (3,); guards checked, the inputs unchanged, every sample written."""
    Ht, Wt, _ = feat.shape
    a, b = _Buf((Ht, Wt, 64)), _Buf((Ht, Wt, 64))
    rgb = _Buf(img + (3,))
    q = guarded.Guarded(img[0] * img[1] * 3, "u8" if bits == 8 else "u16")
    eng.run_tail(a.load(feat), b.load(trunk), img[0], img[1], q.body().view(img + (3,)), rgb.t)
    torch.cuda.synchronize()
    assert np.array_equal(a.take().view(np.uint32), feat.view(np.uint32)) and np.array_equal(b.take().view(np.uint32), trunk.view(np.uint32)), "an input was written"
    f = rgb.take()
    assert not (f.view(np.uint32) == guarded.SENT["f32"]).any(), "a sample of the float plane was not written"
    return f, q.take().reshape(img + (3,))


@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("pid,env,dtype,model,flags", TAIL_CASES, ids=[f"{c[0]}-{c[2]}" for c in TAIL_CASES])
def test_tail_against_float64(hip_lib, monkeypatch, pid, env, dtype, model, flags, scale):
    """Measured on an MI355X: DESIGN.md (What pins the RRDBNet's two ends) holds the largest error / q per path and type."""
    eng = _engine(monkeypatch, dtype, env, scale)
    failures = []
    for (Ht, Wt), img in E.TAIL_TRUNKS[scale]:
        assert eng.tail_paths(Ht, Wt) == flags, f"dispatch flags {eng.tail_paths(Ht, Wt)}, expected {flags}"
        feat, trunk, exact = _exact(Ht, Wt)
        exact, rounded = exact[:img[0], :img[1]], _rounded(Ht, Wt, dtype, model)[:img[0], :img[1]]
        f8, i8 = _run_tail(eng, feat, trunk, img, 8)
        f16, i16 = _run_tail(eng, feat, trunk, img, 16)
        assert np.isfinite(f8).all()
        if f8.tobytes() != f16.tobytes():
            failures.append((Ht, Wt, img, "the float plane depends on the image's sample width"))
        err, q, lim, merr, mlim = E.bounds(f8.astype(np.float64), exact, rounded)
        print(f"x{scale} {pid} {dtype} trunk {Ht}x{Wt} -> {img[0]}x{img[1]}: error {err:.3e}, q {q:.3e}, error / q {_ratio(err, q):.3f} "
              f"(mean error / bound {merr / mlim:.3f})")
        if not (err <= lim and merr <= mlim):
            failures.append((Ht, Wt, img, float(err), float(lim), float(merr), float(mlim)))
        for name, got, top in (("u8", i8, 255), ("u16", i16, 65535)):
            want = E.to_image_f32(f8, top)
            if not np.array_equal(got.astype(np.int64), want):
                failures.append((Ht, Wt, img, f"{name} is not rint of the own plane", int((got != want).sum())))
    assert not failures, failures


def test_default_tail_form_follows_the_size(hip_lib, monkeypatch):
    """FW_RRDB_HR_LAST unset: fused when a workgroup gets at least six steps of the fused kernel's 16-row x 30-column walk."""
    eng = _engine(monkeypatch, "f16", {}, 4)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fused = lambda Ht, Wt: ((4 * Wt + 29) // 30) * ((4 * Ht + 16) // 16) >= 6 * cus
    for Ht, Wt in ((9, 17), (270, 480), (4 * cus, 8), (4 * cus - 4, 7)):
        assert bool(eng.tail_paths(Ht, Wt) & FU) == fused(Ht, Wt), (Ht, Wt)
    assert not fused(9, 17) and fused(270, 480)
    assert eng.tail_paths(9, 17) == P


def test_tail_refuses_what_it_cannot_run(hip_lib, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    eng = RRDBNetEngine(E.NUM_BLOCK, 2, "f16")
    a, b, rgb = _Buf((3, 4, 64)), _Buf((3, 4, 64)), _Buf((12, 16, 3))
    a.load(np.zeros((3, 4, 64), np.float32)), b.load(np.zeros((3, 4, 64), np.float32))
    run = lambda ht=3, wt=4, ih=12, iw=16, bits=8, fa=a.g.ptr(), fb=b.g.ptr(), out=None, f=rgb.g.ptr(): \
        eng._lib.fw_rrdbnet_run_tail(eng._h, fa, fb, ht, wt, ih, iw, bits, out, f, None)
    flags = C.c_int(0)
    assert run() == _lib.FW_ERR_INVALID and b"missing" in eng._lib.fw_last_error()              # no weights yet: not finalised
    assert eng._lib.fw_rrdbnet_tail_paths(eng._h, 3, 4, C.byref(flags)) == _lib.FW_ERR_INVALID
    eng.load_state_dict(E.ends_state(2))
    # the x2 model: a frame of 5 .. 6 x 7 .. 8 pixels has a 3 x 4 trunk and a 10 .. 12 x 14 .. 16 image; nothing else has
    for ih, iw in ((13, 16), (12, 17), (8, 16), (12, 12), (11, 16), (12, 15), (0, 16), (12, 0), (-2, 16)):
        assert run(ih=ih, iw=iw) == _lib.FW_ERR_INVALID and b"image size" in eng._lib.fw_last_error(), (ih, iw)
    for ht, wt in ((0, 4), (3, 0), (-1, 4), (8193, 4)):
        assert run(ht, wt) == _lib.FW_ERR_INVALID and b"trunk size" in eng._lib.fw_last_error(), (ht, wt)
        assert eng._lib.fw_rrdbnet_tail_paths(eng._h, ht, wt, C.byref(flags)) == _lib.FW_ERR_INVALID
    assert run(bits=12) == _lib.FW_ERR_INVALID
    assert run(fa=None) == _lib.FW_ERR_INVALID             # (a NULL trunk is a request: the buffer as run_rrdbs left it)
    assert run(f=None) == _lib.FW_ERR_INVALID and b"no output" in eng._lib.fw_last_error()
    assert eng._lib.fw_rrdbnet_tail_paths(eng._h, 3, 4, None) == _lib.FW_ERR_INVALID
    torch.cuda.synchronize()
    assert guarded.untouched(rgb.take().view(np.uint32), "f32"), "a refused call launched something"
    for ih, iw in ((12, 16), (10, 16), (12, 14), (10, 14)):
        out = _Buf((ih, iw, 3))
        assert run(ih=ih, iw=iw, f=out.g.ptr()) == _lib.FW_OK, (ih, iw, eng._lib.fw_last_error())
        torch.cuda.synchronize()
        assert not (out.take().view(np.uint32) == guarded.SENT["f32"]).any()
    eng.close()


# ---- composition ---------------------------------------------------------------------------------------------------------------------
def _ties(x, dtype):
    """Elements of an fp32 map that sit exactly half-way between two numbers of the operand type: the typed pair (hi, lo) they were
    summed from cannot be told from the sum there ((a, + half a spacing) and (b, - half a spacing) are both pairs a conv epilogue
    writes), everywhere else hi = T(x) and lo = T(x - hi) give the pair back."""
    x = x.astype(np.float64)
    hi = E.round_to(x, dtype)
    return int((np.abs(x - hi) == 0.5 * typed_ulp(x, dtype)).sum())


# (dtype, scale, split trunk, num_block).  One and three RRDBs on the fp32 trunk: two buffers in rotation there, so the tail reads
# buffer 3 num_block mod 2 = 1 - with two RRDBs, and on the split trunk's three buffers with any number, it is buffer 0
# The frames: 17x33, the x2 model's crop; and for that model 18x34 as well, the frame that fills the same trunk
COMPOSITIONS = [(d, s, sp, 2, f) for d in ("f16", "bf16") for s in (4, 2) for sp in (False, True) for f in (((17, 33),) if s == 4 else ((17, 33), (18, 34)))] + \
    [("f16", 4, False, 1, (17, 33)), ("bf16", 2, False, 1, (18, 34))]


@pytest.mark.parametrize("dtype,scale,split,num_block,frame_size", COMPOSITIONS,
                         ids=[f"{d}-x{s}-{'split' if sp else 'f32'}-trunk-{nb}-blocks-{f[0]}x{f[1]}" for d, s, sp, nb, f in COMPOSITIONS])
def test_head_rrdbs_tail_compose_to_the_forward(hip_lib, monkeypatch, dtype, scale, split, num_block, frame_size):
    """run_head -> run_rrdbs(0, num_block) -> run_tail against upscale_device of the same frame: the three entries together are the
    forward.

    * Every row but the x2 model's odd frame (run_rrdbs works in the workspace of the frame that fills its trunk, and the tail of a
      cropped image is refused the trunk it left, asserted): with the trunk left in the workspace (run_tail without an fp32 trunk reads the concat buffer as run_rrdbs left it),
      the float plane and the image equal the forward's byte for byte.  A tail that read another buffer than the one the RRDBs wrote
      last would not: with one RRDB on the fp32 trunk that buffer is 1, not 0.
    * fp32 trunk: the same with the trunk handed over as fp32, which is lossless there.
    * split trunk, fp32 hand-over: hi = T(x), lo = T(x - hi) give the typed pair back except where the sum x sits exactly half-way
      between two numbers of the operand type (`_ties`; 14 to 73 of the 9 792 or 35 904 elements here), and conv_body reads hi alone.
      In front of RRDB 0 the pair is the split of conv_first's fp32 output, so feat_out_f32 is handed over there (trunk_out_f32 is
      pinned to it bit for bit in test_head_against_float64).  Behind the last RRDB the composed tail reads, at a tie, the even
      neighbour where the forward may have read the odd one: both are nearest typed numbers of the same trunk value, so both runs are
      the engine's tail on the fp32 trunk that was handed over, and BOTH planes are held to the 2 q yardstick against the float64 tail
      of that trunk (rrdb_ends_ref.tail_exact / tail_rounded) - hence to twice its limit from each other, asserted as well - and the
      composed image to the rint of the composed plane.  Without ties the identity is required here too."""
    env = {} if split else {"FW_RRDB_SPLIT_TRUNK": "0"}
    eng = _engine(monkeypatch, dtype, env, scale, num_block)
    H, W = frame_size
    frame = E.head_frame(H, W, 8)
    src = _frame_dev(frame)
    img = (scale * H, scale * W)
    new = lambda: (torch.empty(img + (3,), dtype=torch.float32, device="cuda"), torch.empty(img + (3,), dtype=torch.uint8, device="cuda"))
    want_rgb, want_u8 = new()
    eng.upscale_device(src, out=want_u8, out_rgb_f32=want_rgb)
    trunk0, feat = eng.run_head(src)
    trunk1 = eng.run_rrdbs(feat if split else trunk0, 0, num_block)
    ws_rgb, ws_u8 = new()
    uncropped = img == (4 * trunk1.shape[0], 4 * trunk1.shape[1])
    if uncropped:
        eng.run_tail(feat, None, img[0], img[1], ws_u8, ws_rgb)        # the trunk as run_rrdbs left it in the workspace
    else:
        assert eng._lib.fw_rrdbnet_run_tail(eng._h, guarded.ptr(feat), None, trunk1.shape[0], trunk1.shape[1], img[0], img[1], 8, None, guarded.ptr(ws_rgb),
                                            None) == _lib.FW_ERR_INVALID and b"uncropped" in eng._lib.fw_last_error()
    got_rgb, got_u8 = new()
    eng.run_tail(feat, trunk1, img[0], img[1], got_u8, got_rgb)        # the trunk as fp32
    torch.cuda.synchronize()
    want_rgb, want_u8, ws_rgb, ws_u8, got_rgb, got_u8 = (t.cpu().numpy() for t in (want_rgb, want_u8, ws_rgb, ws_u8, got_rgb, got_u8))
    assert np.isfinite(want_rgb).all()
    assert not uncropped or (ws_rgb.tobytes() == want_rgb.tobytes() and ws_u8.tobytes() == want_u8.tobytes()), \
        f"workspace hand-over: planes differ by {np.abs(ws_rgb - want_rgb).max():.3e}, {int((ws_u8 != want_u8).sum())} bytes differ"
    ties = _ties(trunk1.cpu().numpy(), dtype) if split else 0
    same = got_rgb.tobytes() == want_rgb.tobytes() and got_u8.tobytes() == want_u8.tobytes()
    diff = float(np.abs(got_rgb.astype(np.float64) - want_rgb).max())
    print(f"x{scale} {dtype} {'split' if split else 'f32'} trunk, {num_block} blocks, frame {H}x{W}: workspace hand-over {'identical' if uncropped else 'refused'}; fp32 hand-over: {ties} tie elements, "
          f"identical: {same}, max |plane difference| {diff:.3e}")
    if ties == 0:
        assert same, f"fp32 hand-over: planes differ by {diff:.3e}"
        return
    sd = E.ends_state(scale)
    model = E.TailPath(bool(eng.tail_paths(*trunk1.shape[:2]) & P), False)
    f, t = feat.cpu().numpy(), trunk1.cpu().numpy()
    exact = E.tail_exact(f, t, sd)[:img[0], :img[1]]
    rounded = E.tail_rounded(f, t, sd, dtype, model)[:img[0], :img[1]]
    for name, plane in (("forward", want_rgb), ("composed", got_rgb)):
        err, q, lim, merr, mlim = E.bounds(plane.astype(np.float64), exact, rounded)
        print(f"    {name}: error {err:.3e}, q {q:.3e}, error / q {_ratio(err, q):.3f} (mean error / bound {merr / mlim:.3f})")
        assert err <= lim and merr <= mlim, (name, float(err), float(lim), float(merr), float(mlim))
    assert diff <= 2 * lim, (diff, float(lim))
    assert np.array_equal(got_u8.astype(np.int64), E.to_image_f32(got_rgb, 255)), "the composed image is not rint of the composed plane"
    assert np.abs(got_u8.astype(np.int64) - want_u8.astype(np.int64)).max() <= 1
