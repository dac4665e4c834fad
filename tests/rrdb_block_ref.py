"""TEST INFRASTRUCTURE ONLY (never imported by the product): one RRDB of the RRDBNet trunk in float64 on NHWC arrays - the yardstick of
tests/test_rrdb_blocks_gpu.py, which holds fw_rrdbnet_run_rrdbs (the loop body of csrc/rrdbnet.hip's forward) to it.

Two evaluation modes of the same block:

  * exact (``rrdb``): plain float64, the arithmetic of oracle/rrdbnet_ref.rrdb_forward (tests/test_rrdb_block_ref_host.py pins the two
    against each other at 1e-12 relative);
  * operand-rounded (``rrdb_rounded``): float64 with values rounded (through float32, as the kernels do) at exactly the points where
    the engine path under test rounds them.  Every sum stays float64: the model holds the roundings of a path, not its summation order.

Rounding points, read from csrc/rrdbnet.hip (run_rrdb) and the kernels it launches; T = the operand type:

  every path        weights of conv1 .. conv5 typed (pack_conv3x3_weights); biases fp32
                    x1 .. x4 = T(lrelu(conv + bias)), stored typed in planes 2-5; LeakyReLU's slope is fp32(0.2) (lrelu4)
                    every conv reads typed inputs: the trunk's hi planes 0-1 and x1 .. x4.  In a fused pair (FW_RRDB_FUSE_PAIRS /
                    FUSE_MASK, all three FW_PAIR_SLIDE forms) the second conv reads x_a from LDS: the same typed bits that are
                    stored, so the pair and the two single launches share one model
                    conv5's scale: s1 = fp32(0.2) for rdb1 / rdb2 and fp32(0.2f * 0.2f) for rdb3, applied to the whole sum:
                    y = s1 * (conv5 + 5 x [+ 25 R]) - 5 * fp32(0.2) is not 1, and the model says so
  trunk "lo_rrdb"   (default)  x enters as hi = T(x), lo = T(x - hi).  rdb1: y = s1 (conv5 + 5 hi(R)) - R's lo is not read -, stored
                    as T(y) alone; rdb2: the same on rdb1's typed output; rdb3: y = s1 (conv5 + 5 hi(rdb2) + 25 (hi(R) + lo(R))),
                    stored as hi = T(y), lo = T(y - hi)
  trunk "lo_all"    (FW_RRDB_LO=0)  every dense block adds 5 (hi + lo) of its input and stores hi + lo (n_id 2 / 6)
  trunk "f32"       (FW_RRDB_SPLIT_TRUNK=0)  the trunk is fp32 beside the typed planes: y = fp32(s1 conv5 + res1), rdb3:
                    y = fp32((s1 conv5 + res1) * fp32(0.2) + res2); the next conv reads T(y)
  Winograd conv5    (f16; rdb1 / rdb2 by default, rdb3 with FW_RRDB_C5_WINO=2)  U = f16 of the fp32-transformed fp32 weights and V = B^T d
                    in f16 arithmetic, where oracle/winograd_ref.winograd_emulation rounds them (it is called, not restated); the
                    direct f16 conv5 is winograd_ref.split_contract, hi / lo of f16 are winograd_ref.split_hi_lo

The ``defect=`` argument builds wrong blocks on purpose (tests/test_rrdb_block_ref_host.py shows that the GPU test's bounds reject
them): DEFECTS for the yardstick test, TRUNK_DEFECTS for the trunk-only test.

Trunk-only state: every conv5 weight and bias zero.  Then conv5's accumulators hold the identity terms alone and the RRDB is
elementwise, y = s1 (5 x [+ 25 R]) through the path's representation (``trunk_only_run``); zero weights make the Winograd form the
same sum.  Its error bound per element, none of it fitted to what a kernel returns (u = 2^-24, gamma(n) = n u / (1 - n u)):

  * products 5 * typed and 25 * typed are exact in fp32 (11 + 5 bits), and each identity MFMA rounds the running sum once: a sum of
    m terms makes m - 1 roundings, the product with s1 one more: gamma(m) * |s1| sum |terms|.  A single term (rdb1 / rdb2 of
    "lo_rrdb") is one fp32 product, which the model performs itself (the float64 product of two fp32 numbers is exact, rounded to
    fp32 once): exact, so a typed-only hand-over cannot flip;
  * "f32": rdb1 / rdb2 return res1 itself (0 * s1 + res1); rdb3 is res1 * s2 + res2: gamma(2) (|s2 res1| + |res2|);
  * hi + lo written from an fp32 y that may differ from the model's: each side is within half a spacing of its own lo of its own y:
    + ulp_T(lo_model) / 2 + ulp_T(|lo_model| + e) / 2 - or, where e reaches a rounding boundary of hi (the engine's hi may be the
    neighbour and its lo anything up to ulp_T(y) / 2), + ulp_T(ulp_T(y) / 2);
  * an input error e reaches the output as |s1| (5 e_x + 25 e_R).  Where a dense block reads hi alone ("lo_rrdb": rdb1 of a second
    RRDB reads hi(R) of the first one's output), e_x is how far the engine's hi can sit from the model's: rounding is monotone, so it
    lies between T(y - e) and T(y + e) - zero for all but the few elements whose y is within e of a rounding boundary of T, one spacing
    of T there.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from ifnet_glue_ref import gamma, typed_ulp
from oracle import winograd_ref as WR
from restormer_block_ref import round_to

S = float(np.float32(0.2))                                   # lrelu4's slope and conv5's scale, as the kernels hold them
S_RDB3 = float(np.float32(0.2) * np.float32(0.2))            # `0.2f * 0.2f` of run_rrdb
NUM_BLOCK, SCALE = 2, 4

# trunk: "lo_rrdb" | "lo_all" | "f32"; wino12 / wino3: conv5 of rdb1 + rdb2 / of rdb3 in the Winograd form
Path = namedtuple("Path", "trunk wino12 wino3")
DEFECTS = ("xa_unrounded", "lrelu_missing_conv2", "pair34_plane_short", "x3_in_x4_plane", "rdb3_res_from_rrdb_in", "rdb3_s1")
TRUNK_DEFECTS = ("r_lo_dropped", "r_lo_scale5", "r_from_cur", "rdb1_lo_dropped", "out_lo_unwritten")
DROPPED_LO = ("r_lo_dropped", "rdb1_lo_dropped", "out_lo_unwritten")     # held to a 50-fold margin on the CPU
# the trunk shapes of the GPU test (H, W): one pixel, a few, one ring-pair tile and one past it, one row and column past the
# 16 x 32 conv tile, 3 x 3 conv tiles
SHAPES = [(1, 1), (2, 3), (14, 30), (15, 31), (17, 33), (33, 65)]
RUNS = [(0, 1), (1, 1), (0, 2)]                               # (first_block, count)
_DEFAULT = Path("lo_rrdb", True, False)
# (id, FW_RRDB_* read at create, FW_PAIR_SLIDE per launch, dtypes, the f16 model): the engine paths of the GPU test
ENGINE_PATHS = [
    ("default", {}, None, ("f16", "bf16"), _DEFAULT),
    ("C5_WINO=2", {"FW_RRDB_C5_WINO": "2"}, None, ("f16",), Path("lo_rrdb", True, True)),                    # rdb3's residual-plane Winograd form
    ("C5_WINO=0", {"FW_RRDB_C5_WINO": "0"}, None, ("f16",), Path("lo_rrdb", False, False)),                  # the direct split kernel everywhere
    ("LO=0", {"FW_RRDB_LO": "0"}, None, ("f16", "bf16"), Path("lo_all", False, False)),                      # n_id 2 / 6: residual planes keep conv5 off Winograd
    ("SPLIT_TRUNK=0", {"FW_RRDB_SPLIT_TRUNK": "0"}, None, ("f16", "bf16"), Path("f32", False, False)),       # EPI_RESIDUAL with res1 / res2
    ("FUSE_PAIRS=0", {"FW_RRDB_FUSE_PAIRS": "0"}, None, ("f16",), _DEFAULT),                                 # one conv per launch, in place in the concat buffer
    ("FUSE_MASK=1", {"FW_RRDB_FUSE_MASK": "1"}, None, ("f16",), _DEFAULT),
    ("FUSE_MASK=2", {"FW_RRDB_FUSE_MASK": "2"}, None, ("f16",), _DEFAULT),
    ("PAIR_SLIDE=0", {}, "0", ("f16",), _DEFAULT),
    ("PAIR_SLIDE=1", {}, "1", ("f16",), _DEFAULT),
    ("PAIR_SLIDE=2", {}, "2", ("f16",), _DEFAULT),
]


def model_path(path: Path, rt: str) -> Path:
    """The Winograd kernel is f16 only."""
    return path if rt == "f16" else path._replace(wino12=False, wino3=False)


def model_paths():
    """The distinct (dtype, model) pairs behind ENGINE_PATHS."""
    return sorted({(rt, model_path(p, rt)) for _, _, _, dts, p in ENGINE_PATHS for rt in dts})


# ---- states and inputs -------------------------------------------------------------------------------------------------------------
def lively_state(bias_gain: float = 3.0):
    """Two RRDBs with conv5 unshrunk (PyTorch's default initialisation) and the growth convs' biases `bias_gain` times the default, so
    that LeakyReLU's negative branch carries a sizeable share of every growth plane (asserted on the host: 20 .. 80 %)."""
    from framewright_amd.synth import synthetic_rrdbnet_state
    sd = synthetic_rrdbnet_state(NUM_BLOCK, SCALE, seed=2024, conv5_scale=1.0)
    for k in sd:
        if k.startswith("body.") and k.endswith(".bias") and ".conv5." not in k:
            sd[k] = (sd[k] * np.float32(bias_gain)).astype(np.float32)
    return sd


def trunk_only_state():
    sd = lively_state()
    for k in sd:
        if ".conv5." in k:
            sd[k] = np.zeros_like(sd[k])
    return sd


def block_weights(sd, b: int):
    """[rdb][conv] -> (weight fp32 [cout][cin][3][3], bias fp32) of RRDB b."""
    return [[(np.asarray(sd[f"body.{b}.rdb{r}.conv{c}.weight"], np.float32), np.asarray(sd[f"body.{b}.rdb{r}.conv{c}.bias"], np.float32))
             for c in range(1, 6)] for r in range(1, 4)]


def lively_trunk(H: int, W: int, seed: int) -> np.ndarray:
    """fp32 (H, W, 64): both signs, magnitudes over five binades, and lo parts that are large in both operand types: every value lies
    (k + g) / 8 of a bf16 spacing beside a bf16 number, k in {2, 3} and g in [0.25, 0.75] - 0.28 .. 0.47 of a bf16 spacing from the
    nearest bf16 and, a bf16 spacing being eight of f16, at least 0.25 of an f16 spacing from the nearest f16."""
    rng = np.random.default_rng([H, W, seed])
    h = round_to(rng.choice([-1.0, 1.0], (H, W, 64)) * np.exp2(rng.uniform(-3.0, 2.0, (H, W, 64))), "bf16")
    f = (rng.integers(2, 4, (H, W, 64)) + rng.uniform(0.25, 0.75, (H, W, 64))) / 8.0 * rng.choice([-1.0, 1.0], (H, W, 64))
    return (h + f * typed_ulp(h * (1 - 2.0 ** -12), "bf16")).astype(np.float32)     # (the spacing below a power of two is half of that above)


# ---- the block ---------------------------------------------------------------------------------------------------------------------
def _conv(x, w, b):
    """conv3x3 (zero pad 1) + bias in float64: x (H, W, Cin), w (Cout, Cin, 3, 3)."""
    t = F.conv2d(torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(2, 0, 1)[None], torch.from_numpy(np.ascontiguousarray(w, np.float64)),
                 torch.from_numpy(np.ascontiguousarray(b, np.float64)), padding=1)
    return t[0].permute(1, 2, 0).contiguous().numpy()


def _lrelu(t, slope):
    return np.maximum(t, slope * t)


def rrdb(x, weights):
    """One RRDB exactly: x (H, W, 64) float64, weights = block_weights(sd, b).  Returns (y, [x1 .. x4] of rdb3)."""
    x = np.asarray(x, np.float64)
    cur, growth = x, None
    for k in range(3):
        cat = [cur]
        for c in range(4):
            w, b = weights[k][c]
            cat.append(_lrelu(_conv(np.concatenate(cat, 2), w, b), 0.2))
        w, b = weights[k][4]
        cur = _conv(np.concatenate(cat, 2), w, b) * 0.2 + cur
        growth = cat[1:]
    return cur * 0.2 + x, growth


def run_exact(x, sd, first: int, count: int):
    y, growth = np.asarray(x, np.float64), None
    for b in range(first, first + count):
        y, growth = rrdb(y, block_weights(sd, b))
    return y, growth


class Trunk:
    """The trunk between two dense blocks as a path holds it: hi (typed values), lo (typed values or None: not stored), f32 (the fp32
    trunk or None).  ``value`` is what a residual add of the path reads."""

    def __init__(self, hi, lo=None, f32=None, y=None):
        self.hi, self.lo, self.f32, self.y = hi, lo, f32, y          # y: the fp32 value that hi / lo were split from

    @property
    def value(self):
        return self.f32 if self.f32 is not None else (self.hi if self.lo is None else self.hi + self.lo)


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _hi_lo(y, rt):
    """hi = T(y), lo = T(y - hi) of an fp32 y, as the conv epilogue writes them."""
    if rt == "f16":
        hi, lo = WR.split_hi_lo(y)
        return hi.astype(np.float64), lo.astype(np.float64)
    hi = round_to(y, rt)
    return hi, round_to(_f32(y) - hi, rt)


def lay_in(x, rt, path: Path) -> Trunk:
    """trunk_in_f32 in the engine's representation (fw_rrdbnet_run_rrdbs)."""
    x = _f32(x)
    if path.trunk == "f32":
        return Trunk(round_to(x, rt), None, x, x)
    return Trunk(*_hi_lo(x, rt), None, x)


def _conv5(cat, w, b, rt, wino):
    """conv5 + bias of the typed concat buffer (H, W, 192) at the rounding points of its kernel."""
    if wino:
        assert rt == "f16"
        return WR.winograd_emulation(cat.astype(np.float16), w, b)[0]
    if rt == "f16":
        return WR.split_contract(cat.astype(np.float16), w, b)[0]
    return _conv(cat, round_to(w, rt), b)


def rrdb_rounded(t_in: Trunk, weights, rt: str, path: Path, defect: str | None = None):
    """One RRDB at the rounding points of `path` (module docstring), from and to the path's trunk representation.  Returns
    (Trunk, [x1 .. x4] of rdb3 as the typed values of planes 2-5)."""
    assert defect is None or defect in DEFECTS + TRUNK_DEFECTS
    R, cur, growth = t_in, t_in, None
    for k in range(3):
        cat = [cur.hi]
        stored = []                                                   # what planes 2-5 hold
        for c in range(4):
            w, b = weights[k][c]
            src = list(cat)
            if defect == "pair34_plane_short" and c >= 2:             # the pair launched with na one short: x2's chunk is not contracted
                src[2] = np.zeros_like(src[2])
            t = _conv(np.concatenate(src, 2), round_to(w, rt), b)
            raw = t if (defect == "lrelu_missing_conv2" and c == 1) else _lrelu(t, S)
            xa = round_to(raw, rt)
            stored.append(xa)
            # the second conv of a pair (conv2, conv4) reads x_a from LDS: typed - unless the defect hands it the fp32 values
            cat.append(_f32(raw) if (defect == "xa_unrounded" and c in (0, 2)) else xa)
        cat = [cur.hi] + stored                                       # conv3 / conv5 read the planes
        if defect == "x3_in_x4_plane":                                # out_a of the second pair one plane up: x4 lands on it, x3's plane keeps zeros
            cat[3] = stored[2] = np.zeros_like(stored[2])
        w, b = weights[k][4]
        t5 = _conv5(np.concatenate(cat, 2), w, b, rt, path.wino3 if k == 2 else path.wino12)
        growth = stored
        cur = _stage(cur, R, k, t5, rt, path, defect)
    return cur, growth


def run_rounded(x, sd, first: int, count: int, rt: str, path: Path, defect: str | None = None):
    """What fw_rrdbnet_run_rrdbs returns on `path`, in the rounded model: (trunk_out, [x1 .. x4] of the last dense block)."""
    t, growth = lay_in(x, rt, path), None
    for b in range(first, first + count):
        t, growth = rrdb_rounded(t, block_weights(sd, b), rt, path, defect)
    return t.value, growth


def bounds(got, exact, rounded):
    """The yardstick of tests/test_nafblock_gpu.py: (max error, q, its limit 2 q + 1e-6 max |exact|, mean error, its limit)."""
    err, q = np.abs(got - exact).max(), np.abs(rounded - exact).max()
    merr, mq = np.abs(got - exact).mean(), np.abs(rounded - exact).mean()
    return err, q, 2 * q + 1e-6 * np.abs(exact).max(), merr, 2 * mq + 1e-6 * np.abs(exact).mean()


# ---- the trunk-only state: an elementwise model with a derived bound ---------------------------------------------------------------
def _e_hi(t: Trunk, ey, rt):
    """How far the engine's hi may sit from the model's when its fp32 y is within ey of the model's: rounding is monotone, so the
    engine's hi lies between T(y - ey) and T(y + ey).  Zero wherever both are the model's hi: no flip is possible there."""
    return np.maximum(np.abs(round_to(t.y + ey, rt) - t.hi), np.abs(round_to(t.y - ey, rt) - t.hi))


def _e_value(t: Trunk, ey, rt):
    """The same for hi + lo.  |out_e - out_m| <= |out_e - y_e| + |y_e - y_m| + |y_m - out_m|, and hi + lo is within half a spacing of
    its own lo of its own y.  Where no flip of hi is possible the engine's lo is within ey of the model's; where one is, |lo| is at
    most half a spacing of y."""
    lo = np.abs(t.lo)
    tight = 0.5 * typed_ulp(lo, rt) + 0.5 * typed_ulp(lo + ey, rt)
    loose = typed_ulp(0.5 * typed_ulp(np.abs(t.y) + ey, rt), rt)
    return np.where(ey > 0, ey + np.where(_e_hi(t, ey, rt) > 0, loose, tight), 0.0)


def trunk_only_run(x, count: int, rt: str, path: Path, defect: str | None = None):
    """`count` RRDBs of the trunk-only state on `path`: (trunk_out, per-element bound on |engine - trunk_out|) - module docstring."""
    t = lay_in(x, rt, path)
    ey = np.zeros(np.shape(x))                         # bound on |engine's fp32 y - the model's|; the lay-in is a conversion both perform alike
    for _ in range(count):
        R, eyR, cur, eyc = t, ey, t, ey
        for k in range(3):
            last = k == 2
            if path.trunk == "f32":
                if last:
                    eyc = S * eyc + eyR + gamma(2) * (S * np.abs(cur.f32) + np.abs(R.f32))
            else:
                lo_all = path.trunk == "lo_all"
                terms = [5.0 * cur.hi] + ([5.0 * cur.lo] if lo_all else []) + ([25.0 * R.hi, 25.0 * R.lo] if last else [])
                s1 = S_RDB3 if last else S
                e_in = 5.0 * (_e_value(cur, eyc, rt) if lo_all else _e_hi(cur, eyc, rt)) + (25.0 * _e_value(R, eyR, rt) if last else 0.0)
                eyc = s1 * e_in + (gamma(len(terms)) * s1 * sum(np.abs(v) for v in terms) if len(terms) > 1 else 0.0)
            cur = _stage(cur, R, k, 0.0, rt, path, defect)
        t, ey = cur, eyc
    return t.value, ey if path.trunk == "f32" else _e_value(t, ey, rt)


def _stage(cur: Trunk, R: Trunk, k: int, t5, rt: str, path: Path, defect: str | None) -> Trunk:
    """conv5's residual stage of rdb k (0 .. 2): from conv5 + bias (t5; 0 in the trunk-only state), the dense block's input `cur` and
    the RRDB's input `R` to the dense block's output, in the path's representation."""
    last = k == 2
    if path.trunk == "f32":
        y = S * t5 + (R.f32 if (last and defect == "rdb3_res_from_rrdb_in") else cur.f32)
        if last:
            y = y * S + R.f32
        y = _f32(y)
        return Trunk(round_to(y, rt), None, y, y)
    lo_all = path.trunk == "lo_all"
    x_res = cur.hi + cur.lo if (lo_all and not (defect == "rdb1_lo_dropped" and k == 1)) else cur.hi
    s1 = S_RDB3 if last else S
    if last:
        Rsrc = cur if defect == "r_from_cur" else R
        r_lo = Rsrc.lo if Rsrc.lo is not None else 0.0
        if defect == "rdb3_res_from_rrdb_in":
            x_res = R.hi + R.lo if lo_all else R.hi
        if defect == "rdb3_s1":
            s1 = S
        acc = t5 + 5.0 * x_res + 25.0 * Rsrc.hi + (0.0 if defect == "r_lo_dropped" else (5.0 if defect == "r_lo_scale5" else 25.0) * r_lo)
    else:
        acc = t5 + 5.0 * x_res
    y = _f32(s1 * acc)
    if last or lo_all:
        hi, lo = _hi_lo(y, rt)
        if last and defect == "out_lo_unwritten":
            lo = np.zeros_like(lo)
        return Trunk(hi, lo, None, y)
    return Trunk(round_to(y, rt), None, None, y)
