#!/usr/bin/env python3
"""Diagnostic (build with FW_EXTRA_CXXFLAGS=-DFW_PAIR_STAMP): cycles per phase of one tile of the window pair kernel
(csrc/conv3x3_pair_slide.hip, its ST_* slots), wave by wave, at the two pair shapes of RRDBNet on one 1080p frame, and the same
for one warm-up.  A stamped build is slower than the product build (every stamp is an s_memtime behind two scheduling
barriers): read the table for where the cycles go, not for the launch time."""
import ctypes as C
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np, torch
from framewright_amd import build as B
B.build()
from framewright_amd import _lib

H, W, LAUNCHES = 1080, 1920, 20
TILE = ["barrier", "shared items", "x_a item", "x_a tile -> LDS", "tile set-up", "vmcnt waits", "x_a convert+store",
        "x_b convert+store", "carry copy", "first-stage wait"]
WARM = ["barrier", "MFMAs / items", "DMA wait", "convert -> carry", "set-up + DMA issue"]
lib = _lib.load()
dt = _lib.FW_DTYPE_F16
buf = (C.c_ulonglong * 128)()
p = lambda t: C.c_void_p(t.data_ptr())


def pack(w, ch):
    n = lib.fw_pack_conv3x3(dt, None, 32, w.shape[1], 1, ch, None)
    dst = np.zeros(n, np.uint16)
    wc = np.ascontiguousarray(w, np.float32)
    lib.fw_pack_conv3x3(dt, C.c_void_p(wc.ctypes.data), 32, w.shape[1], 1, ch, C.c_void_p(dst.ctypes.data))
    return torch.from_numpy(dst.view(np.int16)).cuda()


tiles_x, tiles_y = (W + 29) // 30, (H + 16) // 16
ntiles = tiles_x * tiles_y
ncu = torch.cuda.get_device_properties(0).multi_processor_count
nwarm = sum(1 for b in range(ncu) if (b * ntiles // ncu) % tiles_y)
print(f"{H} x {W}: {tiles_x} x {tiles_y} = {ntiles} tiles, {ncu} workgroups, {nwarm} of them start with a warm-up")
for na in (2, 4):
    rng = np.random.default_rng(na)
    cin = 32 * na
    x = torch.from_numpy(rng.standard_normal((na, H, W, 32)).astype(np.float32)).cuda().half()
    pa = pack((rng.standard_normal((32, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32), na)
    pb = pack((rng.standard_normal((32, cin + 32, 3, 3)) / np.sqrt(9 * (cin + 32))).astype(np.float32), na + 1)
    ta, tb = torch.zeros(32, device="cuda"), torch.zeros(32, device="cuda")
    oa, ob = torch.empty((H, W, 32), dtype=torch.half, device="cuda"), torch.empty((H, W, 32), dtype=torch.half, device="cuda")
    run = lambda: _lib.check(lib.fw_conv3x3_pair_nhwc(dt, p(x), 32, H * W * 32, na, H, W, p(pa), p(ta), p(pb), p(tb), p(oa), p(ob), 32, None))
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    lib.fw_debug_stamps(0, buf)  # reads and clears
    for _ in range(LAUNCHES):
        run()
    torch.cuda.synchronize()
    lib.fw_debug_stamps(0, buf)
    v = np.array(list(buf), dtype=np.float64).reshape(8, 16)
    clock = v[:, :15].sum(1) / v[:, 15] * 0.1
    tile = v[:, :10] / (ntiles * LAUNCHES)
    warm = v[:, 10:15] / (max(nwarm, 1) * LAUNCHES)
    items = tile[:, 1] + tile[:, 2]
    print(f"\nna = {na} ({cin} -> 32 / {cin + 32} -> 32): cycles per tile ({na} shared items + the x_a item), clock {clock.mean():.2f} GHz")
    print("  wave " + "".join(f"{n:>19}" for n in TILE) + f"{'non-item total':>19}")
    for w in range(8):
        print(f"  {w:4d} " + "".join(f"{c:19.0f}" for c in tile[w]) + f"{tile[w].sum() - items[w]:19.0f}")
    slow, fast = int(np.argmin(tile[:, 0] + tile[:, 9])), int(np.argmax(tile[:, 0] + tile[:, 9]))
    print(f"  slowest wave (least barrier wait) {slow}: {tile[slow].sum():.0f} per tile, {tile[slow].sum() - items[slow]:.0f} outside the items, "
          f"{tile[slow].sum() - items[slow] - tile[slow, 0] - tile[slow, 9]:.0f} of it not waiting at a barrier; fastest wave {fast}: "
          f"{tile[fast].sum() - items[fast]:.0f} outside the items, {tile[fast, 0] + tile[fast, 9]:.0f} of it at barriers")
    print(f"  one warm-up ({na} chunks), cycles:")
    print("  wave " + "".join(f"{n:>19}" for n in WARM) + f"{'total':>19}")
    for w in range(8):
        print(f"  {w:4d} " + "".join(f"{c:19.0f}" for c in warm[w]) + f"{warm[w].sum():19.0f}")
