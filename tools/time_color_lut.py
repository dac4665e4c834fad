#!/usr/bin/env python3
"""The colour grade on the device (csrc/color_lut.hip) on synthetic frames, medians of `--samples` (20):

  - ms per frame of fw_lut3d_apply_u8 / _u16 at 1920 x 1080 and 7680 x 4320 for table sizes 17 (held in LDS), 33 and 65 (read
    through L2), on one frame and on a batch, out of place and in place, next to a `clone()` of the same tensor timed in the same
    run (alternating): a clone reads and writes the same bytes once, which is the bound the kernel is judged against;
  - ms per frame of the reference-shaped NumPy path (tests/color_lut_ref.py) on the same machine, at 1080p only;
  - seconds of `DeviceColorGrader.grade_directory` on 16 PNGs of 1080p against the host loop (read, NumPy grade, write).

Each sample is a host clock around work that ends in a device synchronise; every section runs under its own time limit.  Nothing
is gated on these numbers: they are a record.  Written to profiles/color_lut_timing.json with the digest of the build.

  python tools/time_color_lut.py [--samples 20] [--out profiles/color_lut_timing.json]
"""
import argparse
import json
import signal
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SHAPES = {"1080p": (1080, 1920, 8), "8k": (4320, 7680, 2)}        # height, width, frames of the batch
TABLES = (17, 33, 65)


class SectionTimeout(Exception):
    pass


def limited(seconds, fn):
    """Run fn() under an alarm: a section that exceeds its limit is recorded as such and the tool goes on."""
    def handler(signum, frame):
        raise SectionTimeout()
    old = signal.signal(signal.SIGALRM, handler)
    signal.alarm(seconds)
    try:
        return fn()
    except SectionTimeout:
        return {"timed_out_after_s": seconds}
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "color_lut_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import color_lut_ref as R
    from framewright_amd import build as fw_build
    from framewright_amd import color_grade as G
    from framewright_amd.realesrgan import _imwrite
    if not torch.cuda.is_available():
        raise SystemExit("time_color_lut.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    med = statistics.median
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "samples": args.samples, "kernels": {}}
    graders = {s: G.DeviceColorGrader(G.create_seasonal_lut("autumn", 0.7, s)) for s in TABLES}
    gen = torch.Generator(device=dev).manual_seed(1)

    def kernels(name, h, w, batch, dtype):
        rec = {}
        for n in (1, batch):
            if dtype == torch.uint8:
                clip = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
            else:
                clip = torch.randint(-32768, 32768, (n, h, w, 3), dtype=torch.int16, device=dev, generator=gen)
            work = clip.clone()
            for size, g in graders.items():
                for _ in range(3):
                    g.apply_device(clip), g.apply_device(work, inplace=True), clip.clone()
                torch.cuda.synchronize()
                t = {"out_of_place": [], "in_place": [], "clone": []}
                for _ in range(args.samples):
                    t["out_of_place"].append(timed(lambda: g.apply_device(clip)) / n)
                    t["clone"].append(timed(lambda: clip.clone()) / n)
                    t["in_place"].append(timed(lambda: g.apply_device(work, inplace=True)) / n)
                r = {k + "_ms_per_frame": summary(v) for k, v in t.items()}
                r["ratio_to_clone"] = med(t["out_of_place"]) / med(t["clone"])
                r["in_place_ratio_to_clone"] = med(t["in_place"]) / med(t["clone"])
                rec[f"n{n}_table{size}"] = r
                print(f"{name} {str(dtype)[6:]} n = {n} table {size}: {med(t['out_of_place']):.4f} ms per frame, in place "
                      f"{med(t['in_place']):.4f}, clone {med(t['clone']):.4f}", flush=True)
            del clip, work
        return rec

    for name, (h, w, batch) in SHAPES.items():
        for dtype in (torch.uint8, torch.int16):
            key = f"{name}_{'uint8' if dtype == torch.uint8 else 'uint16'}"
            result["kernels"][key] = limited(120, lambda: kernels(name, h, w, batch, dtype))

    def host_numpy():
        tab = G.create_seasonal_lut("autumn", 0.7, 33).table_f32()
        img = R.test_image(1080, 1920, np.uint8)[0]
        v = []
        for _ in range(3):
            t0 = time.perf_counter()
            R.apply_lut3d(img, tab)
            v.append((time.perf_counter() - t0) * 1e3)
        return {"height": 1080, "width": 1920, "table": 33, "ms_per_frame": summary(v)}

    result["host_numpy_1080p"] = limited(180, host_numpy)
    print("host NumPy:", result["host_numpy_1080p"], flush=True)

    def directory():
        tab = G.create_seasonal_lut("autumn", 0.7, 33).table_f32()
        frames = R.test_image(1080, 1920, np.uint8, n=16, seed=1)
        rec = {"frames": 16, "height": 1080, "width": 1920}
        with tempfile.TemporaryDirectory() as d:
            d = Path(d)
            for k, f in enumerate(frames):
                _imwrite(d / f"frame_{k:08d}.png", f)
            t0 = time.perf_counter()
            G.DeviceColorGrader.grade_directory(d, "autumn", 0.7)
            rec["grade_directory_s"] = time.perf_counter() - t0
            for k, f in enumerate(frames):
                _imwrite(d / f"frame_{k:08d}.png", f)
            t0 = time.perf_counter()
            for path in sorted(d.glob("*.png")):
                _imwrite(path, R.apply_lut3d(G._read_png_bgr(path), tab))
            rec["host_loop_s"] = time.perf_counter() - t0
        return rec

    result["directory_16_png"] = limited(240, directory)
    print("directory:", result["directory_16_png"], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
