#!/usr/bin/env python3
"""Flicker reduction on the device (csrc/flicker.hip), at 1080p, medians of `--samples` (20):

  - ms per frame of fw_lab_l_sums_u8 and of fw_deflicker_lab_u8 on a resident 50-frame batch, next to a `clone()` of the same
    batch timed in the same run (alternating), and their ratios: a clone reads and writes the batch once, which is the bound of
    the fused kernel; the sums only read it;
  - ms per frame of `DeviceFlickerReducer.deflicker_batch_device` (sums, one wait, the maps built on the host, upload, fused kernel);
  - ms per frame of `DeviceTemporalDenoiser.denoise_clip` at the defaults on a 16-frame clip with and without `device_flicker`.

Each sample is a host clock around work that ends in a device synchronise.  Nothing is gated on these numbers: they are a record.
Written to profiles/flicker_timing.json with the digest of the build they were measured on.

  python tools/time_flicker.py [--samples 20] [--out profiles/flicker_timing.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

H, W, BATCH, CLIP = 1080, 1920, 50, 16


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def timed(fn):
    import torch
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "flicker_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from framewright_amd import _lib
    from framewright_amd import build as fw_build
    from framewright_amd import temporal_denoise as TD
    from framewright_amd.synth import synthetic_frames
    if not torch.cuda.is_available():
        raise SystemExit("time_flicker.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "samples": args.samples}

    base = synthetic_frames(CLIP, H, W, seed=4)
    gains = [1.0, 0.7, 0.9, 0.6]
    batch = torch.from_numpy(np.stack([np.clip(np.rint(base[k % CLIP] * gains[k % 4]), 0, 255).astype(np.uint8) for k in range(BATCH)])).to(dev)
    out = torch.empty_like(batch)
    sums = torch.empty(BATCH, dtype=torch.int64, device=dev)
    luts = torch.from_numpy(np.stack([np.clip(np.arange(256) + (k % 21) - 10, 0, 255).astype(np.uint8) for k in range(BATCH)])).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    l_sums = lambda: _lib.check(lib.fw_lab_l_sums_u8(p(batch), BATCH, H, W, p(sums), st))
    fused = lambda: _lib.check(lib.fw_deflicker_lab_u8(p(batch), BATCH, H, W, p(luts), p(out), st))
    reducer = TD.DeviceFlickerReducer()
    whole = lambda: reducer.deflicker_batch_device(batch, 110.0, out=out)
    for _ in range(3):
        l_sums(), fused(), whole(), batch.clone()
    torch.cuda.synchronize()
    sums_ms, fused_ms, whole_ms, clone_ms = [], [], [], []
    for _ in range(args.samples):
        sums_ms.append(timed(l_sums)[0] / BATCH)
        fused_ms.append(timed(fused)[0] / BATCH)
        whole_ms.append(timed(whole)[0] / BATCH)
        clone_ms.append(timed(lambda: batch.clone())[0] / BATCH)
    med = statistics.median
    result["kernels"] = {"batch": BATCH, "l_sums_ms_per_frame": summary(sums_ms), "deflicker_ms_per_frame": summary(fused_ms),
                         "reducer_batch_ms_per_frame": summary(whole_ms), "clone_ms_per_frame": summary(clone_ms),
                         "l_sums_ratio_to_clone": med(sums_ms) / med(clone_ms), "deflicker_ratio_to_clone": med(fused_ms) / med(clone_ms)}
    print(f"L sums {med(sums_ms):.4f} ms per frame ({result['kernels']['l_sums_ratio_to_clone']:.1f} x clone), fused deflicker "
          f"{med(fused_ms):.4f} ({result['kernels']['deflicker_ratio_to_clone']:.1f} x clone), reducer batch {med(whole_ms):.4f}, clone "
          f"{med(clone_ms):.4f}", flush=True)
    del batch, out

    clip = [np.clip(np.rint(f * gains[k % 4]), 0, 255).astype(np.uint8) for k, f in enumerate(base)]
    plain, flick = TD.DeviceTemporalDenoiser(), TD.DeviceTemporalDenoiser(device_flicker=True)
    plain.denoise_clip(clip), flick.denoise_clip(clip)                       # warm-up
    plain_ms, flick_ms = [], []
    for _ in range(args.samples):
        plain_ms.append(timed(lambda: plain.denoise_clip(clip))[0] / CLIP)
        t, (_, res) = timed(lambda: flick.denoise_clip(clip))
        flick_ms.append(t / CLIP)
    result["denoise_clip"] = {"frames": CLIP, "flicker_reduction_applied": res.flicker_reduction_applied,
                              "without_device_flicker_ms_per_frame": summary(plain_ms), "with_device_flicker_ms_per_frame": summary(flick_ms)}
    print(f"denoise_clip, {CLIP} frames: {med(plain_ms):.2f} ms per frame without device_flicker, {med(flick_ms):.2f} with", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
