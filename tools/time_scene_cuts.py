#!/usr/bin/env python3
"""Scene-cut detection on the device (csrc/scene_cuts.hip), at 1080p, medians of `--samples` (20):

  - ms per pair of fw_scene_ssim_u8 on the 49 pairs of a resident 50-frame batch, and of one pair alone; ms per frame of
    fw_hist64x3_u8 on the batch; next to a `clone()` of the same batch timed in the same run (alternating), and their ratios: a
    clone reads and writes the batch once, the SSIM reads two frames per pair (its bound: about one clone per pair), the histogram
    one frame per frame (about half a clone);
  - seconds of `FrameInterpolator.detect_all_scene_changes` on a 16-frame PNG directory with `device_scene_detection` off and on;
  - seconds of `FrameInterpolator.interpolate` x2 on the same directory with the flag off and on (synthetic IFNet weights).

Each sample is a host clock around work that ends in a device synchronise.  Nothing is gated on these numbers: they are a record.
Written to profiles/scene_cuts_timing.json with the digest of the build they were measured on.

  python tools/time_scene_cuts.py [--samples 20] [--dir-samples 20] [--out profiles/scene_cuts_timing.json]

`--dir-samples` is the number of runs of the two directory measurements (seconds each: PNG decoding and encoding on the host).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

H, W, BATCH, CLIP = 1080, 1920, 50, 16


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn):
    import torch
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--dir-samples", type=int, default=20)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "scene_cuts_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from framewright_amd import _lib
    from framewright_amd import build as fw_build
    from framewright_amd import rife as RF
    from framewright_amd.realesrgan import _imwrite
    from framewright_amd.synth import synthetic_frames, synthetic_ifnet_state
    if not torch.cuda.is_available():
        raise SystemExit("time_scene_cuts.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "samples": args.samples}

    base = list(synthetic_frames(CLIP, H, W, seed=4))
    base[CLIP // 2:] = [255 - f[::-1] for f in base[CLIP // 2:]]            # one hard cut in the middle
    batch = torch.from_numpy(np.stack([base[k % CLIP] for k in range(BATCH)])).to(dev)
    pairs = BATCH - 1
    ssim = torch.empty(pairs, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.fw_scene_ssim_workspace_bytes(pairs, H, W) // 8, dtype=torch.float64, device=dev)
    hist = torch.empty((BATCH, 3, 64), dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    ssim_batch = lambda: _lib.check(lib.fw_scene_ssim_u8(p(batch[0]), p(batch[1]), H * W * 3, pairs, H, W, p(ssim), p(ws), st))
    ssim_one = lambda: _lib.check(lib.fw_scene_ssim_u8(p(batch[0]), p(batch[1]), 0, 1, H, W, p(ssim), p(ws), st))
    hists = lambda: _lib.check(lib.fw_hist64x3_u8(p(batch), BATCH, H, W, p(hist), st))
    for _ in range(3):
        ssim_batch(), ssim_one(), hists(), batch.clone()
    torch.cuda.synchronize()
    batch_ms, one_ms, hist_ms, clone_ms = [], [], [], []
    for _ in range(args.samples):
        batch_ms.append(timed(ssim_batch)[0] / pairs)
        one_ms.append(timed(ssim_one)[0])
        hist_ms.append(timed(hists)[0] / BATCH)
        clone_ms.append(timed(lambda: batch.clone())[0] / BATCH)
    med = statistics.median
    frame_gb = H * W * 3 / 1e9
    result["kernels"] = {"batch": BATCH, "ssim_ms_per_pair_in_batch": summary(batch_ms), "ssim_ms_one_pair_alone": summary(one_ms),
                         "hist_ms_per_frame": summary(hist_ms), "clone_ms_per_frame": summary(clone_ms),
                         "ssim_ratio_to_clone": med(batch_ms) / med(clone_ms), "hist_ratio_to_clone": med(hist_ms) / med(clone_ms),
                         "ssim_read_gb_per_s": 2 * frame_gb / (med(batch_ms) * 1e-3), "hist_read_gb_per_s": frame_gb / (med(hist_ms) * 1e-3),
                         "clone_read_plus_write_gb_per_s": 2 * frame_gb / (med(clone_ms) * 1e-3)}
    print(f"SSIM {med(batch_ms):.4f} ms per pair in the batch ({result['kernels']['ssim_ratio_to_clone']:.2f} x clone), {med(one_ms):.4f} ms "
          f"alone; histograms {med(hist_ms):.4f} ms per frame ({result['kernels']['hist_ratio_to_clone']:.2f} x clone); clone "
          f"{med(clone_ms):.4f} ms per frame", flush=True)
    del batch

    os.environ["FRAMEWRIGHT_AMD_SYNTHETIC_WEIGHTS"] = "1"
    eng = RF.IFNetEngine("f16")
    eng.load_state_dict(synthetic_ifnet_state())
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "in"
        src.mkdir()
        for k, f in enumerate(base):
            _imwrite(src / f"frame_{k + 1:08d}.png", f)
        cfg = lambda: RF.InterpolationConfig(target_fps=48, smoothness="low", scene_threshold=0.3)
        runs = {"host": RF.FrameInterpolator(config=cfg(), engine=eng),
                "device": RF.FrameInterpolator(config=cfg(), engine=eng, device_scene_detection=True)}
        n_detect = args.dir_samples
        detect, interp, bounds = {k: [] for k in runs}, {k: [] for k in runs}, {}
        for k, fi in runs.items():                                        # warm-up
            fi.detect_all_scene_changes(src)
            fi.interpolate(src, Path(tmp) / f"warm_{k}", 24.0, 48)
        for i in range(n_detect):
            for k, fi in runs.items():
                t, b = timed(lambda: fi.detect_all_scene_changes(src))
                detect[k].append(t / 1e3)
                bounds[k] = b
                interp[k].append(timed(lambda: fi.interpolate(src, Path(tmp) / f"out_{k}", 24.0, 48))[0] / 1e3)
        result["directory"] = {"frames": CLIP, "runs": n_detect, "boundaries": bounds,
                               "detect_all_scene_changes_s": {k: summary(v) for k, v in detect.items()},
                               "interpolate_x2_s": {k: summary(v) for k, v in interp.items()}}
        print(f"{CLIP}-frame PNG directory: detect_all_scene_changes {med(detect['host']):.3f} s on the host, {med(detect['device']):.3f} s "
              f"with device_scene_detection; interpolate x2 {med(interp['host']):.3f} s / {med(interp['device']):.3f} s", flush=True)
    eng.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
