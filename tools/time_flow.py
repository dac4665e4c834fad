#!/usr/bin/env python3
"""Dense Farneback optical flow on the device (csrc/optical_flow.hip): ms per 1080p and per 4K flow (fw_farneback_flow_u8 alone, and
with the statistics / percentiles / weight map the denoise needs), and ms per flow-compensated output frame at temporal_radius = 3
(six flows, `DeviceTemporalAccumulator(flow_estimator=...)._window_device`, frames resident).  Medians of N >= 20 after warm-up, each
sample a host clock around work that ends in a device synchronise.  Written to profiles/flow_timing.json with the bytes the
algorithm has to move on paper (every pass reads its inputs and writes its outputs once; halos, the bilinear gather's overlap and
the two device sorts are not counted) and the HBM rate that implies, as a fraction of the ~6.3 TB/s a streaming kernel reaches.
There is no earlier device implementation and no OpenCV here to race: the numbers are a record, not a bar.

  python tools/time_flow.py [--samples 30] [--out profiles/flow_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ACHIEVABLE_TBPS = 6.3


def paper_bytes(h, w, channels=3, levels=3, pyr_scale=0.5, iterations=3):
    """Bytes over HBM for one flow if every kernel of csrc/optical_flow.hip read its inputs and wrote its outputs exactly once."""
    scale, usable = 1.0, 0
    while usable < levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        usable += 1
    n_full, total, n_prev, per_level = h * w, 0, 0, []
    for k in range(usable, -1, -1):
        s = pyr_scale ** k
        n = int(round(h * s)) * int(round(w * s))
        b = 2 * (n_full * channels + 4 * n_full)                       # gray + blur of both frames at full resolution
        if k:
            b += 2 * (4 * min(n_full, 4 * n) + 4 * n)                  # resize to the level
        b += 2 * (4 * n + 20 * n)                                      # polynomial expansion
        b += 40 * n + 8 * n_prev + 20 * n                              # first matrices (+ the coarser flow)
        b += (iterations - 1) * 80 * n + 28 * n                        # box mean + solve (+ next matrices); the last stores the flow
        per_level.append({"k": k, "pixels": n, "bytes": b})
        total += b
        n_prev = n
    return total, per_level


def median_ms(fn, samples, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "flow_timing.json"))
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples must be at least 20")
    import torch
    from framewright_amd import build as fw_build
    from framewright_amd import temporal_denoise as TD
    from framewright_amd.synth import synthetic_frames
    if not torch.cuda.is_available():
        raise SystemExit("time_flow.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    est = TD.DeviceFlowEstimator()
    acc = TD.DeviceTemporalAccumulator(flow_estimator=est)
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "samples": args.samples,
              "achievable_tbps": ACHIEVABLE_TBPS, "sizes": {}}
    for name, (h, w) in {"1080p": (1080, 1920), "4k": (2160, 3840)}.items():
        frames = [torch.from_numpy(f.copy()).to(dev) for f in synthetic_frames(7, h, w, seed=4)]
        nbytes, per_level = paper_bytes(h, w)
        flow = median_ms(lambda: est.flow_device(frames[0], frames[3]), args.samples)
        maps = median_ms(lambda: est.maps_device(frames[0], frames[3], weight_map=True), args.samples)
        window = median_ms(lambda: acc._window_device(3, frames), args.samples)
        tbps = nbytes / (flow[0] * 1e-3) / 1e12
        result["sizes"][name] = {
            "height": h, "width": w, "paper_bytes_per_flow": nbytes, "paper_bytes_per_level": per_level,
            "flow_ms": {"median": flow[0], "min": flow[1], "max": flow[2]},
            "flow_with_stats_and_weights_ms": {"median": maps[0], "min": maps[1], "max": maps[2]},
            "radius3_output_frame_ms": {"median": window[0], "min": window[1], "max": window[2]},
            "implied_tbps": tbps, "fraction_of_achievable_hbm": tbps / ACHIEVABLE_TBPS,
        }
        print(f"{name}: flow {flow[0]:.3f} ms ({nbytes / 1e6:.0f} MB on paper -> {tbps:.2f} TB/s, {100 * tbps / ACHIEVABLE_TBPS:.0f} % of {ACHIEVABLE_TBPS}), "
              f"with stats {maps[0]:.3f} ms, radius-3 output frame {window[0]:.3f} ms", flush=True)
        del frames
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
