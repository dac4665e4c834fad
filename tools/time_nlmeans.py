#!/usr/bin/env python3
"""Non-local-means spatial denoise on the device (csrc/nlmeans.hip): ms per 1080p and per 4K frame of the L-plane core (C = 1), the
ab-plane core (C = 2) and the whole coloured call (fw_nlmeans_colored_u8: Lab split, two cores, merge) at h = 6 and h = 10, and ms
per flow-compensated output frame at temporal_radius = 3 with and without the spatial step (frames resident; "without" is
`_window_device` alone, the figure profiles/flow_timing.json calls radius3_output_frame_ms).  Medians of N >= 20 after warm-up, each
sample a host clock around work that ends in a device synchronise.  Written to profiles/nlmeans_timing.json.

Next to each core time: the integer operations per pixel-offset the kernel executes ON PAPER (counted from the source, see
`paper_ops`) and the fraction of the chip's VALU issue rate that implies.  There is no earlier device implementation and no OpenCV
here to race: the numbers are a record, not a bar.

  python tools/time_nlmeans.py [--samples 30] [--out profiles/nlmeans_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# 256 CUs x 4 SIMDs x 32 lanes per clock at ~2.4 GHz: lane-operations per second the vector ALUs can issue
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
ROWS, TEMPLATE, SEARCH = 16, 7, 21


def paper_ops(channels, template=TEMPLATE):
    """Integer vector operations per pixel-offset.  A lane walks ROWS + template - 1 rows for ROWS outputs and 64 lanes produce
    64 - (template - 1) columns.  Per walked row: per channel two byte extracts, a subtract and a multiply-add; four adds for the
    horizontal sum (the lane permutes and the LDS read are not VALU work); two for the running vertical sum.  Per output row: a
    shift and a min for the index, an add for the weight sum, per channel a byte extract and a multiply-add."""
    th2 = template - 1
    per_walked = 4 * channels + 4 + 2
    per_output = 3 + 2 * channels
    return (per_walked * (ROWS + th2) / ROWS + per_output) * 64.0 / (64 - th2)


def median_ms(fn, samples, warmup=3):
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
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "nlmeans_timing.json"))
    args = ap.parse_args()
    if args.samples < 20:
        ap.error("--samples must be at least 20")
    import torch
    from framewright_amd import build as fw_build
    from framewright_amd import temporal_denoise as TD
    from framewright_amd.synth import synthetic_frames
    if not torch.cuda.is_available():
        raise SystemExit("time_nlmeans.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    est = TD.DeviceFlowEstimator()
    acc = TD.DeviceTemporalAccumulator(flow_estimator=est)
    sd = TD.DeviceSpatialDenoiser()
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "samples": args.samples,
              "template_window": TEMPLATE, "search_window": SEARCH, "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S, "sizes": {}}
    for name, (h, w) in {"1080p": (1080, 1920), "4k": (2160, 3840)}.items():
        frames = [torch.from_numpy(f.copy()).to(dev) for f in synthetic_frames(7, h, w, seed=4)]
        lplane = frames[0][:, :, 1].contiguous()
        abplane = frames[0][:, :, :2].contiguous()
        entry = {"height": h, "width": w}
        for hh in (6, 10):
            row = {}
            for key, plane, c in (("l_core_ms", lplane, 1), ("ab_core_ms", abplane, 2)):
                t = median_ms(lambda: sd.nlmeans_device(plane, hh), args.samples)
                ops = paper_ops(c)
                t["paper_int_ops_per_pixel_offset"] = ops
                t["fraction_of_valu_issue_rate"] = ops * h * w * SEARCH * SEARCH / (t["median"] * 1e-3) / VALU_LANE_OPS_PER_S
                row[key] = t
            row["colored_ms"] = median_ms(lambda: sd.denoise_device(frames[0], hh), args.samples)
            entry[f"h{hh}"] = row
            print(f"{name} h={hh}: L core {row['l_core_ms']['median']:.3f} ms ({100 * row['l_core_ms']['fraction_of_valu_issue_rate']:.0f} % of VALU issue), "
                  f"ab core {row['ab_core_ms']['median']:.3f} ms ({100 * row['ab_core_ms']['fraction_of_valu_issue_rate']:.0f} %), "
                  f"coloured call {row['colored_ms']['median']:.3f} ms", flush=True)
        entry["radius3_output_frame_ms"] = median_ms(lambda: acc._window_device(3, frames), args.samples)
        entry["radius3_output_frame_with_spatial_h6_ms"] = median_ms(lambda: sd.denoise_device(acc._window_device(3, frames), 6), args.samples)
        print(f"{name}: radius-3 output frame {entry['radius3_output_frame_ms']['median']:.3f} ms, with the spatial step "
              f"{entry['radius3_output_frame_with_spatial_h6_ms']['median']:.3f} ms", flush=True)
        result["sizes"][name] = entry
        del frames
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
