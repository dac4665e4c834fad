#!/usr/bin/env python3
"""Clip analysis and the temporal-consistency pass on the device (csrc/temporal_chain.hip), at 1080p:

  - ms per frame of fw_frame_stats_u8 on a resident 50-frame batch, next to a `clone()` of the same bytes timed in the same run
    (alternating), and their ratio: the kernel reads the batch once and writes next to nothing, a clone reads and writes it;
  - ms per output frame of `DeviceTemporalConsistencyFilter.apply_device` at radius 2 and radius 3 (an inner frame, frames resident);
  - ms per frame of the whole `DeviceTemporalDenoiser.denoise_clip` at the defaults on a 16-frame clip, and of its phases run on
    their own: the analysis, the accumulate -> non-local means -> edge-preserve chain, the consistency pass.

Medians after warm-up, each sample a host clock around work that ends in a device synchronise.  Nothing is gated on these numbers:
they are a record.  Written to profiles/temporal_chain_timing.json with the digest of the build they were measured on.

  python tools/time_temporal_chain.py [--samples 20] [--clip-runs 3] [--out profiles/temporal_chain_timing.json]
"""
import argparse
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
    ap.add_argument("--clip-runs", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "temporal_chain_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from framewright_amd import build as fw_build
    from framewright_amd import temporal_denoise as TD
    from framewright_amd.synth import synthetic_frames
    if not torch.cuda.is_available():
        raise SystemExit("time_temporal_chain.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "samples": args.samples}

    # fw_frame_stats_u8 against a clone of the same batch, alternating
    base = synthetic_frames(CLIP, H, W, seed=4)
    batch = torch.from_numpy(np.concatenate([base] * 4)[:BATCH].copy()).to(dev)
    analyzer = TD.DeviceClipAnalyzer()
    for _ in range(3):
        analyzer.stats_device(batch)
        batch.clone()
    torch.cuda.synchronize()
    stats_ms, clone_ms = [], []
    for _ in range(args.samples):
        stats_ms.append(timed(lambda: analyzer.stats_device(batch))[0] / BATCH)
        clone_ms.append(timed(lambda: batch.clone())[0] / BATCH)
    gb = H * W * 3 / 1e9
    result["frame_stats"] = {"batch": BATCH, "ms_per_frame": summary(stats_ms), "clone_ms_per_frame": summary(clone_ms),
                             "ratio_to_clone": statistics.median(stats_ms) / statistics.median(clone_ms),
                             "read_gb_per_s": gb / (statistics.median(stats_ms) * 1e-3)}
    print(f"frame stats: {statistics.median(stats_ms):.4f} ms per frame ({result['frame_stats']['read_gb_per_s']:.0f} GB/s read), clone "
          f"{statistics.median(clone_ms):.4f} ms per frame, ratio {result['frame_stats']['ratio_to_clone']:.2f}", flush=True)
    del batch

    # the consistency filter, frames resident
    frames = [torch.from_numpy(f.copy()).to(dev) for f in base[:7]]
    est = TD.DeviceFlowEstimator()
    result["consistency_filter"] = {}
    for radius in (2, 3):
        filt = TD.DeviceTemporalConsistencyFilter(strength=0.5, temporal_radius=radius, flow_estimator=est)
        for _ in range(3):
            filt.apply_device(frames, 3)
        torch.cuda.synchronize()
        ms = [timed(lambda: filt.apply_device(frames, 3))[0] for _ in range(args.samples)]
        result["consistency_filter"][f"radius{radius}_output_frame_ms"] = summary(ms)
        print(f"consistency filter, radius {radius}: {statistics.median(ms):.3f} ms per output frame", flush=True)
    del frames

    # the whole driver at the defaults and its phases on their own
    clip = list(base)
    cfg = TD.TemporalDenoiseConfig()
    den = TD.DeviceTemporalDenoiser(cfg)
    acc = TD.DeviceTemporalAccumulator(temporal_weight_decay=cfg.temporal_weight_decay, flow_estimator=est)
    filt = TD.DeviceTemporalConsistencyFilter(cfg.noise_strength, cfg.temporal_radius, True, est)
    whole, p1, p3, p4 = [], [], [], []
    for run in range(args.clip_runs + 1):
        t, (outs, res) = timed(lambda: den.denoise_clip(clip))
        t1, analysis = timed(lambda: den.analyze(clip))
        cuts = [c for c in analysis["scene_changes"] if c < CLIP]
        t3, mid = timed(lambda: list(acc.denoise_sequence(clip, cfg.temporal_radius, cfg.preserve_edges, cfg.edge_threshold,
                                                          cfg.noise_strength, cuts)))
        t4, _ = timed(lambda: list(filt.apply_sequence(mid)))
        if run:                                                  # run 0 is the warm-up
            whole.append(t / CLIP)
            p1.append(t1 / CLIP)
            p3.append(t3 / CLIP)
            p4.append(t4 / CLIP)
    result["denoise_clip"] = {"frames": CLIP, "runs": args.clip_runs, "scene_changes": res.scene_changes_detected,
                              "avg_noise_reduction": res.avg_noise_reduction, "whole_ms_per_frame": summary(whole),
                              "analysis_ms_per_frame": summary(p1), "chain_ms_per_frame": summary(p3),
                              "consistency_ms_per_frame": summary(p4)}
    print(f"denoise_clip, {CLIP} frames: {statistics.median(whole):.2f} ms per frame; on their own: analysis {statistics.median(p1):.2f}, "
          f"chain {statistics.median(p3):.2f}, consistency pass {statistics.median(p4):.2f}", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
