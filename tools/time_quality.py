#!/usr/bin/env python3
"""Times csrc/quality.hip and framewright_amd/quality.py on the current GPU and writes profiles/quality_timing.json:

  kernel   ms per frame of `fw_quality_stats_u8` at 1920 x 1080 and at 7680 x 4320 (one frame a call, nothing fetched), beside the
           device-to-host copy of the same frame into pinned memory - the least the parent commit would pay to score the frame anywhere
           else - and the achieved bytes per second against the frame's size; the two alternate in one process
  scored   `score_frame` on the same frames: the kernel, the fetch of the few kilobytes and the host epilogue
  cpu      tests/quality_ref.FrameQualityScorer.score_frame at 1080p on the CPU, for scale
  chain    the x4 upscale of a synthetic 1080p clip through `DeviceRestorationPipeline`, per input frame, without a scorer (what the
           parent commit does: the baseline) and with both scorers, alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 5 after 2, 6 frames a run).  The
device's clock is read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_quality.py [--out FILE]
"""
from __future__ import annotations

import json
import shutil
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from framewright_amd import build as fw_build  # noqa: E402

REPEATS, WARMUP = 10, 2


def sclk() -> str:
    exe = shutil.which("rocm-smi")
    if not exe:
        return "not read (no rocm-smi)"
    try:
        text = subprocess.run([exe, "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        lines = [ln.strip() for ln in text.splitlines() if "sclk" in ln.lower()]
        return lines[0] if lines else "not read"
    except Exception as e:  # noqa: BLE001
        return f"not read ({type(e).__name__})"


def alternating(fns: dict, repeats: int = REPEATS, warmup: int = WARMUP) -> dict:
    """median wall-clock ms of each call, the device idle before and after, the calls taking turns"""
    samples = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                samples[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in samples.items()}


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "quality_timing.json"
    fw_build.build()
    import quality_ref as R
    from framewright_amd import quality as Q
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": REPEATS, "clock_before": sclk()}
    scorer = Q.DeviceFrameQualityScorer()
    small = list(synthetic_frames(6, 1080, 1920, seed=7))
    for label, (h, w) in (("1080p", (1080, 1920)), ("8k", (4320, 7680))):
        host = small[0] if label == "1080p" else list(synthetic_frames(1, h, w, seed=9))[0]
        frame = torch.from_numpy(host).cuda()
        pinned = torch.empty(frame.shape, dtype=torch.uint8).pin_memory()
        stats = torch.empty(scorer.statistics_bytes(1, h, w), dtype=torch.uint8, device="cuda")
        row = alternating({"fw_quality_stats_u8": lambda: scorer.statistics_device([frame], out=stats),
                           "device_to_host_copy": lambda: pinned.copy_(frame, non_blocking=True),
                           "score_frame": lambda: scorer.score_frame(frame, 0, 25.0)})
        size = frame.numel()
        row["frame_bytes"] = size
        for k in ("fw_quality_stats_u8", "device_to_host_copy"):
            row[k]["gigabytes_per_second"] = size / row[k]["median_ms"] / 1e6
        row["kernel_over_copy"] = row["fw_quality_stats_u8"]["median_ms"] / row["device_to_host_copy"]["median_ms"]
        res[label] = row
        print(label, json.dumps(row), flush=True)
        del frame, pinned
    ref = R.FrameQualityScorer()
    t0 = time.perf_counter()
    ref.score_frame(small[0], 0, 25.0)
    res["quality_ref_cpu_1080p_ms"] = (time.perf_counter() - t0) * 1e3

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    part = [torch.from_numpy(f).cuda() for f in small]
    pipes = {"without_scorers": DeviceRestorationPipeline(upscaler=sr),
             "with_both_scorers": DeviceRestorationPipeline(upscaler=sr, quality_scorer=Q.DeviceFrameQualityScorer(),
                                                            input_quality_scorer=Q.DeviceFrameQualityScorer(), quality_fps=25.0)}
    shapes = {k: list(p.run_device(part)[0].shape) for k, p in pipes.items()}
    chain = alternating({k: (lambda p=p: p.run_device(part)) for k, p in pipes.items()}, repeats=5, warmup=2)
    for k in chain:
        chain[k] = {"ms_per_input_frame": chain[k]["median_ms"] / len(part), "min": chain[k]["min_ms"] / len(part),
                    "max": chain[k]["max_ms"] / len(part), "output": shapes[k]}
    chain["ratio"] = chain["with_both_scorers"]["ms_per_input_frame"] / chain["without_scorers"]["ms_per_input_frame"]
    chain["clock"], chain["frames_per_run"], chain["runs"] = sclk(), len(part), 5
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
