#!/usr/bin/env python3
"""Times csrc/vhs.hip and framewright_amd/vhs.py on the current GPU and writes profiles/vhs_timing.json: ms per frame at 1920 x 1080
and 720 x 576 (BGR) for each of the five steps and for `process`, one frame and a list of 16, each next to a `clone()` of the same
tensors timed in the same run; `detect_vhs_artifacts` on its own; the host share (the `np.random.choice` permutation for the frame's
edge count and for the worst case of every pixel an edge, the dropout merge, one wait); and the largest relative difference between
the device's FFT magnitudes and NumPy's on the rainbow fixtures of tests/vhs_ref.py.  The steps wait for the device (their decisions
are taken on the host), so these are wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs.  The frames
are `vhs_ref.clip_mix` at the timed size: head-switching noise, tracking rows and dropouts are there to be found and repaired.
Nothing is gated on these numbers.

    python tools/time_vhs.py
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

import vhs_ref as R  # noqa: E402
from framewright_amd import build as fw_build  # noqa: E402

REPEATS, WARMUP = 10, 2


def timed(fn) -> float:
    """median wall-clock ms of one call, the device idle before and after"""
    out = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARMUP:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def host_ms(fn, repeats: int = 5) -> float:
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main() -> None:
    fw_build.build()
    from framewright_amd import vhs as V
    p = V.DeviceVHSProcessor()
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": REPEATS, "sizes": {}}
    steps = {"head_switching": p.remove_head_switching, "tracking": p.fix_tracking_errors, "dropout": p.fix_dropout,
             "chroma_bleed": p.reduce_chroma_bleed, "rainbow": p.remove_rainbow_artifacts, "process": p.process}
    for name, (h, w) in {"1080p": (1080, 1920), "576i": (576, 720)}.items():
        entry: dict = {}
        base = R.clip_mix(h, w, 4)
        for n in (1, 16):
            clip = [torch.from_numpy(base[i % len(base)]).cuda() for i in range(n)]
            row = {"clone_ms_per_frame": timed(lambda: [f.clone() for f in clip]) / n}
            for step, fn in steps.items():
                np.random.seed(0)
                row[f"{step}_ms_per_frame"] = timed(lambda: fn(clip)) / n
            entry[f"list{n}"] = row
        frame = torch.from_numpy(base[2]).cuda()
        np.random.seed(0)
        entry["detect_vhs_artifacts_ms"] = timed(lambda: p.detect_vhs_artifacts(frame))
        n_edges = int(p.edge_counts_device([frame]).sum())
        runs = p.gray_stats_device([frame], runs=True)["runs"]
        one = torch.zeros((1,), dtype=torch.int32, device="cuda")
        entry["host"] = {
            "edges_in_frame": n_edges,
            "choice_ms_frame_edges": host_ms(lambda: np.random.choice(max(n_edges, 100), 100, replace=False)),
            "choice_ms_every_pixel_an_edge": host_ms(lambda: np.random.choice(h * (w - 1), 100, replace=False)),
            "runs_in_frame": int(runs.shape[0]),
            "merge_ms": host_ms(lambda: V._merge_dropouts([(x, y, length, 1) for _, x, y, length in runs.tolist()])),
            "one_wait_ms": timed(lambda: one.cpu()),
            "waits_per_32_frames": {"head_switching": 1, "tracking": 1, "dropout": 2, "chroma_bleed": 2, "rainbow": 0},
        }
        res["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)

    worst = 0.0
    for cname, clip in R.clips().items():
        f = clip[R.ANALYSIS_FRAME]
        if f.ndim != 3:
            continue
        got = p.analysis_device(torch.from_numpy(f).cuda())["rainbow"]
        for a, b in zip(got, R.rainbow_stats(f)):
            if b:
                worst = max(worst, abs(a - b) / abs(b))
    res["rainbow_fft_max_rel_diff_vs_numpy"] = worst
    res["rainbow_margin_required"] = 1e-6
    gold = ROOT / "tests" / "golden" / "vhs_reference_cpu_time.json"
    if gold.exists():                                                 # for context: the reference on the CPU the fixtures were made on
        res["reference_cpu_process_160x120_ms_per_frame"] = json.loads(gold.read_text())["reference_process_160x120_s_per_frame"] * 1e3
    out = ROOT / "profiles" / "vhs_timing.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out, "fft rel diff", worst)


if __name__ == "__main__":
    main()
