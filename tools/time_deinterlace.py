#!/usr/bin/env python3
"""Times csrc/deinterlace.hip on the current GPU and writes profiles/deinterlace_timing.json: ms per frame at 1920 x 1080 and
720 x 576 (BGR) for YADIF, BWDIF and BOB, one frame and a batch of 16, each next to a `clone()` of the same tensors timed in the
same run, and `analyze` on 50 frames.  Synthetic frames, medians of 20 after 3 warm-up runs.  Nothing is gated on these numbers.

    python tools/time_deinterlace.py
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from framewright_amd import build as fw_build  # noqa: E402

REPEATS, WARMUP = 20, 3


def timed(fn) -> float:
    """median ms of one call"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main() -> None:
    fw_build.build()
    from framewright_amd import deinterlace as D
    d = D.DeviceDeinterlacer(D.InterlaceConfig(field_order=D.FieldOrder.TFF))
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": REPEATS, "sizes": {}}
    modes = {"yadif": D.FW_DEINTERLACE_YADIF, "bwdif": D.FW_DEINTERLACE_BWDIF, "bob": D.FW_DEINTERLACE_BOB}
    for name, (h, w) in {"1080p": (1080, 1920), "576i": (576, 720)}.items():
        entry: dict = {}
        for n in (1, 16):
            clip = list(torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda").unbind(0))
            outs = list(torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda").unbind(0))
            row = {"clone_ms_per_frame": timed(lambda: [f.clone() for f in clip]) / n}
            for m, mode in modes.items():
                row[f"{m}_ms_per_frame"] = timed(lambda: d.interpolate_device(clip, mode, 1, outs=outs)) / n
            entry[f"batch{n}"] = row
        clip50 = list(torch.randint(0, 256, (50, h, w, 3), dtype=torch.uint8, device="cuda").unbind(0))
        entry["analyze_50_frames_ms"] = timed(lambda: D.DeviceDeinterlacer().analyze(clip50))
        res["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    out = ROOT / "profiles" / "deinterlace_timing.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
