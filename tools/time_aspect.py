#!/usr/bin/env python3
"""Times csrc/aspect.hip and framewright_amd/aspect.py on the current GPU and writes profiles/aspect_timing.json:

  kernels     ms per frame at 1920 x 1080 BGR of each `fw_aspect_*` entry on a list of 16 frames (the blur on one frame), next to a
              `clone()` of the same tensors timed in the same run
  analysis    `analyze` + `crop_letterbox` on 16 frames at 1080p (one wait for the sums, one crop launch)
  conversion  every conversion method, and PAD with every fill mode, on one 7680 x 4320 frame to 2.39:1 (pillarbox) and 4:3 (letterbox)
  chain       the x4 upscale of a synthetic 1080p clip with 2.39:1 bars through `DeviceRestorationPipeline`, per input frame: without
              the handler (what the parent commit does: the baseline), with the crop, and with the crop and a PAD back to 16:9 -
              in one process, alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 5 after 2, 6 frames a run, so a timed
window is seconds long).  The device's clock while the chain ran is read from rocm-smi where it is there.  Nothing is gated on
these numbers.

    python tools/time_aspect.py
"""
from __future__ import annotations

import json
import shutil
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402

from framewright_amd import build as fw_build  # noqa: E402

REPEATS, WARMUP = 10, 2


def timed(fn, repeats: int = REPEATS, warmup: int = WARMUP) -> float:
    """median wall-clock ms of one call, the device idle before and after"""
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def barred_clip(n: int, h: int, w: int, ratio: float, seed: int):
    """n BGR frames h x w: synthetic content of ``ratio`` in the middle, dark bars (0 .. 8) above and below."""
    from framewright_amd.synth import synthetic_frames
    content = int(w / ratio)
    top = (h - content) // 2
    rng = np.random.RandomState(seed)
    out = []
    for f in synthetic_frames(n, h, w, seed=seed):
        g = rng.randint(0, 9, size=(h, w, 3)).astype(np.uint8)
        g[top:top + content] = np.maximum(f[top:top + content], 40)
        out.append(g)
    return out, top, h - top - content


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


def main() -> None:
    fw_build.build()
    from framewright_amd import aspect as A
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": REPEATS}
    h, w, n = 1080, 1920, 16
    frames, top, bottom = barred_clip(4, h, w, 2.39, seed=7)
    clip = [torch.from_numpy(frames[i % 4]).cuda() for i in range(n)]
    asp = A.DeviceAspectHandler()
    analysis = asp.analyze(clip)
    assert (analysis.top_bar, analysis.bottom_bar) == (top, bottom), (analysis, top, bottom)
    x, y, cw, ch = asp._crop_box(analysis)
    cropped = asp.crop_device(clip, x, y, cw, ch)
    res["bars_1080p"] = {"top": top, "bottom": bottom, "cropped": [ch, cw], "rows_kept": ch / h}
    res["kernels_1080p_ms_per_frame"] = {
        "clone": timed(lambda: [f.clone() for f in clip]) / n,
        "bar_sums_with_fetch": timed(lambda: asp.bar_sums_device(clip)) / n,
        "crop": timed(lambda: asp.crop_device(clip, x, y, cw, ch)) / n,
        "crop_unaligned_columns": timed(lambda: asp.crop_device(clip, 3, y, cw - 6, ch)) / n,
        "pad_color": timed(lambda: asp.pad_device(cropped, h, w, 0, y, A.FillMode.COLOR, (1, 2, 3))) / n,
        "pad_mirror": timed(lambda: asp.pad_device(cropped, h, w, 0, y, A.FillMode.MIRROR)) / n,
        "gauss99_one_frame": timed(lambda: asp.gauss99_device(clip[0])),
    }
    res["analyze_and_crop_1080p_ms_per_frame"] = timed(lambda: asp.crop_letterbox(clip)) / n
    print(json.dumps(res), flush=True)

    big = torch.from_numpy(barred_clip(1, 4320, 7680, 16 / 9, seed=9)[0][0]).cuda()
    conv: dict = {}
    for label, target in (("to_2.39", 2.39), ("to_4:3", "4:3")):
        row = {}
        for method in A.ConversionMethod:
            fills = list(A.FillMode) if method == A.ConversionMethod.PAD else [A.FillMode.BLACK]
            for fill in fills:
                hd = A.DeviceAspectHandler(A.AspectConfig(method=method, fill_mode=fill, fill_color=(9, 9, 9)))
                row[f"{method.value}_{fill.value}"] = timed(lambda: hd.convert_aspect([big], target), repeats=5, warmup=1)
        conv[label] = row
        print(label, json.dumps(row), flush=True)
    res["convert_8k_ms_per_frame"] = conv
    del big

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    m = 6
    part = clip[:m]
    pad_back = A.DeviceAspectHandler(A.AspectConfig(method=A.ConversionMethod.PAD))
    pipes = {"without_handler": DeviceRestorationPipeline(upscaler=sr),
             "crop": DeviceRestorationPipeline(upscaler=sr, aspect_handler=asp),
             "crop_and_pad_to_16:9": DeviceRestorationPipeline(upscaler=sr, aspect_handler=pad_back, aspect_target="16:9")}
    shapes = {k: list(p.run_device(part)[0].shape) for k, p in pipes.items()}               # also the first warm-up of every shape
    samples = {k: [] for k in pipes}
    for i in range(2 + 5):                                             # alternating, so a drift of the box hits all three alike
        for k, p in pipes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.run_device(part)
            torch.cuda.synchronize()
            if i >= 2:
                samples[k].append((time.perf_counter() - t0) * 1e3 / m)
    chain = {k: {"ms_per_input_frame": statistics.median(v), "min": min(v), "max": max(v), "output": shapes[k]} for k, v in samples.items()}
    base = chain["without_handler"]["ms_per_input_frame"]
    for k in ("crop", "crop_and_pad_to_16:9"):
        chain[k]["ratio_to_without_handler"] = chain[k]["ms_per_input_frame"] / base
    chain["clock"] = sclk()
    chain["frames_per_run"], chain["runs"] = m, 5
    res["chain_x4_1080p_2.39_bars"] = chain
    print(json.dumps(chain), flush=True)
    out = ROOT / "profiles" / "aspect_timing.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
