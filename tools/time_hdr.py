#!/usr/bin/env python3
"""Times csrc/hdr.hip and framewright_amd/hdr.py on the current GPU and writes profiles/hdr_timing.json:

  frame    ms per frame of `DeviceHDRConverter.convert_device` (one uint8 frame a call, into a new uint16 tensor) at 1920 x 1080 and at
           7680 x 4320 with the default config (two passes and the LUT launch), with local contrast off (one pass through the tail
           table) and on the float path (neither quantising step: powf per sample), beside the device-to-host copy of the uint16
           frame the stage produces into pinned memory; the calls alternate in one process
  cpu      tests/hdr_ref.convert_frame at 1080p on the CPU, for scale
  chain    the x4 upscale of a synthetic 1080p clip through `DeviceRestorationPipeline`, per input frame, without the converter (what
           the parent commit does: the baseline) and with it, alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 5 after 2, 6 frames a run).  The
device's clock is read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_hdr.py [--out FILE]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402

from framewright_amd import build as fw_build  # noqa: E402
from time_quality import alternating, sclk  # noqa: E402


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "hdr_timing.json"
    fw_build.build()
    import hdr_ref as R
    from framewright_amd import hdr as H
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": 10, "clock_before": sclk()}
    convs = {"default": H.DeviceHDRConverter(), "local_contrast_off": H.DeviceHDRConverter(H.HDRConfig(enable_local_contrast=False)),
             "float_path": H.DeviceHDRConverter(H.HDRConfig(enable_local_contrast=False, saturation_boost=1.0))}
    small = list(synthetic_frames(6, 1080, 1920, seed=7))
    for label, (h, w) in (("1080p", (1080, 1920)), ("8k", (4320, 7680))):
        host = small[0] if label == "1080p" else list(synthetic_frames(1, h, w, seed=9))[0]
        frame = torch.from_numpy(host).cuda()
        converted = convs["default"].convert_frame(frame)
        pinned = torch.empty(converted.shape, dtype=torch.uint16).pin_memory()
        calls = {k: (lambda c=c: c.convert_device([frame])) for k, c in convs.items()}
        calls["device_to_host_copy_u16"] = lambda: pinned.copy_(converted, non_blocking=True)
        row = alternating(calls)
        row["input_bytes"], row["output_bytes"] = frame.numel(), converted.numel() * 2
        for k in convs:
            passes = 2 if k == "default" else 1
            row[k]["gigabytes_per_second"] = (passes * row["input_bytes"] + row["output_bytes"]) / row[k]["median_ms"] / 1e6
            row[k]["over_copy"] = row[k]["median_ms"] / row["device_to_host_copy_u16"]["median_ms"]
        row["device_to_host_copy_u16"]["gigabytes_per_second"] = row["output_bytes"] / row["device_to_host_copy_u16"]["median_ms"] / 1e6
        res[label] = row
        print(label, json.dumps(row), flush=True)
        del frame, pinned, converted
    t0 = time.perf_counter()
    R.convert_frame(small[0], H.HDRConfig())
    res["hdr_ref_cpu_1080p_ms"] = (time.perf_counter() - t0) * 1e3
    res["clock_after_frames"] = sclk()

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    part = [torch.from_numpy(f).cuda() for f in small]
    pipes = {"without_converter": DeviceRestorationPipeline(upscaler=sr),
             "with_converter": DeviceRestorationPipeline(upscaler=sr, hdr_converter=convs["default"])}
    shapes = {k: [list(p.run_device(part)[0].shape), str(p.run_device(part)[0].dtype)] for k, p in pipes.items()}
    chain = alternating({k: (lambda p=p: p.run_device(part)) for k, p in pipes.items()}, repeats=5, warmup=2)
    for k in chain:
        chain[k] = {"ms_per_input_frame": chain[k]["median_ms"] / len(part), "min": chain[k]["min_ms"] / len(part),
                    "max": chain[k]["max_ms"] / len(part), "output": shapes[k]}
    chain["ratio"] = chain["with_converter"]["ms_per_input_frame"] / chain["without_converter"]["ms_per_input_frame"]
    chain["clock"], chain["frames_per_run"], chain["runs"] = sclk(), len(part), 5
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
