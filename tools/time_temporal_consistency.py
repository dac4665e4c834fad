#!/usr/bin/env python3
"""Times csrc/temporal_consistency.hip and framewright_amd/temporal_consistency.py on the current GPU and writes
profiles/temporal_consistency_timing.json:

  kernels   at 1920 x 1080 and at 7680 x 4320: fw_tcons_apply_u8 writing the frame (the hot path), writing the frame, the mask plane
            and the area, and fw_tcons_gray_hist_u8; beside them, in the same process, a device-to-device copy of the same 12 bytes a
            pixel (three frames read into one buffer of three frames: 9 bytes read and 9 written stand for 9 read and 3 written, so
            the copy moves more; both byte counts are in the file) and of one frame, and the device-to-host copy of one frame into
            pinned memory, which is what the stage saves at this point of the chain
  chain     the x4 upscale of a synthetic 1080p clip of four frames through `DeviceRestorationPipeline`, per run, without the stage
            (what the parent commit does) and with it (OPTICAL_FLOW, and HYBRID without a hook), alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 3 after 1).  The device's clock is
read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_temporal_consistency.py [--out FILE]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402

from framewright_amd import _lib  # noqa: E402
from framewright_amd import build as fw_build  # noqa: E402
from time_quality import alternating, sclk  # noqa: E402


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "temporal_consistency_timing.json"
    fw_build.build()
    from framewright_amd import temporal_consistency as TC
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": 10, "clock_before": sclk()}
    lib = _lib.load()
    small = [torch.from_numpy(f).cuda() for f in synthetic_frames(4, 1080, 1920, seed=7)]
    p = _lib.ptr
    for label, (h, w) in (("1080p", (1080, 1920)), ("8k", (4320, 7680))):
        if label == "1080p":
            clip = torch.stack(small[:3])
        else:                                                       # three 8K frames that differ a little: the 1080p ones, each pixel 4 x 4
            clip = torch.stack([f.repeat_interleave(4, 0).repeat_interleave(4, 1) for f in small[:3]])
        prev, cur, nxt = clip.unbind(0)
        dev = cur.device
        st = lambda: _lib.stream_ptr(dev)          # noqa: E731
        dst, dst3 = torch.empty_like(cur), torch.empty_like(clip)
        mask, area = torch.empty((h, w), dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        hist = torch.zeros(256, dtype=torch.int32, device=dev)
        pinned = torch.empty(cur.shape, dtype=torch.uint8).pin_memory()
        calls = {
            "kernel_apply": lambda: _lib.check(lib.fw_tcons_apply_u8(p(prev), p(cur), p(nxt), h, w, 0.02, 0.8, p(dst), None, None, st())),
            "kernel_apply_mask_area": lambda: _lib.check(lib.fw_tcons_apply_u8(p(prev), p(cur), p(nxt), h, w, 0.02, 0.8, p(dst), p(mask), p(area), st())),
            "kernel_gray_hist": lambda: _lib.check(lib.fw_tcons_gray_hist_u8(p(cur), h, w, p(hist), st())),
            "device_copy_three_frames": lambda: dst3.copy_(clip),
            "device_copy_one_frame": lambda: dst.copy_(cur),
            "device_to_host_copy": lambda: pinned.copy_(cur, non_blocking=True),
        }
        row = alternating(calls)
        px = h * w
        row["pixels"], row["frame_bytes"] = px, 3 * px
        row["kernel_apply"]["compulsory_bytes"], row["device_copy_three_frames"]["bytes_moved"] = 12 * px, 18 * px
        row["kernel_apply"]["compulsory_gbytes_per_second"] = 12 * px / row["kernel_apply"]["median_ms"] / 1e6
        row["device_copy_three_frames"]["gbytes_per_second"] = 18 * px / row["device_copy_three_frames"]["median_ms"] / 1e6
        row["device_copy_one_frame"]["gbytes_per_second"] = 6 * px / row["device_copy_one_frame"]["median_ms"] / 1e6
        row["kernel_gray_hist"]["gbytes_per_second"] = 3 * px / row["kernel_gray_hist"]["median_ms"] / 1e6
        # the floor: 12 bytes a pixel at the rate the three-frame copy moved its 18
        row["floor_ms_12_bytes_at_copy_rate"] = row["device_copy_three_frames"]["median_ms"] * 12 / 18
        row["apply_over_floor"] = row["kernel_apply"]["median_ms"] / row["floor_ms_12_bytes_at_copy_rate"]
        row["apply_over_device_to_host_copy"] = row["kernel_apply"]["median_ms"] / row["device_to_host_copy"]["median_ms"]
        row["flicker_area"] = float(TC.area_value(int(area.item()), px))
        res[label] = row
        print(label, json.dumps(row), flush=True)
        del clip, prev, cur, nxt, dst, dst3, mask, pinned
        torch.cuda.empty_cache()
    res["clock_after_frames"] = sclk()

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    stages = {m: TC.DeviceTemporalConsistencyProcessor(TC.CrossAttentionConfig(method=m)) for m in ("optical_flow", "hybrid")}
    pipes = {"without_stage": DeviceRestorationPipeline(upscaler=sr),
             "with_stage_optical_flow": DeviceRestorationPipeline(upscaler=sr, temporal_consistency=stages["optical_flow"]),
             "with_stage_hybrid": DeviceRestorationPipeline(upscaler=sr, temporal_consistency=stages["hybrid"])}
    chain = alternating({k: (lambda q=q: q.run_device(small)) for k, q in pipes.items()}, repeats=3, warmup=1)
    base = chain["without_stage"]["median_ms"]
    for k in list(chain):
        chain[k] = {"ms_per_run": chain[k]["median_ms"], "min": chain[k]["min_ms"], "max": chain[k]["max_ms"],
                    "ms_per_output_frame": chain[k]["median_ms"] / len(small), "ratio_to_without": chain[k]["median_ms"] / base}
    chain["clock"], chain["frames"], chain["runs"] = sclk(), len(small), 3
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
