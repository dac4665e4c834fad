#!/usr/bin/env python3
"""Times csrc/perceptual.hip and framewright_amd/perceptual.py on the current GPU and writes profiles/perceptual_timing.json:

  frames   at 1920 x 1080 and at 7680 x 4320, the default configuration (BALANCED 0.5): each step entry (unsharp, saturation, detail,
           grain), the fused whole without the non-local means, the same steps as step entries chained (what the fusion buys), and -
           with fewer repeats, they are long - the non-local means alone and the fused whole with it; beside them, in the same
           process, the device-to-device copy of the frame's bytes and the device-to-host copy of the frame into pinned memory, which
           is what the stage saves at this point of the chain
  chain    the x4 upscale of a synthetic 1080p clip of four frames through `DeviceRestorationPipeline`, per run, without the stage
           (what the parent commit does) and with it (without and with the non-local means), alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (with the non-local means, and the chain: 3 after
1).  The device's clock is read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_perceptual.py [--out FILE]
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

from framewright_amd import build as fw_build  # noqa: E402
from time_quality import alternating, sclk  # noqa: E402


def without_denoise(PT, plan):
    return PT.PerceptualPlan(**{**plan.to_dict(), "steps": tuple(s for s in plan.steps if s != "denoise"), "h": 0})


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "perceptual_timing.json"
    fw_build.build()
    from framewright_amd import perceptual as PT
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    from framewright_amd.temporal_denoise import DeviceSpatialDenoiser
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": 10, "repeats_with_denoise": 3,
                 "clock_before": sclk()}
    tuner = PT.DevicePerceptualTuner()
    nlm = DeviceSpatialDenoiser()
    plan = tuner.plan()
    light = without_denoise(PT, plan)
    res["plan"] = plan.to_dict()
    small = [torch.from_numpy(f).cuda() for f in synthetic_frames(4, 1080, 1920, seed=7)]
    for label, (h, w) in (("1080p", (1080, 1920)), ("8k", (4320, 7680))):
        frame = small[0] if label == "1080p" else small[0].repeat_interleave(4, 0).repeat_interleave(4, 1).contiguous()
        dst = torch.empty_like(frame)
        pinned = torch.empty(frame.shape, dtype=torch.uint8).pin_memory()

        def chained(x=frame):
            y = tuner.unsharp_device(x, light.w_src, light.w_blur)
            y = tuner.saturation_device(y, light.boost)
            y = tuner.detail_device(y, light.clip_limit)
            return tuner.grain_device(y, x, light.grain_amount)

        calls = {
            "step_unsharp": lambda: tuner.unsharp_device(frame, light.w_src, light.w_blur),
            "step_saturation": lambda: tuner.saturation_device(frame, light.boost),
            "step_detail": lambda: tuner.detail_device(frame, light.clip_limit),
            "step_grain": lambda: tuner.grain_device(frame, frame, light.grain_amount),
            "fused_without_denoise": lambda: tuner.apply_frame_device(frame, out=dst, plan=light),
            "steps_chained_without_denoise": chained,
            "device_copy": lambda: dst.copy_(frame),
            "device_to_host_copy": lambda: pinned.copy_(frame, non_blocking=True),
        }
        row = alternating(calls)
        px = h * w
        row["pixels"], row["frame_bytes"] = px, 3 * px
        row["device_copy"]["gbytes_per_second"] = 6 * px / row["device_copy"]["median_ms"] / 1e6
        fused = row["fused_without_denoise"]["median_ms"]
        row["fused_over_device_copy"] = fused / row["device_copy"]["median_ms"]
        row["fused_over_device_to_host_copy"] = fused / row["device_to_host_copy"]["median_ms"]
        row["fused_over_steps_chained"] = fused / row["steps_chained_without_denoise"]["median_ms"]
        res[label] = row
        print(label, json.dumps(row), flush=True)
        heavy = alternating({"step_denoise": lambda: nlm.denoise_device(frame, plan.h, plan.h),
                             "fused_with_denoise": lambda: tuner.apply_frame_device(frame, out=dst, plan=plan)}, repeats=3, warmup=1)
        row.update(heavy)
        print(label, json.dumps(heavy), flush=True)
        del frame, dst, pinned
        torch.cuda.empty_cache()
    res["clock_after_frames"] = sclk()

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))

    class Light(PT.DevicePerceptualTuner):
        def plan(self):
            return without_denoise(PT, super().plan())

    pipes = {"without_stage": DeviceRestorationPipeline(upscaler=sr),
             "with_stage_without_denoise": DeviceRestorationPipeline(upscaler=sr, perceptual_tuner=Light()),
             "with_stage": DeviceRestorationPipeline(upscaler=sr, perceptual_tuner=tuner)}
    skipped = None
    if res["8k"]["step_denoise"]["median_ms"] > 1000.0:              # four 8K frames a run, four runs: minutes of non-local means
        del pipes["with_stage"]
        skipped = "with_stage: the non-local means alone takes more than a second per 8K frame (step_denoise above)"
    chain = alternating({k: (lambda q=q: q.run_device(small)) for k, q in pipes.items()}, repeats=3, warmup=1)
    base = chain["without_stage"]["median_ms"]
    for k in list(chain):
        chain[k] = {"ms_per_run": chain[k]["median_ms"], "min": chain[k]["min_ms"], "max": chain[k]["max_ms"],
                    "ms_per_input_frame": chain[k]["median_ms"] / len(small), "ratio_to_without": chain[k]["median_ms"] / base}
    chain["clock"], chain["frames"], chain["runs"] = sclk(), len(small), 3
    if skipped:
        chain["skipped"] = skipped
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
