#!/usr/bin/env python3
"""Times csrc/qp_artifacts.hip and framewright_amd/qp_artifacts.py on the current GPU and writes profiles/qp_artifacts_timing.json:

  frame    ms per 1920 x 1080 frame of `DeviceQPArtifactRemover.process_device` (all three removers, the counter dither, into a new
           tensor) and of the bilateral kernel alone (`fw_bilateral_u8c3`, tables already on the device) at qp 18 (d 6, radius 3) and
           qp 40 (d 12, radius 6), and the bilateral at d 15 (radius 7, strength 1); beside the device-to-host copy of the same frame
           into pinned memory and beside the 1080p Restormer frame that follows the stage in the chain; the calls alternate in one process
  steps    the three removers alone at qp 40
  cpu      tests/qp_artifact_ref.process_frame at 1080p on the CPU, for scale
  chain    the x4 upscale of a synthetic 1080p clip through `DeviceRestorationPipeline`, per input frame, without the stage (what the
           parent commit does: the baseline) and with it in front, alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 5 after 2, 6 frames a run).  The
device's clock is read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_qp_artifacts.py [--out FILE]
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

from framewright_amd import _lib  # noqa: E402
from framewright_amd import build as fw_build  # noqa: E402
from time_quality import alternating, sclk  # noqa: E402


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "qp_artifacts_timing.json"
    fw_build.build()
    import qp_artifact_ref as R
    from framewright_amd import qp_artifacts as Q
    from framewright_amd import restormer as RS
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": 10, "clock_before": sclk()}
    lib = _lib.load()
    small = list(synthetic_frames(6, 1080, 1920, seed=7))
    frame = torch.from_numpy(small[0]).cuda()
    h, w = 1080, 1920
    dst = torch.empty_like(frame)
    pinned = torch.empty(frame.shape, dtype=torch.uint8).pin_memory()
    rem = Q.DeviceQPArtifactRemover()
    calls = {}
    tables = {}
    for label, strength in (("qp18", rem.strength_for_qp(18)), ("qp40", rem.strength_for_qp(40)), ("strength1", 1.0)):
        d, sc, ss = Q.blocking_params(strength)
        color, space = (torch.from_numpy(a).cuda() for a in Q.bilateral_tables(d, sc, ss))
        tables[label] = (d, color, space)

        def bilateral(d=d, color=color, space=space):
            _lib.check(lib.fw_bilateral_u8c3(_lib.ptr(frame), _lib.ptr(dst), h, w, 3, d, _lib.ptr(color), _lib.ptr(space), _lib.stream_ptr(frame.device)))

        calls[f"bilateral_{label}_d{d}"] = bilateral
    for qp in (18, 40):
        calls[f"stage_qp{qp}"] = lambda qp=qp: rem.process_device([frame], qp)
    for types in ("blocking", "ringing", "banding"):
        one = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(artifact_types=[Q.ArtifactType(types)]))
        calls[f"{types}_qp40"] = lambda one=one: one.process_device([frame], 40)
    calls["device_to_host_copy"] = lambda: pinned.copy_(frame, non_blocking=True)
    eng = RS.RestormerEngine(dtype="f16", **RS.RESTORMER_ARGS)
    eng.load_state_dict(RS.synthetic_restormer_state(**RS.RESTORMER_ARGS))
    den = torch.empty_like(frame)
    calls["restormer_1080p"] = lambda: eng.denoise_device(frame, out=den)
    row = alternating(calls)
    row["frame_bytes"] = frame.numel()
    for k in list(calls):
        if k not in ("device_to_host_copy", "restormer_1080p"):
            row[k]["over_copy"] = row[k]["median_ms"] / row["device_to_host_copy"]["median_ms"]
            row[k]["over_restormer"] = row[k]["median_ms"] / row["restormer_1080p"]["median_ms"]
    for label, (d, _, _) in tables.items():
        r = max(d // 2, 1)
        taps = sum(1 for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r)
        k = f"bilateral_{label}_d{d}"
        row[k]["taps"] = taps
        row[k]["gigataps_per_second"] = taps * h * w / row[k]["median_ms"] / 1e6
    res["1080p"] = row
    print(json.dumps(row), flush=True)
    eng.close()
    del eng, den
    t0 = time.perf_counter()
    R.process_frame(small[0], 40, rem.config, (0, 0))
    res["qp_artifact_ref_cpu_1080p_qp40_ms"] = (time.perf_counter() - t0) * 1e3
    res["clock_after_frames"] = sclk()

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    part = [torch.from_numpy(f).cuda() for f in small]
    pipes = {"without_stage": DeviceRestorationPipeline(upscaler=sr),
             "with_stage_qp40": DeviceRestorationPipeline(upscaler=sr, artifact_remover=rem, artifact_qp=40)}
    chain = alternating({k: (lambda p=p: p.run_device(part)) for k, p in pipes.items()}, repeats=5, warmup=2)
    for k in chain:
        chain[k] = {"ms_per_input_frame": chain[k]["median_ms"] / len(part), "min": chain[k]["min_ms"] / len(part),
                    "max": chain[k]["max_ms"] / len(part)}
    chain["ratio"] = chain["with_stage_qp40"]["ms_per_input_frame"] / chain["without_stage"]["ms_per_input_frame"]
    chain["clock"], chain["frames_per_run"], chain["runs"] = sclk(), len(part), 5
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
