#!/usr/bin/env python3
"""Times csrc/frame_generation.hip and framewright_amd/frame_generation.py on the current GPU and writes
profiles/frame_generation_timing.json:

  stage     ms per generated 1920 x 1080 frame of `DeviceMissingFrameGenerator.fill_device` on a gap of four frames, for each model,
            with and without grain matching (blend_edges 3); the optical-flow rows carry the two Farneback flows of the gap, a quarter
            each; beside the device-to-host copy of one frame into pinned memory; the calls alternate in one process
  kernels   the four entries alone on one frame (warp and blend, the statistic, the finish with grain and both blends, the
            extrapolation), fw_add_weighted_u8 (the `interpolate` generator) and one Farneback flow
  composed  the optical-flow rows' work from the entries that were exported before this stage: the same two flows, then per frame and
            side two scaled flow planes (torch), zeroed float64 accumulators, fw_flow_accumulate_u8 and fw_flow_accumulate_finish_u8
            (the BORDER_REFLECT_101 remap: the same arithmetic, not the same border rows), fw_add_weighted_u8, and for the grain the
            statistic followed by a host wait for the two deviations, the decision on the host and the finish
  chain     the x4 upscale of a synthetic 1080p clip with one frame in ten missing through `DeviceRestorationPipeline`, per run,
            without the generator (nine frames upscaled: what the parent commit does) and with it (ten), alternating, medians

Wall-clock times between two synchronisations: medians of 10 after 2 warm-up runs (the chain: 3 after 1).  The device's clock is
read from rocm-smi where it is there.  Nothing is gated on these numbers.

    python tools/time_frame_generation.py [--out FILE]
"""
from __future__ import annotations

import ctypes as C
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

GAP = 4


def main() -> None:
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else ROOT / "profiles" / "frame_generation_timing.json"
    fw_build.build()
    from framewright_amd import frame_generation as FG
    from framewright_amd.pipeline import DeviceRestorationPipeline
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import RRDB_MODELS, synthetic_frames, synthetic_rrdbnet_state
    res: dict = {"device": torch.cuda.get_device_name(0), "build": fw_build.source_digest(), "repeats": 10, "gap": GAP, "clock_before": sclk()}
    lib = _lib.load()
    host = list(synthetic_frames(10, 1080, 1920, seed=7))
    frames = [torch.from_numpy(f).cuda() for f in host]
    before, after = frames[0], frames[1]
    dev, (h, w) = before.device, before.shape[:2]
    p, st = _lib.ptr, lambda: _lib.stream_ptr(dev)          # noqa: E731
    pinned = torch.empty(before.shape, dtype=torch.uint8).pin_memory()
    gens = {(m, g): FG.DeviceMissingFrameGenerator(FG.FrameGenerationConfig(model=m, match_grain=g)) for m in ("interpolate_blend", "optical_flow")
            for g in (True, False)}
    calls = {f"stage_{m}_{'grain' if g else 'plain'}": (lambda gen=gen: gen.fill_device([before, after], [0, GAP + 1])) for (m, g), gen in gens.items()}
    calls["device_to_host_copy"] = lambda: pinned.copy_(before, non_blocking=True)

    # the entries alone
    gen = gens[("optical_flow", True)]
    est = gen._flow_estimator()
    (fx, fy), (bx, by) = est.flow_device(before, after), est.flow_device(after, before)
    quantiles, _ = gen._tables_for(dev)
    dst, stds = torch.empty_like(before), torch.tensor([7.0, 5.0], dtype=torch.float32, device=dev)
    g17 = gen._gauss17.ctypes.data_as(C.c_void_p)
    scratch = gen.scratch(int(lib.fw_framegen_grain_scratch_bytes(h, w)), dev)
    key = FG.noise_key(0, 1, FG.TAG_GRAIN)
    calls["kernel_warp_blend"] = lambda: _lib.check(lib.fw_framegen_warp_blend_u8(p(before), p(after), p(fx), p(fy), p(bx), p(by), h, w, 0.4, p(dst), st()))
    calls["kernel_grain_std"] = lambda: _lib.check(lib.fw_framegen_grain_std_u8(p(before), h, w, g17, p(scratch), p(stds[1:2]), st()))
    calls["kernel_finish_grain_two_blends"] = lambda: _lib.check(lib.fw_framegen_finish_u8(p(before), p(dst), h, w, p(stds[0:1]), p(stds[1:2]), None, p(quantiles),
                                                                                         key, p(after), 0.25, p(frames[2]), 0.75, st()))
    calls["kernel_extrapolate"] = lambda: _lib.check(lib.fw_framegen_extrapolate_u8(p(before), p(dst), h, w, None, p(gen._tables_for(dev)[1]), key, st()))
    calls["add_weighted"] = lambda: _lib.check(lib.fw_add_weighted_u8(p(before), 0.6, p(after), 0.4, h * w * 3, p(dst), st()))
    calls["farneback_one_flow"] = lambda: est.flow_device(before, after)

    # the same work from the entries that were exported before
    acc, ws = torch.empty((h, w, 3), dtype=torch.float64, device=dev), torch.empty((h, w), dtype=torch.float64, device=dev)
    warped = [torch.empty_like(before), torch.empty_like(before)]

    def composed(grain: bool):
        (cfx, cfy), (cbx, cby) = est.flow_device(before, after), est.flow_device(after, before)
        ref = torch.empty(1 + GAP, dtype=torch.float32, device=dev)
        if grain:
            gen.grain_std_device(before, ref[0:1])
        for i in range(GAP):
            t = (i + 1) / (GAP + 1)
            for frame, sx, sy, s, o in ((before, cfx, cfy, t, warped[0]), (after, cbx, cby, 1 - t, warped[1])):
                tx, ty = sx * s, sy * s
                acc.zero_(), ws.zero_()
                _lib.check(lib.fw_flow_accumulate_u8(p(frame), p(tx), p(ty), None, 1.0, None, 0.0, 0, h, w, p(acc), p(ws), st()))
                _lib.check(lib.fw_flow_accumulate_finish_u8(p(acc), p(ws), h, w, p(o), st()))
            _lib.check(lib.fw_add_weighted_u8(p(warped[0]), 1 - t, p(warped[1]), t, h * w * 3, p(dst), st()))
            ab, aa = FG.edge_blends(i, GAP, 3, True)
            add = False
            if grain:
                gen.grain_std_device(dst, ref[1 + i:2 + i])
                r, c = ref[0:1].item(), ref[1 + i:2 + i].item()      # the host waits, twice, and decides
                add = c > 0 and r > c
            _lib.check(lib.fw_framegen_finish_u8(p(dst), p(dst), h, w, p(ref[0:1]) if add else None, p(ref[1 + i:2 + i]) if add else None, None,
                                                 p(quantiles) if add else None, key, p(before) if ab is not None else None, ab or 0.0,
                                                 p(after) if aa is not None else None, aa or 0.0, st()))

    calls["composed_optical_flow_grain"] = lambda: composed(True)
    calls["composed_optical_flow_plain"] = lambda: composed(False)
    row = alternating(calls)
    for k in list(calls):
        if k.startswith(("stage_", "composed_")):
            row[k]["ms_per_generated_frame"] = row[k]["median_ms"] / GAP
            row[k]["over_copy"] = row[k]["ms_per_generated_frame"] / row["device_to_host_copy"]["median_ms"]
    for g in ("grain", "plain"):
        row[f"fused_over_composed_{g}"] = row[f"stage_optical_flow_{g}"]["median_ms"] / row[f"composed_optical_flow_{g}"]["median_ms"]
    row["frame_bytes"] = before.numel()
    # bytes the warp kernel must move at the least: two frames and four flow planes read, one frame written
    row["kernel_warp_blend"]["min_gbytes_per_second"] = (3 * h * w * 3 + 4 * h * w * 4) / row["kernel_warp_blend"]["median_ms"] / 1e6
    row["kernel_warp_blend"]["giga_byte_loads_per_second"] = 24 * h * w / row["kernel_warp_blend"]["median_ms"] / 1e6
    res["1080p"] = row
    print(json.dumps(row), flush=True)
    res["clock_after_frames"] = sclk()

    num_block, scale = RRDB_MODELS["RealESRGAN_x4plus"]
    sr = RRDBNetEngine(num_block, scale, "f16", device_id=0)
    sr.load_state_dict(synthetic_rrdbnet_state(num_block, scale, seed=1234))
    numbers = [n for n in range(10) if n != 4]
    part = [frames[n] for n in numbers]
    pipes = {"without_generator": DeviceRestorationPipeline(upscaler=sr),
             "with_generator_interpolate": DeviceRestorationPipeline(upscaler=sr, frame_generator=gens[("interpolate_blend", True)]),
             "with_generator_optical_flow": DeviceRestorationPipeline(upscaler=sr, frame_generator=gens[("optical_flow", True)])}
    chain = alternating({k: (lambda q=q: q.run_device(part, numbers)) for k, q in pipes.items()}, repeats=3, warmup=1)
    base = chain["without_generator"]["median_ms"]
    for k in list(chain):
        n_out = 9 if k == "without_generator" else 10
        chain[k] = {"ms_per_run": chain[k]["median_ms"], "min": chain[k]["min_ms"], "max": chain[k]["max_ms"], "frames_upscaled": n_out,
                    "ms_per_output_frame": chain[k]["median_ms"] / n_out, "ratio_to_without": chain[k]["median_ms"] / base}
    chain["clock"], chain["frames_in"], chain["runs"] = sclk(), len(part), 3
    res["chain_x4_1080p"] = chain
    print(json.dumps(chain), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
