#!/usr/bin/env python3
"""Frame deduplication on the device (csrc/dedup_hash.hip), at 1080p on synthetic frames, medians of `--samples` (20):

  - ms per frame of the dHash path (fw_pil_thumb_u8 gray first 17 x 16, then fw_dhash_pack_u8) and of the pixel-hash path
    (fw_pil_thumb_u8 64 x 64, gray second) on resident clips of n = 1, 16 and 64 frames, next to a `clone()` of the same clip timed
    in the same run (alternating): a clone reads and writes the clip once, a hash reads it once (its bound: about half a clone);
  - ms per frame of `DeviceFrameDeduplicator.hashes_device` on the same clips: the launches, the download and the host's hex / MD5;
  - ms per frame of the host Pillow path on the same machine, from a decoded image (no PNG decoding in the figure): the
    reference's `convert('L').resize((17, 16), LANCZOS)` + comparison, and `resize((64, 64), LANCZOS).convert('L')` + MD5;
  - seconds of `DeviceRestorationPipeline(upscaler=RRDBNet x4)` on a clip in which every third frame repeats the one before, with
    and without the deduplicator (synthetic weights; the upscale stage alone, which is what deduplication shortens).

Each sample is a host clock around work that ends in a device synchronise.  Nothing is gated on these numbers: they are a record.
Written to profiles/dedup_timing.json with the digest of the build they were measured on.

  python tools/time_dedup.py [--samples 20] [--chain-samples 3] [--chain-frames 9] [--out profiles/dedup_timing.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

H, W, SIZES = 1080, 1920, (1, 16, 64)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn):
    import torch
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--chain-samples", type=int, default=3)
    ap.add_argument("--chain-frames", type=int, default=9)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "dedup_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from framewright_amd import _lib
    from framewright_amd import build as fw_build
    from framewright_amd import dedup as DD
    from framewright_amd import pipeline as P
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state
    if not torch.cuda.is_available():
        raise SystemExit("time_dedup.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    med = statistics.median
    result = {"build": fw_build.source_digest(), "device": torch.cuda.get_device_name(0), "height": H, "width": W, "samples": args.samples,
              "pillow": Image.__version__}
    base = list(synthetic_frames(16, H, W, seed=4))
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    dd_d = DD.DeviceFrameDeduplicator(imagehash_available=True)
    dd_p = DD.DeviceFrameDeduplicator(imagehash_available=False)

    result["kernels"] = {}
    for n in SIZES:
        clip = torch.from_numpy(np.stack([base[k % 16] for k in range(n)])).to(dev)
        th_d = torch.empty((n, 16, 17), dtype=torch.uint8, device=dev)
        th_p = torch.empty((n, 64, 64), dtype=torch.uint8, device=dev)
        bits = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.fw_pil_thumb_workspace_bytes(n, H, W, 64, 64, 0), dtype=torch.uint8, device=dev)

        def dhash():
            _lib.check(lib.fw_pil_thumb_u8(p(clip), H * W * 3, n, H, W, 17, 16, 1, p(th_d), p(ws), st))
            _lib.check(lib.fw_dhash_pack_u8(p(th_d), n, 16, p(bits), st))

        pixel = lambda: _lib.check(lib.fw_pil_thumb_u8(p(clip), H * W * 3, n, H, W, 64, 64, 0, p(th_p), p(ws), st))
        for _ in range(3):
            dhash(), pixel(), clip.clone(), dd_d.hashes_device(clip), dd_p.hashes_device(clip)
        torch.cuda.synchronize()
        t = {k: [] for k in ("dhash", "pixel", "clone", "dhash_hashes_device", "pixel_hashes_device")}
        for _ in range(args.samples):
            t["dhash"].append(timed(dhash)[0] / n)
            t["pixel"].append(timed(pixel)[0] / n)
            t["clone"].append(timed(lambda: clip.clone())[0] / n)
            t["dhash_hashes_device"].append(timed(lambda: dd_d.hashes_device(clip))[0] / n)
            t["pixel_hashes_device"].append(timed(lambda: dd_p.hashes_device(clip))[0] / n)
        rec = {k + "_ms_per_frame": summary(v) for k, v in t.items()}
        rec["dhash_ratio_to_clone"] = med(t["dhash"]) / med(t["clone"])
        rec["pixel_ratio_to_clone"] = med(t["pixel"]) / med(t["clone"])
        rec["dhash_read_gb_per_s"] = H * W * 3 / 1e9 / (med(t["dhash"]) * 1e-3)
        rec["pixel_read_gb_per_s"] = H * W * 3 / 1e9 / (med(t["pixel"]) * 1e-3)
        result["kernels"][f"n{n}"] = rec
        print(f"n = {n}: dHash {med(t['dhash']):.4f} ms per frame, pixel hash {med(t['pixel']):.4f}, clone {med(t['clone']):.4f}; "
              f"hashes_device {med(t['dhash_hashes_device']):.4f} / {med(t['pixel_hashes_device']):.4f}", flush=True)
        del clip, ws

    host_d, host_p = [], []
    for k in range(min(args.samples, 8)):
        img = Image.fromarray(np.ascontiguousarray(base[k % 16][:, :, ::-1]))
        t0 = time.perf_counter()
        px = np.asarray(img.convert("L").resize((17, 16), Image.Resampling.LANCZOS))
        _ = px[:, 1:] > px[:, :-1]
        host_d.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        small = img.resize((64, 64), Image.Resampling.LANCZOS).convert("L")
        hashlib.md5(bytes(list(small.getdata())[::4])).hexdigest()
        host_p.append((time.perf_counter() - t0) * 1e3)
    result["host_pillow"] = {"dhash_ms_per_frame": summary(host_d), "pixel_ms_per_frame": summary(host_p), "png_decoding": "not included"}
    print(f"host Pillow: dHash {med(host_d):.2f} ms per frame, pixel hash {med(host_p):.2f}", flush=True)

    frames = [base[k - 1] if k % 3 == 2 else base[k] for k in range(args.chain_frames)]    # every third frame repeats the one before
    sr = RRDBNetEngine(23, 4, "f16")
    sr.load_state_dict(synthetic_rrdbnet_state(23, 4, seed=5))
    clip = [torch.from_numpy(f).to(dev) for f in frames]
    pipes = {"without": P.DeviceRestorationPipeline(upscaler=sr),
             "with_pixel_hash": P.DeviceRestorationPipeline(upscaler=sr, deduplicator=dd_p),
             "with_dhash": P.DeviceRestorationPipeline(upscaler=sr, deduplicator=dd_d)}
    for pipe in pipes.values():
        pipe.run_device(clip)
    torch.cuda.synchronize()
    chain = {k: [] for k in pipes}
    for _ in range(args.chain_samples):
        for k, pipe in pipes.items():
            chain[k].append(timed(lambda: pipe.run_device(clip))[0] / 1e3)
    result["upscale_stage"] = {"frames": len(frames), "model": "RRDBNet x4, 23 blocks, f16, synthetic weights", "runs": args.chain_samples,
                               "unique_frames": {k: (pipe.last_dedup_result.unique_frames if pipe.last_dedup_result else len(frames))
                                                 for k, pipe in pipes.items()},
                               "seconds": {k: summary(v) for k, v in chain.items()}}
    print(f"upscale stage on {len(frames)} frames: {med(chain['without']):.3f} s without, {med(chain['with_pixel_hash']):.3f} s with the "
          f"pixel hash, {med(chain['with_dhash']):.3f} s with the dHash", flush=True)
    sr.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
