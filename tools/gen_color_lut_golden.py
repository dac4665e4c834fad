#!/usr/bin/env python3
"""Writes tests/golden/color_lut_reference.json and .npz from the reference's own `integration/lut.py` (NumPy only, so it runs
on a build machine): table digests, small tables, outputs of `apply_to_image_fast` / `apply_to_image` on the test images of
tests/color_lut_ref.py, whole-cube digests and the hard colours on which the wrong variants of the restatement differ.

    python tools/gen_color_lut_golden.py /path/to/reference/src/framewright/integration/lut.py

Data only: nothing of the reference's program text is written.  Takes a few minutes (two passes over the 8-bit colour cube).
"""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import color_lut_ref as R  # noqa: E402

SEASONS = ["winter", "spring", "summer", "autumn"]
STRENGTHS = [0.0, 0.3, 0.7, 1.0]
FILMS = ["kodak_vision3", "fuji_eterna", "kodachrome", "ektachrome"]
MAX_HARD = 200


def load_reference(path: str):
    spec = importlib.util.spec_from_file_location("reference_lut", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_lut"] = mod
    spec.loader.exec_module(mod)
    return mod


def table(lut) -> np.ndarray:
    return np.asarray(lut.data_3d, np.float64).astype(np.float32)


def main() -> None:
    ref = load_reference(sys.argv[1])
    mgr = ref.LUTManager()
    js: dict = {"numpy": np.__version__}
    npz: dict = {}

    # tables: digests at 33, full at 5
    js["table_sha256"] = {}
    for s in SEASONS:
        for k in STRENGTHS:
            js["table_sha256"][f"seasonal/{s}/{k}"] = R.sha256(table(mgr.create_seasonal_lut(s, k, 33)))
            npz[f"table5/seasonal/{s}/{k}"] = table(mgr.create_seasonal_lut(s, k, 5))
    for f in FILMS:
        js["table_sha256"][f"film/{f}"] = R.sha256(table(mgr.create_film_emulation_lut(f, 33)))
        npz[f"table5/film/{f}"] = table(mgr.create_film_emulation_lut(f, 5))
    js["table_sha256"]["identity"] = R.sha256(table(mgr.create_identity_lut(33)))
    contrast = mgr.create_contrast_lut(1.2, 33)
    js["contrast_1d"] = [list(map(float, row)) for row in contrast.data_1d]
    combined = mgr.combine_luts([mgr.create_seasonal_lut("summer", 0.5, 9), contrast], 5)
    npz["table5/combined_summer9_contrast"] = table(combined)

    # apply_to_image_fast on the test images: autumn 0.7 at every table size, both dtypes (BGR, as the reference reads frames)
    js["image_sha256"] = {}
    for size in R.TABLE_SIZES:
        lut = mgr.create_seasonal_lut("autumn", 0.7, size)
        for h, w in R.IMAGE_SIZES:
            for dt in (np.uint8, np.uint16):
                out = mgr.apply_to_image_fast(R.test_image(h, w, dt)[0], lut)
                assert out.dtype == dt
                js["image_sha256"][f"{size}/{h}x{w}/{np.dtype(dt).name}"] = R.sha256(out)
                if size == 33 and (h, w) in ((3, 5), (7, 13)):
                    npz[f"out/{size}/{h}x{w}/{np.dtype(dt).name}"] = out
    golden = {"autumn_0.7_33": mgr.create_seasonal_lut("autumn", 0.7, 33), "winter_1.0_17": mgr.create_seasonal_lut("winter", 1.0, 17)}
    full16 = R.full_range_u16()
    js["full_range_u16_sha256"] = {k: R.sha256(mgr.apply_to_image_fast(full16, lut)) for k, lut in golden.items()}

    # identity
    ident = mgr.create_identity_lut(33)
    js["identity"] = {}
    for dt in (np.uint8, np.uint16):
        img = R.test_image(64, 64, dt)[0]
        out = mgr.apply_to_image_fast(img, ident)
        js["identity"][np.dtype(dt).name] = {"sha256": R.sha256(out), "returns_input": bool(np.array_equal(out, img))}
    js["identity"]["full_range_u16_returns_input"] = bool(np.array_equal(mgr.apply_to_image_fast(full16, ident), full16))

    # 1D: the contrast LUT on a ramp, and a LUT with three different channels and a domain on three different ramps
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    js["ramp_1d_contrast"] = mgr.apply_to_image_fast(ramp, contrast)[:, 0, :].tolist()
    rng = np.random.default_rng(11)
    odd = ref.LUT(name="odd", lut_type=ref.LUTType.LUT_1D, size=7, domain_min=(0.0, 0.1, 0.2), domain_max=(1.0, 0.9, 0.6),
                  data_1d=[tuple(float(v) for v in row) for row in np.sort(rng.random((7, 3)) * 1.2 - 0.1, axis=0)])
    ramp3 = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=-1).astype(np.uint8)[:, None, :]
    js["odd_1d"] = {"data": [list(r) for r in odd.data_1d], "domain_min": list(odd.domain_min), "domain_max": list(odd.domain_max),
                    "image": ramp3[:, 0, :].tolist(), "out": mgr.apply_to_image_fast(ramp3, odd)[:, 0, :].tolist()}

    # the whole 8-bit cube, strip by strip (the operation is per pixel), and the hard colours found on the way
    js["cube_sha256"], js["hard"], js["variant_changes_u8"] = {}, {}, {}
    for key, lut in golden.items():
        tab = table(lut)
        hard = {v: [] for v in ("lerp32", "reciprocal", "fused")}
        count = {v: 0 for v in hard}

        def fn(img):
            want = mgr.apply_to_image_fast(img, lut)
            assert np.array_equal(R.apply_lut3d(img, tab), want), "the restatement differs from the reference"
            for v in hard:
                bad = (R.apply_lut3d(img, tab, **{v: True}) != want).any(-1)
                count[v] += int(bad.sum())
                if len(hard[v]) < MAX_HARD:
                    hard[v] += [(c.tolist(), o.tolist()) for c, o in zip(img[bad], want[bad])][:MAX_HARD - len(hard[v])]
            return want

        js["cube_sha256"][key] = R.cube_digest(fn)
        js["variant_changes_u8"][key] = count
        js["hard"][key] = {"uint8": {v: {"colours": [c for c, _ in hard[v]], "out": [o for _, o in hard[v]]} for v in hard}}
        # 16 bits: a few million random colours
        h16 = {v: [] for v in ("lerp32", "reciprocal")}
        rng = np.random.default_rng(16)
        for _ in range(8):
            img = rng.integers(0, 65536, size=(512, 1024, 3)).astype(np.uint16)
            want = mgr.apply_to_image_fast(img, lut)
            assert np.array_equal(R.apply_lut3d(img, tab), want)
            for v in h16:
                if len(h16[v]) < MAX_HARD:
                    bad = (R.apply_lut3d(img, tab, **{v: True}) != want).any(-1)
                    h16[v] += [(c.tolist(), o.tolist()) for c, o in zip(img[bad], want[bad])][:MAX_HARD - len(h16[v])]
        js["hard"][key]["uint16"] = {v: {"colours": [c for c, _ in h16[v]], "out": [o for _, o in h16[v]]} for v in h16}
        print(key, js["cube_sha256"][key], count, {v: len(h16[v]) for v in h16}, flush=True)

    out_dir = ROOT / "tests" / "golden"
    (out_dir / "color_lut_reference.json").write_text(json.dumps(js, indent=0, separators=(",", ":")) + "\n")
    np.savez_compressed(out_dir / "color_lut_reference.npz", **npz)
    for f in ("color_lut_reference.json", "color_lut_reference.npz"):
        print(f, (out_dir / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
