#!/usr/bin/env python3
"""Writes tests/golden/hdr_reference.json and .npz from the reference's own `processors/hdr_conversion.py`:

    python tools/gen_hdr_golden.py /path/to/reference/src/framewright/processors/hdr_conversion.py

The reference imports cv2 inside its methods, and cv2 is absent here; without it `convert_frame` returns its input.  A stub module
named `cv2` in `sys.modules` maps the four calls of the frame path to what tests/hdr_ref.py says they mean - `cvtColor` for
BGR2LAB / LAB2BGR / BGR2HSV / HSV2BGR, `createCLAHE(...).apply`, `addWeighted` - so cv2's own bytes stay unpinned, as everywhere in
this project, and everything else (the gamma, the matrix product through the BLAS, the tone map, the quantisations, the highlight
flag, the transfer functions and the 16-bit output) is the reference's own code running.

For every case (a config and an input frame) the generator runs `HDRConverter.convert_frame` and `hdr_ref.convert_frame` and records
the reference's digest.  Where the path is exact - a quantising step on and a rational curve - it asserts equality, also of the
steps 1 - 3 float32 plane as bit patterns.  For the other paths (MOBIUS, whose `np.exp` is the CPU's; the float path, whose `np.power`
is) it records the largest code difference and the number of differing samples it saw against the restatement on this CPU.  The
tables the restatement takes (`hdr_ref.build_tables`) are recorded as built here.  Data only: nothing of the reference's program text
is written.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import logging
import sys
import types
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import hdr_ref as R  # noqa: E402

NPZ_CASES = ("u8_37x53|hdr10|1000|aces|bt2020|lc1|sat1.1|hr1", "u8_37x53|hlg|1000|reinhard|rec709|lc1|sat1.0|hr1",
             "u8_37x53|hdr10|1000|hable|bt2020|lc0|sat1.1|hr0", "u16_24x40|hdr10|4000|aces|bt2020|lc1|sat1.1|hr1",
             "u8_37x53|hdr10|1000|aces|bt2020|lc0|sat1.0|hr1", "u8_37x53|hdr10|1000|mobius|bt2020|lc1|sat1.1|hr1")


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.__version__ = "0.0-restated"
    stub.COLOR_BGR2LAB, stub.COLOR_LAB2BGR, stub.COLOR_BGR2HSV, stub.COLOR_HSV2BGR = 44, 56, 40, 54
    convert = {44: R.bgr2lab, 56: R.lab2bgr, 40: R.bgr2hsv, 54: R.hsv2bgr}
    stub.cvtColor = lambda img, code: convert[code](img)

    class _Clahe:
        def __init__(self, clipLimit=40.0, tileGridSize=(8, 8)):
            self.clip, self.grid = clipLimit, tuple(tileGridSize)

        def apply(self, plane):
            return R.clahe(plane, self.clip, self.grid)

    stub.createCLAHE = lambda clipLimit=40.0, tileGridSize=(8, 8): _Clahe(clipLimit, tileGridSize)
    stub.addWeighted = R.add_weighted
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_hdr", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_hdr"] = mod
    spec.loader.exec_module(mod)
    return mod


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_key(inp: str, c: dict) -> str:
    return "|".join([inp, c["target_format"], str(c["peak_brightness"]), c["tone_mapping"], c["color_space"],
                     f"lc{int(c['enable_local_contrast'])}", f"sat{c['saturation_boost']}", f"hr{int(c['highlight_recovery'])}"])


def cases():
    """(input name, config fields): every curve x PQ / HLG x BT2020 / REC709 x every switch at peak 1000 on the uint8 frame; the
    other peaks, P3, the other PQ format names and the uint16 frame on a smaller cross."""
    out = []
    base = dict(target_format="hdr10", peak_brightness=1000, tone_mapping="aces", color_space="bt2020", enable_local_contrast=True,
                saturation_boost=1.1, highlight_recovery=True)
    for tm in ("reinhard", "aces", "hable", "mobius"):
        for fmt in ("hdr10", "hlg"):
            for cs in ("bt2020", "rec709"):
                for lc in (True, False):
                    for sat in (1.1, 1.0):
                        for hr in (True, False):
                            out.append(("u8_37x53", dict(base, tone_mapping=tm, target_format=fmt, color_space=cs,
                                                         enable_local_contrast=lc, saturation_boost=sat, highlight_recovery=hr)))
            for peak in (400, 4000):
                out.append(("u8_16x24", dict(base, tone_mapping=tm, target_format=fmt, peak_brightness=peak)))
                out.append(("u16_24x40", dict(base, tone_mapping=tm, target_format=fmt, peak_brightness=peak)))
            out.append(("u16_24x40", dict(base, tone_mapping=tm, target_format=fmt, enable_local_contrast=False, saturation_boost=1.0)))
            out.append(("u16_24x40", dict(base, tone_mapping=tm, target_format=fmt, enable_local_contrast=False, saturation_boost=0.8)))
    out.append(("u8_16x24", dict(base, color_space="p3")))
    out.append(("u8_16x24", dict(base, target_format="hdr10plus", saturation_boost=1.5)))
    out.append(("u8_16x24", dict(base, target_format="dolby_vision", peak_brightness=10000)))
    out.append(("u8_40x53", dict(base)))
    out.append(("u8_8x8", dict(base)))
    return out


def main() -> None:
    ref = load_reference(sys.argv[1])
    logging.disable(logging.WARNING)                                 # the reference warns about ffmpeg at every construction
    warnings.simplefilter("ignore", RuntimeWarning)                  # the reference's HLG branch takes the log of negative numbers
    inputs = {"u8_37x53": R.content_frame(37, 53), "u8_16x24": R.content_frame(16, 24), "u8_40x53": R.content_frame(40, 53),
              "u8_8x8": R.content_frame(8, 8), "u16_24x40": R.content_frame(24, 40, np.uint16)}
    npz = {f"input|{k}": v for k, v in inputs.items()}
    js_cases, tables_seen = {}, {}

    # the value types answer alike (framewright_amd.hdr is held to these records by tests/test_hdr_ref_host.py)
    cfg = ref.HDRConfig()
    defaults = {k: (v.value if hasattr(v, "value") else v) for k, v in cfg.__dict__.items()}
    rejected = []
    for bad in ({"peak_brightness": 399}, {"peak_brightness": 10001}, {"saturation_boost": 0.79}, {"saturation_boost": 1.51},
                {"shadow_detail": -0.1}, {"shadow_detail": 2.1}, {"target_format": "hdr11"}, {"tone_mapping": "linear"},
                {"color_space": "xyz"}):
        try:
            ref.HDRConfig(**bad)
            raise AssertionError(bad)
        except ValueError as e:
            rejected.append([bad, str(e)])
    coerced = ref.HDRConfig(target_format="HLG", tone_mapping="Mobius", color_space="REC709")
    assert (coerced.target_format, coerced.tone_mapping, coerced.color_space) == (ref.HDRFormat.HLG, ref.ToneMapping.MOBIUS, ref.ColorSpace.REC709)
    enums = {cls.__name__: {m.name: m.value for m in cls} for cls in (ref.HDRFormat, ref.ToneMapping, ref.ColorSpace)}
    result_defaults = {k: (str(v) if isinstance(v, Path) else v) for k, v in ref.HDRConversionResult().__dict__.items()}
    made = ref.create_hdr_converter("HLG", 600, "Hable", False).config
    created = {k: (v.value if hasattr(v, "value") else v) for k, v in made.__dict__.items()}

    for inp, fields in cases():
        config = ref.HDRConfig(**fields)
        conv = ref.HDRConverter(config)
        conv._opencv_available = True
        frame = inputs[inp]
        got = conv.convert_frame(frame)
        assert got.dtype == np.uint16 and got.shape == frame.shape
        tables = R.build_tables(config)
        tkey = f"{fields['target_format']}|{fields['peak_brightness']}"
        if tkey in tables_seen:
            assert np.array_equal(tables_seen[tkey], tables["tail"])
        tables_seen[tkey] = tables["tail"]
        want = R.convert_frame(frame, config, tables)
        key = case_key(inp, fields)
        exact = R.quantised(config) and fields["tone_mapping"] in R.RATIONAL_CURVES
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        rec = {"config": fields, "input": inp, "sha256": sha(got), "exact": exact, "differing": int((diff != 0).sum()), "max_code_diff": int(diff.max())}
        # steps 1 - 3 as the reference's own private methods form them
        fl = frame.astype(np.float32) / (255.0 if frame.dtype == np.uint8 else 65535.0)
        lin = np.power(np.clip(fl, 0.0, 1.0), 2.2)
        assert np.array_equal(lin.view(np.uint32), R.linearize(frame, tables).view(np.uint32)), key
        if config.color_space in (ref.ColorSpace.BT2020, ref.ColorSpace.P3):
            lin = conv._convert_colorspace_709_to_2020(lin)
            assert np.array_equal(lin.view(np.uint32), R.to_bt2020(R.linearize(frame, tables)).view(np.uint32)), key
        tone = conv._apply_tone_mapping(lin)
        rec["tone_sha256"] = sha(tone)
        mine = R.tone_mapped_plane(frame, config, tables)
        if fields["tone_mapping"] in R.RATIONAL_CURVES:
            assert np.array_equal(tone.view(np.uint32), mine.view(np.uint32)), key
        else:
            rec["tone_differing"] = int((tone.view(np.uint32) != mine.view(np.uint32)).sum())
        if exact:
            assert rec["differing"] == 0, (key, rec)
        js_cases[key] = rec
        if key in NPZ_CASES:
            npz[f"output|{key}"] = got
            npz[f"tone|{key}"] = tone
    assert all(f"output|{k}" in npz for k in NPZ_CASES), [k for k in NPZ_CASES if f"output|{k}" not in npz]

    # the tail table against the reference's transfer functions run on the same 512 values
    x8 = np.arange(256).astype(np.uint8).astype(np.float32) / 255.0
    for tkey, tail in tables_seen.items():
        fmt, peak = tkey.split("|")
        conv = ref.HDRConverter(ref.HDRConfig(target_format=fmt, peak_brightness=int(peak)))
        fn = conv._apply_hlg_transfer if fmt == "hlg" else conv._apply_pq_transfer
        theirs = np.clip(fn(np.stack([x8, x8 * 0.95])) * 65535.0, 0, 65535).astype(np.uint16)
        assert np.array_equal(theirs, tail), tkey
        npz[f"tail|{tkey}"] = tail
    t = R.build_tables(ref.HDRConfig())
    npz["gamma8"], npz["gamma16"] = t["gamma8"], t["gamma16"]

    inexact = [r for r in js_cases.values() if not r["exact"]]
    js = {"numpy": np.__version__, "clip8": t["clip8"], "clip16": t["clip16"], "defaults": defaults, "rejected": rejected, "enums": enums,
          "result_defaults": result_defaults, "created": created,
          "inexact_summary": {"cases": len(inexact), "with_differences": sum(r["differing"] > 0 for r in inexact),
                              "samples_differing": sum(r["differing"] for r in inexact),
                              "max_code_diff": max(r["max_code_diff"] for r in inexact)}}
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"))        # noqa: E731 - one line per case
    head = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js.items())
    body = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js_cases.items())
    (out_dir / "hdr_reference.json").write_text(f'{{{head},\n"cases":{{\n{body}\n}}\n}}\n')
    np.savez_compressed(out_dir / "hdr_reference.npz", **npz)
    for name in ("hdr_reference.json", "hdr_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")
    print(js["inexact_summary"])


if __name__ == "__main__":
    main()
