#!/usr/bin/env python3
"""Writes tests/golden/deinterlace_reference.json and .npz from the reference's own `processors/format/interlace.py`:

    python tools/gen_deinterlace_golden.py /path/to/reference/src/framewright/processors/format/interlace.py

The reference imports cv2, which is absent here.  Its frame path calls two cv2 functions only: `cvtColor(BGR2GRAY)` and
`resize(INTER_LINEAR)`.  A stub module named `cv2` with exactly those two is put in `sys.modules` - the project's 14-bit gray and
`oracle/face_ref.resize_linear_u8` - so cv2's own arithmetic stays unpinned, as everywhere in this project; `_deinterlace_yadif`,
`_deinterlace_bwdif`, `_deinterlace_weave` and everything on gray frames call nothing of the stub.

Recorded: digests (and a few arrays) of the four frame methods on colour and gray lists in both orders; `analyze`,
`detect_telecine`, `inverse_telecine` and the AUTO order on the clips of `deinterlace_ref.analysis_clips()`; per frame the
reference's own hint, combing ratio and frame difference.  The float32 statistics its thresholds see (`diff`, `odd_gradient`,
`even_gradient`, `row_means`) are locals that the reference does not return: they are recorded from
`deinterlace_ref.stats_float32`, a restatement with the reference's types, and tied to the reference only through the asserted
equality of the hint and ratio they lead to.  The generator
asserts that tests/deinterlace_ref.py equals all of it.  Data only: nothing of the reference's program text is written.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import deinterlace_ref as R  # noqa: E402
from oracle.face_ref import resize_linear_u8  # noqa: E402


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.COLOR_BGR2GRAY, stub.INTER_LINEAR = 6, 1
    stub.cvtColor = lambda img, code: R.gray(img)
    stub.resize = lambda img, size, interpolation=1: resize_linear_u8(img, size[0], size[1])
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_interlace", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_interlace"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod


def analysis_record(a) -> dict:
    return {"is_interlaced": bool(a.is_interlaced), "field_order": a.field_order.value, "confidence": float(a.confidence),
            "combing_percentage": float(a.combing_percentage), "telecine_pattern": a.telecine_pattern.value,
            "recommended_method": a.recommended_method.value, "progressive_percentage": float(a.progressive_percentage),
            "tff_percentage": float(a.tff_percentage), "bff_percentage": float(a.bff_percentage),
            "diff_variance": a.details.get("telecine", {}).get("diff_variance")}


def same_analysis(rec: dict, b: R.Analysis) -> None:
    for k in ("is_interlaced", "field_order", "telecine_pattern", "recommended_method", "progressive_percentage", "tff_percentage",
              "bff_percentage", "combing_percentage", "confidence"):
        assert rec[k] == getattr(b, k), (k, rec[k], getattr(b, k))


def main() -> None:
    ref = load_reference(sys.argv[1])
    js: dict = {"numpy": np.__version__, "frames": {}, "analysis": {}}
    npz: dict = {}
    order_of = {"tff": ref.FieldOrder.TFF, "bff": ref.FieldOrder.BFF}

    # frames: every method, both orders, every position of a 4-frame list
    d = ref.Deinterlacer(ref.InterlaceConfig(field_order=ref.FieldOrder.TFF))
    for name, clip in R.frame_clips().items():
        for order, fo in order_of.items():
            parity = 1 if order == "tff" else 0
            outs = {"yadif": d._deinterlace_yadif(clip, fo), "bwdif": d._deinterlace_bwdif(clip, fo), "bob": d._deinterlace_bob(clip, fo),
                    "weave": d._deinterlace_weave(clip, fo)}
            mine = {"yadif": R.yadif(clip, parity), "bwdif": R.bwdif(clip, parity), "bob": R.bob(clip, parity), "weave": list(clip)}
            for m, got in outs.items():
                assert len(got) == len(mine[m]) and all(np.array_equal(a, b) for a, b in zip(got, mine[m])), (name, order, m)
                js["frames"][f"{name}/{order}/{m}"] = [R.sha256(a) for a in got]
                if name in ("9x16x3", "17x33x1") and m != "weave":
                    npz[f"{name}/{order}/{m}"] = np.stack(got)
            assert outs["weave"] is clip

    # analysis
    for name, clip in R.analysis_clips().items():
        d = ref.Deinterlacer(ref.InterlaceConfig())
        h, w = clip[0].shape[:2]
        a = d.analyze(clip)
        rec = analysis_record(a)
        mine = R.analyze(clip)
        same_analysis(rec, mine)
        tel = d.detect_telecine(clip)
        assert tel.value == R.detect_telecine(clip)
        kept_frames = d.inverse_telecine(clip)
        kept = [next(i for i, f in enumerate(clip) if f is k) for k in kept_frames]
        assert kept == R.inverse_telecine_indices(clip), (name, kept)
        forced = [next(i for i, f in enumerate(clip) if f is k) for k in d.inverse_telecine(clip, ref.TelecinePattern.PATTERN_3_2)]
        assert forced == R.inverse_telecine_indices(clip, "3:2")
        auto = d.detect_field_order(clip[:min(20, len(clip))]).value
        assert R.resolve_order(clip, "auto") == (auto if auto != "unknown" else "tff")
        auto_out = ref.Deinterlacer(ref.InterlaceConfig(method=ref.DeinterlaceMethod.BWDIF)).deinterlace(clip)
        want = R.deinterlace(clip, "bwdif", R.resolve_order(clip, "auto"))
        assert all(np.array_equal(x, y) for x, y in zip(auto_out, want))
        per_frame = []
        for i, f in enumerate(clip):
            st = R.stats(f)
            f32 = R.stats_float32(f)
            hint = d._detect_field_order_single(f)
            ratio = float(d._detect_combing(f)[1])
            assert hint == R.order_hint(st, h, w) and ratio == R.comb_ratio(st, h), (name, i)
            row = {"hint": hint, "comb_ratio": ratio, "stats": list(st), "odd_gradient": float(f32["odd_gradient"]),
                   "even_gradient": float(f32["even_gradient"]), "diff": float(f32["diff"]),
                   "row_means": [float(v) for v in f32["row_means"]]}
            if i + 1 < len(clip):
                fd = d._frame_difference(f, clip[i + 1])
                assert fd == R.frame_difference_float32(f, clip[i + 1])
                row["frame_difference"] = float(fd)
            per_frame.append(row)
        js["analysis"][name] = {"analyze": rec, "detect_telecine": tel.value, "inverse_telecine": kept, "inverse_telecine_3_2": forced,
                                "auto_order": auto, "auto_bwdif_sha256": [R.sha256(x) for x in auto_out], "frames": per_frame}
        print(name, rec["field_order"], rec["telecine_pattern"], rec["recommended_method"], len(kept), flush=True)

    out_dir = ROOT / "tests" / "golden"
    (out_dir / "deinterlace_reference.json").write_text(json.dumps(js, indent=0, separators=(",", ":")) + "\n")
    np.savez_compressed(out_dir / "deinterlace_reference.npz", **npz)
    for f in ("deinterlace_reference.json", "deinterlace_reference.npz"):
        print(f, (out_dir / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
