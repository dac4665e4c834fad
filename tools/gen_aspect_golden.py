#!/usr/bin/env python3
"""Writes tests/golden/aspect_reference.json and .npz from the reference's own `processors/format/aspect.py`:

    python tools/gen_aspect_golden.py /path/to/reference/src/framewright/processors/format/aspect.py

The reference imports cv2, which is absent here.  Its frame path calls five cv2 functions; a stub module named `cv2` in `sys.modules`
maps them to what tests/aspect_ref.py says they mean - `cvtColor(BGR2GRAY)` the project's 14-bit gray, `resize` with INTER_LANCZOS4
oracle/lanczos_ref, `resize` with the default interpolation oracle/face_ref, `flip` a NumPy reversal, `GaussianBlur(src, (99, 99), 0)`
the fixed-point blur of `aspect_ref.gaussian_blur_99` - so cv2's own bytes stay unpinned, as everywhere in this project, and everything
else in the file (the bar search, the medians, the crops, the pad geometry, the strips of the mirror fill, which outputs are the input
object) is the reference's own code running.

Recorded for every clip of `aspect_ref.clips()`: the fields of `analyze_frame` on frame 0, the four bars of every frame, the fields of
`analyze`, `detect_aspect` and `detect_letterbox` of frame 0, and for `crop_letterbox` with align_to 2 and 16 one digest over the
output frames, their shape and whether the input list came back.  For every case of `aspect_ref.convert_cases`: one digest of
`convert_aspect` and which frames came back as the input object.  A few whole outputs go to the .npz.  The generator asserts that
tests/aspect_ref.py equals all of it and that the clips reach the cases they exist for.  Data only: nothing of the reference's program
text is written.
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
import aspect_ref as R  # noqa: E402

NPZ_KEYS = ("37x33|pad|mirror|wider", "37x33|pad|blur|narrower", "37x33/gray|fit|color|wider", "32x8|pad|mirror|narrower3")


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.COLOR_BGR2GRAY, stub.INTER_LANCZOS4 = 6, 4

    def resize(img, size, interpolation=None):
        fn = R.resize_lanczos4_u8 if interpolation == stub.INTER_LANCZOS4 else R.resize_linear_u8
        return fn(img, int(size[0]), int(size[1]))

    def flip(img, code):
        return img[::-1] if code == 0 else img[:, ::-1]

    def gaussian_blur(src, ksize, sigma):
        assert tuple(ksize) == (99, 99) and sigma == 0
        return R.gaussian_blur_99(src)

    stub.cvtColor = lambda img, code: R.gray(img)
    stub.resize, stub.flip, stub.GaussianBlur = resize, flip, gaussian_blur
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_aspect", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_aspect"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod


def same_frames(a, b) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def main() -> None:
    ref = load_reference(sys.argv[1])
    js: dict = {"numpy": np.__version__, "analysis": {}, "crops": {}, "convert": {}, "gauss99": R.gauss99_table().tolist()}
    npz: dict = {}

    # the value types answer alike
    for text in ("16:9", " 4:3 ", "2.35:1", "2.0:1", "1.78", "2.36/1", "nonsense", "1.0"):
        a, b = ref.StandardAspectRatio.from_string(text), R.StandardAspectRatio.from_string(text)
        assert (a.value if a else None) == (b.value if b else None), text
    for ar in ref.StandardAspectRatio:
        assert R.StandardAspectRatio(ar.value).decimal == ar.decimal and R.StandardAspectRatio[ar.name].value == ar.value
    for bad in ({"black_threshold": 256}, {"black_threshold": -1}, {"min_bar_size": -1}):
        for cls in (ref.AspectConfig, R.AspectConfig):
            try:
                cls(**bad)
                raise AssertionError(bad)
            except ValueError:
                pass
    assert ref.AspectConfig().__dict__.keys() == R.AspectConfig().__dict__.keys()
    assert all(getattr(ref.AspectConfig(), k) == v or k in ("method", "fill_mode") for k, v in R.AspectConfig().__dict__.items())
    made_ref, made = ref.create_aspect_handler("4:3", "PAD", "nonsense"), R.create_aspect_handler("4:3", "PAD", "nonsense")
    assert (made_ref.config.method.value, made_ref.config.fill_mode.value, made_ref.config.target_ratio) == \
        (made.config.method.value, made.config.fill_mode.value, made.config.target_ratio) == ("pad", "black", "4:3")

    for name, clip in R.clips().items():
        theirs, mine = ref.AspectHandler(ref.AspectConfig()), R.AspectHandler(R.AspectConfig())
        rec = {"frame0": R.analysis_record(theirs.analyze_frame(clip[0])), "clip": R.analysis_record(theirs.analyze(clip)),
               "bars": [[a.top_bar, a.bottom_bar, a.left_bar, a.right_bar] for a in map(theirs.analyze_frame, clip)],
               "detect_aspect": float(theirs.detect_aspect(clip[0])), "detect_letterbox": bool(theirs.detect_letterbox(clip[0]))}
        assert rec["frame0"] == R.analysis_record(mine.analyze_frame(clip[0])), name
        assert rec["clip"] == R.analysis_record(mine.analyze(clip)), (name, rec["clip"], R.analysis_record(mine.analyze(clip)))
        assert rec["bars"] == [[a.top_bar, a.bottom_bar, a.left_bar, a.right_bar] for a in map(mine.analyze_frame, clip)], name
        assert rec["detect_aspect"] == float(mine.detect_aspect(clip[0])) and rec["detect_letterbox"] == bool(mine.detect_letterbox(clip[0]))
        rows, cols = R.bar_sums(clip[0])
        rec["row_sums_sha256"], rec["column_sums_sha256"] = R.sha256(rows), R.sha256(cols)
        js["analysis"][name] = rec
        for align in R.CROP_ALIGNS:
            got = ref.AspectHandler(ref.AspectConfig(align_to=align)).crop_letterbox(clip)
            want = R.AspectHandler(R.AspectConfig(align_to=align)).crop_letterbox(clip)
            assert (got is clip) == (want is clip) and same_frames(got, want), (name, align)
            js["crops"][f"{name}|{align}"] = [R.digest(got), list(got[0].shape), got is clip]
        print(name, rec["bars"][0], rec["clip"]["crop_region"], rec["clip"]["is_variable"], flush=True)

    for name, frames in R.convert_frames().items():
        for key, method, fill, target in R.convert_cases(name, frames):
            theirs = R.handler_for(method, fill, ref.AspectHandler, ref.AspectConfig, ref.ConversionMethod, ref.FillMode)
            their_target = ref.StandardAspectRatio(target.value) if isinstance(target, R.StandardAspectRatio) else target
            got = theirs.convert_aspect(frames, their_target)
            want = R.handler_for(method, fill).convert_aspect(frames, target)
            assert same_frames(got, want), key
            same = [a is b for a, b in zip(got, frames)]
            assert same == [a is b for a, b in zip(want, frames)], key
            js["convert"][key] = [R.digest(got), list(got[0].shape), "".join("01"[v] for v in same)]
            if key in NPZ_KEYS:
                npz[key] = np.stack(got)
        print(name, len(R.convert_cases(name, frames)), "cases", flush=True)
    assert sorted(npz) == sorted(NPZ_KEYS)
    # add_pillarbox / add_letterbox are PAD whatever the configured method
    f = R.convert_frames()["37x33"]
    assert same_frames(ref.AspectHandler().add_pillarbox(f, 2.0), R.AspectHandler().add_pillarbox(f, 2.0))
    assert same_frames(ref.AspectHandler().add_letterbox(f, 0.5), R.AspectHandler().add_letterbox(f, 0.5))

    reached(js)
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"))        # noqa: E731 - one line per clip or case
    sections = []
    for k in ("analysis", "crops", "convert"):
        sections.append(f'{dump(k)}:{{\n' + ",\n".join(f"{dump(n)}:{dump(v)}" for n, v in js[k].items()) + "\n}")
    (out_dir / "aspect_reference.json").write_text(f'{{"numpy":{dump(js["numpy"])},\n"gauss99":{dump(js["gauss99"])},\n' + ",\n".join(sections) + "\n}\n")
    np.savez_compressed(out_dir / "aspect_reference.npz", **npz)
    for name in ("aspect_reference.json", "aspect_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")


def reached(js: dict) -> None:
    """The cases the clips exist for, read off the recorded data (tests/test_aspect_ref_host.py asserts the same)."""
    an, crops = js["analysis"], js["crops"]
    t = an["threshold/37x33"]["frame0"]
    assert (t["top_bar"], t["left_bar"]) == (3, 3)
    assert an["edge_found/37x33"]["frame0"]["top_bar"] == 37 // 3 - 1 and an["edge_lost/37x33"]["frame0"]["top_bar"] == 0
    assert an["edge_found/37x33"]["frame0"]["confidence"] < 1.0
    assert an["black/48x64"]["bars"] == [[0, 0, 0, 0]] * 2
    assert an["variable/37x33"]["clip"]["is_variable"] and not an["letterbox/37x33"]["clip"]["is_variable"]
    tops = sorted(b[0] for b in an["median_half/37x33"]["bars"])
    assert len(tops) == 4 and (tops[1] + tops[2]) % 2 == 1 and an["median_half/37x33"]["clip"]["top_bar"] == (tops[1] + tops[2]) // 2
    s = an["small_bar/48x64"]
    assert s["frame0"]["has_pillarbox"] and not s["clip"]["has_pillarbox"] and not s["frame0"]["has_letterbox"]
    assert crops["letterbox/48x64|2"][1][0] == 30 and crops["letterbox/48x64|16"][1][0] == 16
    assert crops["letterbox/32x8|16"][1][1] == 0                      # the reference returns empty arrays; the device refuses
    assert crops["plain/48x64|2"][2] is True and crops["long/37x33|2"][2] is False


if __name__ == "__main__":
    main()
