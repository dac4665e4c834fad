#!/usr/bin/env python3
"""Writes tests/golden/qp_artifact_reference.json and .npz from the reference's own `processors/qp_artifact_removal.py`:

    python tools/gen_qp_artifact_golden.py /path/to/reference/src/framewright/processors/qp_artifact_removal.py

The reference needs cv2 and cv2 is absent here.  A stub module named `cv2` in `sys.modules` maps the seven calls of the frame path -
`bilateralFilter`, `GaussianBlur`, `cvtColor`, `Canny`, `dilate`, `subtract`, `Laplacian` - to what tests/qp_artifact_ref.py says they
mean, so cv2's own bytes stay unpinned, as everywhere in this project, and everything else is the reference's own code running: the
strength from the QP, the filter parameters, the boundary mask, the dtype promotions and the association of the blends, the order of
the steps, the clipping and the truncation.

The reference draws its dither from numpy's global generator.  The generator seeds `np.random` before every call, draws the same
plane again after the same seed, and hands it to the restatement.  For every case it runs the reference and the restatement and
ASSERTS equality; it records the reference's digest, and inputs and outputs of a few small cases.  It also records what the
reference's value types, its QP detection (with recorded ffprobe answers in subprocess.run's place) and its directory driver (with
in-memory images in cv2.imread's and cv2.imwrite's place) answer.  Data only: nothing of the reference's program text is written.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import logging
import subprocess
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import qp_artifact_ref as R  # noqa: E402

QPS, MULTIPLIERS, BLOCK_SIZES = (10, 18, 28, 34, 40, 51), (0.5, 1.0), (4, 8, 16, 32)
TYPE_SETS = (("all",), ("blocking",), ("ringing",), ("banding",), ("blocking", "banding"), ("mosquito",))
NPZ_CASES = ("f24x40|qp28|m1.0|b8|all", "f24x40|qp40|m1.0|b8|all", "f19x21|qp34|m1.0|b16|blocking", "f24x40|qp18|m0.5|b8|ringing",
             "f24x40|qp51|m1.0|b8|banding", "f3x5|qp40|m1.0|b4|all")
FFPROBE = {
    "frames_with_qp": [{"returncode": 0, "stdout": json.dumps({"frames": [{"pict_type": "I", "qp": "22"}, {"pict_type": "P", "qp": 27},
                                                                          {"pict_type": "B"}, {"pict_type": "B", "qp": "30"}]})}],
    "bpp_0.6": [{"returncode": 0, "stdout": json.dumps({"frames": []})},
                {"returncode": 0, "stdout": json.dumps({"streams": [{"bit_rate": str(int(0.6 * 640 * 360 * 30)), "width": 640, "height": 360}]})}],
    "bpp_0.3": [{"returncode": 0, "stdout": json.dumps({"frames": [{"pict_type": "I"}]})},
                {"returncode": 0, "stdout": json.dumps({"streams": [{"bit_rate": str(int(0.3 * 640 * 360 * 30)), "width": 640, "height": 360}]})}],
    "bpp_0.15": [{"returncode": 1, "stdout": ""},
                 {"returncode": 0, "stdout": json.dumps({"streams": [{"bit_rate": str(int(0.15 * 640 * 360 * 30)), "width": 640, "height": 360}]})}],
    "bpp_0.07": [{"returncode": 0, "stdout": "{}"},
                 {"returncode": 0, "stdout": json.dumps({"streams": [{"bit_rate": str(int(0.07 * 640 * 360 * 30)), "width": 640, "height": 360}]})}],
    "bpp_0.01_default_size": [{"returncode": 0, "stdout": "{}"}, {"returncode": 0, "stdout": json.dumps({"streams": [{"bit_rate": "600000"}]})}],
    "no_bitrate": [{"returncode": 0, "stdout": "{}"}, {"returncode": 0, "stdout": json.dumps({"streams": [{"width": 640, "height": 360}]})}],
    "no_streams": [{"returncode": 0, "stdout": "{}"}, {"returncode": 0, "stdout": json.dumps({"streams": []})}],
    "both_fail": [{"returncode": 1, "stdout": ""}, {"returncode": 1, "stdout": ""}],
    "timeout": [{"timeout": True}],
    "bad_json": [{"returncode": 0, "stdout": "not json"}],
}


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.__version__ = "0.0-restated"
    stub.COLOR_BGR2GRAY, stub.CV_32F = 6, 5

    def cvt(img, code):
        assert code == stub.COLOR_BGR2GRAY
        return R.bgr2gray_u8(img)

    def blur(img, ksize, sigma):
        assert sigma == 0
        if img.dtype == np.uint8 and tuple(ksize) == (5, 5):
            return R.gaussian5_u8(img)
        if img.dtype == np.float32 and tuple(ksize) == (5, 5):
            return R.gaussian5_f32(img)
        assert img.dtype == np.float32 and tuple(ksize) == (15, 15), (img.dtype, ksize)
        return R.gaussian15_f32(img)

    def dilate(img, kernel, iterations=1):
        assert kernel.shape == (3, 3) and kernel.all()
        for _ in range(iterations):
            img = R.dilate3x3_u8(img)
        return img

    def laplacian(img, ddepth):
        assert ddepth == stub.CV_32F and img.dtype == np.float32
        return R.laplacian3_f32(img)

    stub.cvtColor = cvt
    stub.GaussianBlur = blur
    stub.bilateralFilter = lambda img, d, sigmaColor, sigmaSpace: R.bilateral_u8c3(img, d, sigmaColor, sigmaSpace)
    stub.Canny = lambda gray, lo, hi: R.canny_u8(gray, lo, hi)
    stub.dilate = dilate
    stub.subtract = lambda a, b: (a.astype(np.int16) - b).clip(0, 255).astype(np.uint8)
    stub.Laplacian = laplacian
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_qp_artifacts", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_qp_artifacts"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod, stub


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_key(inp: str, qp: int, mult: float, block: int, types) -> str:
    return "|".join([inp, f"qp{qp}", f"m{mult}", f"b{block}", "+".join(types)])


def cases():
    out = []
    for qp in QPS:
        for mult in MULTIPLIERS:
            for types in TYPE_SETS:
                out.append(("f24x40", qp, mult, 8, types))
    for block in BLOCK_SIZES:
        for types in (("all",), ("blocking",)):
            out.append(("f19x21", 34, 1.0, block, types))
            out.append(("f24x40", 40, 0.5, block, types))
    for qp in (18, 40):
        out.append(("f3x5", qp, 1.0, 4, ("all",)))
        out.append(("f1x1", qp, 1.0, 8, ("all",)))
        out.append(("f96x128", qp, 1.0, 8, ("all",)))             # by digest only
    out.append(("f33x70", 28, 1.0, 8, ("all",)))
    return out


def main() -> None:
    ref, stub = load_reference(sys.argv[1])
    logging.disable(logging.CRITICAL)
    inputs = {"f24x40": R.content_frame(24, 40, 1), "f19x21": R.content_frame(19, 21, 2), "f3x5": R.content_frame(3, 5, 3),
              "f1x1": R.content_frame(1, 1, 4), "f33x70": R.content_frame(33, 70, 5), "f96x128": R.content_frame(96, 128, 6)}
    npz = {f"input|{k}": v for k, v in inputs.items() if v.size <= 24 * 40 * 3}
    js_cases = {}
    seed = 1000
    for inp, qp, mult, block, kinds in cases():
        config = ref.QPArtifactConfig(strength_multiplier=mult, block_size=block, use_neural=False,
                                      artifact_types=[ref.ArtifactType(t) for t in kinds])
        remover = ref.QPArtifactRemover(config)
        assert remover._backend == "opencv"
        frame = inputs[inp]
        before = frame.copy()
        strength = remover._get_strength_for_qp(qp)
        assert type(strength) is np.float64 and strength == R.strength_for_qp(qp, mult)
        seed += 1
        np.random.seed(seed)
        got = remover._process_frame(frame, qp)
        np.random.seed(seed)
        noise = np.random.normal(0, 1 + strength * 2, frame.shape).astype(np.float32)
        want = R.process_frame(frame, qp, config, noise)
        key = case_key(inp, qp, mult, block, kinds)
        assert got.dtype == np.uint8 and got.shape == frame.shape and np.array_equal(got, want), key
        assert np.array_equal(frame, before), key
        rec = {"input": inp, "input_sha256": sha(frame), "qp": qp, "multiplier": mult, "block_size": block, "types": list(kinds),
               "strength": float(strength), "noise_seed": seed, "sha256": sha(got)}
        # the three removers alone, through the reference's private methods, on this frame with this strength
        steps = {"blocking": sha(remover._remove_blocking_opencv(frame, strength)), "ringing": sha(remover._remove_ringing_opencv(frame, strength))}
        assert steps["blocking"] == sha(R.remove_blocking(frame, strength, block)) and steps["ringing"] == sha(R.remove_ringing(frame, strength)), key
        np.random.seed(seed)
        steps["banding"] = sha(remover._remove_banding_opencv(frame, strength))
        assert steps["banding"] == sha(R.remove_banding(frame, strength, noise)), key
        rec["steps"] = steps
        js_cases[key] = rec
        if key in NPZ_CASES:
            npz[f"output|{key}"] = got
            npz[f"noise|{key}"] = noise
    assert all(f"output|{k}" in npz for k in NPZ_CASES), [k for k in NPZ_CASES if f"output|{k}" not in npz]

    # the value types
    cfg = ref.QPArtifactConfig()
    defaults = {k: ([t.value for t in v] if isinstance(v, list) else v) for k, v in cfg.__dict__.items()}
    rejected = []
    for bad in ({"strength_multiplier": 0.09}, {"strength_multiplier": 3.01}, {"block_size": 0}, {"block_size": 12}, {"block_size": 64},
                {"manual_qp": -1}, {"manual_qp": 52}):
        try:
            ref.QPArtifactConfig(**bad)
            raise AssertionError(bad)
        except ValueError as e:
            rejected.append([bad, str(e)])
    enums = {cls.__name__: {m.name: m.value for m in cls} for cls in (ref.ArtifactType, ref.CompressionLevel)}
    result_defaults = {k: v for k, v in ref.QPArtifactResult().__dict__.items()}
    made = ref.create_qp_artifact_remover(False, 1.5, False, 0).config
    created = {k: ([t.value for t in v] if isinstance(v, list) else v) for k, v in made.__dict__.items()}
    plain = ref.QPArtifactRemover(ref.QPArtifactConfig(use_neural=False))
    levels = {str(qp): plain._get_compression_level(qp).value for qp in range(0, 52)}
    strengths = {f"{qp}|{m}": float(ref.QPArtifactRemover(ref.QPArtifactConfig(use_neural=False, strength_multiplier=m))._get_strength_for_qp(qp))
                 for qp in range(0, 52) for m in (0.1, 0.5, 1.0, 2.0, 3.0)}

    # the QP detection with recorded ffprobe answers
    ffprobe = {}
    real_run = subprocess.run
    for name, answers in FFPROBE.items():
        calls = []

        def fake(cmd, capture_output=False, text=False, timeout=None, _answers=answers, _calls=calls):
            a = _answers[len(_calls)]
            _calls.append(list(cmd))
            if a.get("timeout"):
                raise subprocess.TimeoutExpired(cmd, timeout)
            return types.SimpleNamespace(returncode=a["returncode"], stdout=a["stdout"], stderr="")

        ref.subprocess.run = fake
        try:
            got = plain.detect_qp_from_video(Path(__file__))
        finally:
            ref.subprocess.run = real_run
        ffprobe[name] = {"answers": answers, "result": got, "calls": len(calls),
                         "commands": [[("<video>" if c == str(Path(__file__)) else c) for c in cmd] for cmd in calls]}
    missing = plain.detect_qp_from_video(Path(__file__).with_name("no_such_video.mp4"))
    assert missing is None

    # the directory driver with in-memory images: frame 2 cannot be read, writing frame 3 raises
    directory = {}
    for qp_arg, manual in ((None, None), (None, 35), (40, 35)):
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = Path(tmp) / "in", Path(tmp) / "out"
            src.mkdir()
            frames = {f"f{i:03d}.png": R.content_frame(12, 16, 10 + i) for i in range(5)}
            for name in frames:
                (src / name).write_bytes(name.encode())
            written, progress = {}, []

            def imread(path):
                return None if Path(path).name == "f002.png" else frames[Path(path).name].copy()

            def imwrite(path, img):
                if Path(path).name == "f003.png":
                    raise OSError("disk full")
                written[Path(path).name] = img

            stub.imread, stub.imwrite = imread, imwrite
            remover = ref.QPArtifactRemover(ref.QPArtifactConfig(use_neural=False, manual_qp=manual, artifact_types=[ref.ArtifactType.BLOCKING]))
            res = remover.remove_artifacts(src, dst, qp_arg, progress.append)
            qp_used = res.detected_qp
            for name, img in written.items():
                assert np.array_equal(img, R.remove_blocking(frames[name], R.strength_for_qp(qp_used, 1.0), 8)), name
            directory[f"qp{qp_arg}|manual{manual}"] = {
                "frames_processed": res.frames_processed, "frames_failed": res.frames_failed, "detected_qp": res.detected_qp,
                "compression_level": res.compression_level.value, "artifacts_removed": res.artifacts_removed, "written": sorted(written),
                "copied": sorted(p.name for p in dst.iterdir()), "progress": progress}
        with tempfile.TemporaryDirectory() as tmp:
            empty = remover.remove_artifacts(Path(tmp), Path(tmp) / "out", qp_arg)
            directory[f"qp{qp_arg}|manual{manual}"]["empty"] = {"frames_processed": empty.frames_processed, "frames_failed": empty.frames_failed,
                                                                 "detected_qp": empty.detected_qp, "artifacts_removed": empty.artifacts_removed}

    js = {"numpy": np.__version__, "strength_type": "numpy.float64", "defaults": defaults, "rejected": rejected, "enums": enums,
          "result_defaults": result_defaults, "created": created, "levels": levels, "strengths": strengths, "ffprobe": ffprobe,
          "directory": directory, "gaussian15": [float(v) for v in R.gaussian15_coeffs()]}
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"))        # noqa: E731 - one line per case
    head = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js.items())
    body = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js_cases.items())
    (out_dir / "qp_artifact_reference.json").write_text(f'{{{head},\n"cases":{{\n{body}\n}}\n}}\n')
    np.savez_compressed(out_dir / "qp_artifact_reference.npz", **npz)
    for name in ("qp_artifact_reference.json", "qp_artifact_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")
    print(len(js_cases), "cases")


if __name__ == "__main__":
    main()
