#!/usr/bin/env python3
"""Writes tests/golden/perceptual_reference.json and .npz from the reference's own `processors/perceptual_tuning.py`:

    python tools/gen_perceptual_golden.py /path/to/reference/src/framewright/processors/perceptual_tuning.py

The reference needs cv2 and cv2 is absent here.  A stub module named `cv2` in `sys.modules` maps the calls of this file -
`fastNlMeansDenoisingColored`, `GaussianBlur` in both forms, `addWeighted`, `cvtColor` (BGR2HSV, HSV2BGR, BGR2LAB, LAB2BGR, BGR2GRAY,
GRAY2BGR), `createCLAHE(...).apply`, `subtract` - to what tests/perceptual_ref.py says they mean, and asserts the arguments the
reference passes, so cv2's own bytes stay unpinned, as everywhere in this project, and everything else is the reference's own code
running: the profile arithmetic, the thresholds, int() of h, the weights, the float32 saturation product and its truncation, the
order of the steps, the grain of the ORIGINAL frame.

For every case the tool runs the reference's `get_profile`, `apply_to_frame`, `adjust_settings`, `create_perceptual_tuner` and
`get_perceptual_profile` and the restatement and ASSERTS equality; it records profiles, plans, value types, digests of every output,
inputs and outputs of a few small cases, and the reference's quirks: `result_gray` is computed and never used, and the restorer never
calls the tuner.  Data only: nothing of the reference's program text is written.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import logging
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import perceptual_ref as R  # noqa: E402

SIZES = ((24, 40), (37, 53))
BALANCES = (0.0, 0.25, 0.5, 0.8, 1.0)
NPZ_CASES = ("balanced0.5|grain1", "enhanced|grain0", "faithful|grain1", "balanced0.8|grain0|limits1")
BASES = {"empty": {}, "full": {"sharpening": 0.5, "denoise": 0.3, "color_enhancement": 0.9, "detail_recovery": 0.2, "tile": 512}}


def cases() -> dict:
    """name -> the keyword arguments of PerceptualConfig (mode by value)"""
    out = {}
    for grain in (True, False):
        g = f"grain{int(grain)}"
        out[f"faithful|{g}"] = {"mode": "faithful", "balance": 0.0, "preserve_grain": grain}
        out[f"enhanced|{g}"] = {"mode": "enhanced", "balance": 1.0, "preserve_grain": grain}
        for b in BALANCES:
            out[f"balanced{b:g}|{g}"] = {"mode": "balanced", "balance": b, "preserve_grain": grain}
        out[f"balanced0.8|{g}|limits1"] = {"mode": "balanced", "balance": 0.8, "preserve_grain": grain, "sharpening_limit": 1.0, "denoise_limit": 1.0}
    out["balanced_fma|grain1"] = {"mode": "balanced", "balance": R.FMA_BALANCE, "preserve_grain": True}     # where a fused tail shows
    out["enhanced|grain0|denoise1"] = {"mode": "enhanced", "balance": 1.0, "preserve_grain": False, "denoise_limit": 1.0}
    return out


class Stub(types.ModuleType):
    """cv2, restated; `log` lists what the reference asked for, `spoil_result_gray` returns noise for the gray of the result."""

    COLOR_BGR2HSV, COLOR_HSV2BGR, COLOR_BGR2LAB, COLOR_LAB2BGR, COLOR_BGR2GRAY, COLOR_GRAY2BGR = 40, 54, 44, 56, 6, 8

    def __init__(self):
        super().__init__("cv2")
        self.__version__ = "0.0-restated"
        self.log, self.spoil_result_gray, self.grays = [], False, 0

    def fastNlMeansDenoisingColored(self, src, dst, h, h_color, template, search):
        assert dst is None and type(h) is int and h == h_color and h > 0 and (template, search) == (7, 21) and src.dtype == np.uint8
        self.log.append(("denoise", h))
        return R.denoise_u8(src, h)

    def GaussianBlur(self, img, ksize, sigma):
        assert img.dtype == np.uint8
        if tuple(ksize) == (0, 0):
            assert sigma == 3 and img.ndim == 3
            self.log.append(("blur19",))
            return R.gaussian_blur_sigma3_u8(img)
        assert tuple(ksize) == (5, 5) and sigma == 0 and img.ndim == 2
        self.log.append(("blur5",))
        return R.gaussian5_u8(img)

    def addWeighted(self, a, alpha, b, beta, gamma):
        assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and gamma == 0
        self.log.append(("add_weighted", float(np.float32(alpha)), float(np.float32(beta))))
        return R.hd.add_weighted(a, alpha, b, beta, 0)

    def cvtColor(self, img, code):
        assert img.dtype == np.uint8
        if code == self.COLOR_BGR2HSV:
            return R.hd.bgr2hsv(img)
        if code == self.COLOR_HSV2BGR:
            self.log.append(("hsv",))
            return R.hd.hsv2bgr(img)
        if code == self.COLOR_BGR2LAB:
            return R.fl.bgr_to_lab_gamma(img)
        if code == self.COLOR_LAB2BGR:
            return R.fl.lab_to_bgr_gamma(img)
        if code == self.COLOR_BGR2GRAY:
            self.grays += 1
            if self.spoil_result_gray and self.grays % 2 == 0:           # the second of the tail's two conversions: `result_gray`
                return np.random.default_rng(self.grays).integers(0, 256, img.shape[:2]).astype(np.uint8)
            return R.bgr2gray_u8(img)
        assert code == self.COLOR_GRAY2BGR and img.ndim == 2
        return np.repeat(img[:, :, None], 3, axis=2)

    def createCLAHE(self, clipLimit=40.0, tileGridSize=(8, 8)):        # noqa: N803 - cv2's keyword names
        assert tuple(tileGridSize) == (8, 8)
        stub = self

        class Clahe:
            def apply(self, plane):
                assert plane.dtype == np.uint8 and plane.ndim == 2
                stub.log.append(("clahe", float(clipLimit)))
                return R.hd.clahe(np.ascontiguousarray(plane), clipLimit)
        return Clahe()

    def subtract(self, a, b):
        assert a.dtype == np.uint8 and b.dtype == np.uint8
        self.log.append(("subtract",))
        return np.maximum(a.astype(np.int64) - b.astype(np.int64), 0).astype(np.uint8)


def load_reference(path: str):
    stub = Stub()
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_perceptual_tuning", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_perceptual_tuning"] = mod
    spec.loader.exec_module(mod)
    return mod, stub


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def expected_log(pl: dict) -> list:
    out = []
    for step in pl["steps"]:
        out += {"denoise": [("denoise", pl["h"])], "sharpen": [("blur19",), ("add_weighted", pl["w_src"], pl["w_blur"])], "colour": [("hsv",)],
                "detail": [("clahe", pl["clip_limit"])], "grain": [("blur5",), ("subtract",), ("add_weighted", 1.0, pl["grain_amount"])]}[step]
    return out


def main() -> None:
    ref, stub = load_reference(sys.argv[1])
    logging.disable(logging.CRITICAL)
    frames = {f"{h}x{w}": R.content_frame(h, w) for h, w in SIZES}
    npz = {f"input|{k}": v for k, v in frames.items()}
    recorded = {}
    for name, kw in cases().items():
        rcfg = R.PerceptualConfig(**{**kw, "mode": R.PerceptualMode(kw["mode"])})
        own_cfg = ref.PerceptualConfig(**{**kw, "mode": ref.PerceptualMode(kw["mode"])})
        own_profile = ref.PerceptualTuner(own_cfg).get_profile()
        assert own_profile.to_dict() == R.profile(rcfg).to_dict(), name
        pl = R.plan(rcfg)
        digests = {}
        for size, frame in frames.items():
            keep = frame.copy()
            stub.log, stub.grays, stub.spoil_result_gray = [], 0, False
            got = ref.PerceptualTuner(own_cfg).apply_to_frame(frame)
            assert stub.log == expected_log(pl), (name, stub.log, pl)
            want = R.apply_to_frame(frame, rcfg)
            assert got.dtype == np.uint8 and got.shape == frame.shape and np.array_equal(got, want), (name, size)
            assert np.array_equal(frame, keep) and got is not frame, name
            if "grain" in pl["steps"]:                                  # `result_gray` plays no part
                stub.spoil_result_gray, stub.grays = True, 0
                assert np.array_equal(ref.PerceptualTuner(own_cfg).apply_to_frame(frame), want) and stub.grays == 2, name
            if not pl["steps"]:
                assert np.array_equal(got, frame), name
            digests[size] = sha(got)
            if name in NPZ_CASES:
                npz[f"output|{name}|{size}"] = got
        recorded[name] = {"config": kw, "profile": own_profile.to_dict(), "plan": pl, "sha256": digests}
    assert R.plan(R.PerceptualConfig())["h"] == 1 and recorded["enhanced|grain0"]["plan"]["h"] == 4 and recorded["enhanced|grain0|denoise1"]["plan"]["h"] == 5
    assert recorded["balanced_fma|grain1"]["plan"]["grain_amount"] == float(np.float32(0.375) - np.float32(2.0 ** -24))
    assert len(R.fused_tail_pairs(recorded["balanced_fma|grain1"]["plan"]["grain_amount"])) > 0
    assert all(len(R.fused_tail_pairs(c["plan"]["grain_amount"])) == 0 for n, c in recorded.items() if n != "balanced_fma|grain1")
    assert recorded["balanced0|grain1"]["plan"]["steps"] == ["grain"] and recorded["faithful|grain0"]["plan"]["steps"] == []

    # adjust_settings
    settings = {}
    for cname, kw in (("default", {}), ("enhanced", {"mode": "enhanced", "balance": 1.0}), ("cast", {"preserve_color_cast": True}),
                      ("faithful_cast", {"mode": "faithful", "balance": 0.0, "preserve_color_cast": True})):
        mode = kw.get("mode", "balanced")
        for content in R.CONTENT_TYPES + ("unknown",):
            for bname, base in BASES.items():
                keep = dict(base)
                own = ref.PerceptualTuner(ref.PerceptualConfig(**{**kw, "mode": ref.PerceptualMode(mode)})).adjust_settings(base, content)
                assert own == R.adjust_settings(R.PerceptualConfig(**{**kw, "mode": R.PerceptualMode(mode)}), base, content) and base == keep
                settings[f"{cname}|{content}|{bname}"] = {"config": {**kw, "mode": mode}, "content_type": content, "base": base, "settings": own}

    # the factories and the value types
    created = {}
    for m in ("faithful", "balanced", "enhanced", "ENHANCED"):
        c = ref.create_perceptual_tuner(m).config
        created[m] = {"mode": c.mode.value, "balance": c.balance}
    try:
        ref.create_perceptual_tuner("vivid")
        raise AssertionError("vivid")
    except ValueError as e:
        created["vivid"] = str(e)
    by_balance = {f"{b:g}": ref.get_perceptual_profile(b).to_dict() for b in (-1.0, 0.0, 0.25, 0.5, 0.8, 1.0, 2.0)}
    for b, d in by_balance.items():
        assert d == R.profile(R.PerceptualConfig(balance=float(b))).to_dict()
    plainv = lambda v: v.value if isinstance(v, ref.PerceptualMode) else v        # noqa: E731
    defaults = {"config": {k: plainv(v) for k, v in ref.PerceptualConfig().__dict__.items()}, "profile": ref.PerceptualProfile().to_dict(),
                "clamped_config": {k: plainv(v) for k, v in ref.PerceptualConfig(balance=3.0, sharpening_limit=-1.0, denoise_limit=7.0).__dict__.items()},
                "clamped_profile": ref.PerceptualProfile(2.0, -1.0, 0.5, 9.0, -3.0).to_dict()}
    enums = {"PerceptualMode": {m.name: m.value for m in ref.PerceptualMode}}

    quirks = {"result_gray_is_unused": True, "gray_conversions_in_the_grain_tail": 2}
    restorer = Path(sys.argv[1]).resolve().parent.parent / "restorer.py"
    if restorer.exists():
        text = restorer.read_text()
        quirks["restorer_calls_the_tuner"] = any(s in text for s in ("PerceptualTuner", "perceptual_tuning", "apply_to_frame"))
        assert quirks["restorer_calls_the_tuner"] is False

    js = {"numpy": np.__version__, "sizes": [list(s) for s in SIZES], "gauss19_table": R.gauss19_table().tolist(), "defaults": defaults,
          "enums": enums, "created": created, "get_perceptual_profile": by_balance, "quirks": quirks,
          "inputs": {k: sha(v) for k, v in frames.items()}}
    out_dir = ROOT / "tests" / "golden"
    dump = lambda v: json.dumps(v, separators=(",", ":"))        # noqa: E731 - one line per case
    head = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in js.items())
    body = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in recorded.items())
    tail = ",\n".join(f"{dump(k)}:{dump(v)}" for k, v in settings.items())
    (out_dir / "perceptual_reference.json").write_text(f'{{{head},\n"cases":{{\n{body}\n}},\n"adjust_settings":{{\n{tail}\n}}\n}}\n')
    np.savez_compressed(out_dir / "perceptual_reference.npz", **npz)
    for name in ("perceptual_reference.json", "perceptual_reference.npz"):
        print(name, (out_dir / name).stat().st_size, "bytes")
    print(len(recorded), "frame cases,", len(settings), "adjust_settings cases")


if __name__ == "__main__":
    main()
