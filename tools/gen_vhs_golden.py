#!/usr/bin/env python3
"""Writes tests/golden/vhs_reference.json and .npz from the reference's own `processors/format/vhs.py`:

    python tools/gen_vhs_golden.py /path/to/reference/src/framewright/processors/format/vhs.py

The reference imports cv2, which is absent here.  Its frame path calls one cv2 function, `cvtColor(BGR2GRAY)`.  A stub module named
`cv2` with exactly that - the project's 14-bit gray - is put in `sys.modules`, so cv2's own gray stays unpinned, as everywhere in
this project; everything else in the file is NumPy arithmetic.

Recorded for every clip of `vhs_ref.clips()`: one digest over the output frames of each of the five list methods at the strengths of
`vhs_ref.recorded_cases`, of `process` with the default configuration, which frames came back as the input object, the fields of
`detect_vhs_artifacts` on frame 2, and the statistics each threshold sees (`vhs_ref.stats_record`: the reference keeps them as
locals, so they are recorded from the restatement and tied to the reference through the asserted equality of every decision).
`np.random.seed(k)` is called before every reference call that reaches `_detect_chroma_bleed`, k is recorded.  For context only, the
reference's own time for `process` on a 160 x 120 clip on the CPU the generator runs on goes to vhs_reference_cpu_time.json.  The generator
asserts that tests/vhs_ref.py equals all of it.  Data only: nothing of the reference's program text is written.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import time
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import vhs_ref as R  # noqa: E402

ANALYSIS_FIELDS = ("head_switching_detected", "head_switching_position", "head_switching_severity", "tracking_errors",
                   "tracking_severity", "tracking_line_positions", "dropout_detected", "dropout_count", "dropout_positions",
                   "chroma_bleed", "chroma_bleed_severity", "rainbow_effect", "dot_crawl", "jitter_detected", "jitter_severity",
                   "overall_degradation")


def load_reference(path: str):
    stub = types.ModuleType("cv2")
    stub.COLOR_BGR2GRAY = 6
    stub.cvtColor = lambda img, code: R.gray(img)
    sys.modules["cv2"] = stub
    spec = importlib.util.spec_from_file_location("reference_vhs", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_vhs"] = mod
    spec.loader.exec_module(mod)
    assert mod.HAS_OPENCV
    return mod


def plain(v):
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, (np.bool_, bool)):
        return bool(v)
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def main() -> None:
    ref = load_reference(sys.argv[1])
    js: dict = {"numpy": np.__version__, "cases": {}, "analysis": {}, "stats": {}, "dropout_log": {}}
    npz: dict = {}
    names = {"head_switching": "remove_head_switching", "tracking": "fix_tracking_errors", "dropout": "fix_dropout",
             "chroma_bleed": "reduce_chroma_bleed", "rainbow": "remove_rainbow_artifacts"}
    seen = {"shift": set(), "dropout": set(), "hs_above": set(), "rainbow": set(), "dot_crawl": set(), "jitter": set(), "few": set()}
    for name, clip in R.clips().items():
        proc = ref.VHSProcessor(ref.VHSConfig())
        cfg = R.Config()
        for method, s in R.recorded_cases(name) + [("process", 0.0)]:
            key, seed = R.case_key(name, method, s), R.seed_of(name, method, s)
            np.random.seed(seed)
            got = proc.process(clip) if method == "process" else getattr(proc, names[method])(clip, strength=s)
            np.random.seed(seed)
            log = []
            if method == "process":
                mine = R.process(clip, cfg)
            elif method == "dropout":
                mine = R.fix_dropout(clip, cfg, s, log)
                if name not in js["dropout_log"] and name.startswith("mix_low"):                     # which repair a box gets does not depend on the strength
                    js["dropout_log"][name] = [[list(b), how, src] for b, how, src in log]
                seen["dropout"] |= {how if how != "temporal" else "temporal" for _, how, _ in log}
            else:
                mine = R.METHODS[method](clip, cfg, s)
            assert len(got) == len(mine) and all(np.array_equal(a, b) for a, b in zip(got, mine)), key
            same = [a is b for a, b in zip(got, clip)]
            assert same == [a is b for a, b in zip(mine, clip)], key
            js["cases"][key] = [R.digest(got), "".join("01"[v] for v in same), seed]
            if method == "chroma_bleed":
                for f, o in zip(clip, got):
                    if o is not f and f.ndim == 3:
                        np.random.seed(seed)
                        seen["shift"].add(int(R.detect_chroma_bleed(f)[1] * 2 * s))
            if name == "mix_low/32x8" and (method, s) in (("process", 0.0), ("rainbow", 0.9), ("dropout", 0.7)):
                npz[key] = np.stack(got)
        frame = clip[R.ANALYSIS_FRAME]
        seed = R.seed_of(name, "analysis", 0.0)
        np.random.seed(seed)
        a = proc.detect_vhs_artifacts(frame)
        np.random.seed(seed)
        mine = R.analyze(frame, cfg)
        rec = {k: plain(getattr(a, k)) for k in ANALYSIS_FIELDS}
        rec["detected_quality"] = a.detected_quality.value
        rec["artifact_types"] = [x.artifact_type.value for x in a.all_artifacts]
        for k in rec:
            assert rec[k] == plain(getattr(mine, k)), (name, k, rec[k], getattr(mine, k))
        g = R.gray(frame)
        if g.shape[1] <= 258:                                         # the reference's float32 correlation is exact here
            shifts = []
            for y in range(1, g.shape[0] - 1, 5):
                c = np.correlate(g[y].astype(np.float32), g[y - 1].astype(np.float32), mode="same")
                shifts.append(int(np.argmax(c)) - g.shape[1] // 2)
            assert shifts == R.jitter_shifts(g).tolist(), name
        rec["seed"] = seed
        js["analysis"][name] = rec
        js["stats"][name] = R.stats_record(frame, cfg)
        if a.head_switching_detected:
            seen["hs_above"].add(a.head_switching_position > cfg.head_switch_height)
        seen["rainbow"].add(bool(a.rainbow_effect)), seen["dot_crawl"].add(bool(a.dot_crawl)), seen["jitter"].add(bool(a.jitter_detected))
        if frame.ndim == 3 and 0 < js["stats"][name]["n_edges"] < 10:
            seen["few"].add(True)
        print(name, rec["artifact_types"][:3], len(rec["artifact_types"]), rec["detected_quality"], flush=True)

    # the cases the clips exist for
    assert seen["shift"] >= {0, 1, 2}, seen
    assert seen["dropout"] >= {"temporal", "spatial", "none"}, seen
    assert seen["hs_above"] == {True, False}, seen
    assert seen["rainbow"] == {True, False} and seen["dot_crawl"] == {True, False} and seen["jitter"] == {True, False}, seen
    assert seen["few"] == {True}, seen

    # for context: the reference's own time for `process` on a 160 x 120 clip of 5 frames on this CPU
    big = R.clip_mix(120, 160, 4)
    t0 = time.perf_counter()
    ref.VHSProcessor(ref.VHSConfig()).process(big)
    per_frame = (time.perf_counter() - t0) / len(big)

    out_dir = ROOT / "tests" / "golden"
    # a measurement, not a fixture: in a file of its own, so that vhs_reference.json is the same in every run
    (out_dir / "vhs_reference_cpu_time.json").write_text(json.dumps({"reference_process_160x120_s_per_frame": per_frame}) + "\n")
    dump = lambda v: json.dumps(v, separators=(",", ":"))        # noqa: E731 - one line per case, clip or frame
    sections = [f'{dump(k)}:{{\n' + ",\n".join(f"{dump(n)}:{dump(v)}" for n, v in js[k].items()) + "\n}" for k in js if k != "numpy"]
    (out_dir / "vhs_reference.json").write_text(f'{{"numpy":{dump(js["numpy"])},\n' + ",\n".join(sections) + "\n}\n")
    np.savez_compressed(out_dir / "vhs_reference.npz", **npz)
    for f in ("vhs_reference.json", "vhs_reference.npz"):
        print(f, (out_dir / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
