"""Writes tests/golden/dedup_reference.json: what the reference's own `FrameDeduplicator` finds on tests/dedup_ref.make_clip.

Runs only where a checkout of the reference is at hand (its path is the argument); only the JSON is committed.  The clips are written
as `frame_%08d.png` into a temporary directory, the reference's `analyze_frames` runs over them with `imagehash` absent - so it
takes its pixel-hash path - and the result's fields and the per-file hashes are recorded.

    python tools/gen_dedup_golden.py /path/to/reference/src/framewright/processors/deduplication.py
"""
import importlib.util
import json
import sys
import tempfile
from dataclasses import asdict
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import dedup_ref as dr  # noqa: E402

CASES = [dict(h=70, w=300, pixel_sample_rate=4), dict(h=135, w=240, pixel_sample_rate=4), dict(h=33, w=131, pixel_sample_rate=3)]


def main():
    spec = importlib.util.spec_from_file_location("reference_deduplication", sys.argv[1])
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref                  # dataclasses look their module up by name
    spec.loader.exec_module(ref)
    if ref.IMAGEHASH_AVAILABLE:
        raise SystemExit("imagehash imports here: this golden records the pixel-hash path")
    out = {"pillow": Image.__version__, "numpy": np.__version__, "cases": []}
    for case in CASES:
        clip = dr.make_clip(case["h"], case["w"])
        with tempfile.TemporaryDirectory() as d:
            d = Path(d)
            for i, f in enumerate(clip):
                Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(d / f"frame_{i + 1:08d}.png")
            dd = ref.FrameDeduplicator(ref.DeduplicationConfig(pixel_sample_rate=case["pixel_sample_rate"]))
            res = dd.analyze_frames(d, 25.0)
            files = sorted(d.glob("frame_*.png"))
            rec = asdict(res)
            rec["frame_mapping"] = {str(k): v for k, v in res.frame_mapping.items()}
            out["cases"].append(dict(case, hashes=[dd._hash_cache[p] for p in files], result=rec, summary=res.summary(),
                                     duplication_ratio=res.duplication_ratio, estimated_original_fps=res.estimated_original_fps))
    path = ROOT / "tests" / "golden" / "dedup_reference.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(path)


if __name__ == "__main__":
    main()
