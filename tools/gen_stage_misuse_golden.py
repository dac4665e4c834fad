#!/usr/bin/env python3
"""Writes tests/golden/stage_misuse.json and tests/golden/stage_outputs.json: what the eleven frame-stage drivers answer to the misuse
listed in tests/stage_misuse_cases.py, and sha256 digests of what their device and host calls produce on seeded synthetic frames.
Every driver constructor asks for a device, so this needs a GPU.

    python tools/gen_stage_misuse_golden.py            # record
    python tools/gen_stage_misuse_golden.py --verify   # record again and compare with the files: nothing may differ

Run it on the commit whose behaviour is to be pinned, before a change that must not alter it, and keep the files only when a second
run (--verify) agrees with the first.  A case with a literal answer in the case list is written with that answer and marked
``"literal": true``: it states an intended difference, not a recording.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import stage_misuse_cases as M  # noqa: E402


def main() -> None:
    verify = "--verify" in sys.argv[1:]
    ctx = M.Context()
    misuse = []
    for driver, label, call, literal in M.misuse_cases():
        rec = {"driver": driver, "case": label, "answer": literal if literal is not None else M.answer(call, ctx)}
        if literal is not None:
            rec["literal"] = True
        misuse.append(rec)
    outputs = M.record_outputs(ctx)
    golden = ROOT / "tests" / "golden"
    failed = False
    for name, data in (("stage_misuse.json", misuse), ("stage_outputs.json", outputs)):
        path = golden / name
        if verify:
            kept = json.loads(path.read_text())
            same = kept == data
            failed |= not same
            print(f"{path}: {'agrees' if same else 'DIFFERS'}")
            if not same and len(kept) == len(data):
                for k, now in (enumerate(data) if isinstance(data, list) else data.items()):
                    old = kept[k] if isinstance(kept, list) else kept.get(k)
                    if old != now:
                        print(f"  {k}: kept {old}\n  {k}: now  {now}")
        else:
            path.write_text(json.dumps(data, indent=0, ensure_ascii=False) + "\n")
            print(f"{path}: {len(data)} cases, {path.stat().st_size} bytes")
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
