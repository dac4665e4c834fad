#!/usr/bin/env python3
"""Writes tests/golden/stage_errors.json: the status and the fw_last_error() message of every invalid call listed in
tests/stage_error_cases.py, as the built library answers them.  The calls are refused before the first HIP call, so this runs on a
build machine without a GPU.

    python tools/gen_stage_errors_golden.py

Run it on the commit whose messages are to be pinned, before a change that must not alter them.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import stage_error_cases as S  # noqa: E402

from framewright_amd import _lib  # noqa: E402


def main() -> None:
    lib = _lib.load()
    records = [S.replay(lib, case) for case in S.cases()]
    for r in records:
        # a refusal is FW_ERR_INVALID from a status entry and 0 from an entry that returns a size or a count
        assert r["status"] in (0, _lib.FW_ERR_INVALID), r
    path = ROOT / "tests" / "golden" / "stage_errors.json"
    path.write_text(json.dumps(records, indent=0, ensure_ascii=False) + "\n")
    print(f"{path}: {len(records)} calls of {len({r['entry'] for r in records})} entries, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
