"""The status and last-error message of every frame-stage entry, pinned: tests/golden/stage_errors.json holds what the library
answered to the invalid calls of tests/stage_error_cases.py when tools/gen_stage_errors_golden.py recorded them, and the same calls
must be answered with the same status and the same message bytes.  Every call is refused before the first HIP call: no kernel is
launched and no device is needed."""
import json

import pytest

import stage_error_cases as S
from framewright_amd import _lib

CASES = S.cases()
# every entry the nine stage files define (scene_cuts, dedup_hash, optical_flow, nlmeans, temporal_chain, flicker, color_lut,
# deinterlace, vhs): include/framewright_hip.h from fw_farneback_scratch_bytes up to, not including, fw_aspect_bar_sums_u8
STAGE_ENTRIES = _lib.EXPORTS[_lib.EXPORTS.index("fw_farneback_scratch_bytes"):_lib.EXPORTS.index("fw_aspect_bar_sums_u8")]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "stage_errors.json").read_text())


def test_every_stage_entry_has_a_case():
    assert len(STAGE_ENTRIES) == 42     # a reordered header must not shrink the set unseen
    assert sorted({c[0] for c in CASES}) == sorted(STAGE_ENTRIES)


def test_golden_lists_the_same_calls(golden):
    assert [(g["entry"], g["args"]) for g in golden] == [(c[0], c[1]) for c in CASES]
    assert all(g["status"] in (0, _lib.FW_ERR_INVALID) for g in golden)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[f"{c[0]}-{c[1].replace(' ', '_')}" for c in CASES])
def test_refusal_is_unchanged(hip_lib, golden, index):
    got = S.replay(hip_lib, CASES[index])
    assert got == golden[index]
