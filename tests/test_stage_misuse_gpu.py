"""The misuse surface and the outputs of the eleven frame-stage drivers, pinned: tests/golden/stage_misuse.json holds what the drivers
answered to the calls of tests/stage_misuse_cases.py when tools/gen_stage_misuse_golden.py recorded them (exception class, message
and code, or a description of the value returned), tests/golden/stage_outputs.json the sha256 of what every driver's device calls
and host calls return on six seeded 40 x 56 frames.  The same calls must be answered the same way and give the same bytes.  The
cases that carry a literal answer in the case list are deliberate differences from the recording ("Stage
drivers (Python)") and are asserted as written there."""
import json

import pytest

import stage_misuse_cases as M

pytestmark = pytest.mark.gpu

CASES = M.misuse_cases()
OUTPUTS = M.output_cases()


def _id(*parts):
    return "-".join(p.replace(" ", "_") for p in parts)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "stage_misuse.json").read_text())


@pytest.fixture(scope="module")
def golden_outputs(golden_dir):
    return json.loads((golden_dir / "stage_outputs.json").read_text())


@pytest.fixture(scope="module")
def ctx(hip_lib):
    return M.Context()


def test_case_list_names_all_eleven_drivers():
    assert len(M.DRIVERS) == 11
    assert sorted({c[0] for c in CASES}) == sorted(M.DRIVERS)
    assert sorted(M.MAKE) == sorted(M.DRIVERS)
    assert sorted({label.split(" ")[0] for label, _ in OUTPUTS}) == sorted(M.DRIVERS)


def test_golden_lists_the_same_cases(golden, golden_outputs):
    assert [(g["driver"], g["case"], g.get("literal", False)) for g in golden] == [(c[0], c[1], c[3] is not None) for c in CASES]
    assert list(golden_outputs) == [label for label, _ in OUTPUTS]


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c[0], c[1]) for c in CASES])
def test_answer_is_unchanged(ctx, golden, index):
    driver, label, call, literal = CASES[index]
    want = literal if literal is not None else golden[index]["answer"]
    assert M.answer(call, ctx) == want


@pytest.mark.parametrize("index", range(len(OUTPUTS)), ids=[_id(label) for label, _ in OUTPUTS])
def test_outputs_are_unchanged(ctx, golden_outputs, index):
    import torch
    label, call = OUTPUTS[index]
    got = call(ctx)
    torch.cuda.synchronize()
    assert M.digest(M.as_frames(got)) == golden_outputs[label]
