"""The misuse surface and the frames of the six network engines, pinned: tests/golden/engine_misuse.json holds what the engines
answered to the calls of tests/engine_misuse_cases.py when tools/gen_engine_misuse_golden.py recorded them (exception class, message
and code, or the value returned), tests/golden/engine_outputs.json the sha256 of the frames of every engine's device and host
forward and of the three stream fan-outs.  The same calls must be answered the same way and give the same bytes.  The cases that
carry a literal answer in the case list are deliberate differences from the recording ("Engine owners
(Python)") and are asserted as written there."""
import json

import pytest

import engine_misuse_cases as M

pytestmark = pytest.mark.gpu

CASES = M.misuse_cases()
OUTPUTS = M.output_cases()
ENGINES = ["NAFNetEngine", "RRDBNetEngine", "IFNetEngine", "RestormerEngine", "SRVGGNetEngine", "AESRGANEngine"]


def _id(*parts):
    return "-".join(p.replace(" ", "_") for p in parts)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "engine_misuse.json").read_text())


@pytest.fixture(scope="module")
def golden_outputs(golden_dir):
    return json.loads((golden_dir / "engine_outputs.json").read_text())


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = M.Context()
    yield c
    c.close()


def test_case_list_names_all_six_engines():
    assert sorted({c[0] for c in CASES}) == sorted(ENGINES)
    assert sorted(M.KINDS) == sorted(ENGINES)


def test_golden_lists_the_same_cases(golden, golden_outputs):
    assert [(g["engine"], g["case"], g.get("literal", False)) for g in golden] == [(c[0], c[1], c[3] is not None) for c in CASES]
    assert list(golden_outputs) == [label for label, _ in OUTPUTS]


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c[0], c[1]) for c in CASES])
def test_answer_is_unchanged(ctx, golden, index):
    engine, label, call, literal = CASES[index]
    want = literal if literal is not None else golden[index]["answer"]
    assert M.answer(call, ctx) == want


@pytest.mark.parametrize("index", range(len(OUTPUTS)), ids=[_id(label) for label, _ in OUTPUTS])
def test_frames_are_unchanged(ctx, golden_outputs, index):
    import torch
    label, call = OUTPUTS[index]
    frames = call(ctx)
    torch.cuda.synchronize()
    assert M.digest(frames) == golden_outputs[label]
