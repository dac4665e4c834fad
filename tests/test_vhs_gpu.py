"""GPU: csrc/vhs.hip and framewright_amd/vhs.py against the contract in tests/vhs_ref.py and the results recorded from the reference
(tests/golden/vhs_reference.json).  Every comparison is exact equality; the jitter shifts are compared for W <= 258 (all clips) and
`rainbow_effect` as a decision, on fixtures that keep the recorded margin."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import vhs_ref as R
from framewright_amd import _lib
from framewright_amd import vhs as V

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NAMES = {"head_switching": "remove_head_switching", "tracking": "fix_tracking_errors", "dropout": "fix_dropout",
         "chroma_bleed": "reduce_chroma_bleed", "rainbow": "remove_rainbow_artifacts"}
CLIPS = R.clips()
SENTINEL, PAD = 0xA5, 64


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "vhs_reference.json").read_text())


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def proc(torch_mod):
    return V.DeviceVHSProcessor()


def upload(torch, clip, offset=None):
    """The clip on the device: one tensor per frame, or (``offset``) views that start that many bytes into a padded allocation."""
    if offset is None:
        return None, [torch.from_numpy(f).cuda() for f in clip]
    host = np.stack(clip)
    flat = np.full(host.size + 2 * PAD, SENTINEL, np.uint8)
    flat[PAD + offset: PAD + offset + host.size] = host.reshape(-1)
    buf = torch.from_numpy(flat).cuda()
    return buf, list(buf[PAD + offset: PAD + offset + host.size].view(host.shape).unbind(0))


def run_case(proc, dev, method, strength, seed, **kw):
    np.random.seed(seed)
    if method == "process":
        return proc.process(dev)
    return getattr(proc, NAMES[method])(dev, strength=strength, **kw)


def check_case(gold, name, dev, got, method, s):
    key = R.case_key(name, method, s)
    assert R.digest([t.cpu().numpy() for t in got]) == gold["cases"][key][0], key
    assert "".join("01"[a is b] for a, b in zip(got, dev)) == gold["cases"][key][1], key   # nothing to change: the input tensor itself


@pytest.mark.parametrize("name", list(CLIPS))
def test_methods_and_process_equal_the_reference(torch_mod, proc, gold, name):
    clip = CLIPS[name]
    _, dev = upload(torch_mod, clip)
    before = [t.clone() for t in dev]
    for method, s in R.recorded_cases(name) + [("process", 0.0)]:
        seed = gold["cases"][R.case_key(name, method, s)][2]
        got = run_case(proc, dev, method, s, seed)
        check_case(gold, name, dev, got, method, s)
        np.random.seed(seed)                                          # and the restatement, byte for byte
        want = R.process(clip, R.Config()) if method == "process" else R.METHODS[method](clip, R.Config(), s)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want)), (name, method, s)
    assert all(torch_mod.equal(a, b) for a, b in zip(dev, before))        # the inputs are never written


@pytest.mark.parametrize("name", ["mix_low/48x64", "mix_low/48x64/gray", "chroma5/48x64", "plain/48x64"])
def test_views_one_byte_into_their_storage(torch_mod, proc, gold, name):
    """The 16-byte-aligned size on frames that start at an odd byte; nothing around the frames is written."""
    buf, dev = upload(torch_mod, CLIPS[name], offset=1)
    for method, s in R.recorded_cases(name) + [("process", 0.0)]:
        got = run_case(proc, dev, method, s, gold["cases"][R.case_key(name, method, s)][2])
        check_case(gold, name, dev, got, method, s)
    host = buf.cpu().numpy()
    assert (host[:PAD + 1] == SENTINEL).all() and (host[-(PAD - 1):] == SENTINEL).all()


def test_nothing_to_do_returns_the_input(torch_mod, proc):
    _, dev = upload(torch_mod, CLIPS["plain/37x33"])
    for m in NAMES.values():
        assert getattr(proc, m)(dev, strength=0.0) is dev and getattr(proc, m)([]) == []
    assert proc.process([]) == []
    off = V.DeviceVHSProcessor(V.VHSConfig(tracking=0, head_switching=0, chroma_bleed=0, rainbow_removal=0, dropout_repair=0))
    assert off.process(dev) is dev and all(a is b for a, b in zip(off.stream(iter(dev), block=2), dev))
    _, gray = upload(torch_mod, CLIPS["jitter/37x33/gray"])
    for m in ("reduce_chroma_bleed", "remove_rainbow_artifacts"):
        out = getattr(proc, m)(gray, strength=1.0)
        assert out is not gray and all(a is b for a, b in zip(out, gray))
    assert all(a is b for a, b in zip(proc.fix_dropout(dev), dev))        # nothing detected


def test_progress_callbacks(torch_mod, proc):
    _, dev = upload(torch_mod, CLIPS["mix_low/37x33"])
    seen = []
    proc.fix_tracking_errors(dev, progress_callback=seen.append)
    assert seen == [(i + 1) / 5 for i in range(5)]
    seen.clear()
    np.random.seed(1)
    proc.process(dev, progress_callback=seen.append)
    assert seen == [(step + (i + 1) / 5) / 5 for step in range(5) for i in range(5)] + [1.0]


@pytest.mark.parametrize("name", list(CLIPS))
def test_detect_vhs_artifacts(torch_mod, proc, gold, name):
    rec, st = gold["analysis"][name], gold["stats"][name]
    frame = torch_mod.from_numpy(CLIPS[name][R.ANALYSIS_FRAME]).cuda()
    np.random.seed(rec["seed"])
    a = proc.detect_vhs_artifacts(frame)
    for k in ("head_switching_detected", "head_switching_position", "head_switching_severity", "tracking_errors", "tracking_severity",
              "tracking_line_positions", "dropout_detected", "dropout_count", "chroma_bleed", "chroma_bleed_severity", "dot_crawl",
              "jitter_detected", "jitter_severity"):
        assert getattr(a, k) == rec[k], (name, k)
    assert [list(p) for p in a.dropout_positions] == rec["dropout_positions"]
    if "rainbow_diag_max" in st:                                      # a decision, on fixtures that keep the margin
        ratio = st["rainbow_diag_max"] / (5 * st["rainbow_mean_mag"]) if st["rainbow_mean_mag"] else 0.0
        assert abs(ratio - 1.0) >= 1e-6
    assert a.rainbow_effect == rec["rainbow_effect"]
    assert a.overall_degradation == rec["overall_degradation"] and a.detected_quality.value == rec["detected_quality"]
    assert [x.artifact_type.value for x in a.all_artifacts] == rec["artifact_types"]
    assert a.summary().startswith(f"VHS Quality: {rec['detected_quality'].upper()}\n")
    # the exact integers behind the decisions; frame.shape[1] <= 258, so the shifts are the reference's too
    stats = proc.gray_stats_device([frame], sums=True)
    host = CLIPS[name][R.ANALYSIS_FRAME]
    assert stats["row_sums"][0].tolist() == R.row_diff_sums(R.gray(host)).tolist()
    extra = proc.analysis_device(frame)
    assert extra["jitter_shifts"].tolist() == st["jitter_shifts"]
    if frame.dim() == 3:
        assert extra["column_sums"].tolist() == R.dot_crawl_column_sums(host).tolist()
        assert int(proc.edge_counts_device([frame]).sum()) == st["n_edges"]


def test_run_list_overflow_runs_again(torch_mod, proc, gold):
    name = "mix_low/48x64"
    _, dev = upload(torch_mod, CLIPS[name])
    want = sorted(tuple(r) for i, f in enumerate(CLIPS[name]) for r in [(i, x, y, n) for x, y, n, _ in R.dropout_runs(R.gray(f), 5)])
    assert len(want) > 8
    for cap in (1, 3, len(want), None):
        runs = proc.gray_stats_device(dev, runs=True, run_capacity=cap)["runs"]
        assert sorted(tuple(r) for r in runs.tolist()) == want, cap
    got = proc.fix_dropout(dev, strength=0.7, _run_capacity=2)
    check_case(gold, name, dev, got, "dropout", 0.7)
    rec = gold["analysis"][name]
    np.random.seed(rec["seed"])
    assert proc.detect_vhs_artifacts(dev[R.ANALYSIS_FRAME], _run_capacity=1).dropout_count == rec["dropout_count"]


def test_repair_groups_split_where_boxes_meet():
    ops = [(0, 2, 10, 3, 11, 1), (1, 0, 5, 10, 5, 1), (1, 0, 7, 10, 13, 2), (1, 0, 30, 10, 5, 1), (0, 1, 34, 10, 3, 1)]
    groups = V._repair_groups(ops)
    assert [len(g) for g in groups] == [2, 2, 1]                      # the fifth box touches the fourth box's right flank


def test_refusals(torch_mod, proc, hip_lib):
    torch = torch_mod
    ok = torch.zeros((32, 8, 3), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((31, 8, 3), dtype=torch.uint8, device="cuda"), torch.zeros((32, 8, 3), dtype=torch.float32, device="cuda"),
                torch.zeros((32, 8, 3), dtype=torch.uint8), torch.zeros((32, 1, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((32, 8, 4), dtype=torch.uint8, device="cuda")):
        for m in NAMES.values():
            with pytest.raises(ValueError):
                getattr(proc, m)([bad])
        with pytest.raises(ValueError):
            proc.process([bad])
        with pytest.raises(ValueError):
            proc.detect_vhs_artifacts(bad)
        with pytest.raises(ValueError):
            list(proc.stream(iter([ok, bad]), block=1))
    with pytest.raises(ValueError):
        proc.process([ok, torch.zeros((32, 9, 3), dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError):
        V.VHSConfig(tracking=1.5)
    with pytest.raises(ValueError):
        V.DeviceVHSProcessor(V.VHSConfig(temporal_radius=40)).fix_dropout([ok])
    # an output that overlaps an input
    buf = torch.zeros((2 * ok.numel(),), dtype=torch.uint8, device="cuda")
    a, b = buf[:ok.numel()].view(ok.shape), buf[16:16 + ok.numel()].view(ok.shape)
    with pytest.raises(ValueError):
        proc.rainbow_device([a], 0.5, outs=[b])
    with pytest.raises(ValueError):
        proc.rainbow_device([a], 0.5, outs=[a])
    p = lambda t: C.c_void_p(t.data_ptr())                           # noqa: E731
    tab = lambda *ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
    spec_i, spec_f = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    i64 = torch.zeros((64,), dtype=torch.int64, device="cuda")
    shifts = (C.c_int32 * 1)(1)
    inv = _lib.FW_ERR_INVALID
    assert hip_lib.fw_vhs_rainbow_u8(tab(a), tab(b), 1, 32, 8, 0.5, 0.5, None) == inv
    assert b"overlaps" in hip_lib.fw_last_error()
    assert hip_lib.fw_vhs_blend_rows_u8(tab(a), tab(a), 1, 32, 24, p(spec_i), p(spec_f), 1, None) == inv
    assert hip_lib.fw_vhs_chroma_shift_u8(tab(a), tab(b), shifts, 1, 32, 8, None) == inv
    assert hip_lib.fw_vhs_chroma_shift_u8(tab(ok), tab(a), (C.c_int32 * 1)(3), 1, 32, 8, None) == inv
    assert hip_lib.fw_vhs_dropout_repair_u8(tab(a), 1, tab(b), 1, 32, 8, 3, p(spec_i), 1, 0.5, None) == inv
    assert hip_lib.fw_vhs_dropout_repair_u8(tab(ok), 1, tab(a), 1, 32, 8, 3, p(spec_i), 1, 0.0, None) == inv
    assert hip_lib.fw_vhs_rainbow_u8(tab(ok), None, 1, 32, 8, 0.5, 0.5, None) == inv
    assert hip_lib.fw_vhs_rainbow_u8(tab(ok), tab(a), 33, 32, 8, 0.5, 0.5, None) == inv
    assert hip_lib.fw_vhs_gray_stats_u8(tab(ok), 1, 32, 8, 3, 5, None, None, None, 0, None, None) == inv
    assert hip_lib.fw_vhs_gray_stats_u8(tab(ok), 1, 32, 8, 2, 5, p(i64), None, None, 0, None, None) == inv
    assert hip_lib.fw_vhs_gray_stats_u8(tab(ok), 1, 32, 8, 3, 5, None, None, p(i64), 4, None, None) == inv
    assert hip_lib.fw_vhs_gray_stats_u8(tab(ok), 1, 20, 8, 3, 5, None, p(i64), None, 0, None, None) == inv
    assert hip_lib.fw_vhs_box_gray_sums_u8(tab(ok), 1, 32, 8, 3, p(spec_i), 0, p(i64), None) == inv
    assert hip_lib.fw_vhs_column_sums_u8(p(ok), 32, 1, p(i64), None) == inv
    assert hip_lib.fw_vhs_jitter_shifts_u8(p(ok), 2, 8, 3, p(spec_i), None) == inv
    assert hip_lib.fw_vhs_saturation_f64(None, 32, 8, p(i64), None) == inv
    assert hip_lib.fw_vhs_edge_counts_u8(tab(ok), 1, 32, 0, p(spec_i), None) == inv
    assert hip_lib.fw_vhs_chroma_samples_u8(tab(ok), 1, 32, 8, p(spec_i), 7000, p(spec_i), None) == inv
    torch.cuda.synchronize()


def test_table_entries_outside_the_frame_are_skipped(torch_mod, proc):
    """The row, box and sample tables are in device memory, where the entry cannot check them: the kernels do."""
    torch = torch_mod
    clip = CLIPS["mix_low/37x33"]
    _, dev = upload(torch, clip[:2])
    out = dev[0].clone()
    rows = np.array([[0, 37, 1, 2], [0, 3, -1, 2], [1, 3, 2, 4], [0, 5, 4, 6]], dtype=np.int32)       # only the last is valid (one dst)
    proc.blend_rows_device([dev[0]], [out], rows, np.array([[0.5, 0.5]] * 4, dtype=np.float32))
    want = clip[0].copy()
    want[5] = (np.float32(0.5) * ((clip[0][4].astype(np.float32) + clip[0][6].astype(np.float32)) / 2) + np.float32(0.5) * clip[0][5].astype(np.float32)).astype(np.uint8)
    assert np.array_equal(out.cpu().numpy(), want)
    sums = proc.box_sums_device(dev, np.array([[0, 30, 3, 4, 1], [2, 0, 0, 1, 1], [0, -1, 0, 2, 2], [1, 2, 3, 4, 5]], dtype=np.int32))
    assert sums.tolist() == [-1, -1, -1, R.box_gray_sum(clip[1], (2, 3, 4, 5))]
    res = dev[1].clone()
    boxes = np.array([[0, 1, 0, 2, 2, 3, 3, 0], [0, 0, 5, 2, 2, 3, 3, 0], [1, 0, 0, 0, 2, 3, 3, 0], [1, 0, 0, 30, 2, 3, 3, 0],
                      [2, 0, 0, 2, 2, 3, 3, 0], [0, 0, 0, 2, 36, 3, 3, 0]], dtype=np.int32)
    proc.repair_device([dev[0]], [res], boxes, 0.5)
    assert torch.equal(res, dev[1])
    offs = proc.chroma_samples_device(dev, np.array([[0, 40, 0], [3, 0, 0], [0, 0, 10000], [0, 0, -1]], dtype=np.int32))
    assert offs.tolist() == [[-2, -2]] * 4


def test_two_runs_are_identical(torch_mod, proc, gold):
    name = "mix_low/64x258"
    _, dev = upload(torch_mod, CLIPS[name])
    outs, sums = [], []
    for _ in range(2):
        np.random.seed(7)
        outs.append([t.cpu().numpy() for t in proc.process(dev)])
        st = proc.gray_stats_device(dev, sums=True, bottom=True)
        sums.append((st["row_sums"], st["bottom"], proc.analysis_device(dev[0])["column_sums"]))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(*sums)) and sums[0][0].dtype == np.int64


def test_a_private_generator_leaves_the_global_one_alone(torch_mod, gold):
    name = "chroma5/48x64"
    _, dev = upload(torch_mod, CLIPS[name])
    seed = gold["cases"][R.case_key(name, "chroma_bleed", 1.0)][2]
    np.random.seed(123)
    state = np.random.get_state()[1].copy()
    got = V.DeviceVHSProcessor(rng=np.random.RandomState(seed)).reduce_chroma_bleed(dev, strength=1.0)
    assert np.array_equal(np.random.get_state()[1], state)
    check_case(gold, name, dev, got, "chroma_bleed", 1.0)            # RandomState(seed) draws what np.random.seed(seed) draws
    p = V.create_vhs_processor(tracking=0.25)
    assert p.config == V.VHSConfig(tracking=0.25) and V.VHSQuality.EP.horizontal_resolution == 200


def test_long_list_crosses_the_batches(torch_mod, proc):
    """More than 32 frames: two statistics launches, dropout batches with neighbours on both sides."""
    base = CLIPS["mix_low/37x33"]
    clip = [base[i % 5] if i % 7 else base[(i + 2) % 5] for i in range(40)]
    _, dev = upload(torch_mod, clip)
    np.random.seed(5)
    got = proc.process(dev)
    np.random.seed(5)
    want = R.process(clip, R.Config())
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
