"""GPU: csrc/perceptual.hip and `framewright_amd.perceptual` against tests/perceptual_ref.py, byte for byte with no pixel excluded.

The stencil kernel's tile is 64 columns by 32 rows with a 9-pixel halo (sharpen) and a 2-pixel halo (grain); CLAHE has 8 x 8 tiles.
Shapes: 24 x 40 (CLAHE tiles divide, one workgroup tile), 37 x 53 (CLAHE pads by reflection, 5 x 7 tiles), 67 x 130 (crosses
workgroup-tile seams both ways), 9 x 200 and 200 x 9 (the 9-pixel halo is as wide as the frame: the 19 taps reflect twice), 8 x 8
(the refusal boundary with detail on).  The grain step also runs at the amount and on the frame where a tail contracted into one
fused multiply-add would give other bytes.  The configurations are the ones tests/golden/perceptual_reference.json records; those with
a non-local-means step run on the small shapes only, and on the others with that step taken out of the plan on both sides."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import perceptual_ref as R
from framewright_amd import _lib
from framewright_amd import perceptual as PT

pytestmark = pytest.mark.gpu
SHAPES = [(24, 40), (37, 53), (67, 130), (9, 200), (200, 9), (8, 8)]
SMALL = [(24, 40), (37, 53), (8, 8)]
sid = lambda s: f"{s[0]}x{s[1]}"        # noqa: E731


def _cases():
    with open(Path(__file__).resolve().parent / "golden" / "perceptual_reference.json") as f:
        return json.load(f)["cases"]


CASES = _cases()


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    _lib.require_gpu()
    return torch


def config_of(kw, module):
    return module.PerceptualConfig(**{**kw, "mode": module.PerceptualMode(kw["mode"])})


@pytest.fixture(scope="module")
def tuner(torch_mod):
    t = PT.DevicePerceptualTuner()
    yield t
    t.close()


@pytest.fixture(scope="module")
def frames():
    return {s: R.content_frame(*s) for s in SHAPES}


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    bad = np.argwhere(np.any(got != want, axis=-1)) if got.ndim == 3 else np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {bad[:4].tolist()}"


def test_device_table_equals_the_restatement(tuner):
    got = tuner.gauss19_table()
    assert got.tolist() == R.gauss19_table().tolist() and int(got.sum()) == 256


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_unsharp_step(torch_mod, tuner, frames, shape):
    x = frames[shape]
    for w_src, w_blur in ((1 + 0.35 * 1.5, -(0.35 * 1.5)), (1 + 0.4 * 1.5, -(0.4 * 1.5)), (1 + 0.9, -0.9)):
        t = cuda(torch_mod, x)
        got = host(torch_mod, tuner.unsharp_device(t, w_src, w_blur))
        want = R.unsharp_u8(x, float(np.float32(w_src)), float(np.float32(w_blur)))
        same(got, want, f"unsharp {shape} {w_src}")
        assert np.array_equal(host(torch_mod, t), x)
    assert ((want == 0) | (want == 255)).any()                   # the sharpened value left [0, 255] somewhere
    if shape == (67, 130):                                       # a kernel whose addWeighted was contracted would not have passed above
        w_src, w_blur = float(np.float32(1 + 0.35 * 1.5)), float(np.float32(-(0.35 * 1.5)))
        assert not np.array_equal(R.add_weighted_fused(x, w_src, R.gaussian_blur_sigma3_u8(x), w_blur), R.unsharp_u8(x, w_src, w_blur))


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_saturation_step(torch_mod, tuner, frames, shape):
    x = frames[shape]
    for boost in (1.075, 1.15):
        same(host(torch_mod, tuner.saturation_device(cuda(torch_mod, x), boost)), R.saturation_u8(x, float(np.float32(boost))), f"saturation {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_clahe_and_detail_steps(torch_mod, tuner, frames, shape):
    x = frames[shape]
    plane = np.ascontiguousarray(R.fl.bgr_to_lab_gamma(x)[:, :, 0])
    for clip in (2.0, 2.6, 1.4):
        same(host(torch_mod, tuner.clahe_device(cuda(torch_mod, plane), clip)), R.hd.clahe(plane, clip), f"clahe {shape} {clip}")
        same(host(torch_mod, tuner.detail_device(cuda(torch_mod, x), clip)), R.detail_u8(x, clip), f"detail {shape} {clip}")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_grain_step(torch_mod, tuner, frames, shape):
    original = frames[shape]
    result = R.content_frame(*shape, seed=5)
    for amount in (0.35, 0.5):
        want = R.grain_tail_u8(result, original, float(np.float32(amount)))
        same(host(torch_mod, tuner.grain_device(cuda(torch_mod, result), cuda(torch_mod, original), amount)), want, f"grain {shape} {amount}")
    assert (R.grain_u8(original) == 0).any() and (R.grain_u8(original) > 0).any()
    # the amount and the frame on which a tail contracted into one multiply-add gives other bytes (perceptual_ref.FMA_BALANCE)
    amount = R.plan(R.PerceptualConfig(balance=R.FMA_BALANCE))["grain_amount"]
    sensitive = R.tail_sensitive_result(result, original, amount)
    want = R.grain_tail_u8(sensitive, original, amount)
    same(host(torch_mod, tuner.grain_device(cuda(torch_mod, sensitive), cuda(torch_mod, original), amount)), want, f"grain {shape}, sensitive")
    assert not np.array_equal(R.grain_tail_fused(sensitive, original, amount), want)


LIMITS_SHAPE = (160, 200)                                       # CLAHE tiles of 20 x 25 = 500 pixels: the integer limit depends on the clip


def test_clahe_limits_above_one(torch_mod, tuner):
    """At the six shapes above every tile has at most 153 pixels and max(int(clip * area / 256), 1) is 1 for every clip: a kernel that
    ignored its limit would pass them.  Here the limits are 5 (2.6), 4 (2.36), 3 (2.0) and 2 (1.4), the outputs differ pairwise, and the
    CLAHE entry, the detail entry and the fused whole are held to the restatement at each."""
    h, w = LIMITS_SHAPE
    clips = (2.6, 1.0 + (0.2 + (0.8 - 0.2) * 0.8) * 2.0, 2.0, 1.4)
    assert [R.clahe_limit(c, h, w) for c in clips] == [5, 4, 3, 2] == [PT.clahe_limit(c, h, w) for c in clips]
    x = R.content_frame(h, w)
    plane = np.ascontiguousarray(R.fl.bgr_to_lab_gamma(x)[:, :, 0])
    planes, details = [], []
    for clip in clips:
        planes.append(R.hd.clahe(plane, clip))
        details.append(R.detail_u8(x, clip))
        same(host(torch_mod, tuner.clahe_device(cuda(torch_mod, plane), clip)), planes[-1], f"clahe, clip {clip}")
        same(host(torch_mod, tuner.detail_device(cuda(torch_mod, x), clip)), details[-1], f"detail, clip {clip}")
    for i in range(len(clips)):
        for j in range(i):
            assert not np.array_equal(planes[i], planes[j]) and not np.array_equal(details[i], details[j]), (clips[i], clips[j])
    for case, limit in (("enhanced|grain1", 5), ("balanced0.8|grain0|limits1", 4), ("balanced0.5|grain1", 3)):
        t = PT.DevicePerceptualTuner(config_of(CASES[case]["config"], PT))
        plan = PT.PerceptualPlan(**{**t.plan().to_dict(), "steps": tuple(s for s in t.plan().steps if s != "denoise"), "h": 0})
        rplan = ref_plan_without_denoise(R.plan(config_of(CASES[case]["config"], R)))
        assert PT.clahe_limit(plan.clip_limit, h, w) == limit and plan.clip_limit == rplan["clip_limit"]
        want = R.apply_plan(x, rplan)
        same(host(torch_mod, t.apply_frame_device(cuda(torch_mod, x), plan=plan)), want, f"{case} at {LIMITS_SHAPE}")
        if limit != 3:                                           # the planted defect: limit 2.0 where the plan says otherwise
            assert not np.array_equal(R.apply_plan(x, {**rplan, "clip_limit": 2.0}), want), case
        t.close()


def test_frames_on_another_gpu_are_refused(torch_mod, tuner, frames):
    if torch_mod.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    with pytest.raises(ValueError, match=r"frames on cuda:0, the tuner's device, expected"):
        tuner.apply_frame_device(torch_mod.from_numpy(frames[(24, 40)]).to("cuda:1"))


def ref_plan_without_denoise(pl):
    return {**pl, "steps": [s for s in pl["steps"] if s != "denoise"], "h": 0}


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_whole(torch_mod, frames, case, shape):
    x = frames[shape]
    rcfg = config_of(CASES[case]["config"], R)
    tuner = PT.DevicePerceptualTuner(config_of(CASES[case]["config"], PT))
    assert tuner.get_profile().to_dict() == CASES[case]["profile"] and tuner.plan().to_dict() == CASES[case]["plan"]
    plan, rplan = tuner.plan(), R.plan(rcfg)
    if plan.h and shape not in SMALL:                            # the non-local means on the small shapes only
        plan = PT.PerceptualPlan(**{**plan.to_dict(), "steps": tuple(s for s in plan.steps if s != "denoise"), "h": 0})
        rplan = ref_plan_without_denoise(rplan)
    t = cuda(torch_mod, x)
    first = tuner.apply_frame_device(t, plan=plan)
    second = tuner.apply_frame_device(t, plan=plan)
    got, again = host(torch_mod, first), host(torch_mod, second)
    same(got, R.apply_plan(x, rplan), f"{case} {shape}")
    assert np.array_equal(got, again) and first.data_ptr() != t.data_ptr()
    assert np.array_equal(host(torch_mod, t), x)                 # the input is left as it is
    if sid(shape) in CASES[case]["sha256"]:                      # the recorded sizes are small ones: nothing was taken out of the plan
        assert hashlib.sha256(got.tobytes()).hexdigest() == CASES[case]["sha256"][sid(shape)]
    tuner.close()


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
@pytest.mark.parametrize("case", ["balanced0.5|grain1", "enhanced|grain0", "balanced0.8|grain1|limits1"])
def test_fused_equals_the_steps_chained(torch_mod, frames, case, shape):
    tuner = PT.DevicePerceptualTuner(config_of(CASES[case]["config"], PT))
    plan = tuner.plan()
    if shape not in SMALL:
        plan = PT.PerceptualPlan(**{**plan.to_dict(), "steps": tuple(s for s in plan.steps if s != "denoise"), "h": 0})
    t = cuda(torch_mod, frames[shape])
    x = t
    for step in plan.steps:
        if step == "denoise":
            from framewright_amd.temporal_denoise import DeviceSpatialDenoiser
            x = DeviceSpatialDenoiser().denoise_device(x, plan.h, plan.h)
        elif step == "sharpen":
            x = tuner.unsharp_device(x, plan.w_src, plan.w_blur)
        elif step == "colour":
            x = tuner.saturation_device(x, plan.boost)
        elif step == "detail":
            x = tuner.detail_device(x, plan.clip_limit)
        else:
            x = tuner.grain_device(x, t, plan.grain_amount)
    same(host(torch_mod, tuner.apply_frame_device(t, plan=plan)), host(torch_mod, x), f"{case} {shape}")
    tuner.close()


def test_no_step_is_a_copy_and_lists_keep_repeats(torch_mod, frames):
    tuner = PT.DevicePerceptualTuner(PT.PerceptualConfig(mode=PT.PerceptualMode.FAITHFUL, preserve_grain=False))
    assert tuner.plan().steps == ()
    x = frames[(24, 40)]
    a, b = cuda(torch_mod, x), cuda(torch_mod, x[::-1])
    outs = tuner.apply_device([a, b, a])
    assert outs[0] is outs[2] and outs[0] is not a and outs[0].data_ptr() != a.data_ptr()
    assert np.array_equal(host(torch_mod, outs[0]), x) and np.array_equal(host(torch_mod, outs[1]), x[::-1])
    tuner.close()
    tuner = PT.DevicePerceptualTuner()
    outs = tuner.apply_device([a, b, a])
    want = R.apply_to_frame(x, R.PerceptualConfig())
    assert outs[0] is outs[2]
    same(host(torch_mod, outs[0]), want, "list")
    got = tuner.apply([x, x[::-1]])
    same(got[0], want, "apply")
    same(got[1], R.apply_to_frame(np.ascontiguousarray(x[::-1]), R.PerceptualConfig()), "apply, flipped")
    same(host(torch_mod, next(tuner.stream(iter([a])))), want, "stream")
    tuner.close()


def test_apply_directory_with_injected_reader_and_writer(torch_mod, frames, tmp_path):
    x = frames[(24, 40)]
    src = tmp_path / "in"
    src.mkdir()
    for name in ("b.png", "a.png", "c.png"):
        (src / name).write_bytes(name.encode())
    written = {}
    tuner = PT.DevicePerceptualTuner()
    n = tuner.apply_directory(src, tmp_path / "out", read_fn=lambda p: None if p.name == "c.png" else x,
                              write_fn=lambda p, img: written.__setitem__(p.name, img))
    assert n == 2 and sorted(written) == ["a.png", "b.png"]
    same(written["a.png"], R.apply_to_frame(x, R.PerceptualConfig()), "directory")
    tuner.close()


def test_refusals(torch_mod, hip_lib, tuner, frames):
    torch = torch_mod
    x = cuda(torch, frames[(24, 40)])
    seven = cuda(torch, R.content_frame(7, 40))
    with pytest.raises(ValueError, match="8 .. 16384 pixels a side expected with detail recovery"):
        tuner.apply_frame_device(seven)
    grain_only = PT.DevicePerceptualTuner(PT.PerceptualConfig(mode=PT.PerceptualMode.FAITHFUL))
    same(host(torch, grain_only.apply_frame_device(seven)), R.apply_to_frame(R.content_frame(7, 40), R.PerceptualConfig(mode=R.PerceptualMode.FAITHFUL)), "7 rows")
    with pytest.raises(ValueError, match="8-bit only"):
        tuner.apply_frame_device(x.to(torch.int16))
    with pytest.raises(ValueError, match="uint8 CUDA tensors H x W x 3"):
        tuner.apply_frame_device(x.float())
    with pytest.raises(ValueError, match="not gray planes"):
        tuner.apply_frame_device(x[:, :, 0].contiguous())
    with pytest.raises(ValueError, match=r"frames on cuda:0, the tuner's device, expected"):
        tuner.apply_frame_device(x.cpu())
    buf = torch.zeros(24 * 40 * 3 + 30, dtype=torch.uint8, device="cuda")
    a, b = buf[:2880].view(24, 40, 3), buf[30:2910].view(24, 40, 3)
    with pytest.raises(ValueError, match="a destination overlaps a source frame"):
        tuner.apply_frame_device(a, out=b)
    st = _lib.stream_ptr(x.device)
    assert hip_lib.fw_ptune_unsharp_u8(_lib.ptr(a), _lib.ptr(b), 24, 40, 1.5, -0.5, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_unsharp_u8: dst overlaps a source frame (every output reads a neighbourhood)"
    assert hip_lib.fw_ptune_grain_u8(_lib.ptr(x), _lib.ptr(a), _lib.ptr(b), 24, 40, 0.5, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_grain_u8: dst overlaps a source frame (every output reads a neighbourhood)"
    assert hip_lib.fw_ptune_unsharp_u8(None, _lib.ptr(b), 24, 40, 1.5, -0.5, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_unsharp_u8: null pointer"
    assert hip_lib.fw_ptune_unsharp_u8(_lib.ptr(x), _lib.ptr(b), 24, 40, float("nan"), -0.5, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_unsharp_u8: finite weights expected"
    assert hip_lib.fw_ptune_apply_u8(_lib.ptr(x), _lib.ptr(b), 24, 40, None, None, st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_apply_u8: null pointer"
    scratch = torch.empty(int(hip_lib.fw_ptune_scratch_bytes(8, 40, None)), dtype=torch.uint8, device="cuda")
    assert hip_lib.fw_ptune_detail_u8(_lib.ptr(seven), _lib.ptr(b), 7, 40, 1, _lib.ptr(scratch), st) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_last_error() == b"fw_ptune_detail_u8: 8 .. 16384 pixels a side expected with detail recovery (8 x 8 CLAHE tiles)"
    assert hip_lib.fw_ptune_scratch_bytes(2, 40, None) == 0 and hip_lib.fw_ptune_scratch_bytes(8, 40, None) == 81920
    grain_only.close()
    with pytest.raises(ValueError, match="the tuner is closed"):
        grain_only.apply_frame_device(x)
