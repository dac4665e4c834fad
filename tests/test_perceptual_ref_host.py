"""CPU: tests/perceptual_ref.py and the host logic of `framewright_amd.perceptual` against what tools/gen_perceptual_golden.py recorded
from the reference's own `processors/perceptual_tuning.py` (tests/golden/perceptual_reference.json / .npz), and the planted defects:
each of them must change at least one byte of the test frames, or a kernel that has it would pass the GPU tests."""
import hashlib
import json

import numpy as np
import pytest

import perceptual_ref as R
from framewright_amd import perceptual as PT


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(golden_dir / "perceptual_reference.json") as f:
        js = json.load(f)
    with np.load(golden_dir / "perceptual_reference.npz") as z:
        arrays = {k: z[k] for k in z.files}
    return js, arrays


def config_of(kw, module):
    return module.PerceptualConfig(**{**kw, "mode": module.PerceptualMode(kw["mode"])})


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def frame(golden, size="24x40"):
    return golden[1][f"input|{size}"]


def test_inputs_are_the_recorded_ones(golden):
    js, arrays = golden
    for h, w in js["sizes"]:
        assert np.array_equal(R.content_frame(h, w), arrays[f"input|{h}x{w}"]) and sha(arrays[f"input|{h}x{w}"]) == js["inputs"][f"{h}x{w}"]


def test_restatement_equals_the_recorded_outputs(golden):
    js, arrays = golden
    seen = 0
    for name, case in js["cases"].items():
        for size, digest in case["sha256"].items():
            got = R.apply_to_frame(arrays[f"input|{size}"], config_of(case["config"], R))
            assert sha(got) == digest, (name, size)
            key = f"output|{name}|{size}"
            if key in arrays:
                assert np.array_equal(got, arrays[key]), key
                seen += 1
    assert seen == 8 and len(js["cases"]) == 18


def test_profiles_and_plans_equal_the_recorded_ones(golden):
    js, _ = golden
    for name, case in js["cases"].items():
        rcfg, pcfg = config_of(case["config"], R), config_of(case["config"], PT)
        assert R.profile(rcfg).to_dict() == case["profile"] and R.plan(rcfg) == case["plan"], name
        p = PT.compute_profile(pcfg)
        assert p.to_dict() == case["profile"] and PT.compute_plan(pcfg, p).to_dict() == case["plan"], name
    plans = {n: c["plan"] for n, c in js["cases"].items()}
    assert plans["balanced0.5|grain1"]["steps"] == ["denoise", "sharpen", "colour", "detail", "grain"] and plans["balanced0.5|grain1"]["h"] == 1
    assert plans["enhanced|grain1"]["h"] == 1 and plans["enhanced|grain0"]["h"] == 4 and plans["enhanced|grain0|denoise1"]["h"] == 5
    assert plans["balanced0|grain1"]["steps"] == ["grain"] and plans["faithful|grain1"]["grain_amount"] == 0.5
    assert plans["faithful|grain0"]["steps"] == [] and plans["enhanced|grain1"]["clip_limit"] == 2.6


def test_value_types_and_factories(golden):
    js, _ = golden
    for module in (R, PT):
        cfg = module.PerceptualConfig()
        assert {**cfg.__dict__, "mode": cfg.mode.value} == js["defaults"]["config"]
        assert module.PerceptualProfile().to_dict() == js["defaults"]["profile"]
        c = module.PerceptualConfig(balance=3.0, sharpening_limit=-1.0, denoise_limit=7.0)
        assert {**c.__dict__, "mode": c.mode.value} == js["defaults"]["clamped_config"]
        assert module.PerceptualProfile(2.0, -1.0, 0.5, 9.0, -3.0).to_dict() == js["defaults"]["clamped_profile"]
        assert {m.name: m.value for m in module.PerceptualMode} == js["enums"]["PerceptualMode"]
    for b, want in js["get_perceptual_profile"].items():
        assert PT.get_perceptual_profile(float(b)).to_dict() == want, b
    with pytest.raises(ValueError) as e:
        PT.create_perceptual_tuner("vivid")
    assert str(e.value) == js["created"]["vivid"]
    assert js["quirks"]["result_gray_is_unused"] is True and js["quirks"]["restorer_calls_the_tuner"] is False


def test_factory_modes(golden, hip_lib):
    js, _ = golden
    for name in ("faithful", "balanced", "enhanced", "ENHANCED"):
        cfg = PT.create_perceptual_tuner(name).config
        assert {"mode": cfg.mode.value, "balance": cfg.balance} == js["created"][name]
    tuner = PT.create_perceptual_tuner("balanced")              # the profile follows the configuration, also after the first call
    assert "sharpen" in tuner.plan().steps
    tuner.config.balance = 0.0
    assert tuner.plan().steps == ("grain",) and tuner.get_profile().to_dict() == js["cases"]["balanced0|grain1"]["profile"]


def test_scratch_is_sized_by_the_plan(hip_lib):
    import ctypes as C
    h, w, frame = 1080, 1920, 1080 * 1920 * 3                      # a frame is a multiple of 256 bytes here

    def need(**on):
        p = PT._Params()
        for k, v in on.items():
            setattr(p, k, v)
        return int(hip_lib.fw_ptune_scratch_bytes(h, w, C.cast(C.pointer(p), C.c_void_p)))

    assert frame % 256 == 0 and int(hip_lib.fw_ptune_scratch_bytes(h, w, None)) == 81920
    assert need() == 0 and need(sharpen=1, colour=1, grain=1) == 0
    assert need(detail=1) == need(detail=1, grain=1) == 81920
    assert need(detail=1, sharpen=1) == need(detail=1, colour=1, grain=1) == 81920 + frame
    assert need(denoise_h=1) == need(denoise_h=1, detail=1, sharpen=1) > 81920 + 2 * frame


def test_adjust_settings_equals_the_recorded_dictionaries(golden):
    js, _ = golden
    assert len(js["adjust_settings"]) == 56
    for name, rec in js["adjust_settings"].items():
        rcfg, pcfg = config_of(rec["config"], R), config_of(rec["config"], PT)
        base = dict(rec["base"])
        assert R.adjust_settings(rcfg, base, rec["content_type"]) == rec["settings"], name
        assert PT.adjust_settings(pcfg, PT.compute_profile(pcfg), base, rec["content_type"]) == rec["settings"], name
        assert base == rec["base"]


def test_gauss19_table(golden):
    k = R.gauss19_table()
    assert k.tolist() == golden[0]["gauss19_table"] and int(k.sum()) == 256 and np.array_equal(k, k[::-1]) and len(k) == 19
    assert int(R.gauss19_table(carry=False).sum()) == 256 and not np.array_equal(R.gauss19_table(carry=False), k)


def test_clahe_limit_is_the_double_arithmetic():
    for h, w in ((24, 40), (37, 53), (8, 8), (2160, 3840)):
        for clip in (2.0, 2.6, 1.4, 1.0 + 0.5 * 2.0):
            assert PT.clahe_limit(clip, h, w) == R.clahe_limit(clip, h, w)
    assert R.clahe_limit(2.6, 24, 40) == 1 and R.clahe_limit(2.6, 2160, 3840) == 1316


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
def changed(a, b) -> int:
    return int(np.count_nonzero(a != b))


def test_defect_blur_table_without_the_carried_error(golden):
    x = frame(golden)
    assert changed(R.gaussian_blur_sigma3_u8(x, R.gauss19_table(carry=False)), R.gaussian_blur_sigma3_u8(x)) > 0
    bad = R.hd.add_weighted(x, 1.525, R.gaussian_blur_sigma3_u8(x, R.gauss19_table(carry=False)), -0.525)
    assert changed(bad, R.unsharp_u8(x, 1.525, -0.525)) > 0


def test_defect_single_reflection():
    """The outermost taps of the table are 0, so the blur reaches 8 pixels: a side of 8 is where one reflection stops being enough
    (-8 -> 8 -> 6), and 8 x 8 is among the GPU shapes."""
    x = R.content_frame(8, 8)
    assert changed(R.gaussian_blur_sigma3_u8(x, reflect=R.reflect_once), R.gaussian_blur_sigma3_u8(x)) > 0
    wide = R.content_frame(9, 200)
    assert changed(R.gaussian_blur_sigma3_u8(wide, reflect=R.reflect_once), R.gaussian_blur_sigma3_u8(wide)) == 0


def test_defect_addweighted_of_the_sharpen_step_contracted(golden):
    x = frame(golden)
    w_src, w_blur = R.plan(R.PerceptualConfig())["w_src"], R.plan(R.PerceptualConfig())["w_blur"]
    assert changed(R.add_weighted_fused(x, w_src, R.gaussian_blur_sigma3_u8(x), w_blur), R.unsharp_u8(x, w_src, w_blur)) > 0


def test_defect_tail_as_one_fused_multiply_add(golden):
    """The tail as ONE fused multiply-add, fma(grain, amount, result), rounds once where the definition rounds the product and then
    the sum.  The two differ only where the rounded product moves the sum across a float32 tie next to a half-integer, and that
    takes an amount whose products come close enough: none of the 65536 (result, grain) pairs differs at 0.35, 0.4 or 0.5, 584
    differ at float32(0.375) - 2^-24, the amount of BALANCED at `FMA_BALANCE` (recorded in the golden).  The frame is the test
    frame as the original and, as the result, the steps in front of the tail with every pixel whose grain has a sensitive partner
    set to it; tests/test_perceptual_gpu.py hands the same pair to `fw_ptune_grain_u8`."""
    x = frame(golden)
    cfg = R.PerceptualConfig(balance=R.FMA_BALANCE)
    pl = R.plan(cfg)
    assert pl["grain_amount"] == golden[0]["cases"]["balanced_fma|grain1"]["plan"]["grain_amount"] and pl["steps"][-1] == "grain"
    result = R.tail_sensitive_result(R.apply_plan(x, {**pl, "steps": pl["steps"][:-1]}), x, pl["grain_amount"])
    n = changed(R.grain_tail_fused(result, x, pl["grain_amount"]), R.grain_tail_u8(result, x, pl["grain_amount"]))
    print("bytes changed by a fused tail:", n)
    assert n > 0


def test_where_a_fused_tail_shows():
    assert len(R.fused_tail_pairs(R.plan(R.PerceptualConfig(balance=R.FMA_BALANCE))["grain_amount"])) == 584
    for amount in (0.35, 0.4, 0.5):                              # the recorded round balances: a contracted tail would go unseen there
        assert len(R.fused_tail_pairs(float(np.float32(amount)))) == 0


def test_defect_clahe_limit_two(golden):
    x = frame(golden, "37x53")
    pl = R.plan(R.PerceptualConfig(mode=R.PerceptualMode.ENHANCED))
    assert pl["clip_limit"] == 2.6
    assert R.clahe_limit(2.6, 2160, 3840) != R.clahe_limit(2.0, 2160, 3840)
    big = R.content_frame(160, 200)                              # tiles of 20 x 25: limit 5 against 3
    assert R.clahe_limit(2.6, 160, 200) == 5 and R.clahe_limit(2.0, 160, 200) == 3
    assert changed(R.detail_u8(big, 2.0), R.detail_u8(big, 2.6)) > 0
    assert R.clahe_limit(2.6, *x.shape[:2]) == R.clahe_limit(2.0, *x.shape[:2]) == 1      # on the small frames the limit is 1 either way


def test_defect_l_blended_instead_of_replaced(golden):
    x = frame(golden)
    assert changed(R.hd.local_contrast_u8(x), R.detail_u8(x, 2.0)) > 0


def test_defect_grain_from_the_result(golden):
    x = frame(golden)
    cfg = R.PerceptualConfig()
    pl = R.plan(cfg)
    result = R.apply_plan(x, {**pl, "steps": [s for s in pl["steps"] if s != "grain"]})
    assert changed(R.grain_tail_u8(result, result, pl["grain_amount"]), R.apply_to_frame(x, cfg)) > 0
    g = R.grain_u8(x)
    assert (g == 0).any() and (g > 0).any()                      # the blur exceeds the gray somewhere: the subtraction saturates


def test_defect_round_for_h(golden):
    x = frame(golden)
    cfg = R.PerceptualConfig(mode=R.PerceptualMode.ENHANCED, preserve_grain=False)
    assert R.plan(cfg)["h"] == 4 and R.plan(cfg, to_int=round)["h"] == 5
    assert changed(R.apply_plan(x, R.plan(cfg, to_int=round)), R.apply_plan(x, R.plan(cfg))) > 0
    assert R.plan(R.PerceptualConfig())["h"] == 1 and 0.4 * (1 - 0.7) * 10 == 1.2000000000000002


def test_content_frame_has_what_the_defects_need(golden):
    x = frame(golden)
    hsv = R.hd.bgr2hsv(x)
    assert (hsv[:, :, 1] == 0).any() and (hsv[:, :, 1] == 255).any()                      # gray and saturated pixels
    sharp = R.unsharp_u8(x, 1.525, -0.525)
    assert (sharp == 0).any() and (sharp == 255).any()
    lab_l = np.ascontiguousarray(R.fl.bgr_to_lab_gamma(x)[:, :, 0])
    assert changed(R.hd.clahe(lab_l, 2.0), lab_l) > 0
