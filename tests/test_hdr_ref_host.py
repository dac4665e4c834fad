"""CPU: tests/hdr_ref.py and the host side of framewright_amd.hdr against what tools/gen_hdr_golden.py recorded from the reference's own
`processors/hdr_conversion.py` (tests/golden/hdr_reference.json and .npz).  The generator asserted the equality with the reference
when it ran; this holds the restatement, fed with the recorded tables, to that record - exactly, for every config in which a quantising
step is on and the curve is rational - and works the cv2 pieces by hand.  The paths that are not bit-pinned (the float path, MOBIUS)
are held to the bounds of DESIGN K20, with numpy's own float32 result as the subject: the rule the device is held to in
tests/test_hdr_gpu.py is no looser than the reference's own noise."""
import hashlib
import json
import warnings
from pathlib import Path

import numpy as np
import pytest

import hdr_ref as R
from framewright_amd import hdr as H

GOLD = Path(__file__).resolve().parent / "golden"
f32 = np.float32


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLD / "hdr_reference.json").read_text())


@pytest.fixture(scope="module")
def npz():
    with np.load(GOLD / "hdr_reference.npz") as z:
        return {k: z[k] for k in z.files}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recorded_tables(gold, npz, fields) -> dict:
    return {"gamma8": npz["gamma8"], "gamma16": npz["gamma16"], "clip8": gold["clip8"], "clip16": gold["clip16"],
            "tail": npz[f"tail|{fields['target_format']}|{fields['peak_brightness']}"]}


def test_the_record_covers_what_it_should(gold):
    cases = gold["cases"].values()
    assert {c["config"]["tone_mapping"] for c in cases} == {"reinhard", "aces", "hable", "mobius"}
    assert {c["config"]["target_format"] for c in cases} == {"hdr10", "hdr10plus", "dolby_vision", "hlg"}
    assert {c["config"]["color_space"] for c in cases} == {"bt2020", "rec709", "p3"}
    assert {c["config"]["peak_brightness"] for c in cases} >= {400, 1000, 4000}
    assert {c["input"][:3] for c in cases} == {"u8_", "u16"}
    switches = {(c["config"]["enable_local_contrast"], c["config"]["saturation_boost"] != 1.0, c["config"]["highlight_recovery"]) for c in cases}
    assert len(switches) == 8
    exact = [c for c in cases if c["exact"]]
    assert len(exact) >= 100 and all(c["differing"] == 0 for c in exact)
    assert (gold["clip8"], gold["clip16"]) == (250, 64225)


def test_every_exact_case_equals_the_reference_output(gold, npz):
    for key, rec in gold["cases"].items():
        config = H.HDRConfig(**rec["config"])
        frame = npz[f"input|{rec['input']}"]
        tables = recorded_tables(gold, npz, rec["config"])
        if rec["config"]["tone_mapping"] in R.RATIONAL_CURVES:
            assert sha(R.tone_mapped_plane(frame, config, tables)) == rec["tone_sha256"], key           # float32 bit patterns
        if rec["exact"]:
            got = R.convert_frame(frame, config, tables)
            assert got.dtype == np.uint16 and sha(got) == rec["sha256"], key
    for name in [k for k in npz if k.startswith("output|")]:
        key = name.split("|", 1)[1]
        rec = gold["cases"][key]
        if rec["exact"]:
            assert np.array_equal(R.convert_frame(npz[f"input|{rec['input']}"], H.HDRConfig(**rec["config"]), recorded_tables(gold, npz, rec["config"])), npz[name])


def test_requantisation_is_the_identity_for_all_256_codes():
    k = np.arange(256).astype(np.uint8)
    assert np.array_equal((np.clip(k.astype(f32) / 255.0, 0, 1) * 255).astype(np.uint8), k)
    assert np.array_equal(R.quantise8(k.astype(f32) / 255.0), k)


@pytest.mark.parametrize("fmt,peak", [("hdr10", 400), ("hdr10", 1000), ("hdr10", 4000), ("hlg", 1000), ("dolby_vision", 10000)])
def test_the_tail_table_is_the_transfer_function_of_its_512_values(gold, npz, fmt, peak):
    config = H.HDRConfig(target_format=fmt, peak_brightness=peak)
    x8 = np.arange(256).astype(np.uint8).astype(f32) / 255.0
    values = np.stack([x8, x8 * 0.95])
    assert values.dtype == np.float32
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # the HLG log of negative numbers must not become an error
        live = R.build_tables(config)["tail"]
        assert np.array_equal(live, R.transfer_and_quantise(values, config))
        assert np.array_equal(live, H.host_tables(config)["tail"])      # the product's own builder, the same expressions
    # the same values through the reference's _apply_pq_transfer / _apply_hlg_transfer, as the generator recorded them on its CPU: a
    # last-bit difference of another CPU's pow moves trunc's argument by less than one code (epsilon_codes), so by one code at most
    recorded = npz[f"tail|{fmt}|{peak}"]
    assert np.abs(live.astype(np.int64) - recorded.astype(np.int64)).max() <= 1
    assert R.float_rule_violations(recorded, values, config) == 0 and R.float_rule_violations(live, values, config) == 0
    assert live[0, 255] >= live[1, 255] and (np.diff(live.astype(np.int64), axis=1) >= 0).all()


def test_host_tables_and_params_of_the_product():
    t = H.host_tables(H.HDRConfig())
    r = R.build_tables(H.HDRConfig())
    assert np.array_equal(t["gamma8"].view(np.uint32), r["gamma8"].view(np.uint32)) and np.array_equal(t["gamma16"].view(np.uint32), r["gamma16"].view(np.uint32))
    assert (t["clip8"], t["clip16"]) == (r["clip8"], r["clip16"]) == (250, 64225)
    assert np.array_equal(t["hsv_div"][:256], R.SDIV) and np.array_equal(t["hsv_div"][256:], R.HDIV)
    p = H.make_params(H.HDRConfig(color_space="p3", saturation_boost=1.005, tone_mapping="hable"), 250)
    assert (p.use_matrix, p.curve, p.transfer, p.local_contrast, p.saturation, p.recover, p.clip_code) == (1, 2, 0, 1, 0, 1, 250)
    assert np.array_equal(np.array(p.matrix[:], f32), R.M_709_2020.ravel())
    assert f32(p.curve_k[7]) == f32(1.0 / R._hable(10.0)) and f32(p.curve_k[6]) == f32(0.02 / 0.30)
    assert H.make_params(H.HDRConfig(target_format="hlg", color_space="rec709"), 250).transfer == 1


# ---- cv2, restated: hand-worked cases ---------------------------------------------------------------------------------------------------
def test_clahe_of_a_constant_plane_is_the_clipped_uniform_lut():
    # 16 x 24: tiles 2 x 3, area 6, limit max(int(2 * 6 / 256), 1) = 1.  One bin holds 6: 5 are clipped, none per bin, the 5 left go to
    # bins 0, 51, 102, 153, 204 (step 256 // 5).  The cumulative sum at 100 is 2 (bins 0, 51) + 1 (the bin itself): round(3 * 255 / 6) = 128
    plane = np.full((16, 24), 100, np.uint8)
    assert np.array_equal(R.clahe(plane), np.full((16, 24), 128, np.uint8))
    # value 0: the bin itself and the redistributed count at 0: round(2 * 42.5) = 85; value 255: everything, 255
    assert R.clahe(np.zeros((16, 24), np.uint8))[0, 0] == 85 and R.clahe(np.full((16, 24), 255, np.uint8))[5, 7] == 255


def test_clahe_one_pixel_tiles_and_padding_geometry():
    assert R.clahe_geometry(8, 8) == (8, 8, 1, 1) and R.clahe_geometry(37, 53) == (40, 56, 5, 7)
    assert R.clahe_geometry(40, 53) == (48, 56, 6, 7) and R.clahe_geometry(72, 136) == (72, 136, 9, 17)
    # 8 x 8: every tile is one pixel, limit 1, nothing clipped: lut[i] = 255 for i >= v, else 0.  The pixel centres are the tile
    # centres (x * 1 - 0.5 + ... : tx1 = x - 1 with weight 0.5 each side), so the result mixes the neighbours' step functions
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 256, (8, 8)).astype(np.uint8)
    luts = R.clahe_luts(plane)
    for ty in range(8):
        for tx in range(8):
            assert np.array_equal(luts[ty, tx], np.where(np.arange(256) >= plane[ty, tx], 255, 0))
    want = np.empty((8, 8), np.uint8)
    for y in range(8):
        for x in range(8):
            v = int(plane[y, x])
            txf, tyf = f32(x) * f32(1 / 1) - f32(0.5), f32(y) * f32(1 / 1) - f32(0.5)
            tx1, ty1 = int(np.floor(txf)), int(np.floor(tyf))
            xa, ya = f32(txf - tx1), f32(tyf - ty1)
            cx = lambda t: min(max(t, 0), 7)                                        # noqa: E731
            l = lambda ty, tx: f32(luts[cx(ty), cx(tx), v])                         # noqa: E731
            top = l(ty1, tx1) * (f32(1) - xa) + l(ty1, tx1 + 1) * xa
            bot = l(ty1 + 1, tx1) * (f32(1) - xa) + l(ty1 + 1, tx1 + 1) * xa
            want[y, x] = min(max(int(np.rint(top * (f32(1) - ya) + bot * ya)), 0), 255)
    assert np.array_equal(R.clahe(plane), want)


def test_clahe_one_tile_worked_by_the_formulas():
    # a 64 x 64 plane: tiles 8 x 8, area 64, limit max(int(128 / 256), 1) = 1: every occupied bin is clipped to 1
    rng = np.random.default_rng(4)
    plane = rng.integers(90, 110, (64, 64)).astype(np.uint8)
    tile = plane[8:16, 16:24]
    hist = np.bincount(tile.ravel(), minlength=256)
    excess = int(np.maximum(hist - 1, 0).sum())
    hist = np.minimum(hist, 1) + excess // 256
    for i in list(range(0, 256, max(256 // (excess % 256), 1)))[:excess % 256]:
        hist[i] += 1
    lut = np.clip(np.rint(np.cumsum(hist).astype(f32) * f32(255.0 / 64)), 0, 255).astype(np.uint8)
    assert hist.sum() == 64 and np.array_equal(R.clahe_luts(plane)[1, 2], lut)
    ramp = np.tile(np.arange(64, dtype=np.uint8) * 4, (64, 1))                      # a smooth ramp: eight pixels a value, all clipped
    out = R.clahe(ramp)
    # every tile holds 8 values 8 times: clipped to 1 each, the 56 cut off go to bins 0, 4, 8 ... (step 256 // 56), so the tile's first
    # value k maps to round((1 + the redistributed bins up to k) * 255 / 64); in the first tile k = 0: round(2 * 3.984375) = 8
    assert out.shape == ramp.shape and out[0, 0] == 8 and out[0, 63] == 255


def test_add_weighted_rounds_half_to_even():
    a = np.array([0, 1, 2, 3, 255, 254, 10], np.uint8)
    b = np.array([1, 2, 3, 6, 255, 255, 10], np.uint8)
    assert R.add_weighted(a, 0.5, b, 0.5, 0).tolist() == [0, 2, 2, 4, 255, 254, 10]          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 4.5 -> 4, 254.5 -> 254


def test_hsv_of_the_pure_hues_and_of_grays():
    hues = {(0, 0, 255): 0, (0, 255, 255): 30, (0, 255, 0): 60, (255, 255, 0): 90, (255, 0, 0): 120, (255, 0, 255): 150}       # BGR -> h
    for bgr, h in hues.items():
        px = np.array([[bgr]], np.uint8)
        assert R.bgr2hsv(px)[0, 0].tolist() == [h, 255, 255]
        assert R.hsv2bgr(np.array([[[h, 255, 255]]], np.uint8))[0, 0].tolist() == list(bgr)
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    hsv = R.bgr2hsv(gray)
    assert (hsv[..., 0] == 0).all() and (hsv[..., 1] == 0).all() and np.array_equal(hsv[..., 2], gray[..., 0])
    assert np.array_equal(R.hsv2bgr(hsv), gray)
    assert np.array_equal(R.adjust_saturation_u8(gray, 1.5), gray)                  # s == 0 stays 0
    # worked: BGR (10, 200, 100): v 200, diff 190, s = (190 * sdiv[200] + 2048) >> 12 with sdiv[200] = round(1044480 / 200) = 5222
    assert R.SDIV[200] == 5222 and R.HDIV[190] == round(122880 / 190) == 647
    s = (190 * 5222 + 2048) >> 12
    h = ((10 - 100 + 2 * 190) * 647 + 2048) >> 12
    assert R.bgr2hsv(np.array([[[10, 200, 100]]], np.uint8))[0, 0].tolist() == [h, s, 200] == [46, 242, 200]
    # a negative hue wraps: BGR (100, 10, 200): v == r, h = (10 - 100) * hdiv[190] -> -14 -> 166
    assert R.bgr2hsv(np.array([[[100, 10, 200]]], np.uint8))[0, 0, 0] == 180 + ((-90 * 647 + 2048) >> 12) == 166
    # the boost truncates: s 242 * 1.1 = 266.2 -> 255; s 100 * 1.1 = 110.000001 -> 110
    assert int(np.clip(f32(242) * f32(1.1), 0, 255)) == 255 and int(f32(100) * f32(1.1)) == 110


def test_the_matrix_is_one_product_and_two_fused_multiply_adds():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b, c = (rng.random(2000).astype(f32) for _ in range(3))
    c[:500] = -(a[:500].astype(np.float64) * b[:500]).astype(f32)                   # cancellation: the low bits of the product decide
    got = R.fma32(a, b, c)

    def exact(x, y, z):                                                             # the exact sum, rounded once to float32
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = f32(float(v))
        cands = [np.nextafter(lo, f32(-np.inf)), lo, np.nextafter(lo, f32(np.inf))]
        best = min(cands, key=lambda t: (abs(Fraction(float(t)) - v), int(t.view(np.uint32)) & 1))
        return best

    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the value types, as recorded from the reference ---------------------------------------------------------------------------------------
def test_config_defaults_validation_and_coercion_are_the_references(gold):
    cfg = H.HDRConfig()
    assert {k: (v.value if hasattr(v, "value") else v) for k, v in cfg.__dict__.items()} == gold["defaults"]
    for bad, message in gold["rejected"]:
        with pytest.raises(ValueError) as e:
            H.HDRConfig(**bad)
        assert str(e.value) == message, bad
    c = H.HDRConfig(target_format="HLG", tone_mapping="Mobius", color_space="REC709")
    assert (c.target_format, c.tone_mapping, c.color_space) == (H.HDRFormat.HLG, H.ToneMapping.MOBIUS, H.ColorSpace.REC709)
    for cls in (H.HDRFormat, H.ToneMapping, H.ColorSpace):
        assert {m.name: m.value for m in cls} == gold["enums"][cls.__name__]
    assert {k: (str(v) if isinstance(v, Path) else v) for k, v in H.HDRConversionResult().__dict__.items()} == gold["result_defaults"]
    import framewright_amd
    assert framewright_amd.DeviceHDRConverter is H.DeviceHDRConverter and framewright_amd.create_hdr_converter is H.create_hdr_converter


# ---- the paths that are not bit-pinned: numpy's own float32 result meets the device's rule ------------------------------------------
@pytest.mark.parametrize("fmt,peak", [("hdr10", 400), ("hdr10", 1000), ("hdr10", 10000), ("hlg", 1000)])
def test_numpy_float32_transfer_meets_the_float_path_rule(fmt, peak):
    config = H.HDRConfig(target_format=fmt, peak_brightness=peak, enable_local_contrast=False, saturation_boost=1.0)
    rng = np.random.default_rng(6)
    plane = np.concatenate([rng.random(200000).astype(f32), np.linspace(0, 1, 70000, dtype=f32), (np.arange(256) / 255.0).astype(f32),
                            f32([0.0, 1.0, 1.0 / 12.0, np.nextafter(f32(1.0 / 12.0), f32(1))])])
    got = R.transfer_and_quantise(plane, config)
    assert R.float_rule_violations(got, plane, config) == 0
    v = R.transfer64(plane, config)
    print(f"{fmt} {peak}: numpy float32 differs from trunc(float64) in {(got != np.floor(v)).sum()} of {plane.size}; "
          f"largest epsilon {R.epsilon_codes(v, config).max():.3f} codes")
    spoiled = got.copy()
    spoiled[::1000] += 2                                                            # the rule is not empty
    assert R.float_rule_violations(spoiled, plane, config) >= 200


@pytest.mark.parametrize("peak", [400, 1000, 4000])
def test_numpy_exp_meets_the_mobius_bound(gold, npz, peak):
    config = H.HDRConfig(tone_mapping="mobius", peak_brightness=peak)
    for name in ("u8_37x53", "u16_24x40"):
        frame = npz[f"input|{name}"]
        lin = R.linear_plane(frame, config)
        d = R.ulp_distance(R.tone_map(lin, config), R.mobius_plane64(lin, config))
        print(f"mobius {peak} {name}: {d.max():.2f} ulp")
        assert d.max() <= R.MOBIUS_ULPS
    assert gold["inexact_summary"]["cases"] >= 40                                    # how many recorded pixels differed from the reference's run
    assert gold["inexact_summary"]["samples_differing"] == sum(c["differing"] for c in gold["cases"].values() if not c["exact"])
