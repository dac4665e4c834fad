"""CPU: the restatement in tests/color_lut_ref.py and the builders of framewright_amd/color_grade.py against what was recorded from
the reference's own integration/lut.py (tests/golden/color_lut_reference.*, tools/gen_color_lut_golden.py), byte for byte; and the
wrong variants of the restatement REJECTED on the recorded hard colours, which is what gives the GPU comparison its teeth."""
import json
from pathlib import Path

import numpy as np
import pytest

import color_lut_ref as R
from framewright_amd import color_grade as G

GOLD = Path(__file__).resolve().parent / "golden"
SEASONS = ["winter", "spring", "summer", "autumn"]
STRENGTHS = [0.0, 0.3, 0.7, 1.0]


@pytest.fixture(scope="module")
def gold():
    js = json.loads((GOLD / "color_lut_reference.json").read_text())
    with np.load(GOLD / "color_lut_reference.npz") as z:
        arrays = {k: z[k] for k in z.files}
    return js, arrays


def golden_luts():
    return {"autumn_0.7_33": G.create_seasonal_lut("autumn", 0.7, 33), "winter_1.0_17": G.create_seasonal_lut("winter", 1.0, 17)}


def test_builders_equal_the_reference_tables(gold):
    js, arrays = gold
    for s in SEASONS:
        for k in STRENGTHS:
            assert R.sha256(G.create_seasonal_lut(s, k, 33).table_f32()) == js["table_sha256"][f"seasonal/{s}/{k}"], (s, k)
            np.testing.assert_array_equal(G.create_seasonal_lut(s, k, 5).table_f32(), arrays[f"table5/seasonal/{s}/{k}"])
    for f in G.FILM_STOCKS:
        assert R.sha256(G.create_film_emulation_lut(f, 33).table_f32()) == js["table_sha256"][f"film/{f}"], f
        np.testing.assert_array_equal(G.create_film_emulation_lut(f, 5).table_f32(), arrays[f"table5/film/{f}"])
    assert R.sha256(G.create_identity_lut(33).table_f32()) == js["table_sha256"]["identity"]
    np.testing.assert_array_equal(G.create_contrast_lut(1.2, 33).data_1d, np.asarray(js["contrast_1d"]))
    comb = G.combine_luts([G.create_seasonal_lut("summer", 0.5, 9), G.create_contrast_lut(1.2, 33)], 5)
    np.testing.assert_array_equal(comb.table_f32(), arrays["table5/combined_summer9_contrast"])
    with pytest.raises(ValueError):
        G.create_seasonal_lut("monsoon")


@pytest.mark.parametrize("size", R.TABLE_SIZES)
def test_restatement_equals_the_reference_on_the_test_images(gold, size):
    js, arrays = gold
    tab = G.create_seasonal_lut("autumn", 0.7, size).table_f32()
    for h, w in R.IMAGE_SIZES:
        for dt in (np.uint8, np.uint16):
            out = R.apply_lut3d(R.test_image(h, w, dt)[0], tab)
            name = f"{size}/{h}x{w}/{np.dtype(dt).name}"
            assert R.sha256(out) == js["image_sha256"][name], name
            if f"out/{name}" in arrays:
                np.testing.assert_array_equal(out, arrays[f"out/{name}"])


def test_restatement_full_range_u16_and_identity(gold):
    js, _ = gold
    full = R.full_range_u16()
    for c in range(3):
        assert np.array_equal(np.sort(full[..., c].reshape(-1)), np.arange(65536))
    for key, lut in golden_luts().items():
        assert R.sha256(R.apply_lut3d(full, lut.table_f32())) == js["full_range_u16_sha256"][key]
    ident = G.create_identity_lut(33).table_f32()
    for dt in (np.uint8, np.uint16):
        img = R.test_image(64, 64, dt)[0]
        out = R.apply_lut3d(img, ident)
        rec = js["identity"][np.dtype(dt).name]
        assert R.sha256(out) == rec["sha256"]
        assert bool(np.array_equal(out, img)) == rec["returns_input"]
    assert js["identity"]["uint8"]["returns_input"]


def _hard(js, key, dtype, variant):
    rec = js["hard"][key][dtype][variant]
    return np.asarray(rec["colours"], dtype).reshape(-1, 1, 3), np.asarray(rec["out"], dtype).reshape(-1, 1, 3)


@pytest.mark.parametrize("key", ["autumn_0.7_33", "winter_1.0_17"])
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_hard_colours_accept_the_restatement_and_reject_the_variants(gold, key, dtype):
    js, _ = gold
    tab = golden_luts()[key].table_f32()
    for variant in ("lerp32", "reciprocal"):
        colours, want = _hard(js, key, dtype, variant)
        assert len(colours) >= 10, "too few hard colours recorded to reject anything"
        np.testing.assert_array_equal(R.apply_lut3d(colours, tab), want)
        wrong = R.apply_lut3d(colours, tab, **{variant: True})
        assert (wrong != want).any(-1).all(), f"the {variant} variant passes on its own hard colours"


def test_fused_variant_on_whatever_the_cube_search_found(gold):
    """In float64 a contracted lerp moves a result by 2^-53 of itself; the search over both cubes records the colours it flips."""
    js, _ = gold
    for key, lut in golden_luts().items():
        colours, want = _hard(js, key, "uint8", "fused")
        assert len(colours) == min(200, js["variant_changes_u8"][key]["fused"])
        if len(colours):
            tab = lut.table_f32()
            np.testing.assert_array_equal(R.apply_lut3d(colours, tab), want)
            assert (R.apply_lut3d(colours, tab, fused=True) != want).any(-1).all()


def test_whole_cube_digest_size_17(gold):
    js, _ = gold
    tab = golden_luts()["winter_1.0_17"].table_f32()
    assert R.cube_digest(lambda img: R.apply_lut3d(img, tab), strip=512) == js["cube_sha256"]["winter_1.0_17"]


def test_byte_tables_equal_the_reference_1d_path(gold):
    js, _ = gold
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    tabs = G.byte_tables_1d(G.create_contrast_lut(1.2, 33))
    np.testing.assert_array_equal(R.apply_table3(ramp, tabs)[:, 0, :], np.asarray(js["ramp_1d_contrast"], np.uint8))
    odd = js["odd_1d"]
    lut = G.LUT(lut_type=G.LUTType.LUT_1D, size=len(odd["data"]), domain_min=tuple(odd["domain_min"]), domain_max=tuple(odd["domain_max"]),
                data_1d=np.asarray(odd["data"], np.float64))
    img = np.asarray(odd["image"], np.uint8)[:, None, :]
    np.testing.assert_array_equal(R.apply_table3(img, G.byte_tables_1d(lut, bgr=True))[:, 0, :], np.asarray(odd["out"], np.uint8))
    # an RGB frame is the BGR frame with its channels reversed, in and out
    rgb = R.apply_table3(np.ascontiguousarray(img[..., ::-1]), G.byte_tables_1d(lut, bgr=False))
    np.testing.assert_array_equal(rgb[..., ::-1][:, 0, :], np.asarray(odd["out"], np.uint8))


def test_cube_files(tmp_path):
    for lut in (G.create_seasonal_lut("autumn", 0.7, 5), G.create_contrast_lut(1.2, 9)):
        lut.comments = ["written by a test"]
        G.write_cube(lut, tmp_path / "a.cube")
        back = G.read_cube(tmp_path / "a.cube")
        assert back.lut_type == lut.lut_type and back.size == lut.size and back.comments == lut.comments
        assert back.title == (lut.title or lut.name)
        a, b = (lut.data_1d, back.data_1d) if lut.lut_type == G.LUTType.LUT_1D else (lut.data_3d, back.data_3d)
        assert np.abs(a - b).max() <= 0.5e-10          # ten decimals
    (tmp_path / "hand.cube").write_text('# graded by hand\nTITLE "Hand made"\n\nDOMAIN_MIN 0.0 0.0 0.0\nDOMAIN_MAX 1.0 2.0 1.0\n'
                                        "LUT_3D_SIZE 2\n# red moves fastest\n0 0 0\n1 0 0\n0 1 0\n1 1 0\n0 0 1\n1 0 1\n0 1 1\n0.5 0.25 0.125\n")
    lut = G.read_cube(tmp_path / "hand.cube")
    assert lut.title == "Hand made" and lut.comments == ["graded by hand", "red moves fastest"]
    assert lut.domain_max == (1.0, 2.0, 1.0) and lut.size == 2 and lut.lut_type == G.LUTType.LUT_3D
    np.testing.assert_array_equal(lut.data_3d[1, 0, 0], [1, 0, 0])
    np.testing.assert_array_equal(lut.data_3d[0, 0, 1], [0, 0, 1])
    np.testing.assert_array_equal(lut.data_3d[1, 1, 1], [0.5, 0.25, 0.125])
    (tmp_path / "one.cube").write_text("LUT_1D_SIZE 3\n0 0 0\n0.5 0.4 0.3\n1 1 1\n")
    one = G.read_cube(tmp_path / "one.cube")
    assert one.lut_type == G.LUTType.LUT_1D and one.data_1d.shape == (3, 3)


def test_non_finite_tables_are_refused():
    lut = G.create_identity_lut(5)
    lut.data_3d[1, 2, 3, 0] = np.nan
    with pytest.raises(ValueError):
        G.check_finite(lut)
    one = G.create_contrast_lut(1.2, 9)
    one.data_1d[4, 1] = np.inf
    with pytest.raises(ValueError):
        G.byte_tables_1d(one)
    with pytest.raises(ValueError):
        G.DeviceColorGrader(lut)          # refused on the host, in front of any use of a device


def test_package_exports():
    import framewright_amd as F
    for name in ("LUT", "LUTType", "DeviceColorGrader", "create_identity_lut", "create_seasonal_lut", "create_film_emulation_lut",
                 "create_contrast_lut", "combine_luts", "read_cube", "write_cube"):
        assert hasattr(F, name), name
