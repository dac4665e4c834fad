"""CPU: tests/qp_artifact_ref.py, the numpy contract of csrc/qp_artifacts.hip, against the record that tools/gen_qp_artifact_golden.py
made from the reference's own `processors/qp_artifact_removal.py` (tests/golden/qp_artifact_reference.*), against hand-worked pieces,
and the host half of `framewright_amd.qp_artifacts` (value types, QP detection, the directory driver) against the same record."""
import hashlib
import json
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

import qp_artifact_ref as R
from framewright_amd import qp_artifacts as Q

QPS, MULTIPLIERS, BLOCK_SIZES = (10, 18, 28, 34, 40, 51), (0.5, 1.0), (4, 8, 16, 32)
SHAPES = {"f24x40": (24, 40, 1), "f19x21": (19, 21, 2), "f3x5": (3, 5, 3), "f1x1": (1, 1, 4), "f33x70": (33, 70, 5), "f96x128": (96, 128, 6)}


@pytest.fixture(scope="module")
def golden(golden_dir):
    js = json.loads((golden_dir / "qp_artifact_reference.json").read_text())
    return js, np.load(golden_dir / "qp_artifact_reference.npz")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Cfg:
    def __init__(self, rec):
        self.strength_multiplier, self.block_size, self.artifact_types = rec["multiplier"], rec["block_size"], rec["types"]


def recorded_noise(rec, shape):
    """The plane the reference drew: np.random.normal after the recorded seed (numpy's legacy generator, whose stream is frozen)."""
    np.random.seed(rec["noise_seed"])
    return np.random.normal(0, 1 + np.float64(rec["strength"]) * 2, shape).astype(np.float32)


# ---- the record --------------------------------------------------------------------------------------------------------------------
def test_every_recorded_case_equals_the_restatement(golden):
    js, npz = golden
    assert js["strength_type"] == "numpy.float64" and len(js["cases"]) >= 90
    for key, rec in js["cases"].items():
        frame = R.content_frame(*SHAPES[rec["input"]])
        assert sha(frame) == rec["input_sha256"], key
        if f"input|{rec['input']}" in npz.files:
            assert np.array_equal(npz[f"input|{rec['input']}"], frame), key
        strength = R.strength_for_qp(rec["qp"], rec["multiplier"])
        assert type(strength) is np.float64 and float(strength) == rec["strength"], key
        noise = recorded_noise(rec, frame.shape)
        got = R.process_frame(frame, rec["qp"], Cfg(rec), noise)
        assert sha(got) == rec["sha256"], key
        if f"output|{key}" in npz.files:
            assert np.array_equal(npz[f"output|{key}"], got) and np.array_equal(npz[f"noise|{key}"], noise), key
        if rec["input"] != "f96x128":
            assert sha(R.remove_blocking(frame, strength, rec["block_size"])) == rec["steps"]["blocking"], key
            assert sha(R.remove_ringing(frame, strength)) == rec["steps"]["ringing"], key
            assert sha(R.remove_banding(frame, strength, noise)) == rec["steps"]["banding"], key


def test_the_record_covers_the_grid(golden):
    cases = list(golden[0]["cases"].values())
    assert {c["qp"] for c in cases} >= set(QPS) and {c["multiplier"] for c in cases} == set(MULTIPLIERS)
    for qp in QPS:
        for m in MULTIPLIERS:
            for t in (["all"], ["blocking"], ["ringing"], ["banding"]):
                assert any(c["qp"] == qp and c["multiplier"] == m and c["types"] == t for c in cases), (qp, m, t)
    for b in BLOCK_SIZES:
        assert any(c["block_size"] == b and c["types"] == ["all"] for c in cases) and any(c["block_size"] == b and c["types"] == ["blocking"] for c in cases)
    assert len(golden[1].files) >= 12 and golden[0]["numpy"]
    mosquito = [c for c in cases if c["types"] == ["mosquito"]]
    assert mosquito and all(c["sha256"] == c["input_sha256"] for c in mosquito)        # nothing to do: the frame as it is


def test_the_npz_is_no_larger_than_the_other_archives(golden_dir):
    size = (golden_dir / "qp_artifact_reference.npz").stat().st_size
    assert size <= max(p.stat().st_size for p in golden_dir.glob("*.npz") if p.name != "qp_artifact_reference.npz")


# ---- hand-worked pieces --------------------------------------------------------------------------------------------------------------
def test_bilateral_of_a_constant_frame_is_the_frame():
    for shape, d in (((7, 9, 3), 15), ((3, 5, 3), 15), ((1, 1, 3), 6), ((12, 4, 3), 8)):
        f = np.empty(shape, np.uint8)
        f[:] = (17, 200, 93)
        assert np.array_equal(R.bilateral_u8c3(f, d, 37.0, 37.0), f)


def test_bilateral_with_a_huge_sigma_color_is_the_circular_space_kernel():
    f = R.content_frame(20, 26, 7)
    for d, sigma_space in ((7, 3.0), (11, 40.0), (15, 100.0)):
        r = d // 2
        color, space = R.bilateral_tables(d, 1e30, sigma_space)
        assert np.all(color == 1.0) and space[r, r] == 1.0
        i = np.arange(-r, r + 1)
        inside = i[:, None] ** 2 + i[None, :] ** 2 <= r * r
        assert np.array_equal(space != 0, inside) and inside.sum() == {3: 29, 5: 81, 7: 149}[r]
        k = space.astype(np.float64)
        k /= k.sum()
        p = R.pad101(f, r).astype(np.float64)
        want = sum(k[a, b] * p[a:a + 20, b:b + 26] for a in range(2 * r + 1) for b in range(2 * r + 1))
        got = R.bilateral_u8c3(f, d, 1e30, sigma_space)
        # float32 sums of at most 149 terms against float64: half an LSB off a tie at the most
        assert np.abs(got - want).max() <= 0.5 + 1e-3


def test_gaussian5_on_an_impulse_gives_the_25_integers():
    f = np.zeros((9, 9, 3), np.uint8)
    f[4, 4] = (255, 128, 1)
    k = np.array([1, 4, 6, 4, 1])
    got = R.gaussian5_u8(f)
    for c, v in enumerate((255, 128, 1)):
        assert np.array_equal(got[2:7, 2:7, c], (np.outer(k, k) * v + 128) >> 8)
    got[2:7, 2:7] = 0
    assert not got.any()
    assert np.array_equal(R.gaussian5_u8(np.full((1, 1, 3), 77, np.uint8)), np.full((1, 1, 3), 77, np.uint8))
    ramp = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(3, 5, 3) * 5
    p = np.pad(ramp.astype(int), ((2, 2), (2, 2), (0, 0)), mode="reflect")
    want = sum(k[a] * k[b] * p[a:a + 3, b:b + 5] for a in range(5) for b in range(5))
    assert np.array_equal(R.gaussian5_u8(ramp), ((want + 128) >> 8).astype(np.uint8))


def test_boundary_mask_of_19x21_with_block_8_column_by_column():
    m = R.boundary_mask(19, 21, 8)
    rows_on = {0, 1, 7, 8, 9, 15, 16, 17}                 # around 0, 8, 16; row 18 is not next to a multiple of 8 below 19
    cols_on = {0, 1, 7, 8, 9, 15, 16, 17}                 # around 0, 8, 16; column 18 .. 20 are free
    for x in range(21):
        for y in range(19):
            assert m[y, x] == float(y in rows_on or x in cols_on), (y, x)
    m = R.boundary_mask(24, 8, 8)                         # no boundary at 24: row 23 stays free
    assert m[23, 4] == 0 and m[22, 4] == 0 and m[17, 4] == 1
    assert R.boundary_mask(3, 5, 4)[:, 2].tolist() == [1, 1, 0] and R.boundary_mask(3, 5, 4)[2].tolist() == [1, 1, 0, 1, 1]
    # the blend: mask 0 keeps the filtered byte, mask 1 is the float64 expression, truncated
    a, b = np.full((1, 2, 3), 200, np.uint8), np.full((1, 2, 3), 101, np.uint8)
    got = R.boundary_blend(a, b, np.array([[0.0, 1.0]], np.float32), np.float64(0.3))
    assert got[0, 0, 0] == 200 and got[0, 1, 0] == int(200 * (1 - 0.3 * 0.5) + 101 * 0.3 * 0.5)


def test_ring_region_and_edges_do_not_meet():
    f = R.content_frame(33, 70, 5)
    ring, edges = R.ring_region(f)
    assert edges.any() and ring.any() and set(np.unique(ring)) <= {0, 255} and not ((ring > 0) & (edges > 0)).any()
    flat = np.full((9, 9, 3), 50, np.uint8)
    assert np.array_equal(R.remove_ringing(flat, np.float64(1.0)), flat)


def test_a_frame_with_a_large_laplacian_everywhere_passes_the_banding_step_unchanged():
    y, x = np.mgrid[0:12, 0:14]
    f = np.repeat((((x + y) % 2) * 200 + 20).astype(np.uint8)[:, :, None], 3, axis=2)            # a checkerboard: |Laplacian| = 800
    assert np.abs(R.laplacian3_f32(R.bgr2gray_u8(f).astype(np.float32))).min() >= 30 and not R.banding_mask(f).any()
    noise = np.full(f.shape, 40.0, np.float32)
    assert np.array_equal(R.remove_banding(f, np.float64(1.0), noise), f)
    flat = np.full((6, 7, 3), 100, np.uint8)               # and a flat frame takes all of it, clipped and truncated
    m = R.banding_mask(flat)
    assert np.abs(m - 1).max() < 1e-6
    got = R.remove_banding(flat, np.float64(0.5), np.full(flat.shape, 3.0, np.float32))
    assert got.min() >= 101 and got.max() <= 101
    assert R.remove_banding(flat, np.float64(1.0), np.full(flat.shape, -500.0, np.float32)).max() == 0
    c = R.gaussian15_coeffs()
    assert c.dtype == np.float32 and abs(float(c.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(c, c[::-1]) and c.argmax() == 7


# ---- the counter generator ----------------------------------------------------------------------------------------------------------
def test_counter_noise_is_reproducible_and_keyed():
    a = R.counter_noise((9, 11, 3), np.float64(0.4), 5, 2)
    assert a.dtype == np.float32 and np.array_equal(a, R.counter_noise((9, 11, 3), np.float64(0.4), 5, 2))
    assert not np.array_equal(a, R.counter_noise((9, 11, 3), np.float64(0.4), 5, 3))
    assert not np.array_equal(a, R.counter_noise((9, 11, 3), np.float64(0.4), 6, 2))
    # a prefix property: the element index alone places a draw, whatever the frame's size
    assert np.array_equal(a.ravel()[:30], R.counter_noise((2, 5, 3), np.float64(0.4), 5, 2).ravel())
    # the product's host half builds the same key and the same tables
    for seed, index in ((0, 0), (5, 2), (2 ** 40 + 3, 77), (-1, 1)):
        assert Q.frame_key(seed, index) == R.frame_key(seed, index)
    assert np.array_equal(Q.noise_table(np.float64(0.4)), R.noise_table(np.float64(0.4)))
    assert np.array_equal(Q.gaussian15_coeffs(), R.gaussian15_coeffs())
    for d, s in ((6, 37.0), (15, 100.0)):
        for x, y in zip(Q.bilateral_tables(d, s, s), R.bilateral_tables(d, s, s)):
            assert np.array_equal(x, y)


def test_counter_noise_moments_over_2_to_the_20_draws():
    n = 1 << 20
    q = R.normal_quantiles()
    assert q.shape == (65536,) and np.all(np.diff(q) > 0) and np.allclose(q, -q[::-1], atol=1e-12) and 4.3 < q[-1] < 4.35
    table_mean, table_std = float(q.mean()), float(np.sqrt((q ** 2).mean()))
    deficit = 1.0 - table_std                       # what the midpoint quantiles and the cut tails take off the unit deviation
    assert 0 <= deficit < 1e-3 and abs(table_mean) < 1e-12
    x = q[R.noise_indices(11, 3, n)]
    # a mean of n draws of deviation <= 1 has deviation 1 / sqrt(n) = 2^-10; the sample deviation has 1 / sqrt(2 n): five of each
    assert abs(float(x.mean())) < 5 / 2 ** 10
    assert abs(float(x.std()) - 1) < 5 / np.sqrt(2 * n) + deficit
    idx = R.noise_indices(11, 3, n)
    assert idx.min() >= 0 and idx.max() <= 65535 and len(np.unique(idx)) > 60000


# ---- the product's host half against the reference's record ---------------------------------------------------------------------------
def test_value_types_answer_as_the_reference(golden):
    js = golden[0]
    cfg = Q.QPArtifactConfig()
    mine = {k: ([t.value for t in v] if isinstance(v, list) else v) for k, v in cfg.__dict__.items()}
    assert mine.pop("seed") == 0 and mine == js["defaults"]
    for bad, message in js["rejected"]:
        with pytest.raises(ValueError) as e:
            Q.QPArtifactConfig(**bad)
        assert str(e.value) == message
    assert {cls.__name__: {m.name: m.value for m in cls} for cls in (Q.ArtifactType, Q.CompressionLevel)} == js["enums"]
    assert dict(Q.QPArtifactResult().__dict__) == js["result_defaults"]
    Q.QPArtifactConfig(strength_multiplier=3.0, manual_qp=51)          # accepted, as the reference accepts it


def test_levels_strengths_and_the_factory(golden, hip_lib):
    js = golden[0]
    made = Q.create_qp_artifact_remover(False, 1.5, False, 0)
    mine = {k: ([t.value for t in v] if isinstance(v, list) else v) for k, v in made.config.__dict__.items()}
    mine.pop("seed")
    assert mine == js["created"]
    r = Q.DeviceQPArtifactRemover()
    assert {str(qp): r.compression_level(qp).value for qp in range(52)} == js["levels"]
    for key, want in js["strengths"].items():
        qp, m = key.split("|")
        s = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(strength_multiplier=float(m))).strength_for_qp(int(qp))
        assert type(s) is np.float64 and float(s) == want, key
    assert r.resolve_qp(None) == 28 and r.resolve_qp(17) == 17
    assert Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(manual_qp=35)).resolve_qp(None) == 35
    assert Q.type_mask([Q.ArtifactType.ALL]) == 7 and Q.type_mask([Q.ArtifactType.RINGING, Q.ArtifactType.BANDING]) == 6
    assert Q.type_mask([Q.ArtifactType.MOSQUITO]) == 0
    with pytest.raises(ValueError, match="qp_artifacts: strength 2 .* is above 1"):
        Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(strength_multiplier=2.0))._strength(51)


def test_detect_qp_from_video_with_recorded_ffprobe_answers(golden, hip_lib):
    js = golden[0]
    r = Q.DeviceQPArtifactRemover()
    assert len(js["ffprobe"]) >= 10
    for name, rec in js["ffprobe"].items():
        calls = []

        def run(cmd, capture_output=False, text=False, timeout=None):
            a = rec["answers"][len(calls)]
            calls.append(["<video>" if c == str(Path(__file__)) else c for c in cmd])
            assert capture_output and text and timeout == 30
            if a.get("timeout"):
                raise subprocess.TimeoutExpired(cmd, timeout)
            return types.SimpleNamespace(returncode=a["returncode"], stdout=a["stdout"], stderr="")

        assert r.detect_qp_from_video(Path(__file__), run=run) == rec["result"], name
        assert calls == rec["commands"], name
    got = {n: rec["result"] for n, rec in js["ffprobe"].items()}
    assert got["frames_with_qp"] == 26 and [got[f"bpp_{b}"] for b in ("0.6", "0.3", "0.15", "0.07")] == [18, 23, 28, 34]
    assert got["bpp_0.01_default_size"] == 40 and got["timeout"] is None and got["both_fail"] is None
    assert r.detect_qp_from_video(Path(__file__).with_name("no_such_video.mp4"), run=None) is None


@pytest.mark.parametrize("qp_arg,manual", [(None, None), (None, 35), (40, 35)])
def test_remove_artifacts_with_in_memory_images(golden, hip_lib, tmp_path, qp_arg, manual):
    want = golden[0]["directory"][f"qp{qp_arg}|manual{manual}"]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = {f"f{i:03d}.png": R.content_frame(12, 16, 10 + i) for i in range(5)}
    for name in frames:
        (src / name).write_bytes(name.encode())
    written, progress = {}, []

    def read(path):
        return None if Path(path).name == "f002.png" else frames[Path(path).name].copy()

    def write(path, img):
        if Path(path).name == "f003.png":
            raise OSError("disk full")
        written[Path(path).name] = img

    r = Q.DeviceQPArtifactRemover(Q.QPArtifactConfig(manual_qp=manual, artifact_types=[Q.ArtifactType.BLOCKING]))
    indices = []

    def process(fs, qp=None, noise=None, first_index=0):                    # the frame path itself is the GPU tests' matter
        indices.append(first_index)
        return [R.process_frame(f, qp, r.config, (r.config.seed, first_index)) for f in fs]

    r.process = process
    res = r.remove_artifacts(src, dst, qp_arg, progress.append, read=read, write=write)
    assert (res.frames_processed, res.frames_failed, res.detected_qp, res.compression_level.value, res.artifacts_removed) == \
        (want["frames_processed"], want["frames_failed"], want["detected_qp"], want["compression_level"], want["artifacts_removed"])
    assert sorted(written) == want["written"] and sorted(p.name for p in dst.iterdir()) == want["copied"] and progress == want["progress"]
    assert res.output_dir == dst and res.processing_time_seconds >= 0 and indices == [0, 1, 3, 4]
    assert (dst / "f003.png").read_bytes() == b"f003.png"                   # the copy of what could not be written
    for name, img in written.items():
        assert np.array_equal(img, R.remove_blocking(frames[name], R.strength_for_qp(res.detected_qp, 1.0), 8))
    empty = r.remove_artifacts(tmp_path / "none", tmp_path / "out2", qp_arg, read=read, write=write)
    assert (empty.frames_processed, empty.frames_failed, empty.detected_qp, empty.artifacts_removed) == \
        (want["empty"]["frames_processed"], want["empty"]["frames_failed"], want["empty"]["detected_qp"], want["empty"]["artifacts_removed"])
    r.close()
    closed = r.remove_artifacts(src, dst, qp_arg, read=read, write=write)
    assert closed.frames_processed == 0 and closed.detected_qp is None and not r.is_available()
