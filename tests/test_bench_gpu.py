"""bench.py on the GPU, in fresh processes at a small frame size: a plain run prints the headline line without the --full legs, and
what --dump-outputs writes is the frame the path hands back for the last timed step; --full adds the legs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FULL_LEGS = ("energy", "parity", "cpu_baseline", "host_to_host")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--height", "136", "--width", "240", *args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_frame(hip_lib, tmp_path):
    res = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert res["steps"] == 3 and res["dtype"] == "f16" and res["unit"] == "frames/s" and res["higher_is_better"] is True
    assert abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
    assert res["roofline"] is None and not any(k in res for k in FULL_LEGS)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["sr_out.npy"]
    got = np.load(tmp_path / "out" / "sr_out.npy")
    assert got.dtype == np.float32 and got.shape == (544, 960, 3)
    # bench.py's inputs: seeded weights, seeded frames (3 distinct for 3 steps), step i on frame i % 3
    from framewright_amd.realesrgan import RRDBNetEngine
    from framewright_amd.synth import synthetic_frames, synthetic_rrdbnet_state
    eng = RRDBNetEngine(23, 4, "f16", device_id=0)
    eng.load_state_dict(synthetic_rrdbnet_state(23, 4, seed=1234))
    frame = torch.from_numpy(np.ascontiguousarray(synthetic_frames(3, 136, 240, seed=2)[2])).cuda()
    want = eng.upscale_device(frame)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    eng.close()
    assert np.array_equal(got, want.astype(np.float32))


def test_full_run_adds_its_legs(hip_lib):
    res = _bench("--full", "--steps", "2", "--warmup", "1", "--cpu-crop", "32")
    assert res["steps"] == 2 and res["roofline"]["bound"] == "mfma" and res["roofline"]["achieved"] > 0
    assert res["parity"]["max_lsb"] <= 1 and res["cpu_baseline"]["value"] > 0 and res["host_to_host"]["frames"] == 2


@pytest.mark.parametrize("config,names", [("rife", ["rife_mid"]), ("tap", ["tap_denoised"]), ("chain", ["chain_mid", "chain_upscaled"])])
def test_dump_outputs_of_every_config(hip_lib, tmp_path, config, names):
    res = _bench("--config", config, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert res["steps"] == 3 and res["roofline"] is None
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == [f"{n}.npy" for n in names]
    for n in names:
        a = np.load(tmp_path / "out" / f"{n}.npy")
        side = (544, 960) if config == "chain" else (136, 240)
        assert a.dtype == np.float32 and a.shape == (*side, 3) and 0 <= a.min() and a.max() <= 255 and a.std() > 0
