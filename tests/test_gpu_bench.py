"""A plain `bench.py --gpus 1 --steps K --warmup W` run on the GPU: the result
line carries the headline alone (none of the --full legs), --steps sets the
number of timed steps, and --dump-outputs writes the image the timed path
computed — checked bit-for-bit against the CPU oracle.  Config A (256x256,
38 triangles) keeps the run to a moment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("alt_traversal", "scalar_valu", "parity", "config_C", "config_E", "config_W")


def test_plain_run_is_lean_and_dumps_its_image(rt2mod, oraclemod, config_scene, tmp_path):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "A", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    sd, spec = config_scene("A")
    samples = spec.width * spec.height * spec.rays * spec.frames
    # both figures are rounded to 3 decimals: half a unit in the last place of each
    rel = 0.0005 / line["ms_per_step"] + 0.0005 / line["value"] + 1e-6
    assert line["value"] == pytest.approx(samples / (line["ms_per_step"] * 1e-3) / 1e6, rel=2 * rel)
    assert line["cpu_baseline"] is None and not [k for k in FULL_ONLY if k in line]

    assert os.listdir(out) == ["image.npy"]
    img = np.load(out / "image.npy")
    assert img.dtype == np.float32 and img.shape == (spec.height, spec.width, 4)
    u = rt2mod.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    acc, _, _, _ = oraclemod.render(sd.triangles(), sd.materials(), u, np.arange(spec.height, dtype=np.int32), 0,
                                    spec.frames, "brute")
    assert np.array_equal(img[..., :3], (acc / np.float32(spec.frames))[..., :3])
