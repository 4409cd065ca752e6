"""bench.py as the measurement runs it: a plain run prints the headline fields only and --dump-outputs writes the frame
of the last timed step, which must be the frame the path computes for the workload's inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import raytracing_engine_amd as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_frame(tmp_path, renderer):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--workload", "spheres8_1080p_4spp", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = lines[0]
    assert line["metric"] == "Mrays/s" and line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"parity", "roofline", "cpu_baseline", "one_frame_at_a_time"} & set(line)  # behind --full
    assert sorted(os.listdir(tmp_path)) == ["rgb.npy"]
    rgb = np.load(tmp_path / "rgb.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (1080, 1920, 3)
    renderer.set_partition(0, 1)
    renderer.set_config(renderer.default_config())
    renderer.set_scene(R.cornell_scene())
    renderer.resize(1920, 1080)
    assert np.array_equal(rgb, renderer.render((0, 0, 0, 1), (0, 0, 0), spp=4))
