"""bench.py's plain run (headline only) and --dump-outputs: what the timed path returned in its last step, from inputs that depend only on
the arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_a_fixed_sample_within_the_limit(tmp_path):
    import bench

    a = np.arange(1000 * 8, dtype=np.float32).reshape(1000, 8)
    bench.dump_outputs(str(tmp_path / "whole"), "y", a, 1 << 20)
    assert np.array_equal(np.load(tmp_path / "whole" / "y.npy"), a)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), "y", a, 100 * a[:1].nbytes)
    s = np.load(tmp_path / "s1" / "y.npy")
    assert s.dtype == np.float32 and s.shape == (100, 8)
    assert np.array_equal(s, np.load(tmp_path / "s2" / "y.npy"))  # the same rows every time
    rows = (s[:, 0] / 8).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(s, a[rows])  # whole rows of the output, in their original order


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run prints the headline line without the --full diagnostics; its dump is the (16384, 2 n^2) result of the seeded batch, the same
    whatever the number of steps, and right against the fp64 CPU oracle."""
    import bench
    from gridcodegenerator_amd import RobotModel
    from oracle.rbd_oracle import Oracle

    dumps = {}
    for steps in (3, 7):
        d = tmp_path / ("steps%d" % steps)
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == steps and line["unit"] == "solves/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert abs(line["value"] - 16384 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        for moved in ("cpu_baseline", "other_configs", "copy_bw_measured_GBps", "end_to_end_solves_per_s", "other_scaling"):
            assert moved not in line, moved
        assert "launch_us_median" not in line["roofline"]
        assert sorted(os.listdir(d)) == ["df_du.npy"]
        dumps[steps] = np.load(d / "df_du.npy")
    got = dumps[3]
    assert got.dtype == np.float32 and got.shape == (16384, 98)
    assert np.array_equal(got, dumps[7])
    robot = RobotModel.from_fixture("iiwa14")
    x = bench.make_inputs(robot.n, 16384)
    idx = np.random.default_rng(1).choice(16384, 64, replace=False)
    ref, _ = Oracle(robot).fd_grad_batch(x[idx].astype(np.float64))
    err = max(np.abs(got[k] - ref[i]).max() / np.abs(ref[i]).max() for i, k in enumerate(idx))
    assert err <= 1e-4, err
