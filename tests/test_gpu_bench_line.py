"""bench.py's plain line and --dump-outputs on the device: a plain run times exactly --steps solves,
prints the headline with what those solves yield and none of --full's legs, and writes the last
solve's outputs as FP64 .npy files that agree with the device arrays --dump-u0 saves."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dump_outputs(tmp_path):
    total, N = 1536, 20
    out = tmp_path / "outputs"
    u0f = tmp_path / "u0.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--global-batch", str(total), "--dump-outputs", str(out), "--dump-u0", str(u0f)],
                       cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "solves/s" and rec["dtype"] == "f64"
    assert rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    np.testing.assert_allclose(rec["value"], total / (rec["ms_per_step"] * 1e-3), rtol=1e-9)
    assert rec["kernels_ms_avg"]["qp_step"] > 0 and rec["roofline"]["frac"] > 0
    for leg in ("host_boundary_solves_per_s", "configs2_qp50", "configs1", "configs4", "closed_loop", "side_rows",
                "cpu_baseline", "cpu_literal_oracle", "parity", "parity_literal"):
        assert leg not in rec, leg
    shapes = {"u0": (total, 2), "status": (total,), "cost": (total,), "X": (total, N + 1, 4), "U": (total, N, 2),
              "PI": (total, N, 4)}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in shapes)
    got = {k: np.load(out / (k + ".npy")) for k in shapes}
    for k, s in shapes.items():
        assert got[k].dtype == np.float64 and got[k].shape == s, k
    ref = np.load(u0f)
    np.testing.assert_array_equal(got["u0"], ref["u0"])
    np.testing.assert_array_equal(got["status"], ref["status"])
    ok = got["status"] == 0
    assert ok.any() and all(np.isfinite(got[k][ok]).all() for k in shapes)
    assert np.abs(got["X"][ok]).max() > 0 and np.abs(got["U"][ok]).max() > 0
