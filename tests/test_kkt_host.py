"""CPU: csrc/qsp_kkt.hpp itself, compiled for the host in a program of its own (tests/stubs/kkt_main.cpp):
kkt_qp_stage, the per-(lane, stage) function of qsp_qp_residuals' kernel, on manufactured QPs with exact
solutions (tests/manufactured_qp.py).  Built with the address and undefined-behaviour sanitizers, as
tests/test_sim_noise_host.py builds its program.  Nothing is loaded into Python.

Every comparison uses the derived bound of tests/kkt_ref.py, |got - ref| <= 64 eps * term scale."""
import subprocess

import numpy as np
import pytest

import host_program
import kkt_ref
import manufactured_qp as mq

ORDER = ("A", "B", "b", "H", "g", "lo", "hi", "dx0")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program.build("kkt_main", tmp_path_factory.mktemp("kkt") / "kkt_main")


def run(exe, path, q, point, s0):
    nb, N = q["b"].shape[:2]
    with open(path, "wb") as fh:
        fh.write(np.array([N, nb, s0, 0], np.int32).tobytes())
        for a in [q[k] for k in ORDER] + list(point):
            fh.write(np.ascontiguousarray(a, np.float64).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "kkt ok", r.stdout
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[1:1 + nb]])
    assert got.shape == (nb, 6)
    return {k: got[:, i] for i, k in enumerate(kkt_ref.QP_KEYS)}


@pytest.mark.parametrize("N", [3, 20])
def test_kkt_qp_stage_on_the_host(exe, tmp_path, N):
    nb = 7
    q = mq.make_batch("Fall", N, nb, 1)
    exact = (q["dx"], q["du"], q["pi"], q["lam"])
    rng = np.random.default_rng(11)
    pert = tuple(a + 1e-3 * rng.uniform(-1, 1, a.shape) for a in exact)
    worst = {}
    for s0 in (0, 1):
        # the exact solution: every residual is rounding
        got = run(exe, tmp_path / "q.bin", q, exact, s0)
        _, scale = kkt_ref.qp_residuals(q, *exact, s0)
        for k in kkt_ref.QP_KEYS:
            worst["exact", k] = max(worst.get(("exact", k), 0.0), kkt_ref.worst_ratio(got[k], 0.0, scale[k]))
            assert np.all(np.abs(got[k]) <= kkt_ref.BOUND * scale[k]), (s0, k, got[k], scale[k])
        # a perturbed point: the numpy restatement
        got = run(exe, tmp_path / "q.bin", q, pert, s0)
        ref, scale = kkt_ref.qp_residuals(q, *pert, s0)
        for k in kkt_ref.QP_KEYS:
            worst["pert", k] = max(worst.get(("pert", k), 0.0), kkt_ref.worst_ratio(got[k], ref[k], scale[k]))
            assert np.all(np.abs(got[k] - ref[k]) <= kkt_ref.BOUND * scale[k]), (s0, k, got[k], ref[k])
        assert got["stat_u"].min() > 1e-5 and got["dyn"].min() > 1e-5      # the perturbation is seen
    # the stage-0 s row off and its multipliers zero: tests/manufactured_qp.py::kkt_residuals
    for name, point in (("exact", exact), ("pert", pert)):
        lam = point[3].copy()
        lam[:, 0, :2] = 0.0
        point = point[:3] + (lam,)
        got = run(exe, tmp_path / "q.bin", q, point, 0)
        ref = mq.kkt_residuals(q, *point)
        _, scale = kkt_ref.qp_residuals(q, *point, 0)
        for k in kkt_ref.QP_KEYS:
            worst["mq-" + name, k] = kkt_ref.worst_ratio(got[k], ref[k], scale[k])
            assert np.all(np.abs(got[k] - ref[k]) <= kkt_ref.BOUND * scale[k]), (name, k, got[k], ref[k])
    print("N = %d: worst |got - ref| / (64 eps term scale): %s" % (N, {k: "%.3f" % v for k, v in worst.items()}))
