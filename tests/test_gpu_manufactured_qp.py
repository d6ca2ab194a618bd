"""GPU: qsp_qp_solve on manufactured QPs whose exact primal-dual solutions are known by construction
(tests/manufactured_qp.py; the CPU side is tests/test_manufactured_qp.py), off the OCP's data: generic A,
B, H, dx0 and bound offsets of order one.  Every factorisation walk (lane walk, matrix cores, associative
scan) at both edges of its horizon range, both lane layouts, 70 QPs per batch so that the last
wavefront group is partial.

Two comparisons per batch, from one qp_solve call:
  - bit for bit against the oracle's kernel-order twin (as tests/test_gpu_twin.py: qp_status, iters, dx,
    du, pi, lam; no tolerance) -- also on the generic state-bound families, where the answers are
    rounding-dominated and any difference of arithmetic order would show;
  - against the exact solution, within 4x the literal restatement's own worst error on the same batch
    (the literal restatement compiles none of the kernels' headers): an error of the shared lane
    arithmetic is on both sides of the first comparison, not of this one.
Measured errors: the table of tests/test_manufactured_qp.py (the device reproduces the twin's bits).
"""
import functools

import numpy as np
import pytest

import manufactured_qp as M
from oracle.oracle import Oracle, make_opts, tw_factor_walk

pytestmark = pytest.mark.gpu

NB = 70
NAMES = ("santal", "balea", "montana", "pulirapid")
EXACT_FAMILIES = ("F0", "Fu", "Fu-ocp", "Fs-small")
BIT_FAMILIES = EXACT_FAMILIES + ("Fs", "Fall")


@pytest.fixture(autouse=True)
def default_walk(monkeypatch):
    monkeypatch.delenv("QSP_MFMA_WALK", raising=False)   # the developer A/B switch library and twin follow


@functools.lru_cache(maxsize=None)
def oracles():
    return Oracle(NAMES), Oracle(NAMES, twin=True)


@functools.lru_cache(maxsize=None)
def batch(name, N):
    return M.named_batch(name, N, NB)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {i}: gpu {a[i]!r} twin {b[i]!r}")


def gpu_qp(q, N, S, scan, s0=0):
    """One qsp_qp_solve of the batch on a handle of its own, whose factorisation walk is the twin's."""
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    op = make_opts(N=N, qp_iters=M.QP_ITERS, stage0_s_bound=s0, stages_per_lane=S, factor_scan=scan)
    s = OcpSolver(N=N, batch=NB, qp_iters=M.QP_ITERS, stages_per_lane=S, factor_scan=bool(scan), stage0_s_bound=bool(s0))
    try:
        s.set_shapes([make_shape(n) for n in NAMES])
        assert s.layout()[0] == S
        assert s.factor_walk() == s.FACTOR_WALKS[tw_factor_walk(op)]
        A, B, b, H, g, lo, hi, act, dx0 = M.qp_args(q, s0)
        r = s.qp_solve(A, B, b, H, g, lo, hi, dx0)
    finally:
        s.close()
    return r, op


@functools.lru_cache(maxsize=None)
def solved(name, N, S, scan):
    """GPU and twin answers of one batch, computed once and shared by the two comparisons."""
    q = batch(name, N)
    r, op = gpu_qp(q, N, S, scan)
    return r, oracles()[1].qp(op, *M.qp_args(q))


@pytest.mark.parametrize("N,S,scan", M.CONFIGS)
@pytest.mark.parametrize("name", BIT_FAMILIES)
def test_bit_identical_to_the_twin(name, N, S, scan):
    r, t = solved(name, N, S, scan)
    for k in ("qp_status", "iters", "dx", "du", "pi", "lam"):
        same(r[k], t[k], f"{name} N={N} S={S} scan={scan}: qp {k}")


@pytest.mark.parametrize("N,S,scan", M.CONFIGS)
@pytest.mark.parametrize("name", EXACT_FAMILIES)
def test_reaches_the_exact_solution(name, N, S, scan):
    """The device's answer against the exact solution: within 4x the literal restatement's own worst
    error on this batch (status-0 lanes; dx, du, and pi where no bound is active), the stop test met on at
    least 85 % of the lanes, inactive multipliers below what the stop test promises (mu over the slack).
    The literal restatement itself is held to 1e-8 max|du*| on F0, Fu and Fu-ocp, as on the CPU, and on
    those families the device takes the literal restatement's path (status and iteration count) on all
    but at most two lanes.  Measured on an MI355X (profiles/manufactured_qp/gpu_tests.txt): 63 .. 70 of 70
    lanes at status 0; max|du - du*| 4.1e-10 .. 3.3e-9 on F0, Fu, Fu-ocp, 2.2e-6 .. 9.9e-5 on Fs-small, equal
    to the literal restatement's to two digits or more; no path difference."""
    q = batch(name, N)
    r = solved(name, N, S, scan)[0]
    op = make_opts(N=N, qp_iters=M.QP_ITERS, stage0_s_bound=0)
    lit = oracles()[0].qp(op, *M.qp_args(q))
    e_lit, e_gpu = M.worst_errors(lit, q), M.worst_errors(r, q)
    print(f"{name} N={N} S={S} scan={scan}: status 0 literal {np.sum(lit['qp_status'] == 0)} gpu {np.sum(r['qp_status'] == 0)}"
          f" of {NB}; literal {e_lit}; gpu {e_gpu}")
    for x in (lit, r):
        assert np.mean(x["qp_status"] == 0) >= M.MIN_CONVERGED
        assert M.inactive_multiplier_excess(x, q) <= 1.0
    keys = ("dx", "du", "pi") if name.startswith("F0") else ("dx", "du")
    if name != "Fs-small":
        for k in keys:
            assert e_lit[k] <= 1e-8 * np.abs(q["du"]).max(), (k, e_lit[k])
        assert M.path_differences(r, lit) <= M.MAX_PATH_DIFFERENCES   # same statuses, same iteration counts
    for k in keys:
        assert e_gpu[k] <= 4.0 * e_lit[k], (k, e_gpu[k], e_lit[k])


@pytest.mark.parametrize("N,S,scan", [(20, 1, 0), (32, 2, 1)])
def test_infeasible_stage0_s_is_status_3(N, S, scan):
    """stage0_s_bound = 1 and dx0's s 0.1 below its bounds: infeasible (3) on every lane, on the device as on
    the twin and the literal restatement; everything the device returns equals the twin's bits."""
    q = M.named_batch("Fu", N, NB, stage0_infeasible=True)
    r, op = gpu_qp(q, N, S, scan, s0=1)
    assert np.all(r["qp_status"] == 3), r["qp_status"]
    lit, tw = oracles()
    assert np.all(lit.qp(op, *M.qp_args(q, 1))["qp_status"] == 3)
    t = tw.qp(op, *M.qp_args(q, 1))
    for k in ("qp_status", "iters", "dx", "du", "pi", "lam"):
        same(r[k], t[k], f"infeasible N={N} S={S} scan={scan}: qp {k}")
