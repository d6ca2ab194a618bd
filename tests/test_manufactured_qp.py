"""The QP solvers of the CPU oracle on manufactured QPs whose exact primal-dual solutions are known
by construction (tests/manufactured_qp.py), off the OCP's data: generic A, B, H, dx0 and bound
offsets of order one, so that no term of the Riccati recursion or the interior point is ~0 or ~1.

The literal restatement (oracle/qsp_oracle.c) is held to the exact solution absolutely; the
kernel-order twin (oracle/qsp_twin.cpp, which compiles the kernels' own lane arithmetic) is held to 4x the
literal restatement's own worst error on the same batch -- the two differ only in association order
(their worst errors agree to two digits below), while a wrong term shows as 1e-2 or more.  The GPU
runs the same batches in tests/test_gpu_manufactured_qp.py.

Measured (64 lanes, mu_stop 1e-10, cap 50; worst over the status-0 lanes, literal = twin to two digits):
    family     lanes at status 0     max|dx - dx*|       max|du - du*|       max|pi - pi*|
    F0         59 .. 64 of 64        2.0e-10 .. 5.0e-10  4.1e-10 .. 7.6e-10  2.9e-10 .. 5.2e-10
    Fu         58 .. 64              3.5e-10 .. 1.7e-09  5.9e-10 .. 3.3e-09  (carries the dual floor: lam to 7.5e-5)
    Fu-ocp     59 .. 63              3.5e-10 .. 1.5e-09  7.0e-10 .. 2.6e-09
    Fs-small   62 .. 64              6.0e-07 .. 2.9e-05  2.2e-06 .. 9.9e-05  6.7e-06 .. 4.9e-03 (truncation: slack ~ mu / lam)
The generic state-bound families Fs and Fall are NOT solved to this accuracy in double: see
test_double_meets_the_dual_floor_on_state_bounds and DESIGN.md section 2.
"""
import functools

import numpy as np
import pytest

import manufactured_qp as M
from oracle.oracle import Oracle, make_opts

NB = 64
EXACT_FAMILIES = ("F0", "Fu", "Fu-ocp", "Fs-small")


@pytest.fixture(autouse=True)
def default_walk(monkeypatch):
    monkeypatch.delenv("QSP_MFMA_WALK", raising=False)   # the developer A/B switch the twin follows


@functools.lru_cache(maxsize=None)
def oracles():
    return Oracle(), Oracle(twin=True)


@functools.lru_cache(maxsize=None)
def batch(name, N):
    return M.named_batch(name, N, NB)


def opts(N, S=0, scan=0, **kw):
    return make_opts(N=N, qp_iters=M.QP_ITERS, stage0_s_bound=0, stages_per_lane=S, factor_scan=scan, **kw)


@functools.lru_cache(maxsize=None)
def literal(name, N):
    """The literal restatement's answer, computed once per batch and shared (callers leave it unchanged)."""
    return oracles()[0].qp(opts(N), *M.qp_args(batch(name, N)))


@pytest.mark.parametrize("N", [3, 20, 50])
@pytest.mark.parametrize("name", list(M.NAMED))
def test_constructed_point_is_the_solution(name, N):
    """The generator's self-test: the constructed point satisfies every KKT condition to 1e-13
    (measured: 2e-15), is feasible, and its objective is not above the literal oracle's answer on any
    lane -- up to the answer's own bound violation d, which can buy at most sum(lam*) d (the multipliers
    are the sensitivities of the optimal value), and 1e-12 relative of rounding."""
    q = batch(name, N)
    res = M.kkt_residuals(q, q["dx"], q["du"], q["pi"], q["lam"])
    for k, v in res.items():
        assert v.max() <= 1e-13, (k, v.max())
    v = np.concatenate([q["dx"][:, :N, 3:4], q["du"]], 2)
    assert np.all(v >= q["lo"] - 1e-15) and np.all(v <= q["hi"] + 1e-15)
    assert np.all(q["lam"] >= 0) and np.all(np.isfinite(q["g"]))
    # every lane keeps LICQ: an active s_k has a free input at stage k-1
    st = q["state"]
    assert not np.any((st[:, 1:, 0] != 0) & (st[:, :-1, 1] != 0) & (st[:, :-1, 2] != 0)) and not st[:, 0, 0].any()
    r = literal(name, N)
    fin = np.isfinite(r["du"]).all((1, 2))
    assert fin.all()
    f_star, f_or = M.objective(q, q["dx"], q["du"]), M.objective(q, r["dx"], r["du"])
    viol = M.kkt_residuals(q, r["dx"], r["du"], r["pi"], r["lam"])["infeas"]
    slackness = q["lam"].sum((1, 2)) * viol + 1e-12 * (1 + np.abs(f_star))
    assert np.all(f_star <= f_or + slackness), float((f_star - f_or - slackness).max())


def test_families_cover_their_active_sets():
    """The families differ as they claim: F0 has no active bound, Fu only input bounds, Fs only state
    bounds, Fall both, each at both sides."""
    N = 20
    for name, (s_act, u_act) in {"F0": (0, 0), "Fu": (0, 1), "Fs": (1, 0), "Fall": (1, 1)}.items():
        st = batch(name, N)["state"]
        assert bool((st[:, :, 0] != 0).any()) == bool(s_act) and bool((st[:, :, 1:] != 0).any()) == bool(u_act), name
        if s_act:
            assert (st[:, :, 0] == 1).any() and (st[:, :, 0] == 2).any()
            assert 0.15 < (st[:, 1:, 0] != 0).mean() < 0.35
        if u_act:
            assert (st[:, :, 1:] == 1).any() and (st[:, :, 1:] == 2).any()
    b70 = M.named_batch("Fu", N, 70)
    for k, v in batch("Fu", N).items():
        np.testing.assert_array_equal(v, b70[k][:NB])    # the GPU's 70 lanes extend these 64


@pytest.mark.parametrize("N,S,scan", M.CONFIGS)
@pytest.mark.parametrize("name", EXACT_FAMILIES)
def test_literal_and_twin_reach_the_exact_solution(name, N, S, scan):
    """Literal restatement and twin (every factorisation walk, both lane layouts) against the exact
    solution.  The literal oracle's own error on F0, Fu (and Fu with the OCP's zero pattern) is bounded
    absolutely, 1e-8 max|du*| (measured: at most 3.3e-9); the twin by 4x the literal oracle's
    worst error on this batch (measured ratio: 1.000 on F0, Fu, Fu-ocp; 0.40 .. 1.13 on Fs-small, whose
    errors are rounding-tinged).  On F0, Fu, Fu-ocp the two also take the same path: the same status and
    iteration count on all but at most two lanes (measured: every lane; manufactured_qp.path_differences).
    pi is compared where no bound is active (F0); both meet the stop test on at least 85 % of the lanes
    (measured: 58 of 64 or more), and their inactive multipliers are below what the stop test promises
    (mu over the slack; measured: 0.055 of that bound at the most)."""
    q = batch(name, N)
    lit, tw = literal(name, N), oracles()[1].qp(opts(N, S, scan), *M.qp_args(q))
    e_lit, e_tw = M.worst_errors(lit, q), M.worst_errors(tw, q)
    print(f"{name} N={N} S={S} scan={scan}: status 0 literal {np.sum(lit['qp_status'] == 0)} twin {np.sum(tw['qp_status'] == 0)}"
          f" of {NB}; literal {e_lit}; twin {e_tw}")
    for r in (lit, tw):
        assert np.mean(r["qp_status"] == 0) >= M.MIN_CONVERGED
        assert M.inactive_multiplier_excess(r, q) <= 1.0
    keys = ("dx", "du", "pi") if name.startswith("F0") else ("dx", "du")
    if name != "Fs-small":
        for k in keys:
            assert e_lit[k] <= 1e-8 * np.abs(q["du"]).max(), (k, e_lit[k])
        assert M.path_differences(tw, lit) <= M.MAX_PATH_DIFFERENCES   # same statuses, same iteration counts
    for k in keys:
        assert e_tw[k] <= 4.0 * e_lit[k], (k, e_tw[k], e_lit[k])


@pytest.mark.parametrize("N,S,scan", [(20, 1, 0), (32, 2, 0), (32, 2, 1)])
def test_infeasible_stage0_s_is_status_3(N, S, scan):
    """stage0_s_bound = 1 and dx0's s 0.1 below its bounds: the fixed stage-0 s cannot be moved, and both
    solvers say infeasible (3) on every lane; with the bound off the same QPs are ordinary."""
    q = M.named_batch("Fu", N, NB, stage0_infeasible=True)
    lit, tw = oracles()
    for s0, want in ((1, 3), (0, None)):
        op = make_opts(N=N, qp_iters=M.QP_ITERS, stage0_s_bound=s0, stages_per_lane=S, factor_scan=scan)
        for o in (lit, tw):
            st = o.qp(op, *M.qp_args(q, s0))["qp_status"]
            if want is None:
                assert np.mean(st == 0) >= M.MIN_CONVERGED and not np.any(st == 3)
            else:
                assert np.all(st == want), st


def quad_bound(N, lam_min=M.GENERIC["lam_range"][0]):
    """How far a status-0 answer may be from the exact solution by the stop test alone: mean(lam t) <
    mu_stop over m = 6N rows leaves an active bound's slack t below m mu_stop / lam_min, and the primal
    point moves by that times the conditioning of the active rows (B's s row, entries of order 0.5,
    triangular in the free inputs: a factor 10 is allowed)."""
    return 10.0 * 6 * N * M.MU_STOP / lam_min


@pytest.mark.parametrize("N", [3, 20, 50])
def test_quad_is_exact_on_state_bounds(N):
    """The literal restatement's QP evaluated in __float128 (Oracle.qp_ext) reaches the exact solution of
    the generic state-bound family Fs, where the double evaluation is wrong by up to 0.3: the formulas
    are right, the double recursion's rounding is the cause.  Bound: quad_bound,
    from the stop test (1.8e-7, 1.2e-6, 3e-6); measured max|du - du*| 2.4e-9, 1.6e-8, 2.0e-6 at
    N = 3, 20, 50 against 0.10, 0.42, 0.14 in double.  The u-stationarity of the
    returned du, pi, lam -- which the stop test tracks as r0 prod(1 - alpha) < qp_tol_stat = 1e-10, exact
    only if every Newton step is -- holds to 1e-10 in quad (measured 1.1e-12 at the most) and fails by O(1) in double."""
    q = batch("Fs", N)
    lit = oracles()[0]
    r = lit.qp_ext(opts(N), *M.qp_args(q), precision="quad")
    m = r["qp_status"] == 0
    e = M.worst_errors(r, q)
    res = M.kkt_residuals(q, r["dx"], r["du"], r["pi"], r["lam"])
    print(f"Fs N={N} quad: status 0 {m.sum()} of {NB}; {e}; stat_u {res['stat_u'][m].max():.1e}")
    assert m.mean() >= M.MIN_CONVERGED
    assert e["dx"] <= quad_bound(N) and e["du"] <= quad_bound(N), e
    assert res["stat_u"][m].max() <= 1e-10
    if N <= 20:   # the double evaluation of the same formulas is off by what a wrong term would give
        assert M.worst_errors(literal("Fs", N), q)["du"] > 1e-2


@pytest.mark.xfail(strict=True, reason="double precision limit of the Riccati recursion under state-bound "
                   "barrier weights lam/t ~ 1e12 (DESIGN.md section 2); a reformulation is a separate change")
@pytest.mark.parametrize("which", ["literal", "twin"])
def test_double_meets_the_dual_floor_on_state_bounds(which):
    """What a status-0 QP should satisfy and, with active state bounds and O(1) multipliers, does not:
    the u-stationarity of the returned du, pi, lam within 1e-8 relative plus the dual-accuracy floor of
    tests/test_oracle.py::test_qp_kkt (N max(lam/t) eps max|lo, hi|), on every status-0 lane of generic Fs,
    N = 20.  Measured: residual up to 1.7 (literal, 24 lanes at status 0) and 2.2 (twin, 38 lanes)
    against floors of 3e-5 .. 7e-3; max|du - du*| 0.42 (literal).  Strict: when the recursion is
    reformulated this test passes and the mark has to go."""
    N = 20
    q = batch("Fs", N)
    r = literal("Fs", N) if which == "literal" else oracles()[1].qp(opts(N, 1, 0), *M.qp_args(q))
    m = r["qp_status"] == 0
    assert m.any()
    res = M.kkt_residuals(q, r["dx"], r["du"], r["pi"], r["lam"])["stat_u"]
    v = np.concatenate([r["dx"][:, :N, 3:4], r["du"]], 2)
    t = np.stack([v - q["lo"], q["hi"] - v], 3).reshape(NB, N, 6)
    sig = np.abs(r["lam"]) / np.maximum(np.abs(t), 1e-300)
    sig[:, 0, :2] = 0.0
    off = np.maximum(np.abs(q["lo"]), np.abs(q["hi"])).reshape(NB, -1).max(1)
    floor = N * sig.reshape(NB, -1).max(1) * np.finfo(float).eps * off
    scale = 1 + np.abs(q["g"]).max(1)
    print(f"Fs N={N} {which}: status 0 {m.sum()}; stat_u max {res[m].max():.2e}; floor {floor[m].min():.1e} .. {floor[m].max():.1e}")
    assert np.all(res[m] <= 1e-8 * scale[m] + floor[m])
