"""CPU: the numpy restatement of the rollout cost / u0 cost landscape (tests/rollout_ref.py) pins
itself -- across the oracle's two formulations of f, on MATLAB's colon grid, and on MATLAB's min rule
-- and hands the GPU tests their tolerance."""
import numpy as np
import pytest

import rollout_ref as R
from conftest import config2_x0, straight_traj

# Largest relative cost difference of the restatement between Oracle() and Oracle(twin=True) on the
# workload of test_restatement_agrees_across_formulations, measured on the CPU: 1.7e-14 (RK4; Euler
# 2.6e-15; x_end 2.6e-15 absolute; the argmin identical on every lane).  The GPU tests compare against
# the restatement within 100 x that: the tolerance comes from the reference's own spread.
MEASURED_SPREAD = 1.7e-14
ROLLOUT_RTOL = 100 * MEASURED_SPREAD


@pytest.fixture(scope="module")
def twin():
    from oracle.oracle import Oracle
    return Oracle(twin=True)


def test_restatement_agrees_across_formulations(oracle, twin):
    B, N = 32, 20
    x0 = config2_x0(B, 21)
    sid = np.arange(B) % 4
    yref = np.repeat(straight_traj()[None, :N], B, 0)
    ye = yref[:, N - 1, :4].copy()
    rng = np.random.default_rng(3)
    tail = np.stack([rng.uniform(0.001, 0.03, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], 2)   # feasible
    un, ut = R.colon_grid(0.0, 0.03), R.colon_grid(-0.05, 0.05)
    cand = R.landscape_candidates(tail, un, ut)
    assert cand.shape == (B, 147, N, 2)
    for integ in ("euler", "rk4"):
        ca, va, xa = R.rollout_cost(oracle, x0, cand, sid, yref, ye, integrator=integ)
        cb, vb, xb = R.rollout_cost(twin, x0, cand, sid, yref, ye, integrator=integ)
        rel = (np.abs(ca - cb) / np.abs(cb)).max()
        dx = np.abs(xa - xb).max()
        print(f"{integ}: max rel cost diff {rel:.2e}, max |x_end diff| {dx:.2e}, max |viol diff| {np.abs(va - vb).max():.2e}")
        assert np.all(np.isfinite(ca)) and np.all(np.isfinite(cb))
        assert rel < 1e-12, rel
        assert dx < 1e-12, dx
        assert rel < ROLLOUT_RTOL and dx < ROLLOUT_RTOL, (rel, dx, "the spread has outgrown ROLLOUT_RTOL")
        assert np.array_equal(R.first_min(ca)[1], R.first_min(cb)[1])
        # the landscape wrapper is the same rollout
        surf, u_min, cmin, imin = R.cost_landscape(twin, x0, tail, un, ut, sid, yref, ye, integrator=integ)
        assert np.array_equal(surf.reshape(B, -1), cb)
        assert np.array_equal(cmin, cb.min(1)) and np.array_equal(imin, cb.argmin(1))
        assert np.array_equal(u_min[:, 0], un[imin // 21]) and np.array_equal(u_min[:, 1], ut[imin % 21])


def test_cost_scale_and_stage0_bound(twin):
    """tau scales the stage terms only; the stage-0 s bound counts only with s0_bound."""
    B, N, M = 4, 5, 3
    x0 = config2_x0(B, 2)
    x0[:, 3] = 0.02                                      # s above uh_s = 0.011 at stage 0
    sid = np.arange(B) % 4
    yref = np.repeat(straight_traj()[None, :N], B, 0)
    ye = yref[:, N - 1, :4].copy()
    U = np.zeros((B, M, N, 2))
    U[..., 0] = 0.01
    c1, v1, x1 = R.rollout_cost(twin, x0, U, sid, yref, ye, tau=R.TS)
    c0, v0, x0e = R.rollout_cost(twin, x0, U, sid, yref, ye, tau=1.0)
    assert np.array_equal(x1, x0e)
    term = 0.5 * (R.WE * (x1 - ye[:, None]) ** 2).sum(-1)
    np.testing.assert_allclose((c0 - term) * R.TS, c1 - term, rtol=1e-9)
    assert np.all(v1 >= 0.02 - 0.011 - 1e-15)
    _, v2, _ = R.rollout_cost(twin, x0, U[:, :, :1], sid, yref[:, :1], ye, s0_bound=False)
    assert np.all(v2 == 0.0)                            # N = 1: only stage 0 exists, and its s is exempt


def test_colon_grid_matches_matlab():
    un, ut = R.colon_grid(0.0, 0.03), R.colon_grid(-0.05, 0.05)        # helper.m:380-381, default bounds
    assert len(un) == 7 and len(ut) == 21
    assert un[0] == 0.0 and ut[0] == -0.05
    assert un[-1] == 0.03 and ut[-1] == 0.05
    np.testing.assert_allclose(np.diff(un), 0.005, rtol=0, atol=1e-15)
    assert len(R.colon_grid(0.0, 0.0)) == 1
    assert len(R.colon_grid(0.0, 0.0049)) == 1          # the colon stops below ub


def test_first_min_rule():
    nan = np.nan
    s = np.array([[3.0, 1.0, 2.0, 1.0],      # tie: the first wins
                  [nan, 5.0, nan, 4.0],      # NaN never wins
                  [nan, nan, nan, nan],      # all NaN: (NaN, 0)
                  [np.inf, nan, np.inf, nan],  # Inf is an entry
                  [2.0, 2.0, 2.0, 2.0],
                  [nan, -0.0, 0.0, nan]])    # -0 == 0: the first
    c, i = R.first_min(s)
    assert list(i) == [1, 3, 0, 0, 0, 1]
    assert c[0] == 1.0 and c[1] == 4.0 and np.isnan(c[2]) and c[3] == np.inf and c[4] == 2.0 and c[5] == 0.0
    # (B, n_un, n_ut) surfaces are read in row-major linear order i n_ut + j
    c, i = R.first_min(s[:2].reshape(2, 2, 2))
    assert list(i) == [1, 3]
