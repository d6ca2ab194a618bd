"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Tolerances: building blocks are independent restatements of the same formulas
(span-based de Boor + hand-derived Jacobian on the GPU vs full-basis sum + forward
AD in the oracle), so they agree to rounding (rtol 1e-9).  The QP and the SQP are
compared on the same inputs; see DESIGN.md §5 for the chaotic-lane policy of the
end-to-end u0 check (BASELINE tolerance 1e-6).
"""
import numpy as np
import pytest

from conftest import config2_x0, straight_traj
from qp_data import build_qp

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")


@pytest.fixture(scope="module")
def gpu():
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=20, batch=64)
    s.set_shapes([make_shape(n) for n in NAMES])
    yield s
    s.close()


def _rand_states(rng, n, b):
    x = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-np.pi, np.pi, n),
                  rng.uniform(-1.5 * b, 1.5 * b, n)], 1)
    u = np.stack([rng.uniform(0.0, 0.03, n), rng.uniform(-0.05, 0.05, n)], 1)
    return x, u


def test_spline_matches_oracle(gpu, oracle):
    rng = np.random.default_rng(0)
    for sid, name in enumerate(NAMES):
        b = oracle.tab["params"][sid, 0]
        knots = oracle.tab["knots"][sid, :oracle.tab["n_ctrl"][sid] + 4]
        s = np.concatenate([rng.uniform(0, b, 500), knots, [b, np.nextafter(b, 0), 0.0, -0.0]])
        C, D, Dd, kap = gpu.eval_spline(s, sid)
        Co, dCo, Do, dDo, kapo = oracle.spline(s, sid)
        np.testing.assert_allclose(C, Co, rtol=1e-12, atol=1e-15, err_msg=name)
        np.testing.assert_allclose(D, Do, rtol=1e-11, atol=1e-13, err_msg=name)
        np.testing.assert_allclose(Dd, dDo, rtol=1e-9, atol=1e-9, err_msg=name)
        ok = np.isfinite(kapo)
        np.testing.assert_allclose(kap[ok], kapo[ok], rtol=1e-9, atol=1e-9, err_msg=name)
        # C(b) = 0 (every half-open indicator is false at the last knot)
        assert np.all(C[len(s) - 4] == 0.0)


def test_dynamics_matches_oracle(gpu, oracle):
    rng = np.random.default_rng(1)
    for sid, name in enumerate(NAMES):
        b = oracle.tab["params"][sid, 0]
        x, u = _rand_states(rng, 2000, b)
        u[:50] = 0.0                       # rho = 0/0: f = 0
        u[50:100, 0] = 0.0                 # rho = +-inf: pure sliding of the contact point
        f, J = gpu.eval_dynamics(x, u, sid)
        fo, Jo = oracle.dynamics(x, u, sid)
        np.testing.assert_allclose(f, fo, rtol=1e-10, atol=1e-14, err_msg=name)
        np.testing.assert_allclose(J, Jo, rtol=1e-8, atol=1e-10, err_msg=name)
        assert np.all(f[:50] == 0.0)


def test_rk4_matches_oracle(gpu, oracle):
    rng = np.random.default_rng(2)
    for sid, name in enumerate(NAMES):
        b = oracle.tab["params"][sid, 0]
        x, u = _rand_states(rng, 2000, b)
        xn, A, B = gpu.eval_rk4(x, u, 0.05, sid)
        xo, Ao, Bo = oracle.rk4(x, u, 0.05, sid)
        np.testing.assert_allclose(xn, xo, rtol=1e-11, atol=1e-14, err_msg=name)
        np.testing.assert_allclose(A, Ao, rtol=1e-8, atol=1e-10, err_msg=name)
        np.testing.assert_allclose(B, Bo, rtol=1e-8, atol=1e-10, err_msg=name)


def test_vbound_matches_oracle(gpu, oracle):
    from oracle.oracle import make_opts
    rng = np.random.default_rng(3)
    op = make_opts()
    for sid, name in enumerate(NAMES):
        b = oracle.tab["params"][sid, 0]
        s = rng.uniform(-2 * b, 2 * b, 1000)
        np.testing.assert_allclose(gpu.eval_vbound(s, sid), oracle.vbound(s, op, sid), rtol=1e-9, atol=1e-12,
                                   err_msg=name)


def _iterate(oracle, op, nb, seed, sqp_iters):
    x0 = config2_x0(nb, seed)
    traj = straight_traj()
    yref = np.repeat(traj[None, :op.N], nb, 0)
    yref_e = yref[:, op.N - 1, :4].copy()
    from oracle.oracle import make_opts
    op2 = make_opts(N=op.N, sqp_iters=sqp_iters)
    r = oracle.ocp_solve(op2, x0, yref, yref_e, X=np.repeat(x0[:, None], op.N + 1, 1))
    return x0, yref, yref_e, r["X"], r["U"]


def test_qp_matches_oracle(gpu, oracle):
    """Every QP that met the stop test on both sides agrees to 1e-7 (relative to the u range),
    except the ill-conditioned ones: the oracle's own solution moves by > 1e-8 when the gradient
    is perturbed by 1e-13 relative (u_t carries only tau W_u = 5e-5 of curvature: DESIGN.md
    section 2).  Status codes (0 stop test met, 2 cap, 3 infeasible) agree on every QP."""
    from oracle.oracle import make_opts
    op = make_opts(N=20)
    x0, yref, yref_e, X, U = _iterate(oracle, op, 64, 7, 3)
    A, B, b, H, g, lo, hi, act, dx0 = build_qp(oracle, op, X, U, yref, yref_e, x0)
    ref = oracle.qp(op, A, B, b, H, g, lo, hi, act, dx0)
    out = gpu.qp_solve(A, B, b, H, g, lo, hi, dx0)
    np.testing.assert_array_equal(out["qp_status"], ref["qp_status"])
    sens = np.zeros(len(x0), bool)
    for f in (1e-13, -1e-13):
        rp = oracle.qp(op, A, B, b, H, g * (1 + f), lo, hi, act, dx0)
        sens |= np.abs(rp["du"] - ref["du"]).max(axis=(1, 2)) > 1e-8
    scale_u = 0.05
    err = np.abs(out["du"] - ref["du"]).max(axis=(1, 2)) / scale_u
    conv = (ref["qp_status"] == 0) & (out["qp_status"] == 0)
    assert conv.mean() > 0.95
    assert sens.mean() < 0.2, sens.mean()
    assert np.median(err) < 1e-8, np.sort(err)[-5:]
    assert err[conv & ~sens].max() < 1e-7, np.sort(err[conv & ~sens])[-5:]


def test_ocp_solve_config2_parity(gpu, oracle):
    """acados-level solve from the controller's cold-start guess (X = x0, U = 0), K = 50."""
    from oracle.oracle import make_opts
    N, nb = 20, 64
    op = make_opts(N=N, sqp_iters=50)
    x0 = config2_x0(nb, 11)
    traj = straight_traj()
    yref = np.repeat(traj[None, :N], nb, 0)
    yref_e = yref[:, N - 1, :4].copy()
    X0 = np.repeat(x0[:, None], N + 1, 1)
    ref = oracle.ocp_solve(op, x0, yref, yref_e, X=X0)
    gpu.set_shape_ids(0)
    gpu.set("constr_x0", x0)
    gpu.set("cost_y_ref", yref)
    gpu.set("cost_y_ref_e", yref_e)
    gpu.set("init_x", X0)
    gpu.set("init_u", np.zeros((nb, N, 2)))
    gpu.solve()
    u0 = gpu.get_u0()
    assert np.all(gpu.get("status") == 0)
    # well-conditioned lanes: the oracle itself is insensitive to rounding-level perturbations of x0
    stable = np.ones(nb, bool)
    for pert in (lambda v: v * (1 + 1e-13), lambda v: v * (1 - 1e-13), lambda v: v + 1e-15):
        xp = pert(x0)
        ref_p = oracle.ocp_solve(op, xp, yref, yref_e, X=np.repeat(xp[:, None], N + 1, 1))
        stable &= (np.abs(ref_p["U"] - ref["U"]).max(axis=(1, 2)) < 1e-9) & \
                  (np.abs(ref_p["cost"] - ref["cost"]) <= 1e-9 * (1.0 + np.abs(ref["cost"])))
    # ... and converged: the full-step SQP sits on a fixed point (K-1 and K iterates agree);
    # lanes in a limit cycle return an arbitrary phase of it
    ref_m = oracle.ocp_solve(make_opts(N=N, sqp_iters=49), x0, yref, yref_e, X=X0)
    stable &= np.abs(ref_m["U"] - ref["U"]).max(axis=(1, 2)) < 1e-9
    d = np.abs(u0 - ref["U"][:, 0]).max(1)
    assert stable.mean() > 0.3
    assert d[stable].max() < 1e-6, (d[stable].max(), np.sort(d[stable])[-5:])
    np.testing.assert_allclose(gpu.get_cost()[stable], ref["cost"][stable], rtol=1e-6, atol=1e-12)


def test_controller_config1_parity(oracle):
    """NMPC_controller.solve semantics, config 1 (santal, x0 = 0, straight reference), 5 closed-loop steps."""
    from oracle.oracle import make_opts
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    N = 20
    s = OcpSolver(N=N, batch=1)
    s.set_shapes([make_shape("santal")])
    traj = straight_traj()
    s.set_reference_trajectory(traj)
    op = make_opts(N=N, sqp_iters=50)
    warm = oracle.new_warm(1, N)
    x = np.zeros((1, 4))
    for i in range(1, 6):
        u_gpu = s.controller_solve(x, i)
        r = oracle.controller_solve(op, x, traj, i, warm)
        assert np.abs(u_gpu - r["u0"]).max() < 1e-6, (i, u_gpu, r["u0"])
        f, _ = oracle.dynamics(x, r["u0"])
        x = x + 0.05 * f
    s.close()


def test_controller_config5_long_horizon(oracle):
    """BASELINE configs[4]: N = 50, curved x_finals reference (x, y, theta; s_ref = 0), a random
    start index per lane, mixed shapes, K = 50.  Full-step SQP converges on few lanes at this
    horizon, so u0 parity is checked on the converged, perturbation-stable ones."""
    import os
    from oracle.oracle import make_opts
    from uclv_qs_pushing_matlab_amd.objects import DATA_DIR, make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    N, nb, K = 50, 96, 50
    xf = np.load(os.path.join(DATA_DIR, "x_finals.npz"))
    traj = np.zeros((len(xf["x"]), 6))
    traj[:, 0], traj[:, 1], traj[:, 2] = xf["x"], xf["y"], xf["theta"]
    rng = np.random.default_rng(55)
    idx = rng.integers(1, len(traj) - N, nb).astype(np.int32)
    x0 = traj[idx - 1, :4] + np.stack([rng.uniform(-0.005, 0.005, nb), rng.uniform(-0.005, 0.005, nb),
                                       rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.03, 0.005, nb)], 1)
    sid = np.arange(nb) % 4
    s = OcpSolver(N=N, batch=nb, sqp_iters=K)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    s.set_reference_trajectory(traj)
    u = s.controller_solve(x0, idx)
    assert np.all(s.get("status") == 0)
    s.close()
    run = lambda x, k, **kw: oracle.controller_solve(make_opts(N=N, sqp_iters=k, **kw), x, traj, idx,  # noqa: E731
                                                     oracle.new_warm(nb, N), shape_id=sid)["u0"]
    ref = run(x0, K)
    stable = np.abs(run(x0, K - 1) - ref).max(1) < 1e-9
    for f in (1e-13, -1e-13, 3e-13):
        stable &= np.abs(run(x0 * (1 + f), K) - ref).max(1) < 1e-9
    # one more IPM iteration somewhere (stop test mu < 1e-10 met a rounding later) must not matter
    stable &= np.abs(run(x0, K, mu_stop=1.5e-10) - ref).max(1) < 1e-9
    assert stable.sum() >= 5, stable.sum()
    d = np.abs(u - ref).max(1)
    assert d[stable].max() < 1e-6, np.sort(d[stable])[-4:]


def test_decagon_spline_matches_oracle():
    """The reference's own spline test geometry (test_bspline_class.m) on the GPU."""
    from conftest import decagon_table
    from oracle.oracle import Oracle
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    tab, P, S, b = decagon_table()
    orc = Oracle(tab=tab)
    sh = _lib.Shape()
    sh.n_ctrl = len(P)
    for i in range(len(P)):
        sh.ctrl[i][0], sh.ctrl[i][1] = P[i]
    for i in range(len(S)):
        sh.knots[i] = S[i]
    sh.b, sh.c_ellipse, sh.mu_sp = b, 0.03, 0.2
    s = OcpSolver(N=10, batch=1)
    s.set_shapes([sh])
    q = np.concatenate([np.linspace(0, b, 1001), S])
    C, D, Dd, kap = s.eval_spline(q, 0)
    s.close()
    Co, _, Do, dDo, kapo = orc.spline(q, 0)
    np.testing.assert_allclose(C, Co, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(D, Do, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(Dd, dDo, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("N,S", [(1, 0), (2, 0), (5, 0), (5, 2), (20, 2), (31, 0), (63, 1), (64, 0), (90, 2),
                                 (126, 2), (127, 0)])
def test_horizon_and_layout_edges(oracle, N, S):
    """Odd/even horizons, padding slots (S = 2 with N + 1 odd), a group filling the whole
    wavefront (N = 63, S = 1), two stages per lane beyond it, up to the largest horizon the
    layout holds (N = 127: 64 lanes of two stages): GPU = oracle at K = 2."""
    from oracle.oracle import make_opts
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    nb, K = 13, 2
    x0 = config2_x0(nb, 100 + N)
    sid = np.arange(nb) % 4
    traj = straight_traj()
    s = OcpSolver(N=N, batch=nb, sqp_iters=K, stages_per_lane=S)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    s.set_reference_trajectory(traj)
    u = s.controller_solve(x0, 1)
    X = s.get("x")
    st = s.get("status")
    cap = s.get("qp_capped")
    s.close()
    w = oracle.new_warm(nb, N)
    r = oracle.controller_solve(make_opts(N=N, sqp_iters=K), x0, traj, 1, w, shape_id=sid)
    assert np.all(st == 0)
    np.testing.assert_array_equal(cap, r["qp_capped"])
    # a QP stopped by the iteration cap returns its last, unconverged iterate (as HPIPM at iter_max),
    # which moves with rounding (N = 126: one such lane, the oracle itself moves 1e-8 under 1e-13
    # input perturbations): held to 1e-5 there, 1e-9 on every other lane
    ok = cap == 0
    np.testing.assert_allclose(u[ok], r["u0"][ok], rtol=0, atol=1e-9)
    # the iterate's far stages of a 6 s horizon (N >= 126) are the loosest-determined part of the QP
    # solution: 4e-9 seen there, held to 1e-8
    np.testing.assert_allclose(X[ok], w["X"].reshape(nb, N + 1, 4)[ok], rtol=0, atol=1e-9 if N <= 90 else 1e-8)
    np.testing.assert_allclose(u[~ok], r["u0"][~ok], rtol=0, atol=1e-5)


MFMA = "matrix cores (v_mfma_f64_4x4x4_4b_f64)"


@pytest.mark.parametrize("N, kw, want", [
    (11, {}, "lane walk"),                                        # five instances per wave: no block each
    (12, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),          # four instances per wave
    (14, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),
    (15, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),
    (20, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),          # the headline
    (31, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),
    (50, {}, "matrix cores (v_mfma_f64_4x4x4_4b_f64)"),          # configs[4]: two stages per lane
    (50, {"factor_scan": True}, "associative scan"),
    (20, {"stages_per_lane": 2}, "lane walk"),                   # 11 lanes: five instances per wave
    # the edges of the rule (qsp_layout.h mfw_fits), one stage per lane ...
    (32, {"stages_per_lane": 1}, "lane walk"),                   # one instance per wave, N > 31
    (63, {"stages_per_lane": 1}, "lane walk"),
    # ... and two: four instances per wave from N = 24, the fullest regions at N = 30, 31, the last horizons
    (22, {"stages_per_lane": 2}, "lane walk"),
    (23, {"stages_per_lane": 2}, "lane walk"),
    (24, {"stages_per_lane": 2}, MFMA),
    (29, {"stages_per_lane": 2}, MFMA),
    (30, {"stages_per_lane": 2}, MFMA),
    (31, {"stages_per_lane": 2}, MFMA),
    (32, {"stages_per_lane": 2}, MFMA),
    (63, {"stages_per_lane": 2}, MFMA),
    (126, {"stages_per_lane": 2}, MFMA),
    (127, {"stages_per_lane": 2}, MFMA),
])
def test_library_reports_its_factor_walk(N, kw, want):
    """qsp_get_factor_walk (ABI 4) reports the walk the launchers take, so bench lines label runs by what
    ran (qsp_solver.hip factor_walk_kind), and the twin emulates that same walk for the same options
    (both read the rule from qsp_layout.h)."""
    from oracle.oracle import make_opts, tw_factor_walk
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=8, **kw)
    try:
        assert s.factor_walk() == want
        op = make_opts(N=N, stages_per_lane=kw.get("stages_per_lane", 0), factor_scan=int(kw.get("factor_scan", False)))
        assert OcpSolver.FACTOR_WALKS[tw_factor_walk(op)] == s.factor_walk()
    finally:
        s.close()


def test_lane_walk_switch_is_reported(monkeypatch):
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    monkeypatch.setenv("QSP_MFMA_WALK", "0")
    from oracle.oracle import make_opts, tw_factor_walk
    for N in (20, 50):
        s = OcpSolver(N=N, batch=8)
        try:
            assert s.factor_walk() == "lane walk"
            assert OcpSolver.FACTOR_WALKS[tw_factor_walk(make_opts(N=N))] == s.factor_walk()
        finally:
            s.close()
