"""Bit-exact GPU parity: the HIP library against the oracle's kernel-order twin (oracle/qsp_twin.cpp).

The library is built with -ffp-contract=off and writes every fused multiply-add out; the twin
runs the same reference path (PusherSliderModel.m:503-603, bspline_shape.m:40-152, the acados
SQP/HPIPM algorithms of NMPC_controller.m:270-300, the solve wrapper :329-423, helper.m:195-322)
on the CPU: the library's own lane arithmetic compiled for the host, inside a sequential
restatement of the kernels' orchestration.  Every operation involved is IEEE-exact
on both sides (scripts/ubench/fp_exact.hip), so the expected result is equality of every bit, on
every lane -- including the lanes where the fixed-K full-step SQP is chaotic, where
any rounding-level difference would show.  Tolerance: none (np.array_equal, NaN == NaN).
"""
import numpy as np
import pytest

from conftest import config2_x0, straight_traj
from qp_data import build_qp

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {i}: gpu {a[i]!r} twin {b[i]!r}")


@pytest.fixture(scope="module")
def twin():
    from oracle.oracle import Oracle
    return Oracle(NAMES, twin=True)


def solver(N, B, **kw):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=B, **kw)
    s.set_shapes([make_shape(n) for n in NAMES])
    return s


def test_building_blocks_bit_identical(twin):
    from oracle.oracle import make_opts
    s = solver(20, 64)
    rng = np.random.default_rng(11)
    n = 4000
    for sid in range(4):
        b = twin.tab["params"][sid, 0]
        knots = twin.tab["knots"][sid, :twin.tab["n_ctrl"][sid] + 4]
        sig = np.concatenate([rng.uniform(-0.1 * b, 1.1 * b, n), knots, [b, np.nextafter(b, 0), 0.0, -0.0]])
        for g, t, name in zip(s.eval_spline(sig, sid), twin.spline(sig, sid), ("C", "D", "Dd", "kappa")):
            same(g, t, f"spline {name} shape {sid}")
        x = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-7.0, 7.0, n),
                      rng.uniform(-1.5 * b, 1.5 * b, n)], 1)
        u = np.stack([rng.uniform(0.0, 0.03, n), rng.uniform(-0.05, 0.05, n)], 1)
        u[:40] = 0.0
        u[40:80, 0] = 0.0
        for g, t, name in zip(s.eval_dynamics(x, u, sid), twin.dynamics(x, u, sid), ("f", "J")):
            same(g, t, f"dynamics {name} shape {sid}")
        for g, t, name in zip(s.eval_rk4(x, u, 0.05, sid), twin.rk4(x, u, 0.05, sid), ("xn", "A", "B")):
            same(g, t, f"rk4 {name} shape {sid}")
        sv = rng.uniform(-2 * b, 2 * b, n)
        same(s.eval_vbound(sv, sid), twin.vbound(sv, make_opts(), sid), f"v_bound shape {sid}")
    s.close()


@pytest.mark.parametrize("N,S,scan", [(20, 1, 0), (20, 2, 0), (50, 2, 0), (20, 2, 1), (50, 2, 1)])
def test_qp_bit_identical(twin, N, S, scan):
    """qsp_qp_solve against the twin's QP on the OCP's Gauss-Newton QPs at perturbed iterates
    (both lane layouts: their recursions associate differently, and each must match its own; at two
    stages per lane also the factorisation as an associative scan, factor_scan)."""
    from oracle.oracle import make_opts
    rng = np.random.default_rng(5 + N + S)
    nb = 192
    op = make_opts(N=N, stages_per_lane=S, factor_scan=scan)
    x0 = config2_x0(nb, 17 + N)
    X = np.repeat(x0[:, None], N + 1, 1) + rng.normal(0, 2e-3, (nb, N + 1, 4))
    U = np.stack([rng.uniform(0, 0.03, (nb, N)), rng.uniform(-0.02, 0.02, (nb, N))], 2)
    traj = straight_traj()
    yref = np.broadcast_to(traj[None, :N], (nb, N, 6)).copy()
    sid = np.arange(nb) % 4
    A, B, b, H, g, lo, hi, act, dx0 = build_qp(twin, op, X, U, yref, yref[:, -1, :4], x0, sid)
    s = solver(N, nb, stages_per_lane=S, factor_scan=bool(scan))
    assert s.layout()[0] == S
    r = s.qp_solve(A.reshape(nb, N, 16), B.reshape(nb, N, 8), b, H, g, lo, hi, dx0)
    s.close()
    t = twin.qp(op, A.reshape(nb, N, 16), B.reshape(nb, N, 8), b, H, g, lo, hi, act, dx0)
    for k in ("dx", "du", "pi", "lam", "iters", "qp_status"):
        same(r[k], t[k], f"qp {k}")
    assert np.mean(t["qp_status"] == 0) > 0.9


def controller_pair(twin, N, B, x0, traj, sid, idx, K=50, steps=1, **kw):
    """Cold-start controller solves (then warm-started repeats) on the GPU and on the twin.  In
    nlp_mode 1 the KKT residuals of each lane's last test (get('residuals')) are compared too."""
    import ctypes as C
    from oracle.oracle import make_opts
    nlp = kw.pop("nlp_mode", 0)
    diag = np.zeros((B, 8))
    if nlp:
        twin.L.tw_set_kkt_diag(diag.ctypes.data_as(C.c_void_p))
    s = None
    try:
        s = solver(N, B, sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI", **kw)
        s.set_shape_ids(sid)
        s.set_reference_trajectory(traj)
        op = make_opts(N=N, sqp_iters=K, nlp_mode=nlp, qp_iters=kw.get("qp_iters", 20), qp_mu_max=kw.get("qp_mu_max", 1e100),
                       stages_per_lane=kw.get("stages_per_lane", 0), factor_scan=int(kw.get("factor_scan", False)))
        warm = twin.new_warm(B, N)
        for step in range(steps):
            u = s.controller_solve(x0, idx + step)
            r = twin.controller_solve(op, x0, traj, idx + step, warm, shape_id=sid)
            same(u, r["u0"], f"u0 (step {step})")
            for f in ("status", "sqp_iter", "qp_iter", "qp_capped", "qp_stalled"):
                same(s.get(f), r[{"sqp_iter": "iters"}.get(f, f)], f"{f} (step {step})")
            same(s.get("x"), warm["X"], f"warm X (step {step})")
            same(s.get("u"), warm["U"], f"warm U (step {step})")
            same(s.get("pi"), warm["PI"], f"warm PI (step {step})")
            same(s.get_cost(), r["cost"], f"cost (step {step})")
            if nlp:   # the twin records the stationarity residual by block (u, x, terminal): the device its max
                want = np.stack([diag[:, :3].max(1), diag[:, 3], diag[:, 4], diag[:, 5]], 1)
                same(s.get("residuals"), want, f"KKT residuals (step {step})")
                r["kkt"] = diag.copy()
    finally:
        # the twin writes through this process-global pointer on every later call: clear it on
        # every exit path, a failed assertion included
        if nlp:
            twin.L.tw_set_kkt_diag(None)
        if s is not None:
            s.close()
    return r


def test_configs1_full_batch_bit_identical(twin):
    """BASELINE configs[1] (B = 4 096 santal lanes, N = 20, K = 50): every lane, every output."""
    from bench import config1_inputs
    x0, traj, sid = config1_inputs(20)
    r = controller_pair(twin, 20, len(x0), x0, traj, sid, 1)
    assert np.mean(r["status"] == 0) > 0.99


def test_bench_workload_bit_identical(twin):
    """BASELINE configs[2] (the headline): all 65 536 lanes, 4 shapes mixed, K = 50, then one
    warm-started step (shifted warm start, y_ref from index 2)."""
    from bench import CONFIG2_BATCH, SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(CONFIG2_BATCH, 20, SEED)
    controller_pair(twin, 20, CONFIG2_BATCH, x0, traj, sid, 1, steps=2)


def test_configs4_bit_identical(twin):
    """BASELINE configs[4]: N = 50 (two stages per lane), B = 16 384, the curved x_finals reference
    with a random start index per lane."""
    from bench import SEED, config4_inputs
    x4, _, _, sid4, traj4, idx4 = config4_inputs(16384, 50, SEED)
    controller_pair(twin, 50, len(x4), x4, traj4, sid4, idx4)


def test_configs4_factor_scan_bit_identical(twin):
    """configs[4] with the S = 2 factorisation as an associative scan (qsp_options.factor_scan): the
    device's scan order, restated by the twin (factor_scan_s2), on the full batch."""
    from bench import SEED, config4_inputs
    x4, _, _, sid4, traj4, idx4 = config4_inputs(16384, 50, SEED)
    controller_pair(twin, 50, len(x4), x4, traj4, sid4, idx4, factor_scan=True)


def test_merit_sqp_bit_identical(twin):
    """The reference's own solver configuration (sqp + merit_backtracking, max_iter 30, tol 1e-6,
    NMPC_controller.m:271-276) on 4 096 configs[2] lanes: statuses, iteration counts, u0, the
    NLP multipliers; two controller steps (the second warm-started from the shifted solution)."""
    from bench import SEED, make_inputs
    # N = 12, 64 lanes: the shortest horizon at which the merit kernel, too, factorises on the matrix
    # cores (N = 12 .. 14 since the range was widened; four instances per wave)
    x12, _, _, sid12, traj12 = make_inputs(64, 12, SEED + 7)
    controller_pair(twin, 12, 64, x12, traj12, sid12, 1, K=30, steps=2, nlp_mode=1)
    x0, _, _, sid, traj = make_inputs(4096, 20, SEED + 7)
    r = controller_pair(twin, 20, 4096, x0, traj, sid, 1, K=30, steps=2, nlp_mode=1)
    # Measured on the twin (= the device, bit for bit): 1 010 of 4 096 lanes meet tol 1e-6 within 30
    # iterations at the second step (1 242 at the first; 1 004 and 1 243 with the lane walk), the rest end at max_iter (status 2).  Why the
    # reference's own SQP stalls on the others -- the iterate chatters across motion-cone boundaries,
    # where the dynamics' Jacobian jumps, and the merit line search ends at alpha_min, damping the
    # multiplier update; exact QP duals do not change it -- is DESIGN.md section 2's residual breakdown
    # (tests/test_merit_diagnosis.py pins it on the literal oracle).
    assert int(np.sum(r["status"] == 0)) == 1010
    # the count depends on the factorisation's rounding order (1 004 with the lane walk's): every lane
    # whose status the order decides sits outside the far stratum of the literal restatement -- on a
    # KKT/Armijo decision edge or rounding-chaotic under 1e-13 x0 probes (tests/merit_strata.py,
    # tests/test_merit_diagnosis.py::test_factor_order_flips_lie_outside_the_far_stratum)
    from merit_strata import classify_order_flips
    from oracle.oracle import Oracle, make_opts
    opl = make_opts(N=20, sqp_iters=30, nlp_mode=1, qp_iters=20, lane_walk=1)
    warm = twin.new_warm(4096, 20)
    lw = [twin.controller_solve(opl, x0, traj, 1 + k, warm, shape_id=sid)["status"] for k in range(2)]
    assert int(np.sum(lw[1] == 0)) == 1004
    flips = [(int(i), 1) for i in np.flatnonzero(lw[1] != r["status"])]
    cls = classify_order_flips(Oracle(NAMES), make_opts(N=20, sqp_iters=30, nlp_mode=1, qp_iters=20), x0, sid, traj,
                               flips)
    assert len(cls) == 8 and all(c["edge"] or c["chaotic"] for c in cls), cls
    assert set(np.unique(r["status"])) <= {0, 2}
    st2 = r["status"] == 2
    assert np.mean(r["kkt"][st2, :3].max(1) >= 1e-6) > 0.95   # stationarity fails on the status-2 lanes


def test_small_batch_fused_loop_bit_identical(twin):
    """B = 960 runs the whole SQP loop in one launch (sqp_loop_kernel); same bits as the twin."""
    from bench import SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(960, 20, SEED + 3)
    controller_pair(twin, 20, 960, x0, traj, sid, 1)


def test_acados_level_solve_bit_identical(twin):
    """qsp_solve ('constr_x0', 'cost_y_ref', 'init_x/u/pi', .solve()) in both NLP modes."""
    from oracle.oracle import make_opts
    N, B = 20, 512
    rng = np.random.default_rng(3)
    x0 = config2_x0(B, 99)
    traj = straight_traj()
    yref = np.broadcast_to(traj[None, 3:3 + N], (B, N, 6)).copy()
    ye = yref[:, -1, :4].copy()
    X = np.repeat(x0[:, None], N + 1, 1) + rng.normal(0, 1e-3, (B, N + 1, 4))
    U = np.stack([rng.uniform(0, 0.02, (B, N)), rng.uniform(-0.01, 0.01, (B, N))], 2)
    PI = rng.normal(0, 1e-3, (B, N, 4))
    sid = np.arange(B) % 4
    for nlp, K in ((0, 10), (1, 30)):
        s = solver(N, B, sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI")
        s.set_shape_ids(sid)
        s.set("constr_x0", x0)
        s.set("cost_y_ref", yref)
        s.set("cost_y_ref_e", ye)
        s.set("init_x", X)
        s.set("init_u", U)
        s.set("init_pi", PI)
        s.solve()
        r = twin.ocp_solve(make_opts(N=N, sqp_iters=K, nlp_mode=nlp), x0, yref, ye, X, U, PI, shape_id=sid)
        same(s.get("x"), r["X"], f"x (nlp {nlp})")
        same(s.get("u"), r["U"], f"u (nlp {nlp})")
        same(s.get("pi"), r["PI"], f"pi (nlp {nlp})")
        for f in ("status", "sqp_iter", "qp_iter", "qp_capped", "qp_stalled"):
            same(s.get(f), r[{"sqp_iter": "iters"}.get(f, f)], f"{f} (nlp {nlp})")
        same(s.get_cost(), r["cost"], f"cost (nlp {nlp})")
        s.close()


def test_closed_loop_bit_identical(twin):
    """helper.closed_loop_matlab on the device (sim_noise, controller delay compensation 0.1 s,
    plant delay 0.05 s, a disturbance with contact re-projection at step 6) against the twin."""
    from oracle.oracle import make_opts
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    N, B, T = 20, 256, 12
    x0 = config2_x0(B, 7)
    traj = straight_traj()
    sid = np.arange(B) % 4
    noise = np.random.default_rng(1).standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    amp = np.random.default_rng(2).uniform(-0.004, 0.004, B)
    s = solver(N, B, sqp_iters=5)
    s.set_shape_ids(sid)
    s.set_reference_trajectory(traj)
    s.set_delay_comp(0.1)
    D = s.delay_cols()
    g = s.closed_loop(x0, T, noise=noise, plant_delay=0.05, disturbance=True, t_dist=6, amplitude=amp)
    s.close()
    xw = np.array([object_selection(n)["xwidth"] for n in NAMES])
    t = twin.closed_loop(make_opts(N=N, sqp_iters=5), x0, traj, T, shape_id=sid, noise=noise, delay_cols=D,
                         plant_delay_cols=1, dist_step=6, dist_amp=amp, xwidth=xw)
    for k in ("X", "Xsim", "U", "status"):
        same(g[k], t[k], f"closed loop {k}")


@pytest.mark.parametrize("mu_max", [0.5, 1e6])
def test_qp_divergence_exit_bit_identical(twin, mu_max):
    """The QP-failure exit (mu >= qp_mu_max: status 4, the SQP stops with its last iterate) on the
    same lanes as the twin: at 0.5 (< mu0) every lane's first QP fails (sqp_iter 0, u0 = the warm-start
    rollout's), at 1e6 a mixture (about 1 % of these lanes' QPs reach it)."""
    from bench import SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(4096, 20, SEED + 11)
    r = controller_pair(twin, 20, 4096, x0, traj, sid, 1, qp_mu_max=mu_max)
    if mu_max < 1.0:
        assert np.all(r["status"] == 4) and np.all(r["iters"] == 0)
    else:
        assert 0 < np.sum(r["status"] == 4) < 200


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("N,S", [(1, 1), (2, 1), (2, 2), (11, 1), (12, 1), (14, 1), (15, 1), (21, 1), (31, 1), (32, 0), (32, 1), (63, 1),
                                 (63, 2), (100, 2), (127, 2)])
def test_horizons_and_layouts_bit_identical(twin, monkeypatch, N, S, fused):
    """Every lane layout the library accepts, at its edges: one stage per lane from N = 1 (32 instances
    per wave) to N = 63 (one instance filling the wave), two stages per lane up to N = 127; the auto
    choice at N = 32 (two stages per lane); the matrix-core factorisation's range 12 <= N <= 31 (four
    instances per wave at N = 12 ... 15, two from N = 21) and the lane walk just below it (N = 11); 97 lanes
    (a partly filled last wave), mixed shapes, both the per-iteration launches and the fused
    small-batch loop (QSP_FUSED_LOOP)."""
    from bench import SEED, make_inputs
    monkeypatch.setenv("QSP_FUSED_LOOP", fused)
    nb = 97
    x0, _, _, sid, traj = make_inputs(nb, N, SEED + N)
    controller_pair(twin, N, nb, x0, traj, sid, 1, K=8, stages_per_lane=S)


@pytest.mark.parametrize("N", [15, 20])
def test_lane_walk_switch_bit_identical(twin, monkeypatch, N):
    """The developer switch QSP_MFMA_WALK=0 (the lane walk where the matrix cores would factorise): the
    library reads it at qsp_create and the twin at every call, so both take the lane walk and stay
    equal bit for bit; merit SQP and fixed-K."""
    from bench import SEED, make_inputs
    monkeypatch.setenv("QSP_MFMA_WALK", "0")
    nb = 300
    x0, _, _, sid, traj = make_inputs(nb, N, SEED + 3 * N)
    controller_pair(twin, N, nb, x0, traj, sid, 1, K=10)
    controller_pair(twin, N, nb, x0, traj, sid, 1, K=10, steps=2, nlp_mode=1)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("N", [2, 3, 32, 63, 100, 127])
def test_factor_scan_horizons_bit_identical(twin, monkeypatch, N, fused):
    """The S = 2 factorisation scan at every lane count it meets (L = 2 ... 64, powers of two or not,
    the terminal stage in either slot), per-iteration launches and the fused small-batch loop."""
    from bench import SEED, make_inputs
    monkeypatch.setenv("QSP_FUSED_LOOP", fused)
    nb = 97
    x0, _, _, sid, traj = make_inputs(nb, N, SEED + N)
    controller_pair(twin, N, nb, x0, traj, sid, 1, K=8, stages_per_lane=2, factor_scan=True)


def test_main_m_controller_and_acados_qp_cap_bit_identical(twin):
    """main.m's own controller (Hp = 10, sqp + merit backtracking, max_iter 30, NMPC_controller.m:271-276)
    at acados' QP iteration cap (qp_solver_iter_max 50, as the MEX sets it), three controller steps; and
    the fixed-K workload at that cap."""
    from bench import SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(2048, 10, SEED + 10)
    controller_pair(twin, 10, 2048, x0, traj, sid, 1, K=30, steps=3, nlp_mode=1, qp_iters=50)
    x0, _, _, sid, traj = make_inputs(2048, 20, SEED + 20)
    controller_pair(twin, 20, 2048, x0, traj, sid, 1, qp_iters=50)


def test_non_default_parameters_bit_identical(twin):
    """Every tunable of the OCP and the solver away from its default (NMPC_controller.m
    update_cost_function :153-164, update_constraints :122-142, the ctor's v_alpha / d_v_bound /
    t_angle0 :98-100 and input bounds :23-26, Ts, the stage-cost scaling, the IPM's parameters), two
    controller steps: the device and the twin read them the same way."""
    from oracle.oracle import make_opts
    from bench import SEED, make_inputs
    N, nb, K = 16, 1024, 12
    W = np.array([2.0, 0.5, 3e-3, 1e-4, 2e-3, 5e-4])
    We = np.array([1e5, 3e5, 10.0, 1.0])
    lh, uh = np.array([-0.05, 0.0, -0.04]), np.array([0.02, 0.025, 0.04])
    ctrl = dict(v_alpha=0.8, d_v=0.001, t_angle0=2.5, u_n_lb=0.001, u_t_ub=0.04)
    ipm = dict(mu0=0.5, t_min=2e-2, frac=0.99, sigma_min=0.05, mu_stop=1e-9, res_stop=1e-9, qp_tol_stat=1e-9,
               qp_tol_eq=1e-9, qp_stall_iters=4, qp_stall_alpha=5e-4)
    x0, _, _, sid, traj = make_inputs(nb, N, SEED + 99)
    x0[:, 3] = np.clip(x0[:, 3], lh[0] + 1e-3, uh[0] - 1e-3)
    s = solver(N, nb, sqp_iters=K, qp_iters=25, Ts=0.04, cost_scale_Ts=False, stage0_s_bound=False, **ipm)
    s.set_shape_ids(sid)
    s.set("cost_W", np.diag(W))
    s.set("cost_W", np.diag(We), stage=N)
    s.set("constr_lh", lh)
    s.set("constr_uh", uh)
    s.set_ctrl_params(ctrl["v_alpha"], ctrl["d_v"], ctrl["t_angle0"], ctrl["u_n_lb"], ctrl["u_t_ub"])
    s.set_reference_trajectory(traj)
    op = make_opts(N=N, sqp_iters=K, qp_iters=25, Ts=0.04, tau=1.0, W=tuple(W), We=tuple(We), lh=tuple(lh),
                   uh=tuple(uh), stage0_s_bound=0, **ctrl, **ipm)
    warm = twin.new_warm(nb, N)
    for step in range(2):
        u = s.controller_solve(x0, 1 + step)
        r = twin.controller_solve(op, x0, traj, 1 + step, warm, shape_id=sid)
        same(u, r["u0"], f"u0 (step {step})")
        for f in ("status", "sqp_iter", "qp_iter", "qp_capped", "qp_stalled"):
            same(s.get(f), r[{"sqp_iter": "iters"}.get(f, f)], f"{f} (step {step})")
        same(s.get("x"), warm["X"], f"warm X (step {step})")
        same(s.get_cost(), r["cost"], f"cost (step {step})")
    s.close()
    assert np.mean(r["status"] == 0) > 0.9


@pytest.mark.parametrize("N,nlp,delay,plant_delay,t_dist", [
    (10, 1, 0.0, 0.0, 0),        # main.m as it runs (Hp = 10, merit SQP, no delay, t_dist past the end)
    (10, 1, 0.35, 0.35, 4),      # main.m's delayed variant (p.set_delay(0.35), set_delay_comp(0.35), main.m:75-76)
    (20, 0, 0.2, 0.0, 9),        # controller-side compensation only
    (50, 0, 0.0, 0.15, 5),       # two stages per lane in the loop, plant delay only
])
def test_closed_loop_variants_bit_identical(twin, N, nlp, delay, plant_delay, t_dist):
    """helper.closed_loop_matlab variants (helper.m:195-322): both NLP modes, controller and plant delay
    buffers of several lengths, the disturbance at several steps, two layouts; every state, input and
    status of every step against the twin."""
    from oracle.oracle import make_opts
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    B, T = 192, 14
    K = 30 if nlp else 4
    x0 = config2_x0(B, 70 + N)
    traj = straight_traj()
    sid = np.arange(B) % 4
    amp = np.random.default_rng(N).uniform(-0.004, 0.004, B)
    s = solver(N, B, sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI", qp_iters=50 if nlp else 20)
    s.set_shape_ids(sid)
    s.set_reference_trajectory(traj)
    s.set_delay_comp(delay)
    D = s.delay_cols()
    g = s.closed_loop(x0, T, plant_delay=plant_delay, disturbance=t_dist > 0, t_dist=t_dist, amplitude=amp)
    s.close()
    Dp = int(np.ceil(plant_delay / 0.05))   # delay_buff_plant as the library forms it (helper.m:211)
    xw = np.array([object_selection(n)["xwidth"] for n in NAMES])
    t = twin.closed_loop(make_opts(N=N, sqp_iters=K, nlp_mode=nlp, qp_iters=50 if nlp else 20), x0, traj, T, shape_id=sid,
                         delay_cols=D, plant_delay_cols=Dp, dist_step=t_dist, dist_amp=amp, xwidth=xw)
    for k in ("X", "Xsim", "U", "status"):
        same(g[k], t[k], f"closed loop {k}")


def test_closed_loops_back_to_back_keep_the_controller_buffer(twin):
    """qsp_closed_loop_ex keeps the controller's input buffer u_buff_contr across calls (it belongs to
    the controller object, NMPC_controller.m:109, and persists across helper.closed_loop_matlab runs);
    only set_delay_comp zeroes it.  A second closed loop on the same handle therefore equals the twin's
    closed loop started from the buffer the first one left (its last D inputs, newest first), bit for
    bit -- and differs from a run with a zeroed buffer."""
    from oracle.oracle import make_opts
    N, B, T, K = 10, 128, 8, 3
    x0 = config2_x0(B, 515)
    traj = straight_traj()
    sid = np.arange(B) % 4
    s = solver(N, B, sqp_iters=K)
    s.set_shape_ids(sid)
    s.set_reference_trajectory(traj)
    s.set_delay_comp(0.15)
    D = s.delay_cols()
    assert D == 3
    g1 = s.closed_loop(x0, T)
    g2 = s.closed_loop(x0, T)                     # same handle, no set_delay_comp in between
    s.close()
    op = make_opts(N=N, sqp_iters=K)
    t1 = twin.closed_loop(op, x0, traj, T, shape_id=sid, delay_cols=D)
    same(g1["U"], t1["U"], "first loop U")
    ub = np.ascontiguousarray(g1["U"][:, ::-1][:, :D])   # u_buff_contr after the first loop: newest first
    t2 = twin.closed_loop(op, x0, traj, T, shape_id=sid, delay_cols=D, ubc0=ub)
    for k in ("X", "U", "status"):
        same(g2[k], t2[k], f"second loop {k}")
    assert np.abs(g2["U"] - g1["U"]).max() > 1e-6    # the carried buffer changed the second loop
