"""GPU: rollout costs and the u0 cost landscape (qsp_rollout_cost, qsp_cost_landscape; helper.m:356-431).

* against the numpy restatement (tests/rollout_ref.py) within ROLLOUT_RTOL, the restatement's own spread
  across the oracle's two formulations x 100 (tests/test_rollout_ref.py).  numpy has no fused
  multiply-add, so that comparison is a tolerance, not bit identity;
* bit identities on the device (== on the raw doubles): landscape vs rollout_cost, independence of M, B,
  position and lane index, the RK4 and Euler steps against the building blocks that already hold them,
  MATLAB's min rule on the device's own surface, the NULL-surface call;
* U_tail = NULL is the solution before the controller's shift;
* optimality of the converged lanes of a 256-lane merit-SQP batch, on the device;
* the helper.py mirrors; the argument checks.

Shapes are the smallest that reach every path: M = 1, 3 (several lanes per workgroup), 65, 147 (one lane
per workgroup), 300 (candidates looped over); grids 1 x 1, 7 x 21, 40 x 30 (1 200 points: looped over);
B = 1, 5, 67; N = 1, 10, 20, 50; four shapes mixed per lane; s negative and s > b."""
import ctypes as C

import numpy as np
import pytest

import rollout_ref as R
from conftest import config2_x0, straight_traj
from test_rollout_ref import ROLLOUT_RTOL

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")


def _solver(B, N, **kw):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    shapes = [make_shape(n) for n in NAMES]
    s = OcpSolver(N=N, batch=B, **kw)
    s.set_shapes(shapes, shape_id=np.arange(B) % 4)
    return s, shapes


def _data(B, N, seed, shapes=None):
    """x0 (some s negative, one s > b), shape ids, references, for B lanes."""
    x0 = config2_x0(B, seed)
    sid = np.arange(B) % 4
    if shapes is not None:
        x0[0, 3] = shapes[0].b + 0.004          # s > b (lane 0: shape 0)
        x0[B // 2, 3] = -0.03                   # s < 0
    yref = np.repeat(straight_traj()[None, :N], B, 0)
    yref[:, :, 1] = 0.001 * np.arange(B)[:, None]      # lanes differ in their references
    return x0, sid, yref, yref[:, N - 1, :4].copy()


def _rand_U(rng, shape):
    return np.stack([rng.uniform(0.001, 0.03, shape), rng.uniform(-0.05, 0.05, shape)], -1)


def _close(got, ref, what):
    err = np.abs(got - ref)
    rel = (err / np.maximum(np.abs(ref), 1e-300)).max()
    print(f"{what}: max rel {rel:.2e}, max abs {err.max():.2e}")
    return rel, err.max()


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("B,M,N", [(67, 3, 20), (5, 65, 10), (1, 147, 50), (5, 1, 1), (5, 300, 10)])
def test_rollout_cost_against_restatement(oracle, B, M, N):
    s, shapes = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 11, shapes)
    U = _rand_U(np.random.default_rng(B * 1000 + M), (B, M, N))
    try:
        for integ in ("euler", "rk4"):
            for scale in (True, False):
                cost, viol, xe = s.rollout_cost(x0, U, integrator=integ, cost_scale=scale, yref=yref, yref_e=ye,
                                                want_viol=True, want_x_end=True)
                rc, rv, rx = R.rollout_cost(oracle, x0, U, sid, yref, ye, integrator=integ,
                                            tau=R.TS if scale else 1.0)
                rel, _ = _close(cost, rc, f"cost {integ} scale={scale}")
                assert rel < ROLLOUT_RTOL
                assert _close(viol, rv, "viol")[1] < ROLLOUT_RTOL
                assert _close(xe, rx, "x_end")[1] < ROLLOUT_RTOL
                assert np.array_equal(viol == 0, rv == 0)
    finally:
        s.close()


@pytest.mark.parametrize("B,N,grid", [(67, 20, (1, 1)), (5, 20, (7, 21)), (5, 10, (40, 30))])
def test_landscape_against_restatement(oracle, B, N, grid):
    s, shapes = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 12, shapes)
    tail = _rand_U(np.random.default_rng(7), (B, N))
    un = np.linspace(0.0, 0.03, grid[0]) if grid[0] > 1 else np.array([0.01])
    ut = np.linspace(-0.05, 0.05, grid[1]) if grid[1] > 1 else np.array([0.002])
    try:
        for integ in ("euler", "rk4"):
            for scale in (True, False):
                r = s.cost_landscape(x0, un, ut, U_tail=tail, integrator=integ, cost_scale=scale, yref=yref, yref_e=ye)
                surf = R.cost_landscape(oracle, x0, tail, un, ut, sid, yref, ye, integrator=integ,
                                        tau=R.TS if scale else 1.0)[0]
                assert r["cost"].shape == (B,) + grid
                assert _close(r["cost"], surf, f"surface {integ} scale={scale}")[0] < ROLLOUT_RTOL
    finally:
        s.close()


# ------------------------------------------------------------------ 2. bit identities on the device
@pytest.mark.parametrize("grid", [(1, 1), (7, 21), (40, 30)])
def test_landscape_equals_rollout_on_assembled_candidates(grid):
    B, N = 5, 20
    s, shapes = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 13, shapes)
    tail = _rand_U(np.random.default_rng(8), (B, N))
    un = np.linspace(0.0, 0.03, grid[0]) if grid[0] > 1 else np.array([0.01])
    ut = np.linspace(-0.05, 0.05, grid[1]) if grid[1] > 1 else np.array([0.002])
    cand = R.landscape_candidates(tail, un, ut)
    try:
        for integ in ("euler", "rk4"):
            r = s.cost_landscape(x0, un, ut, U_tail=tail, integrator=integ, yref=yref, yref_e=ye)
            c = s.rollout_cost(x0, cand, integrator=integ, yref=yref, yref_e=ye)
            assert np.array_equal(r["cost"].reshape(B, -1), c)
    finally:
        s.close()


def test_cost_independent_of_M_position_B_and_lane():
    N = 20
    s5, shapes = _solver(5, N)
    x0, sid, yref, ye = _data(5, N, 14, shapes)
    U = _rand_U(np.random.default_rng(9), (5, 65, N))
    try:
        for integ in ("euler", "rk4"):
            kw = dict(integrator=integ, yref=yref, yref_e=ye, want_viol=True, want_x_end=True)
            full = s5.rollout_cost(x0, U, **kw)
            one = s5.rollout_cost(x0, U[:, 17:18], **kw)                    # M = 1 alone
            three = s5.rollout_cost(x0, U[:, [40, 17, 3]], **kw)            # another position, M = 3
            for f, o, t in zip(full, one, three):
                assert np.array_equal(f[:, 17], o[:, 0]) and np.array_equal(f[:, 17], t[:, 1])
            # lane 3 of B = 5 as lane 43 of B = 67 (43 % 4 == 3: the same shape)
            s67, _ = _solver(67, N)
            try:
                x67, _, y67, e67 = _data(67, N, 15)
                U67 = _rand_U(np.random.default_rng(10), (67, 65, N))
                x67[43], y67[43], e67[43], U67[43] = x0[3], yref[3], ye[3], U[3]
                big = s67.rollout_cost(x67, U67, integrator=integ, yref=y67, yref_e=e67, want_viol=True, want_x_end=True)
                for f, b in zip(full, big):
                    assert np.array_equal(f[3], b[43])
            finally:
                s67.close()
    finally:
        s5.close()


def test_rk4_step_equals_eval_rk4():
    B, M = 5, 3
    s, shapes = _solver(B, 1)
    x0, sid, yref, ye = _data(B, 1, 16, shapes)
    U = _rand_U(np.random.default_rng(11), (B, M, 1))
    try:
        xe = s.rollout_cost(x0, U, integrator="rk4", yref=yref, yref_e=ye, want_x_end=True)[1]
        xn = s.eval_rk4(np.repeat(x0[:, None], M, 1), U[:, :, 0], shape_id=np.repeat(sid, M))[0]
        assert np.array_equal(xe.reshape(-1, 4), xn)
    finally:
        s.close()


def test_euler_rollout_equals_delay_buffer_sim():
    B, N = 5, 10
    s, shapes = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 17, shapes)
    U = _rand_U(np.random.default_rng(12), (B, 1, N))
    try:
        xe = s.rollout_cost(x0, U, integrator="euler", yref=yref, yref_e=ye, want_x_end=True)[1]
        s.set_delay_comp(N * s.Ts)
        assert s.delay_cols() == N
        for k in range(N):                       # the buffer applies the oldest input first: u_0 ... u_{N-1}
            s.delay_buffer_push(U[:, 0, k])
        assert np.array_equal(xe[:, 0], s.delay_buffer_sim(x0))
    finally:
        s.close()


def test_min_rule_on_the_device_surface():
    B, N = 5, 20
    s, shapes = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 18, shapes)
    tail = _rand_U(np.random.default_rng(13), (B, N))
    tail[2, 3, 0] = np.nan                       # lane 2: every entry of its surface is NaN
    grids = [(R.colon_grid(0.0, 0.03), R.colon_grid(-0.05, 0.05)),
             (np.array([0.02, 0.01, 0.01, 0.02, 0.01]), np.array([0.0, 0.03, 0.0, -0.03])),      # exact ties
             (np.array([0.02, np.nan, 0.01, 0.015]), np.array([np.nan, 0.01, 0.0, 0.01, 0.0])),  # NaN entries
             (np.linspace(0.0, 0.03, 40), np.linspace(-0.05, 0.05, 30))]
    try:
        for integ in ("euler", "rk4"):
            for un, ut in grids:
                r = s.cost_landscape(x0, un, ut, U_tail=tail, integrator=integ, yref=yref, yref_e=ye)
                cmin, imin = R.first_min(r["cost"])
                assert np.all(np.isnan(r["cost"][2])) and np.isnan(r["cost_min"][2]) and r["idx_min"][2] == 0
                ok = np.arange(B) != 2
                assert np.all(np.isfinite(r["cost_min"][ok]))
                assert np.array_equal(r["idx_min"], imin)
                assert np.array_equal(r["cost_min"][ok], cmin[ok])
                assert np.array_equal(r["u_min"][:, 0], un[imin // len(ut)], equal_nan=True)
                assert np.array_equal(r["u_min"][:, 1], ut[imin % len(ut)], equal_nan=True)
                q = s.cost_landscape(x0, un, ut, U_tail=tail, integrator=integ, yref=yref, yref_e=ye, want_surface=False)
                assert q["cost"] is None
                for k in ("u_min", "cost_min", "idx_min"):
                    assert np.array_equal(q[k], r[k], equal_nan=True), k
            # the tie grid really ties: its duplicate points hold equal costs, and the first one wins
            un, ut = grids[1]
            r = s.cost_landscape(x0, un, ut, U_tail=tail, integrator=integ, yref=yref, yref_e=ye)
            assert np.array_equal(r["cost"][ok, 1], r["cost"][ok, 2]) and np.array_equal(r["cost"][ok, :, 0], r["cost"][ok, :, 2])
            iu, it = r["idx_min"] // len(ut), r["idx_min"] % len(ut)
            assert not np.any(np.isin(iu[ok], [2, 3, 4])) and not np.any(it[ok] == 2)
    finally:
        s.close()


# ------------------------------------------------------------------ 3. U_tail = NULL
def test_null_tail_is_the_unshifted_solution():
    from uclv_qs_pushing_matlab_amd._lib import QspError
    B, N, K = 5, 20, 3
    traj = straight_traj()
    x0 = config2_x0(B, 19)
    x0[:, 3] = np.abs(x0[:, 3]) * 0.25           # s >= 0: the controller's pre-wrap leaves it bit for bit
    un, ut = R.colon_grid(0.0, 0.03), R.colon_grid(-0.05, 0.05)
    c, _ = _solver(B, N, sqp_iters=K)
    a, _ = _solver(B, N, sqp_iters=K)
    try:
        c.set_reference_trajectory(traj)
        with pytest.raises(QspError, match=r"\(-3\)"):          # QSP_ERR_STATE before any solve
            c.cost_landscape(x0, un, ut)
        c.controller_solve(x0, 1)
        U_shift = c.get("u")
        # the same problem at the acados level: the controller's cold start is u = (u_n_lb, 0) = 0, whose
        # Euler rollout stays at x0 (NMPC_controller.m:351-380); references index_time + k, k = 0..N-1
        yref = np.repeat(traj[None, :N], B, 0)
        a.set("constr_x0", x0)
        a.set("cost_y_ref", yref)
        a.set("cost_y_ref_e", yref[:, N - 1, :4])
        a.set("init_x", np.repeat(x0[:, None], N + 1, 1))
        a.set("init_u", np.zeros((B, N, 2)))
        a.solve()
        U = a.get("u")
        assert np.array_equal(U[:, 1:], U_shift[:, :N - 1]) and not np.array_equal(U, U_shift)
        for integ in ("euler", "rk4"):
            r0 = c.cost_landscape(x0, un, ut, integrator=integ)                     # NULL tail, staged references
            r1 = c.cost_landscape(x0, un, ut, U_tail=U, integrator=integ)
            r2 = c.cost_landscape(x0, un, ut, U_tail=U_shift, integrator=integ)
            assert np.array_equal(r0["cost"], r1["cost"]) and np.array_equal(r0["idx_min"], r1["idx_min"])
            assert not np.array_equal(r0["cost"], r2["cost"])
            # ... and the acados-level handle's own NULL tail and staged references give the same surface
            assert np.array_equal(a.cost_landscape(x0, un, ut, integrator=integ)["cost"], r0["cost"])
    finally:
        c.close()
        a.close()


# ------------------------------------------------------------------ 4. optimality on the device
def test_converged_lanes_are_grid_minima_on_the_device():
    """The criterion and constant of tests/test_gpu_optimality.py, every converged lane at once."""
    N, nb, K = 20, 256, 30
    x0 = config2_x0(nb, 21)
    yref = np.repeat(straight_traj()[None, :N], nb, 0)
    ye = yref[:, N - 1, :4].copy()
    s, _ = _solver(nb, N, sqp_iters=K, nlp_solver_type="SQP")
    try:
        s.set("constr_x0", x0)
        s.set("cost_y_ref", yref)
        s.set("cost_y_ref_e", ye)
        s.set("init_x", np.repeat(x0[:, None], N + 1, 1))
        s.set("init_u", np.zeros((nb, N, 2)))
        s.solve()
        U, status = s.get("u"), s.get("status")
        conv = status == 0
        assert conv.sum() >= 40, conv.sum()
        grid = np.linspace(-2e-4, 2e-4, 9)
        cand = np.repeat(U[:, None], 82, 1)                     # candidate 0: the solution itself
        cand[:, 1:, 0, 0] += np.repeat(grid, 9)
        cand[:, 1:, 0, 1] += np.tile(grid, 9)
        cost, viol = s.rollout_cost(x0, cand, integrator="rk4", cost_scale=True, want_viol=True)
        J0 = cost[:, :1]
        feas = viol[:, 1:] == 0
        gap = np.where(feas, (cost[:, 1:] - J0) / J0, np.inf)[conv]
        print(f"converged {conv.sum()} of {nb}; lanes with feasible grid points {(np.isfinite(gap).any(1)).sum()}; "
              f"feasible points {feas[conv].sum()}; worst relative gap {gap.min():.3e}; "
              f"solution's own viol max {viol[conv, 0].max():.2e}")
        dj = np.abs(s.get_cost()[conv] - cost[conv, 0]) / cost[conv, 0]
        print(f"solver objective vs the solution's rollout cost: max rel {dj.max():.2e} (defects <= tol_eq)")
        assert np.isfinite(gap).any(1).sum() >= 40
        assert gap.min() > -1e-9, gap.min()
    finally:
        s.close()


# ------------------------------------------------------------------ 5. mirrors
def test_helper_mirrors():
    from uclv_qs_pushing_matlab_amd import helper
    from uclv_qs_pushing_matlab_amd.controller import NMPCController
    from uclv_qs_pushing_matlab_amd.model import PusherSliderModel
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    B, Hp = 3, 20
    plant = PusherSliderModel("plant", object_selection("santal"), object_name="santal")
    ctrl = NMPCController("nmpc", plant, 0.05, Hp, batch=B)               # main.m's controller: 'SQP', max_iter 30
    ctrl.create_ocp_solver()
    x = config2_x0(B, 22)
    ctrl.initial_condition_update(x)
    y_ref = np.zeros((6, 201))
    y_ref[0] = 0.01 * np.arange(201) * 0.05
    ctrl.set_reference_trajectory(y_ref)
    ctrl.solve(x, 1)
    t = 1 * ctrl.sample_time                                              # helper.m:280
    u_min, cv, UN, UT = helper.debug_cost_function(x, ctrl.u_n_lb, ctrl.u_t_lb, ctrl.u_n_ub, ctrl.u_t_ub, ctrl, plant, 1, t)
    assert len(UN) == 7 and len(UT) == 21 and UN[-1] == ctrl.u_n_ub and UT[-1] == ctrl.u_t_ub
    assert cv.shape == (B, 21, 7) and np.all(np.isfinite(cv))             # cost_values(j, i): meshgrid layout
    # u_min is the first minimum of cost_values(:) (column-major) and lies on the grid
    flat = cv.transpose(0, 2, 1).reshape(B, -1)
    _, imin = R.first_min(flat)
    assert np.array_equal(u_min[:, 0], UN[imin // 21]) and np.array_equal(u_min[:, 1], UT[imin % 21])
    assert np.all(np.isin(u_min[:, 0], UN)) and np.all(np.isin(u_min[:, 1], UT))
    # the surface is half of evaluate_cost_function on the same candidates: the controller keeps the
    # solution shifted by one stage, so its columns 0..Hp-2 are the tail
    U_shift = ctrl.ocp_solver.get("u")
    for i, j in ((0, 0), (3, 10), (6, 20)):
        u_vect = np.concatenate([np.broadcast_to([UN[i], UT[j]], (B, 1, 2)), U_shift[:, :Hp - 1]], 1)
        c2 = helper.evaluate_cost_function(x, ctrl, plant, t, u_vect)
        assert np.array_equal(0.5 * c2, cv[:, j, i])
    # MATLAB's 2 x Hp layout for one lane's trajectory, broadcast over the lanes
    c_one = helper.evaluate_cost_function(x, ctrl, plant, t, u_vect[0].T)
    assert c_one[0] == c2[0]
    # the probe's references are one column later than the solve's (time_index + n, n = 1..Hp)
    yr, ye = helper._probe_refs(ctrl, t)
    assert np.array_equal(yr, y_ref[:, 1:Hp + 1].T) and np.array_equal(ye, y_ref[:4, Hp])
    assert np.array_equal(helper._probe_refs(ctrl, 199 * 0.05)[0][1:], np.repeat(y_ref[:, -1][None], Hp - 1, 0))
    ctrl.ocp_solver.close()


# ------------------------------------------------------------------ 6. errors
def test_argument_checks_leave_the_handle_usable():
    from uclv_qs_pushing_matlab_amd import _lib
    B, N, M = 5, 10, 3
    s, shapes = _solver(B, N, sqp_iters=3)
    f, shapes = _solver(B, N, sqp_iters=3)
    L, h = s._L, s._h
    x0, sid, yref, ye = _data(B, N, 23)
    U = _rand_U(np.random.default_rng(14), (B, M, N))
    un, ut = np.array([0.01, 0.02]), np.array([0.0, 0.01, 0.02])
    cost, umin, cmin = np.zeros((B, M)), np.zeros((B, 2)), np.zeros(B)
    p = _lib.ptr

    def opts(**kw):
        o = _lib.RolloutOpts()
        L.qsp_default_rollout_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    def roll(o=None, M_=M, x=x0, u=U, c=cost, handle=h):
        return L.qsp_rollout_cost(handle, o if o is not None else opts(), M_, p(x), p(u), p(yref), p(ye), p(c), None, None)

    def land(o=None, x=x0, tail=U[:, 0], n_un=2, g_un=un, n_ut=3, g_ut=ut, um=umin, cm=cmin):
        return L.qsp_cost_landscape(h, o if o is not None else opts(), p(x), p(np.ascontiguousarray(tail)), n_un, p(g_un),
                                    n_ut, p(g_ut), p(yref), p(ye), None, p(um), p(cm), None)

    ARG, STATE = -1, -3
    try:
        assert roll() == 0 and land() == 0
        bad = [roll(handle=None), roll(o=C.POINTER(_lib.RolloutOpts)()), roll(x=None), roll(u=None), roll(c=None),
               roll(M_=0), roll(M_=-2), roll(o=opts(integrator=2)), roll(o=opts(integrator=-1)),
               roll(o=opts(struct_size=8)), roll(o=opts(cost_scale=2)),
               land(o=C.POINTER(_lib.RolloutOpts)()), land(x=None), land(g_un=None), land(g_ut=None), land(um=None),
               land(cm=None), land(n_un=0), land(n_ut=0), land(o=opts(integrator=7)), land(o=opts(struct_size=0))]
        assert bad == [ARG] * len(bad), bad
        assert b"integrator" in L.qsp_last_error() or b"struct_size" in L.qsp_last_error()
        io = _lib.RolloutIO()
        assert L.qsp_rollout_cost_device(h, opts(), M, C.byref(io), None) == ARG        # missing device pointers
        assert L.qsp_rollout_cost_device(h, opts(), M, None, None) == ARG
        lio = _lib.LandscapeIO()
        assert L.qsp_cost_landscape_device(h, opts(), C.byref(lio), None) == ARG
        # NULL tail before any solve: a state error, not an argument error
        assert L.qsp_cost_landscape(h, opts(), p(x0), None, 2, p(un), 3, p(ut), p(yref), p(ye), None, p(umin), p(cmin),
                                    None) == STATE
        # the handle still solves as a fresh one does
        traj = straight_traj()
        for q in (s, f):
            q.set_reference_trajectory(traj)
        xs = config2_x0(B, 24)
        assert np.array_equal(s.controller_solve(xs, 1), f.controller_solve(xs, 1))
        assert np.array_equal(s.get("u"), f.get("u")) and np.array_equal(s.get_cost(), f.get_cost())
        assert roll() == 0 and land() == 0
    finally:
        s.close()
        f.close()


# ------------------------------------------------------------------ 7. device entries equal host entries
def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=torch.device("cuda", 0))


def _dev_out(shape, dtype=np.float64):
    return _dev(np.full(shape, -7, dtype))              # a value no output holds


def _rollout_device(s, M, integ, x0, U, yref, ye, sid=None, U_dev=None):
    """qsp_rollout_cost_device on torch tensors -> (cost, viol, x_end) as numpy."""
    import torch
    from uclv_qs_pushing_matlab_amd._lib import RolloutIO
    B = len(x0)
    ins = [_dev(x0), U_dev if U_dev is not None else _dev(U), _dev(yref), _dev(ye)]
    ids = None if sid is None else _dev(np.asarray(sid, np.int32))
    outs = [_dev_out((B, M)), _dev_out((B, M)), _dev_out((B, M, 4))]
    io = RolloutIO()
    io.x0, io.U, io.yref, io.yref_e = (t.data_ptr() for t in ins)
    io.shape_id = ids.data_ptr() if ids is not None else None
    io.cost, io.viol, io.x_end = (t.data_ptr() for t in outs)
    torch.cuda.synchronize()                            # the tensors are filled before the handle's stream reads them
    s.rollout_cost_device(io, M, integrator=integ)
    s.synchronize()
    return tuple(t.cpu().numpy() for t in outs)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("M", [3, 65])
def test_rollout_cost_device_equals_host(M, integ):
    """B = 5, N = 4: M = 3 (several lanes per workgroup) and 65 (one lane per workgroup); io.shape_id other than
    the handle's against a handle that holds those ids; U 8 bytes past a 16-byte boundary (scalar loads)."""
    import torch
    B, N = 5, 4
    s, shapes = _solver(B, N)
    s2, _ = _solver(B, N)
    x0, sid, yref, ye = _data(B, N, 31, shapes)
    U = _rand_U(np.random.default_rng(100 + M), (B, M, N))
    ids2 = (np.arange(B) + 1) % 4
    s2.set_shape_ids(ids2)
    kw = dict(integrator=integ, yref=yref, yref_e=ye, want_viol=True, want_x_end=True)
    try:
        host = s.rollout_cost(x0, U, **kw)
        dev = _rollout_device(s, M, integ, x0, U, yref, ye)
        for h, d in zip(host, dev):
            assert np.array_equal(h, d)
        host2 = s2.rollout_cost(x0, U, **kw)
        assert not np.array_equal(host2[0], host[0])                 # the other shapes give other costs
        for h, d in zip(host2, _rollout_device(s, M, integ, x0, U, yref, ye, sid=ids2)):
            assert np.array_equal(h, d)
        buf = torch.zeros(U.size + 1, dtype=torch.float64, device=torch.device("cuda", 0))
        assert buf.data_ptr() % 16 == 0
        Uo = buf[1:]
        Uo.copy_(_dev(U).reshape(-1))
        assert Uo.data_ptr() % 16 == 8
        for a, d in zip(dev, _rollout_device(s, M, integ, x0, U, yref, ye, U_dev=Uo)):
            assert np.array_equal(a, d)
    finally:
        s.close()
        s2.close()


@pytest.mark.parametrize("grid", [(3, 5), (9, 8)])
def test_cost_landscape_device_equals_host(grid):
    """B = 5, N = 4, grids of 15 and of 72 points (more than one wave); U_tail given, and NULL after a solve (the
    handle's iterate and staged references); the surface requested, and NULL."""
    import torch
    from uclv_qs_pushing_matlab_amd._lib import LandscapeIO
    B, N = 5, 4
    s, shapes = _solver(B, N, sqp_iters=3)
    x0, sid, yref, ye = _data(B, N, 32, shapes)
    tail = _rand_U(np.random.default_rng(33), (B, N))
    un, ut = np.linspace(0.0, 0.03, grid[0]), np.linspace(-0.05, 0.05, grid[1])
    try:
        s.set_reference_trajectory(straight_traj())
        s.controller_solve(config2_x0(B, 34), 1)
        for integ in ("euler", "rk4"):
            for given in (True, False):
                for surface in (True, False):
                    kw = dict(U_tail=tail, yref=yref, yref_e=ye) if given else {}
                    host = s.cost_landscape(x0, un, ut, integrator=integ, want_surface=surface, **kw)
                    ins = dict(x0=_dev(x0), un_grid=_dev(un), ut_grid=_dev(ut))
                    if given:
                        ins.update(U_tail=_dev(tail), yref=_dev(yref), yref_e=_dev(ye))
                    outs = dict(u_min=_dev_out((B, 2)), cost_min=_dev_out(B), idx_min=_dev_out(B, np.int32))
                    if surface:
                        outs["cost"] = _dev_out((B,) + grid)
                    io = LandscapeIO()
                    for k, t in {**ins, **outs}.items():
                        setattr(io, k, t.data_ptr())
                    io.n_un, io.n_ut = grid
                    torch.cuda.synchronize()
                    s.cost_landscape_device(io, integrator=integ)
                    s.synchronize()
                    assert host["cost"] is None if not surface else np.array_equal(host["cost"], outs["cost"].cpu().numpy())
                    for k in ("u_min", "cost_min", "idx_min"):
                        assert np.array_equal(host[k], outs[k].cpu().numpy()), (k, integ, given, surface)
    finally:
        s.close()
