"""GPU: contact modes and the open-loop simulation (qsp_eval_modes, qsp_get_modes, qsp_open_loop;
helper.m:132-193, PusherSliderModel.m:264-382, 587-589).

* against the numpy restatement (tests/open_loop_ref.py) within OPEN_LOOP_ATOL / MODE_CONE_RTOL, the
  restatement's own spread across the oracle's two formulations x 100 (tests/test_open_loop_ref.py); modes
  are compared where their margin to the cone's edges is at least 1e-9 (NEAR_EDGE);
* bit identities on the device (== on the raw doubles): the modes against qsp_eval_dynamics' Jacobian, the
  open loop against qsp_rollout_cost's Euler x_end, against itself under a plant delay, against
  qsp_eval_spline (clip, S_p) and qsp_eval_modes, independence of B, M, position, requested outputs and
  store path;
* the helper.py / model.py mirrors; the argument checks.

Shapes are the smallest that reach every path: M = 1, 3 (several lanes per workgroup), 65 (one lane per
workgroup), 300 (candidates looped over); B = 1, 5, 67; T = 1, 2, 20, 201 (no multiple of the store tiles
4 and 8, except 20 of 4); store_tile 1, 4, 8; four shapes mixed per lane; s negative and s > b."""
import ctypes as C

import numpy as np
import pytest

import open_loop_ref as R
from conftest import config2_x0, straight_traj
from test_open_loop_ref import DELAY, LAW_SEED, MODE_CONE_RTOL, NEAR_EDGE, OPEN_LOOP_ATOL

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
TS = R.TS
ALL = ("X", "U_out", "S_p", "mode", "mode_steps")


def _solver(B, N=20, **kw):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    shapes = [make_shape(n) for n in NAMES]
    s = OcpSolver(N=N, batch=B, **kw)
    s.set_shapes(shapes, shape_id=np.arange(B) % 4)
    return s, shapes


def _x0(B, seed, shapes):
    """config-2 x0; lane 0 has s > b, lane B // 2 has s < 0 (B >= 3)."""
    x0 = config2_x0(B, seed)
    if B >= 3:
        x0[0, 3] = shapes[0].b + 0.004
        x0[B // 2, 3] = -0.03
    return x0


@pytest.fixture(scope="module")
def dev():
    s, shapes = _solver(1)
    yield s, shapes
    s.close()


# ------------------------------------------------------------------ modes
@pytest.fixture(scope="module")
def law(oracle, dev):
    s, _ = dev
    x, u, sid = R.law_xu(20_000, LAW_SEED, oracle)
    mode, cone = s.eval_modes(x, u, shape_id=sid, want_cone=True)
    return x, u, sid, mode, cone


def test_eval_modes_against_restatement(oracle, law):
    x, u, sid, mode, cone = law
    rm, rc, margin = R.modes(oracle, x, u, sid)
    keep = margin >= NEAR_EDGE
    print(f"modes: {np.sum(~keep)} of {len(keep)} cases left out (margin < {NEAR_EDGE:g}); min margin {margin.min():.2e}")
    assert np.mean(~keep) <= 1e-3
    assert np.array_equal(mode[keep], rm[keep])
    rel = np.abs(cone[:, :2] - rc[:, :2]) / np.abs(rc[:, :2])
    print(f"cone: max rel gamma_l {rel[:, 0].max():.2e}, gamma_r {rel[:, 1].max():.2e}")
    assert rel.max() < MODE_CONE_RTOL
    assert np.array_equal(cone[:, 2], rc[:, 2])                            # u_t / u_n: one IEEE division


def test_mode_is_the_rule_on_the_returned_cone(law):
    _, _, _, mode, cone = law
    assert np.array_equal(mode, R.mode_rule(cone[:, 0], cone[:, 1], cone[:, 2]))
    assert set(np.unique(mode)) == {1, 2, 3}


def test_modes_are_the_branches_of_eval_dynamics(dev, law):
    s, _ = dev
    x, u, sid, mode, cone = law
    _, J = s.eval_dynamics(x, u, shape_id=sid)
    assert np.array_equal(J[:, 3, 5] == 1.0, np.isin(mode, (2, 3)))
    assert np.all((J[:, 3, 5] == 1.0) | (J[:, 3, 5] == 0.0))
    sl, sr = mode == 2, mode == 3
    assert sl.sum() > 1000 and sr.sum() > 1000
    assert np.array_equal(cone[sl, 0], -J[sl, 3, 4])
    assert np.array_equal(cone[sr, 1], -J[sr, 3, 4])


def test_modes_special_inputs(dev):
    s, shapes = dev
    for sid, sh in enumerate(shapes):
        for sv in (0.01, -0.02, sh.b + 0.01, -sh.b - 0.01, 2.5 * sh.b):
            x = np.tile([0.0, 0.0, 0.1, sv], (6, 1))
            u = np.array([[0.0, 0.0], [0.0, 0.02], [0.0, -0.02], [0.01, 0.0], [0.01, 0.05], [0.01, -0.05]])
            mode, cone = s.eval_modes(x, u, shape_id=sid, want_cone=True)
            # u = (0, 0): none; u_n = 0: an infinite ratio slides; u_n > 0: the rule on the cone (u_t = 0 sticks
            # only where the cone holds 0: on curved parts gamma_r > 0 or gamma_l < 0 occurs)
            assert mode[:3].tolist() == [0, 2, 3], (sid, sv, mode)
            assert np.array_equal(mode[3:], R.mode_rule(cone[3:, 0], cone[3:, 1], cone[3:, 2])) and np.all(mode[3:] > 0)
            assert np.all(cone[:, 0] > cone[:, 1])
            assert np.isnan(cone[0, 2]) and cone[1, 2] == np.inf and cone[2, 2] == -np.inf
            f, _ = s.eval_dynamics(x[:1], u[:1], shape_id=sid)
            assert np.all(f == 0.0)                                         # mode 0: f is 0
            # the cone wraps with s as the OCP model does: s and s + b see the same contact point
            m2, c2 = s.eval_modes(x + [0, 0, 0, sh.b], u, shape_id=sid, want_cone=True)
            assert np.array_equal(m2, mode)
            np.testing.assert_allclose(c2[:, :2], cone[:, :2], rtol=1e-9)
    xn = np.full((2, 4), np.nan)
    assert s.eval_modes(xn, [[0.01, 0.0], [0.0, 0.0]]).tolist() == [0, 0]
    assert s.eval_modes([0.0, 0.0, 0.0, 0.01], [np.nan, 0.01]).tolist() == [0]
    assert s.eval_modes([0.0, 0.0, 0.0, 0.01], [0.01, np.inf]).tolist() == [2]
    # theta does not enter the cone
    assert s.eval_modes([0.0, 0.0, np.nan, 0.01], [0.01, 0.0]).tolist() == s.eval_modes([0.0, 0.0, 0.1, 0.01], [0.01, 0.0]).tolist()


@pytest.mark.parametrize("N", [20, 50])
def test_get_modes_is_eval_modes_on_get_x_get_u(N):
    B = 5
    s, shapes = _solver(B, N, sqp_iters=4)
    sid = np.repeat(np.arange(B) % 4, N)
    x0 = _x0(B, 3, shapes)
    traj = straight_traj()
    try:
        s.set("constr_x0", x0)
        s.set("cost_y_ref", np.repeat(traj[None, :N], B, 0))
        s.set("cost_y_ref_e", traj[N - 1, :4])
        s.solve()
        after_solve = (s.get("x"), s.get("u"))
        s.set_reference_trajectory(traj)
        for step in range(2):
            if step:
                s.controller_solve(x0, 1)
                assert not np.array_equal(s.get("u"), after_solve[1])       # the shifted warm start now
            X, U = s.get("x"), s.get("u")
            mode, cone = s.get_modes(want_cone=True)
            em, ec = s.eval_modes(X[:, :N].reshape(-1, 4), U.reshape(-1, 2), shape_id=sid, want_cone=True)
            assert mode.shape == (B, N) and cone.shape == (B, N, 3)
            assert np.array_equal(mode.ravel(), em)
            assert np.array_equal(cone.reshape(-1, 3), ec, equal_nan=True)
            assert np.array_equal(s.get("modes"), mode) and np.array_equal(s.get("modes", 3), mode[:, 3])
            assert np.all(np.isin(mode, (0, 1, 2, 3)))
    finally:
        s.close()


# ------------------------------------------------------------------ open loop: bit identities
def _U(B, M, seed):
    return R.law_open_loop(B, M, seed)


def _eq(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_open_loop_is_rollout_costs_euler_chain():
    B, M, T = 5, 3, 20
    s, shapes = _solver(B)
    x0, U = _x0(B, 5, shapes), _U(B, M, 6)
    try:
        r = s.open_loop(x0, U, T, clip=False, want=ALL)
        assert np.array_equal(r["x_end"], r["X"][:, :, T])
        assert np.array_equal(r["X"][:, :, 0], np.repeat(x0[:, None], M, 1))
        assert np.array_equal(r["U_out"], np.repeat(U[:, :, None], T, 2))
        for t in (1, 2, 20):
            h, _ = _solver(B, t)
            try:
                xe = h.rollout_cost(x0, np.repeat(U[:, :, None], t, 2), integrator="euler", yref=np.zeros((B, t, 6)),
                                    yref_e=np.zeros((B, 4)), want_x_end=True)[1]
            finally:
                h.close()
            assert np.array_equal(r["X"][:, :, t], xe), t
    finally:
        s.close()


@pytest.mark.parametrize("D", [1, 7])
def test_plant_delay_shifts_the_trajectory(D):
    B, M, T = 5, 3, 20
    s, shapes = _solver(B)
    x0, U = _x0(B, 7, shapes), _U(B, M, 8)
    try:
        r0 = s.open_loop(x0, U, T, clip=False, want=ALL)
        rD = s.open_loop(x0, U, T, clip=False, plant_delay=(D - 0.5) * TS, want=ALL)    # ceil -> D columns
        assert np.array_equal(rD["X"][:, :, D:], r0["X"][:, :, :T + 1 - D])
        assert np.array_equal(rD["X"][:, :, :D], np.repeat(np.repeat(x0[:, None, None], M, 1), D, 2))
        assert np.all(rD["mode"][:, :, :D] == 0) and np.array_equal(rD["mode"][:, :, D:], r0["mode"][:, :, :T - D])
        assert np.array_equal(rD["mode_steps"][..., 0], r0["mode_steps"][..., 0] + D - (r0["mode"][:, :, T - D:] == 0).sum(2))
    finally:
        s.close()


@pytest.fixture(scope="module")
def clipped():
    """One clipped, delayed, noisy run with every output, B = 67, M = 3, T = 20, and its inputs."""
    B, M, T, D = 67, 3, 20, 3
    s, shapes = _solver(B)
    x0, U, noise = _x0(B, 9, shapes), _U(B, M, 10), R.draw_noise(T, B, 11)
    x0[1::2, 3] = np.abs(x0[1::2, 3]) + 0.002       # config 2 draws s <= 0.0011: half the lanes inside [0, b)
    r = s.open_loop(x0, U, T, noise=noise, plant_delay=(D - 0.5) * TS, want=ALL)
    yield s, shapes, x0, U, noise, r, (B, M, T, D)
    s.close()


def test_logged_state_includes_the_noise(clipped):
    s, shapes, x0, U, noise, r, (B, M, T, D) = clipped
    assert np.array_equal(r["X"][:, :, 0], np.repeat((x0 + noise[0])[:, None], M, 1))


def test_clip_and_contact_point_are_eval_splines(clipped):
    s, shapes, x0, U, noise, r, (B, M, T, D) = clipped
    sv = r["X"][:, :, :T, 3]
    sid = np.broadcast_to((np.arange(B) % 4)[:, None, None], sv.shape)
    b = np.array([sh.b for sh in shapes])[sid]
    inside = (sv >= 0) & (sv < b)
    assert 0.3 < inside.mean() < 0.7                                        # measured on the restatement: 0.52
    Cv, _, _, kap = s.eval_spline(sv.ravel(), shape_id=sid.ravel())
    with np.errstate(divide="ignore"):
        v = (1.0 / np.abs(kap)).reshape(sv.shape)
    ut = np.repeat(U[:, :, None, 1], T, 2)
    want = np.where(v < ut, v, ut)
    assert np.array_equal(r["U_out"][..., 1][inside], want[inside])
    assert np.array_equal(r["U_out"][..., 0], np.repeat(U[:, :, None, 0], T, 2))
    clipped_steps = (r["U_out"][..., 1] != ut)
    # the clip did act, inside [0, b) and outside (the restatement clips 169 and 185 of the 4 020 steps)
    assert (clipped_steps & inside).sum() > 50 and (clipped_steps & ~inside).sum() > 50
    assert np.all(r["U_out"][..., 1][ut < 0] == ut[ut < 0])                 # MATLAB's min: a negative u_t passes
    assert np.array_equal(r["S_p"][inside], Cv.reshape(sv.shape + (2,))[inside])
    # outside [0, b) the spline is evaluated at mod(s, b): the wrapped point, within rounding of the wrap
    Cw = s.eval_spline(np.mod(sv.ravel(), b.ravel()), shape_id=sid.ravel())[0].reshape(sv.shape + (2,))
    np.testing.assert_allclose(r["S_p"][~inside], Cw[~inside], rtol=0, atol=1e-12)


def test_modes_of_the_run_are_eval_modes_of_its_log(clipped):
    from uclv_qs_pushing_matlab_amd import helper
    s, shapes, x0, U, noise, r, (B, M, T, D) = clipped
    ua = helper.applied_inputs(r["U_out"], D)
    sid = np.broadcast_to((np.arange(B) % 4)[:, None, None], (B, M, T))
    em = s.eval_modes(r["X"][:, :, :T].reshape(-1, 4), ua.reshape(-1, 2), shape_id=sid.ravel())
    assert np.array_equal(r["mode"].ravel(), em)
    assert np.all(r["mode"][:, :, :D] == 0)
    counts = np.stack([(r["mode"] == k).sum(2) for k in range(4)], 2)
    assert np.array_equal(r["mode_steps"], counts) and np.all(counts.sum(2) == T)
    # helper.mode_trace: the same labels from a (B, T) trajectory and its commanded inputs
    mt = helper.mode_trace(s, r["X"][:, 1], r["U_out"][:, 1], plant_delay_cols=D)
    assert np.array_equal(mt, r["mode"][:, 1])


def test_replayed_constant_input_equals_held_input(clipped):
    s, shapes, x0, U, noise, r, (B, M, T, D) = clipped
    rr = s.open_loop(x0, np.repeat(U[:, :, None], T, 2), T, noise=noise, plant_delay=(D - 0.5) * TS, want=ALL)
    assert _eq(r, rr)
    # and a trajectory that does vary is replayed step by step: its first step is the held input's
    Uv = np.repeat(U[:, :, None], T, 2)
    Uv[:, :, 1:] *= 0.5
    rv = s.open_loop(x0, Uv, T, noise=noise, want=ALL)
    rh = s.open_loop(x0, U, T, noise=noise, want=ALL)
    assert np.array_equal(rv["X"][:, :, :2], rh["X"][:, :, :2]) and not np.array_equal(rv["X"][:, :, 2], rh["X"][:, :, 2])
    assert np.array_equal(rv["U_out"][:, :, 1:, 0], Uv[:, :, 1:, 0])


def test_results_do_not_depend_on_position_outputs_or_store_path(clipped):
    s, shapes, x0, U, noise, r, (B, M, T, D) = clipped
    kw = dict(noise=noise, plant_delay=(D - 0.5) * TS)
    # optional outputs set to NULL do not change the others; nor does the store path
    for want in ((), ("mode_steps",), ("X",), ("U_out", "mode"), ("S_p",)):
        for tile in (1, 4, 8):
            q = s.open_loop(x0, U, T, want=want, store_tile=tile, **kw)
            assert set(q) == set(want) | {"x_end"}
            assert all(np.array_equal(q[k], r[k]) for k in q), (want, tile)
    for tile in (1, 4, 8):
        assert _eq(s.open_loop(x0, U, T, want=ALL, store_tile=tile, **kw), r), tile
    # a lane alone (B = 1) equals the same lane inside B = 67
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    for lane in (0, 33, 66):
        one = OcpSolver(N=20, batch=1)
        try:
            one.set_shapes(shapes, shape_id=[lane % 4])
            for tile in (1, 8):
                q = one.open_loop(x0[lane], U[lane:lane + 1], T, noise=noise[:, lane:lane + 1], want=ALL, store_tile=tile,
                                  plant_delay=kw["plant_delay"])
                assert all(np.array_equal(q[k][0], r[k][lane]) for k in q), (lane, tile)
        finally:
            one.close()


@pytest.mark.parametrize("T", [1, 2, 21])
def test_a_candidate_is_the_same_at_any_M(T):
    """M = 1 alone, inside M = 3 (several lanes per workgroup), 65 (one lane per workgroup) and 300 (looped)."""
    B = 5
    s, shapes = _solver(B)
    x0, noise = _x0(B, 12, shapes), R.draw_noise(T, B, 13)
    U300 = _U(B, 300, 14)
    try:
        ref = {}
        for M in (300, 65, 3, 1):
            for tile in (1, 4, 8):
                q = s.open_loop(x0, U300[:, :M], T, noise=noise, plant_delay=0.06, want=ALL, store_tile=tile)
                if M == 300 and tile == 1:
                    ref = q
                assert all(np.array_equal(q[k], ref[k][:, :M]) for k in q), (M, tile)
        # the last candidate, alone
        q = s.open_loop(x0, U300[:, 299:], T, noise=noise, plant_delay=0.06, want=ALL)
        assert all(np.array_equal(q[k], ref[k][:, 299:]) for k in q)
    finally:
        s.close()


# ------------------------------------------------------------------ open loop: against the restatement
@pytest.mark.parametrize("B,M", [(67, 3), (5, 65)])
@pytest.mark.parametrize("delay", [0.0, DELAY])
@pytest.mark.parametrize("with_noise", [False, True])
def test_open_loop_against_restatement(oracle, B, M, delay, with_noise):
    T = 201
    s, shapes = _solver(B)
    x0, U = _x0(B, 15, shapes), _U(B, M, 16)
    noise = R.draw_noise(T, B, 17) if with_noise else None
    sid = np.arange(B) % 4
    try:
        r = s.open_loop(x0, U, T, noise=noise, plant_delay=delay, want=ALL)
        ref = R.open_loop(oracle, x0, U, sid, T, noise=noise, D=int(np.ceil(delay / TS)))
        for k in ("X", "U_out", "S_p", "x_end"):
            err = np.abs(r[k] - ref[k]).max()
            print(f"{k}: max abs diff {err:.2e} (max |ref| {np.abs(ref[k]).max():.3g})")
            assert err < OPEN_LOOP_ATOL, (k, err)
        steps = slice(None) if with_noise else slice(0, 20)
        margin = ref["margin"][:, :, steps]
        keep = ~(margin < NEAR_EDGE)                                        # NaN margin (mode 0): compared
        print(f"modes: {np.sum(~keep)} of {keep.size} steps left out (margin < {NEAR_EDGE:g})")
        assert np.mean(~keep) <= 0.01
        assert np.array_equal(r["mode"][:, :, steps][keep], ref["mode"][:, :, steps][keep])
        if with_noise:
            assert np.abs(r["mode_steps"] - ref["mode_steps"]).max() <= np.sum(~keep, axis=2).max()
        assert np.all(r["mode_steps"].sum(2) == T)
    finally:
        s.close()


@pytest.mark.parametrize("T", [1, 2])
def test_shortest_runs_against_restatement(oracle, T):
    B, M = 5, 3
    s, shapes = _solver(B)
    x0, U, noise = _x0(B, 18, shapes), _U(B, M, 19), R.draw_noise(T, B, 20)
    try:
        r = s.open_loop(x0, U, T, noise=noise, want=ALL)
        ref = R.open_loop(oracle, x0, U, np.arange(B) % 4, T, noise=noise)
        for k in ("X", "U_out", "S_p", "x_end"):
            assert r[k].shape == ref[k].shape
            assert np.abs(r[k] - ref[k]).max() < OPEN_LOOP_ATOL
        assert np.array_equal(r["mode"], ref["mode"]) and np.array_equal(r["mode_steps"], ref["mode_steps"])
    finally:
        s.close()


# ------------------------------------------------------------------ mirrors and errors
def test_helper_and_model_mirrors():
    from uclv_qs_pushing_matlab_amd import helper
    from uclv_qs_pushing_matlab_amd.model import PusherSliderModel
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    B, Ts, time_sim = 5, 0.05, 1.0
    plant = PusherSliderModel("plant", object_selection("santal"), object_name="santal", time_delay=0.12)
    s, shapes = _solver(B)
    try:
        s.set_shape_ids(np.zeros(B, np.int32))
        x0 = config2_x0(B, 21)
        u_n, u_t = np.linspace(0.0, 0.03, B), np.linspace(-0.05, 0.05, B)
        out = helper.open_loop_matlab(plant, x0, u_n, u_t, time_sim, Ts, sim_noise=True, seed=4, solver=s)
        T = 21
        assert len(out) == 8 and len(out[7]) == T and all(o.shape == (B, T) for o in out[:7])
        noise = np.random.default_rng(4).standard_normal((T, B, 4)) * R.NOISE_STD
        r = s.open_loop(x0, np.stack([u_n, u_t], 1)[:, None], T, noise=noise, plant_delay=0.12, want=ALL)
        X = r["X"][:, 0, :T]
        for got, want in zip(out[:7], (X[..., 0], X[..., 1], X[..., 2], r["S_p"][:, 0, :, 0], X[..., 3],
                                       r["U_out"][:, 0, :, 0], r["U_out"][:, 0, :, 1])):
            assert np.array_equal(got, want)
        # the one-lane default: the plant's own evaluator
        one = helper.open_loop_matlab(plant, x0[2], u_n[2], u_t[2], time_sim, Ts)
        r1 = s.open_loop(x0, np.stack([u_n, u_t], 1)[:, None], T, plant_delay=0.12, want=("X",))
        assert one[0].shape == (1, T) and np.array_equal(one[0][0], r1["X"][2, 0, :T, 0])
        # eval_model_variable_shape: x_dot of evalModelVariableShape and the mode as a string
        u = np.array([[0.0, 0.0], [0.01, 0.0], [0.01, 0.05], [0.01, -0.05], [0.0, 0.01]])
        xd, mode = plant.eval_model_variable_shape(x0, u)
        assert np.array_equal(xd, plant.evalModelVariableShape(x0, u))
        assert mode.tolist() == ["", "ST", "SL", "SR", "SL"] and np.all(xd[0] == 0)
        assert helper.convert_str2num(mode).tolist() == [0, 1, 2, 3, 2]
    finally:
        s.close()
        plant._ev.close()


def test_argument_checks_leave_the_handle_usable():
    from uclv_qs_pushing_matlab_amd import _lib
    B, M, T = 5, 3, 4
    s, shapes = _solver(B)
    L, h, p = s._L, s._h, _lib.ptr
    x0, U = config2_x0(B, 22), _U(B, M, 23)
    xe = np.zeros((B, M, 4))

    def opts(**kw):
        o = _lib.OpenLoopOpts()
        L.qsp_default_open_loop_opts(C.byref(o))
        o.n_steps, o.M = T, M
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    def run(o=None, x=x0, u=U, e=xe, handle=h):
        return L.qsp_open_loop(handle, o if o is not None else opts(), p(x), p(u), None, None, None, None, None, None, p(e))

    ARG = -1
    try:
        assert run() == 0
        first = xe.copy()
        bad = [run(handle=None), run(o=C.POINTER(_lib.OpenLoopOpts)()), run(x=None), run(u=None), run(e=None),
               run(o=opts(n_steps=0)), run(o=opts(M=0)), run(o=opts(M=-1)), run(o=opts(u_steps=2)), run(o=opts(u_steps=0)),
               run(o=opts(struct_size=8)), run(o=opts(clip=2)), run(o=opts(store_tile=3)), run(o=opts(Ts=-1.0)),
               run(o=opts(plant_delay=-0.1)), run(o=opts(plant_delay=1e9))]
        assert bad == [ARG] * len(bad), bad
        assert b"plant_delay" in L.qsp_last_error()
        io = _lib.OpenLoopIO()
        assert L.qsp_open_loop_device(h, opts(), C.byref(io), None) == ARG       # missing device pointers
        assert L.qsp_open_loop_device(h, opts(), None, None) == ARG
        md = np.zeros(4, np.int32)
        one = np.zeros(1, np.int32)
        assert L.qsp_eval_modes(h, 0, p(one), p(x0), p(U), p(md), None) == ARG
        assert L.qsp_eval_modes(h, 1, p(one), None, p(U), p(md), None) == ARG
        assert L.qsp_eval_modes(h, 1, p(np.array([4], np.int32)), p(x0), p(U), p(md), None) == ARG   # shape id out of range
        assert L.qsp_get_modes(h, None, None) == ARG and L.qsp_get_modes(None, p(md), None) == ARG
        with pytest.raises(ValueError):
            s.open_loop(x0, U[:, :, :1], T)
        with pytest.raises(KeyError):
            s.open_loop(x0, U, T, want=("Y",))
        assert run() == 0 and np.array_equal(xe, first)
    finally:
        s.close()


# ------------------------------------------------------------------ device entry equals host entry
@pytest.mark.parametrize("tile", [0, 1, 4, 8])
@pytest.mark.parametrize("M", [3, 65])
def test_open_loop_device_equals_host(M, tile):
    """B = 5, T = 9 (tiles of 4 and of 8 steps both end on a partial tile), M = 3 (several lanes per workgroup) and
    65 (one lane per workgroup); clip, a plant delay of two columns, noise, every output; device memory from torch."""
    import torch
    from uclv_qs_pushing_matlab_amd._lib import OpenLoopIO
    B, T = 5, 9
    s, shapes = _solver(B, N=4)
    x0, U = _x0(B, 41, shapes), _U(B, M, 42)
    noise = np.random.default_rng(43).normal(0.0, 1e-4, (T, B, 4))
    dev0 = torch.device("cuda", 0)
    try:
        host = s.open_loop(x0, U, T, noise=noise, plant_delay=2 * TS, clip=True, want=ALL, store_tile=tile)
        ins = dict(x0=x0, U=U, noise=noise)
        outs = {k: np.full_like(v, -7) for k, v in host.items()}                  # a value no output holds
        t = {k: torch.as_tensor(np.ascontiguousarray(v), device=dev0) for k, v in {**ins, **outs}.items()}
        io = OpenLoopIO()
        for k, v in t.items():
            setattr(io, k, v.data_ptr())
        torch.cuda.synchronize()                            # the tensors are filled before the handle's stream reads them
        s.open_loop_device(io, T, M, u_steps=1, plant_delay=2 * TS, clip=True, store_tile=tile)
        s.synchronize()
        assert set(host) == set(ALL) | {"x_end"}
        for k in host:
            assert np.array_equal(host[k], t[k].cpu().numpy()), k
    finally:
        s.close()
