"""GPU: a closed loop against a plant model of its own (qsp_set_plant_*, OcpSolver.set_plant) and the per-lane
closed-loop metrics computed on the device (qsp_closed_loop_metrics).

The reference simulates with `plant` and solves with `controller` (helper.m:195-322).  Here the closed loop is
rebuilt step by step from public calls -- noise, the delay prediction, controller_solve on handle A, the plant's
Euler step on a second handle P that holds the plant's shapes (open_loop with one step and no clip: x + Ts f by
the same fused multiply-add as the closed loop's plant step) -- and the device loop with A.set_plant(...) must
equal it.  Both sides run the same arithmetic, so every comparison is of every bit on every lane.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from closed_loop_metrics_ref import NAMES as METRIC_NAMES, closed_loop_metrics_ref
from conftest import config2_x0, straight_traj

pytestmark = pytest.mark.gpu

TS = 0.05
N, K = 20, 2
ERR_ARG, ERR_STATE = -1, -3


def shape(name, mu_scale=1.0, c_scale=1.0):
    """A named object's qsp_shape, optionally with mu_sp and c_ellipse scaled (a modified copy)."""
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    sh = _lib.Shape.from_buffer_copy(make_shape(name))
    sh.mu_sp = sh.mu_sp * mu_scale
    sh.c_ellipse = sh.c_ellipse * c_scale
    return sh


def controller_handle(B, traj=None, delay=0.0):
    """Handle A: santal on every lane, K = 2 full SQP steps, the config-1 reference."""
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    A = OcpSolver(N=N, batch=B, sqp_iters=K)
    A.set_shapes([shape("santal")])
    A.set_reference_trajectory(straight_traj() if traj is None else traj)
    if delay > 0.0:
        A.set_delay_comp(delay)
    return A


def plant_handle(B, shapes, shape_id=None):
    """Handle P: the plant's shapes on a one-stage handle of the same batch."""
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    P = OcpSolver(N=1, batch=B)
    P.set_shapes(list(shapes), shape_id=np.zeros(B, np.int32) if shape_id is None else shape_id)
    return P


def fma(a, b, c):
    """a * b + c rounded once, elementwise (math.fma where the interpreter has it, else exact rationals)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        x, y, z = float(a[i]), float(b[i]), float(c[i])
        if hasattr(math, "fma"):
            out[i] = math.fma(x, y, z)
        elif all(map(math.isfinite, (x, y, z))):
            out[i] = float(Fraction(x) * Fraction(y) + Fraction(z))
        else:
            out[i] = x * y + z
    return out


def mat_mod(a, b):
    """MATLAB's mod(a, b) as the library restates it (mat_mod, csrc/qsp_math.hpp)."""
    r = fma(-np.floor(a / b), b, a)
    return np.where(r == b, 0.0, r)


def plant_step(P, x, u):
    return P.open_loop(x, np.asarray(u)[:, None, :], 1, clip=False, want=())["x_end"][:, 0]


def harness(A, P, x0, T, noise=None, plant_delay=0.0, predict_with_P=False, dist=None):
    """The closed loop from public calls.  A: the controller's handle, with NO plant installed; P: the plant.
    predict_with_P: the delay prediction's Euler steps go through P from a host copy of the controller's input
    buffer (the plant differs from A's model); else A's own delay_buffer_sim / delay_buffer_push.
    dist: (t_dist, amplitude (B,), xwidth (B,), b (B,)) of the plant's shapes (helper.m:221-236)."""
    B = A.B
    D, Dp = A.delay_cols(), int(np.ceil(plant_delay / TS))
    A.controller_reset()                               # the closed loop's first solve is a cold start
    x = np.array(x0, np.float64)
    ubc = np.zeros((B, D, 2))                          # u_buff_contr, column 0 newest (zero after set_delay_comp)
    ubp = np.zeros((B, Dp, 2))                         # u_buff_plant
    X, Xs, U, ST = [], [], [], []
    for t in range(T):
        if dist is not None and t + 1 == dist[0]:
            _, amp, xw, b = dist
            x = x.copy()
            x[:, 1] = x[:, 1] + amp
            Cy = P.eval_spline(mat_mod(x[:, 3], b), P.shape_ids)[0][:, 1]
            sn = P.reproject_contact(-0.5 * xw, Cy - amp, 0.0, P.shape_ids)
            x[:, 3] = mat_mod(sn, b) - b * (sn < 0.0)                      # wrapped into [-b, b), helper.m:232
        if noise is not None:
            x = x + noise[t]
        X.append(x)
        if predict_with_P:
            xs = x
            for k in range(1, D + 1):                  # oldest (the last column) first
                xs = plant_step(P, xs, ubc[:, D - k])
        else:
            xs = A.delay_buffer_sim(x)
        Xs.append(xs)
        u = A.controller_solve(xs, 1 + t + D)
        ST.append(A.get("status"))
        U.append(u)
        if D > 0:
            ubc = np.concatenate([u[:, None], ubc[:, :-1]], 1)
            if not predict_with_P:
                A.delay_buffer_push(u)
        ua = u
        if Dp > 0:                                     # the plant applies the oldest column, then pushes u
            ua = ubp[:, -1]
            ubp = np.concatenate([u[:, None], ubp[:, :-1]], 1)
        x = plant_step(P, x, ua)
    X.append(x)
    return dict(X=np.stack(X, 1), Xsim=np.stack(Xs, 1), U=np.stack(U, 1), status=np.stack(ST, 1))


def assert_same(got, ref, what):
    for k in ("X", "Xsim", "U", "status"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what}: {k}")


def assert_moved(got, nominal):
    """The plant changed the loop: more than 1e-6 in X on some lane."""
    assert np.abs(got["X"] - nominal["X"]).max() > 1e-6


DELAYS = [(0.0, 0.0), (0.1, 0.1)]


@pytest.mark.parametrize("delay,plant_delay", DELAYS)
def test_harness_equals_the_loop(delay, plant_delay):
    """The harness itself: with P's shapes equal to A's it is A.closed_loop bit for bit (no plant installed;
    this holds without the feature and validates the harness)."""
    B, T = 16, 12
    x0 = config2_x0(B, 51)
    noise = np.random.default_rng(3).standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    A, P = controller_handle(B, delay=delay), plant_handle(B, [shape("santal")])
    r = A.closed_loop(x0, T, noise=noise, plant_delay=plant_delay)
    if delay > 0.0:
        A.set_delay_comp(delay)                        # the controller's buffer persists between runs: zero it
    h = harness(A, P, x0, T, noise=noise, plant_delay=plant_delay)
    assert_same(r, h, "nominal loop against the harness")
    if delay > 0.0:
        A.set_delay_comp(delay)
        h = harness(A, P, x0, T, noise=noise, plant_delay=plant_delay, predict_with_P=True)
        assert_same(r, h, "nominal loop against the harness predicting through P")
    A.close()
    P.close()


PLANTS = {"montana": lambda: shape("montana"), "santal_mu0.7_c1.2": lambda: shape("santal", 0.7, 1.2)}


@pytest.mark.parametrize("delay,plant_delay", DELAYS)
@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_mismatched_plant_equals_harness(plant, delay, plant_delay):
    """A holds santal, the plant is another object or santal with other constants: A.set_plant(...) and
    A.closed_loop equal the harness with P holding the plant, the prediction steps through P as well."""
    B, T = 16, 12
    x0 = config2_x0(B, 52)
    psh = PLANTS[plant]()
    A, P = controller_handle(B, delay=delay), plant_handle(B, [psh])
    nominal = A.closed_loop(x0, T, plant_delay=plant_delay)
    if delay > 0.0:
        A.set_delay_comp(delay)
    A.set_plant(shapes=[psh])
    r = A.closed_loop(x0, T, plant_delay=plant_delay)
    if delay > 0.0:
        # qsp_delay_buffer_sim follows the installed plant: the buffer the run left, through P
        ubc = r["U"][:, ::-1][:, :A.delay_cols()]
        xs = r["X"][:, -1]
        for k in range(1, A.delay_cols() + 1):
            xs = plant_step(P, xs, ubc[:, A.delay_cols() - k])
        np.testing.assert_array_equal(A.delay_buffer_sim(r["X"][:, -1]), xs)
        A.set_delay_comp(delay)
    A.clear_plant()
    h = harness(A, P, x0, T, plant_delay=plant_delay, predict_with_P=True)
    assert_same(r, h, f"plant {plant}")
    assert_moved(r, nominal)
    A.close()
    P.close()


def test_disturbance_is_reprojected_on_the_plant():
    """helper.m:221-236 with a plant of its own: the re-projection uses the plant's contour, xwidth and b."""
    B, T, td = 16, 10, 4
    x0 = config2_x0(B, 53)
    amp = np.linspace(-0.02, 0.02, B)
    psh = shape("montana")
    A, P = controller_handle(B), plant_handle(B, [psh])
    nominal = A.closed_loop(x0, T, disturbance=True, t_dist=td, amplitude=amp)
    A.set_plant(shapes=[psh])
    r = A.closed_loop(x0, T, disturbance=True, t_dist=td, amplitude=amp)
    A.clear_plant()
    h = harness(A, P, x0, T, dist=(td, amp, np.full(B, psh.xwidth), np.full(B, psh.b)))
    assert_same(r, h, "disturbed loop on the plant montana")
    assert_moved(r, nominal)
    assert np.all(np.abs(r["X"][:, td - 1, 3]) <= psh.b)       # wrapped into [-b, b)
    # santal's own re-projection gives another contact point: the plant's contour was used
    assert np.abs(r["X"][:, td - 1, 3] - nominal["X"][:, td - 1, 3]).max() > 1e-6
    A.close()
    P.close()


def test_overrides_equal_tables_and_clear_restores():
    """Three (mu, c) pairs over the lanes as three modified shapes in a plant table plus ids, and as per-lane
    overrides on the unmodified shape: bit-identical; clear_plant() gives the nominal loop back."""
    B, T = 18, 10
    x0 = config2_x0(B, 54)
    scales = [(0.7, 1.2), (1.3, 0.8), (1.0, 1.1)]
    ids = np.arange(B) % 3
    base = shape("santal")
    table = [shape("santal", m, c) for m, c in scales]
    A = controller_handle(B)
    nominal = A.closed_loop(x0, T)
    A.set_plant(shapes=table, shape_id=ids)
    r_table = A.closed_loop(x0, T)
    assert A.plant()["shape_id"].tolist() == ids.tolist()
    A.set_plant(mu_sp=np.array([t.mu_sp for t in table])[ids], c_ellipse=np.array([t.c_ellipse for t in table])[ids])
    p = A.plant()
    assert p["shapes"] is None and p["mu_sp"].shape == (B,)
    r_over = A.closed_loop(x0, T)
    assert_same(r_over, r_table, "overrides against the plant table")
    assert_moved(r_table, nominal)
    # the same through a plant table of the unmodified shape plus the overrides, and one constant at a time
    A.set_plant(shapes=[base], mu_sp=p["mu_sp"], c_ellipse=p["c_ellipse"])
    assert_same(A.closed_loop(x0, T), r_table, "overrides on a plant table")
    A.set_plant(shapes=[shape("santal", 1.0, c) for _, c in scales], shape_id=ids, mu_sp=p["mu_sp"])
    assert_same(A.closed_loop(x0, T), r_table, "mu_sp overridden, c_ellipse from the table")
    A.clear_plant()
    assert A.plant() is None
    assert_same(A.closed_loop(x0, T), nominal, "after clear_plant")
    A.close()


def test_twin_with_the_plants_dynamics():
    """The kernel-order twin as it is: its controller_solve on the controller's shape (warm start carried) and
    its dynamics on the plant's shape, the Euler step formed as an exactly rounded fused multiply-add on the
    host, against the device loop with the plant montana.  U, X and status bit for bit."""
    from oracle.oracle import Oracle, make_opts
    names = ("santal", "balea", "montana", "pulirapid")
    tw = Oracle(names, twin=True)
    B, T = 4, 6
    x0 = config2_x0(B, 55)
    traj = straight_traj()
    A = controller_handle(B)
    A.set_plant(shapes=[shape("montana")])
    r = A.closed_loop(x0, T)
    A.close()
    op = make_opts(N=N, sqp_iters=K)
    warm = tw.new_warm(B, N)
    x = x0.copy()
    X, U, ST = [x], [], []
    for t in range(T):
        ro = tw.controller_solve(op, x, traj, 1 + t, warm, shape_id=names.index("santal"))
        f, _ = tw.dynamics(x, ro["u0"], names.index("montana"))
        x = fma(TS, f, x)
        X.append(x)
        U.append(ro["u0"])
        ST.append(ro["status"])
    np.testing.assert_array_equal(r["U"], np.stack(U, 1))
    np.testing.assert_array_equal(r["X"], np.stack(X, 1))
    np.testing.assert_array_equal(r["status"], np.stack(ST, 1))


def per_lane_tables(B):
    """Short per-lane reference tables (9 columns) of different speeds."""
    t = np.arange(9) * TS
    traj = np.zeros((B, len(t), 6))
    traj[:, :, 0] = np.linspace(0.006, 0.014, B)[:, None] * t
    traj[:, :, 2] = np.linspace(-0.05, 0.05, B)[:, None] * t
    return traj


@pytest.mark.parametrize("per_lane", [False, True])
@pytest.mark.parametrize("with_plant", [False, True])
def test_metrics_equal_the_numpy_reference(with_plant, per_lane):
    """closed_loop_metrics against tests/closed_loop_metrics_ref.py on the same run's closed_loop outputs, the
    modes from P.eval_modes on helper.applied_inputs: bit for bit.  Nominal, and with a plant (a table entry
    plus per-lane overrides), a plant delay and a tightened s bound; on a shared and on per-lane reference tables
    of 9 columns, so that 12 steps from index0 = 1..3 run past the table's end and the clamp is exercised."""
    from uclv_qs_pushing_matlab_amd import helper
    B, T = 16, 12
    x0 = config2_x0(B, 56)
    index0 = 1 + np.arange(B) % 3
    noise = np.random.default_rng(4).standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    traj = per_lane_tables(B) if per_lane else straight_traj(T_end=0.4)
    assert traj.shape[-2] == 9
    plant_delay = 0.1 if with_plant else 0.0
    A = controller_handle(B, traj=None if per_lane else traj)
    if per_lane:
        A.set_reference_trajectories(traj)
    psh = shape("santal")
    if with_plant:
        # a tighter s bound than the start states' range: some lanes are outside it (and their solves fail)
        A.set("constr_lh", [-0.02, 0.0, -0.05])
        psh = shape("montana")
        mu = psh.mu_sp * np.linspace(0.6, 1.4, B)
        c = psh.c_ellipse * np.linspace(1.3, 0.7, B)
        A.set_plant(shapes=[psh], mu_sp=mu, c_ellipse=c)
    r = A.closed_loop(x0, T, index0=index0, noise=noise, plant_delay=plant_delay)
    m = A.closed_loop_metrics(x0, T, index0=index0, noise=noise, plant_delay=plant_delay)
    s_lo, s_hi = A._lh[0], A._uh[0]
    A.close()
    # P holds lane i's plant as shape i: the table entry with the lane's constants
    if with_plant:
        shapes = []
        for i in range(B):
            sh = shape("montana")
            sh.mu_sp, sh.c_ellipse = mu[i], c[i]
            shapes.append(sh)
        P = plant_handle(B, shapes, np.arange(B, dtype=np.int32))
    else:
        P = plant_handle(B, [psh])
    Dp = int(np.ceil(plant_delay / TS))
    ua = helper.applied_inputs(r["U"], Dp)
    modes = P.eval_modes(r["X"][:, :T].reshape(-1, 4), ua.reshape(-1, 2), shape_id=np.repeat(P.shape_ids, T)).reshape(B, T)
    P.close()
    ref = closed_loop_metrics_ref(r["X"], r["U"], r["status"], modes, traj, index0, s_lo, s_hi)
    for j, name in enumerate(METRIC_NAMES):
        np.testing.assert_array_equal(m["metrics"][:, j], ref[:, j], err_msg=name)
        np.testing.assert_array_equal(m[name], ref[:, j], err_msg=name)
    np.testing.assert_array_equal(m["x_end"], r["X"][:, -1])
    np.testing.assert_array_equal(m["status"], r["status"][:, -1])
    # not vacuous: errors accumulate and the modes are counted
    assert np.all(ref[:, 0] > 0) and np.all(ref[:, 1] <= ref[:, 0]) and ref[:, 6:9].sum() > 0
    assert np.all(ref[:, 6:9].sum(1) <= T)
    if with_plant:   # the delayed plant applies zeros first: mode 0 on those steps, counted nowhere
        assert np.all(ref[:, 6:9].sum(1) <= T - Dp)
        assert s_lo == -0.02 and 0 < ref[:, 9].sum() < B * T and ref[:, 5].sum() > 0


def test_errors_leave_the_handle_usable():
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    B, T = 8, 6
    x0 = config2_x0(B, 57)
    A = controller_handle(B)
    nominal = A.closed_loop(x0, T)
    L, h = A._L, A.handle
    good = np.full(B, 0.3)
    # an id outside the plant table
    with pytest.raises(_lib.QspError, match=rf"qsp_set_plant_shape_ids failed \({ERR_ARG}\)"):
        A.set_plant(shapes=[shape("montana")], shape_id=1)
    assert A.plant() is None                                   # what was installed before is back
    with pytest.raises(ValueError):
        A.set_plant(shape_id=0)                                # ids need a table
    assert L.qsp_set_plant_shape_ids(h, _lib.ptr(np.zeros(B, np.int32))) == ERR_STATE
    # overrides that are not finite and > 0
    for bad in (0.0, -0.2, np.nan, np.inf):
        v = good.copy()
        v[B - 1] = bad
        assert L.qsp_set_plant_params(h, _lib.ptr(v), None) == ERR_ARG
        assert L.qsp_set_plant_params(h, _lib.ptr(good), _lib.ptr(v)) == ERR_ARG
        with pytest.raises(_lib.QspError, match=rf"qsp_set_plant_params failed \({ERR_ARG}\)"):
            A.set_plant(mu_sp=v)
    hs, hp = C.c_int32(-1), C.c_int32(-1)
    assert L.qsp_get_plant(h, C.byref(hs), C.byref(hp)) == 0 and (hs.value, hp.value) == (0, 0)
    # metrics: NULL output, no reference table
    o = _lib.ClosedLoopOpts()
    idx = np.ones(B, np.int32)
    assert L.qsp_closed_loop_metrics(h, C.byref(o), _lib.ptr(x0), _lib.ptr(idx), T, None, None, None, None) == ERR_ARG
    S = OcpSolver(N=N, batch=B, sqp_iters=K)
    S.set_shapes([shape("santal")])
    with pytest.raises(_lib.QspError, match=rf"qsp_closed_loop_metrics failed \({ERR_STATE}\)"):
        S.closed_loop_metrics(x0, T)
    S.close()
    # the handle goes on as before; x_end and status alone may be left out
    assert_same(A.closed_loop(x0, T), nominal, "after the refused calls")
    m = np.zeros((B, 10))
    assert L.qsp_closed_loop_metrics(h, None, _lib.ptr(x0), _lib.ptr(idx), T, None, _lib.ptr(m), None, None) == 0
    np.testing.assert_array_equal(m, A.closed_loop_metrics(x0, T)["metrics"])
    hs, hp = C.c_int32(), C.c_int32()
    A.set_plant(shapes=[shape("montana"), shape("balea")], c_ellipse=good)
    assert L.qsp_get_plant(h, C.byref(hs), C.byref(hp)) == 0 and (hs.value, hp.value) == (2, 2)
    A.close()


def same_plant(p, q):
    if p is None or q is None:
        return p is None and q is None
    if (p["shapes"] is None) != (q["shapes"] is None):
        return False
    if p["shapes"] is not None and [bytes(a) for a in p["shapes"]] != [bytes(a) for a in q["shapes"]]:
        return False
    return all((p[k] is None and q[k] is None) or (p[k] is not None and q[k] is not None and np.array_equal(p[k], q[k]))
               for k in ("shape_id", "mu_sp", "c_ellipse"))


def test_helper_takes_a_foreign_plant():
    """helper.closed_loop_matlab(plant, controller, ...) with a plant that is not the controller's: the run of
    test_mismatched_plant_equals_harness through the mirror; the handle's plant is left as it was found, also
    when the call raises."""
    from uclv_qs_pushing_matlab_amd import helper
    from uclv_qs_pushing_matlab_amd._lib import QspError
    from uclv_qs_pushing_matlab_amd.controller import NMPCController
    from uclv_qs_pushing_matlab_amd.model import PusherSliderModel
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    B, time_sim = 8, 0.5
    own = PusherSliderModel("model", object_selection("santal"), 0.0, object_name="santal")
    foreign = PusherSliderModel("real_plant", object_selection("montana"), 0.05, object_name="montana")
    c = NMPCController("nmpc", own, TS, N, batch=B, nlp_solver_type="SQP_RTI", sqp_iters=K)
    c.create_ocp_solver()
    c.set_reference_trajectory(straight_traj().T)
    sv = c.ocp_solver
    x0 = config2_x0(B, 58)
    T = 11
    mu = foreign.shape.mu_sp * np.linspace(0.8, 1.2, B)

    def unpack(out):
        return np.stack([out[0], out[2], out[3]], 2), np.stack([out[6], out[7]], 2), out[10]

    for kw, plant_kw in (({}, {}), (dict(plant_mu_sp=mu, plant_c_ellipse=0.02), dict(mu_sp=mu, c_ellipse=0.02))):
        assert sv.plant() is None
        xyt, u, found = unpack(helper.closed_loop_matlab(foreign, c, x0, time_sim, **kw))
        assert sv.plant() is None
        met = helper.closed_loop_metrics(foreign, c, x0, time_sim, **kw)
        assert sv.plant() is None
        sv.set_plant(shapes=[foreign.shape], **plant_kw)
        r = sv.closed_loop(x0, T, plant_delay=foreign.time_delay)
        m = sv.closed_loop_metrics(x0, T, plant_delay=foreign.time_delay)
        sv.clear_plant()
        np.testing.assert_array_equal(xyt, r["X"][:, :T, :3])
        np.testing.assert_array_equal(u, r["U"])
        np.testing.assert_array_equal(found, r["status"] == 0)
        np.testing.assert_array_equal(met["metrics"], m["metrics"])
    # the controller's own plant object and no overrides: the nominal loop, nothing installed or removed
    nominal = sv.closed_loop(x0, T)
    xyt, u, _ = unpack(helper.closed_loop_matlab(own, c, x0, time_sim))
    np.testing.assert_array_equal(u, nominal["U"])
    assert np.abs(xyt - r["X"][:, :T, :3]).max() > 1e-6
    # overrides alone, on the controller's own plant
    xyt, u, _ = unpack(helper.closed_loop_matlab(own, c, x0, time_sim, plant_mu_sp=0.5 * own.shape.mu_sp))
    sv.set_plant(mu_sp=0.5 * own.shape.mu_sp)
    np.testing.assert_array_equal(u, sv.closed_loop(x0, T)["U"])
    # a plant installed before the call is there after it, also when the call raises
    sv.set_plant(shapes=[shape("balea")], shape_id=0, c_ellipse=np.linspace(0.01, 0.02, B))
    before = sv.plant()
    helper.closed_loop_matlab(foreign, c, x0, time_sim)
    assert same_plant(sv.plant(), before)
    with pytest.raises(QspError):
        helper.closed_loop_matlab(foreign, c, x0, time_sim, plant_mu_sp=-1.0)
    assert same_plant(sv.plant(), before)
    with pytest.raises(QspError):
        helper.closed_loop_metrics(own, c, x0, time_sim, plant_c_ellipse=np.nan)
    assert same_plant(sv.plant(), before)
    sv.close()
