"""GPU: the handle's named device buffers (qsp_capi.hip's Dev<T> members) across regrowth and across handles.

Regrowth: on one handle (B = 5, N = 10, sqp_iters = 3) the calls whose buffers are sized by an argument run with
that argument first growing, then shrinking -- the closed loop's logs, the reference table, the delay buffers,
the plant's own model, the open loop's delay ring -- and each result must equal, bit for bit, the same call on
a fresh handle.  (tests/test_gpu_staging.py does this for the staging pool; these are the buffers beside it.)

Lifecycle: a handle is created, runs every entry that allocates lazily (those calls and test_gpu_staging's ten)
and is closed, eight rounds in one process; every round's outputs must equal round one's bit for bit.  Nothing
here reads the device's free memory: other jobs share the card."""
import ctypes as C

import numpy as np
import pytest

from conftest import config2_x0, straight_traj
from test_gpu_staging import _calls as staging_calls

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
B, TS = 5, 0.05


def _handle(N=10, nlp="SQP_RTI"):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=B, sqp_iters=3, nlp_solver_type=nlp)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=np.arange(B) % 4)
    s.set_reference_trajectory(straight_traj())
    return s


def _closed_loop_no_xsim(s, x0, n, noise, plant_delay):
    """qsp_closed_loop_ex with X_sim = NULL (OcpSolver.closed_loop always asks for it)."""
    from uclv_qs_pushing_matlab_amd import _lib
    x0, idx, nz = _lib.f64(x0), _lib.i32(np.ones(B)), _lib.f64(noise)
    X, U, st = np.zeros((B, n + 1, 4)), np.zeros((B, n, 2)), np.zeros((B, n), np.int32)
    o = _lib.ClosedLoopOpts()
    o.plant_delay = plant_delay
    _lib.check(s._L.qsp_closed_loop_ex(s.handle, C.byref(o), _lib.ptr(x0), _lib.ptr(idx), n, _lib.ptr(nz), _lib.ptr(X),
                                       None, _lib.ptr(U), _lib.ptr(st)), "qsp_closed_loop_ex")
    return X, U, st


def _calls():
    """[(name, f(handle) -> tuple of arrays)] with fixed inputs, in the order grow, then shrink.  Every call
    installs what it depends on (reference table, delay columns, plant) and leaves the handle as _handle() made it."""
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    rng = np.random.default_rng(61)
    x0 = config2_x0(B, 62)
    ref = straight_traj()
    noise = rng.normal(0.0, 1e-4, (7, B, 4))

    def u(*shape):
        return np.stack([rng.uniform(0.001, 0.03, shape), rng.uniform(-0.05, 0.05, shape)], -1)

    def closed_loop(n, xsim):
        def f(s):
            if xsim:
                r = s.closed_loop(x0, n, noise=noise[:n], plant_delay=TS)
                return tuple(r[k] for k in sorted(r))
            return _closed_loop_no_xsim(s, x0, n, noise[:n], TS)
        return f"closed_loop n={n} xsim={xsim}", f

    def metrics(s):
        r = s.closed_loop_metrics(x0, 4, noise=noise[:4], plant_delay=2 * TS)
        return r["metrics"], r["x_end"], r["status"]

    def solve_on(s):
        """The installed table as the device holds it, and one cold controller step on it."""
        s.controller_reset()
        u0 = s.controller_solve(x0, 2)
        out = (s.get_reference_trajectories(), u0, s.get("status"))
        s.set_reference_trajectory(ref)
        return out

    def shared_table(T):
        def f(s):
            s.set_reference_trajectory(ref[:T] * 1.5)
            return solve_on(s)
        return f"reference table T={T}", f

    lanes = ref[None, :40] * np.linspace(0.5, 1.5, B)[:, None, None]

    def lane_tables(s):
        s.set_reference_trajectories(lanes)
        return solve_on(s)

    xa = np.stack([x0[:, 0], x0[:, 1], x0[:, 2]], 1)
    xf = xa + np.array([0.08, 0.01, 0.1])

    def straight_lines(s):
        T = s.gen_straight_lines(xa, xf, 0.0, 3.0, auto_angle=True)
        return (np.array([T]),) + solve_on(s)

    u_buf = u(5, B)

    def delay(cols):
        def f(s):
            s.set_delay_comp(cols * TS)
            for k in range(cols):
                s.delay_buffer_push(u_buf[k])
            r = s.delay_buffer_sim(x0)
            cl = s.closed_loop(x0, 2, plant_delay=TS)       # the solver sees the predicted state
            s.set_delay_comp(0.0)
            return r, np.array([cols]), cl["X"], cl["Xsim"], cl["U"]
        return f"delay_comp cols={cols}", f

    plant_shapes = [make_shape(n) for n in NAMES[::-1]]
    mu, ce = rng.uniform(0.15, 0.25, B), rng.uniform(0.02, 0.04, B)

    def plant(s):
        s.set_plant(shapes=plant_shapes, shape_id=np.arange(B)[::-1] % 4, mu_sp=mu, c_ellipse=ce)
        r = s.closed_loop(x0, 3, noise=noise[:3])
        s.clear_plant()
        return tuple(r[k] for k in sorted(r))

    def no_plant(s):
        r = s.closed_loop(x0, 3, noise=noise[:3])
        return tuple(r[k] for k in sorted(r))

    nz_ol = rng.normal(0.0, 1e-4, (6, B, 4))

    def open_loop(M):
        U = u(B, M)

        def f(s):
            r = s.open_loop(x0, U, 6, noise=nz_ol, plant_delay=3 * TS)
            return tuple(r[k] for k in sorted(r))
        return f"open_loop M={M}", f

    return ([closed_loop(n, xsim) for n in (3, 7, 2) for xsim in (True, False)]
            + [("closed_loop_metrics", metrics), shared_table(30), shared_table(201), ("per-lane tables", lane_tables),
               ("gen_straight_lines", straight_lines), delay(2), delay(5), delay(1),
               ("set_plant", plant), ("clear_plant", no_plant), open_loop(1), open_loop(65), open_loop(3)])


def _same(name, want, got):
    assert len(got) == len(want), name
    for k, (a, g) in enumerate(zip(want, got)):
        assert a.shape == g.shape and np.array_equal(a, g), (name, k)


def test_named_buffers_regrow_and_shrink_like_a_fresh_handle():
    calls = _calls()
    alone = {}
    for name, f in calls:
        s = _handle()
        try:
            alone[name] = f(s)
        finally:
            s.close()
    s = _handle()
    try:
        for name, f in calls:
            _same(name, alone[name], f(s))
    finally:
        s.close()


@pytest.mark.parametrize("N,nlp", [(10, "SQP_RTI"), (10, "SQP"), (32, "SQP_RTI")])
def test_handles_created_and_closed_in_turn_repeat_bit_for_bit(oracle, N, nlp):
    calls = _calls() + staging_calls(oracle, N)
    first = None
    for rnd in range(8):
        s = _handle(N, nlp)
        try:
            if N == 32:
                assert s.layout()[0] == 2          # two stages per lane
            got = [(name, f(s)) for name, f in calls]
        finally:
            s.close()
        if first is None:
            first = got
            continue
        for (name, want), (_, g) in zip(first, got):
            _same(f"round {rnd}: {name}", want, g)
