"""GPU: the host entry points share one staging pool (Staging, qsp_capi.hip) and do not disturb each other.

Ten calls of different array counts and sizes run on one handle (B = 5, N = 10), in order and then in reverse
order, so that every call finds the pool as another one left it -- larger, smaller, holding the other's data.
Each result must equal, bit for bit, the same call made alone on a fresh handle.  The calls carry what they
depend on besides their arguments (references, the tail of U, the delay buffer) themselves."""
import numpy as np
import pytest

from conftest import config2_x0, straight_traj
from qp_data import build_qp

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
B, N, TS = 5, 10, 0.05


def _handle():
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=B, sqp_iters=3)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=np.arange(B) % 4)
    s.set_reference_trajectory(straight_traj())
    return s


def _calls(oracle, N=N):
    """[(name, f(handle) -> tuple of arrays)] with fixed inputs, for a handle of horizon N (B lanes)."""
    from oracle.oracle import make_opts
    rng = np.random.default_rng(51)
    x0 = config2_x0(B, 52)
    yref = np.repeat(straight_traj()[None, :N], B, 0)
    ye = yref[:, N - 1, :4].copy()

    def u(*shape):
        return np.stack([rng.uniform(0.001, 0.03, shape), rng.uniform(-0.05, 0.05, shape)], -1)

    def xu(n):
        x = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-0.05, 0.05, (n, 1))], 1)
        return x, u(n), np.arange(n) % 4

    U_ol, nz_ol = u(B, 65), rng.normal(0.0, 1e-4, (9, B, 4))
    sig = rng.uniform(0.0, 0.05, 3)
    U_ro, tail = u(B, 3, N), u(B, N)
    un, ut = np.linspace(0.0, 0.03, 3), np.linspace(-0.05, 0.05, 5)
    xm, um, sm = xu(7)
    px, py, s0 = rng.uniform(-0.05, -0.03, 2), rng.uniform(-0.02, 0.02, 2), rng.uniform(0.0, 0.05, 2)
    xr, ur, sr = xu(4)
    # two Gauss-Newton QPs of the OCP at perturbed iterates (tests/test_gpu_twin.py::test_qp_bit_identical's)
    op = make_opts(N=N)
    xq = config2_x0(2, 53)
    Xq = np.repeat(xq[:, None], N + 1, 1) + rng.normal(0, 2e-3, (2, N + 1, 4))
    Uq = np.stack([rng.uniform(0, 0.03, (2, N)), rng.uniform(-0.02, 0.02, (2, N))], 2)
    A, Bq, b, H, g, lo, hi, _act, dx0 = build_qp(oracle, op, Xq, Uq, yref[:2].copy(), ye[:2].copy(), xq, np.arange(2))
    nz_cl = rng.normal(0.0, 1e-4, (3, B, 4))
    u_buf = u(2, B)

    def open_loop(s):
        r = s.open_loop(x0, U_ol, 9, noise=nz_ol, plant_delay=2 * TS, want=("X", "U_out", "S_p", "mode", "mode_steps"))
        return tuple(r[k] for k in sorted(r))

    def cost_landscape(s):
        r = s.cost_landscape(x0, un, ut, U_tail=tail, yref=yref, yref_e=ye)
        return tuple(r[k] for k in sorted(r))

    def qp_solve(s):
        r = s.qp_solve(A.reshape(2, N, 16), Bq.reshape(2, N, 8), b, H, g, lo, hi, dx0)
        return tuple(r[k] for k in sorted(r))

    def closed_loop(s):
        s.set_delay_comp(2 * TS)                        # an empty controller buffer, as a fresh handle's
        r = s.closed_loop(x0, 3, noise=nz_cl, plant_delay=TS)
        s.set_delay_comp(0.0)
        return tuple(r[k] for k in sorted(r))

    def delay_buffer_sim(s):
        s.set_delay_comp(2 * TS)
        for k in range(2):
            s.delay_buffer_push(u_buf[k])
        r = s.delay_buffer_sim(x0)
        s.set_delay_comp(0.0)
        return (r,)

    return [("open_loop", open_loop),
            ("eval_spline", lambda s: s.eval_spline(sig, np.arange(3) % 4)),
            ("rollout_cost", lambda s: s.rollout_cost(x0, U_ro, yref=yref, yref_e=ye, want_viol=True, want_x_end=True)),
            ("cost_landscape", cost_landscape),
            ("eval_modes", lambda s: s.eval_modes(xm, um, shape_id=sm, want_cone=True)),
            ("reproject_contact", lambda s: (s.reproject_contact(px, py, s0, shape_id=np.arange(2)),)),
            ("eval_rk4", lambda s: s.eval_rk4(xr, ur, shape_id=sr)),
            ("qp_solve", qp_solve),
            ("closed_loop", closed_loop),
            ("delay_buffer_sim", delay_buffer_sim)]


def test_calls_sharing_the_staging_pool_do_not_disturb_each_other(oracle):
    calls = _calls(oracle)
    alone = {}
    for name, f in calls:
        s = _handle()
        try:
            alone[name] = f(s)
        finally:
            s.close()
    s = _handle()
    try:
        for name, f in calls + calls[::-1]:
            got = f(s)
            assert len(got) == len(alone[name])
            for k, (a, g) in enumerate(zip(alone[name], got)):
                assert np.array_equal(a, g), (name, k)
    finally:
        s.close()
