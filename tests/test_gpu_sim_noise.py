"""GPU: sim_noise generated on the device (qsp_set_sim_noise, csrc/qsp_noise.hpp).

The generator against its numpy restatement (tests/sim_noise_ref.py); the closed loop and the open loop drawing in
their kernels against the same calls with the table that qsp_gen_sim_noise writes, bit for bit; shards and chunks
of a run drawing the whole run's numbers; the errors and the handle's state.  B = 67 (neither a wave nor a block
multiple), four shapes, N = 10, three full SQP steps per solve."""
import ctypes as C

import numpy as np
import pytest

import open_loop_ref as R
from conftest import config2_x0, straight_traj
from sim_noise_ref import sim_noise

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
TS = 0.05
B, N, K = 67, 10, 3
ERR_ARG, ERR_STATE = -1, -3
ALL = ("X", "U_out", "S_p", "mode", "mode_steps")


def _solver(batch=B, lane0=0):
    """A handle of `batch` lanes that stand at the global lanes lane0 .. lane0 + batch - 1 (shape by global lane)."""
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=batch, sqp_iters=K)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=(lane0 + np.arange(batch)) % 4)
    s.set_reference_trajectory(straight_traj())
    return s


def _same(a, b, keys=None):
    for k in (keys or a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------ 1. the generator
def test_generator_matches_numpy_reference():
    """|n_dev - n_ref| <= 1e-13 sigma[c] scale: the argument rounding of cos(2 pi u) is <= 7e-16, the libm errors a few
    ulp, times |r| <= 6.76: about 1e-14, a tenfold margin.  A wrong bit in Philox moves u by >= 2^-32."""
    seed, stream, step0, lane0, T = 0x9E3779B97F4A7C15, 3, 2 ** 32 - 2, 2 ** 31 + 5, 5
    rng = np.random.default_rng(1)
    scale = rng.uniform(0.25, 4.0, B)
    scale[11] = 0.0
    sigma = np.array([2e-5, 3e-4, 1.5e-3, 0.7])
    s = _solver()
    try:
        s.set_sim_noise(seed, sigma=sigma, lane_scale=scale, stream=stream, step_offset=step0, lane_offset=lane0)
        got = s.gen_sim_noise(T)
    finally:
        s.close()
    ref = sim_noise(seed, T, B, sigma=sigma, lane_scale=scale, stream=stream, step_offset=step0, lane_offset=lane0)
    assert got.shape == (T, B, 4)
    bound = 1e-13 * sigma[None, None, :] * scale[None, :, None]
    err = np.abs(got - ref)
    on = scale > 0
    print("max |n_dev - n_ref| / (sigma scale) = %.3e" % (err[:, on] / (sigma[None, None, :] * scale[None, on, None])).max())
    assert np.all(err <= bound)
    assert np.all(got[:, 11] == 0.0)                       # the scale-0 lane, exactly
    assert np.all(got[:, on] != 0.0) and np.all(np.isfinite(got))


# ------------------------------------------------------------------ 2. device path == table path
def test_closed_loop_device_noise_equals_table():
    """plant delay and delay compensation of one step, a disturbance at step 2: X, Xsim, U, status, every bit."""
    T = 6
    x0 = config2_x0(B, 3)
    amp = np.random.default_rng(4).uniform(-2e-3, 2e-3, B)
    kw = dict(plant_delay=TS, disturbance=True, t_dist=2, amplitude=amp)
    s = _solver()
    try:
        s.set_sim_noise(77, stream=1, lane_scale=np.linspace(0.5, 20.0, B))
        table = s.gen_sim_noise(T)
        s.set_delay_comp(TS)                               # zeroes u_buff_contr: both runs start alike
        dev = s.closed_loop(x0, T, noise=None, **kw)
        s.clear_sim_noise()
        s.set_delay_comp(TS)
        tab = s.closed_loop(x0, T, noise=table, **kw)
        s.set_delay_comp(TS)
        free = s.closed_loop(x0, T, noise=None, **kw)
    finally:
        s.close()
    _same(dev, tab, ("X", "Xsim", "U", "status"))
    assert np.abs(dev["X"] - free["X"]).max() > 1e-6 and not np.array_equal(dev["U"], free["U"])


def test_closed_loop_metrics_device_noise_equals_table():
    """qsp_closed_loop_metrics with a per-lane plant: metrics, x_end, status, every bit."""
    T = 6
    x0 = config2_x0(B, 5)
    rng = np.random.default_rng(6)
    s = _solver()
    try:
        s.set_plant(mu_sp=rng.uniform(0.15, 0.3, B), c_ellipse=rng.uniform(0.02, 0.04, B))
        s.set_sim_noise(78, sigma=[1e-4, 1e-4, 2e-3, 3e-4])
        table = s.gen_sim_noise(T)
        dev = s.closed_loop_metrics(x0, T, noise=None)
        s.clear_sim_noise()
        tab = s.closed_loop_metrics(x0, T, noise=table)
        free = s.closed_loop_metrics(x0, T, noise=None)
    finally:
        s.close()
    _same(dev, tab, ("metrics", "x_end", "status"))
    assert not np.array_equal(dev["x_end"], free["x_end"])


@pytest.mark.parametrize("tile", [1, 4, 8])
def test_open_loop_device_noise_equals_table(tile):
    """M = 3, T = 9 (crosses a tile edge of 4 and of 8 steps), two delay columns, clip on: every output, every bit; the
    noise is shared by a lane's candidates."""
    M, T = 3, 9
    x0, U = config2_x0(B, 7), R.law_open_loop(B, M, 8)
    kw = dict(plant_delay=2 * TS, clip=True, want=ALL, store_tile=tile)
    s = _solver()
    try:
        s.set_sim_noise(79, sigma=[1e-4, 1e-4, 1e-3, 1e-4], stream=tile)
        table = s.gen_sim_noise(T)
        dev = s.open_loop(x0, U, T, noise=None, **kw)
        s.clear_sim_noise()
        tab = s.open_loop(x0, U, T, noise=table, **kw)
        free = s.open_loop(x0, U, T, noise=None, **kw)
    finally:
        s.close()
    assert set(dev) == set(ALL) | {"x_end"}
    _same(dev, tab)
    assert np.array_equal(dev["X"][:, :, 0], np.broadcast_to((x0 + table[0])[:, None], (B, M, 4)))
    assert np.abs(dev["X"] - free["X"]).max() > 1e-5


def test_open_loop_device_entry_draws_with_null_noise():
    """qsp_open_loop_device with io->noise == NULL and a generator installed equals the host entry with the table."""
    import torch
    from uclv_qs_pushing_matlab_amd._lib import OpenLoopIO
    M, T = 3, 9
    x0, U = config2_x0(B, 9), R.law_open_loop(B, M, 10)
    kw = dict(plant_delay=2 * TS, clip=True)
    dev0 = torch.device("cuda", 0)
    s = _solver()
    try:
        s.set_sim_noise(80, sigma=[1e-4, 1e-4, 1e-3, 1e-4])
        table = s.gen_sim_noise(T)
        s.clear_sim_noise()
        host = s.open_loop(x0, U, T, noise=table, want=ALL, **kw)
        s.set_sim_noise(80, sigma=[1e-4, 1e-4, 1e-3, 1e-4])
        outs = {k: np.full_like(v, -7) for k, v in host.items()}
        t = {k: torch.as_tensor(np.ascontiguousarray(v), device=dev0) for k, v in {**dict(x0=x0, U=U), **outs}.items()}
        io = OpenLoopIO()
        for k, v in t.items():
            setattr(io, k, v.data_ptr())
        assert not io.noise
        torch.cuda.synchronize()
        s.open_loop_device(io, T, M, u_steps=1, **kw)
        s.synchronize()
        for k in host:
            assert np.array_equal(host[k], t[k].cpu().numpy()), k
    finally:
        s.close()


# ------------------------------------------------------------------ 3. the noise is applied
def test_noise_is_applied_and_streams_differ():
    T = 4
    x0 = config2_x0(B, 11)
    s = _solver()
    try:
        free = s.closed_loop(x0, T)
        s.set_sim_noise(5, stream=0)
        table = s.gen_sim_noise(T)
        a = s.closed_loop(x0, T)
        a2 = s.closed_loop(x0, T)
        s.set_sim_noise(5, stream=1)
        b = s.closed_loop(x0, T)
    finally:
        s.close()
    np.testing.assert_array_equal(a["X"][:, 0], x0 + table[0])     # no disturbance at step 1: exactly x0 + n
    assert np.all(a["X"][:, 0] != x0)
    assert np.abs(a["X"] - free["X"]).max() > 1e-5
    assert not np.array_equal(a["X"], b["X"]) and not np.array_equal(a["U"], b["U"])
    _same(a, a2, ("X", "Xsim", "U", "status"))


# ------------------------------------------------------------------ 4. shards, 5. chunks
def test_shard_reproduces_its_lanes_of_the_whole_batch():
    """A handle of 32 lanes at lane_offset 32 draws and computes lanes 32..63 of a handle of 64."""
    T = 4
    x0 = config2_x0(64, 12)
    scale = np.linspace(1.0, 3.0, 64)
    whole, part = _solver(64), _solver(32, lane0=32)
    try:
        whole.set_sim_noise(13, stream=2, lane_scale=scale)
        part.set_sim_noise(13, stream=2, lane_scale=scale[32:], lane_offset=32)
        tw, tp = whole.gen_sim_noise(T), part.gen_sim_noise(T)
        rw, rp = whole.closed_loop(x0, T), part.closed_loop(x0[32:], T)
    finally:
        whole.close()
        part.close()
    np.testing.assert_array_equal(tp, tw[:, 32:])
    for k in ("X", "U", "status"):
        np.testing.assert_array_equal(rp[k], rw[k][32:], err_msg=k)
    assert not np.array_equal(tw[:, :32], tw[:, 32:])


def test_chunk_reproduces_its_steps_of_the_whole_run():
    s = _solver()
    try:
        s.set_sim_noise(14)
        whole = s.gen_sim_noise(7)
        s.set_sim_noise(14, step_offset=4)
        np.testing.assert_array_equal(s.gen_sim_noise(3), whole[4:7])
        # a closed loop continued from a chunk boundary draws the second chunk's rows
        x0 = config2_x0(B, 15)
        r = s.closed_loop(x0, 2)
        np.testing.assert_array_equal(r["X"][:, 0], x0 + whole[4])
    finally:
        s.close()


# ------------------------------------------------------------------ 6. errors and state
def test_errors_and_state():
    from uclv_qs_pushing_matlab_amd import _lib
    L = _lib.lib()
    T, M = 3, 2
    s, fresh = _solver(), _solver()
    h = s.handle
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    x0, idx = np.ascontiguousarray(config2_x0(B, 16)), np.ones(B, np.int32)
    table = np.zeros((T, B, 4))
    X, U, S = np.zeros((B, T + 1, 4)), np.zeros((B, T, 2)), np.zeros((B, T), np.int32)
    met = np.zeros((B, 10))
    Uo, xe = np.ascontiguousarray(R.law_open_loop(B, M, 17)), np.zeros((B, M, 4))
    oo = _lib.OpenLoopOpts()
    L.qsp_default_open_loop_opts(C.byref(oo))
    oo.n_steps, oo.M = T, M
    try:
        # nothing installed: the table cannot be generated, and get reports none
        assert L.qsp_gen_sim_noise(h, T, p(table)) == ERR_STATE
        assert s.get_sim_noise() is None
        s.set_sim_noise(21, sigma=[1e-4, 2e-4, 3e-4, 4e-4], lane_scale=np.full(B, 2.0), stream=4, step_offset=5,
                        lane_offset=6)
        before = s.get_sim_noise()
        assert (before["seed"], before["stream"], before["step_offset"], before["lane_offset"]) == (21, 4, 5, 6)
        np.testing.assert_array_equal(before["sigma"], [1e-4, 2e-4, 3e-4, 4e-4])
        np.testing.assert_array_equal(before["lane_scale"], np.full(B, 2.0))
        # a table and a generator: ambiguous, on all five entries
        io = _lib.OpenLoopIO()
        io.x0, io.U, io.noise, io.x_end = 1, 1, 1, 1       # never dereferenced: the call is refused first
        both = [L.qsp_closed_loop(h, p(x0), p(idx), T, p(table), p(X), p(U), p(S)),
                L.qsp_closed_loop_ex(h, None, p(x0), p(idx), T, p(table), p(X), None, p(U), p(S)),
                L.qsp_closed_loop_metrics(h, None, p(x0), p(idx), T, p(table), p(met), None, None),
                L.qsp_open_loop(h, C.byref(oo), p(x0), p(Uo), p(table), None, None, None, None, None, p(xe)),
                L.qsp_open_loop_device(h, C.byref(oo), C.byref(io), None)]
        assert both == [ERR_ARG] * 5, both
        assert b"ambiguous" in L.qsp_last_error()

        def gen(**kw):
            g = _lib.SimNoise()
            L.qsp_default_sim_noise(C.byref(g))
            keep = []
            for k, v in kw.items():
                if k == "sigma":
                    g.sigma[:] = v
                elif k == "lane_scale":
                    keep.append(np.ascontiguousarray(v, np.float64))
                    g.lane_scale = keep[-1].ctypes.data
                else:
                    setattr(g, k, v)
            return L.qsp_set_sim_noise(h, C.byref(g))

        def scale_with(v):
            a = np.ones(B)
            a[B - 1] = v
            return a

        size = C.sizeof(_lib.SimNoise)
        t_before = s.gen_sim_noise(T)
        # every refusal leaves the previous installation: what get reports, and what is drawn
        for kw in (dict(sigma=[1e-5, -1e-5, 1e-3, 1e-4]), dict(sigma=[1e-5, 1e-5, float("nan"), 1e-4]),
                   dict(sigma=[float("inf"), 1e-5, 1e-3, 1e-4]),
                   dict(lane_scale=scale_with(float("inf"))), dict(lane_scale=scale_with(float("nan"))),
                   dict(lane_scale=scale_with(-1.0)),
                   dict(step_offset=-1), dict(lane_offset=-1), dict(lane_offset=2 ** 32 - B + 1), dict(lane_offset=2 ** 40),
                   dict(struct_size=size - 8), dict(struct_size=size + 8), dict(struct_size=0)):
            assert gen(**kw) == ERR_ARG, kw
            after = s.get_sim_noise()
            assert all(np.array_equal(after[k], before[k]) for k in before), kw
        assert L.qsp_set_sim_noise(h, None) == ERR_ARG and L.qsp_set_sim_noise(None, None) == ERR_ARG
        np.testing.assert_array_equal(s.gen_sim_noise(T), t_before)
        assert gen(lane_offset=2 ** 32 - B) == 0           # the largest offset is accepted
        assert L.qsp_gen_sim_noise(h, 0, p(table)) == ERR_ARG and L.qsp_gen_sim_noise(h, T, None) == ERR_ARG
        # the python layer refuses alike and keeps its copy
        s.set_sim_noise(**before)
        with pytest.raises(_lib.QspError):
            s.set_sim_noise(1, sigma=[1.0, 1.0, 1.0, float("nan")])
        after = s.get_sim_noise()
        assert all(np.array_equal(after[k], before[k]) for k in before)
        np.testing.assert_array_equal(s.gen_sim_noise(T), t_before)
        # cleared: a closed loop with noise=None is a fresh handle's
        s.clear_sim_noise()
        assert s.get_sim_noise() is None and L.qsp_gen_sim_noise(h, T, p(table)) == ERR_STATE
        _same(s.closed_loop(x0, T), fresh.closed_loop(x0, T), ("X", "Xsim", "U", "status"))
    finally:
        s.close()
        fresh.close()


# ------------------------------------------------------------------ 7. the python helpers
def test_helpers_noise_on_device():
    from uclv_qs_pushing_matlab_amd import helper
    from uclv_qs_pushing_matlab_amd.controller import NMPCController
    from uclv_qs_pushing_matlab_amd.model import PusherSliderModel
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    nb, time_sim = 5, 0.2
    plant = PusherSliderModel("plant", object_selection("santal"), object_name="santal")
    ctrl = NMPCController("nmpc", plant, TS, N, batch=nb, nlp_solver_type="SQP_RTI", sqp_iters=K)
    ctrl.create_ocp_solver()
    y_ref = np.zeros((6, 201))
    y_ref[0] = 0.01 * np.arange(201) * TS
    ctrl.set_reference_trajectory(y_ref)
    sv = ctrl.ocp_solver
    x0 = config2_x0(nb, 18)
    T = len(np.arange(0.0, time_sim + 1e-9, TS))
    try:
        # the handle's own generator survives the call; the call's is (seed, the reference's sigma, no scale)
        sv.set_sim_noise(99, sigma=[1e-3, 0.0, 0.0, 0.0], lane_scale=np.arange(nb, dtype=float), stream=7)
        before = sv.get_sim_noise()
        out = helper.closed_loop_matlab(plant, ctrl, x0, time_sim, sim_noise=True, seed=31, noise_on_device=True)
        m = helper.closed_loop_metrics(plant, ctrl, x0, time_sim, sim_noise=True, seed=31, noise_on_device=True)
        ol = helper.open_loop_matlab(plant, x0, 0.01, 0.002, time_sim, TS, sim_noise=True, seed=31, solver=sv,
                                     noise_on_device=True)
        after = sv.get_sim_noise()
        assert all(np.array_equal(after[k], before[k]) for k in before)
        sv.set_sim_noise(31)
        r = sv.closed_loop(x0, T)
        m2 = sv.closed_loop_metrics(x0, T)
        o2 = sv.open_loop(x0, np.broadcast_to([0.01, 0.002], (nb, 1, 2)), T, clip=True, v_alpha=1.0, Ts=TS,
                          want=("X", "U_out", "S_p"))
        np.testing.assert_array_equal(out[0], r["X"][:, :T, 0])
        np.testing.assert_array_equal(out[6], r["U"][:, :, 0])
        _same(m, m2, ("metrics", "x_end", "status"))
        np.testing.assert_array_equal(ol[0], o2["X"][:, 0, :T, 0])
        # from a handle without a generator the call leaves none; without sim_noise the flag does nothing
        sv.clear_sim_noise()
        helper.closed_loop_matlab(plant, ctrl, x0, time_sim, sim_noise=True, seed=31, noise_on_device=True)
        assert sv.get_sim_noise() is None
        quiet = helper.closed_loop_matlab(plant, ctrl, x0, time_sim, sim_noise=False, noise_on_device=True)
        np.testing.assert_array_equal(quiet[0], helper.closed_loop_matlab(plant, ctrl, x0, time_sim)[0])
        assert not np.array_equal(quiet[0], out[0])
    finally:
        sv.close()
