"""GPU: qsp_gen_waypoints (waypoints_kernel) against its numpy restatement (tests/waypoints_np.py) bit for bit
under every law and yaw rule, against the host mirror TrajectoryGenerator.waypoints_gen on the disturbance
path, installed as a reference table under the closed loop, and its refusals."""
import ctypes as C

import numpy as np
import pytest

import waypoints_np as wnp

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
TS, N = 0.05, 10
U6, U12 = 2.0 ** -6, 2.0 ** -12


def _paths():
    """Five lanes in K = 4 slots; the slots a lane does not use hold NaN (they are not read).
    lane 0  main.m's two-waypoint path, shortened: (0, 0) -> (0.02, 0) at 0.01 m/s
    lane 1  arrival times on samples: 2 s and 3 s are samples 40 and 60
    lane 2  headings 3 pi / 4, -3 pi / 4, 3 pi / 4: the unwrapped yaw leaves [-pi, pi]
    lane 3  at 0.01 m/s a sample covers 0.0005 m: the segment of 2^-12 m holds no sample of the linspace law,
            the one of 3 * 2^-12 m one
    lane 4  another speed, off the origin
    Lanes 2 to 4 have dyadic coordinates: their dx, dy are exact and the headings multiples of pi / 4, which
    every atan2 returns correctly rounded, numpy's and the C library's alike."""
    wp = np.full((5, 4, 2), np.nan)
    vel = np.full((5, 3), np.nan)
    wp[0, :2] = [[0.0, 0.0], [0.02, 0.0]]
    wp[1, :3] = [[0.0, 0.0], [0.02, 0.0], [0.02, 0.01]]
    wp[2] = [[0.0, 0.0], [-U6, U6], [-2 * U6, 0.0], [-3 * U6, U6]]
    wp[3] = [[0.0, 0.0], [U6, 0.0], [U6, U12], [U6 - 3 * U12, U12]]
    wp[4, :2] = [[U6, -U6], [2 * U6, 0.0]]
    n_wp = np.array([2, 3, 4, 4, 2], np.int32)
    vel[0, :1], vel[1, :2], vel[2], vel[3], vel[4, :1] = 0.01, 0.01, 0.01, 0.01, 0.0125
    theta = np.array([0.0, 0.1, -0.2, 0.3, -0.4])
    s_ref = np.array([0.0, 0.004, -0.01, 0.002, -0.03])
    return wp, vel, n_wp, theta, s_ref


def _solver(B):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=B)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=np.arange(B) % 4)
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("yaw", wnp.YAWS)
@pytest.mark.parametrize("law", wnp.LAWS)
def test_device_table_is_the_restatement(law, yaw):
    wp, vel, n_wp, theta, s_ref = _paths()
    B = len(wp)
    th = theta if yaw == "fixed" else None
    T, T_lane, ref = wnp.table(wp, vel, TS, n_wp, law, yaw, th, s_ref)
    # what the shapes are chosen for
    assert (B * T) % 256 != 0 and len(set(T_lane.tolist())) >= 2
    for i in range(B):
        d, h = wnp.segments(wp[i, :n_wp[i]], vel[i, :n_wp[i] - 1])
        q = wnp.arrival_times(d)[-1] / TS
        assert q == np.rint(q) or abs(q - np.rint(q)) > 1e-6, (i, q)
        if i == 1:
            assert np.array_equal(wnp.arrival_times(d), [0.0, 2.0, 3.0]) and 40 * TS == 2.0 and 60 * TS == 3.0
        if i == 2:
            assert not np.array_equal(wnp.segment_yaw(h, "heading_unwrapped", None), h)
        if i == 3:
            assert [int(np.floor(v / TS + 1e-9)) for v in d] == [31, 0, 1]
    s = _solver(B)
    Tg, Tl = s.gen_waypoints(wp, vel, n_wp=n_wp, law=law, yaw=yaw, theta=th, s_ref=s_ref)
    tab = s.get_reference_trajectories()
    s.close()
    assert Tg == T and np.array_equal(Tl, T_lane)
    assert tab.shape == (B, T, 6)
    assert np.array_equal(_bits(tab[:, :, :4]), _bits(ref[:, :, :4]))
    assert np.all(_bits(tab[:, :, 4:]) == 0)
    for i in range(B):
        assert np.array_equal(_bits(tab[i, T_lane[i]:]), _bits(np.repeat(tab[i, T_lane[i] - 1:T_lane[i]], T - T_lane[i], 0)))


def test_disturbance_path_matches_mirror():
    """Three lanes of the 1 201-sample disturbance path (main.m:132-139), each shifted: several blocks per lane."""
    from uclv_qs_pushing_matlab_amd.trajectory import TrajectoryGenerator
    B, K = 3, len(wnp.DISTURBANCE)
    off = np.array([[0.0, 0.0], [0.01, -0.02], [-0.03, 0.005]])
    wp = wnp.DISTURBANCE[None] + off[:, None]
    s_ref = np.array([0.0, 0.01, -0.02])
    s = _solver(B)
    T, T_lane = s.gen_waypoints(wp, 0.01, s_ref=s_ref)
    tab = s.get_reference_trajectories()
    s.close()
    assert T == 1201 and np.all(T_lane == 1201) and T > 4 * 256
    for i in range(B):
        tg = TrajectoryGenerator(TS, 0.01)
        tg.set_target([0.0, 0.0, 0.0, s_ref[i]], [0.0, 0.0, 0.0, 0.0], 0.0, 60.0)
        tg.waypoints_, tg.waypoints_velocities = wp[i], [0.01]
        t, ref = tg.waypoints_gen()
        d, _ = wnp.segments(wp[i], np.full(K - 1, 0.01))
        knots = wnp.arrival_times(d)[1:-1]
        keep = np.all(np.abs(t[:, None] - knots[None]) > 1e-9, axis=1)
        assert len(t) == T and (~keep).sum() <= K - 2
        np.testing.assert_allclose(tab[i, keep, :4], ref[:4].T[keep], rtol=1e-14, atol=1e-15)
        assert np.all(tab[i, :, 4:] == 0.0)


def test_installed_as_a_table():
    """A handle that generated its table and one that was handed the same table run the same closed loop."""
    wp, vel, n_wp, _, _ = _paths()
    wp, vel, n_wp = wp[:4], vel[:4], n_wp[:4]
    B, steps = 4, 30
    a, b = _solver(B), _solver(B)
    T, T_lane = a.gen_waypoints(wp, vel, n_wp=n_wp)
    tab = a.get_reference_trajectories()
    b.set_reference_trajectories(tab)
    x0 = np.concatenate([tab[:, 0, :3], np.zeros((B, 1))], 1)
    ra, rb = a.closed_loop(x0, steps), b.closed_loop(x0, steps)
    past = int(T_lane.min()) + 5
    assert past < T
    xs = np.concatenate([tab[:, past - 1, :3], np.zeros((B, 1))], 1)
    ua, ub = a.controller_solve(xs, past), b.controller_solve(xs, past)
    sa, sb = a.get("status"), b.get("status")
    a.close()
    b.close()
    for k in ("X", "U"):
        assert np.array_equal(_bits(ra[k]), _bits(rb[k])), k
    assert np.array_equal(ra["status"], rb["status"])
    assert np.array_equal(_bits(ua), _bits(ub)) and np.array_equal(sa, sb)


# ------------------------------------------------------------------ refusals
def _valid():
    wp, vel, n_wp, theta, s_ref = _paths()
    return dict(law=0, yaw=0, K=4, wp=wp, n_wp=n_wp, vel=vel, theta=theta, s_ref=s_ref, struct_size=None)


def _edit(**kw):
    def apply(a):
        for k, v in kw.items():
            if callable(v):
                v(a[k])
            else:
                a[k] = v
    return apply


def _set(index, value):
    def put(arr):
        arr[index] = value
    return put


def _equal_waypoints(a):
    a["wp"][2, 2] = a["wp"][2, 1]


REFUSALS = {
    "struct_size_small": _edit(struct_size=8),
    "struct_size_large": _edit(struct_size=24),
    "law_above": _edit(law=2),
    "law_below": _edit(law=-1),
    "yaw_above": _edit(yaw=3),
    "yaw_below": _edit(yaw=-1),
    "K_below": _edit(K=1),
    "K_above": _edit(K=17),
    "n_wp_below": _edit(n_wp=_set(1, 1)),
    "n_wp_above": _edit(n_wp=_set(4, 5)),
    "waypoint_nan": _edit(wp=_set((2, 3, 1), np.nan)),
    "waypoint_inf": _edit(wp=_set((0, 1, 0), np.inf)),
    "theta_nan": _edit(yaw=2, theta=_set(3, np.nan)),
    "theta_missing": _edit(yaw=2, theta=None),
    "s_ref_inf": _edit(s_ref=_set(0, -np.inf)),
    "vel_zero": _edit(vel=_set((1, 1), 0.0)),
    "vel_negative": _edit(vel=_set((2, 0), -0.01)),
    "vel_nan": _edit(vel=_set((0, 0), np.nan)),
    "vel_inf": _edit(vel=_set((3, 2), np.inf)),
    "equal_waypoints_constant_speed": _equal_waypoints,
}


@pytest.fixture(scope="module")
def installed():
    """A handle with a table installed, and that table."""
    wp, vel, n_wp, theta, s_ref = _paths()
    s = _solver(len(wp))
    s.gen_waypoints(wp, vel, n_wp=n_wp, law="segment_linspace", yaw="fixed", theta=theta, s_ref=s_ref)
    yield s, s.get_reference_trajectories()
    s.close()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_leaves_the_table(installed, case):
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd._lib import ptr
    s, before = installed
    a = _valid()
    REFUSALS[case](a)
    o = _lib.WaypointOpts()
    s._L.qsp_default_waypoint_opts(C.byref(o))
    assert (o.struct_size, o.law, o.yaw) == (C.sizeof(_lib.WaypointOpts), 0, 0)
    o.law, o.yaw = a["law"], a["yaw"]
    if a["struct_size"] is not None:
        o.struct_size = a["struct_size"]
    T = C.c_int32(-7)
    Tl = np.full(s.B, -7, np.int32)
    wp, vel = np.ascontiguousarray(a["wp"]), np.ascontiguousarray(a["vel"])
    rc = s._L.qsp_gen_waypoints(s._h, C.byref(o), a["K"], ptr(wp), ptr(a["n_wp"]), ptr(vel), ptr(a["theta"]),
                                ptr(a["s_ref"]), C.byref(T), ptr(Tl))
    assert rc == -1, (case, rc)                                  # QSP_ERR_ARG
    if case.startswith("struct_size"):
        assert b"struct_size" in s._L.qsp_last_error()           # as qsp_options' is refused
    assert T.value == -7 and np.all(Tl == -7)
    after = s.get_reference_trajectories()
    assert np.array_equal(_bits(after), _bits(before))


def test_equal_waypoints_pass_under_linspace():
    """The 0/0 is the constant-speed time law's alone: the linspace law gives such a segment no row."""
    wp, vel, n_wp, _, s_ref = _paths()
    wp[2, 2] = wp[2, 1]
    T, T_lane, ref = wnp.table(wp, vel, TS, n_wp, "segment_linspace", "heading", None, s_ref)
    s = _solver(len(wp))
    Tg, Tl = s.gen_waypoints(wp, vel, n_wp=n_wp, law="segment_linspace", s_ref=s_ref)
    tab = s.get_reference_trajectories()
    s.close()
    assert Tg == T and np.array_equal(Tl, T_lane)
    assert np.array_equal(_bits(tab), _bits(ref))
