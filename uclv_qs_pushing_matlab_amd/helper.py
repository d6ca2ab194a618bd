"""helper.closed_loop_matlab mirror (helper.m:195-322), batched and device-resident.

The whole loop runs on the GPU through qsp_closed_loop_ex, one host round trip per call:
the disturbance branch (:221-236: y offset, contact re-projected onto the contour -- MATLAB's
fminunc restated as a damped Newton iteration), sim_noise (:240-242), the controller's delay
prediction delay_buffer_sim and its input buffer (NMPC_controller.m:112-120, helper.m:255),
NMPC_controller.solve, and the plant step with evalModelVariableShape and the plant's own delay
buffer (:289-307).  Not reproduced: print_ (console output).  The loop simulates with `plant` and solves with
the controller's model, as the reference does: a plant that is not the controller's own object is installed on
the handle for the call (OcpSolver.set_plant), with per-lane friction / limit-surface overrides for Monte-Carlo
runs, and closed_loop_metrics reduces such a run to per-lane metrics on the device.

helper.evaluate_cost_function and helper.debug_cost_function (helper.m:356-431), the reference's
optimality probe, run on the device too (OcpSolver.rollout_cost / cost_landscape): the cost of a control
trajectory rolled out with Euler steps, and the cost surface over a grid of first moves u_0 with the rest
of the solver's trajectory held, with its grid minimiser.  The figures (helper.m:433-451) are not drawn,
and closed_loop_matlab's debug_cost argument stays ignored: call debug_cost_function after a
controller.solve.  Two deliberate deviations (include/qsp_nmpc.h): the model is the OCP's f instead of the
fixed-shape plant.eval_model, and x0 is rolled out as given.

helper.open_loop_matlab (helper.m:132-193) runs on the device as well (OcpSolver.open_loop), and the contact
modes that the reference plots from mode_vect (convert_str2num, my_plot) come from the device too: mode_trace
labels a closed loop's trajectories.  Coding: "ST" 1, "SL" 2, "SR" 3; 0 / "" where u_t / u_n is NaN (both
inputs zero, as a delayed plant's buffer holds at its start), which the reference's if-chain would call "SR".
"""
import contextlib

import numpy as np


def _probe_refs(controller, t):
    """The probe's references: columns time_index + 1 .. time_index + Hp of the controller's table, clamped
    at its end as get_y_ref (NMPC_controller.m:307-313), time_index = round(t / Ts) (helper.m:358,409); the
    terminal term reads column time_index + Hp (helper.m:365,422).  One column later than solve stages them
    (index_time + k, k = 0..Hp-1, :343-346).  -> yref (Hp, 6), yref_e (4,)."""
    if controller.y_ref is None:
        raise RuntimeError("set_reference_trajectory must be called before the cost probe")
    y = np.asarray(controller.y_ref, np.float64)                       # 6 x T
    D = int(controller.delay_buff_comp)
    if D > 0:                                                           # set_reference_trajectory (:428-429)
        pre = np.zeros((6, D))
        pre[5] = y[5, 0]
        y = np.concatenate([pre, y], 1)
    time_index = int(np.round(t / controller.sample_time))              # MATLAB round: t >= 0 here
    idx = np.minimum(time_index + np.arange(1, controller.Hp + 1), y.shape[1])   # 1-based columns
    yref = y[:, idx - 1].T.copy()
    return yref, yref[-1, :4].copy()


def _lanes_x(controller, x):
    return np.broadcast_to(np.asarray(x, np.float64).reshape(-1, 4), (controller.batch, 4))


def evaluate_cost_function(xn, controller, plant, t, u_vect):
    """cost_fcn_ = evaluate_cost_function(xn, controller, plant, t, u_vect) (helper.m:356-367), batched:
    xn (B, 4) or (4,); u_vect (B, Hp, 2), (Hp, 2) or MATLAB's 2 x Hp.  Euler rollout, stage terms unscaled
    and without the 1/2 (:361,366): exactly twice the library's cost_scale = 0 value.  Returns (B,).
    `plant` is kept for the signature: the model is the OCP's f (module docstring)."""
    B, Hp = controller.batch, controller.Hp
    u = np.asarray(u_vect, np.float64)
    if u.ndim == 2 and u.shape == (2, Hp) and Hp != 2:
        u = u.T
    u = np.broadcast_to(u, (B, Hp, 2))
    yref, yref_e = _probe_refs(controller, t)
    c = controller.ocp_solver.rollout_cost(_lanes_x(controller, xn), u[:, None], integrator="euler", cost_scale=False,
                                           yref=yref, yref_e=yref_e)
    return 2.0 * c[:, 0]


def colon(lb, ub, step):
    """MATLAB's lb:step:ub as lb + k step, k = 0..floor((ub - lb) / step + 1e-10)."""
    return lb + np.arange(int(np.floor((ub - lb) / step + 1e-10)) + 1) * step


def debug_cost_function(x0, u_n_lb, u_t_lb, u_n_ub, u_t_ub, controller, plant, index, t, prewrap=False):
    """u_min = debug_cost_function(...) (helper.m:369-431), batched and without the figure: the cost of
    every u_0 on UN = u_n_lb:0.005:u_n_ub x UT = u_t_lb:0.005:u_t_ub (7 x 21 for the default bounds) with
    columns 2..Hp of ocp_solver.get('u') held (:376,413) -- the last solve's solution before the controller's
    shift -- Euler steps and the 1/2 (:418,423).
    Returns (u_min (B, 2), cost_values (B, len(UT), len(UN)): MATLAB's meshgrid layout cost_values(j, i),
    UN, UT).  u_min is the first minimum of cost_values(:) (:430-431).  `index` (the subplot slot) and
    `plant` are kept for the signature.  prewrap=True applies the controller's s pre-wrap
    (NMPC_controller.m:332) to x0 first, so the probe starts from the state the solver saw."""
    UN, UT = colon(u_n_lb, u_n_ub, 0.005), colon(u_t_lb, u_t_ub, 0.005)     # :380-381
    x = _lanes_x(controller, x0).copy()
    if prewrap:
        b = controller._shape_b[controller._shape_id]
        x[:, 3] = np.mod(x[:, 3], b) - b * (x[:, 3] < 0)
    yref, yref_e = _probe_refs(controller, t)
    r = controller.ocp_solver.cost_landscape(x, UN, UT, U_tail=None, integrator="euler", cost_scale=False,
                                             yref=yref, yref_e=yref_e)
    return r["u_min"], np.ascontiguousarray(r["cost"].transpose(0, 2, 1)), UN, UT


@contextlib.contextmanager
def _plant_for_call(plant, controller, plant_mu_sp, plant_c_ellipse):
    """The handle's plant model for one closed-loop call.  A `plant` that is not the controller's own object
    is installed as the plant's shape for every lane (the reference simulates with plant, solves with
    controller: helper.m:226-233, :244, :294-307), per-lane mu_sp / c_ellipse overrides on top; what was
    installed before comes back on every exit path.  With the controller's own plant object and no
    overrides nothing is touched."""
    sv = controller.ocp_solver
    foreign = plant is not controller.plant
    if not foreign and plant_mu_sp is None and plant_c_ellipse is None:
        yield
        return
    prev = sv.plant()
    try:
        sv.set_plant(shapes=[plant.shape] if foreign else None, mu_sp=plant_mu_sp, c_ellipse=plant_c_ellipse)
        yield
    finally:
        if prev is None:
            sv.clear_plant()
        else:
            sv.set_plant(**prev)


@contextlib.contextmanager
def _noise_for_call(solver, on, seed):
    """The handle's sim_noise generator for one call (noise_on_device): installed with `seed`, the reference's
    sigma and no lane scale; what the handle had before comes back on every exit path.  Off: nothing is touched."""
    if not on:
        yield
        return
    prev = solver.get_sim_noise()
    try:
        solver.set_sim_noise(seed)
        yield
    finally:
        if prev is None:
            solver.clear_sim_noise()
        else:
            solver.set_sim_noise(**prev)


def _closed_loop_inputs(controller, x0, time_sim, sim_noise, seed):
    Ts = controller.sample_time
    time_sim_vec = np.arange(0.0, time_sim + 1e-9, Ts)                      # :198
    T = len(time_sim_vec)
    B = controller.batch
    noise = None
    if sim_noise:                                                           # :243-245
        rng = np.random.default_rng(seed)
        noise = rng.standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    x0 = np.broadcast_to(np.asarray(x0, np.float64).reshape(-1, 4), (B, 4))
    return time_sim_vec, T, B, noise, x0


def closed_loop_matlab(plant, controller, x0, time_sim, print_=False, sim_noise=False, debug_cost=False,
                       disturbance_=False, amplitude_dist=0.0, t_dist=0, seed=0, plant_mu_sp=None,
                       plant_c_ellipse=None, noise_on_device=False):
    """Returns (x_s, x_sim, y_s, theta_s, S_p_x, S_p_y, u_n, u_t, time_sim_vec, mode_vect, found_sol),
    each with a leading batch dimension B (helper.m:195-197; x_sim is (B, 2T+1, 4): the reference's
    4 x (2T+1) with its T+1 leading zero columns); amplitude_dist may be per lane.
    The loop simulates with `plant` and solves with the controller's model: a plant other than
    controller.plant is the handle's plant for the call (OcpSolver.set_plant), and plant_mu_sp /
    plant_c_ellipse (scalars or (B,)) override its friction and limit-surface constant per lane.
    noise_on_device with sim_noise: the noise is drawn in the kernels from `seed` (OcpSolver.set_sim_noise, for
    this call) instead of a numpy table: other numbers of the same law, and no T x B x 4 table anywhere."""
    gen = bool(sim_noise and noise_on_device)
    time_sim_vec, T, B, noise, x0 = _closed_loop_inputs(controller, x0, time_sim, sim_noise and not gen, seed)
    with _plant_for_call(plant, controller, plant_mu_sp, plant_c_ellipse), \
            _noise_for_call(controller.ocp_solver, gen, seed):
        r = controller.ocp_solver.closed_loop(x0, T, index0=1, noise=noise, plant_delay=plant.time_delay,
                                              disturbance=bool(disturbance_), t_dist=int(t_dist),
                                              amplitude=amplitude_dist)
    X, U = r["X"][:, :T], r["U"]
    found_sol = r["status"] == 0                                            # :253-260
    S_p = plant.SP.FC(X[:, :, 3].ravel()).reshape(B, T, 2)                 # :316-318
    mode_vect = np.zeros((B, T), dtype="<U1")
    # x_sim = [zeros(nx, T+1) xk_sim ...] (helper.m:203, :247): T + 1 zero columns, then one per step
    x_sim = np.concatenate([np.zeros((B, T + 1, 4)), r["Xsim"]], 1)
    return (X[:, :, 0], x_sim, X[:, :, 1], X[:, :, 2], S_p[..., 0], S_p[..., 1], U[:, :, 0], U[:, :, 1],
            time_sim_vec, mode_vect, found_sol)


def closed_loop_metrics(plant, controller, x0, time_sim, print_=False, sim_noise=False, debug_cost=False,
                        disturbance_=False, amplitude_dist=0.0, t_dist=0, seed=0, plant_mu_sp=None,
                        plant_c_ellipse=None, noise_on_device=False):
    """closed_loop_matlab's run with the same arguments, reduced on the device to per-lane metrics
    (OcpSolver.closed_loop_metrics' dict): no trajectory comes back to the host."""
    gen = bool(sim_noise and noise_on_device)
    _, T, _, noise, x0 = _closed_loop_inputs(controller, x0, time_sim, sim_noise and not gen, seed)
    with _plant_for_call(plant, controller, plant_mu_sp, plant_c_ellipse), \
            _noise_for_call(controller.ocp_solver, gen, seed):
        return controller.ocp_solver.closed_loop_metrics(x0, T, index0=1, noise=noise, plant_delay=plant.time_delay,
                                                         disturbance=bool(disturbance_), t_dist=int(t_dist),
                                                         amplitude=amplitude_dist)


MODE_NUM = {"ST": 1, "SL": 2, "SR": 3, "": 0}      # helper.m:17-23; "" = no indicator set (QSP_MODE_NONE)
MODE_STR = np.array(["", "ST", "SL", "SR"])


def convert_str2num(mode_vect_str):
    """mode_vect_num = convert_str2num(mode_vect_str) (helper.m:17-23) on arrays of "ST"/"SL"/"SR" (and ""
    for the library's mode 0): an int32 array of the same shape."""
    a = np.asarray(mode_vect_str)
    out = np.zeros(a.shape, np.int32)
    for k, v in MODE_NUM.items():
        out[a == k] = v
    if not np.all(np.isin(a, list(MODE_NUM))):
        raise ValueError("convert_str2num: modes must be 'ST', 'SL', 'SR' or ''")
    return out


def convert_num2str(mode_vect_num):
    """The inverse: QSP_MODE_* numbers -> "ST"/"SL"/"SR" ("" for 0)."""
    return MODE_STR[np.asarray(mode_vect_num, np.int64)]


def applied_inputs(U, plant_delay_cols=0):
    """What a plant with a delay buffer of D columns applies at step i of the commanded inputs U (..., T, 2):
    zeros for i < D, then U[i - D] (u_buff_plant starts at zero: helper.m:148,174-176 and :211-212,289-296)."""
    U = np.asarray(U, np.float64)
    D = int(plant_delay_cols)
    if D == 0:
        return U.copy()
    T = U.shape[-2]
    out = np.zeros_like(U)
    out[..., D:, :] = U[..., :max(T - D, 0), :]
    return out


def mode_trace(solver, X, U, plant_delay_cols=0, shape_id=None):
    """Contact modes along a simulated trajectory, e.g. a closed loop's X_traj (B, T [+ 1], 4) and U_traj
    (B, T, 2): the mode of (X[:, i], applied input at step i), the applied input being U shifted by the
    plant's delay with zeros (applied_inputs).  shape_id (B,) or scalar; None: the solver's per-lane ids
    (its batch must then be B).  -> (B, T) int32."""
    U = np.asarray(U, np.float64)
    B, T = U.shape[:2]
    X = np.asarray(X, np.float64)[:, :T]
    ua = applied_inputs(U, plant_delay_cols)
    if shape_id is None:
        if solver.B != B:
            raise ValueError(f"mode_trace: {B} lanes on a solver of batch {solver.B}: pass shape_id")
        shape_id = solver.shape_ids
    sid = np.repeat(np.broadcast_to(np.asarray(shape_id, np.int32), (B,)), T)
    return solver.eval_modes(X.reshape(-1, 4), ua.reshape(-1, 2), shape_id=sid).reshape(B, T)


def open_loop_matlab(plant, x0, u_n, u_t, time_sim, sample_time, sim_noise=False, seed=0, solver=None,
                     noise_on_device=False):
    """[x_s, y_s, theta_s, S_p_x, S_p_y, u_n, u_t, time_sim_vec] = open_loop_matlab(plant, x0, u_n, u_t, time_sim,
    sample_time, sim_noise) (helper.m:132-193), batched: x0 (B, 4) or (4,); u_n, u_t scalars or (B,).  Every
    returned trajectory is (B, T) with T = length(0:sample_time:time_sim); u_t is the commanded input after the
    clip; S_p_y = x(4, :) as helper.m:190 returns it (the contact abscissa s, not the spline's y).  Noise is
    drawn on the host as closed_loop_matlab's (seeded), or with noise_on_device in the kernel (from `seed`,
    OcpSolver.set_sim_noise for this call).  solver: an OcpSolver whose batch and shapes to use
    (default: the plant's own one-lane evaluator, for B = 1)."""
    time_sim_vec = np.arange(0.0, time_sim + 1e-9, sample_time)            # :136
    T = len(time_sim_vec)
    sv = plant._ev if solver is None else solver
    B = sv.B
    x0 = np.broadcast_to(np.asarray(x0, np.float64).reshape(-1, 4), (B, 4))
    U = np.stack([np.broadcast_to(np.asarray(u_n, np.float64), (B,)),
                  np.broadcast_to(np.asarray(u_t, np.float64), (B,))], 1)[:, None]     # (B, 1, 2): repmat, :144
    noise = None
    gen = bool(sim_noise and noise_on_device)
    if sim_noise and not gen:                                               # :154-156
        rng = np.random.default_rng(seed)
        noise = rng.standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    with _noise_for_call(sv, gen, seed):
        r = sv.open_loop(x0, U, T, noise=noise, plant_delay=plant.time_delay, clip=True, v_alpha=0.005 * 200,
                         Ts=sample_time, want=("X", "U_out", "S_p"))
    X = r["X"][:, 0, :T]
    return (X[:, :, 0], X[:, :, 1], X[:, :, 2], r["S_p"][:, 0, :, 0], X[:, :, 3], r["U_out"][:, 0, :, 0],
            r["U_out"][:, 0, :, 1], time_sim_vec)
