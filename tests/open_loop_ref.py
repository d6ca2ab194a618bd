"""numpy restatement of the contact-mode rule and of helper.open_loop_matlab (TEST INFRASTRUCTURE ONLY).

`helper.open_loop_matlab` (helper.m:132-193) step by step over the CPU oracle's f and spline
(`Oracle.dynamics`, `Oracle.spline`; literal restatement or kernel-order twin), and the motion cone from
the oracle's C and C' by PusherSliderModel.m:532-548, in plain numpy.  numpy has no fused multiply-add,
so against the device this is a tolerance comparison, never bit identity; a mode is compared only where
its margin to the cone's edges is not at rounding level.
"""
import numpy as np

TS = 0.05
NOISE_STD = np.array([1e-5, 1e-5, 1e-3, 1e-4])          # helper.m:155
MODE_NONE, MODE_ST, MODE_SL, MODE_SR = 0, 1, 2, 3        # helper.m:17-23 (convert_str2num); 0: no indicator set


def _spline(oracle, s, sid):
    """C, C', tangent-angle rate at s (already wrapped) from either oracle formulation."""
    r = oracle.spline(s, sid)
    return r[0], (r[1] if oracle.twin else r[2]), r[-1]


def motion_cone(oracle, s, sid):
    """gamma_l, gamma_r at the contact point s (PusherSliderModel.m:526-548)."""
    s = np.asarray(s, np.float64).ravel()
    sid = np.broadcast_to(np.asarray(sid, np.int32), s.shape)
    b, c, mu = (oracle.tab["params"][sid, k] for k in range(3))
    sig = np.fmod(s, b) + (s < 0) * b                                       # :526
    Cv, D, _ = _spline(oracle, sig, sid)
    t = D / np.sqrt(D[:, 0] ** 2 + D[:, 1] ** 2)[:, None]                   # bspline_shape.m:108-111
    n = np.stack([t[:, 1], -t[:, 0]], 1)
    px = n[:, 0] * Cv[:, 0] + n[:, 1] * Cv[:, 1]                            # :532-534
    py = t[:, 0] * Cv[:, 0] + t[:, 1] * Cv[:, 1]
    gl = (mu * c ** 2 - px * py + mu * px ** 2) / (c ** 2 + py ** 2 - mu * px * py)     # :547
    gr = (-mu * c ** 2 - px * py - mu * px ** 2) / (c ** 2 + py ** 2 + mu * px * py)    # :548
    return gl, gr


def mode_rule(gl, gr, rho):
    """The OCP model's indicators (PusherSliderModel.m:587-589) as a mode; 0 where none is set (NaN)."""
    with np.errstate(invalid="ignore"):
        st = (rho >= gr) & (rho <= gl)
        return np.where(st, MODE_ST, np.where(rho > gl, MODE_SL, np.where(rho < gr, MODE_SR, MODE_NONE))).astype(np.int32)


def mode_margin(gl, gr, rho):
    """min(|rho - gl| / (1 + |gl|), |rho - gr| / (1 + |gr|)): how far the label is from changing.  Infinite
    where rho is (u_n = 0); NaN where rho is NaN (mode 0: compared always)."""
    with np.errstate(invalid="ignore"):
        return np.minimum(np.abs(rho - gl) / (1 + np.abs(gl)), np.abs(rho - gr) / (1 + np.abs(gr)))


def modes(oracle, x, u, sid):
    """x (n, 4), u (n, 2) -> mode (n,), cone (n, 3) = gamma_l, gamma_r, rho, margin (n,)."""
    x = np.asarray(x, np.float64).reshape(-1, 4)
    u = np.asarray(u, np.float64).reshape(-1, 2)
    gl, gr = motion_cone(oracle, x[:, 3], sid)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = u[:, 1] / u[:, 0]
    return mode_rule(gl, gr, rho), np.stack([gl, gr, rho], 1), mode_margin(gl, gr, rho)


def modes_from_jacobian(J, gl, gr):
    """The mode read off d f / d(x, u) (n, 4, 6): J[3, 5] = i_sl + i_sr in {0, 1}; when sliding -J[3, 4] is the
    active gamma: the edge (gl or gr, from motion_cone) it lies nearer to names the mode.  -> mode, -J[3, 4]."""
    slide = J[:, 3, 5] == 1.0
    assert np.all(slide | (J[:, 3, 5] == 0.0))
    g = -J[:, 3, 4]
    left = np.abs(g - gl) < np.abs(g - gr)
    return np.where(~slide, MODE_ST, np.where(left, MODE_SL, MODE_SR)).astype(np.int32), g


def applied_inputs(U, D):
    """(..., T, 2) commanded -> applied with a delay buffer of D zero columns (helper.m:148,174-176)."""
    out = np.zeros_like(U)
    T = U.shape[-2]
    out[..., D:, :] = U[..., :max(T - D, 0), :]
    return out if D > 0 else U.copy()


def open_loop(oracle, x0, U, sid, T, noise=None, D=0, clip=True, v_alpha=1.0, Ts=TS):
    """x0 (B, 4), U (B, M, 2) or (B, M, T, 2), sid (B,), noise (T, B, 4) or None, D delay columns ->
    dict X (B, M, T+1, 4), U_out (B, M, T, 2), S_p (B, M, T, 2), mode (B, M, T), margin (B, M, T),
    mode_steps (B, M, 4), x_end (B, M, 4)."""
    U = np.asarray(U, np.float64)
    B, M = U.shape[:2]
    n = B * M
    Ur = (np.repeat(U[:, :, None], T, 2) if U.ndim == 3 else U).reshape(n, T, 2)
    x = np.repeat(np.asarray(x0, np.float64)[:, None], M, 1).reshape(n, 4)
    sidf = np.repeat(np.asarray(sid, np.int32), M)
    b = oracle.tab["params"][sidf, 0]
    X = np.zeros((n, T + 1, 4))
    Uo = np.zeros((n, T, 2))
    Sp = np.zeros((n, T, 2))
    mode = np.zeros((n, T), np.int32)
    margin = np.zeros((n, T))
    buf = np.zeros((n, max(D, 1), 2))                                       # u_buff_plant, column 0 newest (:148)
    for i in range(T):
        if noise is not None:
            x = x + np.repeat(noise[i][:, None], M, 1).reshape(n, 4)        # :155
        X[:, i] = x
        u = Ur[:, i].copy()
        sm = np.mod(x[:, 3], b)                                             # MATLAB mod (bspline_shape.m:147,193)
        Cv, _, kap = _spline(oracle, sm, sidf)
        if clip:
            with np.errstate(divide="ignore"):
                v = v_alpha / np.abs(kap)                                   # :162-164
            u[:, 1] = np.where(v < u[:, 1], v, u[:, 1])                     # MATLAB min(v, u_t)
        Uo[:, i] = u
        Sp[:, i] = Cv                                                       # :187
        if D == 0:
            ua = u
        else:                                                               # :174-176
            ua = buf[:, -1].copy()
            buf = np.concatenate([u[:, None], buf[:, :-1]], 1)
        mode[:, i], _, margin[:, i] = modes(oracle, x, ua, sidf)
        x = x + Ts * oracle.dynamics(x, ua, sidf)[0]                        # :180
    X[:, T] = x
    steps = np.stack([(mode == k).sum(1) for k in range(4)], 1).astype(np.int32)
    return dict(X=X.reshape(B, M, T + 1, 4), U_out=Uo.reshape(B, M, T, 2), S_p=Sp.reshape(B, M, T, 2),
                mode=mode.reshape(B, M, T), margin=margin.reshape(B, M, T), mode_steps=steps.reshape(B, M, 4),
                x_end=x.reshape(B, M, 4))


def law_xu(n, seed, oracle):
    """The random (x, u) law of the mode tests: four shapes, s in [-b, 2b], u_n in [0.001, 0.03],
    u_t in +-0.05."""
    rng = np.random.default_rng(seed)
    sid = (np.arange(n) % 4).astype(np.int32)
    b = oracle.tab["params"][sid, 0]
    x = np.stack([rng.uniform(-0.01, 0.03, n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.2, 0.2, n),
                  rng.uniform(-1.0, 2.0, n) * b], 1)
    u = np.stack([rng.uniform(0.001, 0.03, n), rng.uniform(-0.05, 0.05, n)], 1)
    return x, u, sid


def law_open_loop(B, M, seed):
    """Inputs of the open-loop tests: u_n in [0, 0.03] with a few lanes at exactly 0 (main.m:207's own call),
    u_t in +-0.05 -> U (B, M, 2)."""
    rng = np.random.default_rng(seed)
    U = np.stack([rng.uniform(0.0, 0.03, (B, M)), rng.uniform(-0.05, 0.05, (B, M))], -1)
    U[::9, 0, 0] = 0.0
    return U


def draw_noise(T, B, seed):
    return np.random.default_rng(seed).standard_normal((T, B, 4)) * NOISE_STD
