"""Manufactured QPs with exact primal-dual solutions, off the OCP's data (a plain helper module).

Every other QP of the suite is the OCP's own Gauss-Newton QP (qp_data.py): A = I + O(Ts), B = O(Ts),
dx0 ~ 0, W_s = 0, bound offsets below 0.07 -- terms that are ~0 or ~1 there could be wrong unseen.
Here a batch of QPs that qsp_qp_solve accepts is built BACKWARDS from a drawn solution: draw the
dynamics, the primal point, the dynamics multipliers and an active set, then derive b, the bounds
and the gradient g so that the drawn point satisfies the KKT conditions exactly (to rounding).  With
positive H it is the unique minimiser; with LICQ (below) its multipliers are unique too.

What the C ABI requires (include/qsp_nmpc.h, qsp_qp_solve): A the identity except a02, a03, a12, a13,
a23, a33; a diagonal stage Hessian equal on every stage and lane; a terminal Hessian equal on every
lane; bound widths equal on every stage.  Every bound is present (the kernels have no inactive
bound rows); "free" below means strictly inside.

Sign conventions (oracle/qsp_oracle.c, the adjoint recursion of qp_solve; tests/test_oracle.py::
test_qp_kkt), v_k = [dx_k[3], du_k] the bounded components, lam_k = (s lo, s hi, u_n lo, u_n hi, u_t lo, u_t hi):
    inputs              H_u du_k + g_u + B_k' pi_k - lam_lo + lam_hi = 0
    states, 0 < k < N   H_x dx_k + g_x + A_k' pi_k - pi_{k-1} + e_s (lam_hi - lam_lo) = 0
    terminal            We dx_N + g_N - pi_{N-1} = 0
    dynamics            dx_{k+1} = A_k dx_k + B_k du_k + b_k,  dx_0 = dx0
Each lane draws from numpy.random.default_rng([seed, lane]), so a batch of 64 is the first 64 lanes
of the batch of 70 with the same seed.
"""
import numpy as np

# (p_s, p_un, p_ut): the probability that a bounded component sits at a bound (half lower, half upper)
FAMILIES = {"F0": (0.0, 0.0, 0.0), "Fu": (0.0, 0.3, 0.3), "Fs": (0.3, 0.0, 0.0), "Fall": (0.3, 0.3, 0.3)}

GENERIC = dict(W=(2.0, 0.5, 1e-2, 0.3, 0.3, 0.7), We=(3.0, 1.0, 0.5, 0.2), width=(1.5, 2.0, 1.0),
               sc_A=0.2, sc_B=0.5, lam_range=(0.1, 5.0))
# the OCP's zero pattern: no cost on s, so its only curvature is the barrier's
OCP_PATTERN = dict(GENERIC, W=(2.0, 0.5, 1e-2, 0.0, 0.3, 0.7), We=(3.0, 1.0, 0.5, 0.0))
SMALL_LAM = (1e-3, 1e-2)   # the multiplier range of the "Fs-small" family


def make_batch(family, N, nb, seed, W=GENERIC["W"], We=GENERIC["We"], width=GENERIC["width"], sc_A=GENERIC["sc_A"],
               sc_B=GENERIC["sc_B"], lam_range=GENERIC["lam_range"], sc_z=1.0, stage0_infeasible=False):
    """One batch: dict with the QP (A, B, b, H, g, lo, hi, act, dx0, in Oracle.qp's layout) and its
    exact solution (dx, du, pi, lam) plus state (N x 3: 0 free, 1 at lower, 2 at upper).
    sc_z scales the drawn dx*, du* (1: the construction above; the accuracy study varies it with the
    widths to move the bound offsets).  stage0_infeasible: the stage-0 s bounds are moved so that dx0's
    s lies 0.1 below them (a QP that is infeasible where the stage-0 s bound is enforced, and the same
    QP where it is not: that bound is no row of the problem then)."""
    p = FAMILIES[family] if isinstance(family, str) else tuple(family)
    W, We, width = np.asarray(W, float), np.asarray(We, float), np.asarray(width, float)
    q = dict(A=np.zeros((nb, N, 4, 4)), B=np.zeros((nb, N, 4, 2)), b=np.zeros((nb, N, 4)),
             H=np.zeros((nb, 6 * N + 4)), g=np.zeros((nb, 6 * N + 4)), lo=np.zeros((nb, N, 3)),
             hi=np.zeros((nb, N, 3)), act=np.ones((nb, N, 3), np.uint8), dx0=np.zeros((nb, 4)),
             dx=np.zeros((nb, N + 1, 4)), du=np.zeros((nb, N, 2)), pi=np.zeros((nb, N, 4)),
             lam=np.zeros((nb, N, 6)), state=np.zeros((nb, N, 3), np.int8))
    q["H"][:, :6 * N] = np.tile(W, N)
    q["H"][:, 6 * N:] = We
    for l in range(nb):
        rng = np.random.default_rng([seed, l])
        A = np.tile(np.eye(4), (N, 1, 1))
        for i, j in ((0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            A[:, i, j] = sc_A * rng.uniform(-1, 1, N)
        A[:, 3, 3] = rng.uniform(0.9, 1.1, N)
        B = sc_B * rng.uniform(-1, 1, (N, 4, 2))
        dx, du, pi = sc_z * rng.uniform(-1, 1, (N + 1, 4)), sc_z * rng.uniform(-1, 1, (N, 2)), rng.uniform(-1, 1, (N, 4))
        b = dx[1:] - np.einsum("kij,kj->ki", A, dx[:-1]) - np.einsum("kij,kj->ki", B, du)
        v = np.concatenate([dx[:N, 3:4], du], 1)
        # active set: the stage-0 s is fixed by dx0 (always free); s_k may sit at a bound only if an
        # input of stage k-1 is free (LICQ: the active-s rows are triangular in those inputs)
        draw, side = rng.uniform(0, 1, (N, 3)), rng.integers(1, 3, (N, 3))
        state = np.where(draw < np.asarray(p), side, 0)
        state[0, 0] = 0
        for k in range(1, N):
            if state[k, 0] and state[k - 1, 1] and state[k - 1, 2]:
                state[k, 0] = 0
        frac = rng.uniform(0.2, 0.8, (N, 3))
        lo = np.where(state == 1, v, np.where(state == 2, v - width, v - frac * width))
        hi = lo + width
        mult = np.exp(rng.uniform(np.log(lam_range[0]), np.log(lam_range[1]), (N, 3)))
        lam = np.zeros((N, 3, 2))
        lam[:, :, 0] = np.where(state == 1, mult, 0.0)
        lam[:, :, 1] = np.where(state == 2, mult, 0.0)
        dl = lam[:, :, 1] - lam[:, :, 0]    # lam_hi - lam_lo
        g = np.zeros(6 * N + 4)
        gk = g[:6 * N].reshape(N, 6)
        gk[:, 4:] = -(W[4:] * du + np.einsum("kji,kj->ki", B, pi) + dl[:, 1:])
        gx = -(W[:4] * dx[:N] + np.einsum("kji,kj->ki", A, pi))
        gx[1:] += pi[:-1]
        gx[:, 3] -= dl[:, 0]
        gx[0] = rng.uniform(-1, 1, 4)   # dx_0 is fixed: its gradient is free data
        gk[:, :4] = gx
        g[6 * N:] = pi[N - 1] - We * dx[N]
        if stage0_infeasible:
            lo[0, 0] = dx[0, 3] + 0.1
            hi[0, 0] = lo[0, 0] + width[0]
        for name, val in (("A", A), ("B", B), ("b", b), ("g", g), ("lo", lo), ("hi", hi), ("dx0", dx[0]), ("dx", dx),
                          ("du", du), ("pi", pi), ("lam", lam.reshape(N, 6)), ("state", state)):
            q[name][l] = val
    return q


def qp_args(q, stage0_s_bound=0):
    """The positional arguments of Oracle.qp / Oracle.qp_ext after opts."""
    nb, N = q["b"].shape[:2]
    act = q["act"].copy()
    act[:, 0, 0] = 1 if stage0_s_bound else 0
    return (q["A"].reshape(nb, N, 16), q["B"].reshape(nb, N, 8), q["b"], q["H"], q["g"], q["lo"], q["hi"], act, q["dx0"])


def kkt_residuals(q, dx, du, pi, lam):
    """Largest absolute KKT residuals of a point, per lane: dict of (nb,) arrays -- stat_u, stat_x
    (stages 1..N-1 and the terminal one), dyn (dynamics and dx_0 = dx0), infeas (bound violation,
    stage-0 s excluded), comp (lam * slack), dual (negative multipliers)."""
    nb, N = q["b"].shape[:2]
    H, g = q["H"][:, :6 * N].reshape(nb, N, 6), q["g"][:, :6 * N].reshape(nb, N, 6)
    lam = lam.reshape(nb, N, 3, 2)
    dl = lam[..., 1] - lam[..., 0]
    ru = H[..., 4:] * du + g[..., 4:] + np.einsum("lkji,lkj->lki", q["B"], pi) + dl[..., 1:]
    rx = H[..., :4] * dx[:, :N] + g[..., :4] + np.einsum("lkji,lkj->lki", q["A"], pi)
    rx[:, 1:] -= pi[:, :-1]
    rx[..., 3] += dl[..., 0]
    rN = q["H"][:, 6 * N:] * dx[:, N] + q["g"][:, 6 * N:] - pi[:, N - 1]
    dyn = dx[:, 1:] - np.einsum("lkij,lkj->lki", q["A"], dx[:, :N]) - np.einsum("lkij,lkj->lki", q["B"], du) - q["b"]
    v = np.concatenate([dx[:, :N, 3:4], du], 2)
    t = np.stack([v - q["lo"], q["hi"] - v], 3)
    t[:, 0, 0] = 1.0   # the stage-0 s is no variable
    mx = lambda a: np.abs(a).reshape(nb, -1).max(1)
    return dict(stat_u=mx(ru), stat_x=np.maximum(mx(rx[:, 1:]) if N > 1 else 0.0, mx(rN)),
                dyn=np.maximum(mx(dyn), mx(dx[:, 0] - q["dx0"])), infeas=mx(np.minimum(t, 0.0)),
                comp=mx(lam * t), dual=mx(np.minimum(lam, 0.0)))


def objective(q, dx, du):
    """0.5 z'Hz + g'z per lane."""
    nb, N = q["b"].shape[:2]
    z = np.concatenate([np.concatenate([dx[:, :N], du], 2).reshape(nb, 6 * N), dx[:, N]], 1)
    return (0.5 * q["H"] * z * z + q["g"] * z).sum(1)


# ------------------------------------------------------------------ the batches the tests share
# (N, stages per lane, factor_scan): every factorisation walk of tests/test_twin.py::test_factor_walk_table
# at both edges of its range -- lane walk N = 3, 11 and matrix cores N = 12, 20, 31 at one stage per
# lane; matrix cores, and the associative scan, N = 24, 32, 50 at two
CONFIGS = [(3, 1, 0), (11, 1, 0), (12, 1, 0), (20, 1, 0), (31, 1, 0),
           (24, 2, 0), (32, 2, 0), (50, 2, 0), (24, 2, 1), (32, 2, 1), (50, 2, 1)]
NAMED = {"F0": ("F0", {}), "Fu": ("Fu", {}), "Fs": ("Fs", {}), "Fall": ("Fall", {}),
         "Fs-small": ("Fs", dict(lam_range=SMALL_LAM)),
         "F0-ocp": ("F0", dict(W=OCP_PATTERN["W"], We=OCP_PATTERN["We"])),
         "Fu-ocp": ("Fu", dict(W=OCP_PATTERN["W"], We=OCP_PATTERN["We"]))}
# The infeasible-start IPM jams on some lanes (it stops at the cap or the stall exit, far from the
# solution, and says so: status 2 / 4): ~5 % of a batch, ~15 % at N = 3.  The seeds are chosen so that
# the LITERAL oracle alone meets the stop test on >= 85 % of the lanes of F0, Fu, Fs-small and Fu-ocp
# (64 and 70 lanes): seed 1 does at every N but 3; at N = 3, 14 is the first of 1..29 with 90 %.
SEEDS = {3: 14}
QP_ITERS, MU_STOP, MIN_CONVERGED = 50, 1e-10, 0.85


def named_batch(name, N, nb, **kw):
    fam, args = NAMED[name]
    return make_batch(fam, N, nb, SEEDS.get(N, 1), **dict(args, **kw))


def worst_errors(r, q, keys=("dx", "du", "pi", "lam")):
    """max |r - exact| over the lanes that met the stop test (qp_status 0), per quantity."""
    m = r["qp_status"] == 0
    return {k: float(np.abs(r[k][m] - q[k][m]).max()) if m.any() else np.inf for k in keys}


def inactive_multiplier_excess(r, q):
    """Largest lam * slack / (m mu_stop) over the inactive bounds of the status-0 lanes, m = 6N the number
    of bound rows: the stop test leaves mean(lam t) < mu_stop, so every product is below m mu_stop and an
    inactive multiplier below (m mu_stop) / slack -- a value above 1 breaks what the stop test promises.
    The slack is the exact solution's (>= 0.2 of the width), the stage-0 s (no variable) left out."""
    nb, N = q["b"].shape[:2]
    m = r["qp_status"] == 0
    v = np.concatenate([q["dx"][:, :N, 3:4], q["du"]], 2)
    t = np.stack([v - q["lo"], q["hi"] - v], 3)
    side = np.stack([q["state"] != 1, q["state"] != 2], 3)    # the bound rows that are not active
    side[:, 0, 0] = False
    return float((np.where(side, r["lam"].reshape(nb, N, 3, 2) * t, 0.0)[m] / (6 * N * MU_STOP)).max()) if m.any() else 0.0


def path_differences(r, ref):
    """Lanes on which two solvers of the same algorithm took different paths: another status, or (both at
    status 0) another iteration count.  Restatements that differ in association order alone part only
    where a stop test or a step length is decided at rounding level -- measured 0 of 64 on F0, Fu and
    Fu-ocp at every N, one lane on other seeds -- while a wrong term of the predictor-corrector step that
    leaves the fixed point alone (the exact-solution checks cannot see it) showed on 5 .. 13 of 64."""
    both = (r["qp_status"] == 0) & (ref["qp_status"] == 0)
    return int(np.sum(r["qp_status"] != ref["qp_status"]) + np.sum(r["iters"][both] != ref["iters"][both]))


MAX_PATH_DIFFERENCES = 2
