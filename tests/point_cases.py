"""What the GPU tests of the evaluators beside the solve path share (tests/test_gpu_kkt.py, tests/test_gpu_sens.py;
a plain helper module, no tests): bit comparison, a solver with mixed shapes, and the seeded NLP points."""
import numpy as np

from conftest import config2_x0, straight_traj


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_solver(N, B, names, sid, **kw):
    """An OcpSolver of (N, B) with the shapes `names`, lane i on shape sid[i]."""
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver(N=N, batch=B, **kw)
    s.set_shapes([make_shape(n) for n in names], shape_id=sid)
    return s, sid


def cold_solve(s, seed):
    """solve() from the cold start (X = x0 repeated, U = 0) at the config-2 x0 of `seed`, the straight reference."""
    x0, yref = config2_x0(s.B, seed), np.repeat(straight_traj()[None, :s.N], s.B, 0)
    for name, v in (("constr_x0", x0), ("cost_y_ref", yref), ("cost_y_ref_e", yref[:, s.N - 1, :4].copy()),
                    ("init_x", np.repeat(x0[:, None], s.N + 1, 1)), ("init_u", np.zeros((s.B, s.N, 2)))):
        s.set(name, v)
    s.solve()


def nlp_point(s, sid, seed, feasible):
    """A seeded point: U uniform inside the input bounds, X an Euler rollout from the config-2 x0 law, the straight
    reference.  feasible = False (KKT tests), no solution: 1e-3 noise on X (defects, and the s bound on both
    sides), PI in +-1e3, LAM in [0, 1].  feasible = True (sensitivity tests): s clipped into its bounds, a few inputs
    on or within 1e-12 of a bound (slack below t_floor), PI in +-1, LAM zero on about two thirds of the sides."""
    B, N = s.B, s.N
    rng = np.random.default_rng(seed)
    x0 = config2_x0(B, seed)
    U = rng.uniform(s._lh[1:], s._uh[1:], (B, N, 2))
    if feasible:
        U[:, :, 1][rng.uniform(0, 1, (B, N)) < 0.05] = s._uh[2]           # on u_t's upper bound
        U[:, :, 0][rng.uniform(0, 1, (B, N)) < 0.05] = s._lh[1] + 1e-12   # within 1e-12 of u_n's lower bound
    X = np.zeros((B, N + 1, 4))
    X[:, 0] = x0
    for k in range(N):
        X[:, k + 1] = X[:, k] + s.Ts * s.eval_dynamics(X[:, k], U[:, k], shape_id=sid)[0]
        if feasible:
            X[:, k + 1, 3] = np.clip(X[:, k + 1, 3], s._lh[0], s._uh[0])
    if feasible:
        PI = rng.uniform(-1.0, 1.0, (B, N, 4))
        LAM = np.where(rng.uniform(0, 1, (B, N, 6)) < 0.35, rng.uniform(0.0, 1.0, (B, N, 6)), 0.0)
    else:
        X += 1e-3 * rng.uniform(-1, 1, X.shape)
        PI = rng.uniform(-1e3, 1e3, (B, N, 4))
        LAM = rng.uniform(0.0, 1.0, (B, N, 6))
    yref = np.repeat(straight_traj()[None, :N], B, 0)
    return dict(x0=x0, X=X, U=U, PI=PI, LAM=LAM, yref=yref, yref_e=yref[:, N - 1, :4].copy())
