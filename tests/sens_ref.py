"""numpy restatement of the solution sensitivities du_k/dx0 (csrc/qsp_sens.hpp) WITHOUT a Riccati recursion
(a plain helper module, no tests).

The equality-constrained QP of a lane, from stage k0 on,
    min  sum_{k0 <= k < N} 0.5 (dx_k' Hx_k dx_k + du_k' Hu_k du_k) + 0.5 dx_N' H_N dx_N
    s.t. dx_{k+1} = A_k dx_k + B_k du_k,  dx_k0 given,
is assembled as one dense KKT system in z = (du_k0, dx_k0+1, du_k0+1, ..., dx_N) and the dynamics multipliers,
    [ H  C' ] [ z   ]   [ 0 ]
    [ C  0  ] [ lam ] = [ E ],      E = (A_k0 dx_k0, 0, ...),
and solved for the four unit dx_k0 columns with numpy.linalg.solve.  dU_k are the du rows of z; the value
function's Hessian is the Schur complement P_k0 = Hx_k0 - E' lam (the optimal value is -0.5 E' lam); the
stage gain K_k is dU_k of the tail problem that starts at k0 = k.

Also here: the barrier diagonals that the host and GPU tests put into a manufactured batch's H (barrier_H),
the barrier diagonal of an NLP point as qsp_eval_sens forms it (nlp_H), and the scale of the tests' bound.
"""
import numpy as np

import kkt_ref

EPS = np.finfo(float).eps
SIDX = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]   # sidx, qsp_riccati.hpp


def pack_sym(P):
    return np.array([P[i, j] for i, j in SIDX])


def tail_solve(A, B, H, k0):
    """The dense solve of one lane from stage k0: A (N, 4, 4), B (N, 4, 2), H (6N + 4,).  Returns dU (N - k0, 2, 4)
    = d du_k / d dx_k0, P (4, 4), the numerators B_k0' lam (2, 4) of the first stage's inputs and the KKT
    matrix's 2-norm condition number."""
    N = A.shape[0]
    n = N - k0
    nz, nc = 6 * n, 4 * n
    M = np.zeros((nz + nc, nz + nc))
    E = np.zeros((nc, 4))
    for j in range(n):
        k = k0 + j
        u, x = 6 * j, 6 * j + 2
        M[u:u + 2, u:u + 2] = np.diag(H[6 * k + 4:6 * k + 6])
        M[x:x + 4, x:x + 4] = np.diag(H[6 * (k + 1):6 * (k + 1) + 4])   # stage k + 1's state rows; the terminal four at N
        r = nz + 4 * j
        M[r:r + 4, x:x + 4] = np.eye(4)
        M[r:r + 4, u:u + 2] = -B[k]
        if j == 0:
            E[:4] = A[k]
        else:
            M[r:r + 4, x - 6:x - 2] = -A[k]
    M[:nz, nz:] = M[nz:, :nz].T
    rhs = np.zeros((nz + nc, 4))
    rhs[nz:] = E
    sol = np.linalg.solve(M, rhs)
    dU = np.stack([sol[6 * j:6 * j + 2] for j in range(n)])
    lam = sol[nz:]
    P = np.diag(H[6 * k0:6 * k0 + 4]) - E.T @ lam
    return dU, 0.5 * (P + P.T), B[k0].T @ lam[:4], float(np.linalg.cond(M))


def sens(A, B, H):
    """Every output of qsp_qp_sens for a batch: A (nb, N, 4, 4) or (nb, N, 16), B (nb, N, 4, 2) or (nb, N, 8),
    H (nb, 6N + 4).  dict of K0 (nb, 2, 4), K, dU (nb, N, 2, 4), P0 (nb, 10), cond (nb,) the condition number of
    the whole-horizon KKT matrix, numer (nb, N, 2, 4) the numerators B_k' lam of the stage gains
    (the stationarity of du_k: K_k row i = numer_k row i / Hu_k[i])."""
    nb, N = B.shape[:2]
    A, B = A.reshape(nb, N, 4, 4), B.reshape(nb, N, 4, 2)
    out = dict(K0=np.zeros((nb, 2, 4)), K=np.zeros((nb, N, 2, 4)), dU=np.zeros((nb, N, 2, 4)), P0=np.zeros((nb, 10)),
               cond=np.zeros(nb), numer=np.zeros((nb, N, 2, 4)))
    for l in range(nb):
        dU, P, num, cond = tail_solve(A[l], B[l], H[l], 0)
        out["dU"][l], out["K0"][l], out["K"][l, 0], out["P0"][l], out["cond"][l], out["numer"][l, 0] = dU, dU[0], dU[0], pack_sym(P), cond, num
        for k in range(1, N):
            dUk, _, num, _ = tail_solve(A[l], B[l], H[l], k)
            out["K"][l, k], out["numer"][l, k] = dUk[0], num
    return out


def row_scale(ref, name):
    """The scale eps * |row| * cond of one output: |row| the largest entry of the reference's row (a gain's row of
    four; for P0 the largest entry of the lane's P0), cond the lane's condition number."""
    v = ref[name]
    nb = v.shape[0]
    rown = np.abs(v).max(-1, keepdims=True) if name != "P0" else np.abs(v).max(1, keepdims=True)
    cond = ref["cond"].reshape((nb,) + (1,) * (v.ndim - 1))
    return EPS * rown * cond * np.ones_like(v)


OUTPUTS = ("K0", "K", "dU", "P0")


def run_host_program(exe, path, A, B, H):
    """The host program's outputs for a batch: dict of K0, K, dU, P0 and flag, bit for bit as printed."""
    import subprocess
    nb, N = B.shape[:2]
    with open(path, "wb") as fh:
        fh.write(np.array([N, nb, 0, 0], np.int32).tobytes())
        for a in (A, B, H):
            fh.write(np.ascontiguousarray(a, np.float64).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[0] == "sens ok", r.stdout[:200]
    row = lambda ln: np.array([float.fromhex(v) for v in ln.split()])
    out = dict(flag=np.zeros(nb, np.int32), K0=np.zeros((nb, 2, 4)), P0=np.zeros((nb, 10)), K=np.zeros((nb, N, 2, 4)),
               dU=np.zeros((nb, N, 2, 4)))
    for l in range(nb):
        f, k0, p0, k, du = lines[1 + 5 * l:6 + 5 * l]
        out["flag"][l] = int(f)
        out["K0"][l], out["P0"][l] = row(k0).reshape(2, 4), row(p0)
        out["K"][l], out["dU"][l] = row(k).reshape(N, 2, 4), row(du).reshape(N, 2, 4)
    return out


def barrier_H(q, seed, s_pins=True):
    """H of a manufactured batch (tests/manufactured_qp.py) with a barrier diagonal of mixed size added: zero on
    most of the 3 N bounded components of a lane, 10^[2, 10] on a seeded tenth, and on the first lanes the
    cases that must be there -- lane 0: both inputs of stage 1 pinned (1e10, 1e8); lane 1: s pinned at stage 1
    (1e10) and at stage N - 1 (1e6); lane 2: one input of the last stage (1e9).  s_pins = False: the same
    draw with every s entry left at zero (input bounds only).  Returns H and the list of pinned inputs
    (lane, stage, input, d) with d >= 1e6."""
    nb, N = q["b"].shape[:2]
    H = q["H"].copy()
    d = np.zeros((nb, N, 3))
    for l in range(nb):
        rng = np.random.default_rng([seed, l, 77])
        hit = rng.uniform(0, 1, (N, 3)) < 0.1
        d[l] = np.where(hit, 10.0 ** rng.uniform(2, 10, (N, 3)), 0.0)
    if nb > 0:
        d[0, 1, 1], d[0, 1, 2] = 1e10, 1e8
    if nb > 1:
        d[1, 1, 0], d[1, N - 1, 0] = 1e10, 1e6
    if not s_pins:
        d[:, :, 0] = 0.0
    if nb > 2:
        d[2, N - 1, 2] = 1e9
    Hs = H[:, :6 * N].reshape(nb, N, 6)
    Hs[:, :, 3:] += d
    pins = [(l, k, i, d[l, k, 1 + i]) for l in range(nb) for k in range(N) for i in range(2) if d[l, k, 1 + i] >= 1e6]
    return H, pins


# The difference-quotient check of tests/test_gpu_sens.py and its CPU twin run (tests/test_sens_api.py): a batch
# with strict complementarity (input bounds only, multipliers in [0.1, 5]), the step of dx0, how many QPs may
# be left out for an active set that differs between the solves, and the twin's own worst
# |quotient - dense sensitivity| measured on the CPU (tests/test_sens_api.py re-measures it).
QUOT = dict(family="Fu", N=5, nb=16, seed=1, delta=1e-6, max_left_out=2, twin_err=7.1e-8)   # measured 7.030e-8 (literal restatement: 7.029e-8), all 16 kept


def quotient_check(solve, q, delta):
    """Central difference quotients of a QP solver's du in dx0 against the barrier data of its own answer.
    solve(dx0) -> dict with dx, du, lam, qp_status for the batch q at that dx0 (stage0_s_bound off).  Returns
    Q (nb, N, 2, 4) = (du(dx0 + delta e_j) - du(dx0 - delta e_j)) / (2 delta), H (nb, 6N + 4) = q's H plus
    d = lam / slack of the answer at delta = 0, and keep (nb,): status 0 in all nine solves and the same
    active set (a side is active when its multiplier exceeds its slack) in all of them."""
    nb, N = q["b"].shape[:2]

    def active(r):
        v = np.concatenate([r["dx"][:, :N, 3:4], r["du"]], 2)
        t = np.stack([v - q["lo"], q["hi"] - v], 3).reshape(nb, N, 6)
        a = r["lam"] > t
        a[:, 0, :2] = False          # the stage-0 s is no variable
        return a, t

    r0 = solve(q["dx0"])
    a0, t0 = active(r0)
    keep = r0["qp_status"] == 0
    Q = np.zeros((nb, N, 2, 4))
    for j in range(4):
        e = np.zeros(4)
        e[j] = delta
        rp, rm = solve(q["dx0"] + e), solve(q["dx0"] - e)
        for r in (rp, rm):
            keep &= (r["qp_status"] == 0) & (active(r)[0] == a0).all((1, 2))
        Q[..., j] = (rp["du"] - rm["du"]) / (2 * delta)
    d = r0["lam"] / t0
    d[:, 0, :2] = 0.0
    H = q["H"].copy()
    H[:, :6 * N].reshape(nb, N, 6)[:, :, 3:] += d[..., 0::2] + d[..., 1::2]
    return Q, H, keep


def fma(a, b, c):
    """a * b + c with one rounding (exact rational arithmetic, correctly rounded back), as qfma."""
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def implied_lam(X, U, PI, yref, A, B, W, tau):
    """The implied multipliers (B, N, 6) operation for operation as implied_lam (csrc/qsp_point.hpp) on the
    gradient sens_nlp_stage hands it, so that they are the bits the kernel forms: A (nb, N, 4, 4), B (nb, N, 4, 2)
    as qsp_eval_rk4 returns them.  The rule itself is kkt_ref.lam_of_stationarity."""
    nb, N = U.shape[:2]
    r = np.zeros((nb, N, 3))                      # the stationarity of (s, u_n, u_t) without bound multipliers
    chain = lambda c, p: fma(c[3], p[3], fma(c[2], p[2], fma(c[1], p[1], c[0] * p[0])))
    for l in range(nb):
        for k in range(N):
            pk = PI[l, k]
            for i in range(2):
                gu = tau * W[4 + i] * (U[l, k, i] - yref[l, k, 4 + i])
                r[l, k, 1 + i] = gu + chain(B[l, k, :, i], pk)
            if k >= 1:
                gs = tau * W[3] * (X[l, k, 3] - yref[l, k, 3])
                r[l, k, 0] = gs - PI[l, k - 1, 3] + chain(A[l, k, :, 3], pk)
    return kkt_ref.lam_of_stationarity(r).reshape(nb, N, 6)


def nlp_H(X, U, LAM, W, We, tau, lh, uh, s0_bound, t_floor):
    """The diagonal Hessian of qsp_eval_sens at (X, U) with multipliers LAM (B, N, 6), operation for operation as
    sens_barrier / sens_nlp_stage: d = lam_lo / max(v - lh, t_floor) + lam_hi / max(uh - v, t_floor), H = tau W + d;
    (B, 6N + 4) in qsp_qp_sens' layout."""
    nb, N = U.shape[:2]
    v = np.concatenate([X[:, :N, 3:4], U], 2)
    d = LAM[..., 0::2] / np.maximum(v - lh, t_floor) + LAM[..., 1::2] / np.maximum(uh - v, t_floor)
    if not s0_bound:
        d[:, 0, 0] = 0.0
    H = np.zeros((nb, 6 * N + 4))
    Hs = H[:, :6 * N].reshape(nb, N, 6)
    Hs[:] = tau * np.asarray(W)
    Hs[:, :, 3:] = (tau * np.asarray(W)[3:]) + d
    H[:, 6 * N:] = We
    return H
