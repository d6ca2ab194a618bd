"""numpy restatement of the KKT evaluators (csrc/qsp_kkt.hpp; a plain helper module): the residuals of a QP
point (qsp_qp_residuals) and of an NLP iterate (qsp_eval_kkt), with the implied-multiplier rule.

Beside every residual stands its TERM SCALE: the sum of the absolute values of the terms that were added to
form it.  A residual is a sum of at most a dozen products; the library is compiled with -ffp-contract=off
and every fused multiply-add is explicit, so it and numpy differ by association and by the fma's missing
rounding only: each of at most ~14 roundings is below eps times a partial sum, which the term scale bounds.
Hence the comparison the tests use, derived and not measured:

    |got - ref| <= BOUND * term_scale,   BOUND = 64 eps,  eps = 2^-52.

A per-lane maximum obeys the same bound with the largest term scale of its entries, since
|max_i a_i - max_i b_i| <= max_i |a_i - b_i|.
"""
import numpy as np

EPS = 2.0 ** -52
BOUND = 64 * EPS
QP_KEYS = ("stat_u", "stat_x", "dyn", "infeas", "comp", "dual")
PARTS = ("stat_u", "stat_x", "stat_term", "eq_dyn", "eq_x0", "ineq", "comp")


def _mx(a):
    return a.reshape(a.shape[0], -1).max(1) if a.size else np.zeros(a.shape[0])


def worst_ratio(got, ref, scale):
    """max |got - ref| / (BOUND * scale) over the entries (0 / 0 counts as 0; anything / 0 as inf)."""
    err, tol = np.abs(np.asarray(got) - ref), BOUND * np.asarray(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(np.max(r)) if r.size else 0.0


def qp_residuals(q, dx, du, pi, lam, stage0_s_bound):
    """(res, scale): dicts keyed QP_KEYS of (nb,) arrays for the point (dx, du, pi, lam) of the QP batch q
    (tests/manufactured_qp.py's layout and sign conventions)."""
    nb, N = q["b"].shape[:2]
    A, B = q["A"].reshape(nb, N, 4, 4), q["B"].reshape(nb, N, 4, 2)
    H, g = q["H"][:, :6 * N].reshape(nb, N, 6), q["g"][:, :6 * N].reshape(nb, N, 6)
    HN, gN = q["H"][:, 6 * N:], q["g"][:, 6 * N:]
    lam = lam.reshape(nb, N, 3, 2)
    ab = np.abs
    # inputs
    tB = B * pi[..., :, None]                                     # B[j, i] pi[j]
    ru = H[..., 4:] * du + g[..., 4:] + tB.sum(2) + (lam[:, :, 1:, 1] - lam[:, :, 1:, 0])
    su = ab(H[..., 4:] * du) + ab(g[..., 4:]) + ab(tB).sum(2) + ab(lam[:, :, 1:, 1]) + ab(lam[:, :, 1:, 0])
    # states 1..N-1, terminal
    tA = A * pi[..., :, None]                                     # A[j, i] pi[j]
    rx = H[..., :4] * dx[:, :N] + g[..., :4] + tA.sum(2)
    sx = ab(H[..., :4] * dx[:, :N]) + ab(g[..., :4]) + ab(tA).sum(2)
    rx[:, 1:] -= pi[:, :-1]
    sx[:, 1:] += ab(pi[:, :-1])
    rx[..., 3] += lam[:, :, 0, 1] - lam[:, :, 0, 0]
    sx[..., 3] += ab(lam[:, :, 0, 1]) + ab(lam[:, :, 0, 0])
    rN = HN * dx[:, N] + gN - pi[:, N - 1]
    sN = ab(HN * dx[:, N]) + ab(gN) + ab(pi[:, N - 1])
    # dynamics, dx_0 = dx0
    tAx, tBu = A * dx[:, :N, None, :], B * du[:, :, None, :]
    rd = dx[:, 1:] - tAx.sum(3) - tBu.sum(3) - q["b"]
    sd = ab(dx[:, 1:]) + ab(tAx).sum(3) + ab(tBu).sum(3) + ab(q["b"])
    r0, s0 = dx[:, 0] - q["dx0"], ab(dx[:, 0]) + ab(q["dx0"])
    # bounds
    v = np.concatenate([dx[:, :N, 3:4], du], 2)
    t = np.stack([v - q["lo"], q["hi"] - v], 3)
    st = np.stack([ab(v) + ab(q["lo"]), ab(q["hi"]) + ab(v)], 3)
    on = np.ones((nb, N, 3, 2), bool)
    if not stage0_s_bound:
        on[:, 0, 0] = False
    z = lambda a: np.where(on, a, 0.0)
    res = dict(stat_u=_mx(ab(ru)), stat_x=np.maximum(_mx(ab(rx[:, 1:])), _mx(ab(rN))),
               dyn=np.maximum(_mx(ab(rd)), _mx(ab(r0))), infeas=_mx(z(np.maximum(-t, 0.0))),
               comp=_mx(z(ab(lam * t))), dual=_mx(z(np.maximum(-lam, 0.0))))
    scale = dict(stat_u=_mx(su), stat_x=np.maximum(_mx(sx[:, 1:]), _mx(sN)), dyn=np.maximum(_mx(sd), _mx(s0)),
                 infeas=_mx(z(st)), comp=_mx(z(ab(lam) * st)), dual=_mx(z(ab(lam))))
    return res, scale


def lam_of_stationarity(r):
    """The implied-multiplier rule (implied_lam, csrc/qsp_point.hpp), the one statement of it in the tests: r
    (nb, N, 3) the stationarity of (s, u_n, u_t) at stages k < N without bound multipliers -> lam (nb, N, 3, 2) with
    lam_lo = r where r > 0, lam_hi = -r where r < 0, else 0, and the stage-0 s pair 0.  Exact: the bits of lam are
    those of r, so a caller that forms r as the kernel does (tests/sens_ref.py::implied_lam) gets the kernel's."""
    lam = np.stack([np.where(r > 0.0, r, 0.0), np.where(r < 0.0, -r, 0.0)], 3)
    lam[:, 0, 0] = 0.0
    return lam


def nlp_residuals(X, U, PI, LAM, yref, yref_e, xn, A, B, tau, W, We, lh, uh, stage0_s_bound, x0=None):
    """The NLP iterate's residuals from its stage data xn, A, B = one RK4 step with sensitivities at
    (X[:, :N], U) (nb x N x 4, x 4 x 4, x 4 x 2).  LAM None: the implied multipliers.  Returns a dict:
    stage_parts (nb, N + 1, 7: columns PARTS), stage_res (nb, N + 1, 4), parts (nb, 7), res (nb, 4), each
    with its term scale under '<name>_scale'; with LAM None also comp_extra (stage, lane: what the implied
    multipliers' own rounding adds to comp's tolerance, already times BOUND) and lam (nb, N, 6)."""
    nb, N = U.shape[:2]
    ab = np.abs
    W, We, lh, uh = (np.asarray(a, float) for a in (W, We, lh, uh))
    gx = tau * W[:4] * (X[:, :N] - yref[..., :4])
    gu = tau * W[4:] * (U - yref[..., 4:])
    gN = We * (X[:, N] - yref_e)
    tB, tA = B * PI[..., :, None], A * PI[..., :, None]
    ru0, su0 = gu + tB.sum(2), ab(gu) + ab(tB).sum(2)              # without bound multipliers
    rx0, sx0 = gx + tA.sum(2), ab(gx) + ab(tA).sum(2)
    rx0[:, 1:] -= PI[:, :-1]
    sx0[:, 1:] += ab(PI[:, :-1])
    extra = None
    if LAM is None:
        r = np.concatenate([rx0[..., 3:4], ru0], 2)               # (s, u_n, u_t)
        sr = np.concatenate([sx0[..., 3:4], su0], 2)
        lam = lam_of_stationarity(r)
        lam_err = BOUND * np.repeat(sr[..., None], 2, 3)
        lam_err[:, 0, 0] = 0.0
    else:
        lam = LAM.reshape(nb, N, 3, 2)
        lam_err = np.zeros((nb, N, 3, 2))
    ru = ru0 + (lam[:, :, 1:, 1] - lam[:, :, 1:, 0])
    su = su0 + ab(lam[:, :, 1:, 1]) + ab(lam[:, :, 1:, 0])
    rx, sx = rx0.copy(), sx0.copy()
    rx[..., 3] += lam[:, :, 0, 1] - lam[:, :, 0, 0]
    sx[..., 3] += ab(lam[:, :, 0, 1]) + ab(lam[:, :, 0, 0])
    rN, sN = gN - PI[:, N - 1], ab(gN) + ab(PI[:, N - 1])
    rd, sd = xn - X[:, 1:], ab(xn) + ab(X[:, 1:])
    v = np.concatenate([X[:, :N, 3:4], U], 2)
    t = np.stack([v - lh, uh - v], 3)
    st = np.stack([ab(v) + ab(lh), ab(uh) + ab(v)], 3)
    on = np.ones((nb, N, 3, 2), bool)
    if not stage0_s_bound:
        on[:, 0, 0] = False
    z = lambda a: np.where(on, a, 0.0).reshape(nb, N, 6).max(2)
    P, S = np.zeros((nb, N + 1, 7)), np.zeros((nb, N + 1, 7))
    P[:, :N, 0], S[:, :N, 0] = ab(ru).max(2), su.max(2)
    P[:, 1:N, 1], S[:, 1:N, 1] = ab(rx[:, 1:]).max(2), sx[:, 1:].max(2)
    P[:, N, 2], S[:, N, 2] = ab(rN).max(1), sN.max(1)
    P[:, :N, 3], S[:, :N, 3] = ab(rd).max(2), sd.max(2)
    if x0 is not None:
        P[:, 0, 4], S[:, 0, 4] = ab(x0 - X[:, 0]).max(1), (ab(x0) + ab(X[:, 0])).max(1)
    P[:, :N, 5], S[:, :N, 5] = z(np.maximum(-t, 0.0)), z(st)
    P[:, :N, 6], S[:, :N, 6] = z(ab(lam * t)), z(ab(lam) * st)
    extra = np.zeros((nb, N + 1))
    extra[:, :N] = z(lam_err * ab(t))

    def four(M):
        return np.stack([M[..., :3].max(-1), M[..., 3:5].max(-1), M[..., 5], M[..., 6]], -1)
    out = dict(stage_parts=P, stage_parts_scale=S, stage_res=four(P), stage_res_scale=four(S),
               parts=P.max(1), parts_scale=S.max(1), res=four(P.max(1)), res_scale=four(S.max(1)),
               comp_extra=extra, lam=lam.reshape(nb, N, 6))
    return out
